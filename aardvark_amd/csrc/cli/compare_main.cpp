/*
 * compare_main.cpp — `aardvark_amd_compare`: the reference's `aardvark compare` flow (src/main.rs:30-327) on top of the
 * two C-ABIs: libaardvark_feeder.so turns FASTA + BED + truth/query VCFs into region batches, libaardvark_amd.so
 * solves them on the GPU, the feeder library writes summary.tsv.  Option names are the reference's
 * (src/cli/compare.rs), --stratification included.  Outputs: summary.tsv, truth.vcf.gz, query.vcf.gz (+ .tbi).
 * --output-debug writes cli_settings.json, region_summary.tsv.gz and region_sequences.tsv.gz.
 */
#include <dlfcn.h>
#include <algorithm>
#include <atomic>
#include <map>
#include <mutex>
#include <cerrno>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include <sys/stat.h>

#include "../../../include/aardvark_amd.h"
#include "../../../include/aardvark_feeder.h"

namespace {

double seconds_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }

[[noreturn]] void die(int code, const char *what, const char *detail) {
    fprintf(stderr, "error: %s%s%s\n", what, detail && *detail ? ": " : "", detail ? detail : "");
    exit(code);
}

void usage() {
    fprintf(stderr,
            "usage: aardvark_amd_compare -r REF.fa[.gz] -t TRUTH.vcf[.gz] -q QUERY.vcf[.gz] -b REGIONS.bed[.gz] -o OUT_DIR\n"
            "  [--truth-sample S] [--query-sample S] [--compare-label L] [--strat-lists device|host] [--min-variant-gap 50] [--disable-variant-trimming]\n"
            "  [--reference-case upper|raw]  (default upper: soft-masked reference bases are compared as upper case)\n"
            "  [--max-branch-factor 50] [--enable-exact-shortcut] [--enable-haplotype-metrics] [--enable-weighted-haplotype-metrics]\n"
            "  [--enable-record-basepair-metrics] [-s STRAT.tsv] [--output-debug DIR] [--skip N] [--take N] [--device 0 | --devices 0,1,..] [--batch-regions 4000000] [--batch-form packed|wide]\n"
            "  [--context-strata gc|hp|gc,hp]  (GC-content bins and homopolymer classes as further region labels, made on the GPU from the reference alone; with or without -s;\n"
            "   packed feed and --strat-lists device only)  [--context-gc-edges 0,15,..,101] [--context-gc-pad 50] [--context-hp-edges 4,7,12,21] [--context-hp-pad 5]\n"
            "  [--bootstrap B]  (B Poisson-bootstrap replicates of the tallies, 1..4096, summed on the GPU; writes summary_ci.tsv: summary.tsv's rows with percentile intervals of\n"
            "   recall, precision and F1; default 0: off, no file)  [--bootstrap-seed 1] [--bootstrap-level 90|95|99 (default 95)]\n"
            "  [--size-strata]  (writes summary_size.tsv: summary.tsv's GT, HAP and WEIGHTED_HAP rows per size bin of the calls, size = |alt length - ref length|, the bin's\n"
            "   name in the filter column, summed on the GPU; BASEPAIR and RECORD_BP rows are not part of this file: they belong to a region's haplotypes, not to a call)\n"
            "  [--size-edges 1,6,16,50]  (1 to 15 ascending sizes, the first at least 1; default bins len_0 len_1_5 len_6_15 len_16_49 len_ge50)\n"
            "  [--roc QUAL|GQ]  (writes summary_roc.tsv: summary.tsv's GT, HAP and WEIGHTED_HAP rows once per threshold on the query calls' QUAL or FORMAT/GQ, the point's name\n"
            "   in the filter column, summed on the GPU from the ONE comparison of the job: an approximation of a filtered re-run per threshold, which could draw other regions)\n"
            "  [--roc-thresholds 5,10,15,20,25,30,35,40,50,60]  (1 to 31 finite, strictly ascending numbers; points score_all, score_ge_5, ..)\n"
            "  [--kind-strata]  (writes summary_kind.tsv: summary.tsv's GT, HAP and WEIGHTED_HAP rows per call kind — het / hom / nogt by the call's genotype x ts / tv / other by its\n"
            "   two allele bases, the kind's name in the filter column — and kind_ratios.tsv: Ti/Tv and het/hom of the GT counts per region label, variant type and set; summed on the GPU)\n"
            "  [--bootstrap-per-call]  (with --bootstrap B and --size-strata and / or --kind-strata: the replicates of the size-bin and call-kind blocks as well; writes\n"
            "   summary_size_ci.tsv, summary_kind_ci.tsv and kind_ratios_ci.tsv: the rows of the plain files with --bootstrap-level percentile intervals)\n");
}

std::string json_string(const std::string &s) {
    std::string out = "\"";
    for (unsigned char c : s) {
        if (c == '"') out += "\\\"";
        else if (c == '\\') out += "\\\\";
        else if (c == '\n') out += "\\n";
        else if (c == '\t') out += "\\t";
        else if (c == '\r') out += "\\r";
        else if (c < 0x20) {
            char buf[8];
            snprintf(buf, sizeof(buf), "\\u%04x", c);
            out += buf;
        } else out.push_back((char)c);
    }
    return out + "\"";
}

} // namespace

/* One line per region that was not solved.  A region this build REFUSES for its size (more than 60,000 calls, a window of 2^31 bases or
 * more — limits the reference does not have) says so, so that it is not taken for an error the reference would
 * report too. */
static void report_unsolved(const avk_region_batch &b, uint64_t r, int32_t status) {
    const uint64_t calls = (uint64_t)b.t_cnt[r] + b.q_cnt[r], window = b.end[r] - b.start[r];
    if (status == AVK_ST_INVALID_INPUT && (calls > 60000 || window >= (1ull << 31)))
        fprintf(stderr, "Region #%llu (contig %u:%llu-%llu) NOT COMPARED: %llu calls in a window of %llu bases is beyond this build's limits (60,000 calls, 2^31 bases); the reference has no such limit\n",
                (unsigned long long)b.region_id[r], b.contig_idx[r], (unsigned long long)b.start[r], (unsigned long long)b.end[r], (unsigned long long)calls, (unsigned long long)window);
    else
        fprintf(stderr, "Error while solving compare region #%llu (contig %u:%llu-%llu): status %d\n", (unsigned long long)b.region_id[r], b.contig_idx[r],
                (unsigned long long)b.start[r], (unsigned long long)b.end[r], status);
}

int main(int argc, char **argv) {
    setenv("GPU_MAX_HW_QUEUES", "24", 0); /* before the first HIP call: the solver's six streams need hardware queues of their own (include/aardvark_amd.h, avk_ctx_create) */
    const auto t_start = std::chrono::steady_clock::now();
    std::string ref, truth, query, bed, out_dir, truth_sample, query_sample, label = "compare", strat_tsv, debug_dir, strat_lists = "device";
    uint64_t gap = 50, branch = 50, skip = 0, take = 0, batch_regions = 4000000, threads = 1, max_ed = 5000, verbosity = 0;
    bool trimming = true, shortcut = false, hap = false, whap = false, rbp = false;
    bool ref_upper = true; /* --reference-case upper|raw (include/aardvark_feeder.h, avf_genome_load_case) */
    int device = 0;
    std::vector<int> devices; /* --devices: the contexts that share the region batches (the first one is `device`) */
    bool batch_given = false, want_packed = true;
    /* --context-strata: the families asked for, and the tool's default edges and pads (overridden by --context-gc-edges / --context-hp-edges / --context-*-pad) */
    bool cx_gc = false, cx_hp = false, cx_given = false, cx_override = false;
    std::vector<uint32_t> cx_gc_edges = {0, 15, 20, 25, 30, 55, 60, 65, 70, 75, 80, 85, 101}, cx_hp_edges = {4, 7, 12, 21};
    uint32_t cx_gc_pad = 50, cx_hp_pad = 5;
    /* --bootstrap: replicates of the tallies (avk_boot_spec) and the level of summary_ci.tsv's intervals */
    avk_boot_spec boot_spec = {0, 1};
    uint32_t boot_level = 95;
    bool boot_override = false;
    /* --size-strata: per-call tallies by size bin (avk_size_spec) for summary_size.tsv */
    bool size = false, size_override = false;
    std::vector<uint32_t> size_edges = {1, 6, 16, 50};
    /* --roc: the precision-recall curve by the query calls' QUAL or GQ (avk_score_spec) for summary_roc.tsv */
    bool roc = false, roc_override = false;
    /* --kind-strata: per-call tallies by call kind (het / hom x Ti / Tv) for summary_kind.tsv and kind_ratios.tsv */
    bool kind = false;
    bool pcb = false; /* --bootstrap-per-call: replicates of the size-bin and call-kind blocks (avk_callboot.h) */
    std::string roc_field, roc_list = "5,10,15,20,25,30,35,40,50,60";
    auto number_list = [](const std::string &opt, const std::string &list) {
        std::vector<uint32_t> out;
        for (size_t b = 0; b <= list.size();) {
            const size_t e = list.find(',', b);
            const std::string item = list.substr(b, e == std::string::npos ? std::string::npos : e - b);
            char *end = nullptr;
            const unsigned long long x = strtoull(item.c_str(), &end, 10);
            if (item.empty() || *end || x > 0xFFFFFFFFull) die(64, ("invalid value for " + opt).c_str(), list.c_str());
            out.push_back((uint32_t)x);
            if (e == std::string::npos) break;
            b = e + 1;
        }
        return out;
    };
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto val = [&]() -> const char * {
            if (i + 1 >= argc) die(64, "missing value for", a.c_str());
            return argv[++i];
        };
        if (a == "-r" || a == "--reference") ref = val();
        else if (a == "-t" || a == "--truth-vcf") truth = val();
        else if (a == "-q" || a == "--query-vcf") query = val();
        else if (a == "-b" || a == "--regions") bed = val();
        else if (a == "-o" || a == "--output-dir") out_dir = val();
        else if (a == "--truth-sample") truth_sample = val();
        else if (a == "--query-sample") query_sample = val();
        else if (a == "--compare-label") label = val();
        else if (a == "--min-variant-gap") gap = strtoull(val(), nullptr, 10);
        else if (a == "--disable-variant-trimming") trimming = false;
        else if (a == "--reference-case") {
            const std::string v = val();
            if (v != "upper" && v != "raw") die(78, "--reference-case must be 'upper' or 'raw'", "");
            ref_upper = v == "upper";
        }
        else if (a == "--max-branch-factor") branch = strtoull(val(), nullptr, 10);
        else if (a == "--enable-exact-shortcut") shortcut = true;
        else if (a == "--enable-haplotype-metrics") hap = true;
        else if (a == "--enable-weighted-haplotype-metrics") whap = true;
        else if (a == "--enable-record-basepair-metrics") rbp = true;
        else if (a == "--skip") skip = strtoull(val(), nullptr, 10);
        else if (a == "--take") take = strtoull(val(), nullptr, 10);
        else if (a == "--device") device = atoi(val());
        else if (a == "--batch-regions") {
            batch_regions = strtoull(val(), nullptr, 10);
            batch_given = true;
        } else if (a == "--devices") { /* one solver context per entry, e.g. 0,1,2,3 — or 0,0 for two contexts on one GPU */
            std::string list = val();
            devices.clear();
            for (size_t b = 0; b <= list.size();) {
                const size_t e = list.find(',', b);
                const std::string item = list.substr(b, e == std::string::npos ? std::string::npos : e - b);
                if (item.empty()) die(64, "invalid value for --devices", list.c_str());
                devices.push_back(atoi(item.c_str()));
                if (e == std::string::npos) break;
                b = e + 1;
            }
        }
        else if (a == "--batch-form") { /* packed (default; wide when the call set does not fit the form, or with --output-debug) | wide */
            const std::string v = val();
            if (v != "packed" && v != "wide") die(78, "--batch-form must be 'packed' or 'wide'", "");
            want_packed = v == "packed";
        }
        else if (a == "--threads") threads = strtoull(val(), nullptr, 10);          /* accepted for command-line compatibility */
        else if (a == "--max-edit-distance") max_ed = strtoull(val(), nullptr, 10); /* hidden in the reference as well, unused by it */
        else if (a == "-v" || a == "--verbose") verbosity += 1;
        else if (a == "-s" || a == "--stratification") strat_tsv = val();
        else if (a == "--strat-lists") {
            strat_lists = val();
            if (strat_lists != "device" && strat_lists != "host") die(64, "--strat-lists takes device or host", strat_lists.c_str());
        }
        else if (a == "--output-debug") debug_dir = val();
        else if (a == "--context-strata") {
            const std::string v = val();
            if (v != "gc" && v != "hp" && v != "gc,hp" && v != "hp,gc") die(64, "--context-strata takes gc, hp or gc,hp", v.c_str());
            cx_given = true, cx_gc = v.find("gc") != std::string::npos, cx_hp = v.find("hp") != std::string::npos;
        } else if (a == "--context-gc-edges") cx_gc_edges = number_list(a, val()), cx_override = true;
        else if (a == "--context-hp-edges") cx_hp_edges = number_list(a, val()), cx_override = true;
        else if (a == "--context-gc-pad") cx_gc_pad = number_list(a, val())[0], cx_override = true;
        else if (a == "--context-hp-pad") cx_hp_pad = number_list(a, val())[0], cx_override = true;
        else if (a == "--bootstrap") {
            const std::vector<uint32_t> v = number_list(a, val());
            if (v.size() != 1 || v[0] > AVK_BOOT_MAX_REPLICATES) die(64, "--bootstrap takes a number of replicates from 0 (off) to 4096", "");
            boot_spec.replicates = v[0];
        } else if (a == "--bootstrap-seed") {
            const char *v = val();
            char *end = nullptr;
            boot_spec.seed = strtoull(v, &end, 10), boot_override = true;
            if (!*v || *end) die(64, "invalid value for --bootstrap-seed", v);
        } else if (a == "--bootstrap-level") {
            const std::vector<uint32_t> v = number_list(a, val());
            if (v.size() != 1 || (v[0] != 90 && v[0] != 95 && v[0] != 99)) die(64, "--bootstrap-level takes 90, 95 or 99", "");
            boot_level = v[0], boot_override = true;
        }
        else if (a == "--size-strata") size = true;
        else if (a == "--size-edges") size_edges = number_list(a, val()), size_override = true;
        else if (a == "--roc") roc_field = val(), roc = true;
        else if (a == "--kind-strata") kind = true;
        else if (a == "--bootstrap-per-call") pcb = true;
        else if (a == "--roc-thresholds") roc_list = val(), roc_override = true;
        else if (a == "-h" || a == "--help") {
            usage();
            return 0;
        } else die(64, "unknown option", a.c_str());
    }
    if (ref.empty() || truth.empty() || query.empty() || out_dir.empty()) {
        usage();
        return 64;
    }
    if (gap == 0) die(78, "--min-variant-gap must be >0", "");
    if (branch == 0 || branch > 0xFFFFFFFFull) die(78, "--max-branch-factor must be >0", "");
    if (batch_regions == 0) batch_regions = 1;
    /* The context labels exist on one route only: the packed (or escaped) feed with the lists made on the device.  Everything else is refused here, by name:
     * there is no host route for the rule to fall back to. */
    avk_context_spec cx_spec;
    memset(&cx_spec, 0, sizeof(cx_spec));
    uint32_t n_ctx_labels = 0;
    if (cx_override && !cx_given) die(64, "--context-gc-edges, --context-hp-edges, --context-gc-pad and --context-hp-pad need --context-strata", "");
    if (cx_given) {
        if (strat_lists == "host") die(64, "--context-strata needs the labels listed on the GPU: it cannot be combined with --strat-lists host", "");
        if (!want_packed) die(64, "--context-strata needs the packed feed: it cannot be combined with --batch-form wide", "");
        if (!debug_dir.empty()) die(64, "--context-strata cannot be combined with --output-debug (the debug run solves the wide feed)", "");
        if ((cx_gc && cx_gc_edges.size() > AVK_CONTEXT_GC_EDGES_MAX) || (cx_hp && cx_hp_edges.size() > AVK_CONTEXT_HP_EDGES_MAX)) die(64, "--context-strata: too many edges", "");
        if (cx_gc) {
            cx_spec.gc_pad = cx_gc_pad, cx_spec.n_gc_edges = (uint32_t)cx_gc_edges.size();
            for (size_t k = 0; k < cx_gc_edges.size(); ++k) cx_spec.gc_edges[k] = cx_gc_edges[k];
        }
        if (cx_hp) {
            cx_spec.hp_pad = cx_hp_pad, cx_spec.n_hp_edges = (uint32_t)cx_hp_edges.size();
            for (size_t k = 0; k < cx_hp_edges.size(); ++k) cx_spec.hp_edges[k] = cx_hp_edges[k];
        }
        char name[64];
        if (avk_context_label_name(&cx_spec, 0, name, sizeof(name))) die(64, "--context-strata", avk_last_error(nullptr)); /* (the library's own check of the spec) */
        n_ctx_labels = (cx_spec.n_gc_edges ? cx_spec.n_gc_edges - 1 : 0) + cx_spec.n_hp_edges;
    }
    /* The replicates are summed where the blocks are: by kernel behind the packed call (avk_compare_packed_boot; labels from the sets resident on the GPU), or on the
     * host from the wide feed's results (avk_boot_tallies_host).  What neither route carries is refused here, by name. */
    const bool boot = boot_spec.replicates != 0;
    /* --bootstrap-per-call: the replicates of the size-bin and call-kind blocks are summed where those blocks are — on the resident batch by kernel on the packed feed
     * (avk_size_boot_tallies, avk_kind_boot_tallies: --bootstrap keeps the batch resident beside --size-strata / --kind-strata), on the host from the wide feed's
     * results (avk_size_boot_tallies_host, avk_kind_boot_tallies_host).  What neither route carries is refused here, by name, before anything is loaded. */
    if (pcb) {
        if (!boot) die(64, "--bootstrap-per-call needs --bootstrap B (the replicates' count, seed and level are --bootstrap's)", "");
        if (!size && !kind) die(64, "--bootstrap-per-call needs --size-strata or --kind-strata (the blocks whose replicates it sums)", "");
        if (!debug_dir.empty()) die(64, "--bootstrap-per-call cannot be combined with --output-debug (the debug run writes per-region tables, not replicates)", "");
        if (!strat_tsv.empty() && strat_lists == "host" && want_packed)
            die(64, "--bootstrap-per-call on the packed feed reads the labels from the sets on the GPU: it cannot be combined with --strat-lists host", "");
    }
    if (boot_override && !boot) die(64, "--bootstrap-seed and --bootstrap-level need --bootstrap", "");
    if (boot && !debug_dir.empty()) die(64, "--bootstrap cannot be combined with --output-debug (the debug run writes per-region tables, not replicates)", "");
    if (boot && !strat_tsv.empty() && strat_lists == "host" && want_packed)
        die(64, "--bootstrap on the packed feed reads the labels from the sets on the GPU: it cannot be combined with --strat-lists host", "");
    /* The size bins are summed where the per-call outputs are: by kernel on the packed feed (avk_compare_packed_size, or avk_size_tallies on the resident batch when
     * label sums or replicates are wanted of the same batch; scopes from the sets resident on the GPU), or on the host from the wide feed's results
     * (avk_size_tallies_host).  What neither route carries is refused here, by name. */
    avk_size_spec size_spec;
    memset(&size_spec, 0, sizeof(size_spec));
    if (size_override && !size) die(64, "--size-edges needs --size-strata", "");
    if (size) {
        if (size_edges.empty() || size_edges.size() > AVK_SIZE_EDGES_MAX) die(64, "--size-edges takes 1 to 15 strictly ascending sizes, the first at least 1", "");
        size_spec.n_edges = (uint32_t)size_edges.size();
        for (size_t k = 0; k < size_edges.size(); ++k) size_spec.edges[k] = size_edges[k];
        if (!avk_size_n_bins(&size_spec)) die(64, "--size-edges takes 1 to 15 strictly ascending sizes, the first at least 1", ""); /* (the library's own check of the spec) */
        if (!debug_dir.empty()) die(64, "--size-strata cannot be combined with --output-debug (the debug run writes per-region tables, not size bins)", "");
        if (!strat_tsv.empty() && strat_lists == "host" && want_packed)
            die(64, "--size-strata on the packed feed reads the labels from the sets on the GPU: it cannot be combined with --strat-lists host", "");
    }
    /* The curve by query score is summed where the size bins are, on the same routes (avk_compare_packed_score, avk_score_tallies on the resident batch,
     * avk_score_tallies_host on the wide feed); the same combinations are refused, by name. */
    avk_score_spec roc_spec;
    memset(&roc_spec, 0, sizeof(roc_spec));
    if (roc_override && !roc) die(64, "--roc-thresholds needs --roc", "");
    if (roc) {
        if (roc_field != "QUAL" && roc_field != "GQ") die(64, "--roc takes QUAL or GQ: unknown field", roc_field.c_str());
        const char *bad_list = "--roc-thresholds takes 1 to 31 finite, strictly ascending numbers";
        for (size_t b = 0; b <= roc_list.size();) {
            const size_t e = roc_list.find(',', b);
            const std::string item = roc_list.substr(b, e == std::string::npos ? std::string::npos : e - b);
            char *end = nullptr;
            const float x = strtof(item.c_str(), &end);
            if (item.empty() || *end || roc_spec.n_thresholds >= AVK_SCORE_THRESHOLDS_MAX) die(64, bad_list, roc_list.c_str());
            roc_spec.t[roc_spec.n_thresholds++] = x;
            if (e == std::string::npos) break;
            b = e + 1;
        }
        if (!avk_score_n_points(&roc_spec)) die(64, bad_list, roc_list.c_str()); /* (the library's own check of the spec) */
        if (!debug_dir.empty()) die(64, "--roc cannot be combined with --output-debug (the debug run writes per-region tables, not a curve)", "");
        if (!strat_tsv.empty() && strat_lists == "host" && want_packed)
            die(64, "--roc on the packed feed reads the labels from the sets on the GPU: it cannot be combined with --strat-lists host", "");
    }
    /* The call kinds are summed like the size bins: by kernel on the packed feed (avk_compare_packed_kind, or avk_kind_tallies on the resident batch when other sums are
     * wanted of the same batch), or on the host from the wide feed's results (avk_kind_tallies_host).  What neither route carries is refused here, by name. */
    if (kind) {
        if (!debug_dir.empty()) die(64, "--kind-strata cannot be combined with --output-debug (the debug run writes per-region tables, not call kinds)", "");
        if (!strat_tsv.empty() && strat_lists == "host" && want_packed)
            die(64, "--kind-strata on the packed feed reads the labels from the sets on the GPU: it cannot be combined with --strat-lists host", "");
    }
    /* the cap of avk_callboot.h, as soon as the labels are counted: the context labels are known here, the sets' once the table of sets is read */
    auto pcb_cap_check = [&](uint32_t labels) {
        if (!pcb) return;
        const uint64_t keys = (size ? size_spec.n_edges + 1u : 0u) > (kind ? (uint32_t)AVK_N_KINDS : 0u) ? size_spec.n_edges + 1u : (uint32_t)AVK_N_KINDS;
        if (!avk_callboot_blocks_ok((uint64_t)labels + 1, boot_spec.replicates, keys))
            die(64, "--bootstrap-per-call: replicates x (1 + region labels) x keys (size bins, or the 9 kinds) may not exceed 262144 blocks", "");
    };
    pcb_cap_check(n_ctx_labels);
    if (!devices.empty()) device = devices[0];
    if (mkdir(out_dir.c_str(), 0777) != 0 && errno != EEXIST) die(74, "cannot create output folder", out_dir.c_str());
    if (!debug_dir.empty() && mkdir(debug_dir.c_str(), 0777) != 0 && errno != EEXIST) die(74, "cannot create debug folder", debug_dir.c_str());
    if (!debug_dir.empty()) { /* the CLI options as the reference saves them (src/main.rs:64-82; serde field order of CompareSettings) */
        auto opt = [&](const std::string &v) { return v.empty() ? std::string("null") : json_string(v); };
        auto flag = [](bool v) { return std::string(v ? "true" : "false"); };
        std::string samples[2] = {truth_sample, query_sample};
        const std::string *files[2] = {&truth, &query};
        for (int i = 0; i < 2; ++i) { /* the first sample of the file when none was named (src/cli/compare.rs:186-194) */
            char first[4096];
            if (samples[i].empty() && avf_vcf_sample_name(files[i]->c_str(), 0, first, sizeof(first)) == 0) samples[i] = first;
        }
        std::string js = "{\n";
        js += "  \"aardvark_version\": " + json_string(avk_version()) + ",\n";
        js += "  \"reference_fn\": " + json_string(ref) + ",\n";
        js += "  \"truth_vcf_filename\": " + json_string(truth) + ",\n";
        js += "  \"query_vcf_filename\": " + json_string(query) + ",\n";
        js += "  \"regions\": " + opt(bed) + ",\n";
        js += "  \"stratifications\": " + opt(strat_tsv) + ",\n";
        js += "  \"output_folder\": " + json_string(out_dir) + ",\n";
        js += "  \"debug_folder\": " + json_string(debug_dir) + ",\n";
        js += "  \"compare_label\": " + json_string(label) + ",\n";
        js += "  \"truth_sample\": " + json_string(samples[0]) + ",\n";
        js += "  \"query_sample\": " + json_string(samples[1]) + ",\n";
        js += "  \"min_variant_gap\": " + std::to_string(gap) + ",\n";
        js += "  \"disable_variant_trimming\": " + flag(!trimming) + ",\n";
        js += "  \"max_edit_distance\": " + std::to_string(max_ed) + ",\n";
        js += "  \"max_branch_factor\": " + std::to_string(branch) + ",\n";
        js += "  \"enable_exact_shortcut\": " + flag(shortcut) + ",\n";
        js += "  \"enable_haplotype_scoring\": " + flag(hap) + ",\n";
        js += "  \"enable_weighted_haplotype_scoring\": " + flag(whap) + ",\n";
        js += "  \"enable_record_basepair_scoring\": " + flag(rbp) + ",\n";
        js += "  \"threads\": " + std::to_string(threads ? threads : 1) + ",\n";
        js += "  \"verbosity\": " + std::to_string(verbosity) + ",\n";
        js += "  \"skip_blocks\": " + std::to_string(skip) + ",\n";
        js += "  \"take_blocks\": " + (take ? std::to_string(take) : std::string("18446744073709551615")) + "\n}";
        FILE *fp = fopen((debug_dir + "/cli_settings.json").c_str(), "wb");
        if (!fp || fwrite(js.data(), 1, js.size(), fp) != js.size() || fclose(fp) != 0) die(74, "Error while saving CLI options", debug_dir.c_str());
    }

    /* the reference genome, the two call sets and the GPU context come up side by side */
    auto t0 = std::chrono::steady_clock::now();
    avf_genome *genome = nullptr;
    avf_calls *calls[2] = {nullptr, nullptr};
    avk_ctx *ctx = nullptr;
    int rc_calls[2] = {0, 0}, rc_ctx = 0;
    std::string err_calls[2], err_ctx;
    double s_calls[2] = {0, 0}, s_ctx = 0;
    std::thread th_calls[2], th_ctx;
    for (int i = 0; i < 2; ++i)
        th_calls[i] = std::thread([&, i] {
            const auto t = std::chrono::steady_clock::now();
            rc_calls[i] = avf_calls_load(i == 0 ? truth.c_str() : query.c_str(), i == 0 ? truth_sample.c_str() : query_sample.c_str(), trimming ? 1 : 0, &calls[i]);
            if (rc_calls[i]) err_calls[i] = avf_last_error(); /* the error text is per thread */
            s_calls[i] = seconds_since(t);
        });
    std::thread th_reserve;
    th_ctx = std::thread([&] {
        const auto t = std::chrono::steady_clock::now();
        rc_ctx = avk_ctx_create(device, &ctx);
        if (rc_ctx) err_ctx = avk_last_error(nullptr);
        else { /* the staging buffers of the solve stage while the inputs are still being read: a first guess from the size of the reference
                  file (a region per 750 bases is twice the density of a human call set); the exact sizes follow when the calls are loaded */
            struct stat st;
            if (stat(ref.c_str(), &st) == 0 && st.st_size > (256ll << 20)) {
                const bool gz = ref.size() > 3 && ref.compare(ref.size() - 3, 3, ".gz") == 0;
                const uint64_t guess = (uint64_t)st.st_size * (gz ? 4u : 1u) / 750u;
                th_reserve = std::thread([guess, &ctx] { (void)avk_ctx_warmup(ctx, guess, 2 * guess); }); /* (bounce buffer, device code, workspaces) joined before the solve stage */
            }
        }
        s_ctx = seconds_since(t);
    });
    const int rc_genome = avf_genome_load_case(ref.c_str(), ref_upper ? 1 : 0, &genome);
    const std::string err_genome = rc_genome ? avf_last_error() : "";
    const double s_genome = seconds_since(t0);
    for (std::thread &t : th_calls) t.join();
    th_ctx.join();
    if (rc_genome) die(74, "Error while loading reference genome", err_genome.c_str());
    for (int i = 0; i < 2; ++i)
        if (rc_calls[i]) die(74, "Error while building regions", err_calls[i].c_str());
    if (rc_ctx) die(70, "cannot create the GPU context", err_ctx.c_str());
    const double s_load = seconds_since(t0);

    avf_strat *strat = nullptr;
    if (!strat_tsv.empty() && avf_strat_load(strat_tsv.c_str(), &strat)) die(74, "Error while loading stratifications", avf_last_error());
    const uint32_t n_bed_labels = avf_strat_n_labels(strat), n_labels = n_bed_labels + n_ctx_labels; /* the sets' labels, then the context labels */
    if (boot && ((uint64_t)n_labels + 1) * boot_spec.replicates > AVK_BOOT_MAX_BLOCKS)
        die(64, "--bootstrap: replicates x (1 + region labels) may not exceed 16384 blocks", "");
    pcb_cap_check(n_labels);

    /* the reference goes to the GPU (upload + 2-bit packing) while the regions are walked */
    t0 = std::chrono::steady_clock::now();
    int rc_ref = 0;
    std::string err_ref;
    double s_ref = 0;
    std::thread th_ref([&] {
        const auto t = std::chrono::steady_clock::now();
        const uint32_t n_contigs = avf_genome_n_contigs(genome);
        std::vector<const uint8_t *> seqs(n_contigs);
        std::vector<uint64_t> lens(n_contigs);
        for (uint32_t c = 0; c < n_contigs; ++c) {
            seqs[c] = avf_genome_seq(genome, c);
            lens[c] = avf_genome_len(genome, c);
        }
        rc_ref = avk_ref_upload(ctx, n_contigs, seqs.data(), lens.data());
        if (rc_ref) err_ref = avk_last_error(ctx);
        s_ref = seconds_since(t);
    });
    avf_feed *feed = nullptr;
    const int rc_feed = avf_feed_from_calls(2, calls, bed.c_str(), genome, gap, 0, &feed);
    const std::string err_feed = rc_feed ? avf_last_error() : "";
    th_ref.join();
    if (rc_feed) die(74, "Error while building regions", err_feed.c_str());
    if (rc_ref) die(70, "reference upload failed", err_ref.c_str());
    std::thread th_free([&calls] { /* millions of small records: released beside the solve stage */
        avf_calls_free(calls[0]);
        avf_calls_free(calls[1]);
    });
    const avk_region_batch *all = avf_feed_batch(feed);
    /* --roc: the query VCF's scores, one pass over its data lines, gathered into the feed's call order (the packed form's order too); truth entries are NaN */
    std::vector<float> roc_scores(roc ? all->n_variants + 1 : 0);
    if (roc) {
        const uint64_t *rec = avf_feed_var_record(feed);
        uint64_t n_records = 0;
        for (uint64_t v = 0; v < all->n_variants; ++v) n_records = rec[v] + 1 > n_records ? rec[v] + 1 : n_records;
        std::vector<float> per_record(n_records + 1);
        if (avf_vcf_scores(query.c_str(), query_sample.c_str(), roc_field.c_str(), n_records, per_record.data()) ||
            avf_feed_scores(feed, per_record.data(), n_records, roc_scores.data()))
            die(74, "Error while reading the query scores", avf_last_error());
    }
    if (th_reserve.joinable()) th_reserve.join();
    const double s_feed = seconds_since(t0);
    fprintf(stderr, "Loaded %llu truth and %llu query variants; %llu regions.\n", (unsigned long long)avf_feed_loaded_variants(feed, 0),
            (unsigned long long)avf_feed_loaded_variants(feed, 1), (unsigned long long)all->n_regions);

    /* the feed in the library's packed form (10 bytes per region, 5 per call + allele bytes over PCIe instead of 479 MB per whole genome); the wide arrays
     * stay for the writers.  Ordinary memory: pinning it would cost more than the one pass through the library's bounce buffer it saves. */
    avk_packed_batch packed_all;
    avk_packed_escapes esc_all; /* the plain pack first; then the pack with escapes (long alleles, long windows, dense sides); only then the wide form */
    memset(&esc_all, 0, sizeof(esc_all));
    bool packed = false;
    if (want_packed && debug_dir.empty()) {
        int rc_pack = avf_feed_pack(feed, [](void *, size_t bytes) { return malloc(bytes); }, nullptr, &packed_all);
        if (rc_pack == 1) rc_pack = avf_feed_pack_esc(feed, [](void *, size_t bytes) { return malloc(bytes); }, nullptr, &packed_all, &esc_all);
        if (rc_pack < 0) die(70, "cannot pack the region batch", avf_last_error());
        packed = rc_pack == 0;
    }
    if (cx_given && !packed) die(70, "--context-strata needs the packed feed, and this call set does not fit the packed form even with escapes", "");
    const bool escaped = packed && (esc_all.n_esc_regions || esc_all.n_esc_slots || esc_all.n_esc_calls);
    /* regions [first + at, +n): as a batch in the chosen form; `out` is indexed by the feed's call arrays either way */
    auto out_for = [](avk_result_batch out, uint64_t v_first) { /* a packed part's results are indexed from its first call */
        if (out.var_expected) out.var_expected += v_first;
        if (out.var_observed) out.var_observed += v_first;
        if (out.var_class) out.var_class += v_first;
        if (out.var_zyg) out.var_zyg += v_first;
        return out;
    };
    auto compare_part = [&](avk_ctx *c, const avk_region_batch &b, uint64_t at_abs, uint64_t n, const avk_compare_config &cfg, const avk_result_batch &out) -> int {
        if (!packed) return avk_compare_batch(c, &b, &cfg, const_cast<avk_result_batch *>(&out));
        avk_packed_batch part;
        avk_packed_escapes part_esc;
        uint64_t v_first = 0;
        if (avf_packed_slice_esc(feed, &packed_all, &esc_all, at_abs, n, &part, &part_esc, &v_first)) return AVK_E_ARG;
        avk_result_batch shifted = out_for(out, v_first);
        return avk_compare_packed_esc(c, &part, &part_esc, &cfg, &shifted);
    };
    /* the same with the stratified sums: the labels' sums come from the batch's compact results on the device (avk_compare_packed_labels), no metric blocks */
    auto compare_part_labels = [&](avk_ctx *c, uint64_t at_abs, uint64_t n, const avk_compare_config &cfg, const avk_result_batch &out, uint32_t n_lab, const uint64_t *label_off,
                                   const uint32_t *label_idx, uint64_t *sums) -> int {
        avk_packed_batch part;
        avk_packed_escapes part_esc;
        uint64_t v_first = 0;
        if (avf_packed_slice_esc(feed, &packed_all, &esc_all, at_abs, n, &part, &part_esc, &v_first)) return AVK_E_ARG;
        avk_result_batch shifted = out_for(out, v_first);
        avk_region_labels lab;
        lab.n_labels = n_lab, lab.label_off = label_off, lab.label_idx = label_idx;
        return avk_compare_packed_labels(c, &part, &part_esc, &lab, &cfg, &shifted, sums);
    };
    /* ... and with the lists made on the device from the resident interval sets (avk_compare_packed_strata): nothing but the batch goes in */
    auto compare_part_strata = [&](avk_ctx *c, uint64_t at_abs, uint64_t n, const avk_compare_config &cfg, const avk_result_batch &out, const avk_strata *sets, uint64_t *sums) -> int {
        avk_packed_batch part;
        avk_packed_escapes part_esc;
        uint64_t v_first = 0;
        if (avf_packed_slice_esc(feed, &packed_all, &esc_all, at_abs, n, &part, &part_esc, &v_first)) return AVK_E_ARG;
        avk_result_batch shifted = out_for(out, v_first);
        return avk_compare_packed_strata(c, &part, &part_esc, sets, &cfg, &shifted, sums);
    };
    /* --bootstrap on the packed feed: compare_part / compare_part_strata that also add the part's replicates to `reps` (avk_compare_packed_boot; sets may be NULL) */
    auto compare_part_boot = [&](avk_ctx *c, uint64_t at_abs, uint64_t n, const avk_compare_config &cfg, const avk_result_batch &out, const avk_strata *sets, uint64_t *sums,
                                 uint64_t *reps) -> int {
        avk_packed_batch part;
        avk_packed_escapes part_esc;
        uint64_t v_first = 0;
        if (avf_packed_slice_esc(feed, &packed_all, &esc_all, at_abs, n, &part, &part_esc, &v_first)) return AVK_E_ARG;
        avk_result_batch shifted = out_for(out, v_first);
        return avk_compare_packed_boot(c, &part, &part_esc, sets, &cfg, &shifted, sums, &boot_spec, reps);
    };
    /* --bootstrap on the wide feed: the part's replicates from its results on the host (avk_boot_tallies_host: `out` carries the compact BASEPAIR groups) */
    struct HostGroups {
        std::vector<uint32_t> off, groups;
    };
    auto host_groups = [&](uint64_t n, avk_result_batch &out, HostGroups &g) {
        g.off.assign(n + 1, 0), g.groups.assign(4 * (size_t)(n + all->n_variants + 1), 0);
        out.bp_off = g.off.data(), out.bp_groups = g.groups.data();
    };
    auto boot_part_host = [&](const avk_region_batch &b, const avk_result_batch &out, const uint64_t *label_off, const uint32_t *label_idx, uint64_t *reps) -> int {
        avk_region_labels lab;
        lab.n_labels = n_labels, lab.label_off = label_off, lab.label_idx = label_idx;
        return avk_boot_tallies_host(&b, &out, &boot_spec, n_labels ? &lab : nullptr, 16, reps);
    };
    /* --bootstrap-per-call: a context's (or, on the wide feed, a worker's) replicates of the two blocks, found by a key of its own — the context on the packed
     * feed, the worker's block of plain sums on the wide feed — and added on the host at the end, as the contexts' other blocks are */
    struct PerCall {
        std::vector<uint64_t> size_reps, kind_reps;
    };
    std::map<const void *, PerCall> pcb_bufs;
    std::mutex pcb_mutex;
    auto pcb_of = [&](const void *key) -> PerCall & {
        std::lock_guard<std::mutex> lock(pcb_mutex);
        PerCall &pc = pcb_bufs[key];
        const size_t scopes = (size_t)(avf_strat_n_labels(strat) + n_ctx_labels) + 1;
        if (size && pc.size_reps.empty()) pc.size_reps.assign(scopes * boot_spec.replicates * (size_spec.n_edges + 1u) * AVK_CALLBOOT_KEY_WORDS, 0);
        if (kind && pc.kind_reps.empty()) pc.kind_reps.assign(scopes * boot_spec.replicates * AVK_N_KINDS * AVK_CALLBOOT_KEY_WORDS, 0);
        return pc;
    };
    /* --size-strata on the packed feed: the part's results and its size blocks.  Alone it is one call (avk_compare_packed_size); when the labels' sums or the
     * replicates are wanted of the same batch the batch stays resident: solve, download (the capacity retry patches the device view), then the label, bootstrap and
     * size kernels on it — the sums the one-call forms return */
    auto compare_part_size = [&](avk_ctx *c, uint64_t at_abs, uint64_t n, const avk_compare_config &cfg, const avk_result_batch &out, const avk_strata *sets, uint64_t *sums,
                                 uint64_t *reps, uint64_t *blocks) -> int {
        avk_packed_batch part;
        avk_packed_escapes part_esc;
        uint64_t v_first = 0;
        if (avf_packed_slice_esc(feed, &packed_all, &esc_all, at_abs, n, &part, &part_esc, &v_first)) return AVK_E_ARG;
        avk_result_batch shifted = out_for(out, v_first);
        if (!sets && !boot) return avk_compare_packed_size(c, &part, &part_esc, nullptr, &cfg, &size_spec, &shifted, blocks);
        avk_dev_batch *db = nullptr;
        int rc = avk_batch_upload_packed_esc(c, &part, &part_esc, &db);
        if (!rc) rc = avk_compare_resident(c, db, &cfg, nullptr);
        if (!rc) rc = avk_results_download(c, db, &shifted);
        if (!rc && sets) rc = avk_label_tallies_strata(c, db, sets, sums);
        if (!rc && boot) rc = avk_boot_tallies(c, db, &boot_spec, sets, reps);
        if (!rc) rc = avk_size_tallies(c, db, &size_spec, sets, blocks);
        if (!rc && pcb) rc = avk_size_boot_tallies(c, db, &size_spec, &boot_spec, sets, pcb_of(c).size_reps.data());
        if (db) avk_batch_free(c, db);
        return rc;
    };
    /* --roc on the packed feed, the same way: alone one call (avk_compare_packed_score); with label sums, replicates or size bins of the same batch on the resident
     * batch.  A part's scores are the feed's from its first call on */
    auto compare_part_roc = [&](avk_ctx *c, uint64_t at_abs, uint64_t n, const avk_compare_config &cfg, const avk_result_batch &out, const avk_strata *sets, uint64_t *sums,
                                uint64_t *reps, uint64_t *blocks, uint64_t *curve) -> int {
        avk_packed_batch part;
        avk_packed_escapes part_esc;
        uint64_t v_first = 0;
        if (avf_packed_slice_esc(feed, &packed_all, &esc_all, at_abs, n, &part, &part_esc, &v_first)) return AVK_E_ARG;
        avk_result_batch shifted = out_for(out, v_first);
        const float *sc = roc_scores.data() + v_first;
        if (!sets && !boot && !size) return avk_compare_packed_score(c, &part, &part_esc, nullptr, &cfg, &roc_spec, sc, &shifted, curve);
        avk_dev_batch *db = nullptr;
        int rc = avk_batch_upload_packed_esc(c, &part, &part_esc, &db);
        if (!rc) rc = avk_compare_resident(c, db, &cfg, nullptr);
        if (!rc) rc = avk_results_download(c, db, &shifted);
        if (!rc && sets) rc = avk_label_tallies_strata(c, db, sets, sums);
        if (!rc && boot) rc = avk_boot_tallies(c, db, &boot_spec, sets, reps);
        if (!rc && size) rc = avk_size_tallies(c, db, &size_spec, sets, blocks);
        if (!rc && size && pcb) rc = avk_size_boot_tallies(c, db, &size_spec, &boot_spec, sets, pcb_of(c).size_reps.data());
        if (!rc) rc = avk_score_tallies(c, db, &roc_spec, sc, sets, curve);
        if (db) avk_batch_free(c, db);
        return rc;
    };
    /* --kind-strata on the packed feed, the same way: alone one call (avk_compare_packed_kind); with label sums, replicates, size bins or the curve of the same batch
     * on the resident batch */
    auto compare_part_kind = [&](avk_ctx *c, uint64_t at_abs, uint64_t n, const avk_compare_config &cfg, const avk_result_batch &out, const avk_strata *sets, uint64_t *sums,
                                 uint64_t *reps, uint64_t *blocks, uint64_t *curve, uint64_t *kinds) -> int {
        avk_packed_batch part;
        avk_packed_escapes part_esc;
        uint64_t v_first = 0;
        if (avf_packed_slice_esc(feed, &packed_all, &esc_all, at_abs, n, &part, &part_esc, &v_first)) return AVK_E_ARG;
        avk_result_batch shifted = out_for(out, v_first);
        if (!sets && !boot && !size && !roc) return avk_compare_packed_kind(c, &part, &part_esc, nullptr, &cfg, &shifted, kinds);
        avk_dev_batch *db = nullptr;
        int rc = avk_batch_upload_packed_esc(c, &part, &part_esc, &db);
        if (!rc) rc = avk_compare_resident(c, db, &cfg, nullptr);
        if (!rc) rc = avk_results_download(c, db, &shifted);
        if (!rc && sets) rc = avk_label_tallies_strata(c, db, sets, sums);
        if (!rc && boot) rc = avk_boot_tallies(c, db, &boot_spec, sets, reps);
        if (!rc && size) rc = avk_size_tallies(c, db, &size_spec, sets, blocks);
        if (!rc && size && pcb) rc = avk_size_boot_tallies(c, db, &size_spec, &boot_spec, sets, pcb_of(c).size_reps.data());
        if (!rc && roc) rc = avk_score_tallies(c, db, &roc_spec, roc_scores.data() + v_first, sets, curve);
        if (!rc) rc = avk_kind_tallies(c, db, sets, kinds);
        if (!rc && pcb) rc = avk_kind_boot_tallies(c, db, &boot_spec, sets, pcb_of(c).kind_reps.data());
        if (db) avk_batch_free(c, db);
        return rc;
    };
    /* --kind-strata on the wide feed: the part's blocks from its results on the host */
    auto kind_part_host = [&](const avk_region_batch &b, const avk_result_batch &out, const uint64_t *label_off, const uint32_t *label_idx, uint64_t *kinds) -> int {
        avk_region_labels lab;
        lab.n_labels = n_labels, lab.label_off = label_off, lab.label_idx = label_idx;
        const int rc = avk_kind_tallies_host(&b, &out, n_labels ? &lab : nullptr, 16, kinds);
        return rc || !pcb ? rc : avk_kind_boot_tallies_host(&b, &out, &boot_spec, n_labels ? &lab : nullptr, 16, pcb_of(kinds).kind_reps.data());
    };
    /* --roc on the wide feed: the part's curve from its results on the host (the part's call offsets are the feed's) */
    auto roc_part_host = [&](const avk_region_batch &b, const avk_result_batch &out, const uint64_t *label_off, const uint32_t *label_idx, uint64_t *curve) -> int {
        avk_region_labels lab;
        lab.n_labels = n_labels, lab.label_off = label_off, lab.label_idx = label_idx;
        return avk_score_tallies_host(&b, &out, &roc_spec, roc_scores.data(), n_labels ? &lab : nullptr, 16, curve);
    };
    /* --size-strata on the wide feed: the part's blocks from its results on the host */
    auto size_part_host = [&](const avk_region_batch &b, const avk_result_batch &out, const uint64_t *label_off, const uint32_t *label_idx, uint64_t *blocks) -> int {
        avk_region_labels lab;
        lab.n_labels = n_labels, lab.label_off = label_off, lab.label_idx = label_idx;
        const int rc = avk_size_tallies_host(&b, &out, &size_spec, n_labels ? &lab : nullptr, 16, blocks);
        return rc || !pcb ? rc : avk_size_boot_tallies_host(&b, &out, &size_spec, &boot_spec, n_labels ? &lab : nullptr, 16, pcb_of(blocks).size_reps.data());
    };
    auto upload_part = [&](avk_ctx *c, const avk_region_batch &b, uint64_t at_abs, uint64_t n, avk_dev_batch **db, uint64_t *v_first) -> int {
        *v_first = 0;
        if (!packed) return avk_batch_upload(c, &b, db);
        avk_packed_batch part;
        avk_packed_escapes part_esc;
        if (avf_packed_slice_esc(feed, &packed_all, &esc_all, at_abs, n, &part, &part_esc, v_first)) return AVK_E_ARG;
        return avk_batch_upload_packed_esc(c, &part, &part_esc, db);
    };

    /* --skip / --take select regions by position in the iterator (src/main.rs:215-231) */
    const uint64_t first = skip < all->n_regions ? skip : all->n_regions;
    uint64_t count = all->n_regions - first;
    if (take && take < count) count = take;

    t0 = std::chrono::steady_clock::now();
    std::vector<uint64_t> total(AVK_TALLY_LEN, 0), tally(AVK_TALLY_LEN);
    avk_compare_config cfg;
    cfg.max_branch_factor = (uint32_t)branch;
    cfg.enable_sequences = 0;
    cfg.enable_exact_shortcut = shortcut ? 1 : 0;
    std::vector<int32_t> status(all->n_regions, -1); /* regions outside --skip/--take stay unsolved and unwritten */
    std::vector<uint8_t> var_expected(all->n_variants + 1), var_observed(all->n_variants + 1), var_class(all->n_variants + 1);
    /* stratified tallies (SummaryWriter::add_comparison_benchmark, summary.rs:146-163): label l sums the metric blocks of the
     * regions it contains, so the per-region blocks come back from the GPU, in batches that keep them at a few hundred MB */
    const bool debug = !debug_dir.empty();
    /* the per-region blocks only come back to the host for the debug tables; the stratified tallies are summed on the GPU from the region labels the feeder
     * library lists (avf_strat_batch_labels): on the packed feed from the batch's compact results (avk_compare_packed_labels: no per-region blocks at all), on the
     * wide feed from per-region blocks that stay on the device (avk_label_tallies) */
    const bool device_labels = n_labels && !debug;
    const bool compact_labels = device_labels && packed;
    /* --strat-lists device (the default: profiles/strata_device_ab.txt): the interval sets are uploaded once per context and the region -> label lists are made by
     * kernel (avk_strata.inl); host: the feeder library lists them on host threads and they cross with the batch (A/B runs, and the fallback when the sets cannot be
     * exported or uploaded).  The wide feed and the debug run keep their routes. */
    bool strata_route = compact_labels && strat_lists == "device"; /* (falls back to the host route, with a note, when the sets cannot be exported or uploaded) */
    std::vector<uint64_t> sx_tree_off;
    std::vector<uint32_t> sx_start, sx_end_max;
    const uint32_t sx_contigs = avf_genome_n_contigs(genome);
    auto strata_upload = [&](avk_ctx *c, avk_strata **sets) -> int {
        return avk_strata_upload_context(c, n_bed_labels, sx_contigs, sx_tree_off.data(), sx_start.data(), sx_end_max.data(), cx_given ? &cx_spec : nullptr, sets);
    };
    avk_strata *strata = nullptr;
    if (strata_route) {
        sx_tree_off.assign((size_t)n_bed_labels * sx_contigs + 1, 0);
        std::string why;
        if (!n_bed_labels) sx_start.assign(1, 0), sx_end_max.assign(1, 0); /* (context labels alone: no sets to export) */
        else if (avf_strat_export(strat, genome, sx_tree_off.data(), nullptr, nullptr)) why = std::string("cannot export the stratification sets: ") + avf_last_error();
        if (why.empty() && n_bed_labels) {
            sx_start.assign(sx_tree_off.back() + 1, 0), sx_end_max.assign(sx_tree_off.back() + 1, 0);
            if (avf_strat_export(strat, genome, sx_tree_off.data(), sx_start.data(), sx_end_max.data())) why = std::string("cannot export the stratification sets: ") + avf_last_error();
        }
        if (why.empty() && strata_upload(ctx, &strata)) why = std::string("cannot upload the stratification sets: ") + avk_last_error(ctx);
        if (!why.empty() && cx_given) die(70, "--context-strata", why.c_str()); /* (no host route makes these labels) */
        if (!why.empty()) {
            fprintf(stderr, "Warning: %s; the region labels are listed on the host instead (--strat-lists host).\n", why.c_str());
            strata_route = false;
        }
    }
    if (boot && packed && n_labels && !strata_route) die(70, "--bootstrap on the packed feed needs the stratification sets on the GPU, and they could not be put there", "");
    const bool boot_host = boot && !packed; /* the wide feed: avk_boot_tallies_host on each part's results */
    if (size && packed && n_labels && !strata_route) die(70, "--size-strata on the packed feed needs the stratification sets on the GPU, and they could not be put there", "");
    const bool size_host = size && !packed;                            /* the wide feed: avk_size_tallies_host on each part's results */
    const bool size_resident = size && packed && (strata_route || boot || roc || kind); /* label sums, replicates or the score curve of the same batch: the kernels run on the resident batch */
    if (roc && packed && n_labels && !strata_route) die(70, "--roc on the packed feed needs the stratification sets on the GPU, and they could not be put there", "");
    const bool roc_host = roc && !packed;                                   /* the wide feed: avk_score_tallies_host on each part's results */
    const bool roc_resident = roc && packed && (strata_route || boot || size || kind); /* other sums of the same batch: the kernels run on the resident batch */
    if (kind && packed && n_labels && !strata_route) die(70, "--kind-strata on the packed feed needs the stratification sets on the GPU, and they could not be put there", "");
    const bool kind_host = kind && !packed;                                         /* the wide feed: avk_kind_tallies_host on each part's results */
    const bool kind_resident = kind && packed && (strata_route || boot || size || roc); /* other sums of the same batch: the kernels run on the resident batch */
    (void)avk_ctx_set_option(ctx, "emit_group_metrics", (n_labels && !compact_labels) || debug ? 1 : 0);
    if (boot_host || size_resident || roc_resident || kind_resident) (void)avk_ctx_set_option(ctx, "emit_bp_groups", 1);
    std::vector<uint64_t> kind_total(kind ? ((size_t)n_labels + 1) * AVK_N_KINDS * AVK_N_GROUPS * AVK_SIZE_FIELDS : 0, 0);
    if (verbosity && kind)
        fprintf(stderr, "Call kinds: %u kinds in summary_kind.tsv (GT, HAP, WEIGHTED_HAP; no BASEPAIR rows) and their Ti/Tv and het/hom in kind_ratios.tsv; the kinds are summed %s.\n",
                (unsigned)AVK_N_KINDS,
                kind_host       ? "on the host from each batch's results (avk_kind_tallies_host, the wide feed)"
                : kind_resident ? "on the GPU on each resident batch behind its solve and download (avk_kind_tallies)"
                                : "on the GPU behind each batch's solve (avk_compare_packed_kind)");
    const uint32_t roc_points = roc ? roc_spec.n_thresholds + 1 : 0;
    std::vector<uint64_t> roc_total(roc ? ((size_t)n_labels + 1) * roc_points * AVK_N_GROUPS * AVK_SCORE_FIELDS : 0, 0);
    if (verbosity && roc)
        fprintf(stderr, "Score curve: %u points by %s in summary_roc.tsv (GT, HAP, WEIGHTED_HAP; no BASEPAIR rows), from the one comparison of the job; the points are summed %s.\n",
                roc_points, roc_field.c_str(),
                roc_host       ? "on the host from each batch's results (avk_score_tallies_host, the wide feed)"
                : roc_resident ? "on the GPU on each resident batch behind its solve and download (avk_score_tallies)"
                               : "on the GPU behind each batch's solve (avk_compare_packed_score)");
    const uint32_t size_bins = size ? size_spec.n_edges + 1 : 0;
    std::vector<uint64_t> size_total(size ? ((size_t)n_labels + 1) * size_bins * AVK_N_GROUPS * AVK_SIZE_FIELDS : 0, 0);
    if (verbosity && size)
        fprintf(stderr, "Size bins: %u bins in summary_size.tsv (GT, HAP, WEIGHTED_HAP; no BASEPAIR rows); the bins are summed %s.\n", size_bins,
                size_host       ? "on the host from each batch's results (avk_size_tallies_host, the wide feed)"
                : size_resident ? "on the GPU on each resident batch behind its solve and download (avk_size_tallies)"
                                : "on the GPU behind each batch's solve (avk_compare_packed_size)");
    std::vector<uint64_t> boot_total(boot ? ((size_t)n_labels + 1) * boot_spec.replicates * AVK_TALLY_LEN : 0, 0);
    if (verbosity && boot)
        fprintf(stderr, "Bootstrap: %u replicates, seed %llu, %u %% intervals in summary_ci.tsv; the replicates are summed %s.\n", boot_spec.replicates,
                (unsigned long long)boot_spec.seed, boot_level,
                boot_host ? "on the host from each batch's results (avk_boot_tallies_host, the wide feed)" : "on the GPU behind each batch's solve (avk_compare_packed_boot)");
    if (verbosity && pcb)
        fprintf(stderr, "Per-call bootstrap: %u replicates of the %s%s%s in %s%s%s, %u %% intervals; the replicates are summed %s.\n", boot_spec.replicates, size ? "size bins" : "",
                size && kind ? " and the " : "", kind ? "call kinds" : "", size ? "summary_size_ci.tsv" : "", size && kind ? ", " : "", kind ? "summary_kind_ci.tsv and kind_ratios_ci.tsv" : "",
                boot_level,
                !packed ? "on the host from each batch's results (avk_size_boot_tallies_host / avk_kind_boot_tallies_host, the wide feed)"
                        : "on the GPU on each resident batch behind its solve and download (avk_size_boot_tallies / avk_kind_boot_tallies)");
    if (verbosity && compact_labels) {
        if (strata_route)
            fprintf(stderr, "Region labels: listed on the GPU (--strat-lists device, avk_compare_packed_strata): %llu intervals of %u labels uploaded once per context.\n",
                    (unsigned long long)sx_tree_off.back(), n_bed_labels);
        else fprintf(stderr, "Region labels: listed on the host (--strat-lists host, avf_strat_batch_labels) and copied with every batch.\n");
    }
    if (verbosity && cx_given)
        fprintf(stderr, "Context labels: %u (%u GC bins with pad %u, %u homopolymer classes with pad %u), made on the GPU from the reference (--context-strata, avk_strata_upload_context).\n",
                n_ctx_labels, cx_spec.n_gc_edges ? cx_spec.n_gc_edges - 1 : 0, cx_spec.gc_pad, cx_spec.n_hp_edges, cx_spec.hp_pad);
    if (verbosity && n_labels)
        fprintf(stderr, "Stratified sums: %s.\n", compact_labels ? "from the compact results on the GPU (avk_compare_packed_labels), no per-region metric blocks"
                                                     : device_labels ? "from per-region metric blocks on the GPU (avk_label_tallies)"
                                                                     : "from the per-region metric blocks of the debug tables, on the host");
    if (debug && batch_regions > 262144) batch_regions = 262144;
    cfg.enable_sequences = debug ? 1 : 0; /* enable_sequences(region_seq_writer.is_some()), src/main.rs:236 */
    uint32_t mask = AVF_METRIC_GT | AVF_METRIC_BASEPAIR;
    if (hap) mask |= AVF_METRIC_HAP;
    if (whap) mask |= AVF_METRIC_WEIGHTED_HAP;
    if (rbp) mask |= AVF_METRIC_RECORD_BP;
    avf_table *region_table = nullptr, *sequence_table = nullptr;
    if (debug) { /* the debug tables (src/main.rs:163-188) */
        if (avf_region_summary_open((debug_dir + "/region_summary.tsv.gz").c_str(), mask, &region_table) ||
            avf_region_sequences_open((debug_dir + "/region_sequences.tsv.gz").c_str(), &sequence_table))
            die(74, "Error while building debug writers", avf_last_error());
    }
    std::vector<uint8_t> seq_bytes;
    std::vector<uint64_t> seq_off;
    std::vector<uint32_t> seq_stride, seq_len;
    std::vector<uint64_t> strat_total((size_t)n_labels * AVK_TALLY_LEN, 0);
    std::vector<uint32_t> gm, labels(n_labels ? n_labels : 1);
    /* Several contexts (--devices: one per entry, GPUs may repeat) share the region batches: regions are independent, every context
     * solves the batches it draws, the tallies are summed on the host (the sum the benchmark does with one RCCL all-reduce across
     * processes).  The debug tables are written in region order by one context. */
    const size_t n_workers = debug || devices.size() < 2 ? 1 : devices.size();
    /* --devices with the packed feed and no stratification: the job is cut by the library's ONE rule, shard = hash(region_id) % ranks (avk_region_shard, the rule of
     * aardvark_amd/dist.py), every context solves its shard, and the job tally is summed over the ranks — by one RCCL all-reduce (avk_tally_allreduce) when every
     * context has a GPU of its own, on the host when entries repeat (RCCL does not take two ranks on one device). */
    if (verbosity)
        fprintf(stderr, "Batch form: %s (%llu escaped regions, %llu escaped counts, %llu escaped calls); %zu context%s the job.\n",
                !packed ? "wide" : escaped ? "packed with escapes" : "packed", (unsigned long long)esc_all.n_esc_regions, (unsigned long long)esc_all.n_esc_slots,
                (unsigned long long)esc_all.n_esc_calls, n_workers, n_workers == 1 ? " solves" : "s solve");
    bool sharded = false;
    if (verbosity && boot && n_workers > 1 && packed && !n_labels)
        fprintf(stderr, "Bootstrap: the hash-sharded route does not carry the replicates; --bootstrap selects the route on which the contexts share the region batches.\n");
    if (verbosity && size && n_workers > 1 && packed && !n_labels)
        fprintf(stderr, "Size bins: the hash-sharded route does not carry the blocks; --size-strata selects the route on which the contexts share the region batches.\n");
    if (verbosity && roc && n_workers > 1 && packed && !n_labels)
        fprintf(stderr, "Score curve: the hash-sharded route does not carry the blocks; --roc selects the route on which the contexts share the region batches.\n");
    if (verbosity && kind && n_workers > 1 && packed && !n_labels)
        fprintf(stderr, "Call kinds: the hash-sharded route does not carry the blocks; --kind-strata selects the route on which the contexts share the region batches.\n");
    if (n_workers > 1 && packed && !n_labels && !boot && !size && !roc && !kind) {
        sharded = true;
        avk_packed_batch sel;
        avk_packed_escapes sel_esc;
        uint64_t sel_v = 0;
        if (avf_packed_slice_esc(feed, &packed_all, &esc_all, first, count, &sel, &sel_esc, &sel_v)) die(70, "cannot select the regions", avf_last_error());
        bool distinct = true;
        for (size_t i = 0; i < n_workers; ++i)
            for (size_t j = i + 1; j < n_workers; ++j) distinct = distinct && devices[i] != devices[j];
        std::vector<void *> comms(n_workers, nullptr);
        if (distinct) { /* one communicator per context, made here (ncclCommInitAll of RCCL, looked up at run time: the tool does not link it) */
            typedef int (*init_all_fn)(void **, int, const int *);
            void *h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
            init_all_fn init_all = h ? (init_all_fn)dlsym(h, "ncclCommInitAll") : nullptr;
            if (!init_all || init_all(comms.data(), (int)n_workers, devices.data()) != 0) {
                if (verbosity) fprintf(stderr, "RCCL is not available (%s): the ranks' tallies are summed on the host.\n", h ? "ncclCommInitAll failed" : "librccl.so not found");
                distinct = false;
                std::fill(comms.begin(), comms.end(), nullptr);
            }
        }
        std::vector<std::string> worker_err(n_workers);
        std::vector<std::vector<uint64_t>> w_total(n_workers, std::vector<uint64_t>(AVK_TALLY_LEN, 0));
        std::mutex log_mutex;
        std::vector<avk_ctx *> w_ctx(n_workers, nullptr); /* the contexts outlive the workers: the collective runs after every rank is known to have solved its shard */
        w_ctx[0] = ctx;
        auto shard_worker = [&](size_t w) {
            avk_ctx *my = ctx;
            if (w > 0) {
                my = nullptr;
                if (avk_ctx_create(devices[w], &my)) {
                    worker_err[w] = std::string("cannot create the GPU context: ") + avk_last_error(nullptr);
                    return;
                }
                w_ctx[w] = my;
                const uint32_t n_contigs = avf_genome_n_contigs(genome);
                std::vector<const uint8_t *> seqs(n_contigs);
                std::vector<uint64_t> lens(n_contigs);
                for (uint32_t c = 0; c < n_contigs; ++c) seqs[c] = avf_genome_seq(genome, c), lens[c] = avf_genome_len(genome, c);
                if (avk_ref_upload(my, n_contigs, seqs.data(), lens.data())) { /* the reference is replicated: 0.8 GB packed per rank */
                    worker_err[w] = std::string("reference upload failed: ") + avk_last_error(my);
                    return;
                }
                (void)avk_ctx_set_option(my, "emit_group_metrics", 0);
            }
            avk_packed_shard *shard = nullptr;
            if (avk_packed_shard_make_esc(&sel, &sel_esc, all->region_id + first, 0, (uint32_t)w, (uint32_t)n_workers, &shard)) worker_err[w] = "cannot cut the shard";
            else {
                const avk_packed_batch *sb = avk_packed_shard_batch(shard);
                std::vector<int32_t> s_status(sb->n_regions + 1);
                std::vector<uint8_t> s_e(sb->n_variants + 1), s_o(sb->n_variants + 1), s_c(sb->n_variants + 1);
                avk_result_batch so;
                memset(&so, 0, sizeof(so));
                so.status = s_status.data(), so.var_expected = s_e.data(), so.var_observed = s_o.data(), so.var_class = s_c.data(), so.tally = w_total[w].data();
                if (avk_compare_packed_esc(my, sb, avk_packed_shard_escapes(shard), &cfg, &so)) worker_err[w] = std::string("compare failed: ") + avk_last_error(my);
                else {
                    avk_result_batch to; /* the selected regions' part of the job's arrays: regions from `first`, calls from the selection's first call */
                    memset(&to, 0, sizeof(to));
                    to.status = status.data() + first, to.var_expected = var_expected.data() + sel_v, to.var_observed = var_observed.data() + sel_v, to.var_class = var_class.data() + sel_v;
                    (void)avk_packed_shard_scatter(shard, &so, &to);
                    const uint64_t *idx = nullptr;
                    const uint64_t m = avk_packed_shard_regions(shard, &idx);
                    for (uint64_t k = 0; k < m; ++k)
                        if (s_status[k] != 0) {
                            std::lock_guard<std::mutex> lock(log_mutex);
                            avk_region_batch b1 = *all;
                            b1.region_id = all->region_id + first, b1.contig_idx = all->contig_idx + first, b1.start = all->start + first, b1.end = all->end + first;
                            b1.t_off = all->t_off + first, b1.t_cnt = all->t_cnt + first, b1.q_off = all->q_off + first, b1.q_cnt = all->q_cnt + first;
                            report_unsolved(b1, idx[k], s_status[k]);
                        }
                }
                avk_packed_shard_free(shard);
            }
        };
        std::vector<std::thread> pool;
        for (size_t w = 1; w < n_workers; ++w) pool.emplace_back(shard_worker, w);
        shard_worker(0);
        for (std::thread &t : pool) t.join();
        pool.clear();
        bool all_solved = true;
        for (size_t w = 0; w < n_workers; ++w) all_solved = all_solved && worker_err[w].empty();
        /* the collective: entered only when EVERY rank has its sums — a rank that failed above never leaves the others waiting inside ncclAllReduce */
        if (all_solved && distinct) {
            std::vector<std::vector<uint64_t>> reduced = w_total;
            std::vector<std::string> reduce_err(n_workers);
            auto reduce_worker = [&](size_t w) {
                if (avk_tally_allreduce(w_ctx[w], comms[w], reduced[w].data())) reduce_err[w] = avk_last_error(w_ctx[w]);
            };
            for (size_t w = 1; w < n_workers; ++w) pool.emplace_back(reduce_worker, w);
            reduce_worker(0);
            for (std::thread &t : pool) t.join();
            for (size_t w = 0; w < n_workers; ++w)
                if (!reduce_err[w].empty()) { /* the ranks' own tallies are still there: the host sum stands in */
                    if (verbosity) fprintf(stderr, "tally all-reduce failed (%s): the ranks' tallies are summed on the host.\n", reduce_err[w].c_str());
                    distinct = false;
                    break;
                }
            if (distinct) total = reduced[0]; /* every rank holds the job's sums */
        } else if (!all_solved) distinct = false;
        for (size_t w = 0; w < n_workers; ++w) {
            if (comms[w]) {
                typedef int (*destroy_fn)(void *);
                void *h = dlopen("librccl.so", RTLD_NOW | RTLD_NOLOAD);
                destroy_fn destroy = h ? (destroy_fn)dlsym(h, "ncclCommDestroy") : nullptr;
                if (destroy) (void)destroy(comms[w]);
            }
            if (w > 0 && w_ctx[w]) avk_ctx_destroy(w_ctx[w]);
        }
        for (size_t w = 0; w < n_workers; ++w)
            if (!worker_err[w].empty()) die(70, worker_err[w].c_str(), "");
        if (!distinct)
            for (size_t w = 0; w < n_workers; ++w)
                for (size_t k = 0; k < (size_t)AVK_TALLY_LEN; ++k) total[k] += w_total[w][k];
        if (verbosity) fprintf(stderr, "%zu contexts, regions sharded by hash(region_id) %% %zu; the job tally summed %s.\n", n_workers, n_workers, distinct ? "by one RCCL all-reduce" : "on the host");
    }
    if (n_workers > 1 && !sharded) {
        if (!batch_given) { /* about two batches per context */
            batch_regions = (count + 2 * n_workers - 1) / (2 * n_workers);
            if (batch_regions < 100000) batch_regions = 100000;
        }
        const uint64_t n_batches = (count + batch_regions - 1) / batch_regions;
        std::atomic<uint64_t> next_batch{0};
        std::vector<std::string> worker_err(n_workers);
        std::vector<std::vector<uint64_t>> w_total(n_workers, std::vector<uint64_t>(AVK_TALLY_LEN, 0)),
            w_strat(n_workers, std::vector<uint64_t>((size_t)n_labels * AVK_TALLY_LEN, 0)), w_boot(n_workers, std::vector<uint64_t>(boot_total.size(), 0)),
            w_size(n_workers, std::vector<uint64_t>(size_total.size(), 0)), w_roc(n_workers, std::vector<uint64_t>(roc_total.size(), 0)),
            w_kind(n_workers, std::vector<uint64_t>(kind_total.size(), 0));
        std::mutex log_mutex;
        auto worker = [&](size_t w) {
            avk_ctx *my = ctx;
            if (w > 0) {
                my = nullptr;
                if (avk_ctx_create(devices[w], &my)) {
                    worker_err[w] = std::string("cannot create the GPU context: ") + avk_last_error(nullptr);
                    return;
                }
                const uint32_t n_contigs = avf_genome_n_contigs(genome);
                std::vector<const uint8_t *> seqs(n_contigs);
                std::vector<uint64_t> lens(n_contigs);
                for (uint32_t c = 0; c < n_contigs; ++c) {
                    seqs[c] = avf_genome_seq(genome, c);
                    lens[c] = avf_genome_len(genome, c);
                }
                if (avk_ref_upload(my, n_contigs, seqs.data(), lens.data())) {
                    worker_err[w] = std::string("reference upload failed: ") + avk_last_error(my);
                    avk_ctx_destroy(my);
                    return;
                }
                (void)avk_ctx_set_option(my, "emit_group_metrics", n_labels && !compact_labels ? 1 : 0);
                if (boot_host || size_resident || roc_resident || kind_resident) (void)avk_ctx_set_option(my, "emit_bp_groups", 1);
            }
            avk_strata *my_sets = w > 0 ? nullptr : strata;
            if (w > 0 && strata_route && cx_given && strata_upload(my, &my_sets)) { /* (context labels: no host route) */
                worker_err[w] = std::string("--context-strata: cannot upload the stratification sets: ") + avk_last_error(my);
                avk_ctx_destroy(my);
                return;
            }
            if (w > 0 && strata_route && !cx_given && strata_upload(my, &my_sets)) { /* this worker lists its batches' labels on the host */
                std::lock_guard<std::mutex> lock(log_mutex);
                fprintf(stderr, "Warning: cannot upload the stratification sets to context %zu: %s; its region labels are listed on the host.\n", w, avk_last_error(my));
                my_sets = nullptr;
                if (boot || size || roc || kind) { /* (the replicates', the size bins', the curve's and the kinds' scopes are read from the sets on the GPU) */
                    worker_err[w] = boot   ? "--bootstrap: cannot upload the stratification sets to every context"
                                    : size ? "--size-strata: cannot upload the stratification sets to every context"
                                    : roc  ? "--roc: cannot upload the stratification sets to every context"
                                           : "--kind-strata: cannot upload the stratification sets to every context";
                    avk_ctx_destroy(my);
                    return;
                }
            }
            std::vector<uint64_t> w_tally(AVK_TALLY_LEN);
            for (uint64_t bi = next_batch.fetch_add(1); bi < n_batches; bi = next_batch.fetch_add(1)) {
                const uint64_t at = bi * batch_regions;
                const uint64_t n = count - at < batch_regions ? count - at : batch_regions;
                avk_region_batch b = *all;
                b.n_regions = n;
                b.region_id = all->region_id + first + at;
                b.contig_idx = all->contig_idx + first + at;
                b.start = all->start + first + at;
                b.end = all->end + first + at;
                b.t_off = all->t_off + first + at;
                b.t_cnt = all->t_cnt + first + at;
                b.q_off = all->q_off + first + at;
                b.q_cnt = all->q_cnt + first + at;
                avk_result_batch out;
                memset(&out, 0, sizeof(out));
                out.status = status.data() + first + at;
                out.tally = w_tally.data();
                out.var_expected = var_expected.data();
                out.var_observed = var_observed.data();
                out.var_class = var_class.data();
                int rc = 0;
                HostGroups hg;
                if (boot_host) host_groups(n, out, hg);
                if (kind && packed)
                    rc = compare_part_kind(my, first + at, n, cfg, out, strata_route ? my_sets : nullptr, w_strat[w].data(), w_boot[w].data(), w_size[w].data(), w_roc[w].data(),
                                           w_kind[w].data());
                else if (roc && packed)
                    rc = compare_part_roc(my, first + at, n, cfg, out, strata_route ? my_sets : nullptr, w_strat[w].data(), w_boot[w].data(), w_size[w].data(), w_roc[w].data());
                else if (size && packed) rc = compare_part_size(my, first + at, n, cfg, out, strata_route ? my_sets : nullptr, w_strat[w].data(), w_boot[w].data(), w_size[w].data());
                else if (boot && packed) rc = compare_part_boot(my, first + at, n, cfg, out, strata_route ? my_sets : nullptr, w_strat[w].data(), w_boot[w].data());
                else if (strata_route && my_sets) rc = compare_part_strata(my, first + at, n, cfg, out, my_sets, w_strat[w].data());
                else if (n_labels) {
                    std::vector<uint64_t> label_off(n + 1, 0);
                    std::vector<uint32_t> label_idx;
                    rc = avf_strat_batch_labels(strat, genome, all, first + at, n, label_off.data(), nullptr);
                    if (!rc) {
                        label_idx.resize(label_off[n] + 1);
                        rc = avf_strat_batch_labels(strat, genome, all, first + at, n, label_off.data(), label_idx.data());
                    }
                    if (rc) {
                        worker_err[w] = std::string("cannot list the region labels: ") + avf_last_error();
                        break;
                    }
                    if (compact_labels) rc = compare_part_labels(my, first + at, n, cfg, out, n_labels, label_off.data(), label_idx.data(), w_strat[w].data());
                    else {
                        avk_dev_batch *db = nullptr;
                        uint64_t v_first = 0;
                        rc = upload_part(my, b, first + at, n, &db, &v_first);
                        if (!rc) rc = avk_compare_resident(my, db, &cfg, nullptr);
                        avk_result_batch shifted = out_for(out, v_first);
                        if (!rc) rc = avk_results_download(my, db, &shifted);
                        if (!rc) rc = avk_label_tallies(my, db, n_labels, label_off.data(), label_idx.data(), w_strat[w].data());
                        if (db) avk_batch_free(my, db);
                        if (!rc && boot_host && boot_part_host(b, out, label_off.data(), label_idx.data(), w_boot[w].data())) {
                            worker_err[w] = std::string("bootstrap tallies failed: ") + avk_last_error(nullptr);
                            break;
                        }
                        if (!rc && size_host && size_part_host(b, out, label_off.data(), label_idx.data(), w_size[w].data())) {
                            worker_err[w] = std::string("size-bin tallies failed: ") + avk_last_error(nullptr);
                            break;
                        }
                        if (!rc && roc_host && roc_part_host(b, out, label_off.data(), label_idx.data(), w_roc[w].data())) {
                            worker_err[w] = std::string("score curve failed: ") + avk_last_error(nullptr);
                            break;
                        }
                        if (!rc && kind_host && kind_part_host(b, out, label_off.data(), label_idx.data(), w_kind[w].data())) {
                            worker_err[w] = std::string("call-kind tallies failed: ") + avk_last_error(nullptr);
                            break;
                        }
                    }
                } else {
                    rc = compare_part(my, b, first + at, n, cfg, out);
                    if (!rc && boot_host && boot_part_host(b, out, nullptr, nullptr, w_boot[w].data())) {
                        worker_err[w] = std::string("bootstrap tallies failed: ") + avk_last_error(nullptr);
                        break;
                    }
                    if (!rc && size_host && size_part_host(b, out, nullptr, nullptr, w_size[w].data())) {
                        worker_err[w] = std::string("size-bin tallies failed: ") + avk_last_error(nullptr);
                        break;
                    }
                    if (!rc && roc_host && roc_part_host(b, out, nullptr, nullptr, w_roc[w].data())) {
                        worker_err[w] = std::string("score curve failed: ") + avk_last_error(nullptr);
                        break;
                    }
                    if (!rc && kind_host && kind_part_host(b, out, nullptr, nullptr, w_kind[w].data())) {
                        worker_err[w] = std::string("call-kind tallies failed: ") + avk_last_error(nullptr);
                        break;
                    }
                }
                if (rc) {
                    worker_err[w] = std::string("compare failed: ") + avk_last_error(my);
                    break;
                }
                for (size_t k = 0; k < (size_t)AVK_TALLY_LEN; ++k) w_total[w][k] += w_tally[k];
                for (uint64_t r = 0; r < n; ++r)
                    if (out.status[r] != 0) {
                        std::lock_guard<std::mutex> lock(log_mutex);
                        report_unsolved(b, r, out.status[r]);
                    }
            }
            if (w > 0) {
                avk_strata_free(my, my_sets);
                avk_ctx_destroy(my);
            }
        };
        std::vector<std::thread> pool;
        for (size_t w = 1; w < n_workers; ++w) pool.emplace_back(worker, w);
        worker(0);
        for (std::thread &t : pool) t.join();
        for (size_t w = 0; w < n_workers; ++w)
            if (!worker_err[w].empty()) die(70, worker_err[w].c_str(), "");
        for (size_t w = 0; w < n_workers; ++w) {
            for (size_t k = 0; k < (size_t)AVK_TALLY_LEN; ++k) total[k] += w_total[w][k];
            for (size_t k = 0; k < strat_total.size(); ++k) strat_total[k] += w_strat[w][k];
            for (size_t k = 0; k < boot_total.size(); ++k) boot_total[k] += w_boot[w][k]; /* the contexts' blocks, added on the host */
            for (size_t k = 0; k < size_total.size(); ++k) size_total[k] += w_size[w][k];
            for (size_t k = 0; k < roc_total.size(); ++k) roc_total[k] += w_roc[w][k];
            for (size_t k = 0; k < kind_total.size(); ++k) kind_total[k] += w_kind[w][k];
        }
    }
    for (uint64_t at = 0; n_workers == 1 && at < count; at += batch_regions) {
        const uint64_t n = count - at < batch_regions ? count - at : batch_regions;
        avk_region_batch b = *all; /* a window of the region arrays; variant arrays are shared */
        b.n_regions = n;
        b.region_id = all->region_id + first + at;
        b.contig_idx = all->contig_idx + first + at;
        b.start = all->start + first + at;
        b.end = all->end + first + at;
        b.t_off = all->t_off + first + at;
        b.t_cnt = all->t_cnt + first + at;
        b.q_off = all->q_off + first + at;
        b.q_cnt = all->q_cnt + first + at;
        avk_result_batch out;
        memset(&out, 0, sizeof(out));
        out.status = status.data() + first + at;
        out.tally = tally.data();
        out.var_expected = var_expected.data(); /* indexed by the (shared) variant arrays */
        out.var_observed = var_observed.data();
        out.var_class = var_class.data();
        if (debug) {
            gm.resize((size_t)n * AVK_N_GROUPS * AVK_N_FIELDS);
            out.group_metrics = gm.data();
        }
        if (debug) {
            seq_off.resize(n);
            seq_stride.resize(n);
            seq_len.assign(5 * n, 0);
            uint64_t total_seq = 0;
            for (uint64_t r = 0; r < n; ++r) {
                seq_stride[r] = avk_seq_stride(&b, r);
                seq_off[r] = total_seq;
                total_seq += 5ull * seq_stride[r];
            }
            seq_bytes.resize(total_seq + 16);
            out.seq_bytes = seq_bytes.data();
            out.seq_off = seq_off.data();
            out.seq_stride = seq_stride.data();
            out.seq_len = seq_len.data();
        }
        HostGroups hg;
        if (boot_host) host_groups(n, out, hg);
        if (kind && packed) { /* the kinds with the results (and, on the resident batch, every other sum asked for) */
            if (compare_part_kind(ctx, first + at, n, cfg, out, strata_route ? strata : nullptr, strat_total.data(), boot_total.data(), size_total.data(), roc_total.data(),
                                  kind_total.data()))
                die(70, "compare failed", avk_last_error(ctx));
        } else if (roc && packed) { /* the curve with the results (and, on the resident batch, the labels' sums, the replicates and the size blocks) */
            if (compare_part_roc(ctx, first + at, n, cfg, out, strata_route ? strata : nullptr, strat_total.data(), boot_total.data(), size_total.data(), roc_total.data()))
                die(70, "compare failed", avk_last_error(ctx));
        } else if (size && packed) { /* the size blocks with the results (and, on the resident batch, the labels' sums and the replicates) */
            if (compare_part_size(ctx, first + at, n, cfg, out, strata_route ? strata : nullptr, strat_total.data(), boot_total.data(), size_total.data()))
                die(70, "compare failed", avk_last_error(ctx));
        } else if (boot && packed) { /* the one call that also returns the replicates (with the sets' handle: the labels' sums and scopes) */
            if (compare_part_boot(ctx, first + at, n, cfg, out, strata_route ? strata : nullptr, strat_total.data(), boot_total.data())) die(70, "compare failed", avk_last_error(ctx));
        } else if (strata_route) { /* one call: the batch goes in, the sums come back with the results; the lists never exist on the host */
            if (compare_part_strata(ctx, first + at, n, cfg, out, strata, strat_total.data())) die(70, "compare failed", avk_last_error(ctx));
        } else if (compact_labels) { /* one call: the lists go in with the batch, the sums come back with the results */
            std::vector<uint64_t> label_off(n + 1, 0);
            std::vector<uint32_t> label_idx;
            int rc_labels = avf_strat_batch_labels(strat, genome, all, first + at, n, label_off.data(), nullptr);
            if (!rc_labels) {
                label_idx.resize(label_off[n] + 1);
                rc_labels = avf_strat_batch_labels(strat, genome, all, first + at, n, label_off.data(), label_idx.data());
            }
            if (rc_labels) die(70, "cannot list the region labels", avf_last_error());
            if (compare_part_labels(ctx, first + at, n, cfg, out, n_labels, label_off.data(), label_idx.data(), strat_total.data())) die(70, "compare failed", avk_last_error(ctx));
        } else if (device_labels) {
            std::vector<uint64_t> label_off(n + 1, 0);
            std::vector<uint32_t> label_idx;
            int rc_labels = 0;
            std::thread th_labels([&] { /* beside the upload and the kernels */
                rc_labels = avf_strat_batch_labels(strat, genome, all, first + at, n, label_off.data(), nullptr);
                if (!rc_labels) {
                    label_idx.resize(label_off[n] + 1);
                    rc_labels = avf_strat_batch_labels(strat, genome, all, first + at, n, label_off.data(), label_idx.data());
                }
            });
            avk_dev_batch *db = nullptr;
            uint64_t v_first = 0;
            int rc = upload_part(ctx, b, first + at, n, &db, &v_first);
            if (!rc) rc = avk_compare_resident(ctx, db, &cfg, nullptr);
            avk_result_batch shifted = out_for(out, v_first);
            if (!rc) rc = avk_results_download(ctx, db, &shifted);
            th_labels.join();
            if (rc) die(70, "compare failed", avk_last_error(ctx));
            if (rc_labels) die(70, "cannot list the region labels", avf_last_error());
            if (avk_label_tallies(ctx, db, n_labels, label_off.data(), label_idx.data(), strat_total.data())) die(70, "stratified tallies failed", avk_last_error(ctx));
            avk_batch_free(ctx, db);
            if (boot_host && boot_part_host(b, out, label_off.data(), label_idx.data(), boot_total.data())) die(70, "bootstrap tallies failed", avk_last_error(nullptr));
            if (size_host && size_part_host(b, out, label_off.data(), label_idx.data(), size_total.data())) die(70, "size-bin tallies failed", avk_last_error(nullptr));
            if (roc_host && roc_part_host(b, out, label_off.data(), label_idx.data(), roc_total.data())) die(70, "score curve failed", avk_last_error(nullptr));
            if (kind_host && kind_part_host(b, out, label_off.data(), label_idx.data(), kind_total.data())) die(70, "call-kind tallies failed", avk_last_error(nullptr));
        } else {
            if (compare_part(ctx, b, first + at, n, cfg, out)) die(70, "compare failed", avk_last_error(ctx));
            if (boot_host && boot_part_host(b, out, nullptr, nullptr, boot_total.data())) die(70, "bootstrap tallies failed", avk_last_error(nullptr));
            if (size_host && size_part_host(b, out, nullptr, nullptr, size_total.data())) die(70, "size-bin tallies failed", avk_last_error(nullptr));
            if (roc_host && roc_part_host(b, out, nullptr, nullptr, roc_total.data())) die(70, "score curve failed", avk_last_error(nullptr));
            if (kind_host && kind_part_host(b, out, nullptr, nullptr, kind_total.data())) die(70, "call-kind tallies failed", avk_last_error(nullptr));
        }
        for (size_t k = 0; k < (size_t)AVK_TALLY_LEN; ++k) total[k] += tally[k];
        if (debug && (avf_region_summary_rows(region_table, genome, all, first + at, n, out.status, gm.data()) ||
                      avf_region_sequences_rows(sequence_table, genome, all, first + at, n, out.status, seq_bytes.data(), seq_len.data(), seq_off.data(),
                                                seq_stride.data())))
            die(74, "Error while writing the debug tables", avf_last_error());
        for (uint64_t r = 0; n_labels && !device_labels && r < n; ++r) { /* debug runs: the blocks are on the host anyway */
            if (out.status[r] != 0) continue;
            const uint32_t hit = avf_strat_region_labels(strat, genome, all, first + at + r, labels.data(), n_labels);
            const uint32_t *block = gm.data() + (size_t)r * AVK_N_GROUPS * AVK_N_FIELDS;
            for (uint32_t h = 0; h < hit; ++h) {
                uint64_t *dst = strat_total.data() + (size_t)labels[h] * AVK_TALLY_LEN;
                for (int k = 0; k < AVK_N_GROUPS * AVK_N_FIELDS; ++k) dst[k] += block[k];
            }
        }
        for (uint64_t r = 0; r < n; ++r)
            if (out.status[r] != 0) report_unsolved(b, r, out.status[r]);
    }
    const double s_solve = seconds_since(t0);

    t0 = std::chrono::steady_clock::now();
    if (avf_table_close(region_table) || avf_table_close(sequence_table)) die(74, "Error while saving the debug tables", avf_last_error());
    const std::string summary = out_dir + "/summary.tsv";
    if (cx_given) { /* the sets' blocks, then the derived blocks, in label order */
        std::vector<std::string> label_names;
        for (uint32_t l = 0; l < n_bed_labels; ++l) label_names.push_back(avf_strat_label(strat, l));
        for (uint32_t j = 0; j < n_ctx_labels; ++j) {
            char name[64];
            if (avk_context_label_name(&cx_spec, j, name, sizeof(name))) die(70, "context label name", avk_last_error(nullptr));
            label_names.push_back(name);
        }
        std::vector<const char *> name_ptrs;
        for (const std::string &n : label_names) name_ptrs.push_back(n.c_str());
        if (avf_write_summary_named(summary.c_str(), label.c_str(), total.data(), n_labels, name_ptrs.data(), strat_total.data(), mask))
            die(74, "Error while saving summary file", avf_last_error());
    } else if (avf_write_summary_stratified(summary.c_str(), label.c_str(), total.data(), strat, strat_total.data(), mask))
        die(74, "Error while saving summary file", avf_last_error());
    if (boot) { /* summary_ci.tsv: summary.tsv's rows with the replicates' percentile intervals */
        std::vector<std::string> ci_names;
        for (uint32_t l = 0; l < n_bed_labels; ++l) ci_names.push_back(avf_strat_label(strat, l));
        for (uint32_t j = 0; j < n_ctx_labels; ++j) {
            char name[64];
            if (avk_context_label_name(&cx_spec, j, name, sizeof(name))) die(70, "context label name", avk_last_error(nullptr));
            ci_names.push_back(name);
        }
        std::vector<const char *> ci_ptrs;
        for (const std::string &n : ci_names) ci_ptrs.push_back(n.c_str());
        if (avf_write_summary_ci((out_dir + "/summary_ci.tsv").c_str(), label.c_str(), total.data(), n_labels, ci_ptrs.data(), strat_total.data(), mask, boot_spec.replicates,
                                 boot_total.data(), boot_level))
            die(74, "Error while saving summary_ci.tsv", avf_last_error());
    }
    if (size) { /* summary_size.tsv: summary.tsv's GT / HAP / WEIGHTED_HAP rows per scope and size bin */
        std::vector<std::string> sz_names, bin_names;
        for (uint32_t l = 0; l < n_bed_labels; ++l) sz_names.push_back(avf_strat_label(strat, l));
        for (uint32_t j = 0; j < n_ctx_labels; ++j) {
            char name[64];
            if (avk_context_label_name(&cx_spec, j, name, sizeof(name))) die(70, "context label name", avk_last_error(nullptr));
            sz_names.push_back(name);
        }
        for (uint32_t j = 0; j < size_bins; ++j) {
            char name[64];
            if (avk_size_bin_name(&size_spec, j, name, sizeof(name))) die(70, "size bin name", avk_last_error(nullptr));
            bin_names.push_back(name);
        }
        std::vector<const char *> sz_ptrs, bin_ptrs;
        for (const std::string &n : sz_names) sz_ptrs.push_back(n.c_str());
        for (const std::string &n : bin_names) bin_ptrs.push_back(n.c_str());
        if (avf_write_summary_size((out_dir + "/summary_size.tsv").c_str(), label.c_str(), size_bins, bin_ptrs.data(), n_labels, sz_ptrs.data(), size_total.data(), mask))
            die(74, "Error while saving summary_size.tsv", avf_last_error());
        if (pcb) { /* summary_size_ci.tsv: the same rows with the replicates' percentile intervals; the contexts' (workers') blocks are added here, on the host */
            std::vector<uint64_t> reps(((size_t)n_labels + 1) * boot_spec.replicates * size_bins * AVK_CALLBOOT_KEY_WORDS, 0);
            for (const auto &kv : pcb_bufs)
                for (size_t k = 0; k < kv.second.size_reps.size(); ++k) reps[k] += kv.second.size_reps[k];
            if (avf_write_summary_size_ci((out_dir + "/summary_size_ci.tsv").c_str(), label.c_str(), size_bins, bin_ptrs.data(), n_labels, sz_ptrs.data(), size_total.data(), mask,
                                          boot_spec.replicates, reps.data(), boot_level))
                die(74, "Error while saving summary_size_ci.tsv", avf_last_error());
        }
    }
    if (kind) { /* summary_kind.tsv: summary.tsv's GT / HAP / WEIGHTED_HAP rows per scope and call kind; kind_ratios.tsv: their Ti/Tv and het/hom */
        std::vector<std::string> kd_names;
        for (uint32_t l = 0; l < n_bed_labels; ++l) kd_names.push_back(avf_strat_label(strat, l));
        for (uint32_t j = 0; j < n_ctx_labels; ++j) {
            char name[64];
            if (avk_context_label_name(&cx_spec, j, name, sizeof(name))) die(70, "context label name", avk_last_error(nullptr));
            kd_names.push_back(name);
        }
        std::vector<const char *> kd_ptrs;
        for (const std::string &n : kd_names) kd_ptrs.push_back(n.c_str());
        if (avf_write_summary_kind((out_dir + "/summary_kind.tsv").c_str(), label.c_str(), n_labels, kd_ptrs.data(), kind_total.data(), mask))
            die(74, "Error while saving summary_kind.tsv", avf_last_error());
        if (avf_write_kind_ratios((out_dir + "/kind_ratios.tsv").c_str(), label.c_str(), n_labels, kd_ptrs.data(), kind_total.data()))
            die(74, "Error while saving kind_ratios.tsv", avf_last_error());
        if (pcb) { /* summary_kind_ci.tsv and kind_ratios_ci.tsv, likewise */
            std::vector<uint64_t> reps(((size_t)n_labels + 1) * boot_spec.replicates * AVK_N_KINDS * AVK_CALLBOOT_KEY_WORDS, 0);
            for (const auto &kv : pcb_bufs)
                for (size_t k = 0; k < kv.second.kind_reps.size(); ++k) reps[k] += kv.second.kind_reps[k];
            if (avf_write_summary_kind_ci((out_dir + "/summary_kind_ci.tsv").c_str(), label.c_str(), n_labels, kd_ptrs.data(), kind_total.data(), mask, boot_spec.replicates, reps.data(),
                                          boot_level))
                die(74, "Error while saving summary_kind_ci.tsv", avf_last_error());
            if (avf_write_kind_ratios_ci((out_dir + "/kind_ratios_ci.tsv").c_str(), label.c_str(), n_labels, kd_ptrs.data(), kind_total.data(), boot_spec.replicates, reps.data(), boot_level))
                die(74, "Error while saving kind_ratios_ci.tsv", avf_last_error());
        }
    }
    if (roc) { /* summary_roc.tsv: summary.tsv's GT / HAP / WEIGHTED_HAP rows per scope and point of the curve */
        std::vector<std::string> sc_names, point_names;
        for (uint32_t l = 0; l < n_bed_labels; ++l) sc_names.push_back(avf_strat_label(strat, l));
        for (uint32_t j = 0; j < n_ctx_labels; ++j) {
            char name[64];
            if (avk_context_label_name(&cx_spec, j, name, sizeof(name))) die(70, "context label name", avk_last_error(nullptr));
            sc_names.push_back(name);
        }
        for (uint32_t k = 0; k < roc_points; ++k) {
            char name[64];
            if (avk_score_point_name(&roc_spec, k, name, sizeof(name))) die(70, "score point name", avk_last_error(nullptr));
            point_names.push_back(name);
        }
        std::vector<const char *> sc_ptrs, point_ptrs;
        for (const std::string &n : sc_names) sc_ptrs.push_back(n.c_str());
        for (const std::string &n : point_names) point_ptrs.push_back(n.c_str());
        if (avf_write_summary_roc((out_dir + "/summary_roc.tsv").c_str(), label.c_str(), roc_points, point_ptrs.data(), n_labels, sc_ptrs.data(), roc_total.data(), mask))
            die(74, "Error while saving summary_roc.tsv", avf_last_error());
    }
    /* the annotated VCFs (VariantCategorizer): truth.vcf.gz and query.vcf.gz with their .tbi */
    std::string command;
    for (int i = 0; i < argc; ++i) command += (i ? " " : "") + std::string(argv[i]);
    const char *in_vcf[2] = {truth.c_str(), query.c_str()}, *samples[2] = {truth_sample.c_str(), query_sample.c_str()}, *names[2] = {"/truth.vcf.gz", "/query.vcf.gz"};
    {
        int rcs[2] = {0, 0};
        std::string errs[2];
        auto write_one = [&](int src) {
            rcs[src] = avf_write_annotated_vcf((out_dir + names[src]).c_str(), in_vcf[src], samples[src], avk_version(), command.c_str(), genome, all, src,
                                               status.data(), var_expected.data(), var_observed.data(), var_class.data());
            if (rcs[src]) errs[src] = avf_last_error(); /* the error text is per thread */
        };
        std::thread other(write_one, 1);
        write_one(0);
        other.join();
        for (int src = 0; src < 2; ++src)
            if (rcs[src]) die(74, "Error while saving output files", errs[src].c_str());
    }
    const double s_write = seconds_since(t0);

    fprintf(stderr, "Solved:error blocks: %llu : %llu\n", (unsigned long long)total[AVK_TALLY_LEN - 2], (unsigned long long)total[AVK_TALLY_LEN - 1]);
    fprintf(stderr, "stages [s]: load %.3f (side by side: reference %.3f, truth calls %.3f, query calls %.3f, gpu context %.3f), regions %.3f (beside it: reference upload %.3f), "
                    "solve (pack + H2D + kernels + D2H) %.3f, summary + annotated VCFs %.3f\n",
            s_load, s_genome, s_calls[0], s_calls[1], s_ctx, s_feed, s_ref, s_solve, s_write);
    fprintf(stderr, "Comparisons completed in %.3f seconds (%.2f M regions/s in the solve stage).\n", seconds_since(t_start),
            s_solve > 0 ? (double)count / s_solve / 1e6 : 0.0);
    th_free.join();
    avk_strata_free(ctx, strata);
    avk_ctx_destroy(ctx);
    avf_feed_free(feed);
    avf_strat_free(strat);
    avf_genome_free(genome);
    return 0;
}
