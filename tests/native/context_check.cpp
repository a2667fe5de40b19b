/*
 * context_check.cpp — the lane function of aardvark_amd/csrc/avk_context.inl (the sequence-context labels of a stratified job) on the CPU, a program of its own
 * (tests/test_context_strata.py builds it with -fsanitize=address,undefined and runs it; it is never loaded into another process).
 *
 * References of several contigs with odd lengths — clean ones, ones sprinkled with N and lower-case bases, one of N only, one of a single base — packed as
 * avk_pack_reference packs them, in arrays EXACTLY as long as the reference needs (no room behind the bytes, the packed words or the flag words), so that a read
 * outside them is an error of the run.  Spans at every placement around the contigs' first and last bases, around word edges and the flag-word edge, random
 * spans, spans that reach beyond or lie outside their contig; six specs.  cx_span_bits by the 2-bit route and by the bytes alone, and the stores of
 * cx_store_region into masks exactly as long as the labels need, against a restatement of the rule written here base by base.
 */
#define AVK_EMU 1
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <string>
#include <vector>

#include "../../aardvark_amd/csrc/avk_context.inl"

using avk::cx::CxRef;
using avk::cx::CxSpec;

struct Ref {
    std::vector<std::string> contigs;
    std::vector<uint8_t> bytes;
    std::vector<uint32_t> packed, exc;
    std::vector<uint64_t> tab;
    explicit Ref(const std::vector<std::string> &c) : contigs(c) {
        const uint32_t n = (uint32_t)c.size();
        tab.assign(2 * (size_t)n, 0);
        uint64_t total = 0;
        for (uint32_t k = 0; k < n; ++k) tab[k] = total, tab[n + k] = c[k].size(), total += c[k].size();
        for (const std::string &s : c) bytes.insert(bytes.end(), s.begin(), s.end());
        const uint64_t n_words = (total + 15) >> 4;
        packed.assign(n_words, 0);
        exc.assign((n_words + 31) >> 5, 0);
        for (uint64_t p = 0; p < total; ++p) {
            const uint8_t ch = bytes[p];
            const uint32_t code = ch == 'A' ? 0u : ch == 'C' ? 1u : ch == 'G' ? 2u : ch == 'T' ? 3u : 4u;
            if (code > 3u) exc[(p >> 4) >> 5] |= 1u << ((p >> 4) & 31);
            else packed[p >> 4] |= code << (2 * (p & 15));
        }
    }
    CxRef view() const { /* (pointers into this object: made where it is used) */
        const uint32_t n = (uint32_t)contigs.size();
        CxRef v;
        v.bytes = bytes.data(), v.packed = packed.data(), v.exc = exc.data(), v.contig_base = tab.data(), v.contig_len = tab.data() + n, v.n_contigs = n;
        return v;
    }
};

/* the rule, base by base */
static uint32_t rule(const Ref &ref, const CxSpec &s, uint32_t contig, uint64_t first, uint64_t last) {
    if (contig >= ref.contigs.size()) return 0;
    const std::string &seq = ref.contigs[contig];
    uint32_t bits = 0;
    auto counts = [&](uint32_t pad, uint64_t &a, uint64_t &g, uint64_t &run) {
        a = g = run = 0;
        const uint64_t lo = first > pad ? first - pad : 0;
        uint64_t hi = last > ~0ull - 1 - pad ? ~0ull : last + 1 + pad;
        if (hi > seq.size()) hi = seq.size();
        uint64_t cur = 0;
        char prev = 0;
        for (uint64_t p = lo; p < hi; ++p) {
            const char ch = seq[p];
            if (ch != 'A' && ch != 'C' && ch != 'G' && ch != 'T') {
                prev = 0, cur = 0;
                continue;
            }
            a += 1, g += ch == 'C' || ch == 'G';
            cur = ch == prev ? cur + 1 : 1, prev = ch;
            if (cur > run) run = cur;
        }
    };
    uint64_t a, g, run;
    if (s.n_gc_edges > 1) {
        counts(s.gc_pad, a, g, run);
        for (uint32_t i = 0; a && i + 1 < s.n_gc_edges; ++i)
            if ((uint64_t)s.gc_edges[i] * a <= 100 * g && 100 * g < (uint64_t)s.gc_edges[i + 1] * a) bits |= 1u << i;
    }
    if (s.n_hp_edges) {
        counts(s.hp_pad, a, g, run);
        for (uint32_t i = 0; i < s.n_hp_edges; ++i)
            if (s.hp_edges[i] <= run && (i + 1 == s.n_hp_edges || run < s.hp_edges[i + 1])) bits |= 1u << (avk::cx::cx_n_gc_labels(s) + i);
    }
    return bits;
}

static CxSpec make_spec(uint32_t gc_pad, std::vector<uint32_t> gc, uint32_t hp_pad, std::vector<uint32_t> hp) {
    CxSpec s;
    memset(&s, 0, sizeof(s));
    s.gc_pad = gc_pad, s.hp_pad = hp_pad, s.n_gc_edges = (uint32_t)gc.size(), s.n_hp_edges = (uint32_t)hp.size();
    for (size_t i = 0; i < gc.size(); ++i) s.gc_edges[i] = gc[i];
    for (size_t i = 0; i < hp.size(); ++i) s.hp_edges[i] = hp[i];
    return s;
}

int main() {
    std::mt19937_64 rng(12345);
    auto random_seq = [&](size_t n, const char *alphabet) {
        const size_t k = strlen(alphabet);
        std::string s(n, 'A');
        for (size_t i = 0; i < n; ++i) s[i] = alphabet[rng() % k];
        return s;
    };
    const std::vector<Ref> refs = {
        Ref({random_seq(1037, "ACGT"), random_seq(531, "AACCCGGT"), random_seq(16, "ACGT")}),
        Ref({random_seq(523, "AAAACCCCGGGGTTTTNacgt"), random_seq(77, "AAAAAAAAAAAAAAAAAN"), std::string(64, 'N'), std::string("G"), random_seq(1500, "CCCCCCCCCCCCCCCCCCCCCGt")}),
        Ref({std::string(40, 'T') + std::string(40, 'C') + random_seq(7, "ACGT")}),
    };
    const std::vector<CxSpec> specs = {make_spec(50, {0, 15, 20, 25, 30, 55, 60, 65, 70, 75, 80, 85, 101}, 5, {4, 7, 12, 21}), make_spec(0, {10, 50, 90}, 7, {1, 2, 3, 5, 8, 13, 30}),
                                       make_spec(16, {0, 50, 101}, 16, {2, 9}), make_spec(1024, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 50, 99, 100, 101}, 1024,
                                                                                         {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16}),
                                       make_spec(3, {0, 101}, 0, {}), make_spec(0, {}, 0, {1})};
    uint64_t checked = 0, labelled = 0;
    for (const Ref &ref : refs)
        for (const CxSpec &spec : specs) {
            std::vector<uint32_t> all_bits;
            auto check = [&](uint32_t c, uint64_t first, uint64_t last) {
                avk::sx::SxSpan sp;
                sp.first = first, sp.last = last, sp.contig = c, sp.ok = true;
                const uint32_t want = rule(ref, spec, c, first, last), packed = avk::cx::cx_span_bits(ref.view(), spec, sp, false), bytes = avk::cx::cx_span_bits(ref.view(), spec, sp, true);
                if (packed != want || bytes != want) {
                    printf("context_check: contig %u span [%llu, %llu]: rule %#x, 2-bit route %#x, byte route %#x\n", c, (unsigned long long)first, (unsigned long long)last, want, packed, bytes);
                    exit(1);
                }
                sp.ok = false;
                if (avk::cx::cx_span_bits(ref.view(), spec, sp, false)) exit(2);
                all_bits.push_back(want), checked += 1, labelled += want != 0;
            };
            for (uint32_t c = 0; c < ref.contigs.size(); ++c) {
                const uint64_t len = ref.contigs[c].size();
                for (uint64_t first = 0; first < len && first < 70; ++first)
                    for (uint64_t span : {1, 2, 15, 16, 17, 33}) check(c, first, first + span - 1);
                for (uint64_t back = 0; back < len && back < 40; ++back)
                    for (uint64_t span : {1, 3, 16, 200}) check(c, len - 1 - back, len - 1 - back + span - 1); /* (some reach beyond the contig) */
                for (uint64_t first = 490; first < 530 && first < len; ++first) check(c, first, first + (first % 5));
                for (int k = 0; k < 300 && len; ++k) {
                    const uint64_t first = rng() % len;
                    check(c, first, first + rng() % 90);
                }
                check(c, 0, len ? len - 1 : 0), check(c, len, len + 5), check(c, len + 5000, len + 5001), check(c, 0, ~0ull), check(c, 0, ~0ull - 1), check(c, ~0ull, ~0ull);
            }
            check((uint32_t)ref.contigs.size(), 0, 10); /* a contig the reference lacks */
            /* the stores: masks of exactly the words the labels need, after the BED labels' kernel has written its own */
            const uint32_t n_ctx = avk::cx::cx_n_labels(spec);
            const uint64_t n = all_bits.size();
            for (uint32_t n_bed : {0u, 1u, 31u, 32u, 33u, 63u, 64u}) {
                const uint32_t n_words = (n_bed + n_ctx + 31u) / 32u, bed_words = (n_bed + 31u) / 32u;
                std::vector<uint32_t> mask((size_t)n_words * n, 0xDEADBEEFu);
                for (uint32_t w = 0; w < bed_words; ++w)
                    for (uint64_t r = 0; r < n; ++r) mask[avk::sx::sx_mask_at(w, r, n)] = (uint32_t)rng() & (w + 1 == bed_words && (n_bed & 31u) ? (1u << (n_bed & 31u)) - 1u : ~0u);
                const std::vector<uint32_t> before = mask;
                for (uint64_t r = 0; r < n; ++r) avk::cx::cx_store_region(mask.data(), r, n, all_bits[r], n_bed, n_ctx, n_bed == 0);
                for (uint64_t r = 0; r < n; ++r)
                    for (uint32_t l = 0; l < n_words * 32u; ++l) {
                        const bool got = (mask[avk::sx::sx_mask_at(l >> 5, r, n)] >> (l & 31u)) & 1u;
                        const bool want = l < n_bed ? (before[avk::sx::sx_mask_at(l >> 5, r, n)] >> (l & 31u)) & 1u : l - n_bed < n_ctx && ((all_bits[r] >> (l - n_bed)) & 1u);
                        if (got != want) {
                            printf("context_check: stores with %u BED labels: region %llu label %u is %d\n", n_bed, (unsigned long long)r, l, (int)got);
                            return 1;
                        }
                    }
            }
        }
    if (labelled * 4 < checked) {
        printf("context_check: only %llu of %llu spans got a label\n", (unsigned long long)labelled, (unsigned long long)checked);
        return 1;
    }
    printf("context_check: ok (%llu spans, %llu with a label)\n", (unsigned long long)checked, (unsigned long long)labelled);
    return 0;
}
