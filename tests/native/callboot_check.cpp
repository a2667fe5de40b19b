/*
 * callboot_check.cpp — the per-call bootstrap's lane functions (aardvark_amd/csrc/avk_callboot.inl) under AddressSanitizer and UBSan, as a program of its own: every
 * array the lanes may read or write — the batch's, the results', the alleles, the masks, the workgroup's LDS, the sums — is a heap block EXACTLY as long as the
 * kernel's launch makes it, so a read or write one element past any of them stops the program.  The launches are driven as avk_callboot_tally_kernel drives them
 * (tests/emu/callboot_emu.cpp), for both families, region counts around the tile, replicate counts around a launch's, a region of more calls than a piece holds, and
 * scopes in two mask words; the sums are compared with a plain restatement: avk_boot_weight times what sz_lane_call / ck_lane_call give, call by call.
 *
 * The HOST ROUTES' own code runs here too: avk_size_boot_tallies_host / avk_kind_boot_tallies_host are argument checks around callboot_host_sum of
 * aardvark_amd/csrc/avk_callboot_host.h, which has no GPU call and is included here — a tiny wide batch on exact heap blocks, with label lists (a label named twice,
 * a region without labels), 1 and 5 threads, against a direct restatement with avk_boot_weight.
 *
 * Built and run by tests/test_callboot_native.py; never loaded into Python.  (The rule's header alone is compiled as C by the same test.)
 */
#define AVK_EMU 1
#include <stdio.h>
#include <string.h>

#include <memory>

#include "../../aardvark_amd/csrc/avk_callboot.inl"
#include "../../aardvark_amd/csrc/avk_callboot_host.h"

typedef uint8_t u8;
typedef uint32_t u32;
typedef uint64_t u64;

template <class T> static std::unique_ptr<T[]> exact(size_t n) { /* (a zero-length block is still a block of its own: reading it is an error) */
    std::unique_ptr<T[]> p(new T[n]);
    if (n) memset((void *)p.get(), 0, n * sizeof(T));
    return p;
}

static u64 rng_state = 0x9E3779B97F4A7C15ull;
static u32 rnd(u32 n) {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (u32)(rng_state >> 33) % n;
}

static int check(u32 n, u32 B, u32 R, u32 cap, u32 n_labels, u32 grid, u64 seed, int family, u32 n_edges) {
    avk_size_spec spec;
    memset(&spec, 0, sizeof(spec));
    spec.n_edges = n_edges;
    for (u32 k = 0; k < n_edges; ++k) spec.edges[k] = 1 + 2 * k;
    const u32 n_keys = avk_callboot_n_keys(family, &spec);
    /* the batch: 0 .. 4 calls a side, region 1 with 300 + 255 calls, types 0 .. 12 (12: beyond the table), a few unsolved regions, one region without calls */
    auto t_cnt = exact<u32>(n), q_cnt = exact<u32>(n), contig = exact<u32>(n), v_off = exact<u32>(n), region_out = exact<u32>(4 * (size_t)n);
    auto t_off = exact<u64>(n), q_off = exact<u64>(n), start = exact<u64>(n);
    u64 nv = 0;
    for (u32 r = 0; r < n; ++r) {
        t_cnt[r] = r == 2 ? 0 : r == 1 ? 300 : rnd(5), q_cnt[r] = r == 2 ? 0 : r == 1 ? 255 : rnd(5);
        t_off[r] = nv, q_off[r] = nv + t_cnt[r], v_off[r] = (u32)nv;
        nv += t_cnt[r] + q_cnt[r];
        contig[r] = rnd(3), start[r] = 1000 + 977ull * r + ((u64)(r & 1) << 31);
        region_out[4 * r] = r % 11 == 7 ? 21u : 0u;
    }
    auto var_type = exact<u8>(nv), var_zyg = exact<u8>(nv);
    auto a0_len = exact<u32>(nv), a1_len = exact<u32>(nv), var_out = exact<u32>(nv);
    auto a0_off = exact<u64>(nv), a1_off = exact<u64>(nv);
    std::unique_ptr<avk::dp::DpVarInfo[]> vinfo(new avk::dp::DpVarInfo[nv ? nv : 1]);
    u64 na = 0;
    for (u64 v = 0; v < nv; ++v) {
        var_type[v] = (u8)rnd(13), var_zyg[v] = (u8)rnd(8), a0_len[v] = rnd(3) ? 1 : 1 + rnd(9), a1_len[v] = rnd(3) ? 1 : 1 + rnd(9);
        a0_off[v] = na, a1_off[v] = na + a0_len[v], na += a0_len[v] + a1_len[v];
        const u32 e = rnd(3), o = rnd(3); /* (observed may exceed expected: the difference wraps as a 32-bit word, by the rule) */
        var_out[v] = e | o << 8;
        memset((void *)&vinfo[v], 0, sizeof(vinfo[v]));
        vinfo[v].alt_ed = 1 + rnd(12);
    }
    auto alleles = exact<u8>(na);
    for (u64 k = 0; k < na; ++k) alleles[k] = (u8) "ACGTacgtN"[rnd(9)];
    const u32 n_words = (n_labels + 31) / 32;
    auto mask = exact<u32>((size_t)n_words * n);
    for (u32 l = 0; l < n_labels; ++l)
        for (u32 r = 0; r < n; ++r)
            if (l == 0 || (l != 1 && rnd(3) == 0)) mask[avk::sx::sx_mask_at(l >> 5, r, n)] |= 1u << (l & 31); /* label 0: every region; label 1: none */

    avk::lb::LbView v;
    memset((void *)&v, 0, sizeof(v));
    v.in.n_regions = n, v.in.n_variants = nv;
    v.in.contig_idx = contig.get(), v.in.start = start.get(), v.in.t_off = t_off.get(), v.in.q_off = q_off.get(), v.in.t_cnt = t_cnt.get(), v.in.q_cnt = q_cnt.get();
    v.in.var_type = var_type.get(), v.in.var_zyg = var_zyg.get(), v.in.a0_len = a0_len.get(), v.in.a1_len = a1_len.get();
    v.in.a0_off = a0_off.get(), v.in.a1_off = a1_off.get(), v.in.alleles = alleles.get(), v.in.alleles_len = na;
    v.vinfo = vinfo.get(), v.region_out = region_out.get(), v.var_out = var_out.get(), v.v_off = v_off.get();

    const size_t rep_words = (size_t)n_keys * AVK_CALLBOOT_KEY_WORDS, words = ((size_t)n_labels + 1) * B * rep_words;
    auto out = exact<u64>(words), want = exact<u64>(words);
    /* the launches */
    const u32 n_tiles = (n + AVK_CB_TILE - 1) / AVK_CB_TILE;
    const u64 seed_mix = avk_boot_mix(seed), acc_words = AVK_CB_ACC_WORDS(n_keys, R);
    auto add = [](u64 *p, u64 x) { *p += x; };
    for (u32 scope = 0; scope <= n_labels; ++scope)
        for (u32 lo = 0; lo < B; lo += R) {
            const u32 hi = B - lo > R ? lo + R : B;
            for (u32 wg = 0; wg < grid; ++wg) {
                auto lds = exact<u64>((AVK_CB_LDS_BYTES(n_keys, R) + 7) / 8); /* the workgroup's LDS, as long as the launch makes it */
                const avk::cb::CbTile t = avk::cb::cb_tile_at((unsigned char *)lds.get(), n_keys, R);
                for (u32 tile = wg; tile < n_tiles; tile += grid) {
                    u32 any = 0;
                    for (u32 tid = 0; tid < AVK_CB_TILE; ++tid) any |= avk::cb::cb_stage_region(v, (u64)tile * AVK_CB_TILE + tid, n, mask.get(), scope, seed_mix, tid, t);
                    if (!any) continue;
                    const u32 total = avk::cb::cb_ranges(t);
                    for (u32 e = 0; e < AVK_CB_TILE * R; ++e) avk::cb::cb_weight_entry(t, e, R, lo, hi);
                    for (u32 piece = 0; piece < total; piece += cap) {
                        for (u32 tid = 0; tid < cap; ++tid)
                            if (piece + tid < total) avk::cb::cb_stage_record(v, t, family, spec, piece + tid, tid);
                        for (u32 tid = 0; tid < AVK_CB_THREADS; ++tid)
                            if (tid / R < AVK_CB_SLOTS) avk::cb::cb_lane_piece(t, piece, cap, R, tid % R, tid / R);
                    }
                }
                for (u64 q = 0; q < acc_words; ++q) avk::cb::cb_flush_word(t, q, R, n_keys, scope, B, lo, hi, out.get(), add);
            }
        }
    /* the restatement */
    for (u32 r = 0; r < n; ++r) {
        if (region_out[4 * r] != 0) continue;
        const avk::sz::SzLane L = avk::sz::sz_lane_begin(v, r, n, nullptr, 0, 1);
        for (u32 i = 0; i < L.n; ++i) {
            u32 key = 0;
            const avk::lb::LbCall c = family == AVK_CALLBOOT_KIND ? avk::ck::ck_lane_call(v, L, i, key) : avk::sz::sz_lane_call(v, L, i, spec, key);
            const u32 val[AVK_SIZE_VALUES] = {c.gt_tp, c.gt_fn, c.gt_fn_gt, c.hap_tp, c.hap_fn, c.w_tp, c.w_fn};
            const u32 vt = (key >> 4) & 15u;
            for (u32 scope = 0; scope <= n_labels; ++scope) {
                if (scope && !((mask[avk::sx::sx_mask_at((scope - 1) >> 5, r, n)] >> ((scope - 1) & 31)) & 1u)) continue;
                for (u32 b = 0; b < B; ++b) {
                    const u64 wt = avk_boot_weight(seed, contig[r], (u32)start[r], b);
                    for (u32 g : {0u, 1u + vt}) {
                        if (g >= AVK_N_GROUPS) continue;
                        for (u32 k = 0; k < AVK_SIZE_VALUES; ++k) want[AVK_CALLBOOT_AT(scope, B, b, n_keys, key & 15u, g, avk_size_field_of(k, (int)(key >> 8)))] += wt * val[k];
                    }
                }
            }
        }
    }
    if (memcmp(out.get(), want.get(), words * sizeof(u64)) != 0) {
        printf("callboot_check: sums differ (family %d, n %u, B %u, R %u, cap %u, labels %u, grid %u)\n", family, n, B, R, cap, n_labels, grid);
        return 1;
    }
    u64 some = 0;
    for (size_t k = 0; k < words; ++k) some |= out[k];
    if (!some) {
        printf("callboot_check: nothing was summed (n %u, B %u)\n", n, B);
        return 1;
    }
    return 0;
}

/* the textbook edit distance: what the library passes as Variant::alt_ed's rule */
static u64 edit_distance(const u8 *a, u64 n, const u8 *b, u64 m) {
    auto prev = exact<u64>(m + 1), cur = exact<u64>(m + 1);
    for (u64 j = 0; j <= m; ++j) prev[j] = j;
    for (u64 i = 1; i <= n; ++i) {
        cur[0] = i;
        for (u64 j = 1; j <= m; ++j) {
            u64 x = prev[j] + 1;
            if (cur[j - 1] + 1 < x) x = cur[j - 1] + 1;
            if (prev[j - 1] + (a[i - 1] != b[j - 1]) < x) x = prev[j - 1] + (a[i - 1] != b[j - 1]);
            cur[j] = x;
        }
        prev.swap(cur);
    }
    return prev[m];
}

/* callboot_host_sum on a wide batch of n regions: wide or packed per-call results, label lists, `threads` threads */
static int check_host(u32 n, u32 B, u32 n_labels, u32 threads, u64 seed, int family, u32 n_edges, bool packed_results) {
    avk_size_spec spec;
    memset(&spec, 0, sizeof(spec));
    spec.n_edges = n_edges;
    for (u32 k = 0; k < n_edges; ++k) spec.edges[k] = 1 + 2 * k;
    const u32 n_keys = avk_callboot_n_keys(family, &spec);
    auto t_cnt = exact<u32>(n), q_cnt = exact<u32>(n), contig = exact<u32>(n);
    auto t_off = exact<u64>(n), q_off = exact<u64>(n), start = exact<u64>(n);
    auto status = exact<int32_t>(n);
    auto region_packed = exact<u64>(n);
    u64 nv = 0;
    for (u32 r = 0; r < n; ++r) {
        t_cnt[r] = r == 2 ? 0 : r == 1 ? 40 : rnd(5), q_cnt[r] = r == 2 ? 0 : r == 1 ? 33 : rnd(5);
        t_off[r] = nv, q_off[r] = nv + t_cnt[r];
        nv += t_cnt[r] + q_cnt[r];
        contig[r] = rnd(3), start[r] = 1000 + 977ull * r + ((u64)(r & 1) << 31);
        status[r] = r % 11 == 7 ? 21 : 0;
        region_packed[r] = (u64)status[r];
    }
    auto var_type = exact<u8>(nv), var_zyg = exact<u8>(nv), var_expected = exact<u8>(nv), var_observed = exact<u8>(nv), var_packed = exact<u8>(nv);
    auto a0_len = exact<u32>(nv), a1_len = exact<u32>(nv);
    auto a0_off = exact<u64>(nv), a1_off = exact<u64>(nv);
    u64 na = 0;
    for (u64 v = 0; v < nv; ++v) {
        var_type[v] = (u8)rnd(13), var_zyg[v] = (u8)rnd(8), a0_len[v] = rnd(3) ? 1 : 1 + rnd(9), a1_len[v] = rnd(3) ? 1 : 1 + rnd(9);
        a0_off[v] = na, a1_off[v] = na + a0_len[v], na += a0_len[v] + a1_len[v];
        var_expected[v] = (u8)rnd(3), var_observed[v] = (u8)rnd(3);
        var_packed[v] = (u8)(var_expected[v] | var_observed[v] << 2);
    }
    auto alleles = exact<u8>(na);
    for (u64 k = 0; k < na; ++k) alleles[k] = (u8) "ACGTacgtN"[rnd(9)];
    /* the lists: region 0 names label 0 twice, region 3 has none, the others a few */
    auto label_off = exact<u64>(n + 1);
    u64 n_idx = 0;
    for (u32 r = 0; r < n; ++r) label_off[r] = n_idx, n_idx += !n_labels ? 0 : r == 0 ? 2 : r == 3 ? 0 : rnd(3);
    label_off[n] = n_idx;
    auto label_idx = exact<u32>(n_idx);
    for (u64 q = 0; q < n_idx; ++q) label_idx[q] = q < 2 ? 0 : rnd(n_labels);

    avk_region_batch b;
    memset(&b, 0, sizeof(b));
    b.n_regions = n, b.contig_idx = contig.get(), b.start = start.get(), b.t_off = t_off.get(), b.t_cnt = t_cnt.get(), b.q_off = q_off.get(), b.q_cnt = q_cnt.get();
    b.n_variants = nv, b.var_type = var_type.get(), b.var_zyg = var_zyg.get(), b.a0_off = a0_off.get(), b.a0_len = a0_len.get(), b.a1_off = a1_off.get(), b.a1_len = a1_len.get();
    b.allele_bytes = alleles.get(), b.allele_bytes_len = na;
    avk_result_batch res;
    memset(&res, 0, sizeof(res));
    if (packed_results) res.region_packed = region_packed.get(), res.var_packed = var_packed.get();
    else res.status = status.get(), res.var_expected = var_expected.get(), res.var_observed = var_observed.get();
    avk_region_labels lab;
    lab.n_labels = n_labels, lab.label_off = label_off.get(), lab.label_idx = label_idx.get();
    avk_boot_spec bs;
    bs.replicates = B, bs.seed = seed;
    if (!avk_callboot_blocks_ok((u64)n_labels + 1, B, n_keys)) return 1;

    const size_t words = ((size_t)n_labels + 1) * B * n_keys * AVK_CALLBOOT_KEY_WORDS;
    auto out = exact<u64>(words), want = exact<u64>(words);
    if (avk::cbh::callboot_host_sum(&b, &res, family, &spec, &bs, n_labels ? &lab : nullptr, threads, out.get(), edit_distance)) return 1;
    for (u32 r = 0; r < n; ++r) {
        if (status[r] != 0) continue;
        for (int side = 0; side < 2; ++side)
            for (u32 i = 0; i < (side ? q_cnt[r] : t_cnt[r]); ++i) {
                const u64 v = (side ? q_off[r] : t_off[r]) + i;
                const u64 ed = edit_distance(alleles.get() + a0_off[v], a0_len[v], alleles.get() + a1_off[v], a1_len[v]);
                const u32 exp = side ? var_observed[v] : var_expected[v], obs = side ? var_expected[v] : var_observed[v], d = exp - obs;
                const u32 val[AVK_SIZE_VALUES] = {exp == obs, exp != obs, exp != obs && obs > 0, obs, d, (u32)(obs * ed), (u32)((u64)d * ed)};
                const u32 key = family == AVK_CALLBOOT_KIND ? avk_kind_of(avk_kind_gt_of(var_zyg[v]), avk_kind_sub_of(a0_len[v], a1_len[v], alleles[a0_off[v]], alleles[a1_off[v]]))
                                                            : avk_size_bin_of(&spec, avk_size_of(a0_len[v], a1_len[v]));
                for (u32 b2 = 0; b2 < B; ++b2) {
                    const u64 wt = avk_boot_weight(seed, contig[r], (u32)start[r], b2);
                    auto add = [&](u32 scope) {
                        for (u32 g : {0u, 1u + var_type[v]}) {
                            if (g >= AVK_N_GROUPS) continue;
                            for (u32 k = 0; k < AVK_SIZE_VALUES; ++k) want[AVK_CALLBOOT_AT(scope, B, b2, n_keys, key, g, avk_size_field_of(k, side))] += wt * val[k];
                        }
                    };
                    add(0);
                    for (u64 q = label_off[r]; n_labels && q < label_off[r + 1]; ++q) add(1u + label_idx[q]);
                }
            }
    }
    u64 some = 0;
    for (size_t k = 0; k < words; ++k) some |= out[k];
    if (!some || memcmp(out.get(), want.get(), words * sizeof(u64)) != 0) {
        printf("callboot_check: host route differs (family %d, n %u, B %u, labels %u, threads %u)\n", family, n, B, n_labels, threads);
        return 1;
    }
    return 0;
}

int main() {
    const u32 T = AVK_CB_TILE, C = AVK_CB_RECS;
    const u32 ns[] = {4, T - 1, T, T + 1, 2 * T + 1};
    int bad = 0, runs = 0;
    for (int family : {AVK_CALLBOOT_KIND, AVK_CALLBOOT_SIZE}) {
        const u32 n_edges = 4, R = avk::cb::cb_reps(family == AVK_CALLBOOT_KIND ? (u32)AVK_N_KINDS : n_edges + 1, 64 * 1024 - 1024);
        for (u32 n : ns) bad += check(n, 3, R, C, 0, 2, 7 + n, family, n_edges), ++runs;
        for (u32 B : {1u, R, R + 1, 2 * R + 1}) bad += check(2 * T + 1, B, R, C, 2, 3, 100 + B, family, n_edges), ++runs;
        bad += check(T + 5, 2, 2, 7, 34, 2, 9, family, n_edges), ++runs; /* scopes in a second mask word, pieces of 7 records */
    }
    bad += check(T + 1, 3, avk::cb::cb_reps(16, 160 * 1024 - 1024), C, 1, 1, 11, AVK_CALLBOOT_SIZE, 15), ++runs; /* sixteen bins */
    bad += check(T + 1, 19, AVK_CB_REPS_MAX, C, 0, 1, 12, AVK_CALLBOOT_SIZE, 1), ++runs;                            /* two bins, every lane team */
    for (int family : {AVK_CALLBOOT_KIND, AVK_CALLBOOT_SIZE}) { /* the host routes */
        bad += check_host(40, 5, 0, 1, 21, family, 4, false), ++runs;
        bad += check_host(40, 5, 3, 1, 22, family, 4, false), ++runs;
        bad += check_host(41, 7, 3, 5, 23, family, 15, true), ++runs; /* packed results, five threads, sixteen bins */
        bad += check_host(3, 2, 1, 16, 24, family, 1, false), ++runs; /* more threads than regions */
    }
    if (bad) return 1;
    printf("callboot_check: ok (%d launches' worth of cases)\n", runs);
    return 0;
}
