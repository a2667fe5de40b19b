/*
 * score_check.cpp — the score curve's wave code (sc_wave_tile and sc_wave_curve of aardvark_amd/csrc/avk_score.inl, with the lane functions under them) and the
 * rule's header (avk_score.h) under AddressSanitizer and UBSan, as a program of its own: every array the lanes may read or write — the batch's, the results', the
 * scores, the masks, the workgroup's block, the histograms, the curve — is a heap block EXACTLY as long as the kernels' launches make it, so a read or write one
 * element past any of them stops the program.  The launches are driven as the two kernels and their host loop drive them (tests/emu/score_emu.cpp; a wave's lanes
 * are 64 threads, tests/emu/wave_threads.h), for region counts around the wave and the tile, 1, 10 and 31 thresholds and scopes in two mask words; the curve is
 * compared with a plain restatement of the rule, point by point.  The data go beyond what a solver writes — observed above expected (values that wrap in 32 bits),
 * alt_ed in the millions (sums beyond 32 bits within one wave), types beyond the table, scores that are NaN, infinite or exactly a threshold.
 *
 * The HOST route runs here too: avk_score_host_sum of aardvark_amd/csrc/avk_score_host.h, the body of avk_score_tallies_host — the per-thread histograms, the
 * scan from bins to points, every index into the batch's and the results' arrays, the scores and the label lists — on blocks of exactly the interface's lengths,
 * with labels, several threads, both result forms (wide: status, var_expected, var_observed; packed: region_packed, var_packed) and a batch whose query calls do
 * NOT follow their truth calls, against the same restatement.  (The argument checks in front of it stay in avk_host.hip; tests/test_score_rule.py has them.)
 *
 * Built and run by tests/test_score_native.py; never loaded into Python.
 */
#define AVK_EMU 1
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <memory>

#include "../emu/wave_threads.h"

#include "../../aardvark_amd/csrc/avk_score.inl"
#include "../../aardvark_amd/csrc/avk_score_host.h"

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

static int check(u32 n, const avk_score_spec &spec, u32 n_labels, u32 grid) {
    /* the batch: 0 .. 4 calls a side, a few unsolved regions, one region without calls */
    auto t_cnt = exact<u32>(n), q_cnt = exact<u32>(n), v_off = exact<u32>(n), region_out = exact<u32>(4 * (size_t)n);
    auto t_off = exact<u64>(n), q_off = exact<u64>(n);
    u64 nv = 0;
    for (u32 r = 0; r < n; ++r) {
        t_cnt[r] = r == 2 ? 0 : rnd(5), q_cnt[r] = r == 2 ? 0 : rnd(5);
        t_off[r] = nv, q_off[r] = nv + t_cnt[r], v_off[r] = (u32)nv;
        nv += t_cnt[r] + q_cnt[r];
        region_out[4 * r] = r % 11 == 7 ? 21u : 0u;
    }
    auto var_type = exact<u8>(nv), var_zyg = exact<u8>(nv);
    auto a0_len = exact<u32>(nv), a1_len = exact<u32>(nv), var_out = exact<u32>(nv);
    auto scores = exact<float>(nv);
    std::unique_ptr<avk::dp::DpVarInfo[]> vinfo(new avk::dp::DpVarInfo[nv]);
    const u32 K = spec.n_thresholds;
    for (u64 v = 0; v < nv; ++v) {
        var_type[v] = (u8)(rnd(4) ? rnd(3) : rnd(14)), var_zyg[v] = (u8)rnd(6); /* (types 12 and 13 are beyond the table: the joint group only) */
        a0_len[v] = 1, a1_len[v] = 1 + rnd(4);
        const u32 e = rnd(3), o = rnd(16) ? rnd(e + 1) : rnd(3);
        var_out[v] = e | o << 8 | rnd(256) << 16 | rnd(256) << 24;
        memset((void *)&vinfo[v], 0, sizeof(vinfo[v]));
        vinfo[v].alt_ed = rnd(8) ? 1 + rnd(12) : 1 + rnd(90000000);
        const u32 kind = rnd(10);
        const float t = spec.t[rnd(K)];
        scores[v] = kind == 0 ? NAN : kind == 1 ? INFINITY : kind == 2 ? -INFINITY : kind == 3 ? t : kind == 4 ? nextafterf(t, -INFINITY) : kind == 5 ? nextafterf(t, INFINITY)
                                                                                                                                          : spec.t[0] - 3.0f + (float)rnd(1000) * 0.001f * (spec.t[K - 1] - spec.t[0] + 6.0f);
    }
    const u32 n_words = (n_labels + 31) / 32;
    auto mask = exact<u32>((size_t)n_words * n);
    for (u32 l = 0; l < n_labels; ++l)
        for (u32 r = 0; r < n; ++r)
            if (l == 0 || (l != 1 && rnd(3) == 0)) mask[avk::sx::sx_mask_at(l >> 5, r, n)] |= 1u << (l & 31); /* label 0: every region; label 1: none */

    avk::lb::LbView v;
    memset((void *)&v, 0, sizeof(v));
    v.in.n_regions = n, v.in.n_variants = nv;
    v.in.t_off = t_off.get(), v.in.q_off = q_off.get(), v.in.t_cnt = t_cnt.get(), v.in.q_cnt = q_cnt.get();
    v.in.var_type = var_type.get(), v.in.var_zyg = var_zyg.get(), v.in.a0_len = a0_len.get(), v.in.a1_len = a1_len.get();
    v.vinfo = vinfo.get(), v.region_out = region_out.get(), v.var_out = var_out.get(), v.v_off = v_off.get();

    const u32 n_points = K + 1, block_words = AVK_SC_BLOCK_WORDS(n_points), curve_block = AVK_SC_H_WORDS(n_points), n_scopes = 1 + n_labels;
    auto hist = exact<u64>((size_t)n_scopes * block_words);
    const size_t words = (size_t)n_scopes * curve_block;
    auto out = exact<u64>(words), want = exact<u64>(words);
    /* the launches of the histogram kernel */
    u32 per_launch = AVK_SC_LDS_BYTES / (block_words * 8u);
    if (per_launch > AVK_SC_SCOPES_MAX) per_launch = AVK_SC_SCOPES_MAX;
    const u32 n_tiles = (n + AVK_SC_THREADS - 1) / AVK_SC_THREADS;
    auto add = [](u64 *p, u64 x) { __atomic_fetch_add(p, x, __ATOMIC_RELAXED); };
    for (u32 lo = 0; lo < n_scopes; lo += per_launch) {
        const u32 hi = n_scopes - lo > per_launch ? lo + per_launch : n_scopes;
        for (u32 wg = 0; wg < grid; ++wg) {
            auto acc = exact<u64>((size_t)(hi - lo) * block_words);
            for (u32 tile = wg; tile < n_tiles; tile += grid)
                for (u32 wave = 0; wave < AVK_SC_THREADS / 64; ++wave) {
                    if ((u64)tile * AVK_SC_THREADS + wave * 64u >= n) continue; /* (a wave beyond the batch finds no call: not worth 64 threads) */
                    avk_emu::run_wave([&](int lane) {
                        avk::sc::sc_wave_tile(v, (u64)tile * AVK_SC_THREADS + wave * 64u + (u32)lane, n, n_labels ? mask.get() : nullptr, spec, scores.get(), lo, hi, acc.get(), add);
                    });
                }
            for (size_t k = 0; k < (size_t)(hi - lo) * block_words; ++k) hist[(size_t)lo * block_words + k] += acc[k];
        }
    }
    /* the curve kernel: a wave a row; every scope's blocks are handed over as blocks of their own length */
    for (u32 s = 0; s < n_scopes; ++s) {
        auto h = exact<u64>(block_words), row = exact<u64>(curve_block);
        memcpy(h.get(), hist.get() + (size_t)s * block_words, block_words * sizeof(u64));
        for (u32 g = 0; g < AVK_N_GROUPS; ++g) avk_emu::run_wave([&](int) { avk::sc::sc_wave_curve(h.get(), n_points, g, row.get()); });
        memcpy(out.get() + (size_t)s * curve_block, row.get(), curve_block * sizeof(u64));
    }
    /* the restatement: every call of every solved region at every point, in 64-bit sums of 32-bit values */
    static const u32 TF[7] = {AVK_F_GT_TRUTH_TP, AVK_F_GT_TRUTH_FN, AVK_F_GT_TRUTH_FN_GT, AVK_F_HAP_TRUTH_TP, AVK_F_HAP_TRUTH_FN, AVK_F_WHAP_TRUTH_TP, AVK_F_WHAP_TRUTH_FN};
    static const u32 QF[7] = {AVK_F_GT_QUERY_TP, AVK_F_GT_QUERY_FP, AVK_F_GT_QUERY_FP_GT, AVK_F_HAP_QUERY_TP, AVK_F_HAP_QUERY_FP, AVK_F_WHAP_QUERY_TP, AVK_F_WHAP_QUERY_FP};
    auto bin_of = [&](float s) {
        u32 b = 0;
        while (b < K && s >= spec.t[b]) ++b; /* (ascending thresholds: the count of those <= s; NaN stops at once) */
        return b;
    };
    for (u32 r = 0; r < n; ++r) {
        if (region_out[4 * r] != 0) continue;
        u32 tbin = K;
        for (u32 i = 0; i < q_cnt[r]; ++i)
            if (var_out[v_off[r] + t_cnt[r] + i] & 255u) {
                const u32 b = bin_of(scores[q_off[r] + i]);
                tbin = b < tbin ? b : tbin;
            }
        for (u32 i = 0; i < t_cnt[r] + q_cnt[r]; ++i) {
            const bool query = i >= t_cnt[r];
            const u64 c = t_off[r] + i; /* (the query calls follow the truth calls) */
            const u32 x = var_out[v_off[r] + i], ea = x & 255u, oa = (x >> 8) & 255u, exp = query ? oa : ea, obs = query ? ea : oa, d = exp - obs;
            const u64 w = vinfo[c].alt_ed;
            const u32 val[7] = {exp == obs, exp != obs, exp != obs && obs > 0, obs, d, (u32)(obs * w), (u32)(d * w)};
            const u32 bin = query ? bin_of(scores[c]) : obs == 0 ? K : tbin;
            for (u32 s = 0; s < n_scopes; ++s) {
                if (s && !((mask[avk::sx::sx_mask_at((s - 1) >> 5, r, n)] >> ((s - 1) & 31)) & 1u)) continue;
                for (u32 g : {0u, 1u + var_type[c]}) {
                    if (g >= AVK_N_GROUPS) continue;
                    for (u32 k = 0; k < n_points; ++k) {
                        u64 *dst = want.get() + (((size_t)s * n_points + k) * AVK_N_GROUPS + g) * AVK_SCORE_FIELDS;
                        if (k <= bin)
                            for (int q = 0; q < 7; ++q) dst[query ? QF[q] : TF[q]] += val[q];
                        else if (!query)
                            dst[AVK_F_GT_TRUTH_FN] += 1, dst[AVK_F_HAP_TRUTH_FN] += exp, dst[AVK_F_WHAP_TRUTH_FN] += (u32)(exp * w);
                    }
                }
            }
        }
    }
    if (memcmp(out.get(), want.get(), words * sizeof(u64)) != 0) {
        printf("score_check: curves differ (n %u, thresholds %u, labels %u, grid %u)\n", n, K, n_labels, grid);
        return 1;
    }
    u64 some = 0, wide = 0;
    for (size_t k = 0; k < words; ++k) some |= out[k], wide |= out[k] >> 32;
    if (!some || (n >= 64 && !wide)) {
        printf("score_check: nothing was summed, or no sum beyond 32 bits (n %u)\n", n);
        return 1;
    }
    return 0;
}

/* a textbook edit distance for the host route: insertions, deletions and substitutions cost 1 */
static uint64_t plain_edit_distance(const u8 *a, u64 n, const u8 *b, u64 m) {
    std::unique_ptr<u64[]> row(new u64[m + 1]);
    for (u64 j = 0; j <= m; ++j) row[j] = j;
    for (u64 i = 1; i <= n; ++i) {
        u64 diag = row[0];
        row[0] = i;
        for (u64 j = 1; j <= m; ++j) {
            const u64 up = row[j], sub = diag + (a[i - 1] != b[j - 1]);
            u64 x = up + 1 < row[j - 1] + 1 ? up + 1 : row[j - 1] + 1;
            row[j] = x < sub ? x : sub;
            diag = up;
        }
    }
    return row[m];
}

/* The host route: avk_score_host_sum on a batch of n regions whose sides lie apart in the call arrays (all truth calls of the batch, then all query calls, the
 * query side in reverse region order), results in the wide or the packed form */
static int check_host(u32 n, const avk_score_spec &spec, u32 n_labels, u32 threads, bool packed_results) {
    auto t_cnt = exact<u32>(n), q_cnt = exact<u32>(n);
    auto t_off = exact<u64>(n), q_off = exact<u64>(n);
    u64 nt = 0, nq = 0;
    for (u32 r = 0; r < n; ++r) t_cnt[r] = r == 2 ? 0 : rnd(5), q_cnt[r] = r == 2 ? 0 : rnd(5), t_off[r] = nt, nt += t_cnt[r];
    for (u32 r = n; r-- > 0;) q_off[r] = nt + nq, nq += q_cnt[r];
    const u64 nv = nt + nq;
    auto var_type = exact<u8>(nv), ve = exact<u8>(nv), vo = exact<u8>(nv), vp = exact<u8>(nv);
    auto a0_off = exact<u64>(nv), a1_off = exact<u64>(nv);
    auto a0_len = exact<u32>(nv), a1_len = exact<u32>(nv);
    auto scores = exact<float>(nv);
    const u32 K = spec.n_thresholds;
    u64 n_bytes = 0;
    for (u64 v = 0; v < nv; ++v) {
        var_type[v] = (u8)(rnd(4) ? rnd(3) : rnd(14));
        a0_len[v] = 1 + rnd(3), a1_len[v] = 1 + rnd(6);
        a0_off[v] = n_bytes, a1_off[v] = n_bytes + a0_len[v], n_bytes += a0_len[v] + a1_len[v];
        const u32 e = rnd(3), o = rnd(16) ? rnd(e + 1) : rnd(3); /* (0 .. 2: what the packed form's two bits hold as well) */
        ve[v] = (u8)e, vo[v] = (u8)o, vp[v] = (u8)(e | o << 2 | rnd(16) << 4);
        const u32 kind = rnd(8);
        const float t = spec.t[rnd(K)];
        scores[v] = kind == 0 ? NAN : kind == 1 ? INFINITY : kind == 2 ? -INFINITY : kind == 3 ? t : kind == 4 ? nextafterf(t, -INFINITY) : spec.t[0] - 3.0f + (float)rnd(1000) * 0.001f * (spec.t[K - 1] - spec.t[0] + 6.0f);
    }
    auto alleles = exact<u8>(n_bytes);
    for (u64 k = 0; k < n_bytes; ++k) alleles[k] = (u8)"ACGT"[rnd(4)];
    auto status = exact<int32_t>(n);
    auto region_packed = exact<u64>(n);
    for (u32 r = 0; r < n; ++r) status[r] = r % 11 == 7 ? 21 : 0, region_packed[r] = (u64)status[r] | (u64)rnd(1000) << 7;
    /* labels: label 0 on every region, label 1 on none, the others on a third; a region's list may name a label twice (it then counts twice) */
    auto label_off = exact<u64>((size_t)n + 1);
    u64 total = 0;
    for (int pass = 0; pass < 2; ++pass) { /* (the same draws twice: once to size label_idx exactly, once to fill it) */
        const u64 keep = rng_state;
        std::unique_ptr<u32[]> idx = exact<u32>(pass ? total : 0);
        u64 at = 0;
        for (u32 r = 0; r < n; ++r) {
            label_off[r] = at;
            for (u32 l = 0; l < n_labels; ++l) {
                const u32 times = l == 0 ? 1 : l == 1 ? 0 : rnd(3) == 0 ? 1 + (rnd(8) == 0) : 0;
                for (u32 q = 0; q < times; ++q, ++at)
                    if (pass) idx[at] = l;
            }
        }
        label_off[n] = at, total = at;
        if (!pass) {
            rng_state = keep;
            continue;
        }
        avk_region_batch b;
        memset((void *)&b, 0, sizeof(b));
        b.n_regions = n, b.t_off = t_off.get(), b.t_cnt = t_cnt.get(), b.q_off = q_off.get(), b.q_cnt = q_cnt.get();
        b.n_variants = nv, b.var_type = var_type.get(), b.a0_off = a0_off.get(), b.a0_len = a0_len.get(), b.a1_off = a1_off.get(), b.a1_len = a1_len.get();
        b.allele_bytes = alleles.get(), b.allele_bytes_len = n_bytes;
        avk_result_batch res;
        memset((void *)&res, 0, sizeof(res));
        if (packed_results) res.region_packed = region_packed.get(), res.var_packed = vp.get();
        else res.status = status.get(), res.var_expected = ve.get(), res.var_observed = vo.get();
        avk_region_labels lab;
        lab.n_labels = n_labels, lab.label_off = label_off.get(), lab.label_idx = idx.get();
        const u32 n_points = K + 1, n_scopes = 1 + n_labels;
        const size_t words = (size_t)n_scopes * AVK_SC_H_WORDS(n_points);
        auto out = exact<u64>(words), want = exact<u64>(words);
        if (avk_score_host_sum(&b, &res, &spec, scores.get(), n_labels ? &lab : nullptr, threads, plain_edit_distance, out.get())) {
            printf("score_check: the host route refused a valid batch\n");
            return 1;
        }
        static const u32 TF[7] = {AVK_F_GT_TRUTH_TP, AVK_F_GT_TRUTH_FN, AVK_F_GT_TRUTH_FN_GT, AVK_F_HAP_TRUTH_TP, AVK_F_HAP_TRUTH_FN, AVK_F_WHAP_TRUTH_TP, AVK_F_WHAP_TRUTH_FN};
        static const u32 QF[7] = {AVK_F_GT_QUERY_TP, AVK_F_GT_QUERY_FP, AVK_F_GT_QUERY_FP_GT, AVK_F_HAP_QUERY_TP, AVK_F_HAP_QUERY_FP, AVK_F_WHAP_QUERY_TP, AVK_F_WHAP_QUERY_FP};
        auto bin_of = [&](float x) {
            u32 k = 0;
            while (k < K && x >= spec.t[k]) ++k;
            return k;
        };
        for (u32 r = 0; r < n; ++r) {
            if (status[r] != 0) continue;
            u32 tbin = K;
            for (u32 i = 0; i < q_cnt[r]; ++i)
                if (ve[q_off[r] + i]) {
                    const u32 k = bin_of(scores[q_off[r] + i]);
                    tbin = k < tbin ? k : tbin;
                }
            for (u32 i = 0; i < t_cnt[r] + q_cnt[r]; ++i) {
                const bool query = i >= t_cnt[r];
                const u64 c = query ? q_off[r] + (i - t_cnt[r]) : t_off[r] + i;
                const u32 ea = ve[c], oa = vo[c], exp = query ? oa : ea, obs = query ? ea : oa, d = exp - obs;
                const u64 w = plain_edit_distance(alleles.get() + a0_off[c], a0_len[c], alleles.get() + a1_off[c], a1_len[c]);
                const u32 val[7] = {exp == obs, exp != obs, exp != obs && obs > 0, obs, d, (u32)(obs * w), (u32)(d * w)};
                const u32 bin = query ? bin_of(scores[c]) : obs == 0 ? K : tbin;
                for (u32 s = 0; s < n_scopes; ++s) {
                    u32 times = s == 0 ? 1 : 0;
                    for (u64 q = label_off[r]; s && q < label_off[r + 1]; ++q) times += idx[q] == s - 1;
                    for (u32 g : {0u, 1u + var_type[c]}) {
                        if (g >= AVK_N_GROUPS) continue;
                        for (u32 k = 0; k < n_points; ++k) {
                            u64 *dst = want.get() + (((size_t)s * n_points + k) * AVK_N_GROUPS + g) * AVK_SCORE_FIELDS;
                            if (k <= bin)
                                for (int q = 0; q < 7; ++q) dst[query ? QF[q] : TF[q]] += (u64)times * val[q];
                            else if (!query)
                                dst[AVK_F_GT_TRUTH_FN] += times, dst[AVK_F_HAP_TRUTH_FN] += (u64)times * exp, dst[AVK_F_WHAP_TRUTH_FN] += (u64)times * (u32)(exp * w);
                        }
                    }
                }
            }
        }
        u64 some = 0;
        for (size_t k = 0; k < words; ++k) some |= out[k];
        if (memcmp(out.get(), want.get(), words * sizeof(u64)) != 0 || !some) {
            printf("score_check: the host route's curve differs or is empty (n %u, thresholds %u, labels %u, threads %u, packed %d)\n", n, K, n_labels, threads, (int)packed_results);
            return 1;
        }
        /* a call range outside the batch, and a label that is none of the labels: refused, out untouched */
        const u32 victim = n - 1; /* (solved: n - 1 is not 7 mod 11 for the sizes used) */
        const u32 keep_cnt = q_cnt[victim];
        q_cnt[victim] = (u32)(nv - q_off[victim]) + 1;
        int refused = avk_score_host_sum(&b, &res, &spec, scores.get(), nullptr, threads, plain_edit_distance, out.get());
        q_cnt[victim] = keep_cnt;
        if (n_labels && total) {
            idx[0] = n_labels;
            refused += avk_score_host_sum(&b, &res, &spec, scores.get(), &lab, threads, plain_edit_distance, out.get());
        } else
            refused += 1;
        if (refused != 2 || memcmp(out.get(), want.get(), words * sizeof(u64)) != 0) {
            printf("score_check: the host route took an invalid batch, or touched its output while refusing one\n");
            return 1;
        }
    }
    return 0;
}

int main() {
    avk_score_spec one = {1, {20.0f}}, def = {10, {5, 10, 15, 20, 25, 30, 35, 40, 50, 60}}, full;
    full.n_thresholds = AVK_SCORE_THRESHOLDS_MAX;
    for (u32 k = 0; k < AVK_SCORE_THRESHOLDS_MAX; ++k) full.t[k] = -5.0f + 2.0f * (float)k;
    avk_score_spec bad[6] = {{0, {1}}, full, {2, {0, NAN}}, {2, {1, INFINITY}}, {2, {3, 3}}, {3, {1, 9, 8}}};
    bad[1].n_thresholds = AVK_SCORE_THRESHOLDS_MAX + 1;
    int wrong = 0, runs = 0;
    for (const avk_score_spec &b : bad) wrong += avk_score_spec_ok(&b);
    wrong += !avk_score_spec_ok(&one) + !avk_score_spec_ok(&def) + !avk_score_spec_ok(&full) + avk_score_spec_ok(nullptr);
    for (u32 k = 0; k < full.n_thresholds; ++k) /* bin() at every threshold */
        wrong += avk_score_bin_of(&full, nextafterf(full.t[k], -INFINITY)) != k || avk_score_bin_of(&full, full.t[k]) != k + 1;
    wrong += avk_score_bin_of(&def, NAN) != 0 || avk_score_bin_of(&def, INFINITY) != 10 || avk_score_bin_of(&def, -INFINITY) != 0 || avk_score_bin_of(&one, -0.0f) != 0;
    const u32 T = AVK_SC_THREADS;
    for (u32 n : {4u, 63u, 64u, 65u, T + 1}) wrong += check(n, def, 0, 2), ++runs; /* (a batch of one region may be one without calls: four at least) */
    wrong += check(T + 1, one, 3, 3), ++runs;  /* more workgroups than tiles */
    wrong += check(65, def, 7, 1), ++runs;     /* three launches of scopes */
    wrong += check(70, full, 34, 2), ++runs;   /* one scope a launch, scopes in a second mask word */
    wrong += check(70, one, 40, 1), ++runs;    /* many scopes a launch that straddle the mask words */
    /* the host route: no labels and labels, one thread and several (more threads than regions too), both result forms, 1, 10 and 31 thresholds */
    wrong += check_host(70, def, 0, 1, false), ++runs;
    wrong += check_host(70, def, 5, 3, false), ++runs;
    wrong += check_host(301, def, 4, 16, true), ++runs;
    wrong += check_host(5, one, 3, 16, true), ++runs;
    wrong += check_host(70, full, 34, 5, false), ++runs;
    wrong += check_host(64, full, 0, 64, true), ++runs;
    if (wrong) return 1;
    printf("score_check: ok (%d launches' worth of cases)\n", runs);
    return 0;
}
