/*
 * size_check.cpp — the size-bin tally's wave code (aardvark_amd/csrc/avk_sizebin.inl) and the rule's header (avk_sizebin.h) under AddressSanitizer and UBSan, as a
 * program of its own: every array the lanes may read or write — the batch's, the results', the masks, the workgroup's block, the sums — is a heap block EXACTLY as
 * long as the kernel's launch makes it, so a read or write one element past any of them stops the program.  The launches are driven as avk_size_tally_kernel and its
 * host loop drive them (tests/emu/size_emu.cpp; a wave's lanes are 64 threads, tests/emu/wave_threads.h), for region counts around the wave and the tile, 1, 4 and 15
 * edges and scopes in two mask words; the sums are compared with a plain restatement, call by call.  The data go beyond what a solver writes — observed above
 * expected (values that wrap in 32 bits), alt_ed in the millions (sums beyond 32 bits within one wave), types beyond the table — because the wave's reduction must be
 * exact for any words.
 *
 * Built and run by tests/test_size_native.py; never loaded into Python.  (avk_size_tallies_host lives in the HIP translation unit and is checked against the
 * restatement by tests/test_size_rule.py.)
 */
#define AVK_EMU 1
#include <stdio.h>
#include <string.h>

#include <memory>

#include "../emu/wave_threads.h"

#include "../../aardvark_amd/csrc/avk_sizebin.inl"

typedef uint8_t u8;
typedef uint32_t u32;
typedef uint64_t u64;

template <class T> static std::unique_ptr<T[]> exact(size_t n) { /* (a zero-length block is still a block of its own: reading it is an error) */
    std::unique_ptr<T[]> p(new T[n]);
    if (n) memset(p.get(), 0, n * sizeof(T));
    return p;
}

static u64 rng_state = 0x9E3779B97F4A7C15ull;
static u32 rnd(u32 n) {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (u32)(rng_state >> 33) % n;
}

static int check(u32 n, const avk_size_spec &spec, u32 n_labels, u32 grid) {
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
    std::unique_ptr<avk::dp::DpVarInfo[]> vinfo(new avk::dp::DpVarInfo[nv]);
    for (u64 v = 0; v < nv; ++v) {
        var_type[v] = (u8)(rnd(4) ? rnd(3) : rnd(14)), var_zyg[v] = (u8)rnd(6); /* (types 12 and 13 are beyond the table: the joint group only) */
        const u32 kind = rnd(8);
        a0_len[v] = 1, a1_len[v] = 1;
        if (kind >= 5) (rnd(2) ? a0_len[v] : a1_len[v]) = 1 + (kind == 7 ? rnd(6000) : rnd(60));
        const u32 e = rnd(3), o = rnd(16) ? rnd(e + 1) : rnd(3);
        var_out[v] = e | o << 8 | rnd(256) << 16 | rnd(256) << 24;
        memset(&vinfo[v], 0, sizeof(vinfo[v]));
        vinfo[v].alt_ed = rnd(8) ? 1 + rnd(12) : 1 + rnd(90000000);
    }
    const u32 n_words = (n_labels + 31) / 32;
    auto mask = exact<u32>((size_t)n_words * n);
    for (u32 l = 0; l < n_labels; ++l)
        for (u32 r = 0; r < n; ++r)
            if (l == 0 || (l != 1 && rnd(3) == 0)) mask[avk::sx::sx_mask_at(l >> 5, r, n)] |= 1u << (l & 31); /* label 0: every region; label 1: none */

    avk::lb::LbView v;
    memset(&v, 0, sizeof(v));
    v.in.n_regions = n, v.in.n_variants = nv;
    v.in.t_off = t_off.get(), v.in.q_off = q_off.get(), v.in.t_cnt = t_cnt.get(), v.in.q_cnt = q_cnt.get();
    v.in.var_type = var_type.get(), v.in.var_zyg = var_zyg.get(), v.in.a0_len = a0_len.get(), v.in.a1_len = a1_len.get();
    v.vinfo = vinfo.get(), v.region_out = region_out.get(), v.var_out = var_out.get(), v.v_off = v_off.get();

    const u32 n_bins = spec.n_edges + 1, block_words = AVK_SZ_BLOCK_WORDS(n_bins), n_scopes = 1 + n_labels;
    const size_t words = (size_t)n_scopes * block_words;
    auto out = exact<u64>(words), want = exact<u64>(words);
    /* the launches */
    u32 per_launch = AVK_SZ_LDS_BYTES / (block_words * 8u);
    if (per_launch > AVK_SZ_SCOPES_MAX) per_launch = AVK_SZ_SCOPES_MAX;
    const u32 n_tiles = (n + AVK_SZ_THREADS - 1) / AVK_SZ_THREADS;
    auto add = [](u64 *p, u64 x) { __atomic_fetch_add(p, x, __ATOMIC_RELAXED); };
    for (u32 lo = 0; lo < n_scopes; lo += per_launch) {
        const u32 hi = n_scopes - lo > per_launch ? lo + per_launch : n_scopes;
        for (u32 wg = 0; wg < grid; ++wg) {
            auto acc = exact<u64>((size_t)(hi - lo) * block_words);
            for (u32 tile = wg; tile < n_tiles; tile += grid)
                for (u32 wave = 0; wave < AVK_SZ_THREADS / 64; ++wave) {
                    if ((u64)tile * AVK_SZ_THREADS + wave * 64u >= n) continue; /* (a wave beyond the batch finds no call: not worth 64 threads) */
                    avk_emu::run_wave([&](int lane) {
                        avk::sz::sz_wave_tile(v, (u64)tile * AVK_SZ_THREADS + wave * 64u + (u32)lane, n, n_labels ? mask.get() : nullptr, spec, lo, hi, acc.get(), add);
                    });
                }
            for (size_t k = 0; k < (size_t)(hi - lo) * block_words; ++k) out[(size_t)lo * block_words + k] += acc[k];
        }
    }
    /* the restatement: every call of every solved region, in 64-bit sums of 32-bit values */
    static const u32 TF[7] = {AVK_F_GT_TRUTH_TP, AVK_F_GT_TRUTH_FN, AVK_F_GT_TRUTH_FN_GT, AVK_F_HAP_TRUTH_TP, AVK_F_HAP_TRUTH_FN, AVK_F_WHAP_TRUTH_TP, AVK_F_WHAP_TRUTH_FN};
    static const u32 QF[7] = {AVK_F_GT_QUERY_TP, AVK_F_GT_QUERY_FP, AVK_F_GT_QUERY_FP_GT, AVK_F_HAP_QUERY_TP, AVK_F_HAP_QUERY_FP, AVK_F_WHAP_QUERY_TP, AVK_F_WHAP_QUERY_FP};
    for (u32 r = 0; r < n; ++r) {
        if (region_out[4 * r] != 0) continue;
        for (u32 i = 0; i < t_cnt[r] + q_cnt[r]; ++i) {
            const bool query = i >= t_cnt[r];
            const u64 c = t_off[r] + i; /* (the query calls follow the truth calls) */
            const u32 x = var_out[v_off[r] + i], ea = x & 255u, oa = (x >> 8) & 255u, exp = query ? oa : ea, obs = query ? ea : oa, d = exp - obs;
            const u64 w = vinfo[c].alt_ed;
            const u32 val[7] = {exp == obs, exp != obs, exp != obs && obs > 0, obs, d, (u32)(obs * w), (u32)(d * w)};
            const u32 size = a0_len[c] > a1_len[c] ? a0_len[c] - a1_len[c] : a1_len[c] - a0_len[c];
            u32 bin = 0;
            while (bin < spec.n_edges && size >= spec.edges[bin]) ++bin;
            for (u32 s = 0; s < n_scopes; ++s) {
                if (s && !((mask[avk::sx::sx_mask_at((s - 1) >> 5, r, n)] >> ((s - 1) & 31)) & 1u)) continue;
                for (u32 g : {0u, 1u + var_type[c]}) {
                    if (g >= AVK_N_GROUPS) continue;
                    for (int k = 0; k < 7; ++k) want[(((size_t)s * n_bins + bin) * AVK_N_GROUPS + g) * AVK_SIZE_FIELDS + (query ? QF[k] : TF[k])] += val[k];
                }
            }
        }
    }
    if (memcmp(out.get(), want.get(), words * sizeof(u64)) != 0) {
        printf("size_check: sums differ (n %u, edges %u, labels %u, grid %u)\n", n, spec.n_edges, n_labels, grid);
        return 1;
    }
    u64 some = 0, wide = 0;
    for (size_t k = 0; k < words; ++k) some |= out[k], wide |= out[k] >> 32;
    if (!some || (n >= 64 && !wide)) {
        printf("size_check: nothing was summed, or no sum beyond 32 bits (n %u)\n", n);
        return 1;
    }
    return 0;
}

int main() {
    const avk_size_spec one = {1, {2}}, def = {4, {1, 6, 16, 50}}, full = {15, {1, 2, 3, 4, 5, 6, 8, 11, 16, 21, 31, 50, 100, 1000, 5000}};
    const avk_size_spec bad[] = {{0, {1}}, {16, {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}}, {2, {0, 5}}, {2, {3, 3}}, {3, {1, 9, 8}}};
    int wrong = 0, runs = 0;
    for (const avk_size_spec &b : bad) wrong += avk_size_spec_ok(&b);
    wrong += !avk_size_spec_ok(&one) + !avk_size_spec_ok(&def) + !avk_size_spec_ok(&full) + avk_size_spec_ok(nullptr);
    for (u32 e = 0; e < full.n_edges; ++e) /* bin() at every edge */
        wrong += avk_size_bin_of(&full, full.edges[e] - 1) != e || avk_size_bin_of(&full, full.edges[e]) != e + 1;
    wrong += avk_size_bin_of(&def, 0xFFFFFFFFu) != 4 || avk_size_bin_of(&one, 0) != 0;
    const u32 T = AVK_SZ_THREADS;
    for (u32 n : {4u, 63u, 64u, 65u, T + 1}) wrong += check(n, def, 0, 2), ++runs; /* (a batch of one region may be one without calls: four at least) */
    wrong += check(T + 1, one, 3, 3), ++runs;   /* more workgroups than tiles */
    wrong += check(65, def, 7, 1), ++runs;      /* two launches of scopes */
    wrong += check(70, full, 34, 2), ++runs;    /* one scope a launch, scopes in a second mask word */
    wrong += check(70, one, 40, 1), ++runs;     /* fourteen scopes a launch that straddle the mask words */
    if (wrong) return 1;
    printf("size_check: ok (%d launches' worth of cases)\n", runs);
    return 0;
}
