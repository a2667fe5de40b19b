/*
 * boot_check.cpp — the bootstrap tally's lane functions (aardvark_amd/csrc/avk_boot.inl) under AddressSanitizer and UBSan, as a program of its own: every array the
 * lanes may read or write — the batch's, the results', the masks, the tile, the sums — is a heap block EXACTLY as long as the kernel's launch makes it, so a read
 * or write one element past any of them stops the program.  The launches are driven as avk_boot_tally_kernel drives them (tests/emu/boot_emu.cpp), for region counts
 * around the tile, replicate counts around a launch's block and scopes in two mask words; the sums are compared with a plain restatement: avk_boot_weight times the
 * block lb_region_groups gives, region by region.
 *
 * Built and run by tests/test_boot_native.py; never loaded into Python.  (avk_boot_tallies_host lives in the HIP translation unit and is checked against the same
 * restatement by tests/test_boot_rule.py.)
 */
#define AVK_EMU 1
#include <stdio.h>
#include <string.h>

#include <memory>

#include "../../aardvark_amd/csrc/avk_boot.inl"

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

static int check(u32 n, u32 B, u32 n_labels, u32 grid, u64 seed) {
    /* the batch: 0 .. 4 calls a side, types 0 .. 11, a few unsolved regions, one region without calls */
    auto t_cnt = exact<u32>(n), q_cnt = exact<u32>(n), contig = exact<u32>(n), v_off = exact<u32>(n), bp_off = exact<u32>(n + 1), region_out = exact<u32>(4 * (size_t)n);
    auto t_off = exact<u64>(n), q_off = exact<u64>(n), start = exact<u64>(n);
    u64 nv = 0;
    u32 ng = 0;
    for (u32 r = 0; r < n; ++r) {
        t_cnt[r] = r == 2 ? 0 : rnd(5), q_cnt[r] = r == 2 ? 0 : rnd(5);
        t_off[r] = nv, q_off[r] = nv + t_cnt[r], v_off[r] = (u32)nv;
        nv += t_cnt[r] + q_cnt[r];
        contig[r] = rnd(3), start[r] = 1000 + 977ull * r + ((u64)(r & 1) << 31);
        region_out[4 * r] = r % 11 == 7 ? 21u : 0u;
    }
    auto var_type = exact<u8>(nv), var_zyg = exact<u8>(nv);
    auto a0_len = exact<u32>(nv), a1_len = exact<u32>(nv), var_raw = exact<u32>(nv), var_out = exact<u32>(nv);
    std::unique_ptr<avk::dp::DpVarInfo[]> vinfo(new avk::dp::DpVarInfo[nv]);
    for (u64 v = 0; v < nv; ++v) {
        var_type[v] = (u8)rnd(12), var_zyg[v] = (u8)rnd(6), a0_len[v] = 1 + rnd(9), a1_len[v] = 1 + rnd(9), var_raw[v] = 1 + rnd(40);
        const u32 e = rnd(3), o = rnd(e + 1);
        var_out[v] = e | o << 8;
        memset(&vinfo[v], 0, sizeof(vinfo[v]));
        vinfo[v].alt_ed = 1 + rnd(12);
    }
    for (u32 r = 0; r < n; ++r) { /* the joint group, then one per call type of the region */
        u32 types = 0;
        for (u64 v = t_off[r]; v < t_off[r] + t_cnt[r] + q_cnt[r]; ++v) types |= 1u << var_type[v];
        bp_off[r] = ng;
        ng += 1 + (u32)__builtin_popcount(types);
    }
    bp_off[n] = ng;
    auto bp = exact<u32>(4 * (size_t)ng);
    for (size_t k = 0; k < 4 * (size_t)ng; ++k) bp[k] = rnd(300);
    const u32 n_words = (n_labels + 31) / 32;
    auto mask = exact<u32>((size_t)n_words * n);
    for (u32 l = 0; l < n_labels; ++l)
        for (u32 r = 0; r < n; ++r)
            if (l == 0 || (l != 1 && rnd(3) == 0)) mask[avk::sx::sx_mask_at(l >> 5, r, n)] |= 1u << (l & 31); /* label 0: every region; label 1: none */

    avk::lb::LbView v;
    memset(&v, 0, sizeof(v));
    v.in.n_regions = n, v.in.n_variants = nv;
    v.in.contig_idx = contig.get(), v.in.start = start.get(), v.in.t_off = t_off.get(), v.in.q_off = q_off.get(), v.in.t_cnt = t_cnt.get(), v.in.q_cnt = q_cnt.get();
    v.in.var_type = var_type.get(), v.in.var_zyg = var_zyg.get(), v.in.var_raw = var_raw.get(), v.in.a0_len = a0_len.get(), v.in.a1_len = a1_len.get();
    v.vinfo = vinfo.get(), v.region_out = region_out.get(), v.var_out = var_out.get(), v.v_off = v_off.get(), v.bp_off = bp_off.get(), v.bp = bp.get();

    const size_t words = ((size_t)n_labels + 1) * B * AVK_TALLY_LEN;
    auto out = exact<u64>(words), want = exact<u64>(words);
    /* the launches */
    auto blk = exact<u32>((size_t)AVK_BT_TILE_SLOTS * AVK_BT_SLOT), gm = exact<u32>(AVK_BT_TILE);
    auto h = exact<u64>(AVK_BT_TILE);
    auto w = exact<u8>((size_t)AVK_BT_TILE * AVK_BT_REPS);
    avk::bt::BtTile t;
    t.blk = blk.get(), t.h = h.get(), t.gm = gm.get(), t.w = w.get();
    const u32 n_tiles = (n + AVK_BT_TILE - 1) / AVK_BT_TILE;
    const u64 seed_mix = avk_boot_mix(seed);
    auto add = [](u64 *p, u64 x) { *p += x; };
    for (u32 scope = 0; scope <= n_labels; ++scope)
        for (u32 lo = 0; lo < B; lo += AVK_BT_REPS) {
            const u32 hi = B - lo > AVK_BT_REPS ? lo + AVK_BT_REPS : B;
            for (u32 wg = 0; wg < grid; ++wg) {
                auto acc = exact<u64>((size_t)AVK_BT_THREADS * AVK_N_GROUPS);
                for (u32 tile = wg; tile < n_tiles; tile += grid) {
                    u32 any = 0;
                    for (u32 tid = 0; tid < AVK_BT_TILE; ++tid) any |= avk::bt::bt_stage_region(v, (u64)tile * AVK_BT_TILE + tid, n, mask.get(), scope, seed_mix, tid, t);
                    if (!any) continue;
                    for (u32 e = 0; e < AVK_BT_TILE * AVK_BT_REPS; ++e) avk::bt::bt_weight_entry(t, e, lo, hi);
                    for (u32 tid = 0; tid < AVK_BT_THREADS; ++tid) {
                        const u32 bl = tid / AVK_BT_SLOT, f = tid % AVK_BT_SLOT;
                        if (bl >= AVK_BT_REPS) continue;
                        u64(&a)[AVK_N_GROUPS] = *(u64(*)[AVK_N_GROUPS])(acc.get() + (size_t)tid * AVK_N_GROUPS);
                        for (u32 rt = 0; rt < AVK_BT_TILE; ++rt)
                            if (t.gm[rt]) avk::bt::bt_lane_region(t, rt, t.gm[rt], bl, f, a);
                    }
                }
                for (u32 tid = 0; tid < AVK_BT_THREADS; ++tid) {
                    const u32 bl = tid / AVK_BT_SLOT, f = tid % AVK_BT_SLOT;
                    if (bl >= AVK_BT_REPS || lo + bl >= hi) continue;
                    const u64(&a)[AVK_N_GROUPS] = *(const u64(*)[AVK_N_GROUPS])(acc.get() + (size_t)tid * AVK_N_GROUPS);
                    avk::bt::bt_lane_flush(a, scope, B, lo + bl, f, out.get(), add);
                }
            }
        }
    /* the restatement */
    for (u32 r = 0; r < n; ++r) {
        if (region_out[4 * r] != 0) continue;
        u32 block[AVK_LB_WORDS];
        memset(block, 0, sizeof(block));
        avk::lb::lb_region_groups(v, r, [&](u32 g, const u32(&F)[AVK_N_FIELDS]) { memcpy(block + g * AVK_N_FIELDS, F, sizeof(F)); });
        for (u32 scope = 0; scope <= n_labels; ++scope) {
            if (scope && !((mask[avk::sx::sx_mask_at((scope - 1) >> 5, r, n)] >> ((scope - 1) & 31)) & 1u)) continue;
            for (u32 b = 0; b < B; ++b) {
                const u64 wt = avk_boot_weight(seed, contig[r], (u32)start[r], b);
                u64 *dst = want.get() + ((size_t)scope * B + b) * AVK_TALLY_LEN;
                for (int i = 0; i < AVK_LB_WORDS; ++i) dst[i] += wt * block[i];
                dst[AVK_TALLY_SOLVED] += wt;
            }
        }
    }
    if (memcmp(out.get(), want.get(), words * sizeof(u64)) != 0) {
        printf("boot_check: sums differ (n %u, B %u, labels %u, grid %u)\n", n, B, n_labels, grid);
        return 1;
    }
    u64 some = 0;
    for (size_t k = 0; k < words; ++k) some |= out[k];
    if (!some) {
        printf("boot_check: nothing was summed (n %u, B %u)\n", n, B);
        return 1;
    }
    return 0;
}

int main() {
    const u32 T = AVK_BT_TILE, R = AVK_BT_REPS;
    const u32 ns[] = {1, T - 1, T, T + 1, 2 * T + 1}, Bs[] = {1, R - 1, R, R + 1, 2 * R + 1};
    int bad = 0, runs = 0;
    for (u32 n : ns) bad += check(n == 1 ? 4 : n, R + 1, 0, 2, 7 + n), ++runs; /* (a batch of one region may be one without calls: four at least) */
    bad += check(1, 3, 0, 1, 5), ++runs;
    for (u32 B : Bs) bad += check(2 * T + 1, B, 2, 3, 100 + B), ++runs;
    bad += check(3 * T + 5, R + 1, 34, 2, 9), ++runs; /* scopes in a second mask word */
    if (bad) return 1;
    printf("boot_check: ok (%d launches' worth of cases)\n", runs);
    return 0;
}
