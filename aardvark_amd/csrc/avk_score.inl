/*
 * avk_score.inl — the precision-recall curve by query score, summed on the device (the rule: avk_score.h).
 *
 * Two kernels.  avk_score_hist_kernel has avk_size_tally_kernel's shape (avk_sizebin.inl) with a caller-supplied key per call and two things the size rule
 * does not need:
 *
 *   1. truth calls carry no score: before the walk each lane reduces its own region's query calls to the region's truth bin — the minimum bin over the query
 *      calls with hap_tp > 0 — in a plain per-lane loop (no cross-lane step inside it);
 *   2. a truth call that loses its support turns from TP into FN: beside the histogram H[bin][g][14] of the normal values the workgroup keeps Lost[bin][g][3],
 *      the lost values (gt_fn, hap_fn, w_fn) of the truth calls with observed > 0.
 *
 * The wave then walks its regions' calls in step; per scope of the launch the lanes are grouped by key (bin, type, side), the ten sums of a key (seven normal,
 * three lost) are made by ballots, population counts and DPP sums — exact in 64 bits (AVK_SZ_SUM) — and twenty lanes add them to the workgroup's LDS block in
 * one instruction.  After its last tile a workgroup adds its non-zero words to a cleared pool block in HBM.
 *
 * avk_score_curve_kernel turns histogram BINS into curve POINTS: one wave per (scope, group) row, lane = point;
 *   curve[k][f] = sum over bins b >= k of H[b][f]   (+ sum over bins b < k of Lost[b] for f in GT_TRUTH_FN, HAP_TRUTH_FN, WHAP_TRUTH_FN)
 * — a suffix scan and an exclusive prefix scan across the lanes, with the wave's shuffles.
 *
 * Written against avk_wave.h / LbView / sx_mask_at like avk_sizebin.inl; sc_wave_tile and sc_wave_curve are wave code (every lane of the wave calls them, control
 * flow around the cross-lane primitives is wave-uniform), and tests/emu/score_emu.cpp runs the same source on the CPU.
 */
#ifndef AVK_SCORE_INL
#define AVK_SCORE_INL

#include "avk_score.h"
#include "avk_sizebin.inl"

#define AVK_SC_THREADS 256     /* regions a workgroup takes at a time: one lane each, four waves */
#define AVK_SC_LDS_BYTES 65536 /* a workgroup's blocks: one scope of the widest spec (56,576 B); two workgroups a CU */
#define AVK_SC_CU_LDS_BYTES 163840 /* a CU's LDS on gfx950: the host sizes the workgroups a CU from it and a launch's blocks */
#define AVK_SC_SCOPES_MAX 32  /* scopes of a launch: a lane keeps their membership in one word */
#define AVK_SC_VALUES (AVK_SIZE_VALUES + AVK_SCORE_LOST)
#define AVK_SC_ERR_GEOMETRY 1u /* the error word: the launch's blocks do not fit its LDS, or the number of thresholds is out of range — nothing was added (the host checks the
                                * whole spec before it queues anything: the thresholds' order is not looked at again here, which would cost the kernel its scalar copy of them) */

namespace avk {
namespace sc {

typedef dp::u32 u32;
typedef dp::u64 u64;

/* one lane: the truth bin of its region — the minimum bin over its query calls with hap_tp > 0 (the low byte of a query entry: lb_call's toggled reading) */
AVK_DEV u32 sc_truth_bin(const sz::SzLane &L, const avk_score_spec &spec, const float *scores) {
    u32 b = spec.n_thresholds;
    for (u32 i = L.tc; i < L.n; ++i) {
        if ((L.vw[i] & 0xFFu) == 0) continue;
        const u32 q = avk_score_bin_of(&spec, scores[L.qoff + (i - L.tc)]);
        b = q < b ? q : b;
    }
    return b;
}

/* one lane: call i of its region — the key (bin | type << 5 | side << 9; a type beyond the table counts in the joint group only and is keyed as 15), the seven
 * normal values, and the three lost values (all 0 unless it is a truth call with observed > 0) */
AVK_DEV lb::LbCall sc_lane_call(const lb::LbView &v, const sz::SzLane &L, u32 i, const avk_score_spec &spec, const float *scores, u32 tbin, u32 &key, u32 lost[AVK_SCORE_LOST]) {
    const bool query = i >= L.tc;
    const u64 c = query ? L.qoff + (i - L.tc) : L.toff + i;
    const u32 vt = v.in.type_of(c), x = L.vw[i];
    const u64 w = v.vinfo[c].alt_ed;
    const u32 exp = x & 0xFFu, obs = (x >> 8) & 0xFFu; /* (a truth entry's reading) */
    const u32 bin = query ? avk_score_bin_of(&spec, scores[c]) : obs == 0 ? spec.n_thresholds : tbin;
    const bool loses = !query && obs > 0;
    lost[0] = loses ? 1u : 0u, lost[1] = loses ? exp : 0u, lost[2] = loses ? (u32)((u64)exp * w) : 0u;
    key = bin | (vt < (u32)AVK_N_VARIANT_TYPES ? vt : 15u) << 5 | (query ? 1u : 0u) << 9;
    return lb::lb_call(x, query, w);
}

/* The WAVE's regions tile_first + lane: every lane of the wave calls this.  acc: the workgroup's blocks, scope scope_lo first (each AVK_SC_BLOCK_WORDS: H, then
 * Lost), added to with add(p, x) (a 64-bit LDS atomic on the device). */
template <class Add>
AVK_DEV void sc_wave_tile(const lb::LbView &v, u64 r, u64 n, const u32 *mask, const avk_score_spec &spec, const float *scores, u32 scope_lo, u32 scope_hi, u64 *acc, Add &&add) {
    const u32 lane = (u32)wv_lane();
    const u32 n_points = spec.n_thresholds + 1u, n_scopes = scope_hi - scope_lo;
    const sz::SzLane L = sz::sz_lane_begin(v, r, n, mask, scope_lo, scope_hi);
    const u32 tbin = L.member ? sc_truth_bin(L, spec, scores) : 0u; /* (per lane: no cross-lane step inside) */
    const u32 steps = wv_max_u32(L.member ? L.n : 0u);
    for (u32 i = 0; i < steps; ++i) {
        const bool has = L.member && i < L.n;
        u32 key = 0, lost[AVK_SCORE_LOST] = {0, 0, 0};
        lb::LbCall c;
        c.gt_tp = c.gt_fn = c.gt_fn_gt = c.hap_tp = c.hap_fn = c.w_tp = c.w_fn = 0;
        if (has) c = sc_lane_call(v, L, i, spec, scores, tbin, key, lost);
        for (u32 j = 0; j < n_scopes; ++j) {
            u64 pending = wv_ballot(has && ((L.member >> j) & 1u));
            while (pending) { /* (wave-uniform: one round per key that occurs) */
                const u32 key0 = wv_readlane(key, (u32)avk_ctz64(pending));
                const bool same = ((pending >> lane) & 1ull) && key == key0;
                const u64 m = wv_ballot(same);
                u64 sum[AVK_SC_VALUES];
                sum[0] = (u64)avk_popc64(wv_ballot(same && c.gt_tp));
                sum[1] = (u64)avk_popc64(wv_ballot(same && c.gt_fn));
                sum[2] = (u64)avk_popc64(wv_ballot(same && c.gt_fn_gt));
                const u32 hap_tp = same ? c.hap_tp : 0u, hap_fn = same ? c.hap_fn : 0u, w_tp = same ? c.w_tp : 0u, w_fn = same ? c.w_fn : 0u;
                sum[3] = (u64)wv_sum_u32(hap_tp); /* (a byte a lane) */
                sum[4] = AVK_SZ_SUM(hap_fn);
                sum[5] = AVK_SZ_SUM(w_tp);
                sum[6] = AVK_SZ_SUM(w_fn);
                const u64 losers = wv_ballot(same && lost[0]);
                sum[7] = (u64)avk_popc64(losers);
                sum[8] = sum[9] = 0;
                if (losers) { /* (wave-uniform; query keys and unsupported truth calls have none) */
                    const u32 l_hap = same ? lost[1] : 0u, l_w = same ? lost[2] : 0u;
                    sum[8] = (u64)wv_sum_u32(l_hap); /* (a byte a lane) */
                    sum[9] = AVK_SZ_SUM(l_w);
                }
                /* lane k < 10: value k into the joint group; lane 10 + k: into the type's group */
                if (lane < 2u * AVK_SC_VALUES) {
                    const u32 k = lane < AVK_SC_VALUES ? lane : lane - AVK_SC_VALUES;
                    const u32 bin = key0 & 31u, vt = (key0 >> 5) & 15u, query = key0 >> 9;
                    u64 x = sum[0];
#pragma unroll
                    for (int q = 1; q < AVK_SC_VALUES; ++q) x = k == (u32)q ? sum[q] : x;
                    const u32 g = lane < AVK_SC_VALUES ? 0u : 1u + vt;
                    u64 *blk = acc + (u64)j * AVK_SC_BLOCK_WORDS(n_points);
                    const u32 at = k < AVK_SIZE_VALUES ? (bin * AVK_N_GROUPS + g) * AVK_SCORE_FIELDS + avk_size_field_of(k, (int)query)
                                                       : AVK_SC_H_WORDS(n_points) + (bin * AVK_N_GROUPS + g) * AVK_SCORE_LOST + (k - AVK_SIZE_VALUES);
                    if (x && g < (u32)AVK_N_GROUPS) add(blk + at, x);
                }
                pending &= ~m;
            }
        }
    }
}

/* a 64-bit value of lane src (any lane; per lane) */
#define AVK_SC_SHFL64(x, src) ((u64)wv_shfl((u32)(x), (int)(src)) | (u64)wv_shfl((u32)((x) >> 32), (int)(src)) << 32)

/* The WAVE's row (one scope's block `hist`, group g): lane = point.  The lanes at and beyond n_points (<= 32) hold zeros, so five doubling steps cover both
 * scans.  row: the scope's curve block [n_points][AVK_N_GROUPS][AVK_SCORE_FIELDS]; one wave owns a row's words. */
AVK_DEV void sc_wave_curve(const u64 *hist, u32 n_points, u32 g, u64 *row) {
    const u32 lane = (u32)wv_lane();
    const bool on = lane < n_points;
    for (u32 f = 0; f < AVK_SCORE_FIELDS; ++f) {
        u64 x = on ? hist[(lane * AVK_N_GROUPS + g) * AVK_SCORE_FIELDS + f] : 0ull;
        for (u32 d = 1; d < 32u; d <<= 1) { /* inclusive suffix sum: bins >= point */
            const u64 t = AVK_SC_SHFL64(x, (lane + d) & 63u);
            x += lane + d < 64u ? t : 0ull;
        }
        const u32 lj = avk_score_lost_of_field(f); /* (wave-uniform) */
        if (lj) {
            const u64 own = on ? hist[AVK_SC_H_WORDS(n_points) + (lane * AVK_N_GROUPS + g) * AVK_SCORE_LOST + (lj - 1u)] : 0ull;
            u64 y = own;
            for (u32 d = 1; d < 32u; d <<= 1) { /* inclusive prefix sum ... */
                const u64 t = AVK_SC_SHFL64(y, (lane - d) & 63u);
                y += lane >= d ? t : 0ull;
            }
            x += y - own; /* ... made exclusive: bins < point */
        }
        if (on && x) row[(lane * AVK_N_GROUPS + g) * AVK_SCORE_FIELDS + f] += x;
    }
}

} // namespace sc
} // namespace avk

#ifndef AVK_EMU
/* Scopes [scope_lo, scope_hi) over the batch's regions: hist[scope * AVK_SC_BLOCK_WORDS(n_points) + ..] gains the sums.  Dynamic LDS: lds_words 64-bit words,
 * at least (scope_hi - scope_lo) * AVK_SC_BLOCK_WORDS(n_points); a launch that does not hold its blocks sets the error word and adds nothing. */
__global__ void __launch_bounds__(AVK_SC_THREADS) avk_score_hist_kernel(avk::lb::LbView v, const uint32_t *mask, uint32_t n_regions, avk_score_spec spec, const float *scores,
                                                                        uint32_t scope_lo, uint32_t scope_hi, uint32_t lds_words, unsigned long long *hist, uint32_t *err) {
    extern __shared__ __attribute__((aligned(16))) unsigned char avk_smem[];
    unsigned long long *acc = (unsigned long long *)avk_smem;
    const unsigned block_words = AVK_SC_BLOCK_WORDS(spec.n_thresholds + 1u), words = (scope_hi - scope_lo) * block_words;
    if (spec.n_thresholds < 1u || spec.n_thresholds > AVK_SCORE_THRESHOLDS_MAX || scope_hi <= scope_lo || scope_hi - scope_lo > AVK_SC_SCOPES_MAX || words > lds_words) { /* (uniform over the grid) */
        if (threadIdx.x == 0 && blockIdx.x == 0) atomicOr(err, AVK_SC_ERR_GEOMETRY);
        return;
    }
    for (unsigned k = threadIdx.x; k < words; k += AVK_SC_THREADS) acc[k] = 0;
    __syncthreads();
    const uint32_t n_tiles = (n_regions + AVK_SC_THREADS - 1) / AVK_SC_THREADS;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) /* (uniform over the workgroup: every lane of a wave enters sc_wave_tile) */
        avk::sc::sc_wave_tile(v, (uint64_t)tile * AVK_SC_THREADS + threadIdx.x, n_regions, mask, spec, scores, scope_lo, scope_hi, (uint64_t *)acc,
                              [](uint64_t *p, uint64_t x) { atomicAdd((unsigned long long *)p, (unsigned long long)x); });
    __syncthreads();
    for (unsigned k = threadIdx.x; k < words; k += AVK_SC_THREADS) {
        const unsigned long long x = acc[k];
        if (x) atomicAdd(hist + (size_t)scope_lo * block_words + k, x);
    }
}

/* One wave (a workgroup of 64) per (scope, group) row of n_scopes * AVK_N_GROUPS: curve[((scope * n_points + k) * AVK_N_GROUPS + g) * AVK_SCORE_FIELDS + f] gains
 * the row's points.  Nothing is added when the error word is set. */
__global__ void __launch_bounds__(64) avk_score_curve_kernel(const unsigned long long *hist, uint32_t n_points, uint32_t n_scopes, const uint32_t *err, unsigned long long *curve) {
    const uint32_t row = blockIdx.x, scope = row / AVK_N_GROUPS, g = row % AVK_N_GROUPS;
    if (scope >= n_scopes || n_points < 2u || n_points > AVK_SCORE_THRESHOLDS_MAX + 1u || *err) return; /* (uniform over the wave) */
    avk::sc::sc_wave_curve((const uint64_t *)hist + (size_t)scope * AVK_SC_BLOCK_WORDS(n_points), n_points, g, (uint64_t *)curve + (size_t)scope * AVK_SC_H_WORDS(n_points));
}
#endif

#endif /* AVK_SCORE_INL */
