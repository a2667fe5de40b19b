/*
 * avk_sizebin.inl — per-call tallies keyed by the call's SIZE, summed on the device (the rule: avk_sizebin.h).
 *
 * Every label of the stratified tallies is a property of a region; a size bin is a property of a call.  What a call adds is one iteration of lb_side
 * (avk_labels.inl: lb_call) — seven values, to the truth or the query fields of the joint group and of its type's group — and everything it is made of is in HBM
 * after any solve: the per-call words, the calls' types and allele lengths as the packer keeps them, alt_ed, the region's status, and the strata pass's masks for
 * the scopes.  No BASEPAIR groups are read.
 *
 * The region-keyed kernels' accumulation does not carry over: there few regions share a sum, here almost every call of a genome lands in the same few words
 * (bin 0, the joint group and the SNV group).  So the wave reduces before anything is added:
 *
 *   1. one lane per region; the wave walks its regions' calls in step (truth calls, then query calls), as many steps as its longest region has calls;
 *   2. at a step, for each scope of the launch, the lanes with a call in that scope are grouped by key (bin, type, side): the first pending lane's key is
 *      broadcast, the matching lanes are balloted, the three GT counts are population counts of ballots and the four HAP / WEIGHTED_HAP values are summed over the
 *      matching lanes on the DPP network (each as two 16-bit halves, so that the sum of 64 arbitrary 32-bit values is exact);
 *   3. the fourteen sums of a key (seven values x the joint group and the type's group) are added to the workgroup's block in LDS by fourteen lanes, one 64-bit
 *      LDS atomic each on fourteen different words — one instruction per key and step, whatever the number of calls behind it;
 *   4. after its last tile the workgroup adds its non-zero words to global memory.
 *
 * A launch holds the scopes [scope_lo, scope_hi) (scope 0: every region; scope 1 + l: the regions whose bit l is set in the strata pass's masks, sx_mask_at's
 * layout); the host sizes the block of scopes from AVK_SZ_LDS_BYTES.  A scope without a lane at a step costs one ballot.
 *
 * Written against avk_wave.h / DpIn / LbView like avk_labels.inl; sz_wave_tile is wave code (every lane of the wave calls it, control flow around the cross-lane
 * primitives is wave-uniform), and tests/emu/size_emu.cpp runs the same source on the CPU.
 */
#ifndef AVK_SIZEBIN_INL
#define AVK_SIZEBIN_INL

#include "avk_sizebin.h"
#include "avk_labels.inl"
#include "avk_strata.inl"

#define AVK_SZ_THREADS 256                                                    /* regions a workgroup takes at a time: one lane each, four waves */
#define AVK_SZ_LDS_BYTES 40960                                                /* a workgroup's blocks: four workgroups a CU */
#define AVK_SZ_SCOPES_MAX 32                                                  /* scopes of a launch: a lane keeps their membership in one word */
#define AVK_SZ_BLOCK_WORDS(n_bins) ((n_bins) * AVK_N_GROUPS * AVK_SIZE_FIELDS) /* one scope's 64-bit words */

namespace avk {
namespace sz {

typedef dp::u8 u8;
typedef dp::u32 u32;
typedef dp::u64 u64;

/* what a lane keeps of its region for the walk */
struct SzLane {
    u32 member; /* bit j: the region counts in scope scope_lo + j; 0: it does not count at all (beyond the batch, unsolved, calls out of range, in no scope) */
    u32 tc, n;  /* truth calls, calls */
    u64 toff, qoff;
    const u32 *vw;
};

/* one lane: region r of a batch of n for the scopes [scope_lo, scope_hi) (at most AVK_SZ_SCOPES_MAX) */
AVK_DEV SzLane sz_lane_begin(const lb::LbView &v, u64 r, u64 n, const u32 *mask, u32 scope_lo, u32 scope_hi) {
    SzLane L;
    L.member = 0, L.tc = L.n = 0, L.toff = L.qoff = 0, L.vw = v.var_out;
    if (r >= n || v.region_out[4 * r] != 0) return L;
    const u32 tc = v.in.t_cnt_of(r), qc = v.in.q_cnt_of(r);
    const u64 toff = v.in.t_off_of(r), qoff = v.in.q_off_of(r), nv = v.in.n_variants;
    if (toff > nv || (u64)tc > nv - toff || qoff > nv || (u64)qc > nv - qoff) return L; /* (lb_region_groups' refusal: such a region has an empty block) */
    u32 member = 0;
    for (u32 s = scope_lo; s < scope_hi; ++s) {
        u32 in = 1u;
        if (s) {
            const u32 l = s - 1u;
            in = (mask[sx::sx_mask_at(l >> 5, r, n)] >> (l & 31u)) & 1u;
        }
        member |= in << (s - scope_lo);
    }
    L.member = member, L.tc = tc, L.n = tc + qc, L.toff = toff, L.qoff = qoff, L.vw = v.var_out + v.v_off[r];
    return L;
}

/* one lane: call i of its region — the key (bin | type << 4 | side << 8; a type beyond the table counts in the joint group only and is keyed as 15) and the seven values */
AVK_DEV lb::LbCall sz_lane_call(const lb::LbView &v, const SzLane &L, u32 i, const avk_size_spec &spec, u32 &key) {
    const bool query = i >= L.tc;
    const u64 c = query ? L.qoff + (i - L.tc) : L.toff + i;
    const u32 vt = v.in.type_of(c);
    const u32 bin = avk_size_bin_of(&spec, avk_size_of(v.in.a0_len_of(c), v.in.a1_len_of(c)));
    key = bin | (vt < (u32)AVK_N_VARIANT_TYPES ? vt : 15u) << 4 | (query ? 1u : 0u) << 8;
    return lb::lb_call(L.vw[i], query, v.vinfo[c].alt_ed);
}

/* the sum of x over the lanes where on is set (off lanes pass 0), exact in 64 bits: two 16-bit halves of at most 64 x 65,535 each */
#define AVK_SZ_SUM(x) ((u64)wv_sum_u32((x) & 0xFFFFu) + ((u64)wv_sum_u32((x) >> 16) << 16))

/* The WAVE's regions tile_first + lane: every lane of the wave calls this.  acc: the workgroup's blocks, scope scope_lo first, added to with add(p, x) (a 64-bit
 * LDS atomic on the device). */
template <class Add>
AVK_DEV void sz_wave_tile(const lb::LbView &v, u64 r, u64 n, const u32 *mask, const avk_size_spec &spec, u32 scope_lo, u32 scope_hi, u64 *acc, Add &&add) {
    const u32 lane = (u32)wv_lane();
    const u32 n_bins = spec.n_edges + 1u, n_scopes = scope_hi - scope_lo;
    const SzLane L = sz_lane_begin(v, r, n, mask, scope_lo, scope_hi);
    const u32 steps = wv_max_u32(L.member ? L.n : 0u);
    for (u32 i = 0; i < steps; ++i) {
        const bool has = L.member && i < L.n;
        u32 key = 0;
        lb::LbCall c;
        c.gt_tp = c.gt_fn = c.gt_fn_gt = c.hap_tp = c.hap_fn = c.w_tp = c.w_fn = 0;
        if (has) c = sz_lane_call(v, L, i, spec, key);
        for (u32 j = 0; j < n_scopes; ++j) {
            u64 pending = wv_ballot(has && ((L.member >> j) & 1u));
            while (pending) { /* (wave-uniform: one round per key that occurs) */
                const u32 key0 = wv_readlane(key, (u32)avk_ctz64(pending));
                const bool same = ((pending >> lane) & 1ull) && key == key0;
                const u64 m = wv_ballot(same);
                u64 sum[AVK_SIZE_VALUES];
                sum[0] = (u64)avk_popc64(wv_ballot(same && c.gt_tp));
                sum[1] = (u64)avk_popc64(wv_ballot(same && c.gt_fn));
                sum[2] = (u64)avk_popc64(wv_ballot(same && c.gt_fn_gt));
                const u32 hap_tp = same ? c.hap_tp : 0u, hap_fn = same ? c.hap_fn : 0u, w_tp = same ? c.w_tp : 0u, w_fn = same ? c.w_fn : 0u;
                sum[3] = (u64)wv_sum_u32(hap_tp); /* (a byte a lane) */
                sum[4] = AVK_SZ_SUM(hap_fn);
                sum[5] = AVK_SZ_SUM(w_tp);
                sum[6] = AVK_SZ_SUM(w_fn);
                /* lane k < 7: value k into the joint group; lane 7 + k: into the type's group */
                if (lane < 2u * AVK_SIZE_VALUES) {
                    const u32 k = lane < AVK_SIZE_VALUES ? lane : lane - AVK_SIZE_VALUES;
                    const u32 bin = key0 & 15u, vt = (key0 >> 4) & 15u, query = key0 >> 8;
                    u64 x = sum[0];
#pragma unroll
                    for (int q = 1; q < AVK_SIZE_VALUES; ++q) x = k == (u32)q ? sum[q] : x;
                    const u32 g = lane < AVK_SIZE_VALUES ? 0u : 1u + vt;
                    if (x && g < (u32)AVK_N_GROUPS) add(acc + (((u64)j * n_bins + bin) * AVK_N_GROUPS + g) * AVK_SIZE_FIELDS + avk_size_field_of(k, (int)query), x);
                }
                pending &= ~m;
            }
        }
    }
}

} // namespace sz
} // namespace avk

#ifndef AVK_EMU
/* Scopes [scope_lo, scope_hi) over the batch's regions: out[((scope * n_bins + bin) * AVK_N_GROUPS + g) * AVK_SIZE_FIELDS + f] gains the sums.  Dynamic LDS:
 * (scope_hi - scope_lo) * AVK_SZ_BLOCK_WORDS(n_bins) * 8 bytes, at most AVK_SZ_LDS_BYTES. */
__global__ void __launch_bounds__(AVK_SZ_THREADS) avk_size_tally_kernel(avk::lb::LbView v, const uint32_t *mask, uint32_t n_regions, avk_size_spec spec, uint32_t scope_lo,
                                                                        uint32_t scope_hi, unsigned long long *out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char avk_smem[];
    unsigned long long *acc = (unsigned long long *)avk_smem;
    const unsigned block_words = AVK_SZ_BLOCK_WORDS(spec.n_edges + 1u), words = (scope_hi - scope_lo) * block_words;
    for (unsigned k = threadIdx.x; k < words; k += AVK_SZ_THREADS) acc[k] = 0;
    __syncthreads();
    const uint32_t n_tiles = (n_regions + AVK_SZ_THREADS - 1) / AVK_SZ_THREADS;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) /* (uniform over the workgroup: every lane of a wave enters sz_wave_tile) */
        avk::sz::sz_wave_tile(v, (uint64_t)tile * AVK_SZ_THREADS + threadIdx.x, n_regions, mask, spec, scope_lo, scope_hi, (uint64_t *)acc,
                              [](uint64_t *p, uint64_t x) { atomicAdd((unsigned long long *)p, (unsigned long long)x); });
    __syncthreads();
    for (unsigned k = threadIdx.x; k < words; k += AVK_SZ_THREADS) {
        const unsigned long long x = acc[k];
        if (x) atomicAdd(out + (size_t)scope_lo * block_words + k, x);
    }
}
#endif

#endif /* AVK_SIZEBIN_INL */
