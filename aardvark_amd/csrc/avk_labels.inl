/*
 * avk_labels.inl — stratified tallies from the COMPACT results of a device-packed batch.
 *
 * SummaryWriter::add_comparison_benchmark (src/writers/summary.rs:146-163) adds a region's GroupTypeMetrics to every containment label of the region.
 * avk_label_tally_kernel (avk_host.hip) does that from the full 13 x 22 block per region, which every solver kernel then has to write: 1,144 bytes a region
 * where the rest of a region's results are a few dozen.  Everything the block is made of is on the device after a run WITHOUT the blocks: the region's status,
 * expected / observed per call, the calls' type, zygosity and raw space as the caller sent them, Variant::alt_ed (DpVarInfo) and the compact BASEPAIR groups.
 * lb_region_groups below is avk_group_metrics_from_compact (the host's statement of the rule) on that view, one LANE per region — 99.6 % of a genome's regions
 * have at most three calls a side — and lb_region_labels adds its groups to the 64-bit sums of the labels the region's list names.
 *
 * A batch in flight (avk_compare_packed_submit_strata) has no lists: lb_region_labels_mask reads the region's labels straight from the bit masks the strata mask
 * pass leaves (avk_strata.inl: 32 labels a word, word-major), so neither the offsets nor an index array — larger than the batch with hundreds of overlapping
 * labels — exist for the one read they would get.
 *
 * Written against avk_wave.h / DpIn like avk_devpack.inl, so tests/emu/label_emu.cpp and tests/emu/label_mask_emu.cpp run the same functions on the CPU against
 * the oracle's blocks.
 */
#ifndef AVK_LABELS_INL
#define AVK_LABELS_INL

#include "avk_devpack.inl"

#define AVK_LB_WORDS (AVK_N_GROUPS * AVK_N_FIELDS)
#define AVK_LB_LABEL_BYTES (AVK_LB_WORDS * 8) /* one label's 64-bit sums in LDS */
#define AVK_LB_MASK_WORDS 4                                     /* mask words a lane keeps in registers for one launch's block of labels ... */
#define AVK_LB_MASK_BLOCK_MAX (32 * (AVK_LB_MASK_WORDS - 1) + 1) /* ... which therefore holds at most 97 labels, wherever it starts in its first word (160 KB of LDS: 71) */

namespace avk {
namespace lb {

typedef dp::u8 u8;
typedef dp::u32 u32;
typedef dp::u64 u64;

/* the device view of a solved batch: the caller's arrays as the packer keeps them (wide, or the packed source) and the kernels' compact outputs */
struct LbView {
    dp::DpIn in;
    const dp::DpVarInfo *vinfo; /* [n_variants] alt_ed per call */
    const u32 *region_out;      /* [n][4] word 0: status */
    const u32 *var_out;         /* per-call words: expected | observed << 8 | class << 16 | zygosity << 24 */
    const u32 *v_off;           /* [n] first per-call word of a region: truth calls, then query calls */
    const u32 *bp_off, *bp;     /* [n + 1], [groups][4]: the joint group, then one per call type of the region in type order */
};

/* GroupMetrics::add_truth_zygosity (grouped_metrics.rs:183-227) over one side's calls of group g (0: every call; 1 + type: that type's), and the side's
 * sum of copies(zygosity) x raw_space */
struct LbSide {
    u32 gt_tp, gt_fn, gt_fn_gt, hap_tp, hap_fn, w_tp, w_fn;
    u64 tot;
};
/* one call's contribution to them: its per-call word x (truth or query entry) and its alt_ed w.  One iteration of lb_side; avk_sizebin.inl keys the same seven
 * values by the call's size */
struct LbCall {
    u32 gt_tp, gt_fn, gt_fn_gt, hap_tp, hap_fn, w_tp, w_fn;
};
AVK_DEV LbCall lb_call(u32 x, bool query, u64 w) {
    const u32 ea = x & 0xFFu, oa = (x >> 8) & 0xFFu;
    /* the query entries are stored toggled (compare_benchmark.rs:109-123): scored as truth they expected var_observed and observed var_expected */
    const u32 exp = query ? oa : ea, obs = query ? ea : oa;
    LbCall k;
    k.hap_tp = obs;
    k.hap_fn = exp - obs;
    k.w_tp = (u32)((u64)obs * w);
    k.w_fn = (u32)((u64)(u32)(exp - obs) * w);
    k.gt_tp = exp == obs ? 1u : 0u;
    k.gt_fn = exp == obs ? 0u : 1u;
    k.gt_fn_gt = (exp != obs && obs > 0) ? 1u : 0u;
    return k;
}
AVK_DEV LbSide lb_side(const LbView &v, u64 off, u32 cnt, const u32 *vw, bool query, u32 g) {
    LbSide s;
    s.gt_tp = s.gt_fn = s.gt_fn_gt = s.hap_tp = s.hap_fn = s.w_tp = s.w_fn = 0;
    s.tot = 0;
    for (u32 i = 0; i < cnt; ++i) {
        const u64 c = off + i;
        const u32 vt = v.in.type_of(c);
        if (g != 0 && g != 1u + vt) continue;
        const LbCall k = lb_call(vw[i], query, v.vinfo[c].alt_ed);
        s.hap_tp += k.hap_tp;
        s.hap_fn += k.hap_fn;
        s.w_tp += k.w_tp;
        s.w_fn += k.w_fn;
        s.gt_tp += k.gt_tp;
        s.gt_fn += k.gt_fn;
        s.gt_fn_gt += k.gt_fn_gt;
        const u32 z = v.in.zyg_of(c);
        const u64 cz = z == AVK_ZYG_HOM_ALT ? 2u : ((z >= AVK_ZYG_UNPHASED_HET && z <= AVK_ZYG_PHASED_HET10) ? 1u : 0u);
        s.tot += cz * (u64)v.in.raw_of(c, v.in.a0_len_of(c), v.in.a1_len_of(c));
    }
    return s;
}

/* The GroupTypeMetrics of region r, one group at a time: emit(g, F) with the group's AVK_N_FIELDS counters, for g in {0} and {1 + type : the type occurs among
 * the region's calls}, in that order — the order of the region's compact BASEPAIR groups.  Exactly avk_group_metrics_from_compact, 32-bit truncations
 * included.  A group's calls are walked once per group instead of keeping 13 x 22 counters per lane. */
template <class Emit>
AVK_DEV void lb_region_groups(const LbView &v, u64 r, Emit &&emit) {
    const u32 tc = v.in.t_cnt_of(r), qc = v.in.q_cnt_of(r);
    const u64 toff = v.in.t_off_of(r), qoff = v.in.q_off_of(r), nv = v.in.n_variants;
    if (toff > nv || (u64)tc > nv - toff || qoff > nv || (u64)qc > nv - qoff) return;
    const u32 *vw = v.var_out + v.v_off[r];
    u32 types = 0;
    for (u32 i = 0; i < tc; ++i) types |= 1u << (v.in.type_of(toff + i) & 15u);
    for (u32 i = 0; i < qc; ++i) types |= 1u << (v.in.type_of(qoff + i) & 15u);
    types &= (1u << AVK_N_VARIANT_TYPES) - 1u;
    u32 k = v.bp_off[r];
    const u32 hi = v.bp_off[r + 1];
    for (u32 left = 1u | (types << 1); left && k < hi; left &= left - 1, ++k) {
        const u32 g = (u32)__builtin_ctz(left);
        const LbSide T = lb_side(v, toff, tc, vw, false, g), Q = lb_side(v, qoff, qc, vw + tc, true, g);
        const avk_u4 bp = *(const avk_u4 *)(v.bp + 4 * (u64)k);
        u32 F[AVK_N_FIELDS];
        F[AVK_F_GT_TRUTH_TP] = T.gt_tp, F[AVK_F_GT_TRUTH_FN] = T.gt_fn, F[AVK_F_GT_TRUTH_FN_GT] = T.gt_fn_gt;
        F[AVK_F_GT_QUERY_TP] = Q.gt_tp, F[AVK_F_GT_QUERY_FP] = Q.gt_fn, F[AVK_F_GT_QUERY_FP_GT] = Q.gt_fn_gt;
        F[AVK_F_HAP_TRUTH_TP] = T.hap_tp, F[AVK_F_HAP_TRUTH_FN] = T.hap_fn, F[AVK_F_HAP_QUERY_TP] = Q.hap_tp, F[AVK_F_HAP_QUERY_FP] = Q.hap_fn;
        F[AVK_F_WHAP_TRUTH_TP] = T.w_tp, F[AVK_F_WHAP_TRUTH_FN] = T.w_fn, F[AVK_F_WHAP_QUERY_TP] = Q.w_tp, F[AVK_F_WHAP_QUERY_FP] = Q.w_fn;
        /* BASEPAIR from the compact group; RECORD_BP from it and the totals (waffle_solver.rs:455-522) */
        F[AVK_F_BP_TRUTH_TP] = bp.x, F[AVK_F_BP_TRUTH_FN] = bp.y, F[AVK_F_BP_QUERY_TP] = bp.z, F[AVK_F_BP_QUERY_FP] = bp.w;
        F[AVK_F_RBP_TRUTH_TP] = (u32)(2 * T.tot - bp.y);
        F[AVK_F_RBP_TRUTH_FN] = bp.y;
        F[AVK_F_RBP_QUERY_TP] = (u32)(2 * Q.tot - bp.w);
        F[AVK_F_RBP_QUERY_FP] = bp.w;
        emit(g, F);
    }
}

/* One lane: region r into the sums of the labels [label_lo, label_hi) its list names — acc[(l - label_lo) * AVK_LB_WORDS + g * AVK_N_FIELDS + f], 64-bit, added
 * with add(p, x) (an LDS atomic on the device).  Only solved regions count; a label named twice counts twice. */
template <class Add>
AVK_DEV void lb_region_labels(const LbView &v, u64 r, const u64 *label_off, const u32 *label_idx, u32 label_lo, u32 label_hi, u64 *acc, Add &&add) {
    if (v.region_out[4 * r] != 0) return;
    const u64 lo = label_off[r], hi = label_off[r + 1];
    bool any = false;
    for (u64 q = lo; q < hi; ++q) {
        const u32 l = label_idx[q];
        any = any || (l >= label_lo && l < label_hi);
    }
    if (!any) return;
    lb_region_groups(v, r, [&](u32 g, const u32(&F)[AVK_N_FIELDS]) {
        for (u64 q = lo; q < hi; ++q) {
            const u32 l = label_idx[q];
            if (l < label_lo || l >= label_hi) continue;
            u64 *dst = acc + (u64)(l - label_lo) * AVK_LB_WORDS + g * AVK_N_FIELDS;
#pragma unroll
            for (int f = 0; f < AVK_N_FIELDS; ++f)
                if (F[f]) add(dst + f, F[f]);
        }
    });
}

/* The same lane with the region's labels as BIT MASKS: bit (l & 31) of mask[(l >> 5) * n + r] says region r of n is in label l (sx_mask_at's layout).  The block
 * [label_lo, label_hi), at most AVK_LB_MASK_BLOCK_MAX labels, lies in words label_lo >> 5 .. (label_hi - 1) >> 5; each is read once into a register — the lanes of
 * a wave read consecutive words — and the two edge words are cut to the block, which ends on a word only by chance.  A region whose words are all zero reads
 * nothing else, not even its status.  Set bits are walked lowest first: the order of a list made from the same masks (sx_fill_region), and the same sums. */
template <class Add>
AVK_DEV void lb_region_labels_mask(const LbView &v, u64 r, const u32 *mask, u64 n, u32 label_lo, u32 label_hi, u64 *acc, Add &&add) {
    if (label_hi <= label_lo) return;
    const u32 w_lo = label_lo >> 5, w_hi = (label_hi - 1u) >> 5;
    u32 x[AVK_LB_MASK_WORDS];
    u32 any = 0;
#pragma unroll
    for (u32 j = 0; j < AVK_LB_MASK_WORDS; ++j) {
        const u32 w = w_lo + j;
        u32 m = 0;
        if (w <= w_hi) {
            m = mask[(u64)w * n + r];
            if (w == w_lo) m &= ~0u << (label_lo & 31u);
            if (w == w_hi && (label_hi & 31u)) m &= ~0u >> (32u - (label_hi & 31u));
        }
        x[j] = m;
        any |= m;
    }
    if (!any || v.region_out[4 * r] != 0) return;
    lb_region_groups(v, r, [&](u32 g, const u32(&F)[AVK_N_FIELDS]) {
#pragma unroll
        for (u32 j = 0; j < AVK_LB_MASK_WORDS; ++j)
            for (u32 m = x[j]; m; m &= m - 1u) {
                const u32 l = ((w_lo + j) << 5) + (u32)__builtin_ctz(m);
                u64 *dst = acc + (u64)(l - label_lo) * AVK_LB_WORDS + g * AVK_N_FIELDS;
#pragma unroll
                for (int f = 0; f < AVK_N_FIELDS; ++f)
                    if (F[f]) add(dst + f, F[f]);
            }
    });
}

} // namespace lb
} // namespace avk

#ifndef AVK_EMU
/* Labels [label_lo, label_hi) of one launch: the workgroup's LDS holds their sums (the host sizes the block of labels from the LDS the launch gets,
 * avk_label_block), every lane takes regions of its own, the sums are flushed once per workgroup.  Reads per region: status, its list, and for a region with a
 * label of this launch its calls' words and groups — never a 13 x 22 block. */
__global__ void __launch_bounds__(1024) avk_label_tally_compact_kernel(avk::lb::LbView v, const unsigned long long *label_off, const uint32_t *label_idx, uint32_t n_regions,
                                                                       uint32_t label_lo, uint32_t label_hi, unsigned long long *out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char avk_smem[];
    unsigned long long *acc = (unsigned long long *)avk_smem;
    const unsigned words = (label_hi - label_lo) * AVK_LB_WORDS;
    for (unsigned k = threadIdx.x; k < words; k += blockDim.x) acc[k] = 0;
    __syncthreads();
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_regions; r += step)
        avk::lb::lb_region_labels(v, r, (const uint64_t *)label_off, label_idx, label_lo, label_hi, (uint64_t *)acc,
                                  [](uint64_t *p, uint32_t x) { atomicAdd((unsigned long long *)p, (unsigned long long)x); });
    __syncthreads();
    for (unsigned k = threadIdx.x; k < words; k += blockDim.x) {
        const unsigned long long x = acc[k];
        if (x) atomicAdd(out + (size_t)(label_lo + k / AVK_LB_WORDS) * AVK_TALLY_LEN + k % AVK_LB_WORDS, x);
    }
}

/* The same launch for a batch whose labels are the strata pass's bit masks (mask[w * n_regions + r]): same block of labels in LDS, same lanes, same flush; per
 * region the status and at most AVK_LB_MASK_WORDS mask words — no offsets, no index array. */
__global__ void __launch_bounds__(1024) avk_label_tally_mask_kernel(avk::lb::LbView v, const uint32_t *mask, uint32_t n_regions, uint32_t label_lo, uint32_t label_hi,
                                                                    unsigned long long *out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char avk_smem[];
    unsigned long long *acc = (unsigned long long *)avk_smem;
    const unsigned words = (label_hi - label_lo) * AVK_LB_WORDS;
    for (unsigned k = threadIdx.x; k < words; k += blockDim.x) acc[k] = 0;
    __syncthreads();
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_regions; r += step)
        avk::lb::lb_region_labels_mask(v, r, mask, n_regions, label_lo, label_hi, (uint64_t *)acc,
                                       [](uint64_t *p, uint32_t x) { atomicAdd((unsigned long long *)p, (unsigned long long)x); });
    __syncthreads();
    for (unsigned k = threadIdx.x; k < words; k += blockDim.x) {
        const unsigned long long x = acc[k];
        if (x) atomicAdd(out + (size_t)(label_lo + k / AVK_LB_WORDS) * AVK_TALLY_LEN + k % AVK_LB_WORDS, x);
    }
}
#endif

#endif /* AVK_LABELS_INL */
