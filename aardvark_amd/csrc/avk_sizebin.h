/*
 * avk_sizebin.h — the rule of the per-call size bins, ONE statement for the host (include/aardvark_amd.h: avk_size_n_bins, avk_size_bin_name,
 * avk_size_tallies_host) and the device (avk_sizebin.inl), the way avk_boot.h is shared.  The reference has no such table; this is the project's own.
 *
 *   size     size(call) = |a1_len - a0_len|: the net length change of the call as the batch holds it (after the feeder's trimming, escaped lengths resolved).
 *            SNVs and balanced substitutions are size 0.
 *   spec     n_edges ascending edges, 1 <= n_edges <= AVK_SIZE_EDGES_MAX, edges[0] >= 1, strictly ascending; n_bins = n_edges + 1
 *   bin      bin 0: size < edges[0]; bin j: edges[j - 1] <= size < edges[j]; the last bin: size >= edges[n_edges - 1] — the number of edges that are <= size
 *   block    out[((scope * n_bins + bin) * AVK_N_GROUPS + g) * AVK_SIZE_FIELDS + f], 64-bit, f the fields AVK_F_GT_TRUTH_TP .. AVK_F_WHAP_QUERY_FP in enum order
 *            (GT, HAP and WEIGHTED_HAP: BASEPAIR and RECORD_BP are properties of a region's haplotypes and belong to no single call)
 *
 * Plain C: no includes beyond <stdint.h>, no state.
 */
#ifndef AVK_SIZEBIN_H
#define AVK_SIZEBIN_H

#include <stdint.h>

#if defined(__HIPCC__) && !defined(AVK_EMU)
#define AVK_SIZE_FN __host__ __device__ static inline
#else
#define AVK_SIZE_FN static inline
#endif

#define AVK_SIZE_EDGES_MAX 15 /* 1 <= n_edges <= this: at most 16 bins */
#define AVK_SIZE_FIELDS 14    /* AVK_F_GT_TRUTH_TP .. AVK_F_WHAP_QUERY_FP */
#define AVK_SIZE_VALUES 7     /* a call's contribution: gt_tp, gt_fn, gt_fn_gt, hap_tp, hap_fn, w_tp, w_fn — to the truth fields of its side or to the query fields */

typedef struct avk_size_spec {
    uint32_t n_edges;
    uint32_t edges[AVK_SIZE_EDGES_MAX];
} avk_size_spec;

/* 1: the spec is one the rule accepts */
AVK_SIZE_FN int avk_size_spec_ok(const avk_size_spec *s) {
    if (!s || s->n_edges < 1 || s->n_edges > AVK_SIZE_EDGES_MAX || s->edges[0] < 1) return 0;
    for (uint32_t k = 1; k < s->n_edges; ++k)
        if (s->edges[k] <= s->edges[k - 1]) return 0;
    return 1;
}
AVK_SIZE_FN uint32_t avk_size_of(uint32_t a0_len, uint32_t a1_len) { return a1_len > a0_len ? a1_len - a0_len : a0_len - a1_len; }
/* the number of edges <= size.  Every index is static (the loop is unrolled over the struct's capacity): in a kernel the spec stays in scalar registers */
AVK_SIZE_FN uint32_t avk_size_bin_of(const avk_size_spec *s, uint32_t size) {
    uint32_t bin = 0;
#if defined(__HIPCC__) || defined(__clang__)
#pragma unroll
#endif
    for (int k = 0; k < AVK_SIZE_EDGES_MAX; ++k) bin += ((uint32_t)k < s->n_edges && size >= s->edges[k]) ? 1u : 0u;
    return bin;
}
/* bin j holds the sizes lo .. hi, both inclusive; the last bin has no upper bound (*hi = 0xFFFFFFFF) */
AVK_SIZE_FN void avk_size_bin_bounds(const avk_size_spec *s, uint32_t j, uint32_t *lo, uint32_t *hi) {
    *lo = j == 0 ? 0u : s->edges[j - 1];
    *hi = j >= s->n_edges ? 0xFFFFFFFFu : s->edges[j] - 1u;
}
/* the field a value of the contribution lands in: value k (0 .. 6) of a truth call (query = 0) or a query call, in the AVK_F_* order of include/aardvark_amd.h:
 * truth 0 1 4 | 6 7 | 10 11, query 2 3 5 | 8 9 | 12 13 (GT tp, fn, fn_gt | HAP tp, fn | WEIGHTED_HAP tp, fn) */
AVK_SIZE_FN uint32_t avk_size_field_of(uint32_t k, int query) {
    return k < 2 ? (query ? 2u : 0u) + k : k == 2 ? (query ? 5u : 4u) : k < 5 ? (query ? 8u : 6u) + (k - 3u) : (query ? 12u : 10u) + (k - 5u);
}

#endif /* AVK_SIZEBIN_H */
