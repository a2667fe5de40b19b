/*
 * avk_score.h — the rule of the precision-recall curve by query score, ONE statement for the host (include/aardvark_amd.h:
 * avk_score_n_points, avk_score_point_name, avk_score_tallies_host) and the device (avk_score.inl), the way avk_sizebin.h is shared.  The reference has no such
 * table; this is the project's own.  The job is solved ONCE and the curve is derived from that one comparison: it approximates K filtered re-runs.
 *
 *   score    a float per call of the batch, scores[n_variants], indexed like the batch's call arrays; only query entries are read; NaN: missing
 *   spec     n_thresholds finite, strictly ascending thresholds, 1 <= n_thresholds <= AVK_SCORE_THRESHOLDS_MAX; n_points = n_thresholds + 1;
 *            point 0: no filter; point k >= 1: score >= t[k - 1]
 *   bin      of a query call: the number of thresholds <= score, compared in float32 with >= (NaN: 0, +inf: n_thresholds, -inf: 0); the call is kept at the
 *            points 0 .. bin.  Of a truth call: n_thresholds when its observed count is 0 (no filter changes such a call); otherwise the MINIMUM bin over the
 *            query calls of its region with hap_tp > 0 (lb_call's toggled reading), n_thresholds when the region has none — the region's haplotype match needs
 *            all of its matching query calls
 *   point k  a query call with k <= bin adds lb_call's seven values to the query fields, with k > bin nothing (a filtered call is neither TP nor FP); a truth
 *            call with k <= bin adds the same seven values to the truth fields, with k > bin its LOST values: gt_fn = 1, hap_fn = exp, w_fn = (u32)(exp * alt_ed),
 *            0 in the other four — to group 0 and group 1 + type (a type beyond the table: group 0 only), in scope 0 and scope 1 + l for every label l of the region
 *   block    out[((scope * n_points + k) * AVK_N_GROUPS + g) * AVK_SCORE_FIELDS + f], 64-bit, f = AVK_F_GT_TRUTH_TP .. AVK_F_WHAP_QUERY_FP (avk_size_field_of)
 *
 * A histogram BIN (where a call stops being kept) is not a curve POINT (a filter): curve[k] = sum of H[bin >= k], plus sum of Lost[bin < k] in the truth-FN fields.
 *
 * Plain C: no includes beyond <stdint.h> and avk_sizebin.h, no state.
 */
#ifndef AVK_SCORE_H
#define AVK_SCORE_H

#include <stdint.h>

#include "avk_sizebin.h"

/* (forced inline in a kernel: a call would put the spec, whose address it takes, into scratch memory) */
#if defined(__HIPCC__) && !defined(AVK_EMU)
#define AVK_SCORE_FN __host__ __device__ static inline __attribute__((always_inline))
#else
#define AVK_SCORE_FN static inline
#endif

#define AVK_SCORE_THRESHOLDS_MAX 31 /* 1 <= n_thresholds <= this: at most 32 points, a point a lane of half a wave */
#define AVK_SCORE_FIELDS 14         /* AVK_F_GT_TRUTH_TP .. AVK_F_WHAP_QUERY_FP */
#define AVK_SCORE_LOST 3            /* a lost truth call's values: gt_fn, hap_fn, w_fn */

/* the histograms of one scope, on the device (avk_score.inl) and on the host (avk_score_host.h): H[bin][g][14], the normal values, then Lost[bin][g][3], the lost
 * values of truth calls with observed > 0 — in 64-bit words; AVK_SC_H_WORDS is also one scope of the curve's block.  (AVK_N_GROUPS: include/aardvark_amd.h) */
#define AVK_SC_H_WORDS(n_points) ((n_points) * AVK_N_GROUPS * AVK_SCORE_FIELDS)   /* a scope's histogram of normal values ... */
#define AVK_SC_LOST_WORDS(n_points) ((n_points) * AVK_N_GROUPS * AVK_SCORE_LOST)  /* ... and of lost values behind it */
#define AVK_SC_BLOCK_WORDS(n_points) (AVK_SC_H_WORDS(n_points) + AVK_SC_LOST_WORDS(n_points))

typedef struct avk_score_spec {
    uint32_t n_thresholds;
    float t[AVK_SCORE_THRESHOLDS_MAX];
} avk_score_spec;

/* x is neither NaN nor an infinity (x - x is NaN for all three) */
AVK_SCORE_FN int avk_score_finite(float x) { return x - x == 0.0f; }
/* 1: the spec is one the rule accepts.  Every index is static (the loop is unrolled over the struct's capacity): in a kernel the spec stays in scalar registers */
AVK_SCORE_FN int avk_score_spec_ok(const avk_score_spec *s) {
    if (!s || s->n_thresholds < 1 || s->n_thresholds > AVK_SCORE_THRESHOLDS_MAX) return 0;
    int ok = avk_score_finite(s->t[0]);
#if defined(__HIPCC__) || defined(__clang__)
#pragma unroll
#endif
    for (int k = 1; k < AVK_SCORE_THRESHOLDS_MAX; ++k)
        if ((uint32_t)k < s->n_thresholds && !(avk_score_finite(s->t[k]) && s->t[k] > s->t[k - 1])) ok = 0;
    return ok;
}
/* the number of thresholds <= score: a comparison with NaN is false, so a missing score is bin 0.  Every index is static (unrolled over the capacity) */
AVK_SCORE_FN uint32_t avk_score_bin_of(const avk_score_spec *s, float score) {
    uint32_t bin = 0;
#if defined(__HIPCC__) || defined(__clang__)
#pragma unroll
#endif
    for (int k = 0; k < AVK_SCORE_THRESHOLDS_MAX; ++k) bin += ((uint32_t)k < s->n_thresholds && score >= s->t[k]) ? 1u : 0u;
    return bin;
}
/* the field lost value j (gt_fn, hap_fn, w_fn) lands in: GT_TRUTH_FN, HAP_TRUTH_FN, WHAP_TRUTH_FN */
AVK_SCORE_FN uint32_t avk_score_lost_field_of(uint32_t j) { return j == 0 ? 1u : j == 1 ? 7u : 11u; }
/* 1 + j when field f is lost value j's, else 0 */
AVK_SCORE_FN uint32_t avk_score_lost_of_field(uint32_t f) { return f == 1u ? 1u : f == 7u ? 2u : f == 11u ? 3u : 0u; }

#endif /* AVK_SCORE_H */
