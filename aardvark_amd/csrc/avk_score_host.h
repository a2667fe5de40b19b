/*
 * avk_score_host.h — the host route of the curve by query score (avk_score_tallies_host; the rule: avk_score.h) as plain C++: no HIP, no
 * state, alt_ed through a function the caller hands over.  avk_host.hip includes it behind its argument checks with avk::host_edit_distance; the sanitizer
 * program tests/native/score_check.cpp includes the same text with an edit distance of its own, so that every index this route forms — into the batch's and the
 * results' arrays, the scores, the label lists, the threads' histograms and the caller's block — is checked on blocks exactly as long as the interface says.
 *
 * Per thread a histogram pair per scope, H[bin][g][14] and Lost[bin][g][3] (avk_score.inl's layout); the threads' pairs are added and bins become points:
 * kept at the points <= bin (a suffix sum), lost at the points > bin (an exclusive prefix sum into the three truth-FN fields).
 */
#ifndef AVK_SCORE_HOST_H
#define AVK_SCORE_HOST_H

#include <stdint.h>

#include <thread>
#include <vector>

#include "../../include/aardvark_amd.h"
#include "avk_score.h"

/* 0: the curve was ADDED to out[(1 + n_labels) * n_points * AVK_N_GROUPS * AVK_SCORE_FIELDS]; 1: a region's calls lie outside the batch, or a label index is not
 * below n_labels — out untouched.  The caller has checked the spec (avk_score_spec_ok) and that the pointers are there: status or region_packed; var_expected
 * and var_observed, or var_packed; scores[n_variants]; with labels, label_off[n_regions + 1] and label_idx.  edit_distance(a, a_len, b, b_len): Variant::alt_ed */
template <class EditDistance>
static inline int avk_score_host_sum(const avk_region_batch *b, const avk_result_batch *res, const avk_score_spec *sp, const float *scores, const avk_region_labels *lab,
                                     uint32_t threads, EditDistance &&edit_distance, uint64_t *out) {
    const uint32_t n_labels = lab ? lab->n_labels : 0;
    const bool wide_calls = res->var_expected && res->var_observed;
    const uint64_t n = b->n_regions;
    const uint32_t n_points = sp->n_thresholds + 1u;
    const size_t h_words = AVK_SC_H_WORDS(n_points), block = AVK_SC_BLOCK_WORDS(n_points), words = ((size_t)n_labels + 1) * block;
    const uint32_t T = threads < 1 ? 1u : (threads > 64u ? 64u : threads); /* every thread sums into histograms of its own */
    std::vector<std::vector<uint64_t>> part(T);
    std::vector<int> bad(T, 0);
    auto work = [&](uint32_t t) {
        std::vector<uint64_t> &acc = part[t];
        acc.assign(words, 0);
        for (uint64_t r = n * t / T; r < n * (t + 1) / T; ++r) {
            const uint32_t status = res->status ? (uint32_t)res->status[r] : (uint32_t)avk_rp_status(res->region_packed[r]);
            if (status != 0) continue;
            const uint64_t toff = b->t_off[r], qoff = b->q_off[r], nv = b->n_variants;
            const uint32_t tc = b->t_cnt[r], qc = b->q_cnt[r];
            if (toff > nv || tc > nv - toff || qoff > nv || qc > nv - qoff) {
                bad[t] = 1;
                return;
            }
            if (n_labels)
                for (uint64_t q = lab->label_off[r]; q < lab->label_off[r + 1]; ++q)
                    if (lab->label_idx[q] >= n_labels) {
                        bad[t] = 1;
                        return;
                    }
            auto ea_of = [&](uint64_t v) { return wide_calls ? (uint32_t)res->var_expected[v] : (uint32_t)avk_vp_expected(res->var_packed[v]); };
            auto oa_of = [&](uint64_t v) { return wide_calls ? (uint32_t)res->var_observed[v] : (uint32_t)avk_vp_observed(res->var_packed[v]); };
            /* the region's truth bin: the minimum over its query calls with hap_tp > 0 (a query entry's hap_tp is its stored expected count: the toggled reading) */
            uint32_t tbin = sp->n_thresholds;
            for (uint32_t i = 0; i < qc; ++i)
                if (ea_of(qoff + i) > 0) {
                    const uint32_t q = avk_score_bin_of(sp, scores[qoff + i]);
                    tbin = q < tbin ? q : tbin;
                }
            for (int side = 0; side < 2; ++side) {
                const uint64_t off = side == 0 ? toff : qoff;
                const uint32_t cnt = side == 0 ? tc : qc;
                for (uint32_t i = 0; i < cnt; ++i) {
                    const uint64_t v = off + i;
                    const uint32_t vt = b->var_type[v];
                    const uint64_t w = edit_distance(b->allele_bytes + b->a0_off[v], (uint64_t)b->a0_len[v], b->allele_bytes + b->a1_off[v], (uint64_t)b->a1_len[v]);
                    const uint32_t ea = ea_of(v), oa = oa_of(v);
                    /* one iteration of lb_side (avk_labels.inl): the query entries are stored toggled */
                    const uint32_t exp = side == 0 ? ea : oa, obs = side == 0 ? oa : ea;
                    const uint32_t val[AVK_SIZE_VALUES] = {exp == obs ? 1u : 0u, exp == obs ? 0u : 1u, (exp != obs && obs > 0) ? 1u : 0u, obs, exp - obs, (uint32_t)((uint64_t)obs * w),
                                                           (uint32_t)((uint64_t)(uint32_t)(exp - obs) * w)};
                    const bool loses = side == 0 && obs > 0;
                    const uint32_t lost[AVK_SCORE_LOST] = {loses ? 1u : 0u, loses ? exp : 0u, loses ? (uint32_t)((uint64_t)exp * w) : 0u};
                    const uint32_t bin = side == 1 ? avk_score_bin_of(sp, scores[v]) : obs == 0 ? sp->n_thresholds : tbin;
                    auto add = [&](uint32_t scope) {
                        for (uint32_t g : {0u, 1u + vt}) {
                            if (g >= (uint32_t)AVK_N_GROUPS) continue;
                            uint64_t *dst = acc.data() + (size_t)scope * block + ((size_t)bin * AVK_N_GROUPS + g) * AVK_SCORE_FIELDS;
                            for (uint32_t k = 0; k < AVK_SIZE_VALUES; ++k) dst[avk_size_field_of(k, side)] += val[k];
                            uint64_t *ld = acc.data() + (size_t)scope * block + h_words + ((size_t)bin * AVK_N_GROUPS + g) * AVK_SCORE_LOST;
                            for (uint32_t k = 0; k < AVK_SCORE_LOST; ++k) ld[k] += lost[k];
                        }
                    };
                    add(0);
                    if (n_labels)
                        for (uint64_t q = lab->label_off[r]; q < lab->label_off[r + 1]; ++q) add(1u + lab->label_idx[q]);
                }
            }
        }
    };
    std::vector<std::thread> pool;
    for (uint32_t t = 1; t < T; ++t) pool.emplace_back(work, t);
    work(0);
    for (std::thread &th : pool) th.join();
    for (uint32_t t = 0; t < T; ++t)
        if (bad[t]) return 1;
    for (uint32_t t = 1; t < T; ++t)
        for (size_t k = 0; k < words; ++k) part[0][k] += part[t][k];
    /* bins to points */
    std::vector<uint64_t> lost_before(n_points, 0);
    for (uint32_t s = 0; s <= n_labels; ++s) {
        const uint64_t *H = part[0].data() + (size_t)s * block, *Lost = H + h_words;
        for (uint32_t g = 0; g < (uint32_t)AVK_N_GROUPS; ++g)
            for (uint32_t f = 0; f < AVK_SCORE_FIELDS; ++f) {
                const uint32_t lj = avk_score_lost_of_field(f);
                uint64_t kept = 0, lost_sum = 0;
                for (uint32_t k = 0; k < n_points; ++k) {
                    lost_before[k] = lost_sum;
                    if (lj) lost_sum += Lost[((size_t)k * AVK_N_GROUPS + g) * AVK_SCORE_LOST + (lj - 1u)];
                }
                for (uint32_t k = n_points; k-- > 0;) {
                    kept += H[((size_t)k * AVK_N_GROUPS + g) * AVK_SCORE_FIELDS + f];
                    out[(((size_t)s * n_points + k) * AVK_N_GROUPS + g) * AVK_SCORE_FIELDS + f] += kept + lost_before[k];
                }
            }
    }
    return 0;
}

#endif /* AVK_SCORE_HOST_H */
