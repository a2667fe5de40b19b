/*
 * avk_callboot_host.h — the host routes of the per-call tallies' bootstrap replicates (avk_size_boot_tallies_host, avk_kind_boot_tallies_host of
 * include/aardvark_amd.h), as a header: plain host C++ with no GPU call, so that a program of its own can run the very code under a sanitizer
 * (tests/native/callboot_check.cpp).  avk_host.hip checks the arguments (the spec, the cap, the label lists) and then calls callboot_host_sum; the per-call
 * contribution host_call_values is the one avk_size_tallies_host and avk_kind_tallies_host use.  The rule: avk_callboot.h.
 */
#ifndef AVK_CALLBOOT_HOST_H
#define AVK_CALLBOOT_HOST_H

#include <stdint.h>

#include <thread>
#include <utility>
#include <vector>

#include "../../include/aardvark_amd.h"
#include "avk_callboot.h"

namespace avk {
namespace cbh {

/* Variant::alt_ed of two alleles (avk_edit_distance's rule) */
typedef uint64_t (*EditDistance)(const uint8_t *a, uint64_t a_len, const uint8_t *b, uint64_t b_len);

/* a call's contribution on the host, shared by every per-call host route: one iteration of lb_side (avk_labels.inl) for call v of side `side` (0 truth, 1 query: the
 * query entries are stored toggled) with alt_ed w — the seven values of avk_sizebin.h */
static inline void host_call_values(const avk_result_batch *res, bool wide_calls, uint64_t v, int side, uint64_t w, uint32_t (&val)[AVK_SIZE_VALUES]) {
    const uint32_t ea = wide_calls ? res->var_expected[v] : avk_vp_expected(res->var_packed[v]), oa = wide_calls ? res->var_observed[v] : avk_vp_observed(res->var_packed[v]);
    const uint32_t exp = side == 0 ? ea : oa, obs = side == 0 ? oa : ea;
    val[0] = exp == obs ? 1u : 0u, val[1] = exp == obs ? 0u : 1u, val[2] = (exp != obs && obs > 0) ? 1u : 0u, val[3] = obs, val[4] = exp - obs;
    val[5] = (uint32_t)((uint64_t)obs * w), val[6] = (uint32_t)((uint64_t)(uint32_t)(exp - obs) * w);
}

/* out[AVK_CALLBOOT_AT(scope, B, b, n_keys, key, g, f)] gains the sums.  The caller has checked: the family's spec, 1 <= B, the cap, out, the results' arrays (status
 * or region_packed; var_expected and var_observed, or var_packed), the batch's start array, and lab (NULL: scope 0 only; its offsets ascending, its indices below
 * n_labels).  threads: host threads, at most 64, and no more than keep every thread's block of sums within 1 GiB together.  Returns 0, or 1 when a region's calls
 * lie outside the batch (out is then untouched). */
static inline int callboot_host_sum(const avk_region_batch *b, const avk_result_batch *res, int family, const avk_size_spec *sp, const avk_boot_spec *bs, const avk_region_labels *lab,
                                    uint32_t threads, uint64_t *out, EditDistance edit_distance) {
    const uint32_t n_labels = lab ? lab->n_labels : 0;
    const bool wide_calls = res->var_expected && res->var_observed;
    const uint64_t n = b->n_regions;
    const uint32_t B = bs->replicates, n_keys = avk_callboot_n_keys(family, sp);
    const size_t rep_words = (size_t)n_keys * AVK_CALLBOOT_KEY_WORDS, words = ((size_t)n_labels + 1) * B * rep_words;
    uint32_t T = threads < 1 ? 1u : (threads > 64u ? 64u : threads);
    while (T > 1 && (uint64_t)T * words * 8 > (1ull << 30)) --T;
    std::vector<std::vector<uint64_t>> part(T);
    std::vector<int> bad(T, 0);
    auto work = [&](uint32_t t) {
        std::vector<uint64_t> &acc = part[t];
        acc.assign(words, 0);
        std::vector<std::pair<uint32_t, uint32_t>> X; /* X_r, sparse: (word of a replicate's block — below 16 x 182 —, value) */
        std::vector<uint8_t> w(B);
        for (uint64_t r = n * t / T; r < n * (t + 1) / T; ++r) {
            const uint32_t status = res->status ? (uint32_t)res->status[r] : (uint32_t)avk_rp_status(res->region_packed[r]);
            if (status != 0) continue;
            X.clear();
            for (int side = 0; side < 2; ++side) {
                const uint64_t off = side == 0 ? b->t_off[r] : b->q_off[r];
                const uint32_t cnt = side == 0 ? b->t_cnt[r] : b->q_cnt[r];
                if (off > b->n_variants || cnt > b->n_variants - off) {
                    bad[t] = 1;
                    return;
                }
                for (uint32_t i = 0; i < cnt; ++i) {
                    const uint64_t v = off + i;
                    const uint32_t vt = b->var_type[v], l0 = b->a0_len[v], l1 = b->a1_len[v];
                    const uint64_t ed = edit_distance(b->allele_bytes + b->a0_off[v], l0, b->allele_bytes + b->a1_off[v], l1);
                    uint32_t val[AVK_SIZE_VALUES];
                    host_call_values(res, wide_calls, v, side, ed, val);
                    uint32_t key;
                    if (family == AVK_CALLBOOT_KIND) {
                        const bool bytes = l0 == 1u && l1 == 1u && b->a0_off[v] < b->allele_bytes_len && b->a1_off[v] < b->allele_bytes_len;
                        const uint32_t sub = bytes ? avk_kind_sub_of(1u, 1u, b->allele_bytes[b->a0_off[v]], b->allele_bytes[b->a1_off[v]]) : (uint32_t)AVK_KIND_SUB_OTHER;
                        key = avk_kind_of(avk_kind_gt_of(b->var_zyg[v]), sub);
                    } else
                        key = avk_size_bin_of(sp, avk_size_of(l0, l1));
                    for (uint32_t g : {0u, 1u + vt}) {
                        if (g >= AVK_N_GROUPS) continue;
                        for (uint32_t k = 0; k < AVK_SIZE_VALUES; ++k)
                            if (val[k]) X.emplace_back((uint32_t)AVK_CALLBOOT_AT(0, 1, 0, n_keys, key, g, avk_size_field_of(k, side)), val[k]);
                    }
                }
            }
            if (X.empty()) continue;
            const uint64_t h = avk_boot_region_hash(bs->seed, avk_boot_key(b->contig_idx ? b->contig_idx[r] : 0u, (uint32_t)b->start[r]));
            for (uint32_t k = 0; k < B; ++k) w[k] = (uint8_t)avk_boot_weight_of_hash(h, k);
            auto add = [&](uint32_t scope) {
                for (uint32_t k = 0; k < B; ++k) {
                    if (!w[k]) continue;
                    uint64_t *dst = acc.data() + ((size_t)scope * B + k) * rep_words;
                    for (const auto &x : X) dst[x.first] += (uint64_t)w[k] * x.second;
                }
            };
            add(0);
            if (n_labels)
                for (uint64_t q = lab->label_off[r]; q < lab->label_off[r + 1]; ++q) add(1u + lab->label_idx[q]);
        }
    };
    std::vector<std::thread> pool;
    for (uint32_t t = 1; t < T; ++t) pool.emplace_back(work, t);
    work(0);
    for (std::thread &th : pool) th.join();
    for (uint32_t t = 0; t < T; ++t)
        if (bad[t]) return 1;
    for (uint32_t t = 0; t < T; ++t)
        for (size_t k = 0; k < words; ++k) out[k] += part[t][k];
    return 0;
}

} // namespace cbh
} // namespace avk

#endif /* AVK_CALLBOOT_HOST_H */
