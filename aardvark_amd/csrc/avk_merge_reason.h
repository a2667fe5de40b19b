/*
 * avk_merge_reason.h — the numbering of MergeSummaryWriter's merge reasons (src/writers/merge_summary.rs:12-18), ONE function for the host's
 * avk_merge_counts_esc (avk_shard_host.inl), the public avk_merge_counts_reason and the count kernel (avk_mergecount.inl).
 *
 * The reasons are numbered in the order of the reference's derive(Ord) — Different, NoConflict{mask 0 .. 2^k - 1}, MajorityAgree{mask},
 * ConflictSelection{index 0 .. k - 1}, BasepairIdentical — so a job's dense block has 2 + 2 * 2^k + k reasons, each with AVK_N_VARIANT_TYPES types, k inputs and
 * a (pass, fail) pair: entry ((reason * AVK_N_VARIANT_TYPES + type) * k + input) * 2 + (0 pass | 1 fail).
 */
#ifndef AVK_MERGE_REASON_H
#define AVK_MERGE_REASON_H

#include <stdint.h>

#include "../../include/aardvark_amd.h"

#if defined(__HIPCC__) && !defined(AVK_EMU)
#define AVK_MR_HD __host__ __device__ static inline
#else
#define AVK_MR_HD static inline
#endif

namespace avk {
namespace mc {

AVK_MR_HD uint32_t merge_reason(uint32_t n_inputs, uint8_t classification, uint64_t members) {
    const uint32_t masks = 1u << n_inputs;
    switch (classification) {
    case AVK_MERGE_DIFFERENT: return 0;
    case AVK_MERGE_NO_CONFLICT: return 1 + (uint32_t)(members & (masks - 1));
    case AVK_MERGE_MAJORITY_AGREE: return 1 + masks + (uint32_t)(members & (masks - 1));
    case AVK_MERGE_CONFLICT_SELECTION: return 1 + 2 * masks + (uint32_t)(members < n_inputs ? members : 0);
    default: return 1 + 2 * masks + n_inputs; /* AVK_MERGE_IDENTICAL */
    }
}

/* words of the dense block for k inputs (avk_merge_counts_len without its refusal of k outside [2, AVK_MERGE_COUNTS_MAX_INPUTS]) */
AVK_MR_HD uint64_t merge_counts_words(uint32_t n_inputs) { return (2 + 2 * (1ull << n_inputs) + n_inputs) * AVK_N_VARIANT_TYPES * n_inputs * 2; }

} // namespace mc
} // namespace avk

#endif /* AVK_MERGE_REASON_H */
