/*
 * avk_callboot.h — the rule of the bootstrap replicates of the PER-CALL blocks, ONE statement for the host (include/aardvark_amd.h:
 * avk_size_boot_tallies_host, avk_kind_boot_tallies_host) and the device (avk_callboot.inl), the way avk_boot.h and avk_sizebin.h state theirs.  No new
 * randomness: a replicate weighs a region's contribution to a keyed block with the weight the tallies' replicates give that region.
 *
 *   family   AVK_CALLBOOT_SIZE: key = the call's size bin under a spec (avk_sizebin.h), n_keys = n_edges + 1;
 *            AVK_CALLBOOT_KIND: key = the call's kind (avk_callkind.h), n_keys = AVK_N_KINDS
 *   X_r      region r's contribution to avk_size_tallies' block (key = bin) or avk_kind_tallies' block (key = kind): the seven values of each of its calls, to the
 *            truth or the query fields of group 0 and group 1 + type.  Every refusal of those stages applies: an unsolved region and a region whose call ranges
 *            lie outside the batch add nothing; a call type beyond the table counts in the joint group only
 *   w        avk_boot_weight(seed, contig_idx(r), start(r), b) of avk_boot.h, unchanged: the same seed gives a region the same weight here and in avk_boot_tallies
 *   rule     out[scope][b][key][g][f] = sum over the scope's solved regions r of w(r, b) * X_r[key][g][f]
 *   block    out[AVK_CALLBOOT_AT(scope, B, b, n_keys, key, g, f)], 64-bit words that are ADDED to; scope 0: every region; scope 1 + l: label l
 *   cap      (1 + labels) * B * n_keys <= AVK_CALLBOOT_MAX_BLOCKS blocks of AVK_CALLBOOT_BLOCK_BYTES; 1 <= B <= AVK_BOOT_MAX_REPLICATES
 *   law      replicate b summed over its keys is words g * AVK_N_FIELDS + f, f < 14, of replicate b of avk_boot_tallies, for the same seed
 *
 * Plain C: no includes beyond <stdint.h> and the three rule headers, no state.
 */
#ifndef AVK_CALLBOOT_H
#define AVK_CALLBOOT_H

#include <stdint.h>

#include "avk_boot.h"
#include "avk_callkind.h"
#include "avk_sizebin.h"

#ifndef AVK_N_GROUPS
#define AVK_N_GROUPS 13 /* include/aardvark_amd.h: the joint group and one per call type (avk_host.hip checks the number at compile time) */
#endif

enum { AVK_CALLBOOT_SIZE = 0, AVK_CALLBOOT_KIND = 1 };

#define AVK_CALLBOOT_KEY_WORDS (AVK_N_GROUPS * AVK_SIZE_FIELDS)  /* the 64-bit words of one (scope, replicate, key): 182 */
#define AVK_CALLBOOT_BLOCK_BYTES (AVK_CALLBOOT_KEY_WORDS * 8)    /* 1,456 */
#define AVK_CALLBOOT_MAX_BLOCKS 262144u                          /* (scope, replicate, key) blocks of a call: 381.7 MB of sums; 1000 replicates x 9 kinds x 17 scopes
                                                                    are 153,000 */
/* the word of (scope, replicate b of B, key of n_keys, group g, field f) */
#define AVK_CALLBOOT_AT(scope, B, b, n_keys, key, g, f) \
    ((((((uint64_t)(scope) * (B) + (b)) * (n_keys) + (key)) * AVK_N_GROUPS + (g)) * AVK_SIZE_FIELDS) + (f))

/* the keys of a family (0: the family or its spec is not one the rule accepts).  spec is read for AVK_CALLBOOT_SIZE only */
AVK_SIZE_FN uint32_t avk_callboot_n_keys(int family, const avk_size_spec *spec) {
    if (family == AVK_CALLBOOT_KIND) return (uint32_t)AVK_N_KINDS;
    if (family == AVK_CALLBOOT_SIZE && avk_size_spec_ok(spec)) return spec->n_edges + 1u;
    return 0u;
}
/* 1: n_scopes scopes of B replicates of n_keys keys are within the cap */
AVK_SIZE_FN int avk_callboot_blocks_ok(uint64_t n_scopes, uint64_t B, uint64_t n_keys) {
    return n_scopes >= 1 && B >= 1 && B <= AVK_BOOT_MAX_REPLICATES && n_keys >= 1 && n_keys <= 16 && n_scopes <= AVK_CALLBOOT_MAX_BLOCKS &&
           n_scopes * B * n_keys <= AVK_CALLBOOT_MAX_BLOCKS;
}

#endif /* AVK_CALLBOOT_H */
