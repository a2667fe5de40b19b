/*
 * avk_callkind.h — the rule of the per-call kinds, ONE statement for the host (include/aardvark_amd.h: avk_kind_n, avk_kind_name,
 * avk_kind_tallies_host) and the device (avk_callkind.inl), the way avk_sizebin.h is shared.  The reference has no such table; this is the project's own.
 *
 *   kind     kind(call) = 3 * gt + sub, AVK_N_KINDS = 9
 *   gt       from the call's INPUT zygosity (what the batch holds, not the resolved zygosity of the per-call word): 0 het for AVK_ZYG_UNPHASED_HET, _PHASED_HET01
 *            and _PHASED_HET10; 1 hom for AVK_ZYG_HOM_ALT; 2 nogt for anything else
 *   sub      from the two alleles as the batch holds them (after the feeder's trimming, escaped lengths resolved), whatever the call's type: when both are one
 *            byte long, both bytes folded to upper case (b & 0xDF) are one of A C G T and they differ, 0 ts for the pairs {A,G} and {C,T} and 1 tv otherwise;
 *            2 other for every other call — longer or empty alleles, equal bases, N, IUPAC codes, an allele offset outside the allele array
 *   names    het_ts het_tv het_other hom_ts hom_tv hom_other nogt_ts nogt_tv nogt_other
 *   block    out[((scope * AVK_N_KINDS + kind) * AVK_N_GROUPS + g) * AVK_SIZE_FIELDS + f], 64-bit; a call's contribution and the fields f are the size rule's
 *            (avk_sizebin.h: the seven values, avk_size_field_of)
 *
 * Plain C: no includes beyond <stdint.h> and avk_sizebin.h, no state.
 */
#ifndef AVK_CALLKIND_H
#define AVK_CALLKIND_H

#include <stdint.h>

#include "avk_sizebin.h"

#define AVK_KIND_FN AVK_SIZE_FN

#define AVK_N_KINDS 9
enum { AVK_KIND_GT_HET = 0, AVK_KIND_GT_HOM = 1, AVK_KIND_GT_NONE = 2, AVK_KIND_N_GT = 3 };
enum { AVK_KIND_SUB_TS = 0, AVK_KIND_SUB_TV = 1, AVK_KIND_SUB_OTHER = 2, AVK_KIND_N_SUB = 3 };

/* zyg: AVK_ZYG_* of include/aardvark_amd.h (2, 3, 4: the heterozygous ones; 5: homozygous alternate — avk_host.hip checks the numbers at compile time) */
AVK_KIND_FN uint32_t avk_kind_gt_of(uint32_t zyg) { return (zyg >= 2u && zyg <= 4u) ? (uint32_t)AVK_KIND_GT_HET : zyg == 5u ? (uint32_t)AVK_KIND_GT_HOM : (uint32_t)AVK_KIND_GT_NONE; }
/* 0 .. 3 for A C G T in either case, 4 for every other byte.  After the fold A = 0x41, C = 0x43, G = 0x47, T = 0x54 */
AVK_KIND_FN uint32_t avk_kind_base_of(uint32_t byte) {
    const uint32_t u = byte & 0xDFu;
    return u == 0x41u ? 0u : u == 0x43u ? 1u : u == 0x47u ? 2u : u == 0x54u ? 3u : 4u;
}
/* b0, b1: the first byte of either allele; read only when both lengths are 1 (pass anything otherwise) */
AVK_KIND_FN uint32_t avk_kind_sub_of(uint32_t a0_len, uint32_t a1_len, uint32_t b0, uint32_t b1) {
    if (a0_len != 1u || a1_len != 1u) return (uint32_t)AVK_KIND_SUB_OTHER;
    const uint32_t x = avk_kind_base_of(b0 & 0xFFu), y = avk_kind_base_of(b1 & 0xFFu);
    if (x > 3u || y > 3u || x == y) return (uint32_t)AVK_KIND_SUB_OTHER;
    return ((x ^ y) == 2u) ? (uint32_t)AVK_KIND_SUB_TS : (uint32_t)AVK_KIND_SUB_TV; /* A 0 <-> G 2, C 1 <-> T 3: the purines and the pyrimidines */
}
AVK_KIND_FN uint32_t avk_kind_of(uint32_t gt, uint32_t sub) { return 3u * gt + sub; }
/* the name of kind k < AVK_N_KINDS (NULL beyond) */
AVK_KIND_FN const char *avk_kind_name_of(uint32_t k) {
    return k == 0 ? "het_ts" : k == 1 ? "het_tv" : k == 2 ? "het_other" : k == 3 ? "hom_ts" : k == 4 ? "hom_tv" : k == 5 ? "hom_other" : k == 6 ? "nogt_ts" : k == 7 ? "nogt_tv"
         : k == 8 ? "nogt_other" : (const char *)0;
}

#endif /* AVK_CALLKIND_H */
