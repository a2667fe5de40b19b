/*
 * aardvark_amd.h — C-ABI of the MI355X (gfx950) compare hot path.
 *
 * This is the drop-in boundary for the per-region solver of `aardvark compare`:
 * one call replaces the reference's rayon loop
 *     all_regions.into_par_iter().map(|r| solve_compare_region(&r, &genome, cfg, strat))
 * (reference src/main.rs:251-268, src/waffle_solver.rs:122-124) with a batched launch
 * of hand-written HIP kernels.  The reference has no FFI of its own; the flat
 * structures below carry exactly the fields of `CompareRegion`
 * (src/data_types/compare_region.rs:13-26), `Variant` (src/data_types/variants.rs:73-91),
 * `CompareConfig` (src/waffle_solver.rs:94-103) and `CompareBenchmark`
 * (src/data_types/compare_benchmark.rs:9-33).
 *
 * Conventions
 *  - plain pointers + sizes, no C++/torch types; the caller owns every buffer;
 *    nothing is retained after a call returns except what a context owns
 *    (uploaded reference, uploaded batches).
 *  - every function returns 0 on success or a negative AVK_E_* infrastructure code;
 *    per-region solver outcomes are reported in `status[]` (AVK_ST_*), mirroring the
 *    reference's `anyhow::Result` per region (src/main.rs:255-265): a failed region
 *    produces no metrics and the batch continues.
 *  - coordinates are 0-based half-open (src/data_types/coordinates.rs:6-13).
 */
#ifndef AARDVARK_AMD_H
#define AARDVARK_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- enums (ordinals identical to the reference's Rust enums) ------------------ */

/* VariantType, src/data_types/variants.rs:6-31 */
enum {
    AVK_VT_SNV = 0, AVK_VT_INSERTION = 1, AVK_VT_DELETION = 2, AVK_VT_INDEL = 3,
    AVK_VT_SV_INSERTION = 4, AVK_VT_SV_DELETION = 5, AVK_VT_SV_DUPLICATION = 6,
    AVK_VT_SV_INVERSION = 7, AVK_VT_SV_BREAKEND = 8, AVK_VT_TR_CONTRACTION = 9,
    AVK_VT_TR_EXPANSION = 10, AVK_VT_UNKNOWN = 11, AVK_N_VARIANT_TYPES = 12
};

/* PhasedZygosity, src/data_types/phase_enums.rs:33-46 */
enum {
    AVK_ZYG_UNKNOWN = 0, AVK_ZYG_HOM_REF = 1, AVK_ZYG_UNPHASED_HET = 2,
    AVK_ZYG_PHASED_HET01 = 3, AVK_ZYG_PHASED_HET10 = 4, AVK_ZYG_HOM_ALT = 5
};

/* Classification, src/data_types/variant_metrics.rs:12-22 */
enum { AVK_CLASS_UNKNOWN = 0, AVK_CLASS_TP = 1, AVK_CLASS_FN = 2, AVK_CLASS_FP = 3 };

/* Metric block geometry.  A region's GroupTypeMetrics (src/data_types/grouped_metrics.rs:32-37)
 * is 13 groups (group 0 = joint, group 1+t = VariantType t) of 22 counters
 * (GroupMetrics, grouped_metrics.rs:150-161 + summary_metrics.rs:6-15,84-92). */
#define AVK_N_GROUPS 13
#define AVK_N_FIELDS 22
enum {
    AVK_F_GT_TRUTH_TP = 0, AVK_F_GT_TRUTH_FN, AVK_F_GT_QUERY_TP, AVK_F_GT_QUERY_FP,
    AVK_F_GT_TRUTH_FN_GT, AVK_F_GT_QUERY_FP_GT,
    AVK_F_HAP_TRUTH_TP, AVK_F_HAP_TRUTH_FN, AVK_F_HAP_QUERY_TP, AVK_F_HAP_QUERY_FP,
    AVK_F_WHAP_TRUTH_TP, AVK_F_WHAP_TRUTH_FN, AVK_F_WHAP_QUERY_TP, AVK_F_WHAP_QUERY_FP,
    AVK_F_BP_TRUTH_TP, AVK_F_BP_TRUTH_FN, AVK_F_BP_QUERY_TP, AVK_F_BP_QUERY_FP,
    AVK_F_RBP_TRUTH_TP, AVK_F_RBP_TRUTH_FN, AVK_F_RBP_QUERY_TP, AVK_F_RBP_QUERY_FP
};
/* tally block = AVK_N_GROUPS*AVK_N_FIELDS sums, then solved_blocks, error_blocks
 * (src/writers/summary.rs:146-163) */
#define AVK_TALLY_LEN (AVK_N_GROUPS * AVK_N_FIELDS + 2)
#define AVK_TALLY_SOLVED (AVK_N_GROUPS * AVK_N_FIELDS)
#define AVK_TALLY_ERRORS (AVK_N_GROUPS * AVK_N_FIELDS + 1)

/* per-region status: 0 = Ok(CompareBenchmark); >0 = the reference would return Err
 * or panic for this region (class of the error) */
enum {
    AVK_ST_OK = 0,
    AVK_ST_BRANCH_FACTOR = 2,   /* "max_branch_factor must be greater than 0", query_optimizer.rs:177 */
    AVK_ST_NO_RESULTS = 3,      /* "no results found", query_optimizer.rs:331 */
    AVK_ST_NO_GT_RESULT = 4,    /* "No result found for problem", exact_gt_optimizer.rs:347 */
    AVK_ST_UNKNOWN_ALLELE = 5,  /* Allele::Unknown reached an optimizer, exact_gt_optimizer.rs:256 */
    AVK_ST_BAD_ZYGOSITY = 6,    /* assert_eq!(zyg, HomozygousAlternate) panics, query_optimizer.rs:315 */
    AVK_ST_VARIANT_METRICS = 7, /* VariantMetrics::new(.., 0, 0), variant_metrics.rs:57 */
    AVK_ST_TRUTH_FP = 8,        /* assert!(exp >= obs), waffle_solver.rs:322 */
    AVK_ST_RECORD_BP = 9,       /* "Truth/Query TP is less than basepair TP", waffle_solver.rs:492-493 */
    AVK_ST_SEQ_MISMATCH = 10,   /* assert_eq!(regenerated, optimizer sequence), waffle_solver.rs:365-367 */
    AVK_ST_AUTOFAIL_OOB = 11,   /* all_variant_order[auto_fail_index] out of bounds, exact_gt_optimizer.rs:312 */
    AVK_ST_INVALID_INPUT = 20,  /* rejected by host validation (window outside contig, variant outside
                                   window, unsorted variants, empty allele): the reference panics or is undefined */
    AVK_ST_CAPACITY = 21        /* device workspace exhausted at the largest tier AND in the library's own retries with slices of
                                   1, 4 and 16 GB (avk_results_download, context option "capacity_retry", default 1).  The retries repair
                                   what avk_results_download hands to the caller (per-region and per-call arrays, out->tally) and the
                                   batch's region records and metric blocks on the device, so that avk_label_tallies AFTER the download
                                   counts the repaired regions as the totals do; tally_dev of avk_compare_resident was written before
                                   the download and still counts a retried region as failed */
};

/* infrastructure errors (function return values) */
enum {
    AVK_E_OK = 0, AVK_E_ARG = -1, AVK_E_HIP = -2, AVK_E_OOM = -3, AVK_E_STATE = -4
};

/* ---- inputs ---------------------------------------------------------------------- */

/* A batch of CompareRegions in structure-of-arrays form.  Region r owns truth variants
 * [t_off[r], t_off[r]+t_cnt[r]) and query variants [q_off[r], q_off[r]+q_cnt[r]) of the
 * variant arrays; variant v's alleles are allele_bytes[a0_off[v] .. +a0_len[v]) (allele0 =
 * VCF REF after trimming) and [a1_off[v] .. +a1_len[v]) (allele1 = ALT). */
typedef struct avk_region_batch {
    uint64_t n_regions;
    const uint64_t *region_id;   /* CompareRegion::region_id */
    const uint32_t *contig_idx;  /* index into the uploaded reference (Coordinates::chrom) */
    const uint64_t *start;       /* Coordinates::start */
    const uint64_t *end;         /* Coordinates::end (exclusive) */
    const uint64_t *t_off;
    const uint32_t *t_cnt;
    const uint64_t *q_off;
    const uint32_t *q_cnt;

    uint64_t n_variants;
    const uint64_t *var_pos;       /* Variant::position (0-based, contig coordinates) */
    const uint8_t  *var_type;      /* AVK_VT_* */
    const uint8_t  *var_zyg;       /* AVK_ZYG_* (input zygosity of the call) */
    const uint32_t *var_raw_space; /* Variant::raw_allele_space */
    const uint64_t *a0_off;
    const uint32_t *a0_len;
    const uint64_t *a1_off;
    const uint32_t *a1_len;

    const uint8_t *allele_bytes;
    uint64_t allele_bytes_len;
} avk_region_batch;

/* The same batch in the library's COMPACT form: 20 bytes per region and 17 (21 with raw_allele_space) per call instead of 52 and 38 — the form to
 * build when the batch crosses PCIe once per call (a whole genome: 0.23 GB instead of 0.48 GB; the host boundary is bound by that copy).  Constraints
 * that make the narrow fields possible: contigs shorter than 4 Gbp, the calls of a region adjacent in the call arrays (truth calls at
 * [v_off, v_off + t_cnt), query calls right behind them), allele1 of a call right behind its allele0 in allele_bytes, fewer than 2^32 calls and
 * allele bytes, at most 65535 calls per region and side.  The library widens it on the device (one kernel); results are indexed like the arrays here. */
typedef struct avk_compact_batch {
    uint64_t n_regions;
    const uint32_t *contig_idx;    /* [n_regions] may be NULL (contig 0) */
    const uint32_t *start;         /* [n_regions] Coordinates::start */
    const uint32_t *len;           /* [n_regions] end - start */
    const uint32_t *v_off;         /* [n_regions] first call of the region */
    const uint16_t *t_cnt, *q_cnt; /* [n_regions] */
    uint64_t n_variants;
    const uint32_t *var_pos;       /* [n_variants] Variant::position */
    const uint8_t  *var_type_zyg;  /* [n_variants] AVK_VT_* | AVK_ZYG_* << 4 */
    const uint32_t *a_off;         /* [n_variants] allele0 at allele_bytes[a_off ..), allele1 right behind it */
    const uint32_t *a0_len, *a1_len;
    const uint32_t *var_raw_space; /* [n_variants] may be NULL (= the longer allele) */
    const uint8_t  *allele_bytes;
    uint64_t allele_bytes_len;
} avk_compact_batch;

/* The same batch in the PACKED form (round 3): 10 bytes per region and 5 per call plus the allele bytes — what is left when every offset the other forms
 * carry is implied by order: the calls of region r follow those of region r - 1 (truth calls, then query calls), the alleles of call v follow those of
 * call v - 1 (allele0, then allele1), call positions are relative to their region's start.  The library computes the offsets on the device (two prefix
 * sums) and writes the wide arrays there.  A whole genome: 94 MB over PCIe instead of 227 (compact) or 479 (wide).  Constraints: windows shorter than
 * 65,536 bases, at most 255 calls per region and side, alleles of at most 255 bases — these three hold WITHOUT ESCAPES: a batch handed in with an
 * avk_packed_escapes (below) lists the few regions, counts and calls that exceed them —, fewer than 2^32 calls and allele bytes, contigs shorter than 4 Gbp,
 * at most 65,535 contigs.  Results are indexed like the arrays here. */
typedef struct avk_packed_batch {
    uint64_t n_regions;
    const uint16_t *contig_idx;    /* [n_regions] may be NULL (contig 0) */
    const uint32_t *start;         /* [n_regions] Coordinates::start */
    const uint16_t *len;           /* [n_regions] end - start */
    const uint8_t  *t_cnt, *q_cnt; /* [n_regions] */
    uint64_t n_variants;           /* = sum of t_cnt + q_cnt */
    const uint16_t *var_rel_pos;   /* [n_variants] Variant::position - the region's start */
    const uint8_t  *var_type_zyg;  /* [n_variants] AVK_VT_* | AVK_ZYG_* << 4 */
    const uint8_t  *a0_len, *a1_len; /* [n_variants] */
    const uint32_t *var_raw_space; /* [n_variants] may be NULL (= the longer allele) */
    const uint8_t  *allele_bytes;  /* allele0 then allele1 of call 0, of call 1, ... */
    uint64_t allele_bytes_len;     /* = sum of a0_len + a1_len */
} avk_packed_batch;

/* ESCAPES of a packed batch (avk_packed_batch and avk_packed_multi_batch alike): sparse overrides for the few entries whose values do not fit the narrow
 * fields, so that one 300-base insertion, one window of 65,536 bases or one side with 256 calls no longer costs a call set the packed form.  Three sorted
 * lists; an entry that is listed takes its value(s) from the list, whatever the value, and its narrow field(s) MUST be written as 0 (the running sums over the
 * narrow arrays then count it as nothing, and the library adds the listed values).  A listed entry with a non-zero narrow field — len, t_cnt / q_cnt / in_cnt,
 * var_rel_pos, a0_len or a1_len — is AVK_E_ARG from every function that takes the lists, on the device and on the host alike (avk_merge_counts_esc reads the count
 * slots only and checks those).  An entry that is not listed means what it means without escapes.
 *   regions  esc_region[] ascending region indices; esc_len[] the window length (end - start)
 *   counts   esc_slot[] ascending count slots; esc_cnt[] the count.  Compare form: slot 2r = t_cnt of region r, slot 2r + 1 = q_cnt of region r;
 *            multi form: slot m * k + i = in_cnt[m * k + i]
 *   calls    esc_call[] ascending call indices; esc_rel_pos[], esc_a0_len[], esc_a1_len[] replace all THREE narrow fields of the call
 * The indices are those of a larger batch this one is a slice of: region r of the batch is listed as first_region + r, its count slots as first_slot + ..,
 * call v as first_call + v — a slice of a batch is its pointer ranges plus these three bases, no copy.  What is left are the wide form's own limits: fewer
 * than 2^32 calls and allele bytes, contigs shorter than 4 Gbp, at most 65,535 contigs, and per region what INTEGRATION.md section 4 states (60,000 calls,
 * windows and alleles of 2^31 bases): AVK_E_ARG or AVK_ST_INVALID_INPUT exactly as for the same batch handed in wide.  A NULL pointer or three zero
 * counts: no escapes.  A list that is not ascending, or names an entry outside the batch, is AVK_E_ARG. */
typedef struct avk_packed_escapes {
    uint64_t first_region, first_call, first_slot;
    uint64_t n_esc_regions;
    const uint64_t *esc_region;    /* [n_esc_regions] */
    const uint32_t *esc_len;       /* [n_esc_regions] */
    uint64_t n_esc_slots;
    const uint64_t *esc_slot;      /* [n_esc_slots] */
    const uint32_t *esc_cnt;       /* [n_esc_slots] */
    uint64_t n_esc_calls;
    const uint64_t *esc_call;      /* [n_esc_calls] */
    const uint32_t *esc_rel_pos, *esc_a0_len, *esc_a1_len; /* [n_esc_calls] */
} avk_packed_escapes;

/* CompareConfig, src/waffle_solver.rs:94-115 */
typedef struct avk_compare_config {
    uint32_t max_branch_factor;     /* default 50 */
    uint32_t enable_sequences;      /* fill seq_* outputs (debug region_sequences.tsv.gz) */
    uint32_t enable_exact_shortcut; /* hidden --enable-exact-shortcut */
} avk_compare_config;

/* ---- outputs --------------------------------------------------------------------- */

/* Caller-allocated result arrays, positionally aligned with the input batch.
 * Any pointer except `status` may be NULL to skip that output (and `status` too when region_packed is given). */
typedef struct avk_result_batch {
    int32_t  *status;        /* [n_regions] AVK_ST_* */
    uint32_t *ed_h1;         /* [n_regions] CompareBenchmark::bm_edit_distance_h1 */
    uint32_t *ed_h2;         /* [n_regions] */
    uint32_t *n_optima;      /* [n_regions] tied optima returned by optimize_sequences */
    uint16_t *type_present;  /* [n_regions] bit t: VariantType t has an entry in variant_metrics */
    uint32_t *group_metrics; /* [n_regions][AVK_N_GROUPS][AVK_N_FIELDS] full GroupTypeMetrics */

    /* per variant, same indexing as the input variant arrays; query entries are already
     * toggled the way CompareBenchmark::add_swap_benchmark stores them
     * (compare_benchmark.rs:109-123): these are the EA / OA / BD values of the output VCFs */
    uint8_t  *var_expected;  /* [n_variants] */
    uint8_t  *var_observed;  /* [n_variants] */
    uint8_t  *var_class;     /* [n_variants] AVK_CLASS_* */
    uint8_t  *var_zyg;       /* [n_variants] zygosity resolved by the phasing search (GT of output VCFs) */

    /* SequenceBundle (compare_benchmark.rs:166-185) when cfg.enable_sequences:
     * region r, sequence k (0 ref, 1 truth1, 2 truth2, 3 query1, 4 query2) is
     * seq_bytes[seq_off[r] + k*seq_stride[r] .. + seq_len[5*r+k]).  seq_off/seq_stride are
     * INPUTS sized with avk_seq_stride(). */
    uint8_t  *seq_bytes;
    const uint64_t *seq_off;    /* [n_regions] */
    const uint32_t *seq_stride; /* [n_regions] */
    uint32_t *seq_len;          /* [n_regions][5] */

    uint64_t *tally;         /* [AVK_TALLY_LEN] sums over the Ok regions of this batch */

    /* Compact per-region BASEPAIR groups (optional; both or neither): what is left of a region's GroupTypeMetrics once the per-call decisions above are known.
     * Region r owns groups [bp_off[r], bp_off[r + 1]) of bp_groups: the joint group first, then one per VariantType that occurs among the region's
     * calls, in type order; a group is 4 counters: BASEPAIR truth_tp, truth_fn, query_tp, query_fp (summary_metrics.rs:6-15; the doubled values of
     * waffle_solver.rs:335-449).  16 bytes x (1 + call types) per region instead of the 1144-byte block of group_metrics; regions that fail validation own no
     * group, regions that fail in the solver own zeros.  avk_group_metrics_from_compact rebuilds the full 13 x 22 block of a region from these and the
     * per-call outputs. */
    uint32_t *bp_off;        /* [n_regions + 1] */
    uint32_t *bp_groups;     /* [capacity][4] with capacity >= n_regions + n_variants (a region has at most 1 + its number of calls groups) */

    /* The packed result form (optional, each on its own): everything the arrays above say per region in 8 bytes and per call in 1 byte — a whole-genome
     * job's results cross PCIe as 37 MB instead of 96.  A caller that hands in region_packed may leave `status` NULL; one that hands in var_packed needs none
     * of var_expected / var_observed / var_class / var_zyg.  Read them with the avk_rp_* / avk_vp_* accessors below (what the FFI side would do while it
     * builds its CompareBenchmark values) or expand them into the arrays above with avk_results_expand.
     *   region_packed[r] = status (bits 0-6) | "the 8 filtered types have map entries" (bit 7) | n_optima (bits 8-23) | ed_h1 (bits 24-43) | ed_h2 (bits 44-63);
     *                      an edit distance of 2^20 - 1 or more reads as AVK_RP_ED_MAX: ask for ed_h1 / ed_h2 as well if regions can be that far from the
     *                      reference (none of a genome's is: the search gives up on such windows long before, AVK_ST_CAPACITY)
     *   var_packed[v]    = expected (bits 0-1) | observed (bits 2-3) | resolved zygosity AVK_ZYG_* (bits 4-6); the class follows from the two counts and the
     *                      side the call is on (variant_metrics.rs:43-101): avk_vp_class */
    uint64_t *region_packed; /* [n_regions] */
    uint8_t  *var_packed;    /* [n_variants] */

    /* The BASEPAIR groups in their packed form (optional; hand in bp_packed, bp_spilled AND bp_groups, leave bp_off NULL): one word per region instead of
     * 4 + 16 x (1 + call types) bytes.  A region whose groups all equal its joint group — every region with calls of ONE type: a side filtered to the type it
     * consists of is the side itself (waffle_solver.rs:383-445) — and whose four counters are below 128 is that word:
     *   bp_packed[r] = truth_tp | truth_fn << 7 | query_tp << 14 | query_fp << 21                         (bit 31 clear)
     * any other region's groups (the joint one, then one per call type, as above) are SPILLED into bp_groups, in no particular order:
     *   bp_packed[r] = 0x80000000 | index of the region's first group in bp_groups
     * bp_spilled[0] = number of groups in bp_groups.  A genome's regions need 4 + ~2.5 bytes each this way instead of 36 (profiles/r05_bp_packed.txt); regions with a
     * non-zero status hold 0.  avk_group_metrics_from_compact reads either form.  Device-packed batches only (option device_pack, the default). */
    uint32_t *bp_packed;     /* [n_regions] */
    uint32_t *bp_spilled;    /* [1] */
} avk_result_batch;

#define AVK_BP_SPILL 0x80000000u
static inline int      avk_bp_is_spilled(uint32_t w) { return (w & AVK_BP_SPILL) != 0; }
static inline uint32_t avk_bp_spill_index(uint32_t w) { return w & 0x7FFFFFFFu; }
static inline uint32_t avk_bp_counter(uint32_t w, int i) { return (w >> (7 * i)) & 0x7Fu; } /* i: 0 truth_tp, 1 truth_fn, 2 query_tp, 3 query_fp */

#define AVK_RP_ED_MAX 0xFFFFFu
/* the 8 variant types add_basepair_stats filters by (waffle_solver.rs:383-445): a solved region has map entries for them whether they occur or not */
#define AVK_FILTERED_TYPE_MASK ((1u << AVK_VT_SNV) | (1u << AVK_VT_INSERTION) | (1u << AVK_VT_DELETION) | (1u << AVK_VT_INDEL) | (1u << AVK_VT_TR_CONTRACTION) | \
                                (1u << AVK_VT_TR_EXPANSION) | (1u << AVK_VT_SV_DELETION) | (1u << AVK_VT_SV_INSERTION))
static inline uint64_t avk_rp_make(uint32_t status, uint32_t ed_h1, uint32_t ed_h2, uint32_t n_optima, uint32_t type_present) {
    const uint64_t e1 = ed_h1 < AVK_RP_ED_MAX ? ed_h1 : AVK_RP_ED_MAX, e2 = ed_h2 < AVK_RP_ED_MAX ? ed_h2 : AVK_RP_ED_MAX;
    const uint64_t filtered = (type_present & AVK_FILTERED_TYPE_MASK) == AVK_FILTERED_TYPE_MASK ? 1u : 0u;
    return (uint64_t)(status & 0x7Fu) | filtered << 7 | (uint64_t)(n_optima & 0xFFFFu) << 8 | e1 << 24 | e2 << 44;
}
static inline int32_t  avk_rp_status(uint64_t w) { return (int32_t)(w & 0x7Fu); }
static inline uint32_t avk_rp_filtered_types(uint64_t w) { return (uint32_t)(w >> 7) & 1u; }
static inline uint32_t avk_rp_n_optima(uint64_t w) { return (uint32_t)(w >> 8) & 0xFFFFu; }
static inline uint32_t avk_rp_ed_h1(uint64_t w) { return (uint32_t)(w >> 24) & AVK_RP_ED_MAX; }
static inline uint32_t avk_rp_ed_h2(uint64_t w) { return (uint32_t)(w >> 44) & AVK_RP_ED_MAX; }
/* type_present of a region from its packed word and the OR of (1 << type) over its calls */
static inline uint16_t avk_rp_type_present(uint64_t w, uint32_t call_types) {
    return avk_rp_status(w) != 0 ? (uint16_t)0 : (uint16_t)(call_types | (avk_rp_filtered_types(w) ? AVK_FILTERED_TYPE_MASK : 0u));
}
static inline uint8_t avk_vp_make(uint32_t expected, uint32_t observed, uint32_t zyg) { return (uint8_t)((expected & 3u) | (observed & 3u) << 2 | (zyg & 7u) << 4); }
static inline uint8_t avk_vp_expected(uint8_t b) { return (uint8_t)(b & 3u); }
static inline uint8_t avk_vp_observed(uint8_t b) { return (uint8_t)((b >> 2) & 3u); }
static inline uint8_t avk_vp_zyg(uint8_t b) { return (uint8_t)((b >> 4) & 7u); }
/* TP when the counts agree; otherwise a truth call is a FN and a query call (stored toggled) a FP; a call of a failed region has no class */
static inline uint8_t avk_vp_class(uint8_t b, int is_query) {
    if ((b & 15u) == 0) return AVK_CLASS_UNKNOWN;
    return avk_vp_expected(b) == avk_vp_observed(b) ? AVK_CLASS_TP : (is_query ? AVK_CLASS_FP : AVK_CLASS_FN);
}

/* ---- context --------------------------------------------------------------------- */

typedef struct avk_ctx avk_ctx;          /* one per GPU / per host thread */
typedef struct avk_dev_batch avk_dev_batch; /* a region batch resident in HBM */

int  avk_ctx_create(int device_id, avk_ctx **out);
void avk_ctx_destroy(avk_ctx *ctx);
/* last error text of this context (or of the failed create when ctx == NULL) */
const char *avk_last_error(const avk_ctx *ctx);
/* run every launch of this context on an existing hipStream_t (e.g. torch's current stream).  The call BLOCKS until the stream the context used so far is idle
 * (its buffer pool hands memory out in the order of one stream); when that one was the caller's too it should still be alive — if it has been destroyed the
 * call waits for the whole device instead and still switches. */
int  avk_ctx_set_stream(avk_ctx *ctx, void *hip_stream);
/* Context options, forty of them (set them before avk_batch_upload: the work plan of a batch is made at upload).  None of them changes a result: the parity tests run under
 * random sets of them (tests/test_gpu_random_schedules.py).  Round 6 removed 27 names whose A/B comparisons were settled (profiles/r06_options.txt lists them with
 * the value each is now fixed at); what is left is what selects a code path, sizes a workspace, or is needed to reproduce a measurement.
 *   workspace tiers  "lds_bytes_per_wave" (10240), "lds_ed_cap" (48): the small LDS slice of the wave-per-region kernels; "lds2_bytes_per_wave" (40960), "lds2_ed_cap" (48):
 *                    the large one; "ws_bytes_per_wave" (1 MiB): the per-wave HBM slice, "adaptive_ws" (1: sized from the batch's predicted needs), "ws_budget_bytes";
 *                    "big_ws_bytes" (64 MiB): the shared big slices; "hbm_ed_cap"; "waves_per_cu"; 0 bytes disables a tier; "capacity_retry" (1: a region no tier could hold is
 *                    solved again by the library in larger slices)
 *   scheduling       "solo_min_variants" (5: regions with at least this many calls go to the solo launches), "class_c_nodes_x2" (12: nodes per call a search is priced at
 *                    when class C is decided), "class_c_below" (16384: a batch with lane launches and at most this many regions outside them plans those regions for the
 *                    wave-cooperative kernel — a contig, a rank's shard),
 *                    "lds_escalation" (1: in-workgroup escalation of the bulk launch), "static_pct" (75: share of a launch's work list dealt statically), "claim" (2:
 *                    regions per dynamic claim)
 *   lane kernels     "lane_kernel" (1: regions with at most three calls per side on a short window are solved one per LANE, avk_lane.inl / four lanes per region,
 *                    avk_quad.inl), "lane_quad" (1: launches of at most 16 records per wave run four lanes per region), "lane_pairs" (1: regions with the same SNV on
 *                    both sides are looked up, avk_pairs.inl), "lane_min_regions" (2048) / "lane_min_batch" (16384): smaller classes / batches stay with the
 *                    wave-per-region kernels, "lane_node_cap" (32: search nodes the three-call class makes before it hands a region over), "lane_width_one" / "_two" /
 *                    "_three" (64, 64, 16: records a wave takes at a time), "lane_head_width" (16: records per wave in the heads of the classes, the tiles of regions
 *                    with estimated edits; 0 = no head launch), "use_packed_reference" (1: the 2-bit reference; 0: bytes — every region then goes to the wave kernels)
 *   wide kernel      "wide_kernel" (1: large searches on small windows are solved one per WAVE, avk_wide.inl), "wide_lds_bytes" (16384), "wide_retry_lds_bytes" (65536)
 *   long windows     "team_long_windows" (1: a batch of large windows — no region of class C is the wide kernel's — runs the head of the class a WORKGROUP per region,
 *                    avk_region_kernel_team; 0: a wave per region; 2: a workgroup per region whose owner wave takes every job itself, a diagnostic),
 *                    "team_head_regions" (48: how many regions that head has)
 *   boundary         "device_pack" (1: batches are validated, classified, ordered and written in the kernels' layout on the device, avk_devpack.inl; 0: by host threads,
 *                    avk_pack.h — same records either way), "packed_source" (1: an avk_packed_batch is packed from the packed arrays themselves; 0: from a wide copy made
 *                    on the device first, round 5), "kernel_copies" (1: every synchronous call that copies by DMA engine times its own copies in; in every second process of a box they crawl at half the
 *                    link's rate, and from the first such call on the pinned arrays of the context's synchronous calls cross the bus by a copy kernel, every lane 16
 *                    bytes at a time from / to the pinned pages: profiles/r06_copy_engines.txt; 0: always hipMemcpyAsync; 2: always the kernel),
 *                    "split_parts" (1; 2..4: an avk_compare_packed call of pinned arrays runs as that many batches in flight,
 *                    compare_packed_split — slower than the whole call today, profiles/r06_split_call.txt)
 *                    "pack_queue_early" (1: a synchronous avk_compare_packed call on pinned arrays queues the packer's prefix sums and dp_variant from inside its copy
 *                    loop, each right behind the event it waits for, so that they run under the copies also where the streams share a hardware queue; 0: after the
 *                    copies are queued), "pack_chunks" (0; 2..8: such a call also copies its per-region and per-call arrays in that many groups and runs the region
 *                    pass group by group under them, avk_pack_chunks.h, DESIGN section 5 — byte-identical results), "pack_chunk_floor" (1048576: a batch whose
 *                    groups would copy fewer bytes of some array keeps the old order; tests lower it)
 *   outputs          "emit_group_metrics" (0 = kernels skip the per-region 13 x 22 block; the batch tally is always produced), "emit_bp_groups" (1 = kernels write the
 *                    compact per-region BASEPAIR groups; the one-call entry points switch it on when the caller hands the arrays in), "accumulate_tally" (1 =
 *                    avk_compare_resident ADDS the batch tally to tally_dev)
 *                    Options are read when a batch is submitted: a batch in flight (avk_compare_packed_submit .. avk_wait) keeps the values of its submit.
 * The launches of one call run on HIP streams side by side; the HIP runtime gives a process 4 hardware queues by default and streams that share one take turns:
 * avk_ctx_create sets GPU_MAX_HW_QUEUES=24 unless the environment already has it (effective when it is the process's first HIP call).
 *   launch plan      "step_queues" (0: by the value of GPU_MAX_HW_QUEUES when the context was made — below 8 the launch chains of a step are folded onto the context's
 *                    stream and three more, each chain whole and behind another, avk_step_plan.h and DESIGN section 4.7; 4: always folded; 8: always a stream per
 *                    chain — same results either way) */
int  avk_ctx_set_option(avk_ctx *ctx, const char *name, int64_t value);

/* Replaces ReferenceGenome::from_fasta + get_full_chromosome (src/main.rs:94,
 * src/waffle_solver.rs:131): contigs are copied to HBM once (2-bit packed plus the raw
 * bytes needed for windows holding non-ACGT symbols) and owned by the context. */
int  avk_ref_upload(avk_ctx *ctx, uint32_t n_contigs, const uint8_t *const *seqs, const uint64_t *lens);

/* One call = solve_compare_region for every region of the batch: the caller's arrays go to HBM as they are, packing kernels, solver
 * kernels, unpacking kernel, results into the caller's arrays (no per-region work on the host). */
int  avk_compare_batch(avk_ctx *ctx, const avk_region_batch *batch,
                       const avk_compare_config *cfg, avk_result_batch *out);

/* the same for a batch in the compact form */
int  avk_compare_compact(avk_ctx *ctx, const avk_compact_batch *batch, const avk_compare_config *cfg, avk_result_batch *out);
int  avk_batch_upload_compact(avk_ctx *ctx, const avk_compact_batch *batch, avk_dev_batch **out);
/* and in the packed form (replaces the same loop, src/main.rs:251-268; the batch crosses PCIe as 94 MB per whole genome) */
int  avk_compare_packed(avk_ctx *ctx, const avk_packed_batch *batch, const avk_compare_config *cfg, avk_result_batch *out);
/* the same for a packed batch with escapes (esc may be NULL: avk_compare_packed is this call with NULL).  An escaped batch is widened on the device by
 * escape-aware kernels (avk_devpack.inl: dp_widen_packed_esc) and planned from the wide arrays: same work plan, same results as the batch handed in wide. */
int  avk_compare_packed_esc(avk_ctx *ctx, const avk_packed_batch *batch, const avk_packed_escapes *esc, const avk_compare_config *cfg, avk_result_batch *out);

/* The same call in two halves, for a caller with several batches (the reference streams its regions through one rayon loop and collects at the end,
 * src/main.rs:251-268): batches in flight inside ONE context.  avk_compare_packed_submit copies the batch's arrays on the context's copy stream — beside the
 * kernels of the batch submitted before — packs it, queues its solver launches and the copies of its results (on a second copy stream, beside whatever is
 * submitted next) and returns a ticket; avk_wait returns when the results are in `out`'s arrays and frees the ticket.  Tickets may be waited for in any order;
 * at most four are in flight.  The batch's arrays may be reused as soon as the submit has returned; `out`'s arrays belong to the library until the wait returns.
 * Every array of `batch` and `out` must be pinned (avk_host_alloc) for the copies to run beside anything: a batch with a pageable array, with sequence outputs
 * or compact BASEPAIR groups is solved inside the submit (its ticket is complete).  The submit blocks once, while the packer's plan comes back to the host —
 * behind the batch submitted before.  Results are those of avk_compare_packed, bit for bit (tests/test_gpu_async.py). */
/* ---- several GPUs: regions are independent, so a job is cut by ONE rule — shard = hash(region_id) % ranks (region ids are sequential in genome
 * order, region_generation.rs:403-409, the hash spreads dense loci over the ranks) — every rank solves its shard, and the job tally is one all-reduce
 * (SummaryWriter::add_comparison_benchmark over all regions, writers/summary.rs:146-163).  aardvark_amd/dist.py states the same hash for the Python side. */
static inline uint64_t avk_region_hash(uint64_t x) { /* splitmix64's finaliser */
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}
static inline uint32_t avk_region_shard(uint64_t region_id, uint32_t ranks) { return (uint32_t)(avk_region_hash(region_id) % ranks); }
/* the regions of `whole` that rank `rank` of `world` owns (region_id[r], or first_id + r when region_id is NULL), gathered into a packed batch of their own in the
 * whole batch's order; avk_packed_shard_scatter writes a result batch of the shard into the arrays of the whole batch (per-region arrays by region, per-call arrays
 * by call; the tally is left to the caller: add the ranks' tallies, or avk_tally_allreduce) */
typedef struct avk_packed_shard avk_packed_shard;
int  avk_packed_shard_make(const avk_packed_batch *whole, const uint64_t *region_id, uint64_t first_id, uint32_t rank, uint32_t world, avk_packed_shard **out);
/* with escapes: the shard owns escape lists of its own, rebased to the shard's indices (bases 0); avk_packed_shard_escapes returns them (counts 0 when the
 * shard holds no escaped entry) */
int  avk_packed_shard_make_esc(const avk_packed_batch *whole, const avk_packed_escapes *esc, const uint64_t *region_id, uint64_t first_id, uint32_t rank, uint32_t world,
                               avk_packed_shard **out);
const avk_packed_batch *avk_packed_shard_batch(const avk_packed_shard *s);
const avk_packed_escapes *avk_packed_shard_escapes(const avk_packed_shard *s);
uint64_t avk_packed_shard_regions(const avk_packed_shard *s, const uint64_t **index_in_whole);
int  avk_packed_shard_scatter(const avk_packed_shard *s, const avk_result_batch *shard_results, avk_result_batch *whole_results);
void avk_packed_shard_free(avk_packed_shard *s);
/* tally[AVK_TALLY_LEN] (host) summed over the ranks of an RCCL communicator (ncclComm_t), on the context's stream: the job's one collective.  Every rank calls it
 * with its own context and communicator; RCCL is looked up in the process (the caller that made the communicator loaded it), not linked. */
int  avk_tally_allreduce(avk_ctx *ctx, void *nccl_comm, uint64_t *tally);
/* the same collective for any block of `n` 64-bit sums (avk_tally_allreduce is this with n = AVK_TALLY_LEN; a sharded merge sums its summary counters with it) */
int  avk_counts_allreduce(avk_ctx *ctx, void *nccl_comm, uint64_t *counts, uint64_t n);

typedef struct avk_ticket avk_ticket;
int  avk_compare_packed_submit(avk_ctx *ctx, const avk_packed_batch *batch, const avk_compare_config *cfg, avk_result_batch *out, avk_ticket **ticket);
int  avk_wait(avk_ctx *ctx, avk_ticket *ticket);
int  avk_batch_upload_packed(avk_ctx *ctx, const avk_packed_batch *batch, avk_dev_batch **out);
/* both with escapes (NULL: the calls above).  For a submit to stay asynchronous the escape lists must be pinned like the batch's arrays: they are copied on the
 * copy stream with the rest */
int  avk_compare_packed_submit_esc(avk_ctx *ctx, const avk_packed_batch *batch, const avk_packed_escapes *esc, const avk_compare_config *cfg, avk_result_batch *out,
                                   avk_ticket **ticket);
int  avk_batch_upload_packed_esc(avk_ctx *ctx, const avk_packed_batch *batch, const avk_packed_escapes *esc, avk_dev_batch **out);

/* The same in three steps, for callers that keep batches resident in HBM. */
int  avk_batch_upload(avk_ctx *ctx, const avk_region_batch *batch, avk_dev_batch **out);
/* tally_dev: optional device pointer (uint64[AVK_TALLY_LEN]) that receives the batch tally,
 * e.g. a tensor that is then reduced over RCCL; may be NULL. Asynchronous on the context stream. */
int  avk_compare_resident(avk_ctx *ctx, avk_dev_batch *db, const avk_compare_config *cfg, void *tally_dev);
int  avk_results_download(avk_ctx *ctx, avk_dev_batch *db, avk_result_batch *out);
void avk_batch_free(avk_ctx *ctx, avk_dev_batch *db);
int  avk_synchronize(avk_ctx *ctx);

/* bytes needed per sequence slot of region r of `batch` (upper bound of any haplotype length) */
uint32_t avk_seq_stride(const avk_region_batch *batch, uint64_t r);

/* measurement hooks: milliseconds of the solver kernels of the last avk_compare_resident /
 * avk_compare_batch on this context, from hipEvents on the context stream; how many regions
 * each workspace tier solved; algorithmic bytes of the batch (DESIGN.md "bytes per region") */
int  avk_last_kernel_ms(avk_ctx *ctx, float *ms);  /* the dominant launch: first pass of avk_region_kernel_lds */
int  avk_last_solver_ms(avk_ctx *ctx, float *ms);  /* all solver launches of the call (tier passes + tally reduce) */
int  avk_last_tier_counts(avk_ctx *ctx, uint64_t counts[5]); /* regions finished per tier, then capacity failures */
/* Pinned host memory for batch and result arrays (hipHostMalloc behind it; avk_host_free gives it back).  avk_compare_batch / avk_batch_upload /
 * avk_results_download copy arrays that live in such memory by DMA straight from / into them; arrays anywhere else go through a pinned bounce
 * buffer that the library's host threads fill or drain (a whole-genome batch: about 0.5 GB in, 0.1 GB out).  The Rust side would back its
 * FlatBatch vectors with this allocator. */
void *avk_host_alloc(avk_ctx *ctx, size_t bytes);
void  avk_host_free(avk_ctx *ctx, void *p);
/* optional: pins the bounce buffer avk_compare_batch needs for PAGEABLE arrays of a batch of up to n_regions / n_variants (kept by the context, only
 * grows), e.g. while a tool is still reading its inputs; without it the first large call pays for it */
int  avk_ctx_reserve(avk_ctx *ctx, uint64_t n_regions, uint64_t n_variants);
/* optional, for a process that makes ONE large call (the reference's `aardvark compare` is one run per process, src/main.rs:30): what the first call of a context
 * pays for beyond the call itself — the device code brought in, the table of the looked-up class, the bounce buffer of avk_ctx_reserve, the workspaces of a batch
 * of about n_regions regions — done now, e.g. on a thread beside the parsing of the inputs.  Changes no result; without it the first call does the same on demand. */
int  avk_ctx_warmup(avk_ctx *ctx, uint64_t n_regions_hint, uint64_t n_variants_hint);
int  avk_last_compare_was_one_shot(avk_ctx *ctx);  /* 1: the batch of the last avk_compare_batch / avk_optimize_pairs_batch was packed on the device
                                                      (context option device_pack) */
int  avk_last_lane_ms(avk_ctx *ctx, float *ms);    /* start of the call to the end of its lane-per-region launches (0: it had none) */
int  avk_last_lane_solved(avk_ctx *ctx, uint64_t *count); /* regions the lane-per-region kernel finished (last downloaded step);
                                                             they are not counted in any workspace tier */
int  avk_last_region_launches(avk_ctx *ctx, uint64_t *count); /* launches of the packer's region pass the last device-packed upload queued: 1, one more when calls were left
                                                                 to the host's edit distance; with the option pack_chunks = N on a batch that takes the chunked route, N + 1 (the groups and the catch-all) */
int  avk_last_wide_solved(avk_ctx *ctx, uint64_t *count); /* the same for the wave-cooperative kernel of the large searches on small windows (option wide_kernel) */
/* Host utility (no GPU involved): the full GroupTypeMetrics block of region r (13 groups x 22 counters, the layout of group_metrics) from the batch, the
 * per-call outputs var_expected / var_observed of `res` and the region's compact BASEPAIR groups: the GT / HAP / WEIGHTED_HAP counters follow from
 * (expected, observed) per call (grouped_metrics.rs:183-227 and the swap of :268-277), RECORD_BP from the calls' zygosities and raw_allele_space
 * (waffle_solver.rs:455-522).  Only meaningful for regions with status 0.  Returns 0, or AVK_E_ARG. */
int avk_group_metrics_from_compact(const avk_region_batch *batch, uint64_t r, const avk_result_batch *res, uint32_t *out /* [AVK_N_GROUPS * AVK_N_FIELDS] */);
/* Host utility (no GPU involved): the wide arrays of `wide` (whichever of status, ed_h1, ed_h2, n_optima, type_present, var_expected, var_observed, var_class,
 * var_zyg are not NULL) from packed->region_packed / packed->var_packed and the batch.  Calls that no region of the batch owns are left as they are.
 * Returns 0, or AVK_E_ARG (a wide per-region array is wanted without region_packed, a per-call one without var_packed, or a region's call range is outside the
 * batch). */
int avk_results_expand(const avk_region_batch *batch, const avk_result_batch *packed, avk_result_batch *wide);
uint64_t avk_algorithmic_bytes(const avk_region_batch *batch);
/* the same with (1) or without (0) the per-region BASEPAIR groups among the outputs: a run that produces per-region records, per-call decisions and
 * the batch tally only (emit_group_metrics 0) writes no per-region groups */
uint64_t avk_algorithmic_bytes_ex(const avk_region_batch *batch, int with_groups);

/* The device aligner by itself: a batch of DWFALite SCRIPTS (reference src/dwfa/dynamic_wfa.rs:23-276).  Script s works on the two
 * byte strings bytes[base_off[s]..] ("baseline") and bytes[other_off[s]..] ("other") and makes the calls step_off[s] .. step_off[s+1]:
 * step_op 0 = update(baseline[..step_blen], other[..step_olen]) (:68-84), 1 = finalize(..) (:183-198) on ONE aligner state, as the
 * reference's tests do (dynamic_wfa.rs:283-468).  Outputs per step: edit_distance() after the call and a status (0; 2 = the aligner was
 * already finalized, :69-71; AVK_ST_CAPACITY = more than wf_cap wavefront entries; engine 1 only: AVK_ST_INVALID_INPUT for symbols other
 * than ACGT or strings over 192 bases); optionally the final wavefront (final_wf [n][wf_cap], final_wf_len [n]).
 * engine 0: one wavefront per script, the lane-group aligner of the wave-per-region kernels; engine 1: one lane per script, the 2-bit
 * aligner of the lane-per-region kernel. */
int  avk_dwfa_script_batch(avk_ctx *ctx, int engine, uint32_t n_scripts, const uint8_t *bytes, uint64_t n_bytes, const uint64_t *base_off,
                           const uint64_t *other_off, const uint64_t *step_off, const uint8_t *step_op, const uint32_t *step_blen,
                           const uint32_t *step_olen, uint32_t *step_ed, int32_t *step_status, uint32_t wf_cap, uint32_t *final_wf,
                           uint32_t *final_wf_len);
/* profiling builds of the library only (-DAVK_PHASE_TIMING): summed clock ticks per solver phase of the last download:
 * [0] stage, [1] search A, [2] search B, [3] metrics setup, [4] base-pair metrics, [5] record metrics, [6] whole region,
 * [7] region count, [8..13] inside search A: setup, pop + quota, finalise, clone, extend, push */
int  avk_debug_phase_cycles(avk_ctx *ctx, uint64_t out[16]);

/* diagnostic (tools/gpu_hang_probe.py): busy[i] = 1 while stream i of the context still has queued work (0 the caller's stream, 1-2 the
 * solo launches' streams, 3-4 the lane launches' streams; -1 = no such stream), and the first n_counters words of the batch's device
 * counters (work-list claims, list lengths, tile claims) as they are at the time of the call, while the launches may still be running */
int  avk_debug_snapshot(avk_ctx *ctx, avk_dev_batch *db, uint32_t *counters, uint32_t n_counters, int32_t busy[5]);

/* measurement aid (bench.py's roofline by launch class): the work order of a device-packed batch — region order[k] is record k of the order the launches take their regions
 * in — and the plan's counts: counts[0..3] = regions of class C, of those not the wide kernel's, of class B, of all lane classes; counts[4 + 3 fc .. 6 + 3 fc] = first record,
 * regions and head regions of lane class fc (0 .. 5; 5 = the looked-up pairs).  Between class B and the first lane class lies the bulk.  order may be NULL. */
int  avk_debug_work_order(avk_ctx *ctx, avk_dev_batch *db, uint32_t *order, uint64_t counts[22]);

/* test aid, read-only: the 2-bit copy of the current reference that avk_ref_upload made and that every fast kernel reads, and its flag bitmap.  The contigs are packed as one
 * string, contig after contig without padding, B bases in all: base p of that string sits in bits 2 (p % 16) .. 2 (p % 16) + 1 of packed word p / 16, A = 0, C = 1, G = 2, T = 3,
 * any other byte 0; bit w % 32 of flag word w / 32 is set when one of the bytes packed word w covers is not an upper-case A, C, G or T (such windows are read from the byte copy).
 * Positions behind base B - 1 count as 0 and raise no flag.  words_out gets the (B + 15) / 16 packed words that cover the reference, flags_out the whole bitmap of the context,
 * (B + 15) / 16 / 32 + 8 words: the words behind the covered ones are 0.  AVK_E_ARG without a reference or when a capacity (in words) is smaller than that. */
int  avk_debug_ref_packed(avk_ctx *ctx, uint32_t *words_out, uint64_t n_words_cap, uint32_t *flags_out, uint64_t n_flag_words_cap);

/* Stratified tallies on the device (SummaryWriter::add_comparison_benchmark with the region's containment labels,
 * src/writers/summary.rs:146-163): after avk_compare_resident with the option emit_group_metrics set, label l's block of
 * AVK_TALLY_LEN words gets the sum of the metric blocks of the solved regions whose label list names l.  The labels of region r (caller
 * order) are label_idx[label_off[r] .. label_off[r + 1]) — what avf_strat_batch_labels of the feeder library produces.  The sums are
 * ADDED to out[n_labels * AVK_TALLY_LEN] (a job sums over its batches); the per-region blocks never leave the GPU. */
int  avk_label_tallies(avk_ctx *ctx, avk_dev_batch *db, uint32_t n_labels, const uint64_t *label_off, const uint32_t *label_idx, uint64_t *out);

/* The same sums WITHOUT per-region metric blocks (avk_labels.inl): a kernel rebuilds each solved region's block from what a run leaves on the device anyway — status,
 * expected / observed per call, the calls as the caller sent them, Variant::alt_ed and the compact BASEPAIR groups (the rule of avk_group_metrics_from_compact) —
 * and adds it straight into the sums of the region's labels.  emit_group_metrics may be 0; the run must write the BASEPAIR groups.  Semantics are those of
 * avk_label_tallies: sums are ADDED to out[n_labels * AVK_TALLY_LEN], a label named twice in a list counts twice, words AVK_TALLY_SOLVED / AVK_TALLY_ERRORS of a
 * label's block are not touched.  A launch holds the sums of avk_label_block(ctx) labels in LDS; more labels are more passes over the regions. */
typedef struct avk_region_labels {
    uint32_t n_labels;
    const uint64_t *label_off; /* [n_regions + 1], not decreasing */
    const uint32_t *label_idx; /* [label_off[n_regions]] each < n_labels (may be NULL when no region has a label) */
} avk_region_labels;
uint32_t avk_label_block(const avk_ctx *ctx);
/* resident form: a device-packed batch (option device_pack, the default) after avk_compare_resident with the option emit_bp_groups set; otherwise AVK_E_STATE.
 * Called after avk_results_download it also counts the regions the capacity retry repaired. */
int  avk_label_tallies_compact(avk_ctx *ctx, avk_dev_batch *db, const avk_region_labels *labels, uint64_t *out);
/* one-call forms: avk_compare_packed_esc / avk_compare_packed_submit_esc that also return the labels' sums (ADDED to label_tallies[n_labels * AVK_TALLY_LEN]; the
 * submit form adds them in avk_wait, until which `labels`' arrays and label_tallies belong to the library).  The library switches the BASEPAIR groups on itself;
 * regions the capacity retry repairs are counted.  labels == NULL or n_labels == 0: exactly the call without labels.  AVK_E_ARG, before anything is queued: a
 * decreasing label_off, an index >= n_labels, label_off[n_regions] != 0 with a NULL label_idx, a NULL label_tallies. */
int  avk_compare_packed_labels(avk_ctx *ctx, const avk_packed_batch *batch, const avk_packed_escapes *esc, const avk_region_labels *labels, const avk_compare_config *cfg,
                               avk_result_batch *out, uint64_t *label_tallies);
int  avk_compare_packed_submit_labels(avk_ctx *ctx, const avk_packed_batch *batch, const avk_packed_escapes *esc, const avk_region_labels *labels,
                                      const avk_compare_config *cfg, avk_result_batch *out, uint64_t *label_tallies, avk_ticket **ticket);
/* host only: the label lists of a shard's regions gathered from the whole job's, in shard order (avk_packed_shard_regions' index_in_whole).  shard_off gets
 * regions + 1 offsets; shard_idx (NULL: offsets only, to size it) the indices.  Per-rank sums add up over the ranks (avk_counts_allreduce). */
int  avk_packed_shard_labels(const avk_packed_shard *s, const avk_region_labels *whole, uint64_t *shard_off, uint32_t *shard_idx);

/* The stratification sets RESIDENT on the device and the containment lists made there (avk_strata.inl): a stratified job's interval sets are fixed, and what
 * Stratifications::containments (src/parsing/stratifications.rs:189-199) asks of them for a region — CompareRegion::var_coordinates, compare_region.rs:54-66: the
 * smaller of the sides' first call positions to the larger of the sides' LAST call's end — is on the device once the batch is packed.  avk_strata_upload copies
 * the sets to HBM once per context; the calls below then make label_off / label_idx by kernel, in the layout and order of avf_strat_batch_labels, bit for bit,
 * and no list is made on or copied from the host.
 *   tree (label l, contig c) = entries [tree_off[l * n_contigs + c], tree_off[l * n_contigs + c + 1]) of start[] and end_max[]; start sorted within a tree,
 *   end_max the running maximum of the intervals' EXCLUSIVE ends within a tree.  Coordinates are 32-bit (contigs are shorter than 4 Gbp by the packed form's own
 *   limits); avf_strat_export of the feeder library writes the arrays and does the clamping.  A region is in label l when, with k = upper_bound(start, first),
 *   k > 0 and last < end_max[k - 1] (first = the region's start, last = its end - 1).  Regions without calls, with start >= end, with call ranges outside the
 *   batch or a contig >= n_contigs have no labels; a region's status plays no part.
 * AVK_E_ARG, before any allocation: a decreasing tree_off, unsorted starts or a decreasing end_max inside a tree, NULL arrays with a non-zero total (these
 * refusals need no device: with ctx == NULL avk_last_error(NULL) has their text).  n_labels == 0 is a valid, empty set.  A handle belongs to the context it was
 * uploaded to (AVK_E_ARG with another one) and must be freed before that context is destroyed. */
typedef struct avk_strata avk_strata;
int  avk_strata_upload(avk_ctx *ctx, uint32_t n_labels, uint32_t n_contigs,
                       const uint64_t *tree_off,   /* [n_labels * n_contigs + 1], tree (l, c) at l * n_contigs + c */
                       const uint32_t *start,      /* sorted per tree */
                       const uint32_t *end_max,    /* running maximum of the EXCLUSIVE ends per tree */
                       avk_strata **out);
void avk_strata_free(avk_ctx *ctx, avk_strata *strata);
uint32_t avk_strata_n_labels(const avk_strata *strata);
/* the lists a resident, device-packed batch gets (wide, compact or packed upload, with or without escapes), downloaded: label_off[n_regions + 1], label_idx
 * ascending within a region.  label_idx == NULL: the offsets only (label_off[n_regions] = entries needed).  A cap (entries of room in label_idx) that is too
 * small: AVK_E_ARG with the needed size in label_off[n_regions].  Also how a caller gets lists to hand to avk_packed_shard_labels. */
int  avk_strata_region_labels(avk_ctx *ctx, avk_dev_batch *db, const avk_strata *strata, uint64_t *label_off, uint32_t *label_idx, uint64_t cap);
/* avk_label_tallies_compact with the handle in place of the lists: same preconditions, refusals and semantics (sums ADDED to out[n_labels * AVK_TALLY_LEN], words
 * AVK_TALLY_SOLVED / AVK_TALLY_ERRORS untouched, regions the capacity retry repaired counted when called after the download, more than avk_label_block labels
 * are more passes) */
int  avk_label_tallies_strata(avk_ctx *ctx, avk_dev_batch *db, const avk_strata *strata, uint64_t *out);
/* avk_compare_packed_labels with the handle in place of the lists: nothing but the batch goes in, the sums come back with the results.  The lists' count pass
 * runs behind the packer's region passes and its total returns with the packer's plan, the call's one round trip.  strata == NULL or zero labels: exactly the
 * call without labels, launch for launch.  An escaped batch takes the route it takes today. */
int  avk_compare_packed_strata(avk_ctx *ctx, const avk_packed_batch *batch, const avk_packed_escapes *esc, const avk_strata *strata, const avk_compare_config *cfg,
                               avk_result_batch *out, uint64_t *label_tallies);
/* avk_compare_packed_submit_labels with the handle in place of the lists, for a job that keeps batches in flight: the mask pass of the lists' kernels runs with
 * the packer's region passes on the batch's own upload streams, and the label kernel reads a region's labels straight from its mask words behind the solve — no
 * offsets, no index array, nothing made on or copied from the host.  The sums are ADDED to label_tallies[n_labels * AVK_TALLY_LEN] in avk_wait (until which
 * label_tallies belongs to the library); words AVK_TALLY_SOLVED / AVK_TALLY_ERRORS are untouched; the library switches the BASEPAIR groups on itself; regions the
 * capacity retry repairs are counted.  strata == NULL or zero labels: exactly avk_compare_packed_submit_esc, launch for launch.  AVK_E_ARG, before anything is
 * queued: a handle of another context, a NULL label_tallies.  Four batches in flight: AVK_E_STATE, as for every submit.  A batch that cannot be queued (pageable
 * arrays, sequences asked for, ...) is solved at submit by avk_compare_packed_strata and its ticket is complete.
 * Lifetime of the handle: it counts the batches submitted with it that have not been waited for.  avk_strata_free may be called while that count is not zero: it
 * first waits for the streams those batches' mask passes were queued on — nothing else reads the trees — and then frees them; avk_wait on such a ticket uses only
 * what the ticket itself holds (its masks, its sums, the number of labels).  Destroying the context with tickets in flight stays the caller's error. */
int  avk_compare_packed_submit_strata(avk_ctx *ctx, const avk_packed_batch *batch, const avk_packed_escapes *esc, const avk_strata *strata,
                                      const avk_compare_config *cfg, avk_result_batch *out, uint64_t *label_tallies, avk_ticket **ticket);

/* BOOTSTRAP REPLICATES of the tallies (avk_boot.inl; the rule is this project's own, stated in aardvark_amd/csrc/avk_boot.h and DESIGN.md section 5): the region
 * is the resampling unit, region r enters replicate b with the integer weight w(r, b) ~ Poisson(1) that avk_boot_weight gives — a function of the seed, the
 * region's contig and window start and b alone, so a job's replicates do not depend on how it is cut into batches, shards or slices.
 *   block    a replicate's block has AVK_TALLY_LEN words: words 0 .. 285 the sum over the solved regions (status 0) of w(r, b) x the region's block (what
 *            avk_group_metrics_from_compact gives, 32-bit truncations included), word AVK_TALLY_SOLVED the sum of w over them, word AVK_TALLY_ERRORS not touched
 *   scopes   scope 0 is every region; with a strata handle of L labels scope 1 + l is the regions of label l (context labels included)
 *   out      out[(scope * replicates + b) * AVK_TALLY_LEN + word]; sums are ADDED: a job sums over its batches and ranks (avk_counts_allreduce, or on the host)
 *   limits   1 <= replicates <= AVK_BOOT_MAX_REPLICATES and (1 + L) * replicates <= AVK_BOOT_MAX_BLOCKS, otherwise AVK_E_ARG before anything is queued, out untouched
 * A launch holds avk_boot_block(ctx) replicates of one scope; more replicates or scopes are more launches over the regions.  The submit / wait forms and the
 * merge take no spec. */
#include "../aardvark_amd/csrc/avk_boot.h"
typedef struct avk_boot_spec {
    uint32_t replicates;
    uint64_t seed;
} avk_boot_spec;
/* (the shared header defines the rule, host side: static inline uint32_t avk_boot_weight(uint64_t seed, uint32_t contig_idx, uint32_t start, uint32_t b)) */
uint32_t avk_boot_block(const avk_ctx *ctx);
/* resident form; preconditions and refusals are those of avk_label_tallies_strata: a device-packed batch (wide, compact or packed upload, with or without escapes)
 * after avk_compare_resident with the option emit_bp_groups set, otherwise AVK_E_STATE; a handle of another context is AVK_E_ARG.  strata == NULL: scope 0 only.
 * Called after avk_results_download it also counts the regions the capacity retry repaired. */
int  avk_boot_tallies(avk_ctx *ctx, avk_dev_batch *db, const avk_boot_spec *spec, const avk_strata *strata, uint64_t *out);
/* avk_compare_packed_strata that also returns the replicates (ADDED to boot_tallies).  Results, tally and label sums are bit for bit those of the call without a
 * spec; spec == NULL or replicates == 0 is exactly that call, launch for launch (boot_tallies is not read).  The library switches the BASEPAIR groups on itself;
 * regions the capacity retry repairs are counted.  strata == NULL or zero labels: scope 0 only, label_tallies is not read. */
int  avk_compare_packed_boot(avk_ctx *ctx, const avk_packed_batch *batch, const avk_packed_escapes *esc, const avk_strata *strata, const avk_compare_config *cfg,
                             avk_result_batch *out, uint64_t *label_tallies, const avk_boot_spec *spec, uint64_t *boot_tallies);
/* host only (no GPU involved): the same sums from a result batch — the route for batches that were not packed on the device (option device_pack 0).  Region r's
 * block comes from avk_group_metrics_from_compact(batch, r, res) — res needs what that function needs, and status or region_packed —, its key from
 * batch->contig_idx and batch->start, its scopes from labels (NULL: scope 0 only; a label named twice in a region's list counts twice).  threads: host threads
 * (0: one); the regions are cut among them, the sums do not depend on the cut. */
int  avk_boot_tallies_host(const avk_region_batch *batch, const avk_result_batch *res, const avk_boot_spec *spec, const avk_region_labels *labels, uint32_t threads,
                           uint64_t *out);

/* PER-CALL TALLIES BY SIZE BIN (avk_sizebin.inl; the rule is this project's own, stated in aardvark_amd/csrc/avk_sizebin.h and DESIGN.md section 5): how the
 * errors depend on the size of the variant — 1-5 bp indels against 6-15 bp against >= 50 bp — where every label above is a property of a region.
 *   size     size(call) = |a1_len - a0_len| of the call as the batch holds it (after the feeder's trimming, escaped lengths resolved); SNVs are size 0
 *   spec     avk_size_spec { n_edges, edges[AVK_SIZE_EDGES_MAX] }: 1 <= n_edges <= 15, edges[0] >= 1, strictly ascending — anything else is AVK_E_ARG, out
 *            untouched; n_bins = n_edges + 1; bin 0: size < edges[0]; bin j: edges[j - 1] <= size < edges[j]; the last bin: size >= edges[n_edges - 1].
 *            The default spec is {1, 6, 16, 50}: len_0, len_1_5, len_6_15, len_16_49, len_ge50
 *   call     a call of a SOLVED region (status 0) contributes one iteration of GroupMetrics::add_truth_zygosity (grouped_metrics.rs:183-227) as
 *            avk_group_metrics_from_compact states it per call — gt_tp, gt_fn, gt_fn_gt, hap_tp, hap_fn, w_tp, w_fn, the toggled reading of query entries and the
 *            32-bit products included — to the truth fields of its side or to the query fields, of group 0 and group 1 + type, in bin(size), in scope 0 and in
 *            scope 1 + l for every label l of the strata handle that holds the call's region
 *   block    out[((scope * n_bins + bin) * AVK_N_GROUPS + g) * AVK_SIZE_FIELDS + f], f = AVK_F_GT_TRUTH_TP .. AVK_F_WHAP_QUERY_FP (14 fields): GT, HAP and
 *            WEIGHTED_HAP only — BASEPAIR and RECORD_BP are properties of a region's haplotypes (waffle_solver.rs:335-522) and belong to no single call
 *   out      sums are ADDED; the block is additive over batches, slices, shards and ranks (avk_counts_allreduce takes it as it is)
 *   law      for every scope, group and f < 14 the sum over the bins equals word g * AVK_N_FIELDS + f of that scope's tally (avk_result_batch::tally for scope 0,
 *            the label's block of avk_label_tallies_strata for scope 1 + l)
 * The submit / wait forms and the merge take no spec. */
#include "../aardvark_amd/csrc/avk_sizebin.h"
uint32_t avk_size_n_bins(const avk_size_spec *spec);                                        /* n_edges + 1; 0 for a spec the rule refuses */
int  avk_size_bin_name(const avk_size_spec *spec, uint32_t j, char *buf, size_t cap);       /* len_<lo>_<hi> (inclusive), len_<lo> for one size, len_ge<lo> for the last bin */
uint32_t avk_size_block(const avk_ctx *ctx);                                                /* regions a workgroup of the kernel takes at a time */
/* resident form: a device-packed batch (wide, compact or packed upload, with or without escapes) after avk_compare_resident, otherwise AVK_E_STATE; neither
 * emit_bp_groups nor emit_group_metrics is needed; a handle of another context is AVK_E_ARG.  strata == NULL: scope 0 only.  Called after avk_results_download it
 * also counts the regions the capacity retry repaired. */
int  avk_size_tallies(avk_ctx *ctx, avk_dev_batch *db, const avk_size_spec *spec, const avk_strata *strata, uint64_t *out);
/* avk_compare_packed_esc that also returns the block (ADDED to size_out): results and tally are bit for bit those of the plain call; regions the capacity retry
 * repairs are counted.  strata == NULL or zero labels: scope 0 only.  The option device_pack 0 is AVK_E_STATE (host route: avk_size_tallies_host). */
int  avk_compare_packed_size(avk_ctx *ctx, const avk_packed_batch *batch, const avk_packed_escapes *esc, const avk_strata *strata, const avk_compare_config *cfg,
                             const avk_size_spec *spec, avk_result_batch *out, uint64_t *size_out);
/* host only (no GPU involved): the same sums from the wide batch and its results (status or region_packed; var_expected and var_observed, or var_packed), alt_ed
 * by avk_edit_distance's rule, scopes from labels (NULL: scope 0 only; a label named twice in a region's list counts twice).  threads: host threads (0: one); the
 * sums do not depend on the cut. */
int  avk_size_tallies_host(const avk_region_batch *batch, const avk_result_batch *res, const avk_size_spec *spec, const avk_region_labels *labels, uint32_t threads,
                           uint64_t *out);

/* PRECISION-RECALL CURVE BY QUERY SCORE (avk_score.inl; the rule is this project's own, stated in aardvark_amd/csrc/avk_score.h and DESIGN.md section 5): what
 * recall and precision the caller keeps at QUAL >= 20, at every threshold of a list, from ONE solve.  The curve is derived from that one comparison — as hap.py's
 * is — and so approximates K filtered re-runs: a filtered re-run could draw different regions.
 *   score    scores[n_variants], a float per call, indexed like the batch's call arrays; only query entries are read; NaN: missing
 *   spec     avk_score_spec { n_thresholds, t[AVK_SCORE_THRESHOLDS_MAX] }: 1 <= n_thresholds <= 31, every threshold finite, strictly ascending — anything else
 *            is AVK_E_ARG, out untouched; n_points = n_thresholds + 1; point 0: no filter; point k >= 1: score >= t[k - 1]
 *   bin      of a query call: the number of thresholds <= score in float32 (NaN: 0, +inf: n_thresholds, -inf: 0); kept at the points 0 .. bin.  Of a truth call:
 *            n_thresholds when its observed count is 0; otherwise the minimum bin over the query calls of its region with hap_tp > 0 (n_thresholds if none)
 *   point k  a query call with k <= bin adds the seven values of a call of the size rule to the query fields, otherwise nothing; a truth call with k <= bin adds
 *            them to the truth fields, otherwise its LOST values (gt_fn = 1, hap_fn = expected, w_fn = (u32)(expected * alt_ed)) — to group 0 and group 1 + type,
 *            in scope 0 and scope 1 + l for every label l of the strata handle that holds its region; unsolved regions add nothing
 *   block    out[((scope * n_points + k) * AVK_N_GROUPS + g) * AVK_SCORE_FIELDS + f], f = AVK_F_GT_TRUTH_TP .. AVK_F_WHAP_QUERY_FP; sums are ADDED
 *   law      point 0 is the size block summed over its bins, i.e. the first 14 fields of the tally; GT_TRUTH_TP + GT_TRUTH_FN and HAP_TRUTH_TP + HAP_TRUTH_FN
 *            are the same at every point; every TP field and every query field is non-increasing in k
 * The submit / wait forms, the hash-sharded route and the merge take no spec. */
#include "../aardvark_amd/csrc/avk_score.h"
uint32_t avk_score_n_points(const avk_score_spec *spec);                                    /* n_thresholds + 1; 0 for a spec the rule refuses */
int  avk_score_point_name(const avk_score_spec *spec, uint32_t k, char *buf, size_t cap);   /* score_all for point 0, score_ge_<t> (%g) for the others */
uint32_t avk_score_block(const avk_ctx *ctx);                                               /* regions a workgroup of the histogram kernel takes at a time */
/* resident form: a device-packed batch after avk_compare_resident, otherwise AVK_E_STATE; scores (host, n_variants floats; NULL: AVK_E_ARG) are copied into a pool
 * buffer on the call's stream.  strata == NULL: scope 0 only.  An error word from the kernel keeps the block from reaching out. */
int  avk_score_tallies(avk_ctx *ctx, avk_dev_batch *db, const avk_score_spec *spec, const float *scores, const avk_strata *strata, uint64_t *out);
/* avk_compare_packed_esc that also returns the block (ADDED to score_out): results and tally are bit for bit those of the plain call.  The option device_pack 0
 * is AVK_E_STATE (host route: avk_score_tallies_host). */
int  avk_compare_packed_score(avk_ctx *ctx, const avk_packed_batch *batch, const avk_packed_escapes *esc, const avk_strata *strata, const avk_compare_config *cfg,
                              const avk_score_spec *spec, const float *scores, avk_result_batch *out, uint64_t *score_out);
/* host only (no GPU involved): the same rule from the wide batch and its results, scopes from labels (NULL: scope 0 only).  threads: host threads (0: one) */
int  avk_score_tallies_host(const avk_region_batch *batch, const avk_result_batch *res, const avk_score_spec *spec, const float *scores,
                            const avk_region_labels *labels, uint32_t threads, uint64_t *out);

/* PER-CALL TALLIES BY CALL KIND (avk_callkind.inl; the rule is this project's own, stated in aardvark_amd/csrc/avk_callkind.h and DESIGN.md section 5): what kind
 * of call the errors are — the het/hom and Ti/Tv figures every small-variant benchmark carries.
 *   kind     kind(call) = 3 * gt + sub, AVK_N_KINDS = 9: het_ts het_tv het_other hom_ts hom_tv hom_other nogt_ts nogt_tv nogt_other (avk_kind_name)
 *   gt       from the call's INPUT zygosity (var_zyg / var_type_zyg, not the resolved zygosity of the per-call word): 0 het for AVK_ZYG_UNPHASED_HET,
 *            _PHASED_HET01 and _PHASED_HET10; 1 hom for AVK_ZYG_HOM_ALT; 2 nogt for anything else
 *   sub      from the two alleles as the batch holds them (escaped lengths resolved), whatever the call's type: if a0_len == 1 and a1_len == 1, the two bytes
 *            folded to upper case (b & 0xDF) are both one of A C G T and they differ: 0 ts for {A,G} and {C,T}, 1 tv otherwise.  Every other call is 2 other:
 *            longer or empty alleles, equal bases, N, IUPAC codes, an allele offset outside the allele array
 *   call     the size rule's contribution (above): the seven values of a call of a SOLVED region, to the truth fields of a truth call or the query fields of a
 *            query call, of group 0 and group 1 + type, in kind(call), in scope 0 and in scope 1 + l for every label l of the strata handle that holds the
 *            call's region; unsolved regions and regions whose call ranges lie outside the batch add nothing
 *   block    out[((scope * AVK_N_KINDS + kind) * AVK_N_GROUPS + g) * AVK_SIZE_FIELDS + f], 64-bit; sums are ADDED; additive over batches, slices, shards, ranks
 *   law      for every scope, group and f < 14 the sum over the kinds equals the size block summed over its bins: word g * AVK_N_FIELDS + f of that scope's tally
 * The submit / wait forms and the merge take no kinds. */
#include "../aardvark_amd/csrc/avk_callkind.h"
uint32_t avk_kind_n(void);                                      /* AVK_N_KINDS */
int  avk_kind_name(uint32_t k, char *buf, size_t cap);          /* the name of kind k; AVK_E_ARG for k >= AVK_N_KINDS or a buffer that is too small */
uint32_t avk_kind_block(const avk_ctx *ctx);                    /* regions a workgroup of the kernel takes at a time */
/* resident form: a device-packed batch (wide, compact or packed upload, with or without escapes) after avk_compare_resident, otherwise AVK_E_STATE; out == NULL is
 * AVK_E_ARG; both leave out untouched.  A handle of another context is AVK_E_ARG.  strata == NULL: scope 0 only.  Called after avk_results_download it also counts
 * the regions the capacity retry repaired. */
int  avk_kind_tallies(avk_ctx *ctx, avk_dev_batch *db, const avk_strata *strata, uint64_t *out);
/* avk_compare_packed_esc that also returns the block (ADDED to kind_out): results and tally are bit for bit those of the plain call; regions the capacity retry
 * repairs are counted.  strata == NULL or zero labels: scope 0 only.  The option device_pack 0 is AVK_E_STATE (host route: avk_kind_tallies_host). */
int  avk_compare_packed_kind(avk_ctx *ctx, const avk_packed_batch *batch, const avk_packed_escapes *esc, const avk_strata *strata, const avk_compare_config *cfg,
                             avk_result_batch *out, uint64_t *kind_out);
/* host only (no GPU involved): the same sums from the wide batch and its results (status or region_packed; var_expected and var_observed, or var_packed), alt_ed
 * by avk_edit_distance's rule, scopes from labels (NULL: scope 0 only; a label named twice in a region's list counts twice).  threads: host threads (0: one); the
 * sums do not depend on the cut. */
int  avk_kind_tallies_host(const avk_region_batch *batch, const avk_result_batch *res, const avk_region_labels *labels, uint32_t threads, uint64_t *out);

/* BOOTSTRAP REPLICATES OF THE PER-CALL BLOCKS (avk_callboot.inl; the rule is stated in aardvark_amd/csrc/avk_callboot.h and DESIGN.md section 5): the replicates
 * avk_boot_tallies gives the tallies, for the size-bin block and the call-kind block — what an interval on the recall of len_ge50, on het_tv precision or on a
 * Ti/Tv ratio is made from.  No new randomness:
 *   rule     out[scope][b][key][g][f] = sum over the scope's solved regions r of w(r, b) * X_r[key][g][f]; w = avk_boot_weight (the same seed gives a region the
 *            same weight as in avk_boot_tallies); X_r = region r's contribution to avk_size_tallies' block (key = bin) or avk_kind_tallies' block (key = kind),
 *            with every refusal of those stages
 *   block    out[AVK_CALLBOOT_AT(scope, B, b, n_keys, key, g, f)] = out[(((scope * B + b) * n_keys + key) * AVK_N_GROUPS + g) * AVK_SIZE_FIELDS + f], 64-bit; sums
 *            are ADDED; additive over batches, slices, shards and contexts
 *   cap      1 <= replicates <= AVK_BOOT_MAX_REPLICATES and (1 + labels) * replicates * n_keys <= AVK_CALLBOOT_MAX_BLOCKS, otherwise AVK_E_ARG
 *   law      replicate b summed over its keys is words g * AVK_N_FIELDS + f (f < 14) of replicate b of avk_boot_tallies, for the same seed
 * There is no one-call avk_compare_packed_* form and no submit / wait form: a caller that wants these replicates keeps the batch resident. */
#include "../aardvark_amd/csrc/avk_callboot.h"
uint32_t avk_callboot_block(avk_ctx *ctx, uint32_t n_keys);     /* replicates of one scope a launch holds for n_keys keys (1 .. 16; 0 otherwise): more are more launches */
/* resident forms: the preconditions and refusals of avk_size_tallies / avk_kind_tallies, the replicate count's and the cap's; every refusal leaves out untouched */
int  avk_size_boot_tallies(avk_ctx *ctx, avk_dev_batch *db, const avk_size_spec *size_spec, const avk_boot_spec *boot_spec, const avk_strata *strata, uint64_t *out);
int  avk_kind_boot_tallies(avk_ctx *ctx, avk_dev_batch *db, const avk_boot_spec *boot_spec, const avk_strata *strata, uint64_t *out);
/* host only (no GPU involved): the same sums, bit for bit, from the wide batch (with its start array) and its results, as avk_size_tallies_host / avk_kind_tallies_host
 * read them; a label named twice in a region's list counts twice.  threads: host threads (0: one); the sums do not depend on the cut. */
int  avk_size_boot_tallies_host(const avk_region_batch *batch, const avk_result_batch *res, const avk_size_spec *size_spec, const avk_boot_spec *boot_spec,
                                const avk_region_labels *labels, uint32_t threads, uint64_t *out);
int  avk_kind_boot_tallies_host(const avk_region_batch *batch, const avk_result_batch *res, const avk_boot_spec *boot_spec, const avk_region_labels *labels, uint32_t threads,
                                uint64_t *out);

/* SEQUENCE-CONTEXT labels (avk_context.inl): labels that are functions of the reference sequence alone, made by kernel from the reference avk_ref_upload left in
 * HBM — a stratified job needs no BED set for them.  The rule is this project's own (the reference has no such labels):
 *   window   a region's query is the one the interval sets get, [first, last] on its contig; a family's window is [first - pad, last + 1 + pad), clamped to the
 *            contig.  A region without a query (see avk_strata_upload) has no context label.
 *   bases    a base counts when its byte is an upper-case A, C, G or T; every other byte is left out of every count and ends a run.
 *   GC       n_gc_edges percent values in 0..101, strictly ascending, make n_gc_edges - 1 labels.  g = C or G bases of the window, a = counted bases: label i
 *            is set when a > 0 and gc_edges[i] * a <= 100 * g < gc_edges[i + 1] * a (integers).
 *   runs     n_hp_edges run lengths >= 1, strictly ascending, make n_hp_edges labels.  L = the longest run of one counted base inside the window (cut at its
 *            edges): label i is set when hp_edges[i] <= L < hp_edges[i + 1], the last one when L >= hp_edges[n_hp_edges - 1].
 * A family with no edges does not exist; a region gets at most one label per family.  In a handle the context labels follow the BED labels: context label j
 * (GC labels first, then the run labels) is label n_bed + j of every list, mask and sum. */
#define AVK_CONTEXT_PAD_MAX 1024
#define AVK_CONTEXT_GC_EDGES_MAX 17
#define AVK_CONTEXT_HP_EDGES_MAX 16
typedef struct avk_context_spec {
    uint32_t gc_pad, n_gc_edges, gc_edges[AVK_CONTEXT_GC_EDGES_MAX];
    uint32_t hp_pad, n_hp_edges, hp_edges[AVK_CONTEXT_HP_EDGES_MAX];
} avk_context_spec;
/* avk_strata_upload plus the context labels of `spec` behind its n_labels BED labels.  spec == NULL: avk_strata_upload.  n_labels == 0 with a spec: a handle of
 * context labels only (n_contigs is still required: it must be the uploaded reference's).  AVK_E_ARG, with nothing allocated (no device needed: ctx may be NULL):
 * edges that are not strictly ascending, a GC edge above 101, a run edge of 0, n_gc_edges == 1 or above 17, n_hp_edges above 16, a pad above 1024, both families
 * empty.  Every entry point that takes a handle takes this one; each refuses it with AVK_E_ARG, before anything is queued and with the caller's sums untouched,
 * when the context has no reference or its reference has another number of contigs than the handle.  The reference is read where the kernel is queued, on the
 * batch's own stream for a submitted batch: as for the solver kernels, avk_ref_upload must not be called while tickets are in flight.  A handle without context
 * labels queues exactly the launches avk_strata_upload's does. */
int  avk_strata_upload_context(avk_ctx *ctx, uint32_t n_labels, uint32_t n_contigs, const uint64_t *tree_off, const uint32_t *start, const uint32_t *end_max,
                               const avk_context_spec *spec, avk_strata **out);
/* the number of context labels of a handle (avk_strata_n_labels is the total) */
uint32_t avk_strata_n_context_labels(const avk_strata *strata);
/* host only: the stable name of context label j of a spec into buf (NUL-terminated, cut at cap): ctx_gc_<lo>_<hi> (percent, hi exclusive), ctx_hp_<lo>_<hi - 1>
 * (run lengths, inclusive), ctx_hp_ge<lo> for the open-ended last one.  AVK_E_ARG: an invalid spec, j beyond its labels, no room. */
int  avk_context_label_name(const avk_context_spec *spec, uint32_t j, char *buf, size_t cap);

/* Merge path (src/merge_solver.rs:137-143): for pair p, optimize_sequences(set a, set b) and
 * report all_opt_haps[0].is_exact_match().  Pair p compares variant ranges
 * [t_off,t_cnt) vs [q_off,q_cnt) of region p of `batch` exactly like a CompareRegion. */
int  avk_optimize_pairs_batch(avk_ctx *ctx, const avk_region_batch *batch, uint32_t max_branch_factor,
                              int32_t *status, uint8_t *is_exact_match);

/* solve_merge_region (src/merge_solver.rs:110-200) for regions with k inputs each.  The expensive part is the all-pairs
 * exact-match test above; the classification on top of the pair matrix is host logic:
 *   MergeClassification (src/data_types/merge_benchmark.rs:5-14) -> AVK_MERGE_*; `members` = bit i set for the input indices
 *   of NoConflict / MajorityAgree, or the selected index itself for ConflictSelection. */
enum {
    AVK_MERGE_DIFFERENT = 0, AVK_MERGE_IDENTICAL = 1, AVK_MERGE_NO_CONFLICT = 2, AVK_MERGE_MAJORITY_AGREE = 3,
    AVK_MERGE_CONFLICT_SELECTION = 4
};
typedef struct avk_merge_config { /* MergeConfig (src/merge_solver.rs:62-84) */
    uint32_t max_branch_factor;      /* default 50 */
    uint32_t no_conflict_enabled;
    uint32_t majority_voting_enabled;
    int32_t  conflict_selection;     /* -1 = None */
} avk_merge_config;
/* A batch of MultiRegions (src/data_types/multi_region.rs): region m, input i owns variants
 * [in_off[m*k + i], +in_cnt[m*k + i]) of the variant arrays (same meaning as in avk_region_batch). */
typedef struct avk_multi_batch {
    uint64_t n_regions;
    uint32_t n_inputs;               /* k, 2..64 */
    const uint64_t *region_id;
    const uint32_t *contig_idx;
    const uint64_t *start, *end;
    const uint64_t *in_off;          /* [n_regions * k] */
    const uint32_t *in_cnt;          /* [n_regions * k] */
    uint64_t n_variants;
    const uint64_t *var_pos;
    const uint8_t  *var_type, *var_zyg;
    const uint32_t *var_raw_space;
    const uint64_t *a0_off; const uint32_t *a0_len;
    const uint64_t *a1_off; const uint32_t *a1_len;
    const uint8_t  *allele_bytes; uint64_t allele_bytes_len;
} avk_multi_batch;
/* The same batch in the PACKED form (round 3; avk_packed_batch's rules): every offset implied by order — the calls of region m follow those of region
 * m - 1, input by input; the alleles of call v follow those of call v - 1 (allele0, then allele1); call positions are relative to their region's start.
 * 8 + k bytes per region and 5 per call plus the allele bytes: a three-caller whole genome crosses PCIe as 0.13 GB instead of 0.72.  Constraints: windows
 * shorter than 65,536 bases, at most 255 calls per region and input, alleles of at most 255 bases — these three hold WITHOUT ESCAPES (avk_packed_escapes;
 * count slot m * k + i is in_cnt[m * k + i]) —, fewer than 2^32 calls and allele bytes, contigs shorter than 4 Gbp, at most 65,535 contigs. */
typedef struct avk_packed_multi_batch {
    uint64_t n_regions;
    uint32_t n_inputs;               /* k, 2..64 */
    const uint16_t *contig_idx;      /* [n_regions] may be NULL (contig 0) */
    const uint32_t *start;           /* [n_regions] */
    const uint16_t *len;             /* [n_regions] end - start */
    const uint8_t  *in_cnt;          /* [n_regions * k] */
    uint64_t n_variants;             /* = sum of in_cnt */
    const uint16_t *var_rel_pos;     /* [n_variants] position - the region's start */
    const uint8_t  *var_type_zyg;    /* [n_variants] AVK_VT_* | AVK_ZYG_* << 4 */
    const uint8_t  *a0_len, *a1_len; /* [n_variants] */
    const uint32_t *var_raw_space;   /* [n_variants] may be NULL (= the longer allele) */
    const uint8_t  *allele_bytes; uint64_t allele_bytes_len; /* = sum of a0_len + a1_len */
} avk_packed_multi_batch;
/* Host only (no GPU): classification from the pair results.  The pairs of region m are the k(k-1)/2 pairs (i < j) in
 * lexicographic order starting at m * k(k-1)/2; has_unknown_zyg[m] != 0 = some variant of the region has an Unknown zygosity
 * (variant_delta_length bails first, :119-124 -> status AVK_ST_BAD_ZYGOSITY). */
int avk_merge_classify(uint64_t n_regions, uint32_t n_inputs, const uint32_t *in_cnt, const uint8_t *has_unknown_zyg,
                       const int32_t *pair_status, const uint8_t *pair_exact, const avk_merge_config *cfg,
                       int32_t *status, uint8_t *classification, uint64_t *members);
/* All of solve_merge_region for a batch: pairs on the GPU, classification on the host. */
int avk_merge_batch(avk_ctx *ctx, const avk_multi_batch *batch, const avk_merge_config *cfg,
                    int32_t *status, uint8_t *classification, uint64_t *members);
/* the same for a batch in the packed form (offsets by two prefix sums on the device, one kernel that writes the wide arrays there) */
int avk_merge_packed(avk_ctx *ctx, const avk_packed_multi_batch *batch, const avk_merge_config *cfg,
                     int32_t *status, uint8_t *classification, uint64_t *members);
/* ... with escapes (NULL: avk_merge_packed) */
int avk_merge_packed_esc(avk_ctx *ctx, const avk_packed_multi_batch *batch, const avk_packed_escapes *esc, const avk_merge_config *cfg,
                         int32_t *status, uint8_t *classification, uint64_t *members);

/* ---- merge on several GPUs (BASELINE configs[4]): merge regions are mapped exactly like compare regions (src/main.rs:463-478), so the same rule cuts a packed
 * multi-region batch: avk_packed_multi_shard_make gathers the regions rank `rank` of `world` owns (avk_region_shard of region_id[r], or of first_id + r), in the
 * whole batch's order; _scatter writes the shard's status / classification / members at the regions' places in the whole batch's arrays.  The only state a merge
 * keeps across regions is MergeSummaryWriter's map (merge reason with its indices, variant type, input) -> (pass, fail) variant counts
 * (src/writers/merge_summary.rs:12-18, filled by add_merge_benchmark :57-81): avk_merge_counts ADDS a solved batch to a dense block of avk_merge_counts_len(k)
 * sums — entry ((reason * AVK_N_VARIANT_TYPES + type) * k + input) * 2 + (0 pass | 1 fail), reason = avk_merge_counts_reason() — which the ranks sum with one
 * avk_counts_allreduce (RCCL) or on the host, and avf_write_merge_summary_counts of the feeder library writes as the reference's table.  Dense blocks exist for
 * k <= AVK_MERGE_COUNTS_MAX_INPUTS inputs (the reasons carry a subset of the inputs: 2 + 2 * 2^k + k of them); avk_merge_counts_len is 0 beyond, and a job with
 * more inputs writes its summary from the scattered per-region arrays (avf_write_merge_summary).  avk_merge_packed_counts (below) makes a batch's block with the
 * merge call itself, by a kernel behind the classification: no pass over the results on the host. */
typedef struct avk_packed_multi_shard avk_packed_multi_shard;
int  avk_packed_multi_shard_make(const avk_packed_multi_batch *whole, const uint64_t *region_id, uint64_t first_id, uint32_t rank, uint32_t world,
                                 avk_packed_multi_shard **out);
int  avk_packed_multi_shard_make_esc(const avk_packed_multi_batch *whole, const avk_packed_escapes *esc, const uint64_t *region_id, uint64_t first_id, uint32_t rank,
                                     uint32_t world, avk_packed_multi_shard **out);
const avk_packed_multi_batch *avk_packed_multi_shard_batch(const avk_packed_multi_shard *s);
const avk_packed_escapes *avk_packed_multi_shard_escapes(const avk_packed_multi_shard *s);
uint64_t avk_packed_multi_shard_regions(const avk_packed_multi_shard *s, const uint64_t **index_in_whole);
int  avk_packed_multi_shard_scatter(const avk_packed_multi_shard *s, const int32_t *status, const uint8_t *classification, const uint64_t *members,
                                    int32_t *whole_status, uint8_t *whole_classification, uint64_t *whole_members);
void avk_packed_multi_shard_free(avk_packed_multi_shard *s);
#define AVK_MERGE_COUNTS_MAX_INPUTS 10
uint64_t avk_merge_counts_len(uint32_t n_inputs);
uint32_t avk_merge_counts_reason(uint32_t n_inputs, uint8_t classification, uint64_t members);
int  avk_merge_counts(const avk_packed_multi_batch *batch, const int32_t *status, const uint8_t *classification, const uint64_t *members, uint64_t *counts);
/* the same for a batch with escapes (it reads in_cnt; NULL: avk_merge_counts) */
int  avk_merge_counts_esc(const avk_packed_multi_batch *batch, const avk_packed_escapes *esc, const int32_t *status, const uint8_t *classification, const uint64_t *members,
                          uint64_t *counts);
/* The counters WITH the merge call: avk_merge_packed_esc that also ADDS the batch's dense block to counts[avk_merge_counts_len(k)].  Everything
 * avk_merge_counts_esc reads is on the device when the classification ends, so on the device route (device_pack on, k <= 8, a batch that is not empty) a kernel
 * counts there — one lane per (region, input), sums kept in the workgroup's LDS where the block of k inputs fits it (avk_merge_counts_in_lds: k <= 6 with
 * 160 KB) and reduced within the wave beyond — and the block comes back with status / classification / members; every other batch (k = 9 or 10,
 * device_pack = 0, no regions) is solved as by avk_merge_packed_esc and counted by avk_merge_counts_esc here.  The sums are the host function's, word for word.
 *   counts == NULL: avk_merge_packed_esc, launch for launch.
 *   AVK_E_ARG before anything is queued: counts != NULL with n_inputs outside [2, AVK_MERGE_COUNTS_MAX_INPUTS].
 *   AVK_E_ARG with counts untouched: a batch avk_merge_counts_esc refuses, and a call whose type nibble is >= AVK_N_VARIANT_TYPES in ANY region (the host
 *   function looks at solved regions only; such a call leaves its region unsolved).  The three result arrays are then what the call without counters writes.
 * avk_last_merge_counts_on_device: 1 when the context's last call with counters made them by kernel. */
int  avk_merge_packed_counts(avk_ctx *ctx, const avk_packed_multi_batch *batch, const avk_packed_escapes *esc, const avk_merge_config *cfg, int32_t *status,
                             uint8_t *classification, uint64_t *members, uint64_t *counts /* [avk_merge_counts_len(k)], ADDED to */);
int  avk_last_merge_counts_on_device(avk_ctx *ctx);
int  avk_merge_counts_in_lds(avk_ctx *ctx, uint32_t n_inputs); /* 1: the count kernel of this context keeps the block of n_inputs inputs in LDS */

/* ---- one pair solve, several strategies.  The pair matrix of a region depends on the batch and on max_branch_factor alone (src/merge_solver.rs:125-164); the
 * switches no_conflict_enabled / majority_voting_enabled / conflict_selection are read when the last pair is solved (:166-197).  avk_merge_packed_sweep is
 * avk_merge_packed_counts for n_cfgs configs at once: ONE upload and ONE pair solve, then every config's decision — status[n] is the same for all of them,
 * classification and members are config-major: config c owns [c * n, (c + 1) * n) —, and with counts != NULL config c's dense block is ADDED to
 * counts + c * avk_merge_counts_len(k).  On the device route (device_pack on, 2 <= k <= 8, a batch that is not empty) one kernel behind the pair solve reads every
 * region's pair records once and writes all configs' decisions, the count kernel runs once per config behind it on the call's stream, and everything comes back in
 * one copy; every other batch (k = 1 or k > 8, device_pack = 0, no regions) is solved once through the host route, decided by avk_merge_classify_sweep and counted
 * by avk_merge_counts_esc per config.  The answers are the same either way, for every k <= 64, and with n_cfgs = 1 they are avk_merge_packed_counts' word for word.
 *   AVK_E_ARG before anything is queued, with nothing written: n_cfgs is 0 or above AVK_MERGE_SWEEP_MAX; the configs do not all carry the same max_branch_factor
 *   (the pair solve depends on it); a conflict_selection is >= k or < -1; counts != NULL with k outside [2, AVK_MERGE_COUNTS_MAX_INPUTS].
 *   Duplicate configs are allowed.
 *   AVK_E_ARG with counts untouched FOR EVERY CONFIG: what avk_merge_packed_counts refuses (one refused config refuses the call).
 * avk_last_merge_counts_on_device is 1 afterwards only when all configs were counted by kernel. */
#define AVK_MERGE_SWEEP_MAX 8
int  avk_merge_packed_sweep(avk_ctx *ctx, const avk_packed_multi_batch *batch, const avk_packed_escapes *esc, uint32_t n_cfgs, const avk_merge_config *cfgs,
                            int32_t *status /* [n] */, uint8_t *classification /* [n_cfgs * n], config-major */, uint64_t *members /* [n_cfgs * n] */,
                            uint64_t *counts /* NULL, or [n_cfgs * avk_merge_counts_len(k)], ADDED to */);
/* Host only (no GPU): the same decisions from a given pair matrix — avk_merge_classify's arguments with several configs (their max_branch_factor is not read).
 * AVK_E_ARG with nothing written: a NULL array, n_inputs outside [1, 64], n_cfgs 0 or above AVK_MERGE_SWEEP_MAX, a conflict_selection >= n_inputs or < -1. */
int  avk_merge_classify_sweep(uint64_t n_regions, uint32_t n_inputs, const uint32_t *in_cnt, const uint8_t *has_unknown_zyg, const int32_t *pair_status,
                              const uint8_t *pair_exact, uint32_t n_cfgs, const avk_merge_config *cfgs, int32_t *status, uint8_t *classification, uint64_t *members);

/* Host utility (no GPU involved): unit-cost edit distance of two byte strings, the value of the reference's
 * wfa_ed (src/util/sequence_alignment.rs:9-13).  The batch packer uses it for Variant::alt_ed
 * (src/data_types/variants.rs:413-415), which travels to the device with the region records. */
uint64_t avk_edit_distance(const uint8_t *a, uint64_t a_len, const uint8_t *b, uint64_t b_len);

const char *avk_version(void);
/* the build's identity: the first 16 hex digits of the SHA-256 of the kernel and host sources the library was compiled from (csrc/Makefile), "unknown" for a
 * build made another way.  Measurement files (profiles/rNN_pmc_traffic.json) carry it; bench.py reports counter traffic only when it matches the loaded library. */
const char *avk_source_hash(void);

#ifdef __cplusplus
}
#endif
#endif /* AARDVARK_AMD_H */
