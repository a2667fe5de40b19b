/*
 * avk_mergesweep.inl — one pair solve of a merge batch decided under several strategies (avk_merge_packed_sweep, avk_merge_classify_sweep).
 *
 * solve_merge_region (src/merge_solver.rs:110-200) has two halves.  The pair matrix of a region (:125-164) depends on the batch and on max_branch_factor alone;
 * the strategy switches — no_conflict_enabled, majority_voting_enabled, conflict_selection — are read when the last pair is solved (:166-197).  merge_classify_one
 * (avk_devpack.inl) states both halves in one function; here they are two, split at that border:
 *   merge_facts_one   everything the ladder reads, from the pair matrix: status, all_identical, no_conflict, the inputs that are not empty, the first majority set
 *   merge_decide      the if / else if ladder on top of the facts, for ONE set of switches
 * For every input merge_facts_one followed by merge_decide is merge_classify_one (tests/test_merge_sweep_host.py).  The host function
 * avk_merge_classify_sweep (KMAX 64) and the kernel behind avk_merge_packed_sweep (KMAX 8) call the same two functions, as avk_merge_reason.h is shared.
 *
 * The kernel, avk_merge_sweep_kernel: one lane per MultiRegion like avk_dp_merge_classify_kernel, the region's pair records and zygosities read ONCE, status[m]
 * written once, then classification[c * n + m] / members[c * n + m] for every config c of the call — the configs come by value in the kernel argument, so the loop
 * over them is uniform, and lane m writes consecutive addresses within each config's slice.  ms_sweep_lane is one-lane code without cross-lane primitives:
 * tests/native/merge_sweep_check.cpp runs the SAME function on the CPU, under the sanitizers.
 */
#ifndef AVK_MERGESWEEP_INL
#define AVK_MERGESWEEP_INL

#include "avk_merge_reason.h"
#include "avk_wave.h"

namespace avk {
namespace ms {

enum { MS_KMAX = 8 /* = DP_MERGE_KMAX: regions with more inputs are decided by the host function */, MS_MAX_CFGS = AVK_MERGE_SWEEP_MAX };

/* the strategy-independent part of a region's decision */
struct MergeFacts {
    int32_t status;          /* AVK_ST_BAD_ZYGOSITY first, else the first non-zero pair status in lexicographic order; the other fields are 0 then */
    uint32_t all_identical;  /* every pair is an exact match */
    uint32_t no_conflict;    /* every pair has an empty side or is an exact match (:160-164) */
    uint64_t nonempty;       /* bit i: cnt[i] != 0 */
    uint64_t first_majority; /* the match set of the lowest i whose set has at least k / 2 + 1 members, else 0 */
};
/* the switches of one avk_merge_config (12 bytes: max_branch_factor belongs to the pair solve) */
struct MsCfg {
    uint32_t no_conflict_enabled, majority_voting_enabled;
    int32_t conflict_selection;
};

/* The match sets of a region's inputs: row i has bit j set when inputs i and j are an exact match (and bit i).  Up to 64 inputs: a word per input.  Up to 8: the
 * eight rows of eight bits are ONE 64-bit word, so the kernel keeps them in a register pair whatever the index — no array, nothing for scratch. */
template <int KMAX>
struct MatchRows {
    uint64_t row[KMAX];
    AVK_DEV_MEMBER void init(uint32_t k) {
        for (uint32_t i = 0; i < k && i < (uint32_t)KMAX; ++i) row[i] = 1ull << i;
    }
    AVK_DEV_MEMBER void match(uint32_t i, uint32_t j) { row[i] |= 1ull << j, row[j] |= 1ull << i; }
    AVK_DEV_MEMBER uint64_t of(uint32_t i) const { return row[i]; }
};
template <>
struct MatchRows<8> {
    uint64_t rows;
    AVK_DEV_MEMBER void init(uint32_t) { rows = 0x8040201008040201ull; }
    AVK_DEV_MEMBER void match(uint32_t i, uint32_t j) { rows |= (1ull << (8u * i + j)) | (1ull << (8u * j + i)); }
    AVK_DEV_MEMBER uint64_t of(uint32_t i) const { return (rows >> (8u * i)) & 0xFFull; }
};

/* merge_classify_one up to the strategy border, for ONE region with at most KMAX inputs: the same walk over the pairs (lexicographic, pair(p, st, ex) hands out
 * status and exact-match flag of pair p), the same return at the first pair that is not solved */
template <int KMAX, class PairFn>
AVK_HD void merge_facts_one(uint32_t k, const uint32_t *cnt, bool has_unknown, PairFn pair, MergeFacts *f) {
    f->status = 0, f->all_identical = 0, f->no_conflict = 0, f->nonempty = 0, f->first_majority = 0;
    if (has_unknown) { /* variant_delta_length bails on an Unknown zygosity before anything else */
        f->status = AVK_ST_BAD_ZYGOSITY;
        return;
    }
    bool all_identical = true, no_conflict = true;
    uint64_t nonempty = 0;
    for (uint32_t i = 0; i < k; ++i) nonempty |= (uint64_t)(cnt[i] != 0) << i;
    MatchRows<KMAX> match;
    match.init(k);
    uint64_t p = 0;
    for (uint32_t i = 0; i < k; ++i)
        for (uint32_t j = i + 1; j < k; ++j, ++p) {
            int32_t pst;
            bool ex;
            pair(p, pst, ex);
            if (pst != 0) {
                f->status = pst;
                return;
            }
            all_identical = all_identical && ex;
            no_conflict = no_conflict && (((nonempty >> i) & (nonempty >> j) & 1ull) == 0 || ex);
            if (ex) match.match(i, j);
        }
    const uint32_t majority = k / 2 + 1;
    uint64_t first_majority = 0;
    for (uint32_t i = 0; i < k && !first_majority; ++i) {
        uint32_t pc = 0;
        for (uint64_t x = match.of(i); x; x &= x - 1) ++pc;
        if (pc >= majority) first_majority = match.of(i);
    }
    f->all_identical = all_identical ? 1u : 0u, f->no_conflict = no_conflict ? 1u : 0u, f->nonempty = nonempty, f->first_majority = first_majority;
}

/* merge_classify_one's ladder (:166-197) for one set of switches, reading the facts only */
AVK_HD void merge_decide(const MergeFacts &f, const MsCfg &cfg, uint8_t *classification, uint64_t *members) {
    *classification = AVK_MERGE_DIFFERENT;
    *members = 0;
    if (f.status != 0) return;
    if (f.all_identical) *classification = AVK_MERGE_IDENTICAL;
    else if (cfg.no_conflict_enabled && f.no_conflict) {
        *classification = AVK_MERGE_NO_CONFLICT;
        *members = f.nonempty;
    } else if (cfg.majority_voting_enabled && f.first_majority) {
        *classification = AVK_MERGE_MAJORITY_AGREE;
        *members = f.first_majority;
    } else if (cfg.conflict_selection >= 0) {
        *classification = AVK_MERGE_CONFLICT_SELECTION;
        *members = (uint64_t)cfg.conflict_selection;
    }
}

/* what a sweep refuses of a config before anything else happens: a ConflictSelection index that is no input */
AVK_HD bool merge_sweep_cfg_ok(uint32_t k, const avk_merge_config &c) { return c.conflict_selection >= -1 && (c.conflict_selection < 0 || (uint32_t)c.conflict_selection < k); }

/* avk_merge_classify_sweep (include/aardvark_amd.h): avk_merge_classify's arguments with n_cfgs configs; classification / members are config-major.  Nothing is
 * written when an argument is refused.  Plain host code, so that a program of its own can run it under the sanitizers (tests/native/merge_sweep_check.cpp). */
static inline int merge_classify_sweep_host(uint64_t n_regions, uint32_t k, const uint32_t *in_cnt, const uint8_t *has_unknown_zyg, const int32_t *pair_status,
                                            const uint8_t *pair_exact, uint32_t n_cfgs, const avk_merge_config *cfgs, int32_t *status, uint8_t *classification,
                                            uint64_t *members) {
    if (!in_cnt || !cfgs || !status || !classification || !members || (n_regions && (!pair_status || !pair_exact))) return AVK_E_ARG;
    if (k < 1 || k > 64 || n_cfgs < 1 || n_cfgs > (uint32_t)MS_MAX_CFGS) return AVK_E_ARG;
    MsCfg sw[MS_MAX_CFGS];
    for (uint32_t c = 0; c < n_cfgs; ++c) {
        if (!merge_sweep_cfg_ok(k, cfgs[c])) return AVK_E_ARG;
        sw[c].no_conflict_enabled = cfgs[c].no_conflict_enabled, sw[c].majority_voting_enabled = cfgs[c].majority_voting_enabled, sw[c].conflict_selection = cfgs[c].conflict_selection;
    }
    const uint64_t ppr = (uint64_t)k * (k - 1) / 2;
    for (uint64_t m = 0; m < n_regions; ++m) {
        const int32_t *pst = pair_status + m * ppr;
        const uint8_t *pex = pair_exact + m * ppr;
        MergeFacts f;
        merge_facts_one<64>(k, in_cnt + m * k, has_unknown_zyg && has_unknown_zyg[m], [pst, pex](uint64_t p, int32_t &st, bool &ex) {
            st = pst[p];
            ex = pex[p] != 0;
        }, &f);
        status[m] = f.status;
        for (uint32_t c = 0; c < n_cfgs; ++c) merge_decide(f, sw[c], classification + (uint64_t)c * n_regions + m, members + (uint64_t)c * n_regions + m);
    }
    return AVK_E_OK;
}

/* the kernel's argument: the classification launch's view of the batch (DpMerge of avk_devpack.inl) with the call's configs by value */
struct MsSweep {
    const uint32_t *region_out; /* [n_multi * ppr][4] of the pair solve: status, exact */
    const uint64_t *in_off;
    const uint32_t *in_cnt;
    const uint8_t *var_zyg;
    uint64_t n_multi, n_variants;
    uint32_t k, ppr; /* k <= MS_KMAX */
    uint32_t n_cfgs; /* 1 .. MS_MAX_CFGS */
    MsCfg cfg[MS_MAX_CFGS];
    int32_t *status;         /* [n_multi] */
    uint8_t *classification; /* [n_cfgs * n_multi] config-major */
    uint64_t *members;       /* [n_cfgs * n_multi] */
};
AVK_DEV void ms_sweep_lane(const MsSweep &c, uint64_t m) {
    if (m >= c.n_multi) return;
    bool unknown = false;
    for (uint32_t i = 0; i < c.k; ++i) {
        const uint64_t off = c.in_off[m * c.k + i];
        const uint32_t cnt = c.in_cnt[m * c.k + i];
        for (uint32_t v = 0; v < cnt && off + v < c.n_variants; ++v) unknown = unknown || c.var_zyg[off + v] == AVK_ZYG_UNKNOWN;
    }
    const uint32_t *ro = c.region_out + 4 * (m * c.ppr);
    MergeFacts f;
    merge_facts_one<MS_KMAX>(c.k, c.in_cnt + m * c.k, unknown, [ro](uint64_t p, int32_t &pst, bool &ex) {
        pst = (int32_t)ro[4 * p];
        ex = pst == 0 && ro[4 * p + 1] != 0;
    }, &f);
    c.status[m] = f.status;
    for (uint32_t q = 0; q < c.n_cfgs && q < (uint32_t)MS_MAX_CFGS; ++q) {
        uint8_t cl;
        uint64_t mem;
        merge_decide(f, c.cfg[q], &cl, &mem);
        c.classification[(uint64_t)q * c.n_multi + m] = cl;
        c.members[(uint64_t)q * c.n_multi + m] = mem;
    }
}

} // namespace ms
} // namespace avk

#ifndef AVK_EMU
__global__ void __launch_bounds__(256) avk_merge_sweep_kernel(avk::ms::MsSweep c) { avk::ms::ms_sweep_lane(c, (uint64_t)blockIdx.x * 256u + threadIdx.x); }
#endif

#endif /* AVK_MERGESWEEP_INL */
