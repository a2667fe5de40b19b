/*
 * avk_strata.inl — the region -> containment-label lists of a stratified job, made ON THE DEVICE.
 *
 * Stratifications::containments (src/parsing/stratifications.rs:189-199) asks, for every label, whether one of its intervals contains the region's
 * CompareRegion::var_coordinates (compare_region.rs:54-66).  The feeder library answers with a std::map lookup and a binary search per (region, label) on host
 * threads (avf_strat_region_labels + reaches, avf_strat.cpp); the lists then cross PCIe with the batch.  Everything the question needs is on the device once a batch
 * is packed — the region's contig, its sides' first call and last call — and the interval sets are fixed for a job: avk_strata_upload keeps them in HBM as one
 * table of trees, tree (label l, contig c) = entries [tree_off[l * n_contigs + c], tree_off[l * n_contigs + c + 1]) of start[] (sorted) and end_max[] (running
 * maximum of the EXCLUSIVE ends), 32-bit coordinates.
 *
 * sx_region_in_label is the rule, one lane per (region, label); the kernels at the end ask it for every label of 256 consecutive regions — neighbours on the
 * genome searching the same tree, so a wave's searches visit the same few cache lines — and write the CSR lists avk_label_tally_compact_kernel reads:
 * 64-bit label_off, label_idx ascending within a region (the order of the host's loop over the labels).
 *
 * A batch in flight (avk_compare_packed_submit_strata) runs pass 1 alone: its tally reads the masks themselves (lb_region_labels_mask, avk_labels.inl), and neither
 * the scan nor pass 2 is queued for it.
 *
 * Written against avk_wave.h / DpIn like avk_labels.inl, so tests/emu/strata_emu.cpp runs the same rule on the CPU against the host's lists.
 */
#ifndef AVK_STRATA_INL
#define AVK_STRATA_INL

#include "avk_devpack.inl"

namespace avk {
namespace sx {

typedef dp::u32 u32;
typedef dp::u64 u64;

/* the resident interval sets (device pointers) */
struct SxTrees {
    const u64 *tree_off; /* [n_labels * n_contigs + 1] */
    const u32 *start;    /* sorted per tree */
    const u32 *end_max;  /* running maximum of the exclusive ends per tree */
    u32 n_labels, n_contigs;
};

/* CompareRegion::var_coordinates of region r as the query the trees get: [first, last] inclusive on `contig`; ok = false: the region has no labels (no calls,
 * start >= end, call ranges outside the batch, a contig the sets do not know).  The LAST call's end of each side, not the largest end; an empty side is skipped.
 * The status of the region plays no part. */
struct SxSpan {
    u64 first, last;
    u32 contig;
    bool ok;
};
AVK_DEV SxSpan sx_region_span(const dp::DpIn &in, u64 r, u32 n_contigs) {
    SxSpan s;
    s.first = s.last = 0, s.contig = 0, s.ok = false;
    if (r >= in.n_regions) return s;
    const u32 tc = in.t_cnt_of(r), qc = in.q_cnt_of(r);
    const u64 toff = in.t_off_of(r), qoff = in.q_off_of(r), nv = in.n_variants;
    if (toff > nv || (u64)tc > nv - toff || qoff > nv || (u64)qc > nv - qoff) return s;
    const u32 c = in.contig_of(r);
    if (c >= n_contigs) return s;
    const u64 rs = in.start_of(r);
    u64 start = ~0ull, end = 0;
    if (tc) {
        const u64 f = toff, l = toff + tc - 1, e = in.pos_of(l, rs) + in.a0_len_of(l), p = in.pos_of(f, rs);
        start = p < start ? p : start;
        end = e > end ? e : end;
    }
    if (qc) {
        const u64 f = qoff, l = qoff + qc - 1, e = in.pos_of(l, rs) + in.a0_len_of(l), p = in.pos_of(f, rs);
        start = p < start ? p : start;
        end = e > end ? e : end;
    }
    if (start >= end) return s;
    s.first = start, s.last = end - 1, s.contig = c, s.ok = true;
    return s;
}

/* reaches() of avf_strat.cpp on one tree [lo, hi): k = upper_bound(start, first); a hit when k > 0 and the running maximum in front of k reaches `last` —
 * with exclusive ends: last < end_max[k - 1].  An empty tree never hits. */
AVK_DEV bool sx_tree_hit(const SxTrees &t, u64 lo, u64 hi, u64 first, u64 last) {
    u64 a = lo, b = hi;
    while (a < b) { /* the first entry with start > first */
        const u64 mid = a + ((b - a) >> 1);
        if ((u64)t.start[mid] <= first) a = mid + 1;
        else b = mid;
    }
    return a > lo && last < (u64)t.end_max[a - 1];
}

/* THE RULE: is region r contained in label l */
AVK_DEV bool sx_region_in_label(const dp::DpIn &in, const SxTrees &t, u64 r, u32 l) {
    if (l >= t.n_labels) return false;
    const SxSpan s = sx_region_span(in, r, t.n_contigs);
    if (!s.ok) return false;
    const u64 at = (u64)l * t.n_contigs + s.contig;
    return sx_tree_hit(t, t.tree_off[at], t.tree_off[at + 1], s.first, s.last);
}

/* One word of a region's answers: bit j = the region is in label l0 + j, for the cnt <= 32 labels from l0.  bounds(l, lo, hi) hands out tree (l, sp.contig):
 * the mask kernel answers from the row it staged in LDS or from memory, the emulator from memory.  This is the lane's whole work per word in the mask kernel. */
template <class Bounds>
AVK_DEV u32 sx_mask_word(const SxTrees &t, const SxSpan &sp, u32 l0, u32 cnt, Bounds &&bounds) {
    u32 word = 0;
    if (!sp.ok) return 0;
    for (u32 j = 0; j < cnt; ++j) {
        u64 lo, hi;
        bounds(l0 + j, lo, hi);
        if (sx_tree_hit(t, lo, hi, sp.first, sp.last)) word |= 1u << j;
    }
    return word;
}
/* the word-major place of region r's word w in the masks of n regions */
AVK_DEV u64 sx_mask_at(u32 w, u64 r, u64 n) { return (u64)w * n + r; }
/* a region's list from its mask words, ascending, at label_idx[at ..) (stores bounded by idx_cap); returns the number of entries */
AVK_DEV u32 sx_fill_region(const u32 *mask, u64 r, u64 n, u32 n_words, u32 *label_idx, u64 at, u64 idx_cap) {
    u32 k = 0;
    for (u32 w = 0; w < n_words; ++w)
        for (u32 x = mask[sx_mask_at(w, r, n)]; x; x &= x - 1u, ++k)
            if (label_idx && at + k < idx_cap) label_idx[at + k] = w * 32u + (u32)avk_ctz64((u64)x);
    return k;
}

} // namespace sx
} // namespace avk

#ifndef AVK_EMU
/* Pass 1: one lane per region, the loop over the labels OUTSIDE the lane's work.  The answers of a region are kept as a bit mask, 32 labels a word, word-major
 * (mask[w * n + r]: a wave stores 64 consecutive words); the workgroup's number of hits goes to block_sums[block] for the scan.  The row of the tree table the
 * workgroup needs — (lo, hi) of every label's tree on the contig of the workgroup's first region — is staged in LDS 256 labels at a time; a lane on another contig
 * (the few workgroups that straddle a contig boundary) reads its bounds from memory. */
__global__ void __launch_bounds__(256) avk_strata_mask_kernel(avk::dp::DpIn in, avk::sx::SxTrees t, uint32_t n, uint32_t *mask, unsigned long long *block_sums) {
    __shared__ unsigned long long row[2 * 256];
    __shared__ uint32_t part[256];
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const avk::sx::SxSpan sp = avk::sx::sx_region_span(in, r < n ? r : in.n_regions, t.n_contigs);
    const uint32_t c0 = in.contig_of((uint64_t)blockIdx.x * 256u); /* (the workgroup's first region exists: the grid is sized from n) */
    const bool cached = sp.ok && sp.contig == c0;
    uint32_t count = 0;
    for (uint32_t lb = 0; lb < t.n_labels; lb += 256u) {
        const uint32_t mine = lb + threadIdx.x;
        unsigned long long lo = 0, hi = 0;
        if (mine < t.n_labels && c0 < t.n_contigs) {
            const uint64_t at = (uint64_t)mine * t.n_contigs + c0;
            lo = t.tree_off[at], hi = t.tree_off[at + 1];
        }
        row[2 * threadIdx.x] = lo, row[2 * threadIdx.x + 1] = hi;
        __syncthreads();
        const uint32_t chunk = t.n_labels - lb < 256u ? t.n_labels - lb : 256u;
        for (uint32_t j0 = 0; j0 < chunk; j0 += 32u) {
            const uint32_t word = avk::sx::sx_mask_word(t, sp, lb + j0, chunk - j0 < 32u ? chunk - j0 : 32u, [&](uint32_t l, uint64_t &a, uint64_t &b) {
                if (cached) a = row[2 * (l - lb)], b = row[2 * (l - lb) + 1];
                else {
                    const uint64_t at = (uint64_t)l * t.n_contigs + sp.contig;
                    a = t.tree_off[at], b = t.tree_off[at + 1];
                }
            });
            if (r < n) mask[avk::sx::sx_mask_at((lb + j0) >> 5, r, n)] = word;
            count += (uint32_t)__popc(word);
        }
        __syncthreads();
    }
    part[threadIdx.x] = count;
    __syncthreads();
    for (uint32_t st = 128; st > 0; st >>= 1) {
        if (threadIdx.x < st) part[threadIdx.x] += part[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) block_sums[blockIdx.x] = part[0];
}

/* Pass 2, behind the exclusive scan of block_sums (avk_ps_scan_sums_kernel): a region's offset is its workgroup's base plus the hits of the regions in front of
 * it in the workgroup; its list is the set bits of its mask words, ascending.  label_idx == NULL: the offsets only.  idx_cap bounds every store to label_idx. */
__global__ void __launch_bounds__(256) avk_strata_fill_kernel(const uint32_t *mask, uint32_t n, uint32_t n_words, const unsigned long long *block_base,
                                                              unsigned long long *label_off, uint32_t *label_idx, unsigned long long idx_cap) {
    __shared__ uint32_t part[256];
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    uint32_t mine = 0;
    if (r < n) mine = avk::sx::sx_fill_region(mask, r, n, n_words, nullptr, 0, 0);
    part[threadIdx.x] = mine;
    __syncthreads();
    for (uint32_t st = 1; st < 256u; st <<= 1) { /* Hillis-Steele inclusive scan */
        const uint32_t y = threadIdx.x >= st ? part[threadIdx.x - st] : 0u;
        __syncthreads();
        part[threadIdx.x] += y;
        __syncthreads();
    }
    if (r >= n) return;
    unsigned long long at = block_base[blockIdx.x] + (part[threadIdx.x] - mine);
    label_off[r] = at;
    if (r + 1 == n) label_off[n] = at + mine;
    if (label_idx) (void)avk::sx::sx_fill_region(mask, r, n, n_words, label_idx, at, idx_cap);
}
#endif

#endif /* AVK_STRATA_INL */
