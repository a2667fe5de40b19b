/*
 * avk_context.inl — the SEQUENCE-CONTEXT labels of a stratified job, made ON THE DEVICE from the resident reference: GC content and homopolymer runs.
 *
 * The rule is this project's own (the reference has no such labels; DESIGN.md §5 states it in full).  A region's query is sx_region_span's (avk_strata.inl),
 * unchanged; a family widens it by its `pad` to the context window [first - pad, last + 1 + pad), clamped to the contig.  A base COUNTS when its byte is an
 * upper-case A, C, G or T — what avk_pack_reference packs without a flag; every other byte is left out of every count and ends a run.
 *   GC family: n_gc_edges percent values, strictly ascending, make n_gc_edges - 1 labels.  With g the C/G bases and a the counted bases of the window, label i is
 *     set when a > 0 and edge[i] * a <= 100 * g < edge[i + 1] * a — integers only.
 *   Homopolymer family: n_hp_edges run lengths >= 1, strictly ascending, make n_hp_edges labels.  With L the longest run of one counted base inside the window
 *     (cut at its edges), label i is set when edge[i] <= L < edge[i + 1]; the last one when L >= edge[last].
 * A region gets at most one label per family.  The labels are bits 0.. of one word: the GC labels, then the homopolymer labels (at most 16 + 16).
 *
 * cx_scan is the lane's loop: over the window's packed words, 16 bases a word; a word whose flag is set in the exception bitmap is read from the byte copy.  The
 * binning runs once, behind the loop.  Nothing in the loop is cross-lane.  avk_context_mask_kernel (one lane per region, the geometry of avk_strata_mask_kernel)
 * puts the bits behind the BED labels' in the word-major masks that kernel writes.
 *
 * Written against avk_wave.h / DpIn like avk_strata.inl, so tests/emu/context_emu.cpp runs the same rule on the CPU against a numpy restatement.
 */
#ifndef AVK_CONTEXT_INL
#define AVK_CONTEXT_INL

#include "avk_strata.inl"

#define AVK_CX_PAD_MAX 1024u
#define AVK_CX_GC_EDGES_MAX 17u
#define AVK_CX_HP_EDGES_MAX 16u

namespace avk {
namespace cx {

typedef dp::u32 u32;
typedef dp::u64 u64;
typedef dp::u8 u8;

/* avk_context_spec (include/aardvark_amd.h), field for field */
struct CxSpec {
    u32 gc_pad, n_gc_edges, gc_edges[AVK_CX_GC_EDGES_MAX];
    u32 hp_pad, n_hp_edges, hp_edges[AVK_CX_HP_EDGES_MAX];
};
AVK_HD u32 cx_n_gc_labels(const CxSpec &s) { return s.n_gc_edges ? s.n_gc_edges - 1u : 0u; }
AVK_HD u32 cx_n_labels(const CxSpec &s) { return cx_n_gc_labels(s) + s.n_hp_edges; }

/* the resident reference (device pointers): the byte copy, the 2-bit copy, its flag bitmap (bit w & 31 of exc[w >> 5]: word w holds something that is not an
 * upper-case A/C/G/T), the contigs' bases and lengths in the concatenation */
struct CxRef {
    const u8 *bytes;
    const u32 *packed, *exc;
    const u64 *contig_base, *contig_len;
    u32 n_contigs;
};

/* what a window's bases say: counted bases, C/G among them, the longest run */
struct CxCounts {
    u64 a, g, run;
};

/* the code of a byte as avk_pack_reference packs it; 4: not counted */
AVK_DEV u32 cx_code_of_byte(u8 ch) { return ch == 'A' ? 0u : ch == 'C' ? 1u : ch == 'G' ? 2u : ch == 'T' ? 3u : 4u; }

/* One window [lo, hi) of the concatenated reference (lo < hi, inside one contig).  want_run == false: a and g only.  force_bytes: every word by the byte route
 * (the emulator's cross-check of the two routes). */
AVK_DEV CxCounts cx_scan(const CxRef &ref, u64 lo, u64 hi, bool want_run, bool force_bytes) {
    CxCounts c;
    c.a = c.g = c.run = 0;
    u32 prev = 4u;
    u64 cur = 0;
    for (u64 w = lo >> 4; w <= (hi - 1) >> 4; ++w) {
        const u32 j0 = w == lo >> 4 ? (u32)(lo & 15u) : 0u, j1 = w == (hi - 1) >> 4 ? (u32)((hi - 1) & 15u) + 1u : 16u; /* the window's bases of this word: [j0, j1) */
        const bool flagged = force_bytes || ((ref.exc[w >> 5] >> (u32)(w & 31u)) & 1u);
        if (!flagged) {
            const u32 x = ref.packed[w];
            /* C = 01, G = 10: the two bits of a code differ */
            const u32 keep = (j1 == 16u ? 0xFFFFFFFFu : (1u << (2u * j1)) - 1u) & ~((1u << (2u * j0)) - 1u);
            c.a += j1 - j0;
            c.g += (u64)avk_popc64((u64)((x ^ (x >> 1)) & 0x55555555u & keep));
            if (want_run)
                for (u32 j = j0; j < j1; ++j) {
                    const u32 code = (x >> (2u * j)) & 3u;
                    cur = code == prev ? cur + 1 : 1;
                    prev = code;
                    c.run = cur > c.run ? cur : c.run;
                }
        } else {
            const u8 *b = ref.bytes + (w << 4);
            for (u32 j = j0; j < j1; ++j) {
                const u32 code = cx_code_of_byte(b[j]);
                if (code > 3u) {
                    prev = 4u, cur = 0;
                    continue;
                }
                c.a += 1;
                c.g += (code == 1u || code == 2u) ? 1u : 0u;
                cur = code == prev ? cur + 1 : 1;
                prev = code;
                c.run = cur > c.run ? cur : c.run;
            }
        }
    }
    return c;
}

/* the context window of a span on the concatenated reference: false when it is empty (a span outside its contig) */
AVK_DEV bool cx_window(const CxRef &ref, const sx::SxSpan &sp, u32 pad, u64 &lo, u64 &hi) {
    const u64 len = ref.contig_len[sp.contig], base = ref.contig_base[sp.contig];
    u64 a = sp.first > pad ? sp.first - pad : 0, b = sp.last + 1 + pad; /* (last < 2^63 here: positions are sums of 32-bit fields or the caller's coordinates) */
    if (b < sp.last) b = ~0ull;
    if (b > len) b = len;
    if (a >= b) return false;
    lo = base + a, hi = base + b;
    return true;
}

/* the bins, once the window is read */
AVK_DEV u32 cx_gc_bits(const CxSpec &s, const CxCounts &c) {
    if (!c.a) return 0;
    for (u32 i = 0; i + 1 < s.n_gc_edges && i + 1 < AVK_CX_GC_EDGES_MAX; ++i)
        if ((u64)s.gc_edges[i] * c.a <= 100u * c.g && 100u * c.g < (u64)s.gc_edges[i + 1] * c.a) return 1u << i;
    return 0;
}
AVK_DEV u32 cx_hp_bits(const CxSpec &s, const CxCounts &c) {
    const u32 n = s.n_hp_edges < AVK_CX_HP_EDGES_MAX ? s.n_hp_edges : AVK_CX_HP_EDGES_MAX;
    for (u32 i = 0; i < n; ++i)
        if ((u64)s.hp_edges[i] <= c.run && (i + 1 == n || c.run < (u64)s.hp_edges[i + 1])) return 1u << i;
    return 0;
}

/* the labels of a span: GC labels from bit 0, homopolymer labels behind them */
AVK_DEV u32 cx_span_bits(const CxRef &ref, const CxSpec &s, const sx::SxSpan &sp, bool force_bytes) {
    if (!sp.ok || sp.contig >= ref.n_contigs) return 0;
    const bool gc = s.n_gc_edges > 1u, hp = s.n_hp_edges > 0u;
    u32 bits = 0;
    u64 lo, hi;
    if (gc && hp && s.gc_pad == s.hp_pad) { /* one window serves both families */
        if (!cx_window(ref, sp, s.gc_pad, lo, hi)) return 0;
        const CxCounts c = cx_scan(ref, lo, hi, true, force_bytes);
        return cx_gc_bits(s, c) | (cx_hp_bits(s, c) << cx_n_gc_labels(s));
    }
    if (gc && cx_window(ref, sp, s.gc_pad, lo, hi)) bits |= cx_gc_bits(s, cx_scan(ref, lo, hi, false, force_bytes));
    if (hp && cx_window(ref, sp, s.hp_pad, lo, hi)) bits |= cx_hp_bits(s, cx_scan(ref, lo, hi, true, force_bytes)) << cx_n_gc_labels(s);
    return bits;
}

/* THE RULE for region r */
AVK_DEV u32 cx_region_bits(const dp::DpIn &in, const CxRef &ref, const CxSpec &s, u64 r) {
    return cx_span_bits(ref, s, sx::sx_region_span(in, r, ref.n_contigs), false);
}

/* Where the bits go: context label j is overall label n_bed + j, so region r's words n_bed >> 5 .. (n_bed + n_ctx - 1) >> 5 of the word-major masks of n regions
 * (sx_mask_at) — at most two, n_ctx <= 32.  The first one also holds BED labels when n_bed & 31 != 0: the lane that owns the region ORs its bits into what the BED
 * labels' kernel stored there; every other word is stored whole.  fresh (n_bed == 0, that kernel did not run): nothing to OR into. */
AVK_DEV void cx_store_region(u32 *mask, u64 r, u64 n, u32 bits, u32 n_bed, u32 n_ctx, bool fresh) {
    const u32 w0 = n_bed >> 5, sh = n_bed & 31u;
    u32 *at = mask + sx::sx_mask_at(w0, r, n);
    *at = sh && !fresh ? (*at | (bits << sh)) : bits << sh;
    if (sh && sh + n_ctx > 32u) mask[sx::sx_mask_at(w0 + 1u, r, n)] = bits >> (32u - sh);
}

} // namespace cx
} // namespace avk

#ifndef AVK_EMU
/* One lane per region, queued on the same stream directly behind avk_strata_mask_kernel, whose geometry it shares: lane (block, thread) of both kernels owns region
 * block * 256 + thread and that region's mask words, so the word the context labels share with the BED labels is OR-ed in by a plain read-modify-write, and the
 * workgroup's number of context hits is ADDED to the block sum that kernel stored.  fresh (no BED labels: that kernel was not launched): the first word and the
 * block sum are stored instead.  The reduction is the only cross-lane step and sits behind the lanes' loops. */
__global__ void __launch_bounds__(256) avk_context_mask_kernel(avk::dp::DpIn in, avk::cx::CxRef ref, avk::cx::CxSpec spec, uint32_t n_bed, uint32_t n, uint32_t fresh,
                                                               uint32_t *mask, unsigned long long *block_sums) {
    __shared__ uint32_t part[256];
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    uint32_t bits = 0;
    if (r < n) {
        bits = avk::cx::cx_region_bits(in, ref, spec, r);
        avk::cx::cx_store_region(mask, r, n, bits, n_bed, avk::cx::cx_n_labels(spec), fresh != 0u);
    }
    part[threadIdx.x] = (uint32_t)__popc(bits);
    __syncthreads();
    for (uint32_t st = 128; st > 0; st >>= 1) {
        if (threadIdx.x < st) part[threadIdx.x] += part[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) block_sums[blockIdx.x] = (fresh ? 0ull : block_sums[blockIdx.x]) + part[0];
}
#endif

#endif /* AVK_CONTEXT_INL */
