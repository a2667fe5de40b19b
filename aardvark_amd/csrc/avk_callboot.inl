/*
 * avk_callboot.inl — bootstrap replicates of the per-call blocks (size bins, call kinds), summed on the device (the rule: avk_callboot.h).
 *
 * Neither neighbour's shape carries over.  avk_boot_tally_kernel keeps 13 group sums per (replicate, field) lane in registers: a keyed block has n_keys x 13 of
 * them, indexed by a key known only at run time — they would spill.  avk_size_tally_kernel and avk_kind_tally_kernel reduce over a wave whose lanes are regions: a
 * replicate gives every region a weight of its own, so that shape would pay the whole stage once per replicate.  Here LANES ARE REPLICATES:
 *
 *   1. a workgroup stages a TILE of AVK_CB_TILE regions: one lane per region runs sz_lane_begin (the size kernel's lane record, with every refusal it makes) and
 *      leaves the record, the region's h(r) and its number of calls in LDS; lane 0 turns the counts into the tile's record ranges;
 *   2. the lanes fill the tile's weight table w[region][replicate]: ONE mix per (region, replicate) in the whole workgroup;
 *   3. the tile's calls are walked in PIECES of AVK_CB_RECS records, so that a region of any length passes (the escaped form carries sides of more than 255
 *      calls): one lane per record of the piece finds its region in the ranges, runs sz_lane_call or ck_lane_call — the allele-byte gather of ck_sub_of happens
 *      here, once per call, not once per replicate — and writes a record of eight words: the key (key | type << 4 | side << 8), then the seven values;
 *   4. lane (replicate bl, slot s) walks the piece region by region: slot s < 7 owns value s in the joint group, slot 7 + s the same value in the type's group.
 *      A record is the same for every lane of the workgroup, so its address arithmetic is scalar and its reads are LDS broadcasts; the weight is read once per
 *      (region, replicate), and a zero weight — 37 % of them — skips the region.  The lane adds w x value into acc[word][bl]: 64-bit words in LDS with the
 *      replicate index fastest, so that the lanes of a wave that share a slot hit different banks.  Every word has exactly one owning lane (a field names its
 *      value and side, the group names the slot's half), so a plain read-add-write is enough: NO atomic in the walk;
 *   5. after its last tile the workgroup adds its non-zero words to global memory with one 64-bit atomic each.
 *
 * The accumulators cost n_keys x 13 x 14 x 8 bytes a replicate (13.1 KB for the nine kinds, 7.3 KB for the five default bins, 23.3 KB for sixteen bins); the host
 * sizes a launch's replicates R from the LDS the runtime grants (cb_reps: up to gfx950's 160 KB a workgroup, one workgroup a CU) and the AVK_CB_THREADS / 14 lanes
 * teams a workgroup has.  A launch holds R replicates of ONE scope; more replicates or scopes are more launches, as in avk_boot_tally_kernel.  Why 256 lanes and not
 * more: with R <= 18 only 14 R lanes walk; the staging steps use all 256.  Why records of eight words and not packed ones: the walk's inner loop is then one
 * broadcast read of the key, one of the value, and the read-add-write.
 *
 * w x value is exact: w <= 12 and a value is a 32-bit word.  Control flow around every barrier is workgroup-uniform (the tile loop, the piece loop and the skip of a
 * tile without a call all depend on what every lane reads from LDS behind a barrier); no cross-lane primitive is used.
 *
 * Written against avk_wave.h / DpIn / LbView like avk_boot.inl: the lane functions are one-lane code, and tests/emu/callboot_emu.cpp runs the same source on the CPU.
 */
#ifndef AVK_CALLBOOT_INL
#define AVK_CALLBOOT_INL

#include "avk_callboot.h"
#include "avk_callkind.inl"

#define AVK_CB_THREADS 256                                  /* lanes of a workgroup */
#define AVK_CB_TILE 64                                      /* regions a workgroup stages at a time */
#define AVK_CB_RECS 256                                     /* call records of a piece: one lane each */
#define AVK_CB_REC_WORDS 8                                  /* the key, then the seven values */
#define AVK_CB_SLOTS (2 * AVK_SIZE_VALUES)                  /* lanes of a replicate: seven values x (the joint group, the type's group) */
#define AVK_CB_REPS_MAX (AVK_CB_THREADS / AVK_CB_SLOTS)     /* 18 */
#define AVK_CB_LDS_MAX (160 * 1024)                         /* gfx950: a workgroup may take the CU's whole LDS */
/* LDS of a launch of R replicates of n_keys keys: the accumulators, then the tile (h, lane records, call records, ranges, weights) */
#define AVK_CB_ACC_WORDS(n_keys, R) ((size_t)(n_keys) * AVK_CALLBOOT_KEY_WORDS * (R))
#define AVK_CB_TILE_BYTES(R) \
    ((size_t)AVK_CB_TILE * 8 + (size_t)AVK_CB_TILE * sizeof(avk::sz::SzLane) + (size_t)AVK_CB_RECS * AVK_CB_REC_WORDS * 4 + (size_t)(AVK_CB_TILE + 2) * 4 + (size_t)AVK_CB_TILE * (R))
#define AVK_CB_LDS_BYTES(n_keys, R) (AVK_CB_ACC_WORDS(n_keys, R) * 8 + AVK_CB_TILE_BYTES(R))

namespace avk {
namespace cb {

typedef dp::u8 u8;
typedef dp::u32 u32;
typedef dp::u64 u64;

/* one workgroup's accumulators and tile (LDS on the device) */
struct CbTile {
    u64 *acc;         /* [n_keys * AVK_CALLBOOT_KEY_WORDS][R] */
    u64 *h;           /* [AVK_CB_TILE] h(r) */
    sz::SzLane *lane; /* [AVK_CB_TILE] */
    u32 *rec;         /* [cap][AVK_CB_REC_WORDS] the piece's records */
    u32 *pre;         /* [AVK_CB_TILE + 1] region rt's records are pre[rt] .. pre[rt + 1] of the tile (before cb_ranges: pre[1 + rt] is the region's count) */
    u8 *w;            /* [AVK_CB_TILE][R] weights */
};

/* the replicates of a launch for n_keys keys when a workgroup gets lds_bytes of LDS (at least 1: two replicates of sixteen bins fit 64 KB) */
AVK_HD u32 cb_reps(u32 n_keys, u64 lds_bytes) {
    u32 R = AVK_CB_REPS_MAX;
    while (R > 1 && AVK_CB_LDS_BYTES(n_keys, R) > lds_bytes) --R;
    return R;
}

/* a tile's pointers into one buffer laid out as AVK_CB_LDS_BYTES counts it (cap <= AVK_CB_RECS records are used) */
AVK_HD CbTile cb_tile_at(unsigned char *base, u32 n_keys, u32 R) {
    CbTile t;
    t.acc = (u64 *)base;
    t.h = t.acc + AVK_CB_ACC_WORDS(n_keys, R);
    t.lane = (sz::SzLane *)(t.h + AVK_CB_TILE);
    t.rec = (u32 *)(t.lane + AVK_CB_TILE);
    t.pre = t.rec + (size_t)AVK_CB_RECS * AVK_CB_REC_WORDS;
    t.w = (u8 *)(t.pre + AVK_CB_TILE + 2);
    return t;
}

/* step 1, one lane: region r (tile slot rt) of a batch of n regions, for one scope.  seed_mix = avk_boot_mix(seed).  Returns the calls it will add (0: the region
 * does not count — beyond the batch, unsolved, calls out of range, outside the scope — or has no call) */
AVK_DEV u32 cb_stage_region(const lb::LbView &v, u64 r, u64 n, const u32 *mask, u32 scope, u64 seed_mix, u32 rt, const CbTile &t) {
    const sz::SzLane L = sz::sz_lane_begin(v, r, n, mask, scope, scope + 1u);
    const u32 cnt = L.member ? L.n : 0u;
    t.lane[rt] = L;
    t.h[rt] = cnt ? avk_boot_mix(avk_boot_key(v.in.contig_of(r), (u32)v.in.start_of(r)) ^ seed_mix) : 0ull;
    t.pre[1u + rt] = cnt;
    return cnt;
}

/* step 1, ONE lane of the workgroup: the counts into ranges; returns the tile's records */
AVK_DEV u32 cb_ranges(const CbTile &t) {
    u32 sum = 0;
    t.pre[0] = 0;
    for (u32 rt = 0; rt < AVK_CB_TILE; ++rt) {
        sum += t.pre[1u + rt];
        t.pre[1u + rt] = sum;
    }
    return sum;
}

/* step 2, entry e = rt * R + bl of the weight table, for the launch's replicates [b_lo, b_hi) */
AVK_DEV void cb_weight_entry(const CbTile &t, u32 e, u32 R, u32 b_lo, u32 b_hi) {
    const u32 rt = e / R, b = b_lo + e % R;
    t.w[e] = (u8)((t.pre[rt + 1u] > t.pre[rt] && b < b_hi) ? avk_boot_weight_of_hash(t.h[rt], b) : 0u);
}

/* step 3, one lane: record idx of the tile (idx < pre[AVK_CB_TILE]) into slot `slot` of the piece */
AVK_DEV void cb_stage_record(const lb::LbView &v, const CbTile &t, int family, const avk_size_spec &spec, u32 idx, u32 slot) {
    u32 lo = 0, hi = AVK_CB_TILE; /* the last rt with pre[rt] <= idx: its range is not empty, since pre[rt + 1] > idx */
    while (hi - lo > 1u) {
        const u32 mid = (lo + hi) >> 1;
        if (t.pre[mid] <= idx) lo = mid;
        else hi = mid;
    }
    const sz::SzLane L = t.lane[lo];
    u32 key = 0;
    const lb::LbCall c = family == AVK_CALLBOOT_KIND ? ck::ck_lane_call(v, L, idx - t.pre[lo], key) : sz::sz_lane_call(v, L, idx - t.pre[lo], spec, key);
    u32 *d = t.rec + (u64)slot * AVK_CB_REC_WORDS;
    d[0] = key, d[1] = c.gt_tp, d[2] = c.gt_fn, d[3] = c.gt_fn_gt, d[4] = c.hap_tp, d[5] = c.hap_fn, d[6] = c.w_tp, d[7] = c.w_fn;
}

/* step 4, lane (bl, s): the records [lo, hi) of the piece — one region's — with the region's weight w for the lane's replicate */
AVK_DEV void cb_lane_records(const CbTile &t, u32 lo, u32 hi, u32 w, u32 R, u32 bl, u32 s) {
    const u32 k = s < (u32)AVK_SIZE_VALUES ? s : s - (u32)AVK_SIZE_VALUES;
    const bool typed = s >= (u32)AVK_SIZE_VALUES;
    for (u32 slot = lo; slot < hi; ++slot) {
        const u32 *rec = t.rec + (u64)slot * AVK_CB_REC_WORDS;
        const u32 key = rec[0], x = rec[1u + k];
        const u32 g = typed ? 1u + ((key >> 4) & 15u) : 0u; /* (a type beyond the table is keyed as 15: the joint group only) */
        if (x && g < (u32)AVK_N_GROUPS) {
            u64 *p = t.acc + ((((u64)(key & 15u)) * AVK_N_GROUPS + g) * AVK_SIZE_FIELDS + avk_size_field_of(k, (int)(key >> 8))) * R + bl;
            *p += (u64)w * x;
        }
    }
}

/* step 4, lane (bl, s), piece [piece_lo, piece_lo + cap) of a tile: every region with records in the piece */
AVK_DEV void cb_lane_piece(const CbTile &t, u32 piece_lo, u32 cap, u32 R, u32 bl, u32 s) {
    const u32 piece_hi = piece_lo + cap;
    for (u32 rt = 0; rt < AVK_CB_TILE; ++rt) {
        const u32 a = t.pre[rt], b = t.pre[rt + 1u]; /* (the same for every lane: scalar on the device) */
        const u32 lo = a > piece_lo ? a : piece_lo, hi = b < piece_hi ? b : piece_hi;
        if (lo >= hi) continue;
        const u32 w = t.w[rt * R + bl];
        if (w) cb_lane_records(t, lo - piece_lo, hi - piece_lo, w, R, bl, s);
    }
}

/* step 5, accumulator word q = word * R + bl of a launch of the replicates [b_lo, b_hi) of B: into out[AVK_CALLBOOT_AT(scope, B, b_lo + bl, n_keys, 0, 0, 0) + word],
 * added with add(p, x); zero words are skipped */
template <class Add>
AVK_DEV void cb_flush_word(const CbTile &t, u64 q, u32 R, u32 n_keys, u32 scope, u32 B, u32 b_lo, u32 b_hi, u64 *out, Add &&add) {
    const u64 x = t.acc[q];
    const u32 b = b_lo + (u32)(q % R);
    if (x && b < b_hi) add(out + AVK_CALLBOOT_AT(scope, B, b, n_keys, 0, 0, 0) + q / R, x);
}

} // namespace cb
} // namespace avk

#ifndef AVK_EMU
/* Replicates [b_lo, b_hi) (at most R) of scope `scope` over the batch's regions, for a family (AVK_CALLBOOT_SIZE with its spec, or AVK_CALLBOOT_KIND) of n_keys keys:
 * out[AVK_CALLBOOT_AT(scope, B, b, n_keys, key, g, f)] gains the sums.  Dynamic LDS: AVK_CB_LDS_BYTES(n_keys, R). */
__global__ void __launch_bounds__(AVK_CB_THREADS) avk_callboot_tally_kernel(avk::lb::LbView v, const uint32_t *mask, uint32_t n_regions, int family, avk_size_spec spec,
                                                                            uint32_t n_keys, uint32_t scope, unsigned long long seed_mix, uint32_t B, uint32_t b_lo,
                                                                            uint32_t b_hi, uint32_t R, unsigned long long *out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char avk_smem[];
    const avk::cb::CbTile t = avk::cb::cb_tile_at(avk_smem, n_keys, R);
    const uint32_t tid = threadIdx.x, bl = tid % R, s = tid / R;
    const uint64_t acc_words = AVK_CB_ACC_WORDS(n_keys, R);
    for (uint64_t q = tid; q < acc_words; q += AVK_CB_THREADS) t.acc[q] = 0;
    const uint32_t n_tiles = (n_regions + AVK_CB_TILE - 1) / AVK_CB_TILE;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        uint32_t mine = 0;
        if (tid < AVK_CB_TILE) mine = avk::cb::cb_stage_region(v, (uint64_t)tile * AVK_CB_TILE + tid, n_regions, mask, scope, seed_mix, tid, t);
        if (!__syncthreads_or((int)(mine != 0))) continue; /* no call in the tile (nothing of it is read again: the next tile may be staged at once) */
        if (tid == 0) (void)avk::cb::cb_ranges(t);
        __syncthreads();
        const uint32_t total = t.pre[AVK_CB_TILE];
        for (uint32_t e = tid; e < AVK_CB_TILE * R; e += AVK_CB_THREADS) avk::cb::cb_weight_entry(t, e, R, b_lo, b_hi);
        for (uint32_t piece = 0; piece < total; piece += AVK_CB_RECS) { /* (uniform over the workgroup: total is) */
            if (piece + tid < total) avk::cb::cb_stage_record(v, t, family, spec, piece + tid, tid);
            __syncthreads(); /* (the first piece: the weight table as well) */
            if (s < AVK_CB_SLOTS) avk::cb::cb_lane_piece(t, piece, AVK_CB_RECS, R, bl, s);
            __syncthreads(); /* (the next piece's records, or the next tile's staging, overwrite what the walk read) */
        }
    }
    __syncthreads(); /* (the zeroing, for a workgroup that walked nothing) */
    for (uint64_t q = tid; q < acc_words; q += AVK_CB_THREADS)
        avk::cb::cb_flush_word(t, q, R, n_keys, scope, B, b_lo, b_hi, (uint64_t *)out, [](uint64_t *p, uint64_t x) { atomicAdd((unsigned long long *)p, (unsigned long long)x); });
}
#endif

#endif /* AVK_CALLBOOT_INL */
