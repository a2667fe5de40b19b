/*
 * avk_boot.inl — bootstrap replicates of the tallies, summed on the device (the rule: avk_boot.h).
 *
 * A replicate is "an integer weight per region": B replicates are B weighted re-sums of the per-region blocks lb_region_groups (avk_labels.inl) rebuilds from what
 * a run leaves in HBM anyway.  The label kernel's shape does not carry over: there few regions share a sum, here EVERY region of a scope lands on the same few
 * words (the joint group, the SNV group) in every replicate it enters, and LDS atomics on them would serialise.  So no sum is shared between lanes:
 *
 *   1. a workgroup stages a TILE of AVK_BT_TILE regions: one lane per region runs lb_region_groups once and writes the groups that occur, densely, to LDS — a slot
 *      of AVK_BT_SLOT words per group (its 22 fields, then a 1 in the joint group's slot: the region itself, for the AVK_TALLY_SOLVED word) — with the region's
 *      group mask (0: the region does not count — unsolved, or outside the launch's scope) and h(r);
 *   2. the lanes fill the tile's weight table w[region][replicate], ONE mix per (region, replicate) in the whole workgroup;
 *   3. lane (replicate b, field f) walks the tile: every lane of a wave reads the same region — its mask is wave-uniform, so the walk over its groups is a
 *      scalar branch per group — one byte of the table, one word of a slot per group, and adds w x value into 13 sums of its own, one per group, IN REGISTERS
 *      (the group loop is unrolled: every index is static, nothing is spilled);
 *   4. after its last tile the workgroup adds the lanes' sums to global memory, one 64-bit atomic per non-zero sum.
 *
 * A launch holds AVK_BT_REPS replicates of ONE scope (scope 0: every region; scope 1 + l: the regions whose bit l is set in the strata pass's masks, sx_mask_at's
 * layout — no list is made); more replicates or scopes are more launches.  A tile without a counting region is skipped after its masks are read.
 *
 * Written against avk_wave.h / DpIn / LbView like avk_labels.inl: the lane functions are one-lane code, and tests/emu/boot_emu.cpp runs the same source on the CPU.
 */
#ifndef AVK_BOOT_INL
#define AVK_BOOT_INL

#include "avk_boot.h"
#include "avk_labels.inl"
#include "avk_strata.inl"

#define AVK_BT_TILE 32                                        /* regions a workgroup stages at a time */
#define AVK_BT_SLOT 24                                        /* words of a group's slot: 22 fields, the region's 1 (joint group only), one word of padding */
#define AVK_BT_REPS 21                                        /* replicates of a launch: 21 x 24 = 504 of a workgroup's 512 lanes (512, not 1,024: 256 registers a lane — the
                                                                 staging lane's rebuild of a block and the 26 registers of sums do not fit 128 without scratch) */
#define AVK_BT_THREADS 512
#define AVK_BT_WG_PER_CU 1                                      /* workgroups resident on a CU: 131 registers a lane are 3 waves a SIMD, a workgroup takes 2 (forced to 128
                                                                 registers the kernel spills 12 B a lane: not taken) */
#define AVK_BT_TILE_SLOTS (AVK_BT_TILE * AVK_N_GROUPS)        /* a region has at most 13 groups */
#define AVK_BT_F_SOLVED AVK_N_FIELDS                          /* the slot word (and the lane) of the AVK_TALLY_SOLVED sum */

namespace avk {
namespace bt {

typedef dp::u8 u8;
typedef dp::u32 u32;
typedef dp::u64 u64;

/* one workgroup's tile (LDS on the device) */
struct BtTile {
    u32 *blk; /* [AVK_BT_TILE_SLOTS][AVK_BT_SLOT]: region rt's groups from slot rt * AVK_N_GROUPS on, in the order of its mask's set bits */
    u64 *h;   /* [AVK_BT_TILE] h(r) */
    u32 *gm;  /* [AVK_BT_TILE] bit g: group g occurs; 0: the region does not count */
    u8 *w;    /* [AVK_BT_TILE][AVK_BT_REPS] weights */
};

/* step 1, one lane: region r (tile slot rt) of a batch of n regions.  seed_mix = avk_boot_mix(seed).  Returns the mask it wrote. */
AVK_DEV u32 bt_stage_region(const lb::LbView &v, u64 r, u64 n, const u32 *mask, u32 scope, u64 seed_mix, u32 rt, const BtTile &t) {
    u32 gm = 0;
    bool counts = r < n && v.region_out[4 * r] == 0;
    if (counts && scope) {
        const u32 l = scope - 1u;
        counts = (mask[sx::sx_mask_at(l >> 5, r, n)] >> (l & 31u)) & 1u;
    }
    if (counts) {
        u32 *base = t.blk + (u64)rt * AVK_N_GROUPS * AVK_BT_SLOT;
        u32 j = 0;
        lb::lb_region_groups(v, r, [&](u32 g, const u32(&F)[AVK_N_FIELDS]) {
            u32 *d = base + j * AVK_BT_SLOT;
#pragma unroll
            for (int f = 0; f < AVK_N_FIELDS; ++f) d[f] = F[f];
            d[AVK_BT_F_SOLVED] = g == 0 ? 1u : 0u;
            d[AVK_BT_F_SOLVED + 1] = 0;
            gm |= 1u << g;
            ++j;
        });
        if (!(gm & 1u)) { /* (a solved region whose groups cannot be read has an empty block; it is a solved region all the same.  The joint group comes first, so
                             nothing was written) */
            for (int f = 0; f < AVK_BT_SLOT; ++f) base[f] = 0;
            base[AVK_BT_F_SOLVED] = 1u;
            gm = 1u;
        }
        t.h[rt] = avk_boot_mix(avk_boot_key(v.in.contig_of(r), (u32)v.in.start_of(r)) ^ seed_mix);
    }
    t.gm[rt] = gm;
    return gm;
}

/* step 2, entry e = rt * AVK_BT_REPS + bl of the weight table, for the launch's replicates [b_lo, b_hi) */
AVK_DEV void bt_weight_entry(const BtTile &t, u32 e, u32 b_lo, u32 b_hi) {
    const u32 rt = e / AVK_BT_REPS, b = b_lo + e % AVK_BT_REPS;
    t.w[e] = (u8)((t.gm[rt] && b < b_hi) ? avk_boot_weight_of_hash(t.h[rt], b) : 0u);
}

/* step 3, lane (bl, f), tile region rt with the mask gm (the caller's copy of t.gm[rt]: wave-uniform on the device): acc[g] += w x the region's word f of group g */
AVK_DEV void bt_lane_region(const BtTile &t, u32 rt, u32 gm, u32 bl, u32 f, u64 (&acc)[AVK_N_GROUPS]) {
    const u32 w = t.w[rt * AVK_BT_REPS + bl];
    const u32 *slot = t.blk + (u64)rt * AVK_N_GROUPS * AVK_BT_SLOT + f;
#pragma unroll
    for (int g = 0; g < AVK_N_GROUPS; ++g)
        if ((gm >> g) & 1u) {
            acc[g] += (u64)w * *slot;
            slot += AVK_BT_SLOT;
        }
}

/* step 4, lane (replicate b of B, field f): its sums into out[(scope * B + b) * AVK_TALLY_LEN + ..], added with add(p, x); zero sums are skipped */
template <class Add>
AVK_DEV void bt_lane_flush(const u64 (&acc)[AVK_N_GROUPS], u32 scope, u32 B, u32 b, u32 f, u64 *out, Add &&add) {
    u64 *dst = out + ((u64)scope * B + b) * AVK_TALLY_LEN;
    if (f < AVK_N_FIELDS) {
#pragma unroll
        for (int g = 0; g < AVK_N_GROUPS; ++g)
            if (acc[g]) add(dst + g * AVK_N_FIELDS + f, acc[g]);
    } else if (f == AVK_BT_F_SOLVED && acc[0])
        add(dst + AVK_TALLY_SOLVED, acc[0]);
}

} // namespace bt
} // namespace avk

#ifndef AVK_EMU
/* Replicates [b_lo, b_hi) (at most AVK_BT_REPS) of scope `scope` over the batch's regions: out[(scope * B + b) * AVK_TALLY_LEN + word] gains the sums.  LDS:
 * 39,936 + 256 + 128 + 672 bytes and the barrier's word, static (41,248 by the compiler's count: profiles/boot_resource_usage.txt). */
__global__ void __launch_bounds__(AVK_BT_THREADS) avk_boot_tally_kernel(avk::lb::LbView v, const uint32_t *mask, uint32_t n_regions, uint32_t scope, unsigned long long seed_mix,
                                                                        uint32_t B, uint32_t b_lo, uint32_t b_hi, unsigned long long *out) {
    __shared__ uint32_t s_blk[AVK_BT_TILE_SLOTS * AVK_BT_SLOT];
    __shared__ unsigned long long s_h[AVK_BT_TILE];
    __shared__ uint32_t s_gm[AVK_BT_TILE];
    __shared__ uint8_t s_w[AVK_BT_TILE * AVK_BT_REPS];
    avk::bt::BtTile t;
    t.blk = s_blk, t.h = (uint64_t *)s_h, t.gm = s_gm, t.w = s_w;
    const uint32_t tid = threadIdx.x, bl = tid / AVK_BT_SLOT, f = tid % AVK_BT_SLOT;
    uint64_t acc[AVK_N_GROUPS];
#pragma unroll
    for (int g = 0; g < AVK_N_GROUPS; ++g) acc[g] = 0;
    const uint32_t n_tiles = (n_regions + AVK_BT_TILE - 1) / AVK_BT_TILE;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        uint32_t mine = 0;
        if (tid < AVK_BT_TILE) mine = avk::bt::bt_stage_region(v, (uint64_t)tile * AVK_BT_TILE + tid, n_regions, mask, scope, seed_mix, tid, t);
        if (!__syncthreads_or((int)(mine != 0))) continue; /* no region of the tile counts (nothing of it is read again: the next tile may be staged at once) */
        for (uint32_t e = tid; e < AVK_BT_TILE * AVK_BT_REPS; e += AVK_BT_THREADS) avk::bt::bt_weight_entry(t, e, b_lo, b_hi);
        __syncthreads();
        if (bl < AVK_BT_REPS)
            for (uint32_t rt = 0; rt < AVK_BT_TILE; ++rt) {
                const uint32_t gm = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_gm[rt]);
                if (gm) avk::bt::bt_lane_region(t, rt, gm, bl, f, acc);
            }
        __syncthreads(); /* (the next tile's staging overwrites what the walk read) */
    }
    if (bl < AVK_BT_REPS && b_lo + bl < b_hi)
        avk::bt::bt_lane_flush(acc, scope, B, b_lo + bl, f, (uint64_t *)out, [](uint64_t *p, uint64_t x) { atomicAdd((unsigned long long *)p, (unsigned long long)x); });
}
#endif

#endif /* AVK_BOOT_INL */
