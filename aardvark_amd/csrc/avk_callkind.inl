/*
 * avk_callkind.inl — per-call tallies keyed by the call's KIND (genotype x substitution class), summed on the device (the rule: avk_callkind.h; DESIGN.md
 * section 5).
 *
 * The size bins say how long a call is; the kind says what it is: heterozygous or homozygous-alternate by its input zygosity, transition or transversion by its
 * two allele bytes.  What a call adds is the size rule's contribution (lb_call: seven values to the truth or the query fields of the joint group and of its
 * type's group).  Everything is in HBM after any solve; the allele bytes are the one thing no tally stage has read before: a call whose alleles are both one
 * byte long reads them, gathered — one 2-byte read where allele 1 lies right behind allele 0 (always so in the packed and compact forms), two 1-byte reads
 * otherwise (the wide form names two offsets).  A call with a0_len != 1 or a1_len != 1 reads no allele byte; an offset outside the allele array reads none
 * either and is `other`.
 *
 * The accumulation is avk_sizebin.inl's, because the distribution is the same and more so: almost every call of a genome is het_ts or hom_ts in the joint and the
 * SNV group.  One lane per region (sz_lane_begin: the size kernel's lane record, reused as it is); the wave walks its regions' calls in step; per step and scope
 * the lanes are grouped by key (kind, type, side), counts are population counts of ballots, the four HAP / WEIGHTED_HAP sums run over the DPP network as 16-bit
 * halves (AVK_SZ_SUM), and fourteen lanes add a key's sums to LDS with one 64-bit LDS atomic each — one instruction per key, step and scope.  Nothing global is
 * touched inside the call loop; a workgroup adds its non-zero words to global memory once.
 *
 * KEY GROUPING: the first-pending-key loop, not one ballot per kind.  The key space that matters is kind x type x side — 9 x 13 x 2 — of which a step holds two
 * to four: a loop over the fixed space would pay nine ballots (v_cmp + s_and on the exec mask, then an s_cbranch each to skip the empty ones) per step and scope
 * before the type and the side are split at all, and the split needs the pending loop anyway.  In the ISA the loop's round is s_ff1_i32_b64, v_readlane_b32,
 * v_cmp_eq_u32 and four more v_cmp for the ballots: cheaper than the nine it would follow, and its trip count is the number of keys that occur.
 *
 * A launch holds the scopes [scope_lo, scope_hi); a scope's block is 9 x 13 x 14 x 8 = 13,104 B, so AVK_CK_LDS_BYTES (40 KB: four workgroups a CU) holds three.
 *
 * Written against avk_wave.h / DpIn / LbView like avk_sizebin.inl; ck_wave_tile is wave code (every lane of the wave calls it, control flow around the cross-lane
 * primitives is wave-uniform), and tests/emu/kind_emu.cpp runs the same source on the CPU.
 */
#ifndef AVK_CALLKIND_INL
#define AVK_CALLKIND_INL

#include "avk_callkind.h"
#include "avk_sizebin.inl"

#define AVK_CK_THREADS 256                                                  /* regions a workgroup takes at a time: one lane each, four waves */
#define AVK_CK_LDS_BYTES 40960                                              /* a workgroup's blocks: four workgroups a CU */
#define AVK_CK_BLOCK_WORDS (AVK_N_KINDS * AVK_N_GROUPS * AVK_SIZE_FIELDS)   /* one scope's 64-bit words */
#define AVK_CK_SCOPES (AVK_CK_LDS_BYTES / (AVK_CK_BLOCK_WORDS * 8))         /* scopes of a launch: 3 */

namespace avk {
namespace ck {

typedef dp::u8 u8;
typedef dp::u32 u32;
typedef dp::u64 u64;

/* one lane: sub of call c — the gathered read of its two allele bytes, when it has two */
AVK_DEV u32 ck_sub_of(const dp::DpIn &in, u64 c) {
    const u32 l0 = in.a0_len_of(c), l1 = in.a1_len_of(c);
    if (l0 != 1u || l1 != 1u) return (u32)AVK_KIND_SUB_OTHER;
    const u64 o0 = in.a0_off_of(c), o1 = in.a1_off_of(c);
    if (o0 >= in.alleles_len || o1 >= in.alleles_len) return (u32)AVK_KIND_SUB_OTHER;
    u32 b0, b1;
    if (o1 == o0 + 1u) { /* allele 1 right behind allele 0: one read serves both */
        uint16_t h;
        __builtin_memcpy(&h, in.alleles + o0, 2);
        b0 = h & 0xFFu, b1 = h >> 8;
    } else
        b0 = in.alleles[o0], b1 = in.alleles[o1];
    return avk_kind_sub_of(1u, 1u, b0, b1);
}

/* one lane: call i of its region — the key (kind | type << 4 | side << 8; a type beyond the table counts in the joint group only and is keyed as 15) and the seven values */
AVK_DEV lb::LbCall ck_lane_call(const lb::LbView &v, const sz::SzLane &L, u32 i, u32 &key) {
    const bool query = i >= L.tc;
    const u64 c = query ? L.qoff + (i - L.tc) : L.toff + i;
    const u32 vt = v.in.type_of(c);
    const u32 kind = avk_kind_of(avk_kind_gt_of(v.in.zyg_of(c)), ck_sub_of(v.in, c));
    key = kind | (vt < (u32)AVK_N_VARIANT_TYPES ? vt : 15u) << 4 | (query ? 1u : 0u) << 8;
    return lb::lb_call(L.vw[i], query, v.vinfo[c].alt_ed);
}

/* The WAVE's regions tile_first + lane: every lane of the wave calls this.  acc: the workgroup's blocks, scope scope_lo first, added to with add(p, x) (a 64-bit
 * LDS atomic on the device). */
template <class Add>
AVK_DEV void ck_wave_tile(const lb::LbView &v, u64 r, u64 n, const u32 *mask, u32 scope_lo, u32 scope_hi, u64 *acc, Add &&add) {
    const u32 lane = (u32)wv_lane();
    const u32 n_scopes = scope_hi - scope_lo;
    const sz::SzLane L = sz::sz_lane_begin(v, r, n, mask, scope_lo, scope_hi);
    const u32 steps = wv_max_u32(L.member ? L.n : 0u);
    for (u32 i = 0; i < steps; ++i) {
        const bool has = L.member && i < L.n;
        u32 key = 0;
        lb::LbCall c;
        c.gt_tp = c.gt_fn = c.gt_fn_gt = c.hap_tp = c.hap_fn = c.w_tp = c.w_fn = 0;
        if (has) c = ck_lane_call(v, L, i, key);
        for (u32 j = 0; j < n_scopes; ++j) {
            u64 pending = wv_ballot(has && ((L.member >> j) & 1u));
            while (pending) { /* (wave-uniform: one round per key that occurs) */
                const u32 key0 = wv_readlane(key, (u32)avk_ctz64(pending));
                const bool same = ((pending >> lane) & 1ull) && key == key0;
                const u64 m = wv_ballot(same);
                u64 sum[AVK_SIZE_VALUES];
                sum[0] = (u64)avk_popc64(wv_ballot(same && c.gt_tp));
                sum[1] = (u64)avk_popc64(wv_ballot(same && c.gt_fn));
                sum[2] = (u64)avk_popc64(wv_ballot(same && c.gt_fn_gt));
                const u32 hap_tp = same ? c.hap_tp : 0u, hap_fn = same ? c.hap_fn : 0u, w_tp = same ? c.w_tp : 0u, w_fn = same ? c.w_fn : 0u;
                sum[3] = (u64)wv_sum_u32(hap_tp); /* (a byte a lane) */
                sum[4] = AVK_SZ_SUM(hap_fn);
                sum[5] = AVK_SZ_SUM(w_tp);
                sum[6] = AVK_SZ_SUM(w_fn);
                /* lane k < 7: value k into the joint group; lane 7 + k: into the type's group */
                if (lane < 2u * AVK_SIZE_VALUES) {
                    const u32 k = lane < AVK_SIZE_VALUES ? lane : lane - AVK_SIZE_VALUES;
                    const u32 kind = key0 & 15u, vt = (key0 >> 4) & 15u, query = key0 >> 8;
                    u64 x = sum[0];
#pragma unroll
                    for (int q = 1; q < AVK_SIZE_VALUES; ++q) x = k == (u32)q ? sum[q] : x;
                    const u32 g = lane < AVK_SIZE_VALUES ? 0u : 1u + vt;
                    if (x && g < (u32)AVK_N_GROUPS) add(acc + (((u64)j * AVK_N_KINDS + kind) * AVK_N_GROUPS + g) * AVK_SIZE_FIELDS + avk_size_field_of(k, (int)query), x);
                }
                pending &= ~m;
            }
        }
    }
}

} // namespace ck
} // namespace avk

#ifndef AVK_EMU
/* Scopes [scope_lo, scope_hi) over the batch's regions: out[((scope * AVK_N_KINDS + kind) * AVK_N_GROUPS + g) * AVK_SIZE_FIELDS + f] gains the sums.  Dynamic LDS:
 * (scope_hi - scope_lo) * AVK_CK_BLOCK_WORDS * 8 bytes, at most AVK_CK_LDS_BYTES. */
__global__ void __launch_bounds__(AVK_CK_THREADS) avk_kind_tally_kernel(avk::lb::LbView v, const uint32_t *mask, uint32_t n_regions, uint32_t scope_lo, uint32_t scope_hi,
                                                                        unsigned long long *out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char avk_smem[];
    unsigned long long *acc = (unsigned long long *)avk_smem;
    const unsigned words = (scope_hi - scope_lo) * AVK_CK_BLOCK_WORDS;
    for (unsigned k = threadIdx.x; k < words; k += AVK_CK_THREADS) acc[k] = 0;
    __syncthreads();
    const uint32_t n_tiles = (n_regions + AVK_CK_THREADS - 1) / AVK_CK_THREADS;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) /* (uniform over the workgroup: every lane of a wave enters ck_wave_tile) */
        avk::ck::ck_wave_tile(v, (uint64_t)tile * AVK_CK_THREADS + threadIdx.x, n_regions, mask, scope_lo, scope_hi, (uint64_t *)acc,
                              [](uint64_t *p, uint64_t x) { atomicAdd((unsigned long long *)p, (unsigned long long)x); });
    __syncthreads();
    for (unsigned k = threadIdx.x; k < words; k += AVK_CK_THREADS) {
        const unsigned long long x = acc[k];
        if (x) atomicAdd(out + (size_t)scope_lo * AVK_CK_BLOCK_WORDS + k, x);
    }
}
#endif

#endif /* AVK_CALLKIND_INL */
