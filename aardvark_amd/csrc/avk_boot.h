/*
 * avk_boot.h — the rule of the bootstrap replicates, ONE statement for the host (include/aardvark_amd.h: avk_boot_weight,
 * avk_boot_tallies_host) and the device (avk_boot.inl), the way avk_merge_reason.h is shared.  The reference has no such rule; this is the project's own.
 *
 *   unit     the region: what the solver treats as independent
 *   scheme   Poisson bootstrap: region r enters replicate b with an integer weight w(r, b) ~ Poisson(1); nothing is drawn per batch or per rank
 *   key      key(r) = (uint64) contig_idx(r) << 32 | start(r) — the window start as the packed form carries it: the same in any batch, shard or slice
 *   uniform  h(r) = mix(key(r) ^ mix(seed)) once per region; u(r, b) = mix(h(r) + b) >> 32, one mix per (region, replicate); mix = splitmix64's finaliser
 *            (avk_region_hash of include/aardvark_amd.h, restated here so that device code can call it)
 *   weight   w = #{ k in 0 .. 11 : u >= T[k] },  T[k] = floor(2^32 * sum_{j <= k} e^-1 / j!)  — 0 .. 12; the thirteenth threshold is 2^32 - 1
 *
 * Plain C: no includes beyond <stdint.h>, no state.
 */
#ifndef AVK_BOOT_H
#define AVK_BOOT_H

#include <stdint.h>

#if defined(__HIPCC__) && !defined(AVK_EMU)
#define AVK_BOOT_FN __host__ __device__ static inline
#else
#define AVK_BOOT_FN static inline
#endif

#define AVK_BOOT_MAX_REPLICATES 4096u /* 1 <= replicates <= this */
#define AVK_BOOT_MAX_BLOCKS 16384u    /* (1 + labels) * replicates <= this: 37.7 MB of sums */
#define AVK_BOOT_N_THRESHOLDS 12

/* floor(2^32 * P(Poisson(1) <= k)), k = 0 .. 11, computed with exact arithmetic (tests/test_boot_rule.py recomputes them with 50 digits) */
#define AVK_BOOT_T0 1580030168u
#define AVK_BOOT_T1 3160060337u
#define AVK_BOOT_T2 3950075421u
#define AVK_BOOT_T3 4213413783u
#define AVK_BOOT_T4 4279248373u
#define AVK_BOOT_T5 4292415291u
#define AVK_BOOT_T6 4294609777u
#define AVK_BOOT_T7 4294923276u
#define AVK_BOOT_T8 4294962463u
#define AVK_BOOT_T9 4294966817u
#define AVK_BOOT_T10 4294967252u
#define AVK_BOOT_T11 4294967292u

AVK_BOOT_FN uint64_t avk_boot_mix(uint64_t x) { /* splitmix64's finaliser */
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}
AVK_BOOT_FN uint64_t avk_boot_key(uint32_t contig_idx, uint32_t start) { return (uint64_t)contig_idx << 32 | start; }
/* h(r): once per region */
AVK_BOOT_FN uint64_t avk_boot_region_hash(uint64_t seed, uint64_t key) { return avk_boot_mix(key ^ avk_boot_mix(seed)); }
/* w from u: a sum of twelve comparisons, no table and no branch (the same code in a lane of the kernel) */
AVK_BOOT_FN uint32_t avk_boot_weight_of_uniform(uint32_t u) {
    return (uint32_t)(u >= AVK_BOOT_T0) + (u >= AVK_BOOT_T1) + (u >= AVK_BOOT_T2) + (u >= AVK_BOOT_T3) + (u >= AVK_BOOT_T4) + (u >= AVK_BOOT_T5) + (u >= AVK_BOOT_T6) +
           (u >= AVK_BOOT_T7) + (u >= AVK_BOOT_T8) + (u >= AVK_BOOT_T9) + (u >= AVK_BOOT_T10) + (u >= AVK_BOOT_T11);
}
/* w(r, b) from h(r): one mix */
AVK_BOOT_FN uint32_t avk_boot_weight_of_hash(uint64_t h, uint32_t b) { return avk_boot_weight_of_uniform((uint32_t)(avk_boot_mix(h + b) >> 32)); }
/* the rule in one call: w(r, b) of the region at (contig_idx, start) */
AVK_BOOT_FN uint32_t avk_boot_weight(uint64_t seed, uint32_t contig_idx, uint32_t start, uint32_t b) {
    return avk_boot_weight_of_hash(avk_boot_region_hash(seed, avk_boot_key(contig_idx, start)), b);
}

#endif /* AVK_BOOT_H */
