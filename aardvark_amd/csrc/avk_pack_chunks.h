/*
 * avk_pack_chunks.h — the chunk plan of a packed compare call whose region pass runs under its copies (context option pack_chunks; Upload::copy_packed_chunked
 * of avk_upload.inl queues it, avk_dp_region_chunk_kernel of avk_devpack_host.inl runs it).
 *
 * Plain C++, no HIP: the host cuts the batch, the region pass's workgroups evaluate the ownership rule, and tests/native/pack_chunks_check.cpp sweeps both on the CPU.
 *
 * The host knows n_regions and n_variants but not which calls a region owns — the packed form has no offsets, and a host pass over the counts is not wanted.  So the
 * two kinds of arrays are cut independently: the per-region arrays (start, len, contig_idx) into K ranges of whole 256-region blocks of the region pass, the per-call
 * arrays (var_rel_pos, var_type_zyg, var_raw_space) into K equal ranges of [0, n_variants).  Group j of the copies is region range j followed by call chunk j; the
 * device decides, from the running sum of the counts, which blocks a group completes (pc_launch_of_block).
 */
#ifndef AVK_PACK_CHUNKS_H
#define AVK_PACK_CHUNKS_H
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AVK_PC_HD __host__ __device__ inline
#else
#define AVK_PC_HD inline
#endif

namespace avk {
namespace pc {

enum { PC_MAX_GROUPS = 8, PC_BLOCK = 256 };

/* k = 0: the batch keeps the old order of its copies and the one region launch behind them */
struct ChunkPlan {
    uint32_t k;
    uint32_t block_cut[PC_MAX_GROUPS + 1]; /* region range j = blocks [block_cut[j], block_cut[j + 1]) */
    uint64_t call_cut[PC_MAX_GROUPS + 1];  /* call chunk j = calls [call_cut[j], call_cut[j + 1]) */
    uint64_t n_regions, n_variants;
};
struct Range {
    uint64_t first, count;
};

AVK_PC_HD uint32_t pc_blocks(uint64_t n_regions) { return (uint32_t)((n_regions + PC_BLOCK - 1) / PC_BLOCK); }
AVK_PC_HD Range pc_region_range(const ChunkPlan &p, uint32_t j) { /* in regions; the last block of the batch may be short */
    uint64_t lo = (uint64_t)p.block_cut[j] * PC_BLOCK, hi = (uint64_t)p.block_cut[j + 1] * PC_BLOCK;
    if (lo > p.n_regions) lo = p.n_regions;
    if (hi > p.n_regions) hi = p.n_regions;
    Range r = {lo, hi - lo};
    return r;
}
AVK_PC_HD Range pc_call_range(const ChunkPlan &p, uint32_t j) {
    Range r = {p.call_cut[j], p.call_cut[j + 1] - p.call_cut[j]};
    return r;
}

/* The plan for `want` groups.  floor_bytes: the least a group's copy of any one array may be (the narrowest per-region array has 2 bytes an entry — len, contig_idx —,
 * the narrowest per-call array 1 — var_type_zyg); a batch too small for that, an empty one, or want outside 2 .. PC_MAX_GROUPS gets k = 0. */
inline ChunkPlan plan_chunks(uint64_t n_regions, uint64_t n_variants, int64_t want, uint64_t floor_bytes) {
    ChunkPlan p;
    p.k = 0, p.n_regions = n_regions, p.n_variants = n_variants;
    for (int j = 0; j <= PC_MAX_GROUPS; ++j) p.block_cut[j] = 0, p.call_cut[j] = 0;
    if (want < 2 || want > PC_MAX_GROUPS || !n_regions || !n_variants || n_regions > 0x7FFFFFFFull || n_variants > 0x7FFFFFFFull) return p;
    const uint32_t k = (uint32_t)want, nb = pc_blocks(n_regions);
    for (uint32_t j = 0; j <= k; ++j) {
        p.block_cut[j] = (uint32_t)((uint64_t)nb * j / k);
        p.call_cut[j] = n_variants * j / k;
    }
    p.k = k;
    for (uint32_t j = 0; j < k; ++j)
        if (pc_region_range(p, j).count * 2u < floor_bytes || pc_call_range(p, j).count < floor_bytes) {
            p.k = 0;
            break;
        }
    return p;
}

/* Which launch runs block b, whose last region's calls end at call index `calls_end` (exclusive; 0 when no region up to the block's end has a call):
 *   o = the call chunk that holds the block's last call: the least o with calls_end <= call_cut[o + 1] (a block without calls so far: chunk 0);
 *   g = the region range that holds the block;
 *   the block runs in launch max(o, g): launch j is queued behind group j's copies, so by then region ranges 0 .. j and call chunks 0 .. j have arrived, and max(o, g)
 *   is the first launch for which both of the block's have.  A block whose region range arrives after its call chunk (g > o) is thereby taken by the first later
 *   group whose region range includes it: group g.
 * Returns k (no group: the catch-all launch behind the last group) when calls_end lies beyond n_variants — counts that do not add up to what the caller said;
 * the batch is refused once the state block is back, and no group launch reads a call that has not arrived. */
AVK_PC_HD uint32_t pc_launch_of_block(const ChunkPlan &p, uint32_t b, uint64_t calls_end) {
    uint32_t g = 0, o = 0;
    while (g + 1 < p.k && b >= p.block_cut[g + 1]) ++g;
    while (o < p.k && calls_end > p.call_cut[o + 1]) ++o;
    return o >= p.k ? p.k : (o > g ? o : g);
}

} // namespace pc
} // namespace avk
#endif
