/*
 * avk_devpack_host.inl — the kernels around avk_devpack.inl and the host side of a device-packed batch.  Included by avk_host.hip.
 * Here: the kernels, the context's buffer pool, the copies in and out (copy_in, the copy kernel, the engines' rate check), the strata launches and the download.
 * The upload itself is avk_upload.inl (its forms and argument checks: avk_upload_forms.h), included right behind this file.
 *
 * The host's part of avk_batch_upload / avk_compare_batch is now: queue the copies of the caller's arrays (straight from the caller's memory
 * when it is pinned — avk_host_alloc —, through a pinned bounce buffer filled by the host threads when it is not), queue a dozen
 * kernels, read ONE small state block back (sizes of the variable-length outputs, batch-level errors), queue the writers.  Device
 * buffers come from a pool the context keeps, so a call allocates nothing after the first one of its size.
 */

/* ---------------------------------------------------------------------------------- kernels */
namespace dpk = avk::dp;

__global__ void __launch_bounds__(256) avk_dp_expand_pairs_kernel(dpk::DpPairs c) { dpk::dp_expand_pairs(c, (uint64_t)blockIdx.x * 256u + threadIdx.x); }
__global__ void __launch_bounds__(256) avk_dp_merge_classify_kernel(dpk::DpMerge c) { dpk::dp_merge_classify(c, (uint64_t)blockIdx.x * 256u + threadIdx.x); }

__global__ void __launch_bounds__(256) avk_dp_widen_kernel(dpk::DpCompact c) { dpk::dp_widen(c, (uint64_t)blockIdx.x * 256u + threadIdx.x); }
__global__ void __launch_bounds__(256) avk_dp_widen_packed_kernel(dpk::DpPacked c) { dpk::dp_widen_packed(c, (uint64_t)blockIdx.x * 256u + threadIdx.x); }
__global__ void __launch_bounds__(256) avk_dp_widen_packed_multi_kernel(dpk::DpPackedMulti c) { dpk::dp_widen_packed_multi(c, (uint64_t)blockIdx.x * 256u + threadIdx.x); }
__global__ void __launch_bounds__(256) avk_dp_widen_packed_esc_kernel(dpk::DpPacked c, dpk::DpEsc e) { dpk::dp_widen_packed_esc(c, e, (uint64_t)blockIdx.x * 256u + threadIdx.x); }
__global__ void __launch_bounds__(256) avk_dp_widen_packed_multi_esc_kernel(dpk::DpPackedMulti c, dpk::DpEsc e, uint64_t *w_in_off) {
    dpk::dp_widen_packed_multi_esc(c, e, w_in_off, (uint64_t)blockIdx.x * 256u + threadIdx.x);
}
/* One escape list of a packed batch (avk_packed_escapes), one workgroup: checks that idx[] is strictly ascending inside [lo, hi) and that the narrow fields `z` of
 * every listed entry are 0 (dp_esc_entry_bad: the check sits here, with the sparse lists, not in the widening's every lane) — *err is set otherwise —, writes
 * the exclusive sums of a[i] + b[i] to before[0 .. n] (b may be NULL; a NULL: a list without values to sum) and adds their total to *total: the sums over the narrow
 * arrays count a listed entry as 0, this is what they lack.  The lists are sparse (a genome's long alleles: thousands), so one workgroup's chunks of 1024 do. */
__global__ void __launch_bounds__(1024) avk_esc_scan_kernel(const uint64_t *idx, const uint32_t *a, const uint32_t *b, uint64_t n, uint64_t lo, uint64_t hi, dpk::DpEscNarrow z,
                                                            uint64_t *before, uint64_t *total, uint64_t *err) {
    __shared__ uint64_t part[1024];
    __shared__ uint64_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (uint64_t base = 0; base < n; base += 1024u) {
        const uint64_t i = base + threadIdx.x;
        if (i < n && dpk::dp_esc_entry_bad(idx, i, lo, hi, z)) *err = 1; /* (every writer stores the same word) */
        const uint64_t x = i < n && a ? (uint64_t)a[i] + (b ? (uint64_t)b[i] : 0ull) : 0ull;
        part[threadIdx.x] = x;
        __syncthreads();
        for (uint32_t st = 1; st < 1024u; st <<= 1) { /* Hillis-Steele inclusive scan */
            const uint64_t y = threadIdx.x >= st ? part[threadIdx.x - st] : 0ull;
            __syncthreads();
            part[threadIdx.x] += y;
            __syncthreads();
        }
        if (i < n && before) before[i] = carry + part[threadIdx.x] - x;
        __syncthreads();
        if (threadIdx.x == 1023u) carry += part[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (before) before[n] = carry;
        if (total) *total += carry;
    }
}
/* Exclusive prefix sum of a[i] + b[i] over n byte pairs (the packed form's offsets: calls per region, allele bytes per call): per-workgroup sums of 4096
 * elements, a one-workgroup scan of those sums, then every workgroup scans its own 4096 again from its base.  16 elements per thread, waves and workgroup
 * combined through LDS. */
#define AVK_PS_BLOCK 4096u
__device__ inline uint32_t avk_ps_thread_sum(const uint8_t *a, const uint8_t *b, uint64_t n, uint64_t i0, uint32_t (&v)[16]) {
    uint32_t s = 0;
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) {
        const uint64_t i = i0 + k;
        v[k] = i < n ? (uint32_t)a[i] + (b ? (uint32_t)b[i] : 0u) : 0u; /* b == NULL: the sum of one array */
        s += v[k];
    }
    return s;
}
__global__ void __launch_bounds__(256) avk_ps_block_sums_kernel(const uint8_t *a, const uint8_t *b, uint64_t n, uint64_t *block_sums) {
    __shared__ uint32_t part[256];
    uint32_t v[16];
    part[threadIdx.x] = avk_ps_thread_sum(a, b, n, (uint64_t)blockIdx.x * AVK_PS_BLOCK + threadIdx.x * 16u, v);
    __syncthreads();
    for (uint32_t st = 128; st > 0; st >>= 1) {
        if (threadIdx.x < st) part[threadIdx.x] += part[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) block_sums[blockIdx.x] = part[0];
}
__global__ void __launch_bounds__(1024) avk_ps_scan_sums_kernel(uint64_t *block_sums, uint32_t n_blocks, uint64_t *total) { /* one workgroup: in-place exclusive scan */
    __shared__ uint64_t part[1024];
    __shared__ uint64_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (uint32_t base = 0; base < n_blocks; base += 1024u) {
        const uint32_t i = base + threadIdx.x;
        const uint64_t x = i < n_blocks ? block_sums[i] : 0ull;
        part[threadIdx.x] = x;
        __syncthreads();
        for (uint32_t st = 1; st < 1024u; st <<= 1) { /* Hillis-Steele inclusive scan */
            const uint64_t y = threadIdx.x >= st ? part[threadIdx.x - st] : 0ull;
            __syncthreads();
            part[threadIdx.x] += y;
            __syncthreads();
        }
        if (i < n_blocks) block_sums[i] = carry + part[threadIdx.x] - x;
        __syncthreads();
        if (threadIdx.x == 1023u) carry += part[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0 && total) *total = carry;
}
__global__ void __launch_bounds__(256) avk_ps_apply_kernel(const uint8_t *a, const uint8_t *b, uint64_t n, const uint64_t *block_base, uint64_t *out) {
    __shared__ uint32_t part[256];
    uint32_t v[16];
    const uint64_t i0 = (uint64_t)blockIdx.x * AVK_PS_BLOCK + threadIdx.x * 16u;
    const uint32_t mine = avk_ps_thread_sum(a, b, n, i0, v);
    part[threadIdx.x] = mine;
    __syncthreads();
    for (uint32_t st = 1; st < 256u; st <<= 1) {
        const uint32_t y = threadIdx.x >= st ? part[threadIdx.x - st] : 0u;
        __syncthreads();
        part[threadIdx.x] += y;
        __syncthreads();
    }
    uint64_t run = block_base[blockIdx.x] + (part[threadIdx.x] - mine);
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) {
        if (i0 + k < n) out[i0 + k] = run;
        run += v[k];
    }
}

__global__ void __launch_bounds__(256) avk_dp_variant_kernel(dpk::DpArgs a) { dpk::dp_variant(a, (uint64_t)blockIdx.x * 256u + threadIdx.x); }

/* dp_region for 256 regions; the workgroup's sums of the three scanned quantities and its count of regions per lane class go to
 * column-major block_sums[quantity][block]: no global atomics (56,000 waves adding to the one counter of the modal class took 1.3 ms of this kernel's 1.6) */
#define AVK_DP_NS 4 /* scanned quantities: per-call output words, blob words, sequence bytes, compact BASEPAIR groups */
#define AVK_DP_BS (AVK_DP_NS + AVK_FAST_CLASSES + avk::dp::DP_NEED_BUCKETS)
/* (block: the workgroup's 256 regions; n_blocks: the batch's workgroups, the stride of a column — the launches of the chunked route cover a part of them each) */
__device__ inline void avk_dp_region_block(const dpk::DpArgs &a, uint64_t *block_sums, uint32_t block, uint32_t n_blocks) {
    __shared__ unsigned long long sums[AVK_DP_BS];
    if (threadIdx.x < AVK_DP_BS) sums[threadIdx.x] = 0;
    __syncthreads();
    uint32_t nc = 0, bw = 0, fc = 0, nb = 0xFFu, ng = 0;
    uint64_t sq = 0;
    dpk::dp_region(a, (uint64_t)block * 256u + threadIdx.x, nc, bw, sq, fc, nb, ng);
    if (__ballot(nb != 0xFFu)) /* class C regions: rare on a small-window genome */
        for (uint32_t c = 0; c < dpk::DP_NEED_BUCKETS; ++c) {
            const unsigned long long m = __ballot(nb == c);
            if (m && (threadIdx.x & 63u) == 0) atomicAdd(&sums[AVK_DP_NS + AVK_FAST_CLASSES + c], (unsigned long long)__popcll(m));
        }
    for (uint32_t c = 1; c <= AVK_FAST_CLASSES; ++c) { /* one LDS atomic per wave and class */
        const unsigned long long m = __ballot(fc == c);
        if (m && (threadIdx.x & 63u) == 0) atomicAdd(&sums[AVK_DP_NS - 1 + c], (unsigned long long)__popcll(m));
    }
    /* per-wave sums on the DPP network, 16 bits at a time so that 64 lanes cannot overflow a word; one LDS atomic per wave and quantity */
    const uint32_t nc_w = wv_sum_u32(nc); /* at most 64 x 60000 */
    const unsigned long long bw_w = (unsigned long long)wv_sum_u32(bw & 0xFFFFu) + ((unsigned long long)wv_sum_u32(bw >> 16) << 16);
    const unsigned long long sq_w = (unsigned long long)wv_sum_u32((uint32_t)sq & 0xFFFFu) + ((unsigned long long)wv_sum_u32((uint32_t)(sq >> 16) & 0xFFFFu) << 16) +
                                    ((unsigned long long)wv_sum_u32((uint32_t)(sq >> 32)) << 32);
    const uint32_t ng_w = wv_sum_u32(ng); /* at most 64 x 13 */
    if ((threadIdx.x & 63u) == 0) {
        if (ng_w) atomicAdd(&sums[3], (unsigned long long)ng_w);
        if (nc_w) atomicAdd(&sums[0], (unsigned long long)nc_w);
        if (bw_w) atomicAdd(&sums[1], bw_w);
        if (sq_w) atomicAdd(&sums[2], sq_w);
    }
    __syncthreads();
    if (threadIdx.x < AVK_DP_BS) block_sums[(size_t)threadIdx.x * n_blocks + block] = sums[threadIdx.x]; /* one column per quantity */
}
__global__ void __launch_bounds__(256) avk_dp_region_kernel(dpk::DpArgs a, uint64_t *block_sums) { avk_dp_region_block(a, block_sums, blockIdx.x, gridDim.x); }

/* The region pass of a packed batch whose copies are cut into groups (avk_pack_chunks.h): launch j runs behind the copies of group j and covers the blocks of the
 * region ranges 0 .. j.  A workgroup runs here iff pc_launch_of_block names this launch — the same answer for all its lanes, from the running sum of the counts at the
 * block's end (p_voff has no entry behind the last region: the last block adds that region's two counts).  launch == p.k is the catch-all behind the last group: the
 * blocks the rule gives to no group (their calls end beyond n_variants).  The rule is a function of the block alone, so every block has exactly one launch and no
 * state is kept between the launches. */
__global__ void __launch_bounds__(256) avk_dp_region_chunk_kernel(dpk::DpArgs a, uint64_t *block_sums, avk::pc::ChunkPlan p, uint32_t launch, uint32_t n_blocks) {
    const uint32_t b = blockIdx.x;
    if (b >= n_blocks) return;
    const uint64_t r_end = ((uint64_t)b + 1u) * 256u, n = a.in.n_regions;
    const uint64_t calls_end = r_end < n ? a.in.pk_voff[r_end] : a.in.pk_voff[n - 1] + a.in.pk_tc[n - 1] + a.in.pk_qc[n - 1];
    if (avk::pc::pc_launch_of_block(p, b, calls_end) != launch) return;
    avk_dp_region_block(a, block_sums, b, n_blocks);
}

/* one workgroup per column of the block sums: the scanned quantities get their exclusive scan in place and their total, the class and
 * workspace-bucket columns their sum (one workgroup walking all AVK_DP_BS columns of 14,000 rows took 0.2 ms of a 10 ms call) */
__global__ void __launch_bounds__(1024) avk_dp_scan_blocks_kernel(uint64_t *block_sums, uint32_t n_blocks, dpk::DpState *st) {
    __shared__ unsigned long long part[1024];
    const uint32_t q = blockIdx.x, t = threadIdx.x, per = (n_blocks + 1023u) / 1024u;
    uint64_t *col = block_sums + (size_t)q * n_blocks;
    const uint32_t lo = t * per < n_blocks ? t * per : n_blocks, hi = lo + per < n_blocks ? lo + per : n_blocks;
    unsigned long long s = 0;
    for (uint32_t b = lo; b < hi; ++b) s += col[b];
    part[t] = s;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {
        const unsigned long long x = t >= d ? part[t - d] : 0ull;
        __syncthreads();
        part[t] += x;
        __syncthreads();
    }
    if (q < AVK_DP_NS) {
        unsigned long long run = part[t] - s;
        for (uint32_t b = lo; b < hi; ++b) {
            const unsigned long long v = col[b];
            col[b] = run;
            run += v;
        }
    }
    if (t == 1023) {
        const unsigned long long total = part[1023];
        if (q == 0) st->total_v = total;
        else if (q == 1) st->total_blob_words = total;
        else if (q == 2) st->total_seq = total;
        else if (q == 3) st->total_groups = total;
        else if (q < AVK_DP_NS + AVK_FAST_CLASSES) st->have[q - AVK_DP_NS] = total;
        else st->need_hist[q - AVK_DP_NS - AVK_FAST_CLASSES] = total;
    }
}

/* per-region offsets: the block's base + the exclusive scan inside the block */
__global__ void __launch_bounds__(256) avk_dp_scan_apply_kernel(dpk::DpArgs a, const uint64_t *block_sums) {
    __shared__ unsigned long long sh[AVK_DP_NS][256];
    const uint32_t t = threadIdx.x;
    const uint64_t r = (uint64_t)blockIdx.x * 256u + t;
    unsigned long long v[AVK_DP_NS] = {0, 0, 0, 0};
    if (r < a.in.n_regions) {
        const uint32_t tc = a.in.t_cnt_of(r), qc = a.in.q_cnt_of(r);
        const uint64_t toff = a.in.t_off_of(r), qoff = a.in.q_off_of(r), nv = a.in.n_variants;
        if (!(toff > nv || (uint64_t)tc > nv - toff || qoff > nv || (uint64_t)qc > nv - qoff)) { /* as dp_region counted it */
            v[0] = (unsigned long long)tc + qc;
            v[1] = a.rinfo[r].blob_bytes / 4u;
            v[2] = 5ull * a.rinfo[r].seq_stride;
            const uint32_t ps = a.rinfo[r].pre_status;
            v[3] = (ps & 0xFFFFu) ? 0u : 1u + (unsigned)__popc(ps >> 16); /* as dp_region counted the compact BASEPAIR groups */
        }
    }
    for (int q = 0; q < AVK_DP_NS; ++q) sh[q][t] = v[q];
    __syncthreads();
    for (uint32_t d = 1; d < 256; d <<= 1) {
        unsigned long long x[AVK_DP_NS];
        for (int q = 0; q < AVK_DP_NS; ++q) x[q] = t >= d ? sh[q][t - d] : 0ull;
        __syncthreads();
        for (int q = 0; q < AVK_DP_NS; ++q) sh[q][t] += x[q];
        __syncthreads();
    }
    if (r < a.in.n_regions) {
        const uint64_t *bs = block_sums + blockIdx.x; /* column q of this workgroup: bs[q * gridDim.x] */
        const size_t col = gridDim.x;
        a.v_off[r] = (uint32_t)(bs[0] + sh[0][t] - v[0]);
        a.blob_off8[r] = (uint32_t)((bs[col] + sh[1][t] - v[1]) / 2ull);
        a.seq_off[r] = bs[2 * col] + sh[2][t] - v[2];
        a.bp_off[r] = (uint32_t)(bs[3 * col] + sh[3][t] - v[3]);
        if (r + 1 == a.in.n_regions) a.bp_off[r + 1] = (uint32_t)(bs[3 * col] + sh[3][t]);
    }
}

__global__ void avk_dp_lane_switch_kernel(dpk::DpArgs a) {
    if (blockIdx.x == 0 && threadIdx.x == 0) dpk::dp_lane_switch(a);
}

/* counting sort, pass 1: the histogram of the buckets (in LDS per workgroup, one global atomic per bucket the workgroup met) */
__global__ void __launch_bounds__(1024) avk_dp_hist_kernel(dpk::DpArgs a) {
    __shared__ uint32_t h[dpk::DP_NB];
    for (uint32_t k = threadIdx.x; k < dpk::DP_NB; k += 1024u) h[k] = 0;
    __syncthreads();
    const uint64_t r = (uint64_t)blockIdx.x * 1024u + threadIdx.x;
    if (r < a.in.n_regions) {
        const uint32_t b = dpk::dp_bucket_of(a, r);
        a.bucket16[r] = (uint16_t)b;
        atomicAdd(&h[b], 1u);
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < dpk::DP_NB; k += 1024u)
        if (h[k]) atomicAdd(&a.st->hist[k], h[k]);
}

/* dp_bucket_bases by one workgroup: thread t scans its 9 consecutive buckets, the 256 partial sums are scanned in LDS (one thread walking the 2,304
 * buckets in global memory took 50 us) */
__global__ void __launch_bounds__(256) avk_dp_bucket_bases_kernel(dpk::DpArgs a) {
    static_assert(dpk::DP_NB % 256 == 0, "buckets per thread");
    enum { PER = dpk::DP_NB / 256 };
    __shared__ uint32_t part[256];
    dpk::DpState &s = *a.st;
    const uint32_t t = threadIdx.x;
    uint32_t h[PER], sum = 0;
    for (int k = 0; k < PER; ++k) h[k] = s.hist[t * PER + k], sum += h[k];
    part[t] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 256; d <<= 1) {
        const uint32_t x = t >= d ? part[t - d] : 0u;
        __syncthreads();
        part[t] += x;
        __syncthreads();
    }
    uint32_t run = part[t] - sum;
    for (int k = 0; k < PER; ++k) {
        s.base[t * PER + k] = run;
        s.cursor[t * PER + k] = run;
        run += h[k];
    }
    if (t == 255) s.base[dpk::DP_NB] = run;
    __threadfence();
    __syncthreads();
    if (t == 0) dpk::dp_bucket_plan(a);
}

/* pass 2: a workgroup reserves its share of every bucket with one atomic and ranks its regions inside the share in LDS.  The order inside a
 * bucket is the caller's at the granularity of a workgroup (1024 regions) — a bucket holds regions of one cost, so nothing depends on it. */
__global__ void __launch_bounds__(1024) avk_dp_scatter_kernel(dpk::DpArgs a) {
    __shared__ uint32_t h[dpk::DP_NB];
    for (uint32_t k = threadIdx.x; k < dpk::DP_NB; k += 1024u) h[k] = 0;
    __syncthreads();
    const uint64_t r = (uint64_t)blockIdx.x * 1024u + threadIdx.x;
    uint32_t b = 0;
    if (r < a.in.n_regions) {
        b = a.bucket16[r];
        atomicAdd(&h[b], 1u);
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < dpk::DP_NB; k += 1024u)
        if (h[k]) h[k] = atomicAdd(&a.st->cursor[k], h[k]);
    __syncthreads();
    if (r < a.in.n_regions) a.order[dpk::dp_order_slot(a, b, atomicAdd(&h[b], 1u))] = (uint32_t)r;
}

__global__ void __launch_bounds__(256) avk_dp_fast_records_kernel(dpk::DpArgs a, uint32_t n_tiles_total) {
    const uint32_t tile = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (tile >= n_tiles_total) return;
    uint32_t fc = 0;
    for (uint32_t c = 0; c < AVK_FAST_CLASSES; ++c)
        if (tile >= a.st->tile_first[c] && tile < a.st->tile_first[c] + a.st->fast_tiles[c]) fc = c;
    dpk::dp_fast_record(a, fc, tile - a.st->tile_first[fc], lane);
}

/* region records + blobs of the work-order positions [0, n_items): the regions the wave-per-region launches read from the start (classes C, B, bulk) — or
 * every region, when a run has no lane launches */
__global__ void __launch_bounds__(256) avk_dp_region_records_kernel(dpk::DpArgs a, uint32_t n_items) {
    const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (k < n_items) dpk::dp_region_record(a, k);
}
__global__ void __launch_bounds__(256) avk_dp_region_records_wave_kernel(dpk::DpArgs a) {
    const uint32_t n_big = a.st->n_big, n_waves = gridDim.x * 4u;
    for (uint32_t item = blockIdx.x * 4u + (threadIdx.x >> 6); item < n_big; item += n_waves) dpk::dp_region_record_wave(a, item);
}

/* how many calls of the batch's range some region owns (DpIn::owned) */
__global__ void __launch_bounds__(256) avk_dp_count_owned_kernel(const uint8_t *owned, uint64_t n, dpk::DpState *st) {
    __shared__ uint32_t part;
    if (threadIdx.x == 0) part = 0;
    __syncthreads();
    uint32_t mine = 0;
    for (uint64_t i = ((uint64_t)blockIdx.x * 256u + threadIdx.x) * 16u, e = i + 16u < n ? i + 16u : n; i < e; ++i) mine += owned[i] ? 1u : 0u;
    if (mine) atomicAdd(&part, mine);
    __syncthreads();
    if (threadIdx.x == 0 && part) atomicAdd(&st->n_owned, part);
}

/* alt_ed of the calls dp_variant left to the host */
__global__ void avk_dp_patch_ed_kernel(dpk::DpVarInfo *vinfo, const uint32_t *idx, const uint32_t *ed, uint32_t n) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) {
        vinfo[idx[k]].alt_ed = ed[k];
        vinfo[idx[k]].flags &= ~(uint32_t)dpk::DP_VF_PENDING;
    }
}

/* A workgroup takes AVK_UNPACK_TILES tiles of 256 consecutive regions, lane t region t of every tile, and reserves the places of all their spilled groups with ONE
 * atomic.  Every workgroup of a genome has a region that spills, so with a tile per workgroup 13,935 returning atomics met on one word, took most of the kernel's
 * 187 us and kept it at that when the per-call outputs had left it (profiles/unpack_records_ab.txt); where the groups of a region lie in the list is the atomics'
 * order either way, the region's word names the place. */
enum { AVK_UNPACK_TILES = 8 };
__global__ void __launch_bounds__(256) avk_dp_unpack_kernel(dpk::DpOut o, uint8_t *pair_exact) {
    const uint64_t r0 = (uint64_t)blockIdx.x * (256u * AVK_UNPACK_TILES) + threadIdx.x;
    uint32_t word[AVK_UNPACK_TILES], need[AVK_UNPACK_TILES], mine = 0, at = 0;
#pragma unroll
    for (uint32_t k = 0; k < AVK_UNPACK_TILES; ++k) {
        need[k] = dpk::dp_unpack_bp_need(o, r0 + 256u * k, word[k]);
        mine += need[k];
    }
    if (o.bp_packed) { /* an exclusive scan of the lanes' needs: a lane's regions lie one behind the other from `at` */
        __shared__ uint32_t wave_sum[4], base;
        const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
        uint32_t incl = mine;
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t y = (uint32_t)__shfl_up((int)incl, d, 64);
            if (lane >= d) incl += y;
        }
        if (lane == 63) wave_sum[wv] = incl;
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t total = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
            base = total ? atomicAdd(o.bp_spill_count, total) : 0u;
        }
        __syncthreads();
        uint32_t before = 0;
        for (uint32_t k = 0; k < wv; ++k) before += wave_sum[k];
        at = base + before + incl - mine;
    }
#pragma unroll
    for (uint32_t k = 0; k < AVK_UNPACK_TILES; ++k) {
        const uint64_t r = r0 + 256u * k;
        dpk::dp_unpack(o, r, need[k], word[k], at);
        at += need[k];
        if (pair_exact && r < o.n_regions) pair_exact[r] = (o.region_out[4 * r] == 0 && o.region_out[4 * r + 1] != 0) ? 1 : 0; /* all_opt_haps[0].is_exact_match() */
    }
}

/* the per-call outputs of a dense batch read from its packed source: four consecutive calls per lane (dp_unpack_calls) */
__global__ void __launch_bounds__(256) avk_dp_unpack_calls_kernel(dpk::DpOut o, uint64_t n_calls) {
    dpk::dp_unpack_calls(o, n_calls, (uint64_t)blockIdx.x * 256u + threadIdx.x);
}

/* ---------------------------------------------------------------------------------- host threads */
namespace {

/* A small persistent pool for the loops that are left on the host (copies between pageable and pinned memory): workers sleep on a condition
 * variable between loops; one loop at a time (calls on different contexts take turns). */
class AvkPool {
  public:
    static AvkPool &get() {
        static AvkPool p;
        return p;
    }
    /* runs fn(t) for t in [0, nt) on the workers (t = 0 on the caller) and returns when all are done */
    void run(unsigned nt, const std::function<void(unsigned)> &fn) {
        if (nt <= 1) {
            fn(0);
            return;
        }
        std::lock_guard<std::mutex> one(loop_mutex_);
        ensure(nt - 1);
        {
            std::lock_guard<std::mutex> lk(m_);
            fn_ = &fn;
            want_ = nt - 1;
            next_ = 0;
            done_ = 0;
            gen_ += 1;
        }
        cv_.notify_all();
        fn(0);
        for (int spin = 0; spin < 4000 && done_.load(std::memory_order_acquire) != want_; ++spin) __builtin_ia32_pause();
        std::unique_lock<std::mutex> lk(m_);
        cv_done_.wait(lk, [&] { return done_ == want_; });
        fn_ = nullptr;
    }

  private:
    AvkPool() {}
    ~AvkPool() {
        {
            std::lock_guard<std::mutex> lk(m_);
            stop_ = true;
            gen_ += 1;
        }
        cv_.notify_all();
        for (auto &t : workers_) t.join();
    }
    void ensure(unsigned n) {
        while (workers_.size() < n) workers_.emplace_back([this] { work(); });
    }
    void work() {
        uint64_t seen = 0;
        for (;;) {
            const std::function<void(unsigned)> *fn = nullptr;
            unsigned t = 0;
            for (int spin = 0; spin < 20000 && gen_.load(std::memory_order_acquire) == seen; ++spin) __builtin_ia32_pause();
            {
                std::unique_lock<std::mutex> lk(m_);
                cv_.wait(lk, [&] { return stop_ || (gen_ != seen && next_ < want_); });
                if (stop_) return;
                t = ++next_; /* 1 .. want_ */
                seen = gen_; /* one index per loop and worker */
                fn = fn_;
            }
            (*fn)(t);
            {
                std::lock_guard<std::mutex> lk(m_);
                done_ += 1;
                if (done_ == want_) cv_done_.notify_all();
            }
        }
    }
    std::mutex m_, loop_mutex_;
    std::condition_variable cv_, cv_done_;
    std::vector<std::thread> workers_;
    const std::function<void(unsigned)> *fn_ = nullptr;
    unsigned want_ = 0, next_ = 0;
    std::atomic<unsigned> done_{0};
    std::atomic<uint64_t> gen_{0};
    bool stop_ = false;
};

template <class F> void avk_parallel_for(uint64_t n, unsigned nt, F f) { /* f(thread, lo, hi) */
    if (nt <= 1 || n < 4096) {
        f(0u, (uint64_t)0, n);
        return;
    }
    AvkPool::get().run(nt, [&](unsigned t) { f(t, n * t / nt, n * (t + 1) / nt); });
}

unsigned avk_host_threads() {
    unsigned nt = avk_usable_cpus();
    if (nt > 16) nt = 16;
    if (nt < 1) nt = 1;
    if (const char *e = getenv("AVK_HOST_THREADS")) {
        const int v = atoi(e);
        if (v >= 1 && v <= 256) nt = (unsigned)v;
    }
    return nt;
}

/* ---- pinned memory handed to the caller (avk_host_alloc): arrays that live there are copied by DMA without a host pass */
struct PinnedRange {
    const uint8_t *lo, *hi;
};
std::mutex g_pinned_mutex;
std::vector<PinnedRange> g_pinned;

bool is_pinned(const void *p, size_t bytes) {
    if (!p) return true;
    const uint8_t *lo = (const uint8_t *)p;
    {
        std::lock_guard<std::mutex> lk(g_pinned_mutex);
        for (const PinnedRange &r : g_pinned)
            if (lo >= r.lo && lo + bytes <= r.hi) return true;
    }
    if (bytes < (1u << 20)) return false; /* small arrays: the bounce buffer costs less than asking the runtime */
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return attr.type == hipMemoryTypeHost;
}

} // namespace

/* ---- the context's pool of device buffers: every buffer is used in the order of the context's stream (side streams are forked from and joined
 * into it), so a released buffer may be handed out again at once — whatever is still queued on it runs before the next user's work */
static int pool_alloc(avk_ctx *ctx, void **p, size_t bytes) {
    *p = nullptr;
    if (bytes == 0) bytes = 16;
    bytes = (bytes + 255) & ~(size_t)255;
    {
        std::lock_guard<std::mutex> lk(ctx->pool_mutex);
        int best = -1;
        for (size_t i = 0; i < ctx->pool.size(); ++i) {
            const auto &b = ctx->pool[i];
            if (b.used || b.bytes < bytes || b.bytes > 2 * bytes + (1u << 20)) continue;
            if (best < 0 || b.bytes < ctx->pool[(size_t)best].bytes) best = (int)i;
        }
        if (best >= 0) {
            ctx->pool[(size_t)best].used = true;
            ctx->pool_free_bytes -= ctx->pool[(size_t)best].bytes;
            *p = ctx->pool[(size_t)best].p;
            return 0;
        }
    }
    const bool timing = getenv("AVK_TIMING") != nullptr;
    const auto t_malloc = std::chrono::steady_clock::now();
    hipError_t e = hipMalloc(p, bytes);
    if (timing) fprintf(stderr, "avk pool: no cached buffer of %zu bytes, hipMalloc %.3f ms\n", bytes, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_malloc).count());
    if (e == hipErrorOutOfMemory) { /* give the cached buffers back and try again */
        (void)hipGetLastError();
        std::vector<void *> drop;
        {
            std::lock_guard<std::mutex> lk(ctx->pool_mutex);
            for (size_t i = 0; i < ctx->pool.size();) {
                if (!ctx->pool[i].used) {
                    drop.push_back(ctx->pool[i].p);
                    ctx->pool_free_bytes -= ctx->pool[i].bytes;
                    ctx->pool.erase(ctx->pool.begin() + (long)i);
                } else
                    ++i;
            }
        }
        for (void *q : drop) (void)hipFree(q);
        e = hipMalloc(p, bytes);
    }
    if (e != hipSuccess) {
        *p = nullptr;
        return fail(ctx, e == hipErrorOutOfMemory ? AVK_E_OOM : AVK_E_HIP, "device allocation of %zu bytes failed: %s", bytes, hipGetErrorString(e));
    }
    std::lock_guard<std::mutex> lk(ctx->pool_mutex);
    ctx->pool.push_back({*p, bytes, true});
    return 0;
}

static void pool_release(avk_ctx *ctx, void *p) {
    if (!p) return;
    bool drop = false;
    {
        std::lock_guard<std::mutex> lk(ctx->pool_mutex);
        for (size_t i = 0; i < ctx->pool.size(); ++i)
            if (ctx->pool[i].p == p) {
                if (ctx->pool_free_bytes + ctx->pool[i].bytes > (size_t)ctx->pool_cache_bytes) { /* beyond the cache limit: back to the runtime */
                    ctx->pool.erase(ctx->pool.begin() + (long)i);
                    drop = true;
                } else {
                    ctx->pool[i].used = false;
                    ctx->pool_free_bytes += ctx->pool[i].bytes;
                }
                break;
            }
    }
    if (drop) {
        const auto t_free = std::chrono::steady_clock::now();
        (void)hipFree(p);
        if (getenv("AVK_TIMING")) fprintf(stderr, "avk pool: cache limit reached, hipFree %.3f ms\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_free).count());
    }
}

/* avk_ctx_warmup: the buffers a device-packed batch of about n regions / nv calls takes from the pool, allocated, written once (fresh device memory is scrubbed
 * when it is first touched: 2.5 GB of them made the packing kernels of a process's first whole-genome call take 16 ms instead of 1.5) and put back.  A later
 * request takes a cached buffer that is at least as large and at most twice as large (pool_alloc): the sizes only have to be about right. */
static int pool_prewarm(avk_ctx *ctx, uint64_t n, uint64_t nv) {
    std::vector<size_t> sizes;
    auto add = [&](size_t bytes, int count) {
        for (int i = 0; i < count; ++i) sizes.push_back(bytes);
    };
    add((size_t)(n + 1) * 8, 5);   /* start, end, t_off, q_off, seq_off */
    add((size_t)(n + 1) * 4, 16);  /* counts, contig, per-region offsets, work order, the eight hand-over lists */
    add((size_t)(n + 1) * sizeof(dpk::DpRegionInfo), 1);
    add((size_t)(n + 1) * sizeof(AvkDevRegion), 1);
    add((size_t)n * 16 + 16, 2);   /* region records out, their caller-order form */
    add((size_t)n * 20 + 4, 1);
    add((size_t)(nv + 1) * 8, 3);  /* positions, allele offsets */
    add((size_t)(nv + 1) * 4, 5);  /* allele lengths, raw space, per-call words out and their caller-order form */
    add((size_t)nv + 16, 3);
    add((size_t)(nv + 1) * sizeof(dpk::DpVarInfo), 2); /* (and the call slots of the lane candidates) */
    add((size_t)n * 190, 1);       /* region blobs: 2.2 calls per region */
    add((size_t)n * 52, 1);        /* fast records */
    add((size_t)nv * 3 + 16, 1);   /* allele bytes */
    add((size_t)n * 10 + 16, 1);   /* the packed form's region and call records */
    add((size_t)nv * 5 + 16, 1);
    std::vector<void *> got;
    int rc = 0;
    for (size_t s : sizes) {
        void *p = nullptr;
        rc = pool_alloc(ctx, &p, s);
        if (rc) break;
        got.push_back(p);
        if (hipMemsetAsync(p, 0, s, ctx->stream) != hipSuccess) (void)hipGetLastError();
    }
    for (void *p : got) pool_release(ctx, p);
    return rc;
}

static void pool_destroy(avk_ctx *ctx) {
    for (auto &b : ctx->pool) (void)hipFree(b.p);
    ctx->pool.clear();
    ctx->pool_free_bytes = 0;
    if (ctx->h_bounce) (void)hipHostFree(ctx->h_bounce);
    ctx->h_bounce = nullptr;
    ctx->bounce_bytes = 0;
    if (ctx->h_dpstate) (void)hipHostFree(ctx->h_dpstate);
    ctx->h_dpstate = nullptr;
}

template <typename T> static int pool_alloc_t(avk_ctx *ctx, avk_dev_batch *db, T **p, size_t count) {
    void *q = nullptr;
    const int rc = pool_alloc(ctx, &q, count * sizeof(T));
    *p = (T *)q;
    if (!rc && db) db->pooled.push_back(q);
    return rc;
}

static int bounce_reserve(avk_ctx *ctx, size_t bytes) {
    if (bytes <= ctx->bounce_bytes) return 0;
    bytes += bytes / 8 + (1u << 20);
    if (ctx->h_bounce) {
        AVK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        (void)hipHostFree(ctx->h_bounce);
        ctx->h_bounce = nullptr;
        ctx->bounce_bytes = 0;
    }
    AVK_HIP(ctx, hipHostMalloc((void **)&ctx->h_bounce, bytes, hipHostMallocDefault));
    ctx->bounce_bytes = bytes;
    return 0;
}

/* ---- copies between the caller's arrays and the device ---------------------------------------------------------------------- */
struct CopySeg {
    const void *host; /* caller's array (source of an upload, destination of a download) */
    void *dev;
    size_t bytes;
    hipStream_t stream = nullptr;     /* uploads: a stream other than the context's for this array */
    hipEvent_t then_record = nullptr; /* uploads: recorded on that stream behind this array's copy */
    bool direct = false;              /* uploads: the caller has established that the array is pinned (copy_in does not look it up again) */
    std::function<void()> then_call;  /* uploads: called on the queueing thread right behind that record — work that waits for the event is queued HERE, in front of the
                                         copies that follow (upload_device_packed's chunked route says why) */
};

/* Copies between PINNED host arrays and HBM by a kernel instead of a DMA engine (round 6).  hipMemcpyAsync hands such a copy to an SDMA engine, and which engine a
 * process gets is the driver's round robin: of the processes started one after the other on one box, every second or third copied at HALF the rate the first one got —
 * 23.5 instead of 47 GB/s in, 2.4 instead of 1.2 ms out, a whole-genome call 9.5 ms instead of 6.5, for the life of the process (profiles/r06_copy_engines.txt).  In a
 * synchronous call nothing else runs while its arrays cross the bus, so the compute units do it: every lane moves 16 bytes at a time straight from / to the pinned
 * pages (they are mapped into the device's address space), at the link's rate in every process.  The asynchronous boundary keeps the engines: its copies run beside
 * kernels. */
__global__ void __launch_bounds__(256) avk_copy_kernel(const uint8_t *src, uint8_t *dst, size_t bytes) {
    const size_t tid = (size_t)blockIdx.x * 256u + threadIdx.x, nthreads = (size_t)gridDim.x * 256u;
    if ((((uintptr_t)src | (uintptr_t)dst) & 15u) == 0) {
        typedef unsigned int avk_v4u __attribute__((ext_vector_type(4)));
        const size_t n16 = bytes >> 4;
        const avk_v4u *s16 = (const avk_v4u *)src;
        avk_v4u *d16 = (avk_v4u *)dst;
        size_t i = tid;
        for (; i + 3 * nthreads < n16; i += 4 * nthreads) { /* four loads in flight per lane: the link's latency is microseconds */
            const avk_v4u a0 = __builtin_nontemporal_load(s16 + i), a1 = __builtin_nontemporal_load(s16 + i + nthreads), a2 = __builtin_nontemporal_load(s16 + i + 2 * nthreads),
                          a3 = __builtin_nontemporal_load(s16 + i + 3 * nthreads);
            __builtin_nontemporal_store(a0, d16 + i), __builtin_nontemporal_store(a1, d16 + i + nthreads), __builtin_nontemporal_store(a2, d16 + i + 2 * nthreads),
                __builtin_nontemporal_store(a3, d16 + i + 3 * nthreads);
        }
        for (; i < n16; i += nthreads) d16[i] = __builtin_nontemporal_load(s16 + i);
        for (size_t i = (n16 << 4) + tid; i < bytes; i += nthreads) dst[i] = src[i];
    } else if ((((uintptr_t)src | (uintptr_t)dst) & 3u) == 0) {
        const size_t n4 = bytes >> 2;
        const uint32_t *s4 = (const uint32_t *)src;
        uint32_t *d4 = (uint32_t *)dst;
        for (size_t i = tid; i < n4; i += nthreads) d4[i] = s4[i];
        for (size_t i = (n4 << 2) + tid; i < bytes; i += nthreads) dst[i] = src[i];
    } else
        for (size_t i = tid; i < bytes; i += nthreads) dst[i] = src[i];
}
/* Which of the two this context's synchronous copies use (option kernel_copies: 1 = decided by measurement, 0 = the engines, 2 = the kernel).  A probe copy of a
 * fresh buffer says nothing — it ran at 43-55 GB/s in processes whose calls then crawled — so the calls time THEMSELVES: two event records around the copies in of every
 * call that uses the engine (upload_device_packed); the first call whose arrays cross below 36 GB/s switches the context to the kernel for good.  A process that
 * drew a full-rate engine keeps it: it is 0.4 ms per whole-genome call faster than the kernel and leaves the CUs to dp_variant. */
static bool copies_by_kernel(const avk_ctx *ctx) { return ctx->kernel_copies == 2 || (ctx->kernel_copies == 1 && !ctx->engines_fast); }
static hipError_t kernel_copy(avk_ctx *ctx, void *dst, const void *src, size_t bytes, hipStream_t stream) {
    if (!bytes) return hipSuccess;
    size_t blocks = (bytes / 16 + 255) / 256;
    const size_t cap = (size_t)ctx->n_cus * (size_t)(ctx->copy_blocks_per_cu > 0 ? ctx->copy_blocks_per_cu : 8);
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(avk_copy_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, (const uint8_t *)src, (uint8_t *)dst, bytes);
    return hipGetLastError();
}

/* host -> device on the context's stream (or the segment's): straight from pinned arrays; pageable ones through the bounce buffer, piece by piece — the host threads
 * fill pieces while this thread queues the copy of every piece that is ready.  on_pack_stream: the upload of a submitted batch, whose copies run beside the kernels of
 * the batch before: always the engines, and not timed */
static int copy_in(avk_ctx *ctx, const std::vector<CopySeg> &segs, bool on_pack_stream) {
    struct Piece {
        const uint8_t *src;
        uint8_t *dev;
        size_t off, bytes;
        hipStream_t stream;
        hipEvent_t then_record; /* after this piece (the last of its segment) */
        bool direct;            /* pinned source: no staging */
        const std::function<void()> *then_call;
    };
    std::vector<Piece> pieces;
    size_t staged = 0;
    const size_t piece_bytes = 4u << 20;
    for (const CopySeg &s : segs) {
        hipStream_t stream = s.stream ? s.stream : ctx->stream;
        if (!s.bytes || !s.host) {
            if (s.then_record) pieces.push_back({nullptr, nullptr, 0, 0, stream, s.then_record, true, &s.then_call});
            continue;
        }
        if (s.direct || is_pinned(s.host, s.bytes)) {
            pieces.push_back({(const uint8_t *)s.host, (uint8_t *)s.dev, 0, s.bytes, stream, s.then_record, true, &s.then_call});
            continue;
        }
        for (size_t o = 0; o < s.bytes; o += piece_bytes) {
            const size_t nb = s.bytes - o < piece_bytes ? s.bytes - o : piece_bytes;
            pieces.push_back({(const uint8_t *)s.host + o, (uint8_t *)s.dev + o, staged, nb, stream, o + nb == s.bytes ? s.then_record : (hipEvent_t) nullptr, false,
                              o + nb == s.bytes ? &s.then_call : nullptr});
            staged += (nb + 63) & ~(size_t)63;
        }
    }
    if (pieces.empty()) return 0;
    if (staged) {
        const int rc = bounce_reserve(ctx, staged);
        if (rc) return rc;
    }
    const bool timing = getenv("AVK_TIMING") != nullptr;
    size_t direct_bytes = 0;
    for (const Piece &p : pieces) direct_bytes += p.direct ? p.bytes : 0;
    const bool by_kernel = !on_pack_stream && direct_bytes >= (8u << 20) && copies_by_kernel(ctx); /* (small batches: the engines' latency is what counts) */
    const bool timed_engine = !on_pack_stream && !by_kernel && ctx->kernel_copies == 1 && direct_bytes >= (8u << 20) && staged == 0 && ctx->ev_cp0 && ctx->ev_cp1;
    if (timed_engine) (void)hipEventRecord(ctx->ev_cp0, ctx->stream);
    ctx->cp_timed_bytes = 0;
    bool cp1_recorded = false;
    auto issue = [&](const Piece &p) -> hipError_t { /* pieces are queued in segment order, whatever their source */
        const auto t0 = std::chrono::steady_clock::now();
        hipError_t e = hipSuccess;
        if (p.bytes && p.direct && by_kernel) e = kernel_copy(ctx, p.dev, p.src, p.bytes, p.stream); /* (a queued upload's copies run beside kernels: the engines) */
        else if (p.bytes) e = hipMemcpyAsync(p.dev, p.direct ? p.src : ctx->h_bounce + p.off, p.bytes, hipMemcpyHostToDevice, p.stream);
        const auto t1 = std::chrono::steady_clock::now();
        if (e == hipSuccess && p.then_record) e = hipEventRecord(p.then_record, p.stream);
        /* the engine's rate is that of the copies alone: behind the last piece the closing event goes in FRONT of whatever the piece's hook queues (kernels that wait for
         * this very copy would stand between the copy and the event where the streams share a hardware queue; what earlier hooks queued is over long before) */
        if (e == hipSuccess && timed_engine && &p == &pieces.back()) cp1_recorded = hipEventRecord(ctx->ev_cp1, ctx->stream) == hipSuccess;
        if (e == hipSuccess && p.then_record && p.then_call && *p.then_call) (*p.then_call)();
        if (timing) {
            const double a = std::chrono::duration<double, std::milli>(t1 - t0).count(), b = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
            if (a > 0.5 || b > 0.5)
                fprintf(stderr, "avk copy_in: queueing a copy of %zu bytes on the %s stream took %.3f ms, the event record behind it %.3f ms\n", p.bytes,
                        p.stream == ctx->stream ? "context's" : "side", a, b);
        }
        return e;
    };
    hipError_t herr = hipSuccess;
    const unsigned nt = avk_host_threads();
    if (!staged || nt <= 1) {
        for (size_t k = 0; k < pieces.size() && herr == hipSuccess; ++k) {
            if (!pieces[k].direct) memcpy(ctx->h_bounce + pieces[k].off, pieces[k].src, pieces[k].bytes);
            herr = issue(pieces[k]);
        }
    } else {
        std::atomic<size_t> next(0);
        std::vector<std::atomic<uint8_t>> ready(pieces.size());
        for (size_t k = 0; k < pieces.size(); ++k) ready[k].store(pieces[k].direct ? 1 : 0);
        AvkPool::get().run(nt + 1, [&](unsigned t) {
            if (t == 0) { /* this thread queues, the others fill */
                for (size_t k = 0; k < pieces.size() && herr == hipSuccess; ++k) {
                    while (!ready[k].load(std::memory_order_acquire)) std::this_thread::yield();
                    herr = issue(pieces[k]);
                }
                return;
            }
            for (;;) {
                const size_t k = next.fetch_add(1);
                if (k >= pieces.size()) break;
                if (pieces[k].direct) continue;
                memcpy(ctx->h_bounce + pieces[k].off, pieces[k].src, pieces[k].bytes);
                ready[k].store(1, std::memory_order_release);
            }
        });
    }
    if (herr != hipSuccess) return fail(ctx, AVK_E_HIP, "host to device copy failed: %s", hipGetErrorString(herr));
    if (timed_engine && cp1_recorded) ctx->cp_timed_bytes = direct_bytes; /* (read by engine_rate_check once the stream has been waited for) */
    return 0;
}
/* behind a host synchronisation with the context's stream: how fast the engine moved the arrays of the copy_in before it */
static void engine_rate_check(avk_ctx *ctx) {
    if (!ctx->cp_timed_bytes) return;
    float ms = 0;
    if (hipEventElapsedTime(&ms, ctx->ev_cp0, ctx->ev_cp1) == hipSuccess && ms > 0) {
        ctx->engine_in_gbs = ctx->cp_timed_bytes / (ms * 1e-3) / 1e9;
        if (ms > ctx->cp_timed_bytes / 36e9 * 1e3 + 0.15) { /* below 36 GB/s, with 0.15 ms for the dozen copies' own latencies (a rank's shard is 10 MB) */
            /* two timed calls in a row: a half-rate engine is slow in every call, one slow measurement (another process on the link, the region pass beside the
             * copies) is not a reason to give the engine up for the life of the context */
            if (++ctx->engine_slow_calls >= 2) ctx->engines_fast = false;
            if (getenv("AVK_TIMING"))
                fprintf(stderr, "avk copies: the DMA engine moved this call's arrays at %.1f GB/s: %s\n", ctx->engine_in_gbs,
                        ctx->engines_fast ? "one slow call, the next one decides" : "synchronous calls copy by kernel from now on");
        } else {
            ctx->engine_slow_calls = 0;
            if (getenv("AVK_TIMING")) fprintf(stderr, "avk copies: the DMA engine moved this call's arrays at %.1f GB/s\n", ctx->engine_in_gbs);
        }
    } else
        (void)hipGetLastError();
    ctx->cp_timed_bytes = 0;
}

/* device -> host: queues the copies (pinned destinations directly, the others into the bounce buffer); finish_copy_out waits for the stream and
 * moves the bounced parts into the caller's arrays on the host threads */
struct CopyOut {
    struct Part {
        void *host;
        size_t off, bytes;
    };
    std::vector<Part> parts;
};
static int copy_out(avk_ctx *ctx, const std::vector<CopySeg> &segs, CopyOut *co) {
    size_t staged = 0;
    for (const CopySeg &s : segs)
        if (s.bytes && s.host && !is_pinned(s.host, s.bytes)) staged += (s.bytes + 63) & ~(size_t)63;
    if (staged) {
        const int rc = bounce_reserve(ctx, staged);
        if (rc) return rc;
    }
    size_t off = 0, pinned_bytes = 0;
    for (const CopySeg &s : segs) pinned_bytes += s.bytes && s.host && is_pinned(s.host, s.bytes) ? s.bytes : 0;
    const bool by_kernel = pinned_bytes >= (8u << 20) && copies_by_kernel(ctx);
    for (const CopySeg &s : segs) {
        if (!s.bytes || !s.host) continue;
        if (is_pinned(s.host, s.bytes)) {
            if (by_kernel) AVK_HIP(ctx, kernel_copy(ctx, (void *)s.host, s.dev, s.bytes, ctx->stream));
            else AVK_HIP(ctx, hipMemcpyAsync((void *)s.host, s.dev, s.bytes, hipMemcpyDeviceToHost, ctx->stream));
            continue;
        }
        AVK_HIP(ctx, hipMemcpyAsync(ctx->h_bounce + off, s.dev, s.bytes, hipMemcpyDeviceToHost, ctx->stream));
        co->parts.push_back({(void *)s.host, off, s.bytes});
        off += (s.bytes + 63) & ~(size_t)63;
    }
    return 0;
}
static int finish_copy_out(avk_ctx *ctx, const CopyOut &co) {
    AVK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (co.parts.empty()) return 0;
    struct Piece {
        uint8_t *dst;
        const uint8_t *src;
        size_t bytes;
    };
    std::vector<Piece> pieces;
    const size_t piece_bytes = 4u << 20;
    for (const auto &p : co.parts)
        for (size_t o = 0; o < p.bytes; o += piece_bytes) pieces.push_back({(uint8_t *)p.host + o, ctx->h_bounce + p.off + o, p.bytes - o < piece_bytes ? p.bytes - o : piece_bytes});
    std::atomic<size_t> next(0);
    const unsigned nt = pieces.size() > 1 ? avk_host_threads() : 1;
    AvkPool::get().run(nt, [&](unsigned) {
        for (;;) {
            const size_t k = next.fetch_add(1);
            if (k >= pieces.size()) break;
            memcpy(pieces[k].dst, pieces[k].src, pieces[k].bytes);
        }
    });
    return 0;
}

/* ---- upload ---------------------------------------------------------------------------------------------------------------- */
static void release_pooled(avk_ctx *ctx, avk_dev_batch *db) {
    for (void *p : db->pooled) pool_release(ctx, p);
    db->pooled.clear();
}

/* the arrays of an avk_packed_batch already in device memory (a staging slot of avk_compare_packed_submit, filled on the context's copy stream): nothing is copied,
 * the context's stream waits for `ready`; the block stays with the caller (the allele bytes and raw spaces are read until the batch's solve is over) */
/* ---- the containment lists of a stratified batch, made on the device (avk_strata.inl) ------------------------------------------------------------------ */
static avk::sx::SxTrees strata_trees(const avk_strata *st) {
    avk::sx::SxTrees t;
    t.tree_off = st->d_tree_off, t.start = st->d_start, t.end_max = st->d_end_max, t.n_labels = st->n_bed_labels, t.n_contigs = st->n_contigs;
    return t;
}
static inline uint32_t strata_words(const avk_strata *st) { return (st->n_labels + 31u) / 32u; }
static inline uint32_t strata_blocks(uint64_t n) { return (uint32_t)((n + 255) / 256); }
/* The mask pass of a handle: the BED labels' kernel (a handle with such labels), then — ONLY for a handle with context labels — avk_context_mask_kernel directly
 * behind it on the same stream, same grid.  The reference is the context's as it is now (the entry points have checked that it is there and has the handle's
 * number of contigs: strata_handle_check). */
static void strata_mask_kernels(const avk_strata *st, const dpk::DpIn &in, uint64_t n, uint32_t *d_mask, uint64_t *d_sums, hipStream_t s) {
    const uint32_t nb = strata_blocks(n);
    if (st->n_bed_labels || !st->n_ctx_labels) /* (the second term: a handle without context labels launches what it always launched, with whatever labels it has) */
        hipLaunchKernelGGL(avk_strata_mask_kernel, dim3(nb), dim3(256), 0, s, in, strata_trees(st), (uint32_t)n, d_mask, (unsigned long long *)d_sums);
    if (st->n_ctx_labels) {
        const avk_ctx *ctx = st->ctx;
        avk::cx::CxRef ref;
        ref.bytes = ctx->d_ref, ref.packed = ctx->d_ref2b, ref.exc = ctx->d_refexc, ref.contig_base = ctx->d_contig_tab, ref.contig_len = ctx->d_contig_tab + ctx->contig_len.size(),
        ref.n_contigs = (uint32_t)ctx->contig_len.size();
        hipLaunchKernelGGL(avk_context_mask_kernel, dim3(nb), dim3(256), 0, s, in, ref, st->spec, st->n_bed_labels, (uint32_t)n, st->n_bed_labels ? 0u : 1u, d_mask,
                           (unsigned long long *)d_sums);
    }
}
/* pass 1 and the scan of its workgroup sums: d_mask[strata_words * n], d_sums[strata_blocks(n) + 1] — the workgroups' bases, then the number of list entries */
static hipError_t strata_count_launch(const avk_strata *st, const dpk::DpIn &in, uint64_t n, uint32_t *d_mask, uint64_t *d_sums, hipStream_t s) {
    if (!n) return hipSuccess;
    const uint32_t nb = strata_blocks(n);
    strata_mask_kernels(st, in, n, d_mask, d_sums, s);
    hipLaunchKernelGGL(avk_ps_scan_sums_kernel, dim3(1), dim3(1024), 0, s, d_sums, nb, d_sums + nb);
    return hipGetLastError();
}
/* pass 1 alone, for a batch whose tally reads the masks themselves (avk_compare_packed_submit_strata): no scan, no list; d_sums[strata_blocks(n)] only takes the
 * workgroups' counts the kernel writes */
static hipError_t strata_mask_launch(const avk_strata *st, const dpk::DpIn &in, uint64_t n, uint32_t *d_mask, uint64_t *d_sums, hipStream_t s) {
    if (!n) return hipSuccess;
    strata_mask_kernels(st, in, n, d_mask, d_sums, s);
    return hipGetLastError();
}
/* pass 2: the offsets, and with d_idx the indices (idx_cap entries of room) */
static hipError_t strata_fill_launch(const avk_strata *st, uint64_t n, const uint32_t *d_mask, const uint64_t *d_sums, uint64_t *d_off, uint32_t *d_idx, uint64_t idx_cap, hipStream_t s) {
    if (!n) return hipMemsetAsync(d_off, 0, 8, s);
    hipLaunchKernelGGL(avk_strata_fill_kernel, dim3(strata_blocks(n)), dim3(256), 0, s, d_mask, (uint32_t)n, strata_words(st), (const unsigned long long *)d_sums, (unsigned long long *)d_off,
                       d_idx, (unsigned long long)idx_cap);
    return hipGetLastError();
}
/* avk_compare_packed_strata: pass 1 rides behind the packer's region passes, and the number of list entries comes back with the packer's state block — the
 * call's one round trip — so the index array is sized without a round trip of its own.  mask_only (a submitted batch): the mask pass alone, on the upload's
 * stream; nothing comes back, total stays 0. */
struct StrataJob {
    const avk_strata *st;
    uint32_t *d_mask;
    uint64_t *d_sums;
    uint64_t total = 0;
    bool counted = false;
    bool mask_only = false;
};

struct PackedOnDevice {
    uint8_t *t_cnt, *q_cnt, *a0_len, *a1_len, *var_type_zyg, *alleles;
    uint32_t *start, *raw;
    uint16_t *len, *contig, *rel_pos;
    hipEvent_t ready;
    /* the escape lists of the batch (avk_packed_escapes), copied with the rest; NULL without escapes */
    uint64_t *esc_region, *esc_slot, *esc_call;
    uint32_t *esc_len, *esc_cnt, *esc_rel, *esc_a0, *esc_a1;
    /* the label lists of a batch submitted with labels (avk_region_labels), copied with the rest; NULL without labels */
    uint64_t *lab_off;
    uint32_t *lab_idx;
};
/* host: the narrow per-entry fields of a packed batch with its escapes applied — for the host-side utilities (shards, merge counts, the merge path's host
 * fallback).  cnt[] has one entry per count slot: 2r / 2r + 1 = t_cnt / q_cnt of region r (compare form, cnt_b given), or in_cnt as it is (multi form, cnt_b NULL).
 * false: a list is not ascending or names an entry outside the batch, or a listed entry's narrow field is not 0 (the rule of avk_packed_escapes; the device refuses
 * the same batches: dp_esc_entry_bad). */
struct PackedWideHost {
    std::vector<uint32_t> len, cnt, rel, a0, a1;
};
static bool packed_widen_host(const uint16_t *len, uint64_t n, const uint8_t *cnt_a, const uint8_t *cnt_b, uint64_t n_slots, const uint16_t *rel, const uint8_t *a0, const uint8_t *a1,
                              uint64_t nv, const avk_packed_escapes *esc, PackedWideHost &w) {
    w.len.resize(n + 1), w.cnt.resize(n_slots + 1), w.rel.resize(nv + 1), w.a0.resize(nv + 1), w.a1.resize(nv + 1);
    for (uint64_t r = 0; r < n; ++r) w.len[r] = len[r];
    if (cnt_b)
        for (uint64_t r = 0; r < n; ++r) w.cnt[2 * r] = cnt_a[r], w.cnt[2 * r + 1] = cnt_b[r];
    else
        for (uint64_t i = 0; i < n_slots; ++i) w.cnt[i] = cnt_a[i];
    for (uint64_t v = 0; v < nv; ++v) w.rel[v] = rel[v], w.a0[v] = a0[v], w.a1[v] = a1[v];
    if (!esc_present(esc)) return true;
    if (!esc_arrays_ok(esc)) return false;
    auto listed = [](const uint64_t *idx, uint64_t p, uint64_t first, uint64_t count) { return idx[p] >= first && idx[p] - first < count && (p == 0 || idx[p - 1] < idx[p]); };
    for (uint64_t p = 0; p < esc->n_esc_regions; ++p) {
        if (!listed(esc->esc_region, p, esc->first_region, n)) return false;
        const uint64_t r = esc->esc_region[p] - esc->first_region;
        if (len[r]) return false;
        w.len[r] = esc->esc_len[p];
    }
    for (uint64_t p = 0; p < esc->n_esc_slots; ++p) {
        if (!listed(esc->esc_slot, p, esc->first_slot, n_slots)) return false;
        const uint64_t i = esc->esc_slot[p] - esc->first_slot;
        if (w.cnt[i]) return false;
        w.cnt[i] = esc->esc_cnt[p];
    }
    for (uint64_t p = 0; p < esc->n_esc_calls; ++p) {
        if (!listed(esc->esc_call, p, esc->first_call, nv)) return false;
        const uint64_t v = esc->esc_call[p] - esc->first_call;
        if (rel[v] || a0[v] || a1[v]) return false;
        w.rel[v] = esc->esc_rel_pos[p], w.a0[v] = esc->esc_a0_len[p], w.a1[v] = esc->esc_a1_len[p];
    }
    return true;
}

/* ---- download of a device-packed batch: dp_unpack on the device, then plain copies into the caller's arrays ------------------------- */
/* `later` (avk_compare_packed_submit): the copies out go on the context's copy-out stream behind `later->ev_unpacked`, the tally into `later->h_tally`, nothing is
 * waited for and the device buffers of the caller's layout stay in `later->temps` until avk_wait has seen `later->ev_done` (every destination must be pinned) */
struct DownloadLater {
    std::vector<void *> temps;
    uint64_t *h_tally;
    hipEvent_t ev_unpacked, ev_done;
    /* the parts of ONE split call (compare_packed_split) spill their BASEPAIR groups into one device buffer behind one counter: a part's dp_unpack appends where the
     * part before it stopped, the words it writes index the call's one list, and the caller reads the count and copies the list once, after the last part */
    uint32_t *shared_spill = nullptr, *shared_spill_count = nullptr;
    /* a batch submitted with labels (avk_compare_packed_submit_labels): the labels' sums cross with the results, in front of ev_done */
    const void *lab_dev = nullptr;
    void *lab_host = nullptr;
    size_t lab_bytes = 0;
};
static int download_device_packed(avk_ctx *ctx, const CallSpec &spec, avk_dev_batch *db, avk_result_batch *out, uint8_t *pair_exact, uint64_t *tally_words /* [AVK_TALLY_STRIDE] */,
                                  DownloadLater *later = nullptr) {
    const uint64_t n = db->n_regions, nv = db->n_variants_host;
    hipStream_t s = ctx->stream;
    std::vector<void *> temps;
    int rc = 0;
    auto tmp = [&](size_t bytes) -> void * {
        void *p = nullptr;
        if (!rc) rc = pool_alloc(ctx, &p, bytes);
        if (p) temps.push_back(p);
        return p;
    };
    auto done = [&](int code) {
        for (void *p : temps) pool_release(ctx, p);
        return code;
    };
    dpk::DpOut o;
    memset(&o, 0, sizeof(o));
    o.region_out = db->d_region_out, o.var_out = db->d_var_out, o.v_off = db->d_voff, o.t_off = db->d_in_t_off, o.q_off = db->d_in_q_off, o.t_cnt = db->d_in_t_cnt,
    o.q_cnt = db->d_in_q_cnt, o.n_regions = n, o.n_variants = nv, o.mode = db->last_mode;
    o.pk_voff = db->d_pk_voff, o.pk_tc = db->d_pk_tc, o.pk_qc = db->d_pk_qc;
    if (out->status || !out->region_packed) o.status = (int32_t *)tmp((n + 1) * 4);
    if (out->region_packed) o.region_packed = (uint64_t *)tmp((n + 1) * 8);
    if (out->ed_h1) o.ed_h1 = (uint32_t *)tmp((n + 1) * 4);
    if (out->ed_h2) o.ed_h2 = (uint32_t *)tmp((n + 1) * 4);
    if (out->n_optima) o.n_optima = (uint32_t *)tmp((n + 1) * 4);
    if (out->type_present) o.type_present = (uint16_t *)tmp((n + 1) * 2);
    const bool want_var = db->last_mode == 0 && (out->var_expected || out->var_observed || out->var_class || out->var_zyg || out->var_packed) && db->v_hi > db->v_lo;
    const uint64_t nvr = db->v_hi - db->v_lo; /* the calls this batch owns: only they are copied back */
    o.v_lo = db->v_lo;
    if (want_var) {
        if (out->var_expected) o.var_expected = (uint8_t *)tmp(nvr + 16);
        if (out->var_observed) o.var_observed = (uint8_t *)tmp(nvr + 16);
        if (out->var_class) o.var_class = (uint8_t *)tmp(nvr + 16);
        if (out->var_zyg) o.var_zyg = (uint8_t *)tmp(nvr + 16);
        if (out->var_packed) o.var_packed = (uint8_t *)tmp(nvr + 16);
    }
    uint8_t *d_exact = pair_exact ? (uint8_t *)tmp(n + 16) : nullptr;
    const bool want_bp_packed = out->bp_packed && out->bp_spilled && out->bp_groups && db->d_bp && db->d_bp_off && db->last_mode == 0;
    const bool bp_shared = later && later->shared_spill && later->shared_spill_count;
    if (want_bp_packed) {
        if (later && !bp_shared) return done(fail(ctx, AVK_E_STATE, "the packed BASEPAIR groups need a synchronous call"));
        o.bp_off_dev = db->d_bp_off, o.bp_dev = db->d_bp;
        o.bp_packed = (uint32_t *)tmp((n + 1) * 4);
        if (bp_shared) o.bp_spill = later->shared_spill, o.bp_spill_count = later->shared_spill_count;
        else {
            o.bp_spill = (uint32_t *)tmp(((size_t)db->n_bp_groups + 1) * 16);
            o.bp_spill_count = (uint32_t *)tmp(256);
            if (!rc && hipMemsetAsync(o.bp_spill_count, 0, 4, s) != hipSuccess) rc = fail(ctx, AVK_E_HIP, "result unpacking failed: %s", hipGetErrorString(hipGetLastError()));
        }
    }
    if (rc) return done(rc);
    if (!ctx->h_dpstate) {
        hipError_t e = hipHostMalloc((void **)&ctx->h_dpstate, sizeof(dpk::DpState) + 32, hipHostMallocDefault);
        if (e != hipSuccess) return done(fail(ctx, AVK_E_HIP, "pinned state block: %s", hipGetErrorString(e)));
    }
    static_assert(sizeof(dpk::DpState) >= AVK_TALLY_STRIDE * 8, "the pinned state block also receives the tally");
    hipError_t e = hipSuccess;
    if (want_var && !db->var_dense) { /* calls of the range that no region of this batch owns keep what the caller's arrays hold (another batch of the job may own them) */
        std::vector<CopySeg> pre = {{out->var_expected ? out->var_expected + db->v_lo : nullptr, o.var_expected, out->var_expected ? nvr : 0},
                                    {out->var_observed ? out->var_observed + db->v_lo : nullptr, o.var_observed, out->var_observed ? nvr : 0},
                                    {out->var_class ? out->var_class + db->v_lo : nullptr, o.var_class, out->var_class ? nvr : 0},
                                    {out->var_zyg ? out->var_zyg + db->v_lo : nullptr, o.var_zyg, out->var_zyg ? nvr : 0},
                                    {out->var_packed ? out->var_packed + db->v_lo : nullptr, o.var_packed, out->var_packed ? nvr : 0}};
        rc = copy_in(ctx, pre, false);
        if (rc) return done(rc);
    }
    /* A dense batch read from its packed source: word j of var_out is call v_lo + j (dp_unpack_calls), so the per-call outputs are made four calls per lane and the
     * region kernel keeps the per-region words only.  The two launches share no output.  Every other batch — wide and compact sources, a slice that is not dense,
     * DP_NOTE_OUTSIDE, the pair form — takes the region kernel alone, as before. */
    const bool by_element = want_var && db->var_dense && db->d_pk_voff && db->last_mode == 0 && db->n_variants_dev == nvr;
    dpk::DpOut o_regions = o;
    if (by_element) o_regions.var_expected = o_regions.var_observed = o_regions.var_class = o_regions.var_zyg = o_regions.var_packed = nullptr;
    if (e == hipSuccess && n && by_element) {
        hipLaunchKernelGGL(avk_dp_unpack_calls_kernel, dim3((unsigned)((nvr + 1023) / 1024)), dim3(256), 0, s, o, nvr);
        e = hipGetLastError();
    }
    if (e == hipSuccess && n) {
        hipLaunchKernelGGL(avk_dp_unpack_kernel, dim3((unsigned)((n + 256 * AVK_UNPACK_TILES - 1) / (256 * AVK_UNPACK_TILES))), dim3(256), 0, s, o_regions, d_exact);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return done(fail(ctx, AVK_E_HIP, "result unpacking failed: %s", hipGetErrorString(e)));
    std::vector<CopySeg> segs = {{out->status, o.status, out->status ? n * 4 : 0}, {out->region_packed, o.region_packed, out->region_packed ? n * 8 : 0},
                                 {out->ed_h1, o.ed_h1, n * 4}, {out->ed_h2, o.ed_h2, n * 4}, {out->n_optima, o.n_optima, n * 4},
                                 {out->type_present, o.type_present, n * 2}, {pair_exact, d_exact, pair_exact ? n : 0}};
    if (want_var) {
        segs.push_back({out->var_expected ? out->var_expected + db->v_lo : nullptr, o.var_expected, out->var_expected ? nvr : 0});
        segs.push_back({out->var_observed ? out->var_observed + db->v_lo : nullptr, o.var_observed, out->var_observed ? nvr : 0});
        segs.push_back({out->var_class ? out->var_class + db->v_lo : nullptr, o.var_class, out->var_class ? nvr : 0});
        segs.push_back({out->var_zyg ? out->var_zyg + db->v_lo : nullptr, o.var_zyg, out->var_zyg ? nvr : 0});
        segs.push_back({out->var_packed ? out->var_packed + db->v_lo : nullptr, o.var_packed, out->var_packed ? nvr : 0});
    }
    if (out->group_metrics && spec.emit_gm && db->d_gm) segs.push_back({out->group_metrics, db->d_gm, n * AVK_N_GROUPS * AVK_N_FIELDS * sizeof(uint32_t)});
    if (want_bp_packed) segs.push_back({out->bp_packed, o.bp_packed, n * sizeof(uint32_t)}); /* (the spilled groups and their count: below, behind the other copies — or the split call's, once) */
    else if (out->bp_off && out->bp_groups && db->d_bp && db->d_bp_off && db->last_mode == 0) {
        segs.push_back({out->bp_off, db->d_bp_off, (n + 1) * sizeof(uint32_t)});
        segs.push_back({out->bp_groups, db->d_bp, (size_t)db->n_bp_groups * 4 * sizeof(uint32_t)});
    }
    if (later) { /* queued on the copy-out stream, finished by avk_wait */
        hipStream_t so = ctx->copy_out_stream;
        hipError_t el = hipEventRecord(later->ev_unpacked, s);
        if (el == hipSuccess) el = hipStreamWaitEvent(so, later->ev_unpacked, 0);
        for (const CopySeg &sg : segs)
            if (el == hipSuccess && sg.bytes && sg.host) el = hipMemcpyAsync((void *)sg.host, sg.dev, sg.bytes, hipMemcpyDeviceToHost, so);
        if (el == hipSuccess) el = hipMemcpyAsync(later->h_tally, db->d_tally, (size_t)AVK_TALLY_STRIDE * 8, hipMemcpyDeviceToHost, so);
        if (el == hipSuccess && later->lab_bytes) el = hipMemcpyAsync(later->lab_host, later->lab_dev, later->lab_bytes, hipMemcpyDeviceToHost, so);
        if (el == hipSuccess) el = hipEventRecord(later->ev_done, so);
        if (el != hipSuccess) {
            (void)hipStreamSynchronize(so);
            return done(fail(ctx, AVK_E_HIP, "queueing the results' copies failed: %s", hipGetErrorString(el)));
        }
        later->temps.swap(temps);
        return 0;
    }
    CopyOut co;
    rc = copy_out(ctx, segs, &co);
    if (rc) return done(rc);
    e = hipMemcpyAsync(ctx->h_dpstate, db->d_tally, (size_t)AVK_TALLY_STRIDE * 8, hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) return done(fail(ctx, AVK_E_HIP, "tally download failed: %s", hipGetErrorString(e)));
    if (want_bp_packed) {
        /* how many groups were spilled decides how much of the list is copied.  The count rides behind the copies above (they start right behind dp_unpack, without
         * a word from the host), the list — a tenth of the results — behind the count: round 5 read the count first and every copy waited for that round trip */
        uint32_t *h_count = (uint32_t *)((uint8_t *)ctx->h_dpstate + sizeof(dpk::DpState));
        e = hipMemcpyAsync(h_count, o.bp_spill_count, 4, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return done(fail(ctx, AVK_E_HIP, "result unpacking failed: %s", hipGetErrorString(e)));
        const uint32_t spilled = *h_count;
        out->bp_spilled[0] = spilled;
        if (spilled) { /* (pinned: queued, finish_copy_out waits for it; pageable: a blocking copy — the bounce buffer holds the parts queued above) */
            const size_t tail_bytes = (size_t)spilled * 4 * sizeof(uint32_t);
            e = is_pinned(out->bp_groups, tail_bytes) ? (copies_by_kernel(ctx) ? kernel_copy(ctx, out->bp_groups, o.bp_spill, tail_bytes, s)
                                                                            : hipMemcpyAsync(out->bp_groups, o.bp_spill, tail_bytes, hipMemcpyDeviceToHost, s))
                                                      : hipMemcpy(out->bp_groups, o.bp_spill, tail_bytes, hipMemcpyDeviceToHost);
            if (e != hipSuccess) return done(fail(ctx, AVK_E_HIP, "result unpacking failed: %s", hipGetErrorString(e)));
        }
    }
    if (getenv("AVK_TIMING")) { /* the last mark of the call's device timeline: behind the copies out */
        if (!ctx->ev_tl[4] && hipEventCreate(&ctx->ev_tl[4]) != hipSuccess) ctx->ev_tl[4] = nullptr, (void)hipGetLastError();
        if (ctx->ev_tl[4]) (void)hipEventRecord(ctx->ev_tl[4], s);
    }
    rc = finish_copy_out(ctx, co);
    if (rc) return done(rc);
    memcpy(tally_words, ctx->h_dpstate, (size_t)AVK_TALLY_STRIDE * 8);
    return done(0);
}

/* every region record and blob of a device-packed batch (a run without lane launches, the host-side view) */
static int ensure_all_records(avk_ctx *ctx, avk_dev_batch *db, hipStream_t s) {
    if (!db->dev_packed || db->records_full || !db->n_regions) return 0;
    const uint32_t n = (uint32_t)db->n_regions;
    /* n_big restarts: the wave-level writer takes the large regions of this pass */
    AVK_HIP(ctx, hipMemsetAsync(&db->dp_args.st->n_big, 0, sizeof(uint32_t), s));
    hipLaunchKernelGGL(avk_dp_region_records_kernel, dim3((n + 255) / 256), dim3(256), 0, s, db->dp_args, n);
    hipLaunchKernelGGL(avk_dp_region_records_wave_kernel, dim3(256), dim3(256), 0, s, db->dp_args);
    AVK_HIP(ctx, hipGetLastError());
    db->records_full = true;
    return 0;
}

/* The host-side view of a device-packed batch (region records, blobs, the map from per-call output words to the caller's calls), fetched only when
 * something needs it: the capacity retry and the sequence outputs of avk_results_download. */
static int materialize_host_view(avk_ctx *ctx, avk_dev_batch *db) {
    if (!db->dev_packed || !db->host.regions.empty() || !db->n_regions) return 0;
    const uint64_t n = db->n_regions;
    {
        const int rf = ensure_all_records(ctx, db, ctx->stream);
        if (rf) return rf;
        AVK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    avk::PodVec<AvkDevRegion> recs;
    recs.resize(n);
    AVK_HIP(ctx, hipMemcpy(recs.data(), db->d_regions, n * sizeof(AvkDevRegion), hipMemcpyDeviceToHost));
    db->host.regions.resize(n);
    uint64_t blob_words = 2;
    for (uint64_t k = 0; k < n; ++k) {
        db->host.regions[recs[k].orig] = recs[k];
        const uint64_t end = 2ull * recs[k].blob_off + recs[k].blob_bytes / 4;
        if (recs[k].blob_bytes && end > blob_words) blob_words = end;
    }
    db->host.blob.resize(blob_words);
    AVK_HIP(ctx, hipMemcpy(db->host.blob.data(), db->d_blob, blob_words * 4, hipMemcpyDeviceToHost));
    std::vector<uint64_t> toff(n), qoff(n);
    if (db->d_pk_voff) { /* read from its packed source: the running sum of the calls, the query calls behind the truth calls */
        std::vector<uint8_t> tcs(n);
        AVK_HIP(ctx, hipMemcpy(toff.data(), db->d_pk_voff, n * 8, hipMemcpyDeviceToHost));
        AVK_HIP(ctx, hipMemcpy(tcs.data(), db->d_pk_tc, n, hipMemcpyDeviceToHost));
        for (uint64_t r = 0; r < n; ++r) qoff[r] = toff[r] + tcs[r];
    } else {
        AVK_HIP(ctx, hipMemcpy(toff.data(), db->d_in_t_off, n * 8, hipMemcpyDeviceToHost));
        AVK_HIP(ctx, hipMemcpy(qoff.data(), db->d_in_q_off, n * 8, hipMemcpyDeviceToHost));
    }
    db->host.dev2host.resize(db->n_variants_dev);
    for (uint64_t r = 0; r < n; ++r) {
        const AvkDevRegion &dr = db->host.regions[r];
        for (uint32_t k = 0; k < dr.t_cnt + dr.q_cnt; ++k) db->host.dev2host[dr.v_off + k] = k < dr.t_cnt ? toff[r] + k : qoff[r] + (k - dr.t_cnt);
    }
    return 0;
}
