/*
 * avk_host.hip — libaardvark_amd.so: the C-ABI of include/aardvark_amd.h on top of the gfx950
 * solver kernels.  Host code here owns device memory, streams and launches; the per-region
 * algorithm lives in avk_solver.inl and runs only on the GPU (there is no CPU path in this
 * library: without a HIP device every entry point fails with AVK_E_HIP).
 *
 * Launch shape: persistent workgroups of independent wavefronts, one wavefront solves one
 * region end to end in its workspace slice.  A step starts up to three launches side by side — the bulk (small LDS
 * slices, caller's stream) and, on two side streams, the solo launches of the regions the upload-time work plan
 * predicted to need a large LDS slice or an HBM slice — followed by one HBM launch for whatever still overflowed
 * (its list length is read on the device, so nothing returns to the host in between) and the tally reduce, which
 * also clears the counters for the next step.
 */
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/aardvark_amd.h"
#include "avk_pack.h"
#include "avk_pack_chunks.h"
#include "avk_counters.h"
#include "avk_step_plan.h"
#include "avk_step_geometry.h"
#include "avk_upload_forms.h"
#include "avk_solver.inl"
#include "avk_lane.inl"
#include "avk_quad.inl"
#include "avk_wide.inl"
#include "avk_dwfa_script.inl"
#include "avk_devpack.inl"
#include "avk_labels.inl"
#include "avk_strata.inl"
#include "avk_context.inl"
#include "avk_boot.inl"
#include "avk_callboot_host.h"
#include "avk_mergecount.inl"
#include "avk_mergesweep.inl"
static_assert((int)avk::ms::MS_KMAX == (int)avk::dp::DP_MERGE_KMAX, "the sweep kernel decides what the classification kernel decides");

/* ---------------------------------------------------------------------------------- kernels */
/* LDS passes: regions in the LDS slice of their wavefront (small slices at high occupancy first, then
 * the overflow of that pass with large slices at one workgroup per CU) */
#ifndef AVK_LDS_WAVES_PER_SIMD
#define AVK_LDS_WAVES_PER_SIMD 4
#endif
__global__ void __launch_bounds__(256, AVK_LDS_WAVES_PER_SIMD) avk_region_kernel_lds(AvkKernelArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char avk_smem[];
    const unsigned wave_in_block = threadIdx.x >> 6;
    const unsigned wave_id = blockIdx.x * (blockDim.x >> 6) + wave_in_block;
    if (a.high_priority) __builtin_amdgcn_s_setprio(3); /* solo launch: the long searches are the critical path */
    if (a.esc_bytes) { /* the workgroup's tail: control words and tally (AvkKernelArgs::esc_bytes) */
        for (unsigned k = threadIdx.x; k < AVK_WG_TAIL_BYTES / 4; k += blockDim.x) ((unsigned *)(avk_smem + a.esc_bytes))[k] = 0;
        __syncthreads();
    }
    avk::region_worker<true>(a, wave_id, avk_smem + (size_t)wave_in_block * a.tier[a.pass_tier].ws_bytes);
}

/* HBM passes: regions that outgrew the LDS tiers, in the wave's private HBM slice */
__global__ void __launch_bounds__(256, 2) avk_region_kernel_hbm(AvkKernelArgs a) {
    const unsigned wave_id = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    avk::region_worker<false>(a, wave_id, (unsigned char *)0);
}

/* The long windows, a workgroup per region (avk_solver.inl "a region on a TEAM of wavefronts"): wave 0 claims regions and runs their searches, its three siblings
 * take the independent pieces it posts — haplotype extensions of a popped node's children, the alignments of the metrics.  Every wave has an HBM slice: the
 * owner's is the region's workspace, a sibling's is its scratch. */
__global__ void __launch_bounds__(256, 2) avk_region_kernel_team(AvkKernelArgs a) {
    __shared__ avk::TeamBox box;
    for (unsigned k = threadIdx.x; k < sizeof(box) / 4; k += blockDim.x) ((uint32_t *)&box)[k] = 0;
    __syncthreads();
    const unsigned w = threadIdx.x >> 6;
    if (a.high_priority) __builtin_amdgcn_s_setprio(3);
    if (w == 0) {
        avk::region_worker<false, false, true>(a, blockIdx.x * 4u, (unsigned char *)0, &box);
        wv_sync();
        if ((threadIdx.x & 63u) == 0) avk_wg_store(&box.quit, 1u);
    } else if (a.team == 1) { /* (2 = the owner alone takes every job: a diagnostic) */
        avk::team_helper(&box, a.hbm_ws + (uint64_t)(blockIdx.x * 4u + w) * a.tier[a.pass_tier].ws_bytes, a.tier[a.pass_tier].ws_bytes, w, 4u);
    }
}

/* the same two for the regions the lanes handed back: device-packed batches (avk_devpack.inl) write the region record and blob of such a region
 * on demand, in the wave that is about to solve it (AvkKernelArgs::lazy_dp) */
__global__ void __launch_bounds__(256, AVK_LDS_WAVES_PER_SIMD) avk_region_kernel_lds_lazy(AvkKernelArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char avk_smem[];
    const unsigned wave_in_block = threadIdx.x >> 6;
    const unsigned wave_id = blockIdx.x * (blockDim.x >> 6) + wave_in_block;
    if (a.esc_bytes) {
        for (unsigned k = threadIdx.x; k < AVK_WG_TAIL_BYTES / 4; k += blockDim.x) ((unsigned *)(avk_smem + a.esc_bytes))[k] = 0;
        __syncthreads();
    }
    avk::region_worker<true, true>(a, wave_id, avk_smem + (size_t)wave_in_block * a.tier[a.pass_tier].ws_bytes);
}
__global__ void __launch_bounds__(256, 2) avk_region_kernel_hbm_lazy(AvkKernelArgs a) {
    const unsigned wave_id = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    avk::region_worker<false, true>(a, wave_id, (unsigned char *)0);
}

/* Small regions, one per LANE (avk_lane.inl): a workgroup is four independent waves, each claims tiles of 64 fast records; the
 * workgroup's LDS holds the four waves' per-lane arrays and one shared tally that is flushed once */
#ifndef AVK_LANE_WPE
#define AVK_LANE_WPE 3
#endif
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(AVK_LANE_WPE))) avk_lane_kernel(AvkKernelArgs a, avk::lane::LaneArgs la) {
    extern __shared__ __attribute__((aligned(16))) unsigned char avk_smem[];
    uint32_t *smem = (uint32_t *)avk_smem;
    const unsigned wave_in_block = threadIdx.x >> 6;
    const unsigned wave_id = blockIdx.x * (blockDim.x >> 6) + wave_in_block;
    const uint32_t rows = avk::lane::lane_rows(la.W, la.nm, la.ed_max, la.qcap, la.pool);
    const uint32_t wave_words = rows << la.lanes_log2;
    uint32_t *wg_tally = smem + (size_t)(blockDim.x >> 6) * wave_words;
    for (unsigned k = threadIdx.x; k < 288; k += blockDim.x) wg_tally[k] = 0;
    __syncthreads();
    uint32_t n_ok = 0, n_err = 0;
    uint64_t *part = a.tally + (uint64_t)(blockIdx.x % AVK_TALLY_COPIES) * AVK_TALLY_STRIDE;
    avk::lane::lane_worker(a, la, wave_id, smem + (size_t)wave_in_block * wave_words, wg_tally, n_ok, n_err, blockDim.x == 64 ? part : (uint64_t *)0);
    n_ok = wv_sum_u32(n_ok);
    n_err = wv_sum_u32(n_err);
    if ((threadIdx.x & 63u) == 0) {
        if (n_ok) {
            atomicAdd((unsigned long long *)(part + AVK_TALLY_SOLVED), (unsigned long long)n_ok);
            atomicAdd((unsigned long long *)(part + AVK_TALLY_LANE_SOLVED), (unsigned long long)n_ok);
        }
        if (n_err) {
            atomicAdd((unsigned long long *)(part + AVK_TALLY_ERRORS), (unsigned long long)n_err);
            atomicAdd((unsigned long long *)(part + AVK_TALLY_LANE_SOLVED), (unsigned long long)n_err);
        }
    }
    __syncthreads();
    for (unsigned k = threadIdx.x; k < AVK_N_GROUPS * AVK_N_FIELDS; k += blockDim.x) {
        const uint32_t v = wg_tally[k];
        if (v) atomicAdd((unsigned long long *)(part + k), (unsigned long long)v);
    }
}

/* The expensive small regions — the heads of the lane classes and the three-call class — one per QUAD (avk_quad.inl): the same records, rows and
 * results as avk_lane_kernel at 16 (8, 4) records per wave, four lanes on every region instead of one */
#ifndef AVK_QUAD_WPE
#define AVK_QUAD_WPE 3
#endif
static __device__ __forceinline__ void avk_quad_body(const AvkKernelArgs &a, const avk::lane::LaneArgs &la) {
    extern __shared__ __attribute__((aligned(16))) unsigned char avk_smem[];
    uint32_t *smem = (uint32_t *)avk_smem;
    const uint32_t rows = avk::quad::quad_rows(la.W, la.nm, la.ed_max, la.qcap, la.pool);
    const uint32_t wave_words = rows << la.lanes_log2;
    uint32_t *wg_tally = smem + wave_words;
    for (unsigned k = threadIdx.x; k < 288; k += blockDim.x) wg_tally[k] = 0;
    __syncthreads();
    uint32_t n_ok = 0, n_err = 0;
    uint64_t *part = a.tally + (uint64_t)(blockIdx.x % AVK_TALLY_COPIES) * AVK_TALLY_STRIDE;
    avk::quad::quad_worker(a, la, blockIdx.x, smem, wg_tally, n_ok, n_err, part);
    n_ok = wv_sum_u32(n_ok);
    n_err = wv_sum_u32(n_err);
    if ((threadIdx.x & 63u) == 0) {
        if (n_ok) {
            atomicAdd((unsigned long long *)(part + AVK_TALLY_SOLVED), (unsigned long long)n_ok);
            atomicAdd((unsigned long long *)(part + AVK_TALLY_LANE_SOLVED), (unsigned long long)n_ok);
        }
        if (n_err) {
            atomicAdd((unsigned long long *)(part + AVK_TALLY_ERRORS), (unsigned long long)n_err);
            atomicAdd((unsigned long long *)(part + AVK_TALLY_LANE_SOLVED), (unsigned long long)n_err);
        }
    }
    __syncthreads();
    for (unsigned k = threadIdx.x; k < AVK_N_GROUPS * AVK_N_FIELDS; k += blockDim.x) {
        const uint32_t v = wg_tally[k];
        if (v) atomicAdd((unsigned long long *)(part + k), (unsigned long long)v);
    }
}
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(AVK_QUAD_WPE))) avk_quad_kernel(AvkKernelArgs a, avk::lane::LaneArgs la) { avk_quad_body(a, la); }
/* The same code for launches whose LDS slice holds a CU to two waves per SIMD anyway (the three-call class: 20 KB per one-wave workgroup, seven per CU): built for two
 * waves per SIMD it has 256 registers and spills nothing (at three: 168 registers, 26 VGPR + 214 SGPR spills, 108 bytes of scratch per lane) */
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) avk_quad_kernel_wide_regs(AvkKernelArgs a, avk::lane::LaneArgs la) { avk_quad_body(a, la); }

/* Regions with large searches on small windows, one per wave, every lane a piece of the search (avk_wide.inl): one-wave workgroups, the region's tables in
 * the workgroup's LDS */
__global__ void __launch_bounds__(64) avk_wide_kernel(AvkKernelArgs a, avk::wide::WideArgs wa) {
    extern __shared__ __attribute__((aligned(16))) unsigned char avk_smem[];
    avk::wide::wide_worker<false>(a, wa, blockIdx.x, (uint32_t *)avk_smem);
}
/* the same for regions the lanes handed back (device-packed batches write their records on demand, AvkKernelArgs::lazy_dp) */
__global__ void __launch_bounds__(64) avk_wide_kernel_lazy(AvkKernelArgs a, avk::wide::WideArgs wa) {
    extern __shared__ __attribute__((aligned(16))) unsigned char avk_smem[];
    avk::wide::wide_worker<true>(a, wa, blockIdx.x, (uint32_t *)avk_smem);
}

/* regions with the same SNV on both sides (avk_pairs.inl): table rows copied out, 64 regions per wave at a time */
__global__ void __launch_bounds__(256) avk_pair_kernel(AvkKernelArgs a, avk::pairs::PairArgs pa) {
    avk::pairs::pair_worker(a, pa, a.tally + (uint64_t)(blockIdx.x % AVK_TALLY_COPIES) * AVK_TALLY_STRIDE);
}

/* DWFALite scripts (avk_dwfa_script.inl): engine 0 one script per wavefront, engine 1 one script per lane */
__global__ void __launch_bounds__(256) avk_dwfa_wave_kernel(AvkDwfaArgs a) {
    const unsigned wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (wave < a.n_scripts) avk::dwfa_script_wave(a, wave);
}
__global__ void __launch_bounds__(64) avk_dwfa_lane_kernel(AvkDwfaArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char avk_smem[];
    const unsigned s = blockIdx.x * 64u + threadIdx.x;
    if (s < a.n_scripts) avk::lane::dwfa_script_lane(a, s, (uint32_t *)avk_smem);
}

/* Stratified tallies (SummaryWriter::add_comparison_benchmark with containment regions, writers/summary.rs:146-163): label l sums the
 * metric blocks of the solved regions whose label list names it.  One wave per region at a time; a workgroup keeps the tallies of the
 * AVK_LABEL_BLOCK labels of this launch in LDS (64-bit adds) and flushes them once — HBM traffic is the 1144-byte metric block of
 * every region that has a label in the block, read once. */
#define AVK_LABEL_BLOCK 16
#define AVK_GM_WORDS (AVK_N_GROUPS * AVK_N_FIELDS)
__global__ void __launch_bounds__(256) avk_label_tally_kernel(const uint32_t *gm, const uint32_t *region_out, const unsigned long long *label_off,
                                                             const uint32_t *label_idx, uint32_t n_regions, uint32_t label_lo, uint32_t label_hi,
                                                             unsigned long long *out) {
    __shared__ unsigned long long acc[AVK_LABEL_BLOCK * AVK_GM_WORDS];
    for (unsigned k = threadIdx.x; k < AVK_LABEL_BLOCK * AVK_GM_WORDS; k += blockDim.x) acc[k] = 0;
    __syncthreads();
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), n_waves = gridDim.x * (blockDim.x >> 6);
    for (unsigned r = wave; r < n_regions; r += n_waves) {
        if (region_out[4u * r] != 0) continue; /* only solved regions count */
        const unsigned long long lo = label_off[r], hi = label_off[r + 1];
        bool any = false;
        for (unsigned long long q = lo; q < hi; ++q) {
            const uint32_t l = label_idx[q];
            any = any || (l >= label_lo && l < label_hi);
        }
        if (!any) continue;
        uint32_t v[5];
        const uint32_t *block = gm + (size_t)r * AVK_GM_WORDS;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const unsigned i = lane + 64u * (unsigned)j;
            v[j] = i < AVK_GM_WORDS ? block[i] : 0u;
        }
        for (unsigned long long q = lo; q < hi; ++q) {
            const uint32_t l = label_idx[q];
            if (l < label_lo || l >= label_hi) continue;
            unsigned long long *dst = acc + (size_t)(l - label_lo) * AVK_GM_WORDS;
#pragma unroll
            for (int j = 0; j < 5; ++j)
                if (v[j]) atomicAdd(dst + lane + 64u * (unsigned)j, (unsigned long long)v[j]);
        }
    }
    __syncthreads();
    for (unsigned k = threadIdx.x; k < (label_hi - label_lo) * AVK_GM_WORDS; k += blockDim.x) {
        const unsigned long long x = acc[k];
        if (x) atomicAdd(out + (size_t)(label_lo + k / AVK_GM_WORDS) * AVK_TALLY_LEN + k % AVK_GM_WORDS, x);
    }
}

/* packs the uploaded reference: 16 bases per word, 2 bits each, plus one flag per word for anything that is
 * not an upper-case A/C/G/T (those windows are read from the byte copy).  One thread per packed word. */
__global__ void avk_pack_reference(const uint8_t *bytes, uint64_t n_bases, uint32_t *packed, uint32_t *exc) {
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t n_words = (n_bases + 15) >> 4;
    uint32_t word = 0, bad = 0;
    if (w < n_words) {
        for (int j = 0; j < 16; ++j) {
            const uint64_t p = w * 16 + j;
            uint32_t code = 0;
            if (p < n_bases) {
                const uint8_t ch = bytes[p];
                if (ch == 'A') code = 0;
                else if (ch == 'C') code = 1;
                else if (ch == 'G') code = 2;
                else if (ch == 'T') code = 3;
                else bad = 1;
            }
            word |= code << (2 * j);
        }
        packed[w] = word;
    }
    const unsigned long long m = __ballot(bad != 0);
    const unsigned lane = threadIdx.x & 63u;
    if (w < n_words + 64 && (lane & 31u) == 0) { /* 64 consecutive words = two 32-bit flag words */
        const uint64_t fw = w >> 5;
        if (fw <= ((n_words + 31) >> 5)) exc[fw] = lane == 0 ? (uint32_t)m : (uint32_t)(m >> 32);
    }
}

/* sums the partial tallies into out[0 .. AVK_TALLY_STRIDE) (and the caller's device tally, if any), then clears
 * the partial tallies and the work / overflow counters for the next call on this batch */
/* The records of class C (work order 0 .. n_c - 1) that are not for avk_wide.inl by what they say themselves (avk_wide_static_ok), as a list: a few dozen among
 * thousands, each a long search on a wave of the HBM tier.  Their launch used to walk the whole class in claims of four and solved the not-wide records of a claim one
 * after the other. */
__global__ void __launch_bounds__(256) avk_notwide_list_kernel(const AvkDevRegion *regions, uint32_t n_c, uint32_t *list, uint32_t *count) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_c) return;
    const AvkDevRegion *g = regions + i;
    if (avk_wide_static_ok(g->len, g->grow, g->ed_bound, g->t_cnt, g->q_cnt, g->pre_status)) return;
    list[atomicAdd(count, 1u)] = i;
}

__global__ void avk_tally_reduce(uint64_t *partials, uint64_t *out, uint64_t *out_user, uint32_t *counters, unsigned n_counters, unsigned accumulate) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    for (unsigned k = i; k < n_counters; k += gridDim.x * blockDim.x) counters[k] = 0;
    if (i >= AVK_TALLY_STRIDE) return;
    uint64_t s = 0;
    for (int c = 0; c < AVK_TALLY_COPIES; ++c) {
        s += partials[(size_t)c * AVK_TALLY_STRIDE + i];
        partials[(size_t)c * AVK_TALLY_STRIDE + i] = 0;
    }
    out[i] = s;
    if (out_user && i < AVK_TALLY_LEN) out_user[i] = accumulate ? out_user[i] + s : s; /* accumulate: a job's running total over its batches */
}

/* ---------------------------------------------------------------------------------- context */
namespace {

std::string g_create_error;
std::mutex g_create_mutex;

struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
};

struct PoolBlk { /* a device buffer of the context's pool (avk_devpack_host.inl) */
    void *p;
    size_t bytes;
    bool used;
};

} // namespace

#define AVK_STREAM_ORDER_DEFAULT "stwxxabxxcd" /* profiles/r06_stream_order.txt */

struct avk_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string err;
    /* reference */
    uint8_t *d_ref = nullptr;
    uint32_t *d_ref2b = nullptr, *d_refexc = nullptr;
    int64_t use_packed_reference = 1;
    std::vector<uint64_t> contig_base, contig_len;
    uint64_t *d_contig_tab = nullptr; /* contig_base[n_contigs] then contig_len[n_contigs], for the device-side packer */
    /* device-side packing (avk_devpack_host.inl, avk_upload.inl) */
    int64_t adaptive_ws = 1;               /* device-packed batches size their per-wave HBM slices by the predicted need of their class C regions (option ws_bytes_per_wave is the minimum) */
    int64_t ws_budget_bytes = 96ll << 30;  /* at most this much HBM for those slices: fewer waves per launch when the slices are large */
    int64_t device_pack = 1;               /* batches are validated, classified, ordered and written ON THE DEVICE from the caller's arrays (0: avk_pack.h on the host threads) */
    int64_t pool_cache_bytes = 12ll << 30; /* released device buffers the context keeps for the next batch (beyond: back to the runtime) */
    std::vector<PoolBlk> pool;
    std::mutex pool_mutex;
    size_t pool_free_bytes = 0;
    uint8_t *h_bounce = nullptr; /* pinned staging for caller arrays that are not pinned (grow-only) */
    size_t bounce_bytes = 0;
    void *h_dpstate = nullptr;   /* pinned: the packer's state block / the tally of a download */
    /* the asynchronous boundary (avk_compare_packed_submit / avk_wait): a copy stream each way and a ring of staging slots OUTSIDE the stream-ordered pool — the
     * packed arrays of batch k + 1 cross the bus while batch k is being solved, the results of batch k while batch k + 1 is being packed */
    hipStream_t copy_in_stream = nullptr, copy_out_stream = nullptr;
    hipStream_t pack_stream = nullptr, pack_side_stream = nullptr; /* the packing kernels of a submitted batch, beside the solver launches of the batch before */
    hipEvent_t ev_packed = nullptr, ev_pool_fence = nullptr;
    bool pool_fence_pending = false; /* buffers went back to the pool in the order of the context's stream since the packing stream last waited for it */
    int64_t async_pack_stream = 1;                                 /* option: 0 = a submitted batch is packed on the context's stream, behind the solve of the batch before */
    struct StageSlot {
        uint8_t *dev = nullptr; /* one device block for the eleven arrays of an avk_packed_batch */
        size_t bytes = 0;
        uint64_t *h_tally = nullptr; /* pinned: the batch's tally lands here */
        hipEvent_t ev_in = nullptr, ev_unpacked = nullptr, ev_done = nullptr;
        bool busy = false;
        uint64_t *h_labels = nullptr; /* pinned: the label sums of a batch submitted with labels land here (grown on demand) */
        size_t h_labels_words = 0;
    } stage[4];
    hipEvent_t ev_lab0 = nullptr, ev_lab1 = nullptr; /* AVK_TIMING: around the label kernels */
    int64_t label_lds_bytes = 0;       /* LDS a launch of avk_label_tally_compact_kernel gets (0: not asked yet) */
    int64_t callboot_lds_bytes = 0;    /* LDS a launch of avk_callboot_tally_kernel gets (0: not asked yet) */
    int64_t mergecount_lds_bytes = 0;  /* ... and a launch of avk_merge_count_kernel */
    int last_merge_counts_on_device = 0; /* the last avk_merge_packed_counts with counters made them by kernel */
    /* options */
    int64_t lds_bytes_per_wave = 10 * 1024;
    int64_t lds_ed_cap = 48;
    int64_t lds2_bytes_per_wave = 40 * 1024;
    int64_t lds2_ed_cap = 48;
    int64_t waves_per_cu = 16;
    int64_t solo_min_variants = 5; /* regions with at least this many variants go to solo waves (0 = no solo waves) */
    int64_t solo_blocks_max = 128;
    int64_t timing_events = 1; /* record the events avk_last_kernel_ms / avk_last_solver_ms read (three per call) */
    bool kernel_attrs_set = false; /* ensure_kernel_attrs has run */
    int64_t static_pct = AVK_STATIC_PCT; /* share of a launch's work list dealt statically; the rest is claimed */
    int64_t claim = AVK_CLAIM;           /* regions per claim */
    int64_t class_c_below = 16384; /* a batch with lane launches and at most this many regions outside them plans those regions as class C: the wide kernel (0: no such rule) */
    int64_t class_c_nodes_x2 = 12; /* a region is sent to the HBM solo launch when 0.5 x this x N nodes outgrow a tier-1 slice */
    int64_t solo_regions_per_wave = 4; /* predicted-hard regions beyond solo waves x this lead the bulk list */
    int64_t accumulate_tally = 0; /* avk_compare_resident adds to the caller's device tally instead of overwriting it */
    int64_t lds_escalation = 1; /* in-workgroup escalation of the bulk launch (AvkKernelArgs::esc_bytes) */
    int64_t lds2_overflow_pass = 0; /* 1: a launch of its own with large LDS slices between the bulk and the HBM tier */
    int64_t bulk_full_grid = 0; /* 1: keep the bulk grid at full size (late workgroups only claim); measured unstable */
    int64_t bulk_fit = 1;       /* 1: no more workgroups in the bulk launch than its list has regions for (a genome leaves it three dozen regions: 664 workgroups of 40 KB of
                                   LDS queued for them beside the lane launches) */
    int64_t ws_bytes_per_wave = 1 << 20;
    int64_t big_ws_bytes = 64ll << 20; /* (256 MB until round 5: the shared slices were 2.1 GB of a fresh process's first hipMalloc; a batch whose packer predicts larger regions gets 1 GB slices, upload_device_packed) */
    int64_t big_waves = 8;
    int64_t emit_group_metrics = 1;
    int64_t team_long_windows = 1;         /* 1: the launch of the long windows runs a workgroup per region (avk_region_kernel_team); 0: a wave per region (round 5) */
    int64_t team_head_regions = 48;        /* a batch of large windows (no region of class C is the wide kernel's): this many regions at the head of the class go to a team launch */
    int64_t split_parts = 1;               /* > 1: a large avk_compare_packed call runs as this many batches in flight (compare_packed_split; measured slower than the whole call while a half genome's step costs 2.0 of the whole's 2.4 ms: profiles/r06_split_call.txt) ... */
                                           /* ... when every part has at least 4096 regions and every array of the caller's is pinned */
    int64_t copy_blocks_per_cu = 8; /* workgroups of avk_copy_kernel per CU (AVK_COPY_BLOCKS in the environment overrides: a tuning aid) */
    int64_t kernel_copies = 1;  /* the pinned arrays of a synchronous call cross the bus 0: by the DMA engine the process drew, 2: by a copy kernel, 1: by whichever a measurement of
                                   the engine says (avk_devpack_host.inl: copies_by_kernel) */
    bool engines_fast = true;   /* no two consecutive timed calls of this context have seen their arrays cross below 36 GB/s on the engine */
    int engine_slow_calls = 0;  /* timed calls in a row below that rate (engine_rate_check: one noisy measurement does not switch the context for good) */
    double engine_in_gbs = 0;
    size_t cp_timed_bytes = 0;  /* bytes between ev_cp0 and ev_cp1 of the last engine-timed copy_in (0: none pending) */
    hipEvent_t ev_cp0 = nullptr, ev_cp1 = nullptr;
    int64_t pack_chunks = 0;    /* N = 2 .. 8: a synchronous packed compare call's per-region and per-call arrays cross in N groups and the region pass runs group by group under
                                   the copies (avk_pack_chunks.h, upload_device_packed); 0: one region launch behind the last copy.  Off: two groups gain
                                   0.09 ms of a whole-genome call over pack_queue_early alone, with four hardware queues and with 24 — inside the spread of the
                                   four-queue runs (profiles/pack_chunks_ab.txt) */
    int64_t pack_queue_early = 1; /* 1: such a call queues the side stream's steps (prefix sums, dp_variant) from inside copy_in, each right behind the event it waits for, so
                                     that they run under the copies also where the side stream shares the copy stream's hardware queue; 0: after the copies are queued */
    int64_t pack_chunk_floor = 1 << 20; /* a batch whose groups would copy less than this many bytes of some array keeps the old order (tests lower it so that small batches chunk) */
    hipEvent_t ev_pack_group[avk::pc::PC_MAX_GROUPS] = {nullptr}; /* behind the copies of group j (made when first used; the last group records ev_copy_mid) */
    uint64_t last_region_launches = 0; /* launches of the region pass the last device-packed upload queued (avk_last_region_launches) */
    int64_t packed_source = 1;  /* 1: a batch in the packed form is packed from the packed arrays themselves (no wide copy of the caller's arrays in HBM); 0: round 5's widening pass */
    int64_t emit_bp_groups = 0; /* kernels write the compact per-region BASEPAIR groups (avk_result_batch::bp_groups) */
    int64_t capacity_retry = 1; /* avk_results_download solves regions that exhausted the last workspace tier again with larger slices */
    int64_t lane_kernel = 1; /* small regions go to the lane-per-region kernel (avk_lane.inl) */
    int64_t lane_min_regions = 2048; /* a lane class is launched when it holds at least this many regions (x16 for the two-call classes, x2 for the three-call
                                        class): a launch lasts at least as long as its slowest tile, which a small class cannot amortise.  8192 until the end of round 4;
                                        since the lanes keep node states and skip mirror-image optima their classes pay at a quarter of the size: an eighth-of-a-genome
                                        step 2.0 -> 1.5 ms, a quarter-genome step 3.6 -> 2.15 ms, the whole genome unchanged (profiles/r04_lane_min.txt) */
    int64_t lane_width_one = 64, lane_width_two = 64, lane_width_three = 16; /* records a wave takes at a time (64, 32, 16) in the one- / two- / three-call classes */
    int64_t lane_max_calls = AVK_FAST_MAXV;           /* classes with more calls per side stay with the wave-per-region kernels */
    int64_t lane_max_est = 15;                        /* regions whose estimated edits (fast_cost_key, avk_pack.h) exceed this stay with the wave-per-region kernels */
    int64_t pair_classes = 1;                         /* 1: pair batches (merge) plan their large searches as classes C / B like compare batches do, so that the wide kernel
                                                         and the solo launches take them at the start of the step; 0 (until the end of round 4): everything the lanes do not take
                                                         goes through the bulk and what overflows there through an HBM launch at the very end — a 3-caller whole-genome merge
                                                         call 22.5 -> 16 ms */
    int64_t lane_head_auto = 1;                       /* 1: a head of fewer regions than the machine has lane waves for takes fewer records per wave (lane_head_width is the most):
                                                         under 24,576 regions 8, under 8,192 regions 4 — an eighth-of-a-genome step 1.5 -> 1.2 ms, a quarter genome 2.15 -> 1.95 */
    int64_t lane_head_width = 16;                     /* records a wave takes at a time in the HEAD of a lane class: the tiles of regions with estimated edits (0 = no head launch) */
    int64_t lane_metrics_ed_cap = 0;                  /* lanes hand a region over when an alignment of its metrics phase passes this distance (0 = as far as the LDS rows allow: 30 / 54) */
    int64_t hbm_ed_cap = 1024;                        /* the per-wave HBM slices size a region's wavefronts by the region's own bound (the sum of its calls' edit distances) when that is at most this;
                                                         0: two entries per base of the window for every region (rounds 1-2).  Large windows: 1.64 -> 1.21 s per 49 k-region step, whole genome -3 % */
    int64_t het_search_min = AVK_HET_SEARCH_MIN;      /* regions with at least this many unphased heterozygous calls go to class C and stay out of the three-call lane class (0 = no such rule) */
    int64_t lane_head_est = 1;                        /* regions with at least this many estimated edits (fast_cost_key) form the narrow-tiled head of their lane class */
    int64_t lane_pairs = 1;                           /* regions with the same SNV on both sides are looked up in a table the solver fills (avk_pairs.inl); 0: they stay in the one-call classes */
    avk::pairs::PairTable *d_pair_tab = nullptr;      /* the table, made for max_branch_factor pair_tab_mbf */
    uint32_t *d_pair_aux = nullptr;                   /* probe records, probe reference and the scratch outputs of the probe launch */
    int64_t pair_tab_mbf = -1;
    int64_t pair_blocks_per_cu = 4;                   /* workgroups (4 waves) of the lookup launch per CU */
    int64_t lane_stripe = 0;                          /* 1: the heads' records dealt out over their claims (avk_stripe_slot, avk_dev_types.h) instead of most expensive first.  Measured
                                                         WORSE (whole genome 4.84 -> 5.40 ms per step): regions of one cost key take the same path through the search, a claim of equals
                                                         runs in lockstep, a claim of unequals takes turns */
    int64_t lane_head_stream = 0;                     /* 1: the heads of the two-call classes on a stream of their own (a synchronised step: 5.4 -> 5.1 ms;
                                                         steps queued back to back: 6.0 -> 6.5 ms — more streams, worse starts; off) */
    int64_t lane_min_batch = 16384;                   /* a RESIDENT batch with fewer lane regions than this is solved by the wave-per-region kernels alone (not applied when lane_min_regions is 0, nor by the one-shot path of avk_compare_batch) */
    int64_t hbm_early_blocks = 64;                    /* workgroups (x 4 waves, 1 MB of HBM workspace each) of the launch behind the three-call lane class */
    int64_t hbm_solo_blocks = 64;                     /* most workgroups (x 4 waves, 1 MB of HBM workspace each) of the HBM solo launch */
    int64_t lane_node_cap = 32;                       /* search nodes the three-call lane class makes before it hands a region over */
    int64_t lane_quad = 1;                            /* 1: lane launches of at most 16 records per wave (the heads, the three-call class) run four lanes per region: avk_quad_kernel, avk_quad.inl */
    int64_t lane_pool = -1;                           /* node states a lane keeps during its search (avk_lane.inl NodePool): -1 = by class (2 / 4 / 6 for one / two / three calls per side), 0 = none */
    int64_t lane_waves_three = 0;                     /* > 0: at most this many one-wave workgroups of the three-call class per CU (its waves take 17 KB of LDS each) */
    int64_t lane_waves_per_cu = 12;                   /* at most this many one-wave workgroups of a lane launch per CU */
    int64_t wide_kernel = 1;                          /* regions with large searches on small windows (class C, what the three-call lane class hands back) go to the wave-cooperative kernel of avk_wide.inl first */
    int64_t wide_lds_bytes = 16 * 1024;               /* LDS of one of its waves: 1.2 KB of tables, the region's 2^T + 2^Q full-length sequences, the rest search nodes (10 words each, at most 240) and 32 wavefront blocks */
    int64_t wide_retry_lds_bytes = 64 * 1024;         /* LDS per wave of the second launch over what the class C launch handed over (0: none) */
    int64_t wide_blocks = 512;                        /* most one-wave workgroups of its class C launch */
    int64_t wide_lane_handbacks = 1;                  /* what the one- and two-call lane classes hand back goes through avk_wide.inl too, ahead of the LDS launch */
    int64_t wide_lazy_blocks = 512;                   /* one-wave workgroups of its launch for what the three-call lane class hands back (a short list, its length known on the device only) */
    uint64_t last_wide_solved = 0;
    uint64_t last_lane_solved = 0;
    int last_one_shot = 0; /* the last avk_compare_batch / avk_optimize_pairs_batch packed its batch on the device */
    int n_cus = 0;
    /* workspaces (grown on demand) */
    uint8_t *d_ws = nullptr;
    size_t ws_alloc = 0;
    uint8_t *d_big = nullptr;
    size_t big_alloc = 0;
    /* measurement */
    hipEvent_t ev0 = nullptr, ev1 = nullptr, evk1 = nullptr; /* ev0..ev1 all solver launches, ev0..evk1 the first (dominant) one */
    hipEvent_t ev_lane = nullptr; /* after the lane-kernel launches of a step */
    bool ev_lane_valid = false;
    hipStream_t lane_stream = nullptr, lane_stream2 = nullptr; /* the lane-kernel launches run beside the wave-per-region launches: two-call classes / one-call classes */
    hipEvent_t ev_lane_fork = nullptr;
    hipStream_t lane_stream3 = nullptr; /* the three-call class: long tiles, few of them, beside everything else */
    hipStream_t lane_stream4 = nullptr; /* the head launches of the two-call classes (long: beside the rest of their class, not ahead of it) */
    hipEvent_t ev_hb[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}; /* ends of the lane classes' head launches (handback_chains) */
    hipEvent_t ev_tl[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}; /* AVK_TIMING only: marks of a boundary call on the context's stream (first copy, last copy, work order, writers, results)
                                                                                     and, [5], behind the region pass on whichever stream it ran */
    bool tl_region_valid = false; /* ev_tl[5] was recorded by the last upload */
    hipEvent_t ev_copy_alleles = nullptr; /* packed upload: behind the allele bytes' copy (dp_variant starts there) */
    hipEvent_t ev_copy_fork = nullptr, ev_copy_mid = nullptr, ev_copy_join = nullptr; /* packed upload: all but the counts cross on lane_stream4 beside the offset kernels */
    hipStream_t side_stream = nullptr, side_stream2 = nullptr; /* solo launches (LDS, HBM): one stream each, they run side by side */
    hipStream_t spare_stream[16] = {nullptr}; /* never used: see avk_ctx_create */
    int n_placeholders = 0;                   /* how many of them avk_ctx_create made (and destroyed again) */
    hipStream_t wide_stream = nullptr; /* the class C records that are not for the wide kernel (the step, avk_step.inl) */
    /* the step's plan (avk_step_plan.h): which stream each launch chain of the step is queued on */
    int64_t step_queues = 0;       /* option: 0 by the process's hardware queues (step_folded_auto), 4 the folded plan, 8 a stream per chain */
    bool step_folded_auto = false; /* GPU_MAX_HW_QUEUES below AVK_STEP_QUEUES_WIDE when the context was made */
    hipStream_t fold_stream[AVK_STEP_SLOTS_FOLDED - 1] = {nullptr, nullptr, nullptr}; /* the folded plan's streams beside the caller's */
    bool last_step_chains = false; /* the last step ran with hand-back chains (it recorded no AVK_END_DONE) */
    std::thread reaper; /* releases the buffers of the last large batch behind the caller (avk_batch_free) */
    std::mutex reaper_mutex;
    hipEvent_t ev_fork = nullptr;
    hipEvent_t ev_end[AVK_N_ENDS] = {nullptr}; /* the ends of the step's chains, by AvkStepEnd (avk_step_plan.h) */
    bool ev_valid = false;
    uint64_t last_tiers[5] = {0, 0, 0, 0, 0};
    uint64_t last_phase[16] = {0};
};

struct avk_dev_batch {
    avk::PackedBatch host; /* regions/variants kept for the scatter maps */
    uint64_t n_regions = 0, n_variants_dev = 0, n_variants_host = 0;
    bool want_seq = false;
    uint64_t seq_total = 0;
    AvkDevRegion *d_regions = nullptr;
    uint32_t *d_blob = nullptr; /* region blobs (AvkBlobVar in avk_dev_types.h) */
    uint32_t *d_region_out = nullptr; /* [n][4] */
    uint32_t *d_gm = nullptr;
    uint32_t *d_var_out = nullptr;    /* [nv] */
    uint8_t *d_seq = nullptr;
    uint32_t *d_seqlen = nullptr;
    uint64_t *d_tally = nullptr;    /* [AVK_TALLY_STRIDE]: AVK_TALLY_LEN sums, 5 tier counters, 8 profiling words */
    uint64_t *d_partials = nullptr; /* [AVK_TALLY_COPIES][AVK_TALLY_STRIDE] */
    uint32_t *d_counters = nullptr; /* AVK_N_COUNTERS words the launches of a step coordinate through: avk_counters.h says which are whose */
    uint32_t *d_overflow = nullptr, *d_overflow2 = nullptr, *d_overflow3 = nullptr, *d_overflow4 = nullptr;
    uint32_t *d_notwide = nullptr;   /* [n + 1] class C records that are not avk_wide.inl's, then their number (avk_notwide_list_kernel, once per batch) */
    bool notwide_ready = false;
    uint32_t *d_overflow8 = nullptr; /* what the second, large-LDS launch of avk_wide.inl over class C's leftovers could not take either */
    uint32_t *d_overflow5 = nullptr, *d_overflow6 = nullptr, *d_overflow7 = nullptr; /* what the launches of avk_wide.inl could not take: of class C, of the three-call lane class's hand-backs, of the other lane classes' */
    avk::WorkPlan plan;
    uint32_t *d_fast = nullptr; /* fast records of the lane-per-region kernel (avk_dev_types.h), tiles of 64 */
    uint64_t fast_word_base[AVK_FAST_CLASSES] = {0}; /* first word of the class's tiles in d_fast */
    uint32_t fast_tiles[AVK_FAST_CLASSES] = {0};
    avk_compare_config last_cfg = {50, 0, 0}; /* the configuration of the last run (the capacity retry of avk_results_download repeats it) */
    uint32_t last_mode = 0;
    bool has_run = false;
    bool bp_valid = false; /* d_bp holds the groups of the last run (it ran in compare mode with emit_bp_groups) */
    bool scratch_clean = false; /* partial tallies and counters are zero */
    bool with_gm = true;
    /* device-packed batches (avk_devpack_host.inl): every buffer comes from the context's pool; `host` stays empty unless the capacity retry or
     * the sequence outputs ask for it (materialize_host_view) */
    bool dev_packed = false;
    std::vector<void *> pooled;
    uint64_t *d_in_t_off = nullptr, *d_in_q_off = nullptr; /* the caller's t_off / q_off / t_cnt / q_cnt: dp_unpack scatters the per-call outputs with them */
    uint32_t *d_in_t_cnt = nullptr, *d_in_q_cnt = nullptr, *d_voff = nullptr;
    const uint64_t *d_pk_voff = nullptr; /* a compare batch read from its packed source (DpIn::pk_*): these three stand in for the four arrays above */
    const uint8_t *d_pk_tc = nullptr, *d_pk_qc = nullptr;
    avk::dp::DpArgs dp_args; /* the packer's arguments: the writers of region records run again for the regions a launch turns out to need */
    avk::dp::DpArgs *d_dp_args = nullptr; /* the same in device memory (AvkKernelArgs::lazy_dp) */
    uint32_t lazy_from = 0;               /* first work-order index without a record (the lane classes' segment) */
    uint32_t *d_bp_off = nullptr, *d_bp = nullptr; /* compact per-region BASEPAIR groups: first group of a region (caller order), the groups (allocated when a run asks for them) */
    uint64_t n_bp_groups = 0;
    uint64_t *d_m_in_off = nullptr;       /* merge batches (avk_merge_batch): the MultiRegions' in_off / in_cnt and the calls' zygosities, for the classification kernel */
    uint32_t *d_m_in_cnt = nullptr;
    uint8_t *d_in_zyg = nullptr;
    uint8_t *d_in_type = nullptr;         /* ... and their types, for the count kernel (avk_mergecount.inl) */
    uint64_t n_multi = 0;
    uint32_t m_inputs = 0;
    uint64_t v_lo = 0, v_hi = 0;          /* the calls the batch's regions own: results are copied back for this range of the caller's arrays only */
    bool var_dense = false;               /* every call of the range is owned by a region of the batch */
    int64_t big_bytes_eff = 0;            /* shared big slices of this batch's launches when the packer predicts regions beyond the largest bucket (0: the option big_ws_bytes) */
    int64_t ws_bytes_eff = 0;             /* per-wave HBM slice of this batch's launches when the packer's prediction asks for more than the option ws_bytes_per_wave (0: the option) */
    bool records_full = false; /* every region has its AvkDevRegion + blob (false: only the regions outside the lane classes, until a launch asks for more) */
};

/* the interval sets of a stratified job, resident in HBM (avk_strata_upload; the layout of avk_strata.inl) */
/* the batches submitted with a handle and not yet waited for (avk_compare_packed_submit_strata), and the streams their mask passes — the only readers of the
 * trees — were queued on.  Shared by the handle and those tickets, so a ticket never looks at a handle that may have been freed. */
struct StrataUse {
    uint32_t in_flight = 0;
    std::vector<hipStream_t> streams;
};
struct avk_strata {
    avk_ctx *ctx = nullptr;
    uint32_t n_labels = 0, n_contigs = 0; /* n_labels: ALL labels, the BED labels then the context labels */
    uint32_t n_bed_labels = 0;            /* the labels the trees answer for */
    uint32_t n_ctx_labels = 0;            /* the sequence-context labels behind them (avk_context.inl); 0: the handle queues no context kernel */
    avk::cx::CxSpec spec{};
    uint64_t n_intervals = 0;
    uint64_t *d_tree_off = nullptr;
    uint32_t *d_start = nullptr, *d_end_max = nullptr;
    std::shared_ptr<StrataUse> use = std::make_shared<StrataUse>();
};

namespace {

int fail(avk_ctx *ctx, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf;
    else {
        std::lock_guard<std::mutex> lk(g_create_mutex);
        g_create_error = buf;
    }
    return code;
}

#define AVK_HIP(ctx, call)                                                                                  \
    do {                                                                                                     \
        hipError_t e_ = (call);                                                                              \
        if (e_ != hipSuccess)                                                                                \
            return fail(ctx, e_ == hipErrorOutOfMemory ? AVK_E_OOM : AVK_E_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)

template <typename T> int dev_alloc(avk_ctx *ctx, T **p, size_t count) {
    *p = nullptr;
    size_t bytes = count * sizeof(T);
    if (bytes == 0) bytes = 16;
    AVK_HIP(ctx, hipMalloc((void **)p, bytes));
    return 0;
}

void free_batch_buffers(avk_dev_batch *db) {
    if (db->dev_packed) return; /* pooled buffers: release_pooled */
    void *ptrs[] = {db->d_regions, db->d_blob, db->d_region_out, db->d_gm, db->d_var_out,
                    db->d_seq, db->d_seqlen, db->d_tally, db->d_partials, db->d_counters, db->d_overflow, db->d_overflow2, db->d_overflow3, db->d_overflow4, db->d_overflow5, db->d_overflow6, db->d_overflow7, db->d_overflow8, db->d_notwide, db->d_fast,
                    db->d_bp_off, db->d_bp};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
}

} // namespace

/* What one call wants of the functions below it, handed down by argument: the context holds options and resources, nothing that lasts for one call only. */
struct StrataJob;
struct LabelFix;
struct CallSpec {
    bool emit_gm = true, emit_bp = false;                /* what the kernels write for this batch: per-region metric blocks, compact BASEPAIR groups */
    hipStream_t up_stream = nullptr, up_side = nullptr;  /* the upload's streams; NULL: the context's stream and lane_stream4 (a submitted batch packs on streams of its own) */
    StrataJob *strata = nullptr;                         /* the packer's region passes also run the batch's containment pass (avk_compare_packed_strata: masks and the
                                                          * lists' size; avk_compare_packed_submit_strata: the masks alone) */
    LabelFix *label_fix = nullptr;                       /* the capacity retry of the download adds the repaired regions' blocks to the labels' sums */
};
/* the resident entry points: the options as they are at the time of the call */
static CallSpec call_spec(const avk_ctx *ctx) {
    CallSpec spec;
    spec.emit_gm = ctx->emit_group_metrics != 0, spec.emit_bp = ctx->emit_bp_groups != 0;
    return spec;
}
/* the one-call forms: per-region metric blocks only when the caller has an array for them, the groups when it has a place for them — or the call reads them itself
 * (need_bp: the label kernel, the shared spill list of a split call) */
static CallSpec call_spec(const avk_ctx *ctx, const avk_result_batch *out, bool need_bp) {
    CallSpec spec = call_spec(ctx);
    if (!out->group_metrics) spec.emit_gm = false;
    if (need_bp || ((out->bp_off || (out->bp_packed && out->bp_spilled)) && out->bp_groups)) spec.emit_bp = true;
    return spec;
}

#include "avk_devpack_host.inl"
#include "avk_upload.inl"

extern "C" {

const char *avk_version(void) { return "aardvark_amd 0.1 (gfx950)"; }
#ifndef AVK_SOURCE_HASH
#define AVK_SOURCE_HASH "unknown"
#endif
const char *avk_source_hash(void) { return AVK_SOURCE_HASH; }

uint64_t avk_edit_distance(const uint8_t *a, uint64_t a_len, const uint8_t *b, uint64_t b_len) { return avk::host_edit_distance(a, a_len, b, b_len); }

const char *avk_last_error(const avk_ctx *ctx) {
    if (ctx) return ctx->err.c_str();
    std::lock_guard<std::mutex> lk(g_create_mutex);
    return g_create_error.c_str();
}

/* the streams of the folded step plan: at context creation when the process has few hardware queues, else when a step first asks for them (option step_queues=4) */
static hipError_t ensure_fold_streams(avk_ctx *ctx) {
    for (hipStream_t &st : ctx->fold_stream)
        if (!st) {
            const hipError_t e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
            if (e != hipSuccess) return e;
        }
    return hipSuccess;
}

int avk_ctx_create(int device_id, avk_ctx **out) {
    if (!out) return AVK_E_ARG;
    *out = nullptr;
    /* six streams side by side need hardware queues of their own (the runtime's default is 4 and streams that share one run in turn);
     * read by the runtime when it initialises, so this helps when this is the process's first HIP call; the caller's setting wins (with fewer than eight queues
     * the step folds its chains onto four streams: below) */
    setenv("GPU_MAX_HW_QUEUES", "24", 0); /* 8 are enough for this library alone; with a communicator (RCCL) in the process 8 make the step 6.0 ms instead of 3.8 */
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) return fail(nullptr, AVK_E_HIP, "no HIP device available (%s)", e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    if (device_id < 0 || device_id >= n) return fail(nullptr, AVK_E_ARG, "device %d out of range (have %d)", device_id, n);
    avk_ctx *ctx = new avk_ctx();
    ctx->device = device_id;
    e = hipSetDevice(device_id);
    if (e != hipSuccess) {
        delete ctx;
        return fail(nullptr, AVK_E_HIP, "hipSetDevice failed: %s", hipGetErrorString(e));
    }
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, device_id);
    if (e != hipSuccess) {
        delete ctx;
        return fail(nullptr, AVK_E_HIP, "hipGetDeviceProperties failed: %s", hipGetErrorString(e));
    }
    ctx->n_cus = prop.multiProcessorCount;
    if (const char *e = getenv("AVK_COPY_BLOCKS")) ctx->copy_blocks_per_cu = atoi(e) > 0 ? atoi(e) : ctx->copy_blocks_per_cu;
    if (const char *e = getenv("AVK_WIDE_BLOCKS")) ctx->wide_blocks = atoi(e) > 0 ? atoi(e) : ctx->wide_blocks;
    if (hipStreamCreate(&ctx->stream) != hipSuccess) {
        delete ctx;
        return fail(nullptr, AVK_E_HIP, "hipStreamCreate failed");
    }
    ctx->own_stream = true;
    { /* the step's plan, by the hardware queues the runtime will see (the variable as it stands after the setenv above; not a number: a stream per chain).  The folded
       * plan's three streams are made directly behind the context's own, ahead of every other stream, so that the four take the process's first four queues
       * (profiles/step_four_queues.txt has the queue ids of a trace); AVK_STREAM_ORDER below does not place them */
        const char *q = getenv("GPU_MAX_HW_QUEUES");
        const int nq = q ? atoi(q) : 0;
        ctx->step_folded_auto = nq > 0 && nq < AVK_STEP_QUEUES_WIDE;
        if (ctx->step_folded_auto && ensure_fold_streams(ctx) != hipSuccess) {
            avk_ctx_destroy(ctx);
            return fail(nullptr, AVK_E_HIP, "hipStreamCreate failed");
        }
    }
    if (hipEventCreate(&ctx->ev0) != hipSuccess || hipEventCreate(&ctx->ev1) != hipSuccess || hipEventCreate(&ctx->evk1) != hipSuccess ||
        hipEventCreate(&ctx->ev_lane) != hipSuccess ||
        /* the buffer pool's fence exists from the start: a resident upload that releases its temporaries in stream order BEFORE the first asynchronous submit must be
         * able to record it (upload_device_packed), or the first packing on pack_stream could be handed buffers that queued kernels still read */
        hipEventCreateWithFlags(&ctx->ev_pool_fence, hipEventDisableTiming) != hipSuccess) {
        avk_ctx_destroy(ctx);
        return fail(nullptr, AVK_E_HIP, "hipEventCreate failed");
    }
    /* the solo launches get streams of the highest priority: they are the critical path, and HIP never folds streams of
     * different priorities onto one hardware queue (with a communicator library in the process the default-priority streams
     * of a process share queues, and a shared queue would serialise the solo launches with the bulk) */
    int prio_low = 0, prio_high = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_low, &prio_high);
    { /* the side and lane streams run at the default priority: with hardware queues of their own (GPU_MAX_HW_QUEUES >= 8) a high priority changes
       * nothing (4.94 / 4.98 ms per whole-genome step), with the runtime's default of 4 queues it costs 0.9 ms (7.0 / 7.9 ms);
       * AVK_STREAM_PRIORITY=high brings it back for experiments */
        const char *pe = getenv("AVK_STREAM_PRIORITY");
        if (!pe || strcmp(pe, "high") != 0) prio_high = 0;
    }
    const unsigned evf = getenv("AVK_TIMING") ? hipEventDefault : hipEventDisableTiming; /* the events that end the launch chains can be read when the stage timing is on */
    /* The runtime hands streams their hardware queues in the order they are made, and which launches share a queue's pipe shows in the step: streams that nothing is
     * ever queued on, made between the others, move a shard's resident step between 1.05 and 1.64 ms and a genome's between 2.38 and 2.95 (profiles/r05_stream_order.txt,
     * profiles/r06_stream_order.txt: a local search over the order, every candidate in fresh processes).  AVK_STREAM_ORDER: the order the seven side streams are made in,
     * a letter each — s side, t side2, w wide, a b c d the four lane streams, x a stream nothing is ever queued on; i o p q: the copy-in, copy-out, packing and
     * packing-side streams of the asynchronous calls (made at the first submit when the order does not name them). */
    const char *order = getenv("AVK_STREAM_ORDER") ? getenv("AVK_STREAM_ORDER") : AVK_STREAM_ORDER_DEFAULT;
    int n_spare = 0;
    bool ok = true;
    for (const char *o = order; *o && ok; ++o) {
        hipStream_t *st = *o == 's' ? &ctx->side_stream : *o == 't' ? &ctx->side_stream2 : *o == 'w' ? &ctx->wide_stream : *o == 'a' ? &ctx->lane_stream : *o == 'b' ? &ctx->lane_stream2 :
                          *o == 'c' ? &ctx->lane_stream3 : *o == 'd' ? &ctx->lane_stream4 : *o == 'i' ? &ctx->copy_in_stream : *o == 'o' ? &ctx->copy_out_stream :
                          *o == 'p' ? &ctx->pack_stream : *o == 'q' ? &ctx->pack_side_stream : (*o == 'x' && n_spare < 16) ? &ctx->spare_stream[n_spare++] : nullptr;
        if (st && !*st) ok = hipStreamCreateWithPriority(st, hipStreamNonBlocking, prio_high) == hipSuccess;
    }
    /* the placeholders have done their work once the others exist: the streams made behind them keep their place, and a process that held on to four idle streams
     * pushed a second process on the same GPU over the number of hardware queues the scheduler maps at a time — the tool's solve stage 0.02 -> 0.10-0.21 s beside
     * bench.py's own context (profiles/r06_stream_order.txt).  AVK_KEEP_SPARES=1 keeps them (to reproduce that). */
    ctx->n_placeholders = n_spare;
    if (!getenv("AVK_KEEP_SPARES"))
        for (int k = 0; k < n_spare; ++k) {
            if (ctx->spare_stream[k]) (void)hipStreamDestroy(ctx->spare_stream[k]);
            ctx->spare_stream[k] = nullptr;
        }
    hipStream_t *all[7] = {&ctx->side_stream, &ctx->side_stream2, &ctx->wide_stream, &ctx->lane_stream, &ctx->lane_stream2, &ctx->lane_stream3, &ctx->lane_stream4};
    for (hipStream_t *st : all) /* (a letter the order left out) */
        if (ok && !*st) ok = hipStreamCreateWithPriority(st, hipStreamNonBlocking, prio_high) == hipSuccess;
    for (hipEvent_t &ev : ctx->ev_end)
        if (ok) ok = hipEventCreateWithFlags(&ev, evf) == hipSuccess;
    if (!ok ||
        hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->ev_hb[0], hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&ctx->ev_hb[1], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->ev_hb[2], hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&ctx->ev_hb[3], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->ev_hb[4], hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&ctx->ev_hb[5], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->ev_hb[6], hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&ctx->ev_hb[7], hipEventDisableTiming) != hipSuccess ||
        hipEventCreate(&ctx->ev_cp0) != hipSuccess || hipEventCreate(&ctx->ev_cp1) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->ev_copy_alleles, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->ev_copy_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->ev_copy_mid, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->ev_copy_join, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->ev_lane_fork, hipEventDisableTiming) != hipSuccess) {
        avk_ctx_destroy(ctx);
        return fail(nullptr, AVK_E_HIP, "cannot create the side streams / events of the context");
    }
    *out = ctx;
    return 0;
}

void avk_ctx_destroy(avk_ctx *ctx) {
    if (!ctx) return;
    {
        std::lock_guard<std::mutex> lock(ctx->reaper_mutex);
        if (ctx->reaper.joinable()) ctx->reaper.join();
    }
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    for (auto &sl : ctx->stage) { /* staging slots of the asynchronous boundary */
        if (sl.dev) (void)hipFree(sl.dev);
        if (sl.h_tally) (void)hipHostFree(sl.h_tally);
        if (sl.h_labels) (void)hipHostFree(sl.h_labels);
        if (sl.ev_in) (void)hipEventDestroy(sl.ev_in);
        if (sl.ev_unpacked) (void)hipEventDestroy(sl.ev_unpacked);
        if (sl.ev_done) (void)hipEventDestroy(sl.ev_done);
    }
    if (ctx->pack_stream) (void)hipStreamDestroy(ctx->pack_stream);
    if (ctx->pack_side_stream) (void)hipStreamDestroy(ctx->pack_side_stream);
    if (ctx->ev_packed) (void)hipEventDestroy(ctx->ev_packed);
    if (ctx->ev_pool_fence) (void)hipEventDestroy(ctx->ev_pool_fence);
    if (ctx->copy_in_stream) (void)hipStreamDestroy(ctx->copy_in_stream);
    if (ctx->copy_out_stream) (void)hipStreamDestroy(ctx->copy_out_stream);
    pool_destroy(ctx);
    if (ctx->d_contig_tab) (void)hipFree(ctx->d_contig_tab);
    if (ctx->d_ref) (void)hipFree(ctx->d_ref);
    if (ctx->d_ref2b) (void)hipFree(ctx->d_ref2b);
    if (ctx->d_refexc) (void)hipFree(ctx->d_refexc);
    if (ctx->d_ws) (void)hipFree(ctx->d_ws);
    if (ctx->d_big) (void)hipFree(ctx->d_big);
    for (hipEvent_t &t : ctx->ev_tl)
        if (t) (void)hipEventDestroy(t);
    for (hipEvent_t &t : ctx->ev_pack_group)
        if (t) (void)hipEventDestroy(t);
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev_lab0) (void)hipEventDestroy(ctx->ev_lab0);
    if (ctx->ev_lab1) (void)hipEventDestroy(ctx->ev_lab1);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    if (ctx->evk1) (void)hipEventDestroy(ctx->evk1);
    if (ctx->ev_lane) (void)hipEventDestroy(ctx->ev_lane);
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    if (ctx->d_pair_tab) (void)hipFree(ctx->d_pair_tab);
    if (ctx->d_pair_aux) (void)hipFree(ctx->d_pair_aux);
    if (ctx->ev_lane_fork) (void)hipEventDestroy(ctx->ev_lane_fork);
    if (ctx->lane_stream) (void)hipStreamDestroy(ctx->lane_stream);
    if (ctx->lane_stream2) (void)hipStreamDestroy(ctx->lane_stream2);
    for (hipEvent_t e : ctx->ev_end)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : ctx->ev_hb)
        if (e) (void)hipEventDestroy(e);
    if (ctx->ev_cp0) (void)hipEventDestroy(ctx->ev_cp0);
    if (ctx->ev_cp1) (void)hipEventDestroy(ctx->ev_cp1);
    if (ctx->ev_copy_alleles) (void)hipEventDestroy(ctx->ev_copy_alleles);
    if (ctx->ev_copy_fork) (void)hipEventDestroy(ctx->ev_copy_fork);
    if (ctx->ev_copy_mid) (void)hipEventDestroy(ctx->ev_copy_mid);
    if (ctx->ev_copy_join) (void)hipEventDestroy(ctx->ev_copy_join);
    if (ctx->lane_stream4) (void)hipStreamDestroy(ctx->lane_stream4);
    if (ctx->lane_stream3) (void)hipStreamDestroy(ctx->lane_stream3);
    if (ctx->side_stream) (void)hipStreamDestroy(ctx->side_stream);
    if (ctx->side_stream2) (void)hipStreamDestroy(ctx->side_stream2);
    if (ctx->wide_stream) (void)hipStreamDestroy(ctx->wide_stream);
    for (hipStream_t fs : ctx->fold_stream)
        if (fs) (void)hipStreamDestroy(fs);
    for (hipStream_t sp : ctx->spare_stream)
        if (sp) (void)hipStreamDestroy(sp);
    if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

int avk_ctx_set_stream(avk_ctx *ctx, void *hip_stream) {
    if (!ctx) return AVK_E_ARG;
    (void)hipSetDevice(ctx->device);
    /* the buffer pool and the bounce buffer hand memory out again in the order of ONE stream: whatever the previous stream still has queued (the writers of an
     * upload's temporaries, say) is finished before another stream may be given the same buffers — also when the previous stream was the caller's */
    if (ctx->stream != (hipStream_t)hip_stream) {
        const hipError_t e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) {
            /* a caller's stream that is gone already (the header asks for it to be alive; the handle must not stay installed either way): whatever was queued on the
             * device is finished instead, and the switch goes through */
            (void)hipGetLastError();
            if (ctx->own_stream) return fail(ctx, AVK_E_HIP, "hipStreamSynchronize: %s", hipGetErrorString(e));
            AVK_HIP(ctx, hipDeviceSynchronize());
        }
    }
    if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    ctx->stream = (hipStream_t)hip_stream;
    ctx->own_stream = false;
    return 0;
}

int avk_ctx_set_option(avk_ctx *ctx, const char *name, int64_t value) {
    if (!ctx || !name) return AVK_E_ARG;
    std::string n(name);
    if (n == "lds_bytes_per_wave") {
        if (value < 0 || value > 40 * 1024) return fail(ctx, AVK_E_ARG, "lds_bytes_per_wave must be in [0, 40960]");
        ctx->lds_bytes_per_wave = value & ~15ll;
    } else if (n == "lds2_bytes_per_wave") {
        if (value < 0 || value > 40 * 1024) return fail(ctx, AVK_E_ARG, "lds2_bytes_per_wave must be in [0, 40960]");
        ctx->lds2_bytes_per_wave = value & ~15ll;
    } else if (n == "lds2_ed_cap") {
        if (value < 1 || value > 4096) return fail(ctx, AVK_E_ARG, "lds2_ed_cap must be in [1, 4096]");
        ctx->lds2_ed_cap = value;
    } else if (n == "lds_ed_cap") {
        if (value < 1 || value > 4096) return fail(ctx, AVK_E_ARG, "lds_ed_cap must be in [1, 4096]");
        ctx->lds_ed_cap = value;
    } else if (n == "solo_min_variants") {
        if (value < 0) return fail(ctx, AVK_E_ARG, "solo_min_variants must not be negative");
        ctx->solo_min_variants = value;
    } else if (n == "accumulate_tally") {
        ctx->accumulate_tally = value ? 1 : 0;
    } else if (n == "lds_escalation") {
        ctx->lds_escalation = value ? 1 : 0;
    } else if (n == "class_c_below") {
        if (value < 0) return fail(ctx, AVK_E_ARG, "class_c_below must not be negative");
        ctx->class_c_below = value;
    } else if (n == "class_c_nodes_x2") {
        if (value < 1 || value > 1000) return fail(ctx, AVK_E_ARG, "class_c_nodes_x2 must be in [1, 1000]");
        ctx->class_c_nodes_x2 = value;
    } else if (n == "static_pct") {
        if (value < 0 || value > 100) return fail(ctx, AVK_E_ARG, "static_pct must be in [0, 100]");
        ctx->static_pct = value;
    } else if (n == "claim") {
        if (value < 1 || value > 64) return fail(ctx, AVK_E_ARG, "claim must be in [1, 64]");
        ctx->claim = value;
    } else if (n == "step_queues") {
        if (value != 0 && value != AVK_STEP_SLOTS_FOLDED && value != AVK_STEP_QUEUES_WIDE) return fail(ctx, AVK_E_ARG, "step_queues must be 0 (by GPU_MAX_HW_QUEUES), 4 (the folded plan) or 8 (a stream per chain)");
        ctx->step_queues = value;
    } else if (n == "wide_kernel") {
        ctx->wide_kernel = value ? 1 : 0;
    } else if (n == "wide_lds_bytes") {
        if (value < 8 * 1024 || value > 64 * 1024) return fail(ctx, AVK_E_ARG, "wide_lds_bytes must be in [8192, 65536]");
        ctx->wide_lds_bytes = value & ~15ll;
    } else if (n == "wide_retry_lds_bytes") {
        if (value < 0 || value > 64 * 1024) return fail(ctx, AVK_E_ARG, "wide_retry_lds_bytes must be in [0, 65536]");
        ctx->wide_retry_lds_bytes = value & ~15ll;
    } else if (n == "waves_per_cu") {
        if (value < 1 || value > 32) return fail(ctx, AVK_E_ARG, "waves_per_cu must be in [1, 32]");
        ctx->waves_per_cu = value;
    } else if (n == "ws_bytes_per_wave") {
        if (value < 0) return fail(ctx, AVK_E_ARG, "ws_bytes_per_wave must be >= 0");
        ctx->ws_bytes_per_wave = (value + 255) & ~255ll;
    } else if (n == "big_ws_bytes") {
        if (value < 0) return fail(ctx, AVK_E_ARG, "big_ws_bytes must be >= 0");
        ctx->big_ws_bytes = (value + 255) & ~255ll;
    } else if (n == "use_packed_reference") {
        ctx->use_packed_reference = value ? 1 : 0;
    } else if (n == "adaptive_ws") {
        ctx->adaptive_ws = value ? 1 : 0;
    } else if (n == "ws_budget_bytes") {
        if (value < (1ll << 30)) return fail(ctx, AVK_E_ARG, "ws_budget_bytes must be at least 1 GiB");
        ctx->ws_budget_bytes = value;
    } else if (n == "device_pack") {
        ctx->device_pack = value ? 1 : 0;
    } else if (n == "team_long_windows") {
        if (value < 0 || value > 2) return fail(ctx, AVK_E_ARG, "team_long_windows must be 0, 1 or 2 (2: the owner wave takes every job itself, a diagnostic)");
        ctx->team_long_windows = value;
    } else if (n == "team_head_regions") {
        if (value < 0 || value > 1024) return fail(ctx, AVK_E_ARG, "team_head_regions must be 0..1024");
        ctx->team_head_regions = value;
    } else if (n == "split_parts") {
        if (value < 1 || value > 4) return fail(ctx, AVK_E_ARG, "split_parts must be 1..4");
        ctx->split_parts = value;
    } else if (n == "kernel_copies") {
        if (value < 0 || value > 2) return fail(ctx, AVK_E_ARG, "kernel_copies must be 0 (engines), 1 (by measurement) or 2 (kernel)");
        ctx->kernel_copies = value;
    } else if (n == "packed_source") {
        ctx->packed_source = value ? 1 : 0;
    } else if (n == "pack_chunks") {
        if (value != 0 && (value < 2 || value > avk::pc::PC_MAX_GROUPS)) return fail(ctx, AVK_E_ARG, "pack_chunks must be 0 (one region launch behind the copies) or 2..8 groups");
        ctx->pack_chunks = value;
    } else if (n == "pack_queue_early") {
        ctx->pack_queue_early = value ? 1 : 0;
    } else if (n == "pack_chunk_floor") {
        if (value < 0) return fail(ctx, AVK_E_ARG, "pack_chunk_floor must not be negative");
        ctx->pack_chunk_floor = value;
    } else if (n == "emit_bp_groups") {
        ctx->emit_bp_groups = value ? 1 : 0;
    } else if (n == "emit_group_metrics") {
        ctx->emit_group_metrics = value ? 1 : 0;
    } else if (n == "capacity_retry") {
        ctx->capacity_retry = value ? 1 : 0;
    } else if (n == "lane_kernel") {
        ctx->lane_kernel = value ? 1 : 0;
    } else if (n == "lane_min_regions") {
        if (value < 0) return fail(ctx, AVK_E_ARG, "lane_min_regions must not be negative");
        ctx->lane_min_regions = value;
    } else if (n == "lane_width_one" || n == "lane_width_two" || n == "lane_width_three") {
        if (value != 64 && value != 32 && value != 16 && value != 8 && value != 4 && value != 2 && value != 1) return fail(ctx, AVK_E_ARG, "%s must be 64, 32, 16, 8, 4, 2 or 1", name);
        (n == "lane_width_one" ? ctx->lane_width_one : (n == "lane_width_two" ? ctx->lane_width_two : ctx->lane_width_three)) = value;
    } else if (n == "lane_head_width") {
        if (value != 0 && value != 64 && value != 32 && value != 16 && value != 8 && value != 4) return fail(ctx, AVK_E_ARG, "lane_head_width must be 0, 64, 32, 16, 8 or 4");
        ctx->lane_head_width = value;
    } else if (n == "hbm_ed_cap") {
        if (value < 0 || value > 1000000) return fail(ctx, AVK_E_ARG, "hbm_ed_cap must be 0..1000000");
        ctx->hbm_ed_cap = value;
    } else if (n == "lane_pairs") {
        ctx->lane_pairs = value ? 1 : 0;
    } else if (n == "lane_min_batch") {
        if (value < 0) return fail(ctx, AVK_E_ARG, "lane_min_batch must not be negative");
        ctx->lane_min_batch = value;
    } else if (n == "lane_node_cap") {
        if (value < 8 || value > 250) return fail(ctx, AVK_E_ARG, "lane_node_cap must be 8..250");
        ctx->lane_node_cap = value;
    } else if (n == "lane_quad") {
        ctx->lane_quad = value ? 1 : 0;
    } else
        return fail(ctx, AVK_E_ARG, "unknown option '%s'", name);
    return 0;
}

int avk_ref_upload(avk_ctx *ctx, uint32_t n_contigs, const uint8_t *const *seqs, const uint64_t *lens) {
    if (!ctx || (n_contigs && (!seqs || !lens))) return AVK_E_ARG;
    AVK_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->d_ref) {
        AVK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        (void)hipFree(ctx->d_ref);
        ctx->d_ref = nullptr;
        if (ctx->d_ref2b) (void)hipFree(ctx->d_ref2b);
        if (ctx->d_refexc) (void)hipFree(ctx->d_refexc);
        ctx->d_ref2b = ctx->d_refexc = nullptr;
    }
    ctx->contig_base.assign(n_contigs, 0);
    ctx->contig_len.assign(n_contigs, 0);
    uint64_t total = 0;
    for (uint32_t c = 0; c < n_contigs; ++c) {
        ctx->contig_base[c] = total;
        ctx->contig_len[c] = lens[c];
        total += lens[c];
    }
    /* any failure leaves the context WITHOUT a reference (later calls then fail with "avk_ref_upload has not been called") */
    hipError_t e = hipMalloc((void **)&ctx->d_ref, total + 64);
    for (uint32_t c = 0; c < n_contigs && e == hipSuccess; ++c)
        if (lens[c]) e = hipMemcpyAsync(ctx->d_ref + ctx->contig_base[c], seqs[c], lens[c], hipMemcpyHostToDevice, ctx->stream);
    const uint64_t n_words = (total + 15) >> 4;
    if (ctx->d_contig_tab) (void)hipFree(ctx->d_contig_tab);
    ctx->d_contig_tab = nullptr;
    if (e == hipSuccess) e = hipMalloc((void **)&ctx->d_contig_tab, ((size_t)2 * n_contigs + 2) * sizeof(uint64_t));
    if (e == hipSuccess && n_contigs) e = hipMemcpyAsync(ctx->d_contig_tab, ctx->contig_base.data(), (size_t)n_contigs * 8, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess && n_contigs) e = hipMemcpyAsync(ctx->d_contig_tab + n_contigs, ctx->contig_len.data(), (size_t)n_contigs * 8, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMalloc((void **)&ctx->d_ref2b, (n_words + 80) * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&ctx->d_refexc, ((n_words >> 5) + 8) * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemsetAsync(ctx->d_ref2b, 0, (n_words + 80) * sizeof(uint32_t), ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(ctx->d_refexc, 0, ((n_words >> 5) + 8) * sizeof(uint32_t), ctx->stream);
    if (e == hipSuccess) {
        const uint64_t threads = ((n_words + 63) / 64 + 1) * 64;
        hipLaunchKernelGGL(avk_pack_reference, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, ctx->stream, ctx->d_ref, total, ctx->d_ref2b, ctx->d_refexc);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(ctx->stream);
        if (ctx->d_ref) (void)hipFree(ctx->d_ref);
        if (ctx->d_ref2b) (void)hipFree(ctx->d_ref2b);
        if (ctx->d_refexc) (void)hipFree(ctx->d_refexc);
        if (ctx->d_contig_tab) (void)hipFree(ctx->d_contig_tab);
        ctx->d_contig_tab = nullptr;
        ctx->d_ref = nullptr;
        ctx->d_ref2b = ctx->d_refexc = nullptr;
        ctx->contig_base.clear();
        ctx->contig_len.clear();
        return fail(ctx, e == hipErrorOutOfMemory ? AVK_E_OOM : AVK_E_HIP, "reference upload failed: %s", hipGetErrorString(e));
    }
    return 0;
}

uint32_t avk_seq_stride(const avk_region_batch *batch, uint64_t r) {
    if (!batch || r >= batch->n_regions) return 0;
    return avk::seq_stride_of(batch, r);
}

/* DESIGN.md "algorithmic bytes per region" (SURVEY.md 8d): in — 2-bit window, 12 B record and 2-bit alleles per call, 16 B header; out — 16 B
 * record, 2 B per call and, when the run writes per-region BASEPAIR groups (with_groups), 16 B for the joint group and 16 B per call type present */
uint64_t avk_algorithmic_bytes_ex(const avk_region_batch *b, int with_groups) {
    if (!b) return 0;
    uint64_t total = 0;
    for (uint64_t r = 0; r < b->n_regions; ++r) {
        uint64_t L = b->end[r] > b->start[r] ? b->end[r] - b->start[r] : 0;
        uint64_t bytes = (L + 3) / 4 + 16 + 16 + (with_groups ? 16 : 0);
        uint32_t types = 0;
        for (int side = 0; side < 2; ++side) {
            uint64_t off = side == 0 ? b->t_off[r] : b->q_off[r];
            uint32_t cnt = side == 0 ? b->t_cnt[r] : b->q_cnt[r];
            if (off > b->n_variants || cnt > b->n_variants - off) continue;
            for (uint32_t i = 0; i < cnt; ++i) {
                uint64_t v = off + i;
                bytes += 12 + (b->a0_len[v] + 3) / 4 + (b->a1_len[v] + 3) / 4 + 2;
                types |= 1u << (b->var_type[v] & 15);
            }
        }
        if (with_groups) bytes += 16ull * (uint64_t)__builtin_popcount(types);
        total += bytes;
    }
    return total;
}
uint64_t avk_algorithmic_bytes(const avk_region_batch *b) { return avk_algorithmic_bytes_ex(b, 1); }

/* the wide result arrays from the packed form (include/aardvark_amd.h) */
int avk_results_expand(const avk_region_batch *b, const avk_result_batch *packed, avk_result_batch *wide) {
    if (!b || !packed || !wide) return AVK_E_ARG;
    const bool want_region = wide->status || wide->ed_h1 || wide->ed_h2 || wide->n_optima || wide->type_present;
    const bool want_calls = wide->var_expected || wide->var_observed || wide->var_class || wide->var_zyg;
    if ((want_region && !packed->region_packed) || (want_calls && !packed->var_packed)) return AVK_E_ARG;
    if (!want_region && !want_calls) return 0;
    std::atomic<int> bad(0);
    const uint64_t n = b->n_regions, piece = 1u << 16, pieces = (n + piece - 1) / piece;
    std::atomic<uint64_t> next(0);
    AvkPool::get().run(pieces > 1 ? avk_host_threads() : 1, [&](unsigned) {
        for (;;) {
            const uint64_t p = next.fetch_add(1);
            if (p >= pieces) break;
            for (uint64_t r = p * piece; r < n && r < (p + 1) * piece; ++r) {
                uint32_t types = 0;
                for (int side = 0; side < 2; ++side) {
                    const uint64_t off = side == 0 ? b->t_off[r] : b->q_off[r];
                    const uint32_t cnt = side == 0 ? b->t_cnt[r] : b->q_cnt[r];
                    if (off > b->n_variants || cnt > b->n_variants - off) {
                        bad.store(1);
                        continue;
                    }
                    for (uint32_t i = 0; i < cnt; ++i) {
                        const uint64_t v = off + i;
                        if (b->var_type && b->var_type[v] < AVK_N_VARIANT_TYPES) types |= 1u << b->var_type[v];
                        if (!want_calls) continue;
                        const uint8_t x = packed->var_packed[v];
                        if (wide->var_expected) wide->var_expected[v] = avk_vp_expected(x);
                        if (wide->var_observed) wide->var_observed[v] = avk_vp_observed(x);
                        if (wide->var_class) wide->var_class[v] = avk_vp_class(x, side);
                        if (wide->var_zyg) wide->var_zyg[v] = avk_vp_zyg(x);
                    }
                }
                if (!want_region) continue;
                const uint64_t w = packed->region_packed[r];
                if (wide->status) wide->status[r] = avk_rp_status(w);
                if (wide->ed_h1) wide->ed_h1[r] = avk_rp_ed_h1(w);
                if (wide->ed_h2) wide->ed_h2[r] = avk_rp_ed_h2(w);
                if (wide->n_optima) wide->n_optima[r] = avk_rp_n_optima(w);
                if (wide->type_present) wide->type_present[r] = avk_rp_type_present(w, types);
            }
        }
    });
    return bad.load() ? AVK_E_ARG : 0;
}

/* GroupTypeMetrics of one region from its compact BASEPAIR groups and the per-call outputs (include/aardvark_amd.h) */
int avk_group_metrics_from_compact(const avk_region_batch *b, uint64_t r, const avk_result_batch *res, uint32_t *out) {
    const bool bp_packed = res && res->bp_packed && res->bp_spilled;
    if (!b || !res || !out || r >= b->n_regions || !((res->var_expected && res->var_observed) || res->var_packed) || !(res->bp_off || bp_packed) || !res->bp_groups) return AVK_E_ARG;
    const bool wide_calls = res->var_expected && res->var_observed; /* otherwise the packed bytes */
    memset(out, 0, sizeof(uint32_t) * AVK_N_GROUPS * AVK_N_FIELDS);
    uint32_t types = 0;
    uint64_t tot[2][1 + AVK_N_VARIANT_TYPES];
    memset(tot, 0, sizeof(tot));
    for (int side = 0; side < 2; ++side) {
        const uint64_t off = side == 0 ? b->t_off[r] : b->q_off[r];
        const uint32_t cnt = side == 0 ? b->t_cnt[r] : b->q_cnt[r];
        if (off > b->n_variants || cnt > b->n_variants - off) return AVK_E_ARG;
        for (uint32_t i = 0; i < cnt; ++i) {
            const uint64_t v = off + i;
            const uint32_t vt = b->var_type[v];
            if (vt >= AVK_N_VARIANT_TYPES) return AVK_E_ARG;
            types |= 1u << vt;
            const uint64_t w = avk::host_edit_distance(b->allele_bytes + b->a0_off[v], b->a0_len[v], b->allele_bytes + b->a1_off[v], b->a1_len[v]); /* Variant::alt_ed */
            /* the query entries are stored toggled (compare_benchmark.rs:109-123): scored as truth they expected var_observed and observed var_expected */
            const uint32_t ea = wide_calls ? res->var_expected[v] : avk_vp_expected(res->var_packed[v]), oa = wide_calls ? res->var_observed[v] : avk_vp_observed(res->var_packed[v]);
            const uint32_t exp = side == 0 ? ea : oa, obs = side == 0 ? oa : ea;
            const int f_gt_tp = side ? AVK_F_GT_QUERY_TP : AVK_F_GT_TRUTH_TP, f_gt_fn = side ? AVK_F_GT_QUERY_FP : AVK_F_GT_TRUTH_FN, f_gt_fn_gt = side ? AVK_F_GT_QUERY_FP_GT : AVK_F_GT_TRUTH_FN_GT;
            const int f_hap_tp = side ? AVK_F_HAP_QUERY_TP : AVK_F_HAP_TRUTH_TP, f_hap_fn = side ? AVK_F_HAP_QUERY_FP : AVK_F_HAP_TRUTH_FN;
            const int f_w_tp = side ? AVK_F_WHAP_QUERY_TP : AVK_F_WHAP_TRUTH_TP, f_w_fn = side ? AVK_F_WHAP_QUERY_FP : AVK_F_WHAP_TRUTH_FN;
            for (uint32_t g : {0u, 1u + vt}) { /* GroupMetrics::add_truth_zygosity (grouped_metrics.rs:183-227) on the joint group and the type's */
                uint32_t *G = out + g * AVK_N_FIELDS;
                G[f_hap_tp] += obs;
                G[f_hap_fn] += exp - obs;
                G[f_w_tp] += (uint32_t)(obs * w);
                G[f_w_fn] += (uint32_t)((exp - obs) * w);
                if (exp == obs) G[f_gt_tp] += 1;
                else {
                    G[f_gt_fn] += 1;
                    if (obs > 0) G[f_gt_fn_gt] += 1;
                }
            }
            const uint32_t z = b->var_zyg[v];
            const uint64_t cz = z == AVK_ZYG_HOM_ALT ? 2 : ((z >= AVK_ZYG_UNPHASED_HET && z <= AVK_ZYG_PHASED_HET10) ? 1 : 0);
            const uint64_t raw = b->var_raw_space ? b->var_raw_space[v] : (b->a0_len[v] > b->a1_len[v] ? b->a0_len[v] : b->a1_len[v]);
            tot[side][0] += cz * raw;
            tot[side][1 + vt] += cz * raw;
        }
    }
    /* BASEPAIR from the compact groups (joint, then the region's call types in type order); RECORD_BP from them and the totals (waffle_solver.rs:455-522) */
    uint32_t simple[4] = {0, 0, 0, 0}; /* the packed form's word: every group of the region is this one */
    uint32_t lo = 0, hi = 0;
    bool one_for_all = false;
    if (bp_packed) {
        const uint32_t w = res->bp_packed[r], n_groups = 1u + (uint32_t)__builtin_popcount(types);
        if (avk_bp_is_spilled(w)) {
            lo = avk_bp_spill_index(w), hi = lo + n_groups;
            if (hi > res->bp_spilled[0]) return AVK_E_ARG;
        } else {
            for (int i = 0; i < 4; ++i) simple[i] = avk_bp_counter(w, i);
            one_for_all = true, hi = n_groups;
        }
    } else
        lo = res->bp_off[r], hi = res->bp_off[r + 1];
    uint32_t k = lo;
    for (uint32_t left = 1u | (types << 1); left; left &= left - 1, ++k) {
        if (k >= hi) return AVK_E_ARG; /* the region owns no groups (it failed validation) or fewer than its call types */
        const uint32_t g = (uint32_t)__builtin_ctz(left);
        uint32_t *G = out + g * AVK_N_FIELDS;
        const uint32_t *bp = one_for_all ? simple : res->bp_groups + 4 * (size_t)k;
        for (int i = 0; i < 4; ++i) G[AVK_F_BP_TRUTH_TP + i] = bp[i];
        G[AVK_F_RBP_TRUTH_TP] = (uint32_t)(2 * tot[0][g] - bp[1]);
        G[AVK_F_RBP_TRUTH_FN] = bp[1];
        G[AVK_F_RBP_QUERY_TP] = (uint32_t)(2 * tot[1][g] - bp[3]);
        G[AVK_F_RBP_QUERY_FP] = bp[3];
    }
    return k == hi ? 0 : AVK_E_ARG;
}

static int upload_internal(avk_ctx *ctx, const CallSpec &spec, const avk_region_batch *batch, bool pairs_mode, avk_dev_batch **out) {
    if (!ctx || !batch || !out) return AVK_E_ARG;
    *out = nullptr;
    if (!ctx->d_ref) return fail(ctx, AVK_E_STATE, "avk_ref_upload has not been called");
    AVK_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->device_pack) return upload_device_packed(ctx, spec, UploadSource::of(batch, pairs_mode), nullptr, out);
    const bool timing = getenv("AVK_TIMING") != nullptr;
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    const auto t_start = now();
    avk_dev_batch *db = new avk_dev_batch();
    db->n_regions = batch->n_regions;
    db->n_variants_host = batch->n_variants;
    /* sequence slots are laid out by the library: prefix of 5 * stride */
    std::vector<uint64_t> seq_off(batch->n_regions);
    std::vector<uint32_t> seq_stride(batch->n_regions);
    uint64_t seq_total = 0;
    {
        const uint64_t nr = batch->n_regions;
        size_t nt = avk_usable_cpus();
        if (nt > 16) nt = 16;
        if (nt > nr / 65536 + 1) nt = (size_t)(nr / 65536 + 1);
        auto part = [&](size_t t) {
            for (uint64_t r = nr * t / nt; r < nr * (t + 1) / nt; ++r) seq_stride[r] = avk::seq_stride_of(batch, r);
        };
        std::vector<std::thread> pool;
        for (size_t t = 1; t < nt; ++t) pool.emplace_back(part, t);
        part(0);
        for (auto &th : pool) th.join();
    }
    for (uint64_t r = 0; r < batch->n_regions; ++r) {
        seq_off[r] = seq_total;
        seq_total += 5ull * seq_stride[r];
    }
    db->seq_total = seq_total;
    std::string err;
    int rc = avk::pack_batch(batch, ctx->contig_base, ctx->contig_len, seq_off.data(), seq_stride.data(), &db->host, &err, 0, (uint32_t)ctx->lane_max_est, ctx->lane_pairs != 0 && !pairs_mode, (uint32_t)ctx->het_search_min);
    if (rc) {
        delete db;
        return fail(ctx, rc, "%s", err.c_str());
    }
    const uint64_t n = db->n_regions, nv = db->host.variants.size();
    db->n_variants_dev = nv;
    const auto t_packed = now();
    if (pairs_mode) { /* solve_merge_region's pre-checks (merge_solver.rs:119-147, :211-223) */
        for (uint64_t r = 0; r < n; ++r) {
            AvkDevRegion &dr = db->host.regions[r];
            if ((dr.pre_status & 0xFFFFu) == AVK_ST_INVALID_INPUT) continue;
            if (db->host.zyg_flags[r] & 1) dr.pre_status = AVK_ST_BAD_ZYGOSITY;                           /* Unknown: delta computation bails */
            else if (db->host.delta_t[r] != db->host.delta_q[r]) dr.pre_status = AVK_PRE_SKIP_OK;        /* different net length: not exact, optimizer not run */
            else if (db->host.zyg_flags[r] & 2) dr.pre_status = AVK_ST_BAD_ZYGOSITY;                      /* optimizer would hit assert_eq! */
            else dr.pre_status = 0;
        }
    }
#define AVK_TRY(x)                \
    do {                          \
        int rc_ = (x);            \
        if (rc_) {                \
            free_batch_buffers(db); \
            delete db;            \
            return rc_;           \
        }                         \
    } while (0)
    AVK_TRY(dev_alloc(ctx, &db->d_regions, n));
    AVK_TRY(dev_alloc(ctx, &db->d_blob, db->host.blob.size()));
    AVK_TRY(dev_alloc(ctx, &db->d_region_out, n * 4));
    AVK_TRY(dev_alloc(ctx, &db->d_var_out, nv));
    AVK_TRY(dev_alloc(ctx, &db->d_seqlen, n * 5));
    AVK_TRY(dev_alloc(ctx, &db->d_tally, (size_t)AVK_TALLY_STRIDE));
    AVK_TRY(dev_alloc(ctx, &db->d_partials, (size_t)AVK_TALLY_STRIDE * AVK_TALLY_COPIES));
    AVK_TRY(dev_alloc(ctx, &db->d_counters, (size_t)AVK_N_COUNTERS));
    AVK_TRY(dev_alloc(ctx, &db->d_overflow, n + 1024));
    AVK_TRY(dev_alloc(ctx, &db->d_overflow2, n + 1));
    AVK_TRY(dev_alloc(ctx, &db->d_overflow3, 3 * (n + 1) + 1024)); /* (the lanes' hand-backs: a segment per chain, per head launch and for the looked-up pairs) */
    AVK_TRY(dev_alloc(ctx, &db->d_overflow4, n + 1));
    AVK_TRY(dev_alloc(ctx, &db->d_overflow5, n + 1));
    AVK_TRY(dev_alloc(ctx, &db->d_overflow6, n + 1));
    AVK_TRY(dev_alloc(ctx, &db->d_overflow7, n + 1));
    AVK_TRY(dev_alloc(ctx, &db->d_overflow8, n + 1));
    AVK_TRY(dev_alloc(ctx, &db->d_notwide, n + 2));
#undef AVK_TRY
    { /* compact BASEPAIR groups: 1 + the region's call types each (none for regions that fail validation), as the device packer counts them */
        std::vector<uint32_t> bp_off(n + 1, 0);
        for (uint64_t r = 0; r < n; ++r) {
            const uint32_t ps = db->host.regions[r].pre_status;
            bp_off[r + 1] = bp_off[r] + ((ps & 0xFFFFu) ? 0u : 1u + (uint32_t)__builtin_popcount(ps >> 16));
        }
        db->n_bp_groups = bp_off[n];
        hipError_t eb = hipMalloc((void **)&db->d_bp_off, (n + 2) * sizeof(uint32_t));
        if (eb == hipSuccess) eb = hipMemcpy(db->d_bp_off, bp_off.data(), (n + 1) * sizeof(uint32_t), hipMemcpyHostToDevice);
        if (eb != hipSuccess) {
            free_batch_buffers(db);
            delete db;
            return fail(ctx, AVK_E_HIP, "batch upload failed: %s", hipGetErrorString(eb));
        }
    }
    /* work order: the regions predicted to outgrow the small LDS slice first (solo waves take them), then the
     * rest; within each part the regions with the most variants (the expensive searches) are dealt first, so
     * they overlap with the bulk instead of forming the tail */
    const auto t_alloc = now();
    std::vector<uint32_t> order;
    db->plan = avk::plan_work_order(db->host, avk::bulk_slice_bytes((uint64_t)ctx->lds_bytes_per_wave), (uint32_t)ctx->lds_ed_cap, (uint64_t)ctx->lds2_bytes_per_wave,
                                    (uint32_t)ctx->lds2_ed_cap, pairs_mode && !ctx->pair_classes ? 0u : (uint32_t)ctx->solo_min_variants, 50, &order, (uint32_t)ctx->class_c_nodes_x2,
                                    ctx->lane_kernel && ctx->use_packed_reference && ctx->d_ref2b ? (uint64_t)ctx->lane_min_regions : 0xFFFFFFFFull, (uint32_t)ctx->lane_max_calls,
                                    (uint64_t)ctx->lane_min_batch, ctx->lane_stripe ? (uint32_t)ctx->lane_head_width : 0u, (uint32_t)ctx->lane_head_est, (uint32_t)ctx->het_search_min,
                                    (uint64_t)ctx->class_c_below);
    const auto t_plan = now();
    hipError_t e = hipSuccess;
    /* the records go up in work order: a wave reads record k of its launch's range, no index list in between */
    const avk::PodVec<AvkDevRegion> sorted = avk::regions_in_work_order(db->host, order);
    avk::PodVec<uint32_t> fast;
    if (db->plan.n_fast_total) {
        fast = avk::build_fast_records(db->host, order, db->plan, db->fast_word_base, db->fast_tiles);
        e = hipMalloc((void **)&db->d_fast, fast.size() * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMemcpyAsync(db->d_fast, fast.data(), fast.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream);
    }
    if (n && e == hipSuccess) e = hipMemcpyAsync(db->d_regions, sorted.data(), n * sizeof(AvkDevRegion), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(db->d_blob, db->host.blob.data(), db->host.blob.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        free_batch_buffers(db);
        delete db;
        return fail(ctx, AVK_E_HIP, "batch upload failed: %s", hipGetErrorString(e));
    }
    if (timing)
        fprintf(stderr, "avk upload: pack %.3f ms, alloc %.3f ms, plan %.3f ms, copy %.3f ms\n", ms(t_start, t_packed), ms(t_packed, t_alloc), ms(t_alloc, t_plan),
                ms(t_plan, now()));
    *out = db;
    return 0;
}

int avk_batch_upload(avk_ctx *ctx, const avk_region_batch *batch, avk_dev_batch **out) { return ctx ? upload_internal(ctx, call_spec(ctx), batch, false, out) : AVK_E_ARG; }

void avk_batch_free(avk_ctx *ctx, avk_dev_batch *db) {
    if (!db) return;
    if (ctx) {
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
    }
    if (ctx && db->dev_packed) { /* back to the context's pool: nothing to wait for */
        release_pooled(ctx, db);
        delete db;
        return;
    }
    /* a large batch holds a dozen device buffers and about a gigabyte of host records: releasing them takes 0.1 s, which a tool that
     * works through its batches one after the other should not wait for.  One release runs behind the caller at a time. */
    if (ctx && db->n_regions >= 65536) {
        std::lock_guard<std::mutex> lock(ctx->reaper_mutex);
        if (ctx->reaper.joinable()) ctx->reaper.join();
        const int device = ctx->device;
        ctx->reaper = std::thread([db, device] {
            (void)hipSetDevice(device);
            free_batch_buffers(db);
            delete db;
        });
        return;
    }
    free_batch_buffers(db);
    delete db;
}

/* the solver step: Step, run_internal, the lane launches' helpers, ensure_kernel_attrs, ensure_pair_table */
#include "avk_step.inl"

int avk_compare_resident(avk_ctx *ctx, avk_dev_batch *db, const avk_compare_config *cfg, void *tally_dev) {
    return ctx ? run_internal(ctx, call_spec(ctx), db, cfg, tally_dev, 0) : AVK_E_ARG;
}

#ifdef AVK_QUAD_WAVE_LOG
/* profiling build only (make quad-wave-log): the wave log of the quad launches, 6 x 4096 x 4 words; cleared by the call */
extern "C" int avk_debug_wave_log(unsigned long long *dst) {
    if (hipMemcpyFromSymbol(dst, HIP_SYMBOL(avk_wave_log_buf), sizeof(avk_wave_log_buf)) != hipSuccess) return AVK_E_HIP;
    std::vector<unsigned long long> z(sizeof(avk_wave_log_buf) / 8, 0);
    return hipMemcpyToSymbol(HIP_SYMBOL(avk_wave_log_buf), z.data(), sizeof(avk_wave_log_buf)) == hipSuccess ? 0 : AVK_E_HIP;
}
#endif

int avk_synchronize(avk_ctx *ctx) {
    if (!ctx) return AVK_E_ARG;
    AVK_HIP(ctx, hipSetDevice(ctx->device));
    AVK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

int avk_last_kernel_ms(avk_ctx *ctx, float *ms) {
    if (!ctx || !ms) return AVK_E_ARG;
    if (!ctx->ev_valid) return fail(ctx, AVK_E_STATE, "no launch has been timed yet");
    AVK_HIP(ctx, hipEventSynchronize(ctx->evk1));
    AVK_HIP(ctx, hipEventElapsedTime(ms, ctx->ev0, ctx->evk1));
    return 0;
}

int avk_last_lane_ms(avk_ctx *ctx, float *ms) {
    if (!ctx || !ms) return AVK_E_ARG;
    *ms = 0;
    if (!ctx->ev_valid) return fail(ctx, AVK_E_STATE, "no launch has been timed yet");
    if (!ctx->ev_lane_valid) return 0; /* the last call had no lane-kernel launches */
    AVK_HIP(ctx, hipEventSynchronize(ctx->ev_lane));
    AVK_HIP(ctx, hipEventElapsedTime(ms, ctx->ev0, ctx->ev_lane));
    return 0;
}

int avk_last_lane_solved(avk_ctx *ctx, uint64_t *count) {
    if (!ctx || !count) return AVK_E_ARG;
    *count = ctx->last_lane_solved;
    return 0;
}

int avk_last_region_launches(avk_ctx *ctx, uint64_t *count) {
    if (!ctx || !count) return AVK_E_ARG;
    *count = ctx->last_region_launches;
    return 0;
}

int avk_last_wide_solved(avk_ctx *ctx, uint64_t *count) {
    if (!ctx || !count) return AVK_E_ARG;
    *count = ctx->last_wide_solved;
    return 0;
}

int avk_last_solver_ms(avk_ctx *ctx, float *ms) {
    if (!ctx || !ms) return AVK_E_ARG;
    if (!ctx->ev_valid) return fail(ctx, AVK_E_STATE, "no launch has been timed yet");
    AVK_HIP(ctx, hipEventSynchronize(ctx->ev1));
    AVK_HIP(ctx, hipEventElapsedTime(ms, ctx->ev0, ctx->ev1));
    return 0;
}

/* profiling builds (-DAVK_PHASE_TIMING): summed s_memtime ticks per solver phase of the last download */
int avk_debug_phase_cycles(avk_ctx *ctx, uint64_t out[16]) {
    if (!ctx || !out) return AVK_E_ARG;
    memcpy(out, ctx->last_phase, sizeof(ctx->last_phase));
    return 0;
}

/* diagnostic: which of the context's streams still have work queued (caller's, two solo streams, two lane streams) and the batch's
 * device counters as they are NOW (copied on a stream of its own, beside whatever is running) */
int avk_debug_snapshot(avk_ctx *ctx, avk_dev_batch *db, uint32_t *counters, uint32_t n_counters, int32_t busy[5]) {
    if (!ctx || !db || !counters || !busy) return AVK_E_ARG;
    AVK_HIP(ctx, hipSetDevice(ctx->device));
    static hipStream_t probe = nullptr;
    if (!probe) AVK_HIP(ctx, hipStreamCreateWithFlags(&probe, hipStreamNonBlocking));
    hipStream_t ss[5] = {ctx->stream, ctx->side_stream, ctx->side_stream2, ctx->lane_stream, ctx->lane_stream2}; /* (lane_stream3 joins lane_stream2 or lane_stream) */
    for (int i = 0; i < 5; ++i) busy[i] = ss[i] ? (hipStreamQuery(ss[i]) == hipErrorNotReady ? 1 : 0) : -1;
    (void)hipGetLastError();
    if (n_counters > AVK_N_COUNTERS) n_counters = AVK_N_COUNTERS;
    AVK_HIP(ctx, hipMemcpyAsync(counters, db->d_counters, (size_t)n_counters * sizeof(uint32_t), hipMemcpyDeviceToHost, probe));
    AVK_HIP(ctx, hipStreamSynchronize(probe));
    return 0;
}

/* The work order of a device-packed batch and the plan behind it: region order[k] is record k; [0, n_hbm) class C, [n_hbm, n_hbm + n_hard) class B, then the bulk, then the
 * lane classes from fast_base[fc] (n_fast[fc] regions each, the first n_fast_heavy[fc] its head); class AVK_FAST_PAIR is looked up.  A measurement aid: bench.py prices every
 * launch class with the algorithmic bytes of ITS regions.  counts[0..3] = n_hbm, n_hbm_notwide, n_hard, n_fast_total; [4 + 3 fc ..] = fast_base, n_fast, n_fast_heavy of
 * class fc (22 words).  order may be NULL.  Host-packed batches: AVK_E_STATE. */
int avk_debug_work_order(avk_ctx *ctx, avk_dev_batch *db, uint32_t *order, uint64_t counts[22]) {
    if (!ctx || !db || !counts) return AVK_E_ARG;
    if (!db->dev_packed || !db->dp_args.order) return fail(ctx, AVK_E_STATE, "the batch was not packed on the device");
    AVK_HIP(ctx, hipSetDevice(ctx->device));
    counts[0] = db->plan.n_hbm, counts[1] = db->plan.n_hbm_notwide, counts[2] = db->plan.n_hard, counts[3] = db->plan.n_fast_total;
    for (int fc = 0; fc < AVK_FAST_CLASSES; ++fc) counts[4 + 3 * fc] = db->plan.fast_base[fc], counts[5 + 3 * fc] = db->plan.n_fast[fc], counts[6 + 3 * fc] = db->plan.n_fast_heavy[fc];
    if (order && db->n_regions) {
        AVK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        AVK_HIP(ctx, hipMemcpy(order, db->dp_args.order, (size_t)db->n_regions * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    return 0;
}

/* The 2-bit copy of the current reference and its flag bitmap, as avk_pack_reference left them (avk_ref_upload): a test aid, read-only.  The packed words are those that
 * cover the reference; the flag words are the whole bitmap the context allocated, so that a test also sees what lies behind the covered part. */
int avk_debug_ref_packed(avk_ctx *ctx, uint32_t *words_out, uint64_t n_words_cap, uint32_t *flags_out, uint64_t n_flag_words_cap) {
    if (!ctx) return AVK_E_ARG;
    if (!ctx->d_ref || !ctx->d_ref2b || !ctx->d_refexc) return fail(ctx, AVK_E_ARG, "avk_ref_upload has not been called");
    uint64_t total = 0;
    for (uint64_t len : ctx->contig_len) total += len;
    const uint64_t n_words = (total + 15) >> 4, n_flag_words = (n_words >> 5) + 8;
    if (!flags_out || (n_words && !words_out) || n_words_cap < n_words || n_flag_words_cap < n_flag_words)
        return fail(ctx, AVK_E_ARG, "avk_debug_ref_packed needs room for %llu packed words and %llu flag words", (unsigned long long)n_words, (unsigned long long)n_flag_words);
    AVK_HIP(ctx, hipSetDevice(ctx->device));
    AVK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (n_words) AVK_HIP(ctx, hipMemcpy(words_out, ctx->d_ref2b, (size_t)n_words * sizeof(uint32_t), hipMemcpyDeviceToHost));
    AVK_HIP(ctx, hipMemcpy(flags_out, ctx->d_refexc, (size_t)n_flag_words * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return 0;
}

int avk_last_tier_counts(avk_ctx *ctx, uint64_t counts[5]) {
    if (!ctx || !counts) return AVK_E_ARG;
    memcpy(counts, ctx->last_tiers, sizeof(ctx->last_tiers));
    return 0;
}


/* Regions that exhausted the last workspace tier (AVK_ST_CAPACITY) are solved again by the library itself, in slices of 1, 4 and 16 GB
 * (the reference grows its vectors without bound, dynamic_wfa.rs:152; an MI355X has 288 GB): the regions are rebuilt from the packed
 * batch the context keeps, sent through the big-slice tier alone, and their results are written over the failed ones.  `fixed`
 * receives, per level, the sub-batch results. */
namespace {
struct CapacityFix {
    std::vector<uint32_t> idx; /* caller region index of the sub-batch's regions */
    std::vector<int32_t> status;
    std::vector<uint32_t> ed1, ed2, nopt, seq_len, gm, bp_off, bp;
    std::vector<uint16_t> present;
    std::vector<uint8_t> ve, vo, vc, vz, seq;
    std::vector<uint64_t> seq_off, v_first; /* first sub-batch variant of a region (truth first, then query) */
    std::vector<uint32_t> seq_stride;
    std::vector<uint64_t> tally;
};
} // namespace

static int results_download_impl(avk_ctx *ctx, const CallSpec &spec, avk_dev_batch *db, avk_result_batch *out, struct DownloadLater *later, const uint64_t *tally_ready);
/* sub_spec: what the sub-batch's kernels write (emit_gm, emit_bp) — the blocks and groups the repair needs, whatever the caller's batch ran with */
static int rerun_capacity_regions(avk_ctx *ctx, const CallSpec &sub_spec, avk_dev_batch *db, const std::vector<uint32_t> &cap, bool want_seq, uint64_t slice_bytes, CapacityFix *fx) {
    const bool want_gm = sub_spec.emit_gm, want_bp = sub_spec.emit_bp;
    const uint64_t m = cap.size();
    std::vector<uint64_t> rid(m), st(m), en(m), toff(m), qoff(m), vpos, a0off, a1off;
    std::vector<uint32_t> cidx(m), tcnt(m), qcnt(m), vraw, a0len, a1len;
    std::vector<uint8_t> vtype, vzyg, arena;
    fx->idx = cap;
    fx->v_first.assign(m, 0);
    for (uint64_t k = 0; k < m; ++k) {
        const AvkDevRegion &dr = db->host.regions[cap[k]];
        uint32_t c = 0;
        while (c + 1 < ctx->contig_base.size() && ctx->contig_base[c + 1] <= dr.ref_off) c += 1;
        rid[k] = cap[k];
        cidx[k] = c;
        st[k] = dr.ref_off - ctx->contig_base[c];
        en[k] = st[k] + dr.len;
        const uint32_t N = dr.t_cnt + dr.q_cnt;
        const uint8_t *base = (const uint8_t *)(db->host.blob.data() + 2ull * dr.blob_off);
        const AvkBlobVar *bv = (const AvkBlobVar *)base;
        const uint8_t *ba = base + (((uint64_t)N * sizeof(AvkBlobVar) + 15) & ~15ull);
        toff[k] = vpos.size();
        tcnt[k] = dr.t_cnt;
        qoff[k] = vpos.size() + dr.t_cnt;
        qcnt[k] = dr.q_cnt;
        fx->v_first[k] = vpos.size();
        for (uint32_t i = 0; i < N; ++i) {
            vpos.push_back(st[k] + bv[i].rel_pos);
            vtype.push_back((uint8_t)(bv[i].type_zyg & 0xFF));
            vzyg.push_back((uint8_t)((bv[i].type_zyg >> 8) & 0xFF));
            vraw.push_back(bv[i].raw_space);
            a0off.push_back(arena.size());
            a0len.push_back(bv[i].a0_len);
            arena.insert(arena.end(), ba + bv[i].a_off, ba + bv[i].a_off + bv[i].a0_len);
            a1off.push_back(arena.size());
            a1len.push_back(bv[i].a1_len);
            arena.insert(arena.end(), ba + bv[i].a_off + bv[i].a0_len, ba + bv[i].a_off + bv[i].a0_len + bv[i].a1_len);
        }
    }
    arena.push_back(0);
    avk_region_batch b;
    memset(&b, 0, sizeof(b));
    b.n_regions = m;
    b.region_id = rid.data(), b.contig_idx = cidx.data(), b.start = st.data(), b.end = en.data(), b.t_off = toff.data(), b.t_cnt = tcnt.data(), b.q_off = qoff.data(),
    b.q_cnt = qcnt.data();
    b.n_variants = vpos.size();
    b.var_pos = vpos.data(), b.var_type = vtype.data(), b.var_zyg = vzyg.data(), b.var_raw_space = vraw.data(), b.a0_off = a0off.data(), b.a0_len = a0len.data(),
    b.a1_off = a1off.data(), b.a1_len = a1len.data(), b.allele_bytes = arena.data(), b.allele_bytes_len = arena.size();
    const uint64_t nvs = vpos.size();
    fx->status.assign(m, 0), fx->ed1.assign(m, 0), fx->ed2.assign(m, 0), fx->nopt.assign(m, 0), fx->present.assign(m, 0);
    fx->ve.assign(nvs + 1, 0), fx->vo.assign(nvs + 1, 0), fx->vc.assign(nvs + 1, 0), fx->vz.assign(nvs + 1, 0);
    fx->tally.assign(AVK_TALLY_LEN, 0);
    avk_result_batch o;
    memset(&o, 0, sizeof(o));
    o.status = fx->status.data(), o.ed_h1 = fx->ed1.data(), o.ed_h2 = fx->ed2.data(), o.n_optima = fx->nopt.data(), o.type_present = fx->present.data();
    o.var_expected = fx->ve.data(), o.var_observed = fx->vo.data(), o.var_class = fx->vc.data(), o.var_zyg = fx->vz.data(), o.tally = fx->tally.data();
    if (want_gm) {
        fx->gm.assign(m * AVK_N_GROUPS * AVK_N_FIELDS, 0);
        o.group_metrics = fx->gm.data();
    }
    if (want_bp) {
        fx->bp_off.assign(m + 1, 0);
        fx->bp.assign((m + nvs + 1) * 4, 0);
        o.bp_off = fx->bp_off.data(), o.bp_groups = fx->bp.data();
    }
    if (want_seq) {
        fx->seq_off.assign(m, 0), fx->seq_stride.assign(m, 0), fx->seq_len.assign(m * 5, 0);
        uint64_t total = 0;
        for (uint64_t k = 0; k < m; ++k) {
            fx->seq_stride[k] = avk::seq_stride_of(&b, k);
            fx->seq_off[k] = total;
            total += 5ull * fx->seq_stride[k];
        }
        fx->seq.assign(total + 16, 0);
        o.seq_bytes = fx->seq.data(), o.seq_off = fx->seq_off.data(), o.seq_stride = fx->seq_stride.data(), o.seq_len = fx->seq_len.data();
    }
    /* the big-slice tier alone.  The one save and restore of options left: run_internal reads these seven in some thirty places, and they are tuning the caller set
     * for its own batches, not something a call decides — nothing between the two lines below returns early */
    const int64_t keep[] = {ctx->lds_bytes_per_wave, ctx->lds2_bytes_per_wave, ctx->ws_bytes_per_wave, ctx->big_ws_bytes, ctx->big_waves, ctx->lane_kernel, ctx->capacity_retry};
    ctx->lds_bytes_per_wave = 0, ctx->lds2_bytes_per_wave = 0, ctx->ws_bytes_per_wave = 0, ctx->big_ws_bytes = (int64_t)slice_bytes, ctx->big_waves = m < 4 ? (int64_t)m : 4,
    ctx->lane_kernel = 0, ctx->capacity_retry = 0;
    avk_dev_batch *sub = nullptr;
    int rc = upload_internal(ctx, sub_spec, &b, false, &sub);
    if (!rc) rc = run_internal(ctx, sub_spec, sub, &db->last_cfg, nullptr, 0);
    if (!rc) rc = results_download_impl(ctx, sub_spec, sub, &o, nullptr, nullptr);
    if (sub) avk_batch_free(ctx, sub);
    ctx->lds_bytes_per_wave = keep[0], ctx->lds2_bytes_per_wave = keep[1], ctx->ws_bytes_per_wave = keep[2], ctx->big_ws_bytes = keep[3], ctx->big_waves = keep[4],
    ctx->lane_kernel = keep[5], ctx->capacity_retry = keep[6];
    return rc;
}

} /* extern "C" */
/* a one-call form with labels (avk_compare_packed_labels, avk_wait of a submit with labels): its label kernel ran before the capacity retry, so the blocks of the
 * regions the retry repairs are added to the labels' sums here, on the host */
struct LabelFix {
    const avk_region_labels *lab; /* NULL: the lists were made on the device (avk_compare_packed_strata) and a repaired region's few entries are fetched from there */
    uint64_t *out; /* [n_labels * AVK_TALLY_LEN] */
    const uint64_t *d_off = nullptr;
    const uint32_t *d_idx = nullptr;
    const uint32_t *d_mask = nullptr; /* no lists at all (avk_compare_packed_submit_strata): a repaired region's n_words mask words, word-major over n regions */
    uint32_t n_words = 0;
    uint64_t n = 0;               /* regions of the batch */
    std::vector<uint64_t> h_off;  /* the device lists' offsets, fetched once, at the first repaired region */
    hipError_t err = hipSuccess;  /* a failed fetch: the call that set the fix up fails with it */
};
static void label_fix_add(LabelFix *lf, uint64_t r, const uint32_t *block) {
    if (!lf->lab && lf->d_mask) { /* one strided copy of the region's words (the mask pass finished before the solve), made into the region's small list */
        if (lf->err != hipSuccess || !lf->n_words || r >= lf->n) return;
        std::vector<uint32_t> words(lf->n_words), idx;
        lf->err = hipMemcpy2D(words.data(), 4, lf->d_mask + r, (size_t)lf->n * 4, 4, lf->n_words, hipMemcpyDeviceToHost);
        if (lf->err != hipSuccess) return;
        for (uint32_t w = 0; w < lf->n_words; ++w) /* (set bits lowest first: the order of the kernels' lists) */
            for (uint32_t x = words[w]; x; x &= x - 1u) idx.push_back(w * 32u + (uint32_t)__builtin_ctz(x));
        const uint64_t off[2] = {0, idx.size()};
        const avk_region_labels one{lf->n_words * 32u, off, idx.data()};
        LabelFix host{&one, lf->out};
        label_fix_add(&host, 0, block);
        return;
    }
    if (!lf->lab) { /* (the list kernels finished before the solve whose results the retry has just read) */
        if (lf->err != hipSuccess) return;
        if (lf->h_off.empty()) {
            lf->h_off.resize((size_t)lf->n + 1);
            lf->err = hipMemcpy(lf->h_off.data(), lf->d_off, (size_t)(lf->n + 1) * 8, hipMemcpyDeviceToHost);
            if (lf->err != hipSuccess) return;
        }
        const uint64_t be[2] = {lf->h_off[r], lf->h_off[r + 1]};
        if (be[1] <= be[0]) return;
        std::vector<uint32_t> idx((size_t)(be[1] - be[0]));
        lf->err = hipMemcpy(idx.data(), lf->d_idx + be[0], idx.size() * 4, hipMemcpyDeviceToHost);
        if (lf->err != hipSuccess) return;
        for (const uint32_t l : idx) {
            uint64_t *dst = lf->out + (size_t)l * AVK_TALLY_LEN;
            for (int i = 0; i < AVK_N_GROUPS * AVK_N_FIELDS; ++i) dst[i] += block[i];
        }
        return;
    }
    for (uint64_t q = lf->lab->label_off[r]; q < lf->lab->label_off[r + 1]; ++q) {
        uint64_t *dst = lf->out + (size_t)lf->lab->label_idx[q] * AVK_TALLY_LEN;
        for (int i = 0; i < AVK_N_GROUPS * AVK_N_FIELDS; ++i) dst[i] += block[i];
    }
}
/* avk_results_download in one piece (later == NULL), or in the two pieces of the asynchronous boundary: everything up to the queued copies (later given, tally_ready
 * NULL), and everything behind them — the tally, the statistics, the capacity retry — once the copies have arrived (tally_ready = the batch's tally words) */
static int results_download_impl(avk_ctx *ctx, const CallSpec &spec, avk_dev_batch *db, avk_result_batch *out, DownloadLater *later, const uint64_t *tally_ready) {
    if (!ctx || !db || !out || !(out->status || out->region_packed)) return AVK_E_ARG;
    AVK_HIP(ctx, hipSetDevice(ctx->device));
    const uint64_t n = db->n_regions, nv = db->n_variants_dev;
    const bool timing = getenv("AVK_TIMING") != nullptr;
    const auto t_begin = std::chrono::steady_clock::now();
    std::vector<uint64_t> tally((size_t)AVK_TALLY_STRIDE);
    if (tally_ready) memcpy(tally.data(), tally_ready, (size_t)AVK_TALLY_STRIDE * sizeof(uint64_t));
    if (later && !(db->dev_packed && db->var_dense && !(out->seq_bytes && out->seq_len && out->seq_off && out->seq_stride && db->d_seq)))
        return fail(ctx, AVK_E_STATE, "results can only be queued for a device-packed batch that owns all its calls, without sequence outputs");
    hipStream_t s = ctx->stream;
    const bool want_seq = out->seq_bytes && out->seq_len && out->seq_off && out->seq_stride && db->d_seq;
    std::vector<uint8_t> seq;
    std::vector<uint32_t> seqlen;
#define D2H(dst, src, bytes) \
    if ((bytes) > 0) AVK_HIP(ctx, hipMemcpyAsync((dst), (src), (bytes), hipMemcpyDeviceToHost, s))
    if (want_seq) {
        seq.resize(db->seq_total + 16);
        seqlen.resize(n * 5 + 1);
        D2H(seq.data(), db->d_seq, db->seq_total);
        D2H(seqlen.data(), db->d_seqlen, n * 5 * sizeof(uint32_t));
    }
    std::chrono::steady_clock::time_point t_copied;
    /* the host-side writers of a region's and a call's results: whichever of the wide arrays and of the packed form the caller handed in */
    auto put_region = [&](uint64_t r, uint32_t st, uint32_t e1, uint32_t e2, uint32_t nopt, uint32_t present) {
        if (out->status) out->status[r] = (int32_t)st;
        if (out->ed_h1) out->ed_h1[r] = e1;
        if (out->ed_h2) out->ed_h2[r] = e2;
        if (out->n_optima) out->n_optima[r] = nopt;
        if (out->type_present) out->type_present[r] = (uint16_t)present;
        if (out->region_packed) out->region_packed[r] = avk_rp_make(st, e1, e2, nopt, present);
    };
    auto put_call = [&](uint64_t hv, uint32_t ea, uint32_t oa, uint32_t cls, uint32_t zyg) {
        if (out->var_expected) out->var_expected[hv] = (uint8_t)ea;
        if (out->var_observed) out->var_observed[hv] = (uint8_t)oa;
        if (out->var_class) out->var_class[hv] = (uint8_t)cls;
        if (out->var_zyg) out->var_zyg[hv] = (uint8_t)zyg;
        if (out->var_packed) out->var_packed[hv] = avk_vp_make(ea, oa, zyg);
    };
    auto status_of = [&](uint64_t r) -> int32_t { return out->status ? out->status[r] : avk_rp_status(out->region_packed[r]); };
    if (tally_ready) { /* the copies were queued earlier and have arrived */
        t_copied = std::chrono::steady_clock::now();
    } else if (db->dev_packed) { /* the caller's layout is made on the device (dp_unpack); the copies land in the caller's arrays */
        const int rc = download_device_packed(ctx, spec, db, out, nullptr, tally.data(), later);
        if (rc || later) return rc;
        t_copied = std::chrono::steady_clock::now();
        if (want_seq) {
            const int rv = materialize_host_view(ctx, db);
            if (rv) return rv;
        }
    } else {
        std::vector<uint32_t> rout(n * 4 + 4), vout(nv + 1);
        D2H(rout.data(), db->d_region_out, n * 4 * sizeof(uint32_t));
        if (out->group_metrics && spec.emit_gm && db->d_gm) D2H(out->group_metrics, db->d_gm, n * AVK_N_GROUPS * AVK_N_FIELDS * sizeof(uint32_t));
        if (out->bp_off && out->bp_groups && db->d_bp && db->d_bp_off) {
            D2H(out->bp_off, db->d_bp_off, (n + 1) * sizeof(uint32_t));
            D2H(out->bp_groups, db->d_bp, (size_t)db->n_bp_groups * 4 * sizeof(uint32_t));
        }
        const bool want_calls = out->var_expected || out->var_observed || out->var_class || out->var_zyg || out->var_packed;
        if (want_calls) D2H(vout.data(), db->d_var_out, nv * sizeof(uint32_t));
        D2H(tally.data(), db->d_tally, (size_t)AVK_TALLY_STRIDE * sizeof(uint64_t));
        AVK_HIP(ctx, hipStreamSynchronize(s));
        t_copied = std::chrono::steady_clock::now();
        for (uint64_t r = 0; r < n; ++r) {
            const uint32_t *w = rout.data() + 4 * r;
            put_region(r, w[0], w[1], w[2], w[3] & 0xFFFFu, w[3] >> 16);
        }
        for (uint64_t v = 0; want_calls && v < nv; ++v) {
            const uint32_t w = vout[v];
            put_call(db->host.dev2host[v], w & 0xFF, (w >> 8) & 0xFF, (w >> 16) & 0xFF, w >> 24);
        }
    }
#undef D2H
    if (timing)
        fprintf(stderr, "avk download%s: kernels + copies %.3f ms, unpack %.3f ms\n", db->dev_packed ? " (device-packed)" : "", std::chrono::duration<double, std::milli>(t_copied - t_begin).count(),
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_copied).count());
    if (out->tally) memcpy(out->tally, tally.data(), AVK_TALLY_LEN * sizeof(uint64_t));
    memcpy(ctx->last_tiers, tally.data() + AVK_TALLY_LEN, 5 * sizeof(uint64_t));
    ctx->last_lane_solved = tally[AVK_TALLY_LANE_SOLVED];
    ctx->last_wide_solved = tally[AVK_TALLY_WIDE_SOLVED];
    memcpy(ctx->last_phase, tally.data() + AVK_TALLY_LEN + 5, 16 * sizeof(uint64_t));
    if (want_seq) {
        for (uint64_t r = 0; r < n; ++r) {
            const AvkDevRegion &dr = db->host.regions[r];
            for (int k = 0; k < 5; ++k) {
                uint32_t len = seqlen[5 * r + k];
                if (len > out->seq_stride[r]) len = out->seq_stride[r];
                memcpy(out->seq_bytes + out->seq_off[r] + (uint64_t)k * out->seq_stride[r], seq.data() + dr.seq_off + (uint64_t)k * dr.seq_stride, len);
                out->seq_len[5 * r + k] = len;
            }
        }
    }
    /* no solvable region stays a capacity failure: larger slices, level by level (an overflow status is only allowed when
     * the library itself solves the region again) */
    if (ctx->capacity_retry && db->has_run && db->last_mode == 0 && ctx->last_tiers[4] > 0) { /* (the kernels count the regions they give up on: a step without
                                                                                                  any — every step of a genome — does not walk over its 3.6 million
                                                                                                  statuses, 1.4 ms of one host thread) */
        std::vector<uint32_t> cap;
        for (uint64_t r = 0; r < n; ++r)
            if (status_of(r) == AVK_ST_CAPACITY) cap.push_back((uint32_t)r);
        if (!cap.empty()) { /* the retry rebuilds the regions from the packed records: a device-packed batch fetches them now */
            const int rv = materialize_host_view(ctx, db);
            if (rv) return rv;
        }
        const bool big_grown = !cap.empty();
        const size_t big_before = ctx->big_alloc;
        int retry_rc = 0;
        uint64_t keep_tiers[5];
        memcpy(keep_tiers, ctx->last_tiers, sizeof(keep_tiers));
        const uint64_t keep_lane_solved = ctx->last_lane_solved, keep_wide_solved = ctx->last_wide_solved;
        for (uint64_t slice = 1ull << 30; !cap.empty() && slice <= (16ull << 30); slice <<= 2) {
            if ((int64_t)slice <= ctx->big_ws_bytes) continue;
            CapacityFix fx;
            const bool dev_gm = spec.emit_gm && db->d_gm; /* the batch keeps per-region blocks on the device (avk_label_tallies reads them) */
            /* ... or the compact view avk_label_tallies_compact reads: the repaired region's per-call words and BASEPAIR groups are patched as well */
            const bool dev_compact = db->dev_packed && db->bp_valid && db->d_bp && db->d_bp_off && db->d_var_out;
            const bool want_gm = (out->group_metrics && spec.emit_gm && db->d_gm) || dev_gm || spec.label_fix != nullptr;
            const bool want_bp_words = out->bp_packed && out->bp_spilled && out->bp_groups && db->d_bp;
            const bool want_bp = (out->bp_off && out->bp_groups && db->d_bp) || want_bp_words || dev_compact;
            CallSpec sub_spec;
            sub_spec.emit_gm = want_gm, sub_spec.emit_bp = want_bp;
            const int rc = rerun_capacity_regions(ctx, sub_spec, db, cap, want_seq, slice, &fx);
            if (rc == AVK_E_OOM) break; /* the device cannot hold slices of this size: the regions keep their status */
            if (rc) { /* reported after the statistics and the shared slices are back as they were (below) */
                retry_rc = rc;
                break;
            }
            std::vector<uint32_t> still;
            for (uint64_t k = 0; k < fx.idx.size(); ++k) {
                const uint32_t r = fx.idx[k];
                if (fx.status[k] == AVK_ST_CAPACITY) {
                    still.push_back(r);
                    continue;
                }
                put_region(r, (uint32_t)fx.status[k], fx.ed1[k], fx.ed2[k], fx.nopt[k], fx.present[k]);
                { /* the batch on the device learns of the repair as well: its region record, and its metric block when it keeps them — the per-label sums of
                   * avk_label_tallies count every solved region, as the totals do */
                    const uint32_t w4[4] = {(uint32_t)fx.status[k], fx.ed1[k], fx.ed2[k], fx.nopt[k] | ((uint32_t)fx.present[k] << 16)};
                    hipError_t ew = hipMemcpyAsync(db->d_region_out + 4 * (size_t)r, w4, sizeof(w4), hipMemcpyHostToDevice, s);
                    if (ew == hipSuccess && dev_gm)
                        ew = hipMemcpyAsync(db->d_gm + (size_t)r * AVK_N_GROUPS * AVK_N_FIELDS, fx.gm.data() + (size_t)k * AVK_N_GROUPS * AVK_N_FIELDS,
                                            sizeof(uint32_t) * AVK_N_GROUPS * AVK_N_FIELDS, hipMemcpyHostToDevice, s);
                    if (ew == hipSuccess) ew = hipStreamSynchronize(s); /* (w4 and fx leave scope) */
                    if (ew != hipSuccess && !retry_rc) retry_rc = fail(ctx, AVK_E_HIP, "capacity retry: %s", hipGetErrorString(ew));
                }
                const AvkDevRegion &dr = db->host.regions[r];
                for (uint32_t i = 0; i < dr.t_cnt + dr.q_cnt; ++i) {
                    const uint64_t sv = fx.v_first[k] + i;
                    put_call(db->host.dev2host[dr.v_off + i], fx.ve[sv], fx.vo[sv], fx.vc[sv], fx.vz[sv]);
                }
                if (dev_compact) { /* the device's per-call words and groups of the region, as the kernels would have left them */
                    const uint32_t nc = dr.t_cnt + dr.q_cnt, ng = fx.bp_off[k + 1] - fx.bp_off[k];
                    std::vector<uint32_t> words(nc + 1);
                    for (uint32_t i = 0; i < nc; ++i) {
                        const uint64_t sv = fx.v_first[k] + i;
                        words[i] = (uint32_t)fx.ve[sv] | (uint32_t)fx.vo[sv] << 8 | (uint32_t)fx.vc[sv] << 16 | (uint32_t)fx.vz[sv] << 24;
                    }
                    uint32_t bo[2] = {0, 0};
                    hipError_t ew = hipMemcpyAsync(bo, db->d_bp_off + r, sizeof(bo), hipMemcpyDeviceToHost, s);
                    if (ew == hipSuccess && nc) ew = hipMemcpyAsync(db->d_var_out + dr.v_off, words.data(), (size_t)nc * 4, hipMemcpyHostToDevice, s);
                    if (ew == hipSuccess) ew = hipStreamSynchronize(s);
                    if (ew == hipSuccess && ng && bo[1] - bo[0] == ng) { /* the same calls, so the same groups */
                        ew = hipMemcpyAsync(db->d_bp + 4 * (size_t)bo[0], fx.bp.data() + 4 * (size_t)fx.bp_off[k], 16 * (size_t)ng, hipMemcpyHostToDevice, s);
                        if (ew == hipSuccess) ew = hipStreamSynchronize(s);
                    }
                    if (ew != hipSuccess && !retry_rc) retry_rc = fail(ctx, AVK_E_HIP, "capacity retry: %s", hipGetErrorString(ew));
                }
                if (spec.label_fix && fx.status[k] == 0) label_fix_add(spec.label_fix, r, fx.gm.data() + (size_t)k * AVK_N_GROUPS * AVK_N_FIELDS);
                if (want_gm && out->group_metrics) memcpy(out->group_metrics + (size_t)r * AVK_N_GROUPS * AVK_N_FIELDS, fx.gm.data() + (size_t)k * AVK_N_GROUPS * AVK_N_FIELDS, sizeof(uint32_t) * AVK_N_GROUPS * AVK_N_FIELDS);
                if (want_bp_words) { /* the packed form: the repaired region's groups join the spilled ones */
                    const uint32_t ng = fx.bp_off[k + 1] - fx.bp_off[k], at = out->bp_spilled[0];
                    memcpy(out->bp_groups + 4 * (size_t)at, fx.bp.data() + 4 * (size_t)fx.bp_off[k], 16 * (size_t)ng);
                    out->bp_packed[r] = AVK_BP_SPILL | at;
                    out->bp_spilled[0] = at + ng;
                } else if (want_bp && out->bp_off && out->bp_groups && out->bp_off[r + 1] - out->bp_off[r] == fx.bp_off[k + 1] - fx.bp_off[k]) /* the same calls, so the same groups */
                    memcpy(out->bp_groups + 4 * (size_t)out->bp_off[r], fx.bp.data() + 4 * (size_t)fx.bp_off[k], 16 * (size_t)(fx.bp_off[k + 1] - fx.bp_off[k]));
                if (want_seq)
                    for (int q = 0; q < 5; ++q) {
                        uint32_t len = fx.seq_len[5 * k + q];
                        if (len > out->seq_stride[r]) len = out->seq_stride[r];
                        memcpy(out->seq_bytes + out->seq_off[r] + (uint64_t)q * out->seq_stride[r], fx.seq.data() + fx.seq_off[k] + (uint64_t)q * fx.seq_stride[k], len);
                        out->seq_len[5 * r + q] = len;
                    }
            }
            if (out->tally) { /* the sub-batch's sums come from its solved regions only */
                for (int i = 0; i < AVK_N_GROUPS * AVK_N_FIELDS; ++i) out->tally[i] += fx.tally[i];
                out->tally[AVK_TALLY_SOLVED] += fx.tally[AVK_TALLY_SOLVED];
                out->tally[AVK_TALLY_ERRORS] -= fx.tally[AVK_TALLY_SOLVED];
            }
            cap.swap(still);
        }
        memcpy(ctx->last_tiers, keep_tiers, sizeof(keep_tiers)); /* the statistics of the caller's batch, not of the retries */
        ctx->last_lane_solved = keep_lane_solved;
        ctx->last_wide_solved = keep_wide_solved;
        if (big_grown && ctx->big_alloc > big_before && ctx->d_big) { /* give the large slices back */
            (void)hipStreamSynchronize(ctx->stream);
            (void)hipFree(ctx->d_big);
            ctx->d_big = nullptr;
            ctx->big_alloc = 0;
        }
        if (retry_rc) return retry_rc;
    }
    return 0;
}

extern "C" {

int avk_results_download(avk_ctx *ctx, avk_dev_batch *db, avk_result_batch *out) { return ctx ? results_download_impl(ctx, call_spec(ctx), db, out, nullptr, nullptr) : AVK_E_ARG; }

/* ---- the asynchronous boundary: one context, batches in flight -------------------------------------------------------------------------------
 * The reference streams its regions through a rayon loop and collects at the end (src/main.rs:251-268); a caller with several batches gets the same here:
 * avk_compare_packed_submit returns when batch k is QUEUED — its arrays crossed (or are crossing) the bus on the context's copy-in stream while batch k - 1 was
 * being solved, its results will cross on the copy-out stream while batch k + 1 is packed — and avk_wait(ticket) returns when the results are in the caller's
 * arrays.  The call blocks once in the middle (the packer's plan comes back to the host), which is where it waits for the batch before it. */
struct avk_ticket {
    int slot = -1;          /* staging slot, -1: the batch was solved synchronously at submit (pageable arrays) */
    int rc = 0;
    avk_dev_batch *db = nullptr;
    avk_result_batch out;
    DownloadLater later;
    CallSpec spec; /* what the batch was submitted with: the copies out were queued with it, avk_wait finishes the download with it */
    /* submitted with labels: the lists (the caller's arrays, read again should the capacity retry repair a region), where the sums go, the device sums */
    bool has_lab = false;
    avk_region_labels lab;
    uint64_t *lab_out = nullptr;
    void *d_lab_out = nullptr;
    /* submitted with resident sets (avk_compare_packed_submit_strata): the job of the packer's mask pass, the masks and the workgroup counts it writes, the number
     * of labels, and the count it shares with the handle — nothing of the handle itself, which may be freed before avk_wait */
    bool has_strata = false;
    StrataJob sjob{nullptr, nullptr, nullptr};
    uint32_t n_labels = 0;
    void *d_mask = nullptr, *d_mask_sums = nullptr;
    std::shared_ptr<StrataUse> strata_use;
};

/* ---- stratified sums from the compact results (avk_labels.inl) -------------------------------------------------------------------------------- */
static int64_t label_lds(avk_ctx *ctx) { /* the LDS a launch of the label kernel really gets: the whole CU's where the runtime grants it */
    if (!ctx->label_lds_bytes) {
        int64_t b = 64 * 1024;
        if (hipFuncSetAttribute((const void *)avk_label_tally_compact_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess &&
            hipFuncSetAttribute((const void *)avk_label_tally_mask_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess)
            b = 160 * 1024;
        else {
            (void)hipGetLastError();
            int attr = 0;
            if (hipDeviceGetAttribute(&attr, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device) == hipSuccess && attr > 0 && attr < b) b = attr;
            else (void)hipGetLastError();
        }
        ctx->label_lds_bytes = b;
    }
    return ctx->label_lds_bytes;
}
static uint32_t label_block(avk_ctx *ctx) {
    const int64_t b = label_lds(ctx) / AVK_LB_LABEL_BYTES;
    return b < 1 ? 1u : (uint32_t)b;
}
/* the refusals of every entry point with labels, before anything is queued */
static int labels_check(avk_ctx *ctx, uint64_t n, const avk_region_labels *lab, const uint64_t *label_tallies) {
    if (!lab->label_off) return fail(ctx, AVK_E_ARG, "label_off missing");
    for (uint64_t r = 0; r < n; ++r)
        if (lab->label_off[r + 1] < lab->label_off[r]) return fail(ctx, AVK_E_ARG, "label_off must not decrease");
    const uint64_t n_idx = lab->label_off[n];
    if (n_idx && !lab->label_idx) return fail(ctx, AVK_E_ARG, "label_idx missing: label_off names %llu entries", (unsigned long long)n_idx);
    for (uint64_t q = lab->label_off[0]; q < n_idx; ++q)
        if (lab->label_idx[q] >= lab->n_labels) return fail(ctx, AVK_E_ARG, "label index %u of %u", lab->label_idx[q], lab->n_labels);
    if (!label_tallies) return fail(ctx, AVK_E_ARG, "label_tallies missing");
    return 0;
}
/* the label kernel over the blocks of labels, on stream s behind the batch's solve: d_out[n_labels * AVK_TALLY_LEN] gains the sums.  d_mask given: the labels
 * come from the strata pass's bit masks (avk_label_tally_mask_kernel), d_off and d_idx are not read. */
static int labels_launch(avk_ctx *ctx, avk_dev_batch *db, const uint64_t *d_off, const uint32_t *d_idx, uint32_t n_labels, uint64_t *d_out, hipStream_t s,
                         const uint32_t *d_mask = nullptr) {
    const uint64_t n = db->n_regions;
    if (!n || !n_labels) return 0;
    avk::lb::LbView v;
    memset(&v, 0, sizeof(v));
    v.in = db->dp_args.in, v.vinfo = db->dp_args.vinfo, v.region_out = db->d_region_out, v.var_out = db->d_var_out, v.v_off = db->d_voff, v.bp_off = db->d_bp_off, v.bp = db->d_bp;
    uint32_t B = label_block(ctx);
    if (d_mask && B > AVK_LB_MASK_BLOCK_MAX) B = AVK_LB_MASK_BLOCK_MAX; /* (a lane keeps the block's mask words in registers) */
    const bool timing = getenv("AVK_TIMING") != nullptr;
    if (timing) {
        if (!ctx->ev_lab0 && hipEventCreate(&ctx->ev_lab0) != hipSuccess) ctx->ev_lab0 = nullptr, (void)hipGetLastError();
        if (!ctx->ev_lab1 && hipEventCreate(&ctx->ev_lab1) != hipSuccess) ctx->ev_lab1 = nullptr, (void)hipGetLastError();
        if (ctx->ev_lab0) (void)hipEventRecord(ctx->ev_lab0, s);
    }
    for (uint32_t lo = 0; lo < n_labels; lo += B) {
        const uint32_t hi = n_labels - lo > B ? lo + B : n_labels;
        const size_t lds = (size_t)(hi - lo) * AVK_LB_LABEL_BYTES;
        /* a CU runs 2,048 work-items: two workgroups where their sums fit beside each other */
        const uint32_t per_cu = lds * 2 <= (size_t)label_lds(ctx) ? 2u : 1u;
        uint64_t blocks = (n + 1023) / 1024;
        if (blocks > (uint64_t)ctx->n_cus * per_cu) blocks = (uint64_t)ctx->n_cus * per_cu;
        if (d_mask) hipLaunchKernelGGL(avk_label_tally_mask_kernel, dim3((unsigned)blocks), dim3(1024), lds, s, v, d_mask, (uint32_t)n, lo, hi, (unsigned long long *)d_out);
        else
            hipLaunchKernelGGL(avk_label_tally_compact_kernel, dim3((unsigned)blocks), dim3(1024), lds, s, v, (const unsigned long long *)d_off, d_idx, (uint32_t)n, lo, hi,
                               (unsigned long long *)d_out);
        AVK_HIP(ctx, hipGetLastError());
    }
    if (timing && ctx->ev_lab1) (void)hipEventRecord(ctx->ev_lab1, s);
    return 0;
}
/* ... with the sums cleared first (clear) and queued back to the host behind the kernels (host given), all on the context's stream */
static int label_sums_queue(avk_ctx *ctx, avk_dev_batch *db, const void *d_off, const void *d_idx, uint32_t n_labels, void *d_out, bool clear, uint64_t *host,
                            const uint32_t *d_mask = nullptr) {
    const size_t bytes = (size_t)n_labels * AVK_TALLY_LEN * sizeof(uint64_t);
    hipError_t e = clear ? hipMemsetAsync(d_out, 0, bytes, ctx->stream) : hipSuccess;
    if (e != hipSuccess) return fail(ctx, AVK_E_HIP, host ? "label tallies failed: %s" : "label sums: %s", hipGetErrorString(e)); /* (no host copy: the submit, with its own text) */
    const int rc = labels_launch(ctx, db, (const uint64_t *)d_off, (const uint32_t *)d_idx, n_labels, (uint64_t *)d_out, ctx->stream, d_mask);
    if (rc) return rc;
    if (host && (e = hipMemcpyAsync(host, d_out, bytes, hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess) return fail(ctx, AVK_E_HIP, "label tallies failed: %s", hipGetErrorString(e));
    return 0;
}
static void labels_timing_print(avk_ctx *ctx, const char *route, uint32_t n_labels, uint64_t n, uint64_t n_idx) { /* behind a synchronisation with the kernels' stream */
    if (!getenv("AVK_TIMING") || !ctx->ev_lab0 || !ctx->ev_lab1) return;
    float ms = 0;
    if (hipEventElapsedTime(&ms, ctx->ev_lab0, ctx->ev_lab1) != hipSuccess) {
        (void)hipGetLastError();
        return;
    }
    const uint32_t B = label_block(ctx);
    fprintf(stderr, "avk label tallies (compact, %s): %u labels in %u launches of at most %u, %llu regions, %llu list entries: kernels %.3f ms\n", route, n_labels, (n_labels + B - 1) / B, B,
            (unsigned long long)n, (unsigned long long)n_idx, ms);
}

static int stage_slot_prepare(avk_ctx *ctx, avk_ctx::StageSlot &sl, size_t bytes) {
    if (!ctx->copy_in_stream || !ctx->copy_out_stream || !ctx->pack_stream || !ctx->pack_side_stream) {
        /* the four streams of the asynchronous calls, made at the first submit (a context that never submits does not hold their hardware queues: two processes on a
         * GPU with twelve streams each are more than the scheduler maps at a time).  The placeholders of avk_ctx_create are gone by now and their queues would be the
         * first to be handed out again — to these four, which then sit exactly where nothing was meant to (two genomes in flight: 4.8 ms per genome instead of 4.4):
         * the placeholders are made again for the moment, as they were when the order was searched. */
        hipStream_t ph[16];
        int n_ph = 0;
        if (!getenv("AVK_KEEP_SPARES"))
            for (; n_ph < ctx->n_placeholders && n_ph < 16; ++n_ph)
                if (hipStreamCreateWithFlags(&ph[n_ph], hipStreamNonBlocking) != hipSuccess) break;
        hipError_t e = hipSuccess;
        if (!ctx->copy_in_stream) e = hipStreamCreateWithFlags(&ctx->copy_in_stream, hipStreamNonBlocking);
        if (e == hipSuccess && !ctx->copy_out_stream) e = hipStreamCreateWithFlags(&ctx->copy_out_stream, hipStreamNonBlocking);
        if (e == hipSuccess && !ctx->pack_stream) e = hipStreamCreateWithFlags(&ctx->pack_stream, hipStreamNonBlocking);
        if (e == hipSuccess && !ctx->pack_side_stream) e = hipStreamCreateWithFlags(&ctx->pack_side_stream, hipStreamNonBlocking);
        for (int k = 0; k < n_ph; ++k) (void)hipStreamDestroy(ph[k]);
        AVK_HIP(ctx, e);
    }
    if (!ctx->ev_packed) AVK_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_packed, hipEventDisableTiming));
    if (!ctx->ev_pool_fence) AVK_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_pool_fence, hipEventDisableTiming));
    if (!sl.ev_in) {
        AVK_HIP(ctx, hipEventCreateWithFlags(&sl.ev_in, hipEventDisableTiming));
        AVK_HIP(ctx, hipEventCreateWithFlags(&sl.ev_unpacked, hipEventDisableTiming));
        AVK_HIP(ctx, hipEventCreateWithFlags(&sl.ev_done, hipEventDisableTiming));
        AVK_HIP(ctx, hipHostMalloc((void **)&sl.h_tally, (size_t)AVK_TALLY_STRIDE * sizeof(uint64_t), hipHostMallocDefault));
    }
    if (sl.bytes < bytes) {
        if (sl.dev) AVK_HIP(ctx, hipFree(sl.dev)); /* (the slot is free: nothing of an earlier batch reads it) */
        sl.dev = nullptr, sl.bytes = 0;
        const size_t want = bytes + bytes / 8 + (1u << 20);
        hipError_t e = hipMalloc((void **)&sl.dev, want);
        if (e != hipSuccess) return fail(ctx, e == hipErrorOutOfMemory ? AVK_E_OOM : AVK_E_HIP, "staging slot of %zu bytes: %s", want, hipGetErrorString(e));
        sl.bytes = want;
    }
    return 0;
}

/* the eleven arrays of `batch` into a staging slot: the slot is (re)sized and the copies are queued on the copy-in stream, counts and lengths first as in
 * avk_compare_packed — nothing of this context reads or writes the slot */
static int stage_layout(avk_ctx *ctx, avk_ctx::StageSlot &sl, const avk_packed_batch *batch, const avk_packed_escapes *esc, PackedOnDevice *pre,
                        const avk_region_labels *lab = nullptr) {
    const uint64_t n = batch->n_regions, nv = batch->n_variants, alen = batch->allele_bytes_len;
    const bool has_contig = batch->contig_idx != nullptr, has_raw = batch->var_raw_space != nullptr;
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const uint64_t er = esc ? esc->n_esc_regions : 0, es = esc ? esc->n_esc_slots : 0, ec = esc ? esc->n_esc_calls : 0; /* (esc: NULL unless it lists something) */
    const size_t need = 2 * up(n + 16) + 3 * up(nv + 16) + up(n * 4 + 16) + 2 * up(n * 2 + 16) + up(nv * 2 + 16) + up(nv * 4 + 16) + up(alen + 16) +
                        (esc ? up(er * 8 + 16) + up(er * 4 + 16) + up(es * 8 + 16) + up(es * 4 + 16) + up(ec * 8 + 16) + 3 * up(ec * 4 + 16) : 0) +
                        (lab ? up((n + 1) * 8 + 16) + up(lab->label_off[n] * 4 + 16) : 0);
    {
        const int rc = stage_slot_prepare(ctx, sl, need);
        if (rc) return rc;
    }
    memset(pre, 0, sizeof(*pre));
    uint8_t *q = sl.dev;
    auto take = [&](size_t bytes) {
        uint8_t *r = q;
        q += up(bytes + 16);
        return r;
    };
    pre->t_cnt = take(n), pre->q_cnt = take(n), pre->a0_len = take(nv), pre->a1_len = take(nv), pre->start = (uint32_t *)take(n * 4), pre->len = (uint16_t *)take(n * 2);
    pre->contig = (uint16_t *)take(n * 2), pre->rel_pos = (uint16_t *)take(nv * 2), pre->var_type_zyg = take(nv), pre->raw = (uint32_t *)take(nv * 4), pre->alleles = take(alen);
    pre->ready = sl.ev_in;
    if (esc) { /* the escape lists ride on the copy stream with the rest */
        pre->esc_region = (uint64_t *)take(er * 8), pre->esc_len = (uint32_t *)take(er * 4), pre->esc_slot = (uint64_t *)take(es * 8), pre->esc_cnt = (uint32_t *)take(es * 4);
        pre->esc_call = (uint64_t *)take(ec * 8), pre->esc_rel = (uint32_t *)take(ec * 4), pre->esc_a0 = (uint32_t *)take(ec * 4), pre->esc_a1 = (uint32_t *)take(ec * 4);
        const struct { const void *src; void *dst; size_t bytes; } ce[] = {
            {esc->esc_region, pre->esc_region, er * 8}, {esc->esc_len, pre->esc_len, er * 4}, {esc->esc_slot, pre->esc_slot, es * 8}, {esc->esc_cnt, pre->esc_cnt, es * 4},
            {esc->esc_call, pre->esc_call, ec * 8}, {esc->esc_rel_pos, pre->esc_rel, ec * 4}, {esc->esc_a0_len, pre->esc_a0, ec * 4}, {esc->esc_a1_len, pre->esc_a1, ec * 4}};
        for (const auto &c : ce)
            if (c.bytes && c.src && hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyHostToDevice, ctx->copy_in_stream) != hipSuccess) {
                (void)hipStreamSynchronize(ctx->copy_in_stream);
                return fail(ctx, AVK_E_HIP, "queueing the batch's copies failed: %s", hipGetErrorString(hipGetLastError()));
            }
    }
    if (lab) { /* the label lists ride on the copy stream as well */
        const uint64_t n_idx = lab->label_off[n];
        pre->lab_off = (uint64_t *)take((n + 1) * 8), pre->lab_idx = (uint32_t *)take(n_idx * 4);
        hipError_t el = hipMemcpyAsync(pre->lab_off, lab->label_off, (n + 1) * 8, hipMemcpyHostToDevice, ctx->copy_in_stream);
        if (el == hipSuccess && n_idx) el = hipMemcpyAsync(pre->lab_idx, lab->label_idx, n_idx * 4, hipMemcpyHostToDevice, ctx->copy_in_stream);
        if (el != hipSuccess) {
            (void)hipStreamSynchronize(ctx->copy_in_stream);
            return fail(ctx, AVK_E_HIP, "queueing the batch's copies failed: %s", hipGetErrorString(el));
        }
    }
    const struct { const void *src; void *dst; size_t bytes; } cp[] = {
        {batch->t_cnt, pre->t_cnt, n}, {batch->q_cnt, pre->q_cnt, n}, {batch->a0_len, pre->a0_len, nv}, {batch->a1_len, pre->a1_len, nv}, {batch->start, pre->start, n * 4},
        {batch->len, pre->len, n * 2}, {batch->contig_idx, pre->contig, has_contig ? n * 2 : 0}, {batch->var_rel_pos, pre->rel_pos, nv * 2}, {batch->var_type_zyg, pre->var_type_zyg, nv},
        {batch->var_raw_space, pre->raw, has_raw ? nv * 4 : 0}, {batch->allele_bytes, pre->alleles, alen}};
    hipError_t e = hipSuccess;
    for (const auto &c : cp)
        if (e == hipSuccess && c.bytes && c.src) e = hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyHostToDevice, ctx->copy_in_stream);
    if (e == hipSuccess) e = hipEventRecord(sl.ev_in, ctx->copy_in_stream);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(ctx->copy_in_stream);
        return fail(ctx, AVK_E_HIP, "queueing the batch's copies failed: %s", hipGetErrorString(e));
    }
    return 0;
}
static bool packed_inputs_pinned(const avk_packed_batch *batch, const avk_packed_escapes *esc = nullptr) {
    const uint64_t n = batch->n_regions, nv = batch->n_variants, alen = batch->allele_bytes_len;
    if (esc && !(is_pinned(esc->esc_region, esc->n_esc_regions * 8) && is_pinned(esc->esc_len, esc->n_esc_regions * 4) && is_pinned(esc->esc_slot, esc->n_esc_slots * 8) &&
                 is_pinned(esc->esc_cnt, esc->n_esc_slots * 4) && is_pinned(esc->esc_call, esc->n_esc_calls * 8) && is_pinned(esc->esc_rel_pos, esc->n_esc_calls * 4) &&
                 is_pinned(esc->esc_a0_len, esc->n_esc_calls * 4) && is_pinned(esc->esc_a1_len, esc->n_esc_calls * 4)))
        return false;
    return is_pinned(batch->t_cnt, n) && is_pinned(batch->q_cnt, n) && is_pinned(batch->a0_len, nv) && is_pinned(batch->a1_len, nv) && is_pinned(batch->start, n * 4) &&
           is_pinned(batch->len, n * 2) && is_pinned(batch->contig_idx, n * 2) && is_pinned(batch->var_rel_pos, nv * 2) && is_pinned(batch->var_type_zyg, nv) &&
           is_pinned(batch->var_raw_space, nv * 4) && is_pinned(batch->allele_bytes, alen);
}

static int submit_impl(avk_ctx *ctx, const avk_packed_batch *batch, const avk_compare_config *cfg, avk_result_batch *out, avk_ticket **ticket, uint32_t *shared_spill,
                       uint32_t *shared_spill_count, const avk_packed_escapes *esc = nullptr, const avk_region_labels *lab = nullptr, uint64_t *label_tallies = nullptr,
                       const avk_strata *st = nullptr);
int avk_compare_packed_submit(avk_ctx *ctx, const avk_packed_batch *batch, const avk_compare_config *cfg, avk_result_batch *out, avk_ticket **ticket) {
    return submit_impl(ctx, batch, cfg, out, ticket, nullptr, nullptr);
}
int avk_compare_packed_submit_esc(avk_ctx *ctx, const avk_packed_batch *batch, const avk_packed_escapes *esc, const avk_compare_config *cfg, avk_result_batch *out,
                                  avk_ticket **ticket) {
    return submit_impl(ctx, batch, cfg, out, ticket, nullptr, nullptr, esc);
}
/* shared_spill / shared_spill_count: the device list and counter the parts of one split call spill their BASEPAIR groups into (compare_packed_split); with them a
 * batch that returns the packed groups can be queued like any other.  st (avk_compare_packed_submit_strata, which has checked the handle): the labels come from
 * the resident sets — the packer's region passes run the mask pass, the tally reads the masks; lab is NULL then. */
static int submit_impl(avk_ctx *ctx, const avk_packed_batch *batch, const avk_compare_config *cfg, avk_result_batch *out, avk_ticket **ticket, uint32_t *shared_spill,
                       uint32_t *shared_spill_count, const avk_packed_escapes *esc, const avk_region_labels *lab, uint64_t *label_tallies, const avk_strata *st) {
    if (lab && lab->n_labels == 0) lab = nullptr; /* (no labels: the call without them, launch for launch) */
    if (st && st->n_labels == 0) st = nullptr;
    if (lab && batch) { /* (first of all: these refusals need no device, avk_last_error(NULL) has their text when ctx is NULL) */
        const int rl = labels_check(ctx, batch->n_regions, lab, label_tallies);
        if (rl) return rl;
    }
    if (!ctx || !batch || !cfg || !out || !ticket || !(out->status || out->region_packed)) return AVK_E_ARG;
    *ticket = nullptr;
    if (!esc_present(esc)) esc = nullptr;
    if (!esc_arrays_ok(esc)) return fail(ctx, AVK_E_ARG, "escape arrays missing");
    if (!ctx->d_ref) return fail(ctx, AVK_E_STATE, "avk_ref_upload has not been called");
    AVK_HIP(ctx, hipSetDevice(ctx->device));
    const uint64_t n = batch->n_regions, nv = batch->n_variants;
    if (n && (!batch->start || !batch->len || !batch->t_cnt || !batch->q_cnt)) return fail(ctx, AVK_E_ARG, "region arrays missing");
    if (nv && (!batch->var_rel_pos || !batch->var_type_zyg || !batch->a0_len || !batch->a1_len || !batch->allele_bytes)) return fail(ctx, AVK_E_ARG, "variant arrays missing");
    const bool timing = getenv("AVK_TIMING") != nullptr;
    static const auto t_epoch = std::chrono::steady_clock::now();
    auto now_ms = [&] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_epoch).count(); };
    const double ts0 = now_ms();
    avk_ticket *t = new avk_ticket();
    t->out = *out;
    /* arrays that are not pinned cannot be copied behind the caller's back: such a batch is solved here and now, its ticket is complete */
    bool pinned = packed_inputs_pinned(batch, esc);
    pinned = pinned && is_pinned(out->status, n * 4) && is_pinned(out->region_packed, n * 8) && is_pinned(out->ed_h1, n * 4) && is_pinned(out->ed_h2, n * 4) && is_pinned(out->n_optima, n * 4) &&
             is_pinned(out->type_present, n * 2) && is_pinned(out->var_expected, nv) && is_pinned(out->var_observed, nv) && is_pinned(out->var_class, nv) && is_pinned(out->var_zyg, nv) &&
             is_pinned(out->var_packed, nv) && is_pinned(out->group_metrics, n * AVK_N_GROUPS * AVK_N_FIELDS * 4);
    if (lab) pinned = pinned && is_pinned(lab->label_off, (n + 1) * 8) && is_pinned(lab->label_idx, lab->label_off[n] * 4);
    const bool seq_out = out->seq_bytes && out->seq_len && out->seq_off && out->seq_stride && cfg->enable_sequences;
    int slot = -1;
    const bool bp_words = out->bp_packed && out->bp_spilled && out->bp_groups && !out->bp_off;
    const bool bp_queueable = bp_words && shared_spill && shared_spill_count && is_pinned(out->bp_packed, n * 4);
    const bool can_queue = pinned && !seq_out && (bp_queueable || !((out->bp_off || out->bp_packed) && out->bp_groups));
    for (int i = 0; i < 4 && slot < 0 && can_queue; ++i)
        if (!ctx->stage[i].busy) {
            slot = i;
            break;
        }
    if (slot < 0 && can_queue) {
        delete t;
        return fail(ctx, AVK_E_STATE, "four batches are in flight: avk_wait for one of them first");
    }
    if (slot < 0) { /* solved here and now (it uses no staging slot): a complete ticket on success, no ticket on failure — the caller owns what it is handed */
        const int rc_now = lab  ? avk_compare_packed_labels(ctx, batch, esc, lab, cfg, out, label_tallies)
                           : st ? avk_compare_packed_strata(ctx, batch, esc, st, cfg, out, label_tallies)
                                : avk_compare_packed_esc(ctx, batch, esc, cfg, out);
        if (rc_now) {
            delete t;
            return rc_now;
        }
        t->rc = 0;
        *ticket = t;
        return AVK_E_OK;
    }
    avk_ctx::StageSlot &sl = ctx->stage[slot];
    PackedOnDevice pre;
    int rc = stage_layout(ctx, sl, batch, esc, &pre, lab);
    const size_t lab_words = (size_t)(lab ? lab->n_labels : st ? st->n_labels : 0) * AVK_TALLY_LEN;
    if (!rc && lab_words && sl.h_labels_words < lab_words) { /* the pinned block the sums land in */
        if (sl.h_labels) (void)hipHostFree(sl.h_labels);
        sl.h_labels = nullptr, sl.h_labels_words = 0;
        hipError_t eh = hipHostMalloc((void **)&sl.h_labels, lab_words * sizeof(uint64_t), hipHostMallocDefault);
        if (eh != hipSuccess) rc = fail(ctx, AVK_E_HIP, "pinned block of the label sums: %s", hipGetErrorString(eh));
        else sl.h_labels_words = lab_words;
    }
    if (!rc && st) { /* the masks of this batch and the workgroup counts the mask kernel writes beside them: the ticket's until avk_wait */
        rc = pool_alloc(ctx, &t->d_mask, (size_t)n * strata_words(st) * 4 + 16);
        if (!rc) rc = pool_alloc(ctx, &t->d_mask_sums, ((size_t)strata_blocks(n) + 1) * 8);
    }
    if (rc) {
        (void)hipStreamSynchronize(ctx->copy_in_stream);
        pool_release(ctx, t->d_mask), pool_release(ctx, t->d_mask_sums);
        delete t;
        return rc;
    }
    if (lab) t->has_lab = true, t->lab = *lab, t->lab_out = label_tallies;
    if (st) {
        t->has_strata = true, t->n_labels = st->n_labels, t->lab_out = label_tallies;
        t->sjob = StrataJob{st, (uint32_t *)t->d_mask, (uint64_t *)t->d_mask_sums};
        t->sjob.mask_only = true;
    }
    const double ts1 = now_ms();
    sl.busy = true;
    t->slot = slot;
    CallSpec spec = t->spec = call_spec(ctx, out, bp_queueable || lab || st); /* (the ticket keeps the emit flags; the packing streams and the mask job are this call's alone) */
    if (st) spec.strata = &t->sjob;
    t->later.h_tally = sl.h_tally, t->later.ev_unpacked = sl.ev_unpacked, t->later.ev_done = sl.ev_done;
    t->later.shared_spill = bp_queueable ? shared_spill : nullptr, t->later.shared_spill_count = bp_queueable ? shared_spill_count : nullptr;
    /* Packing on a stream of its own: its kernels stream the batch's arrays through HBM while the solver launches of the batch before are busy with their searches,
     * and the plan's round trip to the host no longer waits for that solve.  Pool buffers stay ordered: what this upload is handed was released either by an upload
     * (on this same stream) or by a batch whose work is over (avk_wait). */
    if (ctx->async_pack_stream) {
        spec.up_stream = ctx->pack_stream, spec.up_side = ctx->pack_side_stream;
        if (ctx->pool_fence_pending) { /* a synchronous upload released buffers behind kernels of the context's stream that may still be queued */
            (void)hipStreamWaitEvent(ctx->pack_stream, ctx->ev_pool_fence, 0);
            ctx->pool_fence_pending = false;
        }
    }
    rc = upload_device_packed(ctx, spec, UploadSource::of(batch, esc), &pre, &t->db);
    if (!rc && spec.up_stream) {
        hipError_t e = hipEventRecord(ctx->ev_packed, spec.up_stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(ctx->stream, ctx->ev_packed, 0);
        if (e != hipSuccess) rc = fail(ctx, AVK_E_HIP, "packed upload: %s", hipGetErrorString(e));
    }
    const double ts2 = now_ms();
    if (!rc) rc = run_internal(ctx, spec, t->db, cfg, nullptr, 0);
    if (!rc && st && n && !t->sjob.counted) rc = fail(ctx, AVK_E_STATE, "strata masks: the upload did not make them");
    if (!rc && st) { /* behind the solve's tally reduce: the label kernel on the masks, its sums cross with the results */
        const size_t words = (size_t)st->n_labels * AVK_TALLY_LEN;
        rc = pool_alloc(ctx, &t->d_lab_out, words * sizeof(uint64_t));
        if (!rc) rc = label_sums_queue(ctx, t->db, nullptr, nullptr, st->n_labels, (uint64_t *)t->d_lab_out, true, nullptr, (const uint32_t *)t->d_mask);
        t->later.lab_dev = t->d_lab_out, t->later.lab_host = sl.h_labels, t->later.lab_bytes = words * sizeof(uint64_t);
    }
    if (!rc && lab) { /* behind the solve's tally reduce: the label kernel, its sums cross with the results */
        const size_t words = (size_t)lab->n_labels * AVK_TALLY_LEN;
        rc = pool_alloc(ctx, &t->d_lab_out, words * sizeof(uint64_t));
        if (!rc) rc = label_sums_queue(ctx, t->db, pre.lab_off, pre.lab_idx, lab->n_labels, (uint64_t *)t->d_lab_out, true, nullptr);
        t->later.lab_dev = t->d_lab_out, t->later.lab_host = sl.h_labels, t->later.lab_bytes = words * sizeof(uint64_t);
    }
    const double ts3 = now_ms();
    if (!rc) rc = results_download_impl(ctx, spec, t->db, out, &t->later, nullptr);
    if (timing)
        fprintf(stderr, "avk submit (slot %d): called at %.3f ms; copies queued +%.3f, packed and planned +%.3f, solver launches queued +%.3f, results queued +%.3f\n", slot, ts0, ts1 - ts0,
                ts2 - ts0, ts3 - ts0, now_ms() - ts0);
    if (rc) { /* nothing of this batch stays in flight */
        (void)hipStreamSynchronize(ctx->copy_in_stream);
        (void)hipStreamSynchronize(ctx->pack_stream);
        (void)hipStreamSynchronize(ctx->pack_side_stream);
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipStreamSynchronize(ctx->copy_out_stream);
        for (void *p : t->later.temps) pool_release(ctx, p);
        if (t->d_lab_out) pool_release(ctx, t->d_lab_out);
        pool_release(ctx, t->d_mask), pool_release(ctx, t->d_mask_sums);
        if (t->db) avk_batch_free(ctx, t->db);
        sl.busy = false;
        delete t;
        return rc;
    }
    if (st) { /* the handle counts this batch until avk_wait; avk_strata_free meanwhile waits for the stream the mask pass ran on */
        t->sjob.st = nullptr;
        t->strata_use = st->use;
        StrataUse &u = *t->strata_use;
        const hipStream_t ms = spec.up_stream ? spec.up_stream : ctx->stream;
        u.in_flight += 1;
        if (std::find(u.streams.begin(), u.streams.end(), ms) == u.streams.end()) u.streams.push_back(ms);
    }
    ctx->last_one_shot = 1;
    *ticket = t;
    return 0;
}

int avk_wait(avk_ctx *ctx, avk_ticket *t) {
    if (!ctx || !t) return AVK_E_ARG;
    if (t->slot < 0) { /* solved at submit */
        const int rc = t->rc;
        delete t;
        return rc;
    }
    (void)hipSetDevice(ctx->device);
    avk_ctx::StageSlot &sl = ctx->stage[t->slot];
    const auto tw0 = std::chrono::steady_clock::now();
    hipError_t e = hipEventSynchronize(sl.ev_done);
    const auto tw1 = std::chrono::steady_clock::now();
    int rc = e == hipSuccess ? 0 : fail(ctx, AVK_E_HIP, "waiting for the batch's results failed: %s", hipGetErrorString(e));
    if (!rc) { /* the tally, the statistics and — should a region have come back AVK_ST_CAPACITY — the retry, as in avk_results_download */
        LabelFix lf{t->has_strata ? nullptr : &t->lab, t->lab_out};
        if (t->has_strata) lf.d_mask = (const uint32_t *)t->d_mask, lf.n_words = (t->n_labels + 31u) / 32u, lf.n = t->db->n_regions; /* a repaired region's labels: its own mask words */
        CallSpec spec = t->spec;
        if (t->has_lab || t->has_strata) spec.label_fix = &lf; /* (a region the retry repairs was not solved when the label kernel ran) */
        rc = results_download_impl(ctx, spec, t->db, &t->out, nullptr, sl.h_tally);
        if (!rc && lf.err != hipSuccess) rc = fail(ctx, AVK_E_HIP, "label tallies: the mask words of the regions the capacity retry repaired could not be fetched: %s", hipGetErrorString(lf.err));
        if (!rc && t->has_strata) {
            const size_t words = (size_t)t->n_labels * AVK_TALLY_LEN;
            for (size_t k = 0; k < words; ++k) t->lab_out[k] += sl.h_labels[k];
            labels_timing_print(ctx, "submitted, masks", t->n_labels, t->db->n_regions, 0);
        }
        if (!rc && t->has_lab) {
            const size_t words = (size_t)t->lab.n_labels * AVK_TALLY_LEN;
            for (size_t k = 0; k < words; ++k) t->lab_out[k] += sl.h_labels[k];
            labels_timing_print(ctx, "submitted", t->lab.n_labels, t->db->n_regions, t->lab.label_off[t->db->n_regions]);
        }
    }
    if (t->d_lab_out) pool_release(ctx, t->d_lab_out);
    pool_release(ctx, t->d_mask), pool_release(ctx, t->d_mask_sums);
    if (t->strata_use && --t->strata_use->in_flight == 0) t->strata_use->streams.clear();
    /* the batch's buffers go back to the pool: its work is over (the copies out ran behind its last kernel), so whoever is handed them next may use them at once */
    for (void *p : t->later.temps) pool_release(ctx, p);
    if (t->db) {
        release_pooled(ctx, t->db);
        delete t->db;
    }
    sl.busy = false;
    if (getenv("AVK_TIMING"))
        fprintf(stderr, "avk wait (slot %d): results arrived after %.3f ms, tally and buffers %.3f ms\n", t->slot, std::chrono::duration<double, std::milli>(tw1 - tw0).count(),
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tw1).count());
    delete t;
    return rc;
}

int avk_last_compare_was_one_shot(avk_ctx *ctx) { return ctx ? ctx->last_one_shot : 0; }

} /* extern "C" */
#include "avk_shard_host.inl"
extern "C" {

/* pinned host memory for the caller's batch and result arrays: arrays that live there are copied by DMA, no host pass (pageable arrays go through
 * a pinned bounce buffer that the host threads fill) */
void *avk_host_alloc(avk_ctx *ctx, size_t bytes) {
    if (ctx) (void)hipSetDevice(ctx->device);
    void *p = nullptr;
    if (bytes == 0) bytes = 16;
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        if (ctx) fail(ctx, AVK_E_OOM, "cannot pin %zu bytes of host memory", bytes);
        return nullptr;
    }
    std::lock_guard<std::mutex> lk(g_pinned_mutex);
    g_pinned.push_back({(const uint8_t *)p, (const uint8_t *)p + bytes});
    return p;
}

void avk_host_free(avk_ctx *ctx, void *p) {
    if (!p) return;
    if (ctx) {
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
    }
    {
        std::lock_guard<std::mutex> lk(g_pinned_mutex);
        for (size_t i = 0; i < g_pinned.size(); ++i)
            if (g_pinned[i].lo == (const uint8_t *)p) {
                g_pinned.erase(g_pinned.begin() + (long)i);
                break;
            }
    }
    (void)hipHostFree(p);
}

/* what a batch of this size will need, ahead of the first call: the pinned bounce buffer for pageable arrays (callers whose arrays come from
 * avk_host_alloc need none) and the device buffers of the pool */
int avk_ctx_reserve(avk_ctx *ctx, uint64_t n_regions, uint64_t n_variants) {
    if (!ctx) return AVK_E_ARG;
    if (n_regions > 0x7FFFFFFFull || n_variants > 0x7FFFFFFFull) return 0;
    AVK_HIP(ctx, hipSetDevice(ctx->device));
    return bounce_reserve(ctx, (size_t)n_regions * 52 + (size_t)n_variants * 48 + (1u << 20));
}

/* What a process's FIRST large call pays for beyond the call itself, done ahead of it (a tool: on a thread beside its parsing): the device code is brought in by a
 * launch of nothing, the table of the looked-up class is made for the default branch factor, and the workspaces of a batch of that size are allocated (7 GB for a
 * genome; fresh device memory is scrubbed when it is handed out).  Nothing here changes a result; every step is also made on demand by the call that needs it. */
/* a small call through every kind of launch on a context of its own (the caller's may be taking its reference at this moment): a kernel's FIRST launch in a
 * process costs about a millisecond — the dozen packing kernels of a first whole-genome call took 16 ms instead of 1.5 */
static void warm_kernels(int device) {
    avk_ctx *t = nullptr;
    if (avk_ctx_create(device, &t) || !t) return;
    const char *opts[] = {"lane_min_regions", "lane_min_batch", "emit_group_metrics", "adaptive_ws"}; /* (adaptive_ws 0: with the class C threshold below the packer
                                                                                                          would predict, and this context allocate, tens of GB of slices) */
    for (const char *o : opts) (void)avk_ctx_set_option(t, o, 0);
    (void)avk_ctx_set_option(t, "big_ws_bytes", 8 << 20);
    (void)avk_ctx_set_option(t, "ws_bytes_per_wave", 256 << 10); /* (the warm-up's regions are tiny: 0.4 GB of slices instead of 1.7 — what this context frees at its end is
                                                                   memory the caller's first call may be handed next, and has to wait for while it is scrubbed) */
    (void)avk_ctx_set_option(t, "class_c_nodes_x2", 1000); /* every region the lanes do not take is planned as class C: the wide kernel, the HBM launches */
    (void)avk_ctx_set_option(t, "lane_node_cap", 8);       /* ... and the three-call class hands back (8: the option's smallest value) */
    const uint32_t L = 120, n_contig = 1u << 16;
    std::vector<uint8_t> contig(n_contig);
    uint32_t x = 12345u;
    for (uint32_t i = 0; i < n_contig; ++i) {
        x = x * 1664525u + 1013904223u;
        contig[i] = "ACGT"[x >> 30];
    }
    std::vector<uint32_t> start;
    std::vector<uint16_t> len, rel;
    std::vector<uint8_t> tc, qc, tz, a0l, a1l, alle;
    auto other = [](uint8_t b) { return (uint8_t)(b == 'A' ? 'C' : 'A'); };
    for (uint32_t r = 0; r < 448; ++r) { /* calls per side: 1 (the looked-up class and its neighbours), 2, 3, 5 */
        const uint32_t per = r < 256 ? 1u : (r < 320 ? 2u : (r < 384 ? 3u : 5u)), s0 = 100u + r * 140u;
        start.push_back(s0), len.push_back((uint16_t)L), tc.push_back((uint8_t)per), qc.push_back((uint8_t)per);
        for (uint32_t side = 0; side < 2; ++side)
            for (uint32_t k = 0; k < per; ++k) {
                const uint32_t p = 10u + 20u * k;
                rel.push_back((uint16_t)p);
                tz.push_back((uint8_t)(AVK_VT_SNV | ((r & 1u ? AVK_ZYG_UNPHASED_HET : AVK_ZYG_HOM_ALT) << 4)));
                a0l.push_back(1), a1l.push_back(1);
                alle.push_back(contig[s0 + p]);
                alle.push_back(side && (r & 2u) && k == 0 ? (uint8_t)(other(contig[s0 + p]) == 'C' ? 'G' : 'T') : other(contig[s0 + p]));
            }
    }
    avk_packed_batch b;
    memset(&b, 0, sizeof(b));
    b.n_regions = start.size(), b.start = start.data(), b.len = len.data(), b.t_cnt = tc.data(), b.q_cnt = qc.data();
    b.n_variants = rel.size(), b.var_rel_pos = rel.data(), b.var_type_zyg = tz.data(), b.a0_len = a0l.data(), b.a1_len = a1l.data();
    b.allele_bytes = alle.data(), b.allele_bytes_len = alle.size();
    std::vector<int32_t> status(b.n_regions);
    std::vector<uint32_t> e1(b.n_regions), e2(b.n_regions), no(b.n_regions);
    std::vector<uint16_t> tp(b.n_regions);
    std::vector<uint8_t> ve(b.n_variants), vo(b.n_variants), vc(b.n_variants), vz(b.n_variants);
    std::vector<uint64_t> tally(AVK_TALLY_LEN);
    avk_result_batch out;
    memset(&out, 0, sizeof(out));
    out.status = status.data(), out.ed_h1 = e1.data(), out.ed_h2 = e2.data(), out.n_optima = no.data(), out.type_present = tp.data();
    out.var_expected = ve.data(), out.var_observed = vo.data(), out.var_class = vc.data(), out.var_zyg = vz.data(), out.tally = tally.data();
    const uint8_t *seqs[1] = {contig.data()};
    const uint64_t lens[1] = {n_contig};
    avk_compare_config cfg = {50, 0, 0};
    if (avk_ref_upload(t, 1, seqs, lens) == 0) (void)avk_compare_packed(t, &b, &cfg, &out);
    avk_ctx_destroy(t);
}

int avk_ctx_warmup(avk_ctx *ctx, uint64_t n_regions_hint, uint64_t n_variants_hint) {
    if (!ctx) return AVK_E_ARG;
    AVK_HIP(ctx, hipSetDevice(ctx->device));
    int rc = avk_ctx_reserve(ctx, n_regions_hint, n_variants_hint);
    if (rc) return rc;
    warm_kernels(ctx->device);
    unsigned *d_scratch = nullptr;
    struct ScratchGuard { /* released on every way out, the AVK_HIP early returns included */
        unsigned *&p;
        ~ScratchGuard() {
            if (p) (void)hipFree(p);
            p = nullptr;
        }
    } scratch_guard{d_scratch};
    AVK_HIP(ctx, hipMalloc((void **)&d_scratch, (size_t)AVK_TALLY_STRIDE * (AVK_TALLY_COPIES + 1) * sizeof(uint64_t) + AVK_N_COUNTERS * sizeof(uint32_t)));
    AVK_HIP(ctx, hipMemsetAsync(d_scratch, 0, (size_t)AVK_TALLY_STRIDE * (AVK_TALLY_COPIES + 1) * sizeof(uint64_t) + AVK_N_COUNTERS * sizeof(uint32_t), ctx->stream));
    uint64_t *parts = (uint64_t *)d_scratch;
    hipLaunchKernelGGL(avk_tally_reduce, dim3((AVK_TALLY_STRIDE + 63) / 64), dim3(64), 0, ctx->stream, parts, parts + (size_t)AVK_TALLY_STRIDE * AVK_TALLY_COPIES, (uint64_t *)nullptr,
                       (uint32_t *)(parts + (size_t)AVK_TALLY_STRIDE * (AVK_TALLY_COPIES + 1)), (unsigned)AVK_N_COUNTERS, 0u);
    AVK_HIP(ctx, hipGetLastError());
    rc = ensure_kernel_attrs(ctx);
    if (rc) return rc;
    if (ctx->lane_kernel && ctx->lane_pairs) {
        rc = ensure_pair_table(ctx, 50, ctx->stream);
        if (rc) return rc;
    }
    if (n_regions_hint >= 65536 && ctx->ws_bytes_per_wave > 0) {
        /* The workspaces the step (avk_step_geometry.h) sizes for a batch of a genome's size, allocated HERE, on the thread that runs beside the caller's parsing: hipMalloc of the
         * 4.8 + 2.1 GB they were until round 5 took 0.39 s (device memory is scrubbed when it is handed out).  Round 4 took and released as many bytes instead, counting on memory the process has
         * held once to come back at once: it does in two runs of three — in the third the first call's own hipMalloc paid the 0.39 s inside the tool's solve stage
         * (profiles/r05_first_solve.txt: "avk run: workspaces (.. allocated now ..) 387 ms"). */
        /* (a genome has lane launches, which leave the other kernels a few thousand regions) */
        const AvkStepGeometryIn gin = {ctx->n_cus, ctx->waves_per_cu, 16384, 0, true, ctx->ws_bytes_per_wave, ctx->ws_budget_bytes, ctx->hbm_solo_blocks, ctx->hbm_early_blocks, ctx->big_waves, ctx->big_ws_bytes};
        const AvkStepGeometry geo = avk_step_geometry(gin);
        const size_t ws_need = geo.ws_need, big_need = geo.big_need;
        if (ws_need > ctx->ws_alloc && !geo.shrunk) { /* (slices past the budget: the step that has them sizes them) */
            if (ctx->d_ws) (void)hipFree(ctx->d_ws);
            ctx->d_ws = nullptr, ctx->ws_alloc = 0;
            if (hipMalloc((void **)&ctx->d_ws, ws_need + 256) == hipSuccess) ctx->ws_alloc = ws_need;
            else ctx->d_ws = nullptr, (void)hipGetLastError(); /* (the first call asks again, and reports) */
        }
        if (ctx->big_ws_bytes > 0 && big_need > ctx->big_alloc) {
            if (ctx->d_big) (void)hipFree(ctx->d_big);
            ctx->d_big = nullptr, ctx->big_alloc = 0;
            if (hipMalloc((void **)&ctx->d_big, big_need + 256) == hipSuccess) ctx->big_alloc = big_need;
            else ctx->d_big = nullptr, (void)hipGetLastError();
        }
    }
    if (n_regions_hint >= 65536 && ctx->device_pack) {
        /* ... and the largest of the batch's own buffers, taken from the context's pool and put back: the first call finds them cached (a cached buffer serves requests
         * of half its size and more, so the hints only have to be about right).  Without them a process's first whole-genome call waited 0.1 s inside one hipMalloc — the
         * 675 MB arena of the region blobs (profiles/r05_first_solve.txt).  AVK_WARM_POOL=1 takes and clears every buffer of the batch instead. */
        if (getenv("AVK_WARM_POOL")) {
            rc = pool_prewarm(ctx, n_regions_hint, n_variants_hint);
            if (rc) return rc;
        } else {
            const size_t n = (size_t)n_regions_hint, nv = (size_t)n_variants_hint;
            const size_t sizes[] = {n * 190, n * 64, n * 64, n * 52, nv * 16, nv * 16, nv * 8, nv * 8, nv * 8}; /* blobs, region records, region info, fast records, call info and slots, positions and allele offsets */
            std::vector<void *> got;
            for (size_t b : sizes) {
                void *p = nullptr;
                if (pool_alloc(ctx, &p, b)) break;
                got.push_back(p);
            }
            for (void *p : got) pool_release(ctx, p);
        }
    }
    AVK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

static int upload_compact(avk_ctx *ctx, const CallSpec &spec, const avk_compact_batch *batch, avk_dev_batch **out) {
    if (!ctx || !batch || !out) return AVK_E_ARG;
    *out = nullptr;
    if (!ctx->d_ref) return fail(ctx, AVK_E_STATE, "avk_ref_upload has not been called");
    AVK_HIP(ctx, hipSetDevice(ctx->device));
    return upload_device_packed(ctx, spec, UploadSource::of(batch), nullptr, out);
}
int avk_batch_upload_compact(avk_ctx *ctx, const avk_compact_batch *batch, avk_dev_batch **out) { return ctx ? upload_compact(ctx, call_spec(ctx), batch, out) : AVK_E_ARG; }

static int upload_packed(avk_ctx *ctx, const CallSpec &spec, const avk_packed_batch *batch, const avk_packed_escapes *esc, avk_dev_batch **out) {
    if (!ctx || !batch || !out) return AVK_E_ARG;
    *out = nullptr;
    if (!ctx->d_ref) return fail(ctx, AVK_E_STATE, "avk_ref_upload has not been called");
    AVK_HIP(ctx, hipSetDevice(ctx->device));
    return upload_device_packed(ctx, spec, UploadSource::of(batch, esc), nullptr, out);
}
int avk_batch_upload_packed_esc(avk_ctx *ctx, const avk_packed_batch *batch, const avk_packed_escapes *esc, avk_dev_batch **out) {
    return ctx ? upload_packed(ctx, call_spec(ctx), batch, esc, out) : AVK_E_ARG;
}
int avk_batch_upload_packed(avk_ctx *ctx, const avk_packed_batch *batch, avk_dev_batch **out) { return avk_batch_upload_packed_esc(ctx, batch, nullptr, out); }

/* One large call as `parts` batches in flight (context option split_parts; avk_compare_packed below): the regions are independent (src/main.rs:251-268 maps over
 * them), so the batch is cut into ranges of regions — the packed form has no explicit offsets, a range of regions with its calls and allele bytes is a packed batch of
 * its own — that go through the staging slots of the asynchronous boundary: the arrays of part k + 1 cross the bus and are packed while part k is solved, the results of
 * part k cross while part k + 1 is solved.  Same outputs, byte for byte: per-region and per-call arrays land at the parts' places in the caller's arrays, the tallies are
 * added, the parts' spilled BASEPAIR groups form one list (one device buffer, one counter).  Returns -1 when the call does not qualify (the caller then runs it whole). */
static int compare_packed_split(avk_ctx *ctx, const avk_packed_batch *batch, const avk_compare_config *cfg, avk_result_batch *out) {
    const uint64_t n = batch->n_regions, nv = batch->n_variants;
    int64_t parts = ctx->split_parts;
    if (parts > 4) parts = 4;
    if (parts < 2 || !ctx->async_pack_stream || n / (uint64_t)parts < 4096) return -1;
    if (cfg->enable_sequences && out->seq_bytes) return -1;
    if (out->bp_off || (out->bp_packed && !(out->bp_spilled && out->bp_groups)) || out->group_metrics) return -1;
    for (int i = 0; i < 4; ++i)
        if (ctx->stage[i].busy) return -1; /* batches of the caller's are in flight: the slots are theirs */
    if (!packed_inputs_pinned(batch)) return -1;
    if (!(is_pinned(out->status, n * 4) && is_pinned(out->region_packed, n * 8) && is_pinned(out->ed_h1, n * 4) && is_pinned(out->ed_h2, n * 4) && is_pinned(out->n_optima, n * 4) &&
          is_pinned(out->type_present, n * 2) && is_pinned(out->var_expected, nv) && is_pinned(out->var_observed, nv) && is_pinned(out->var_class, nv) && is_pinned(out->var_zyg, nv) &&
          is_pinned(out->var_packed, nv) && is_pinned(out->bp_packed, n * 4)))
        return -1;
    const bool want_bp = out->bp_packed != nullptr;
    /* where the parts begin: regions in equal shares, their calls and allele bytes by the running sums the packed form implies (host threads: two byte arrays read once) */
    uint64_t r0[5], v0[5], a0[5];
    for (int k = 0; k <= parts; ++k) r0[k] = n * (uint64_t)k / (uint64_t)parts;
    v0[0] = a0[0] = 0;
    {
        const unsigned threads = avk_host_threads();
        for (int k = 0; k < parts; ++k) {
            std::vector<uint64_t> partial(threads + 1, 0);
            avk_parallel_for(r0[k + 1] - r0[k], threads, [&](unsigned t, uint64_t lo, uint64_t hi) {
                uint64_t sum = 0;
                for (uint64_t r = r0[k] + lo; r < r0[k] + hi; ++r) sum += (uint64_t)batch->t_cnt[r] + batch->q_cnt[r];
                partial[t] += sum;
            });
            uint64_t calls = 0;
            for (uint64_t x : partial) calls += x;
            v0[k + 1] = v0[k] + calls;
            if (v0[k + 1] > nv) return fail(ctx, AVK_E_ARG, "packed batch: the call counts sum to more than n_variants %llu", (unsigned long long)nv);
            std::fill(partial.begin(), partial.end(), 0);
            avk_parallel_for(calls, threads, [&](unsigned t, uint64_t lo, uint64_t hi) {
                uint64_t sum = 0;
                for (uint64_t v = v0[k] + lo; v < v0[k] + hi; ++v) sum += (uint64_t)batch->a0_len[v] + batch->a1_len[v];
                partial[t] += sum;
            });
            uint64_t bytes = 0;
            for (uint64_t x : partial) bytes += x;
            a0[k + 1] = a0[k] + bytes;
        }
        if (v0[parts] != nv || a0[parts] != batch->allele_bytes_len)
            return fail(ctx, AVK_E_ARG, "packed batch: the call counts sum to %llu (n_variants %llu), the allele lengths to %llu (allele_bytes_len %llu)", (unsigned long long)v0[parts],
                        (unsigned long long)nv, (unsigned long long)a0[parts], (unsigned long long)batch->allele_bytes_len);
    }
    uint32_t *d_spill = nullptr, *d_count = nullptr;
    if (want_bp) { /* every region has at most 1 + its calls groups */
        int rc = pool_alloc(ctx, (void **)&d_spill, (size_t)(n + nv + 1) * 16);
        if (!rc) rc = pool_alloc(ctx, (void **)&d_count, 256);
        if (!rc && hipMemsetAsync(d_count, 0, 4, ctx->stream) != hipSuccess) rc = fail(ctx, AVK_E_HIP, "split call: %s", hipGetErrorString(hipGetLastError()));
        if (rc) {
            if (d_spill) pool_release(ctx, d_spill);
            if (d_count) pool_release(ctx, d_count);
            return rc;
        }
        out->bp_spilled[0] = 0;
    }
    avk_ticket *tickets[4] = {nullptr, nullptr, nullptr, nullptr};
    std::vector<uint64_t> part_tally((size_t)parts * AVK_TALLY_LEN, 0);
    int rc = 0;
    int queued = 0;
    for (int k = 0; k < parts && !rc; ++k) {
        avk_packed_batch pb = *batch;
        pb.n_regions = r0[k + 1] - r0[k], pb.n_variants = v0[k + 1] - v0[k], pb.allele_bytes_len = a0[k + 1] - a0[k];
        pb.contig_idx = batch->contig_idx ? batch->contig_idx + r0[k] : nullptr;
        pb.start = batch->start + r0[k], pb.len = batch->len + r0[k], pb.t_cnt = batch->t_cnt + r0[k], pb.q_cnt = batch->q_cnt + r0[k];
        pb.var_rel_pos = batch->var_rel_pos + v0[k], pb.var_type_zyg = batch->var_type_zyg + v0[k], pb.a0_len = batch->a0_len + v0[k], pb.a1_len = batch->a1_len + v0[k];
        pb.var_raw_space = batch->var_raw_space ? batch->var_raw_space + v0[k] : nullptr;
        pb.allele_bytes = batch->allele_bytes + a0[k];
        avk_result_batch po = *out;
#define AVK_PART(field, at) po.field = out->field ? out->field + (at) : nullptr
        AVK_PART(status, r0[k]), AVK_PART(region_packed, r0[k]), AVK_PART(ed_h1, r0[k]), AVK_PART(ed_h2, r0[k]), AVK_PART(n_optima, r0[k]), AVK_PART(type_present, r0[k]);
        AVK_PART(var_expected, v0[k]), AVK_PART(var_observed, v0[k]), AVK_PART(var_class, v0[k]), AVK_PART(var_zyg, v0[k]), AVK_PART(var_packed, v0[k]);
        AVK_PART(bp_packed, r0[k]);
#undef AVK_PART
        po.tally = part_tally.data() + (size_t)k * AVK_TALLY_LEN;
        rc = submit_impl(ctx, &pb, cfg, &po, &tickets[k], d_spill, d_count);
        if (!rc) queued = k + 1;
    }
    /* everything of every part is on the device's queues; the spilled groups' count and the list itself once the last part's results have crossed */
    if (!rc && queued == parts && want_bp) {
        hipError_t e = tickets[parts - 1]->slot >= 0 ? hipEventSynchronize(ctx->stage[tickets[parts - 1]->slot].ev_done) : hipSuccess;
        for (int k = 0; k + 1 < parts && e == hipSuccess; ++k)
            if (tickets[k]->slot >= 0) e = hipEventSynchronize(ctx->stage[tickets[k]->slot].ev_done);
        uint32_t spilled = 0;
        if (e == hipSuccess) e = hipMemcpyAsync(&spilled, d_count, 4, hipMemcpyDeviceToHost, ctx->copy_out_stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->copy_out_stream);
        if (e == hipSuccess && spilled) e = hipMemcpyAsync(out->bp_groups, d_spill, (size_t)spilled * 16, hipMemcpyDeviceToHost, ctx->copy_out_stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->copy_out_stream);
        if (e != hipSuccess) rc = fail(ctx, AVK_E_HIP, "split call: %s", hipGetErrorString(e));
        out->bp_spilled[0] = spilled; /* (a part's capacity repair, should there be one, appends behind these: avk_wait below) */
    }
    uint64_t tiers[5] = {0, 0, 0, 0, 0}, lane_solved = 0, wide_solved = 0;
    for (int k = 0; k < queued; ++k) {
        const int rw = avk_wait(ctx, tickets[k]);
        if (rw && !rc) rc = rw;
        for (int i = 0; i < 5; ++i) tiers[i] += ctx->last_tiers[i];
        lane_solved += ctx->last_lane_solved, wide_solved += ctx->last_wide_solved;
    }
    if (d_spill) pool_release(ctx, d_spill);
    if (d_count) pool_release(ctx, d_count);
    if (rc) return rc;
    memcpy(ctx->last_tiers, tiers, sizeof(tiers));
    ctx->last_lane_solved = lane_solved, ctx->last_wide_solved = wide_solved;
    if (out->tally) {
        memset(out->tally, 0, AVK_TALLY_LEN * sizeof(uint64_t));
        for (int k = 0; k < parts; ++k)
            for (int i = 0; i < AVK_TALLY_LEN; ++i) out->tally[i] += part_tally[(size_t)k * AVK_TALLY_LEN + i];
    }
    ctx->last_one_shot = 1;
    return 0;
}

int avk_compare_packed(avk_ctx *ctx, const avk_packed_batch *batch, const avk_compare_config *cfg, avk_result_batch *out) {
    return avk_compare_packed_esc(ctx, batch, nullptr, cfg, out);
}
int avk_dwfa_script_batch(avk_ctx *ctx, int engine, uint32_t n_scripts, const uint8_t *bytes, uint64_t n_bytes, const uint64_t *base_off, const uint64_t *other_off,
                          const uint64_t *step_off, const uint8_t *step_op, const uint32_t *step_blen, const uint32_t *step_olen, uint32_t *step_ed,
                          int32_t *step_status, uint32_t wf_cap, uint32_t *final_wf, uint32_t *final_wf_len) {
    if (!ctx || !bytes || !base_off || !other_off || !step_off || !step_op || !step_blen || !step_olen || !step_ed || !step_status) return AVK_E_ARG;
    if (engine != 0 && engine != 1) return fail(ctx, AVK_E_ARG, "engine must be 0 (wave per script) or 1 (lane per script)");
    if (n_scripts == 0) return 0;
    if (wf_cap < 3) return fail(ctx, AVK_E_ARG, "wf_cap must be at least 3");
    AVK_HIP(ctx, hipSetDevice(ctx->device));
    const uint64_t n_steps = step_off[n_scripts];
    for (uint32_t s = 0; s < n_scripts; ++s) {
        if (step_off[s + 1] < step_off[s] || base_off[s] > n_bytes || other_off[s] > n_bytes) return fail(ctx, AVK_E_ARG, "script %u: offsets out of range", s);
        for (uint64_t k = step_off[s]; k < step_off[s + 1]; ++k)
            if (step_op[k] > 1 || base_off[s] + step_blen[k] > n_bytes || other_off[s] + step_olen[k] > n_bytes)
                return fail(ctx, AVK_E_ARG, "script %u: a step reads past the byte arena", s);
    }
    AvkDwfaArgs a;
    memset(&a, 0, sizeof(a));
    a.wf_cap = wf_cap;
    a.n_scripts = n_scripts;
    std::vector<void *> allocs;
    auto up = [&](const void *src, size_t nbytes, void **dst) -> hipError_t {
        hipError_t e = hipMalloc(dst, nbytes ? nbytes : 16);
        if (e != hipSuccess) return e;
        allocs.push_back(*dst);
        return nbytes && src ? hipMemcpyAsync(*dst, src, nbytes, hipMemcpyHostToDevice, ctx->stream) : hipSuccess;
    };
    hipError_t e = up(bytes, n_bytes, (void **)&a.bytes);
    if (e == hipSuccess) e = up(base_off, n_scripts * sizeof(uint64_t), (void **)&a.base_off);
    if (e == hipSuccess) e = up(other_off, n_scripts * sizeof(uint64_t), (void **)&a.other_off);
    if (e == hipSuccess) e = up(step_off, (n_scripts + 1) * sizeof(uint64_t), (void **)&a.step_off);
    if (e == hipSuccess) e = up(step_op, n_steps, (void **)&a.step_op);
    if (e == hipSuccess) e = up(step_blen, n_steps * sizeof(uint32_t), (void **)&a.step_blen);
    if (e == hipSuccess) e = up(step_olen, n_steps * sizeof(uint32_t), (void **)&a.step_olen);
    if (e == hipSuccess) e = up(nullptr, n_steps * sizeof(uint32_t), (void **)&a.step_ed);
    if (e == hipSuccess) e = up(nullptr, n_steps * sizeof(int32_t), (void **)&a.step_status);
    if (e == hipSuccess && final_wf) e = up(nullptr, (size_t)n_scripts * wf_cap * sizeof(uint32_t), (void **)&a.final_wf);
    if (e == hipSuccess && final_wf_len) e = up(nullptr, (size_t)n_scripts * sizeof(uint32_t), (void **)&a.final_wf_len);
    if (e == hipSuccess && engine == 0) e = up(nullptr, (size_t)n_scripts * wf_cap * sizeof(uint32_t), (void **)&a.ws);
    if (e == hipSuccess) {
        if (engine == 0) hipLaunchKernelGGL(avk_dwfa_wave_kernel, dim3((n_scripts + 3) / 4), dim3(256), 0, ctx->stream, a);
        else hipLaunchKernelGGL(avk_dwfa_lane_kernel, dim3((n_scripts + 63) / 64), dim3(64), (size_t)(3 * (AVK_DWFA_LANE_W + 1) + 3 * ((2 * AVK_DWFA_LANE_ED + 2 + 3) / 4)) * 256, ctx->stream, a);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(step_ed, a.step_ed, n_steps * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(step_status, a.step_status, n_steps * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && final_wf) e = hipMemcpyAsync(final_wf, a.final_wf, (size_t)n_scripts * wf_cap * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && final_wf_len) e = hipMemcpyAsync(final_wf_len, a.final_wf_len, (size_t)n_scripts * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    for (void *p : allocs) (void)hipFree(p);
    if (e != hipSuccess) return fail(ctx, AVK_E_HIP, "avk_dwfa_script_batch failed: %s", hipGetErrorString(e));
    return 0;
}

int avk_label_tallies(avk_ctx *ctx, avk_dev_batch *db, uint32_t n_labels, const uint64_t *label_off, const uint32_t *label_idx, uint64_t *out) {
    if (!ctx || !db || !label_off || !out || (label_off[db->n_regions] && !label_idx)) return AVK_E_ARG;
    if (n_labels == 0) return 0;
    if (!db->d_gm) return fail(ctx, AVK_E_STATE, "the batch has no per-region metric blocks on the device: set emit_group_metrics before avk_compare_resident");
    AVK_HIP(ctx, hipSetDevice(ctx->device));
    const uint64_t n = db->n_regions, n_idx = label_off[n];
    for (uint64_t r = 0; r < n; ++r)
        if (label_off[r + 1] < label_off[r]) return fail(ctx, AVK_E_ARG, "label_off must not decrease");
    for (uint64_t q = 0; q < n_idx; ++q)
        if (label_idx[q] >= n_labels) return fail(ctx, AVK_E_ARG, "label index %u of %u", label_idx[q], n_labels);
    unsigned long long *d_off = nullptr, *d_out = nullptr;
    uint32_t *d_idx = nullptr;
    int rc = dev_alloc(ctx, &d_off, (size_t)n + 1);
    if (!rc) rc = dev_alloc(ctx, &d_idx, (size_t)n_idx);
    if (!rc) rc = dev_alloc(ctx, &d_out, (size_t)n_labels * AVK_TALLY_LEN);
    std::vector<uint64_t> host((size_t)n_labels * AVK_TALLY_LEN, 0);
    hipError_t e = hipSuccess;
    if (!rc) {
        e = hipMemcpyAsync(d_off, label_off, (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess && n_idx) e = hipMemcpyAsync(d_idx, label_idx, n_idx * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemsetAsync(d_out, 0, host.size() * sizeof(uint64_t), ctx->stream);
        uint32_t blocks = (uint32_t)ctx->n_cus * 4u;
        if ((uint64_t)blocks * 4 > n) blocks = (uint32_t)((n + 3) / 4);
        const bool timing = getenv("AVK_TIMING") != nullptr;
        if (timing && e == hipSuccess) e = hipEventRecord(ctx->ev0, ctx->stream);
        for (uint32_t lo = 0; lo < n_labels && e == hipSuccess && n; lo += AVK_LABEL_BLOCK) {
            const uint32_t hi = lo + AVK_LABEL_BLOCK < n_labels ? lo + AVK_LABEL_BLOCK : n_labels;
            hipLaunchKernelGGL(avk_label_tally_kernel, dim3(blocks), dim3(256), 0, ctx->stream, db->d_gm, db->d_region_out, d_off, d_idx, (uint32_t)n, lo, hi, d_out);
            e = hipGetLastError();
        }
        if (timing && e == hipSuccess) {
            e = hipEventRecord(ctx->ev1, ctx->stream);
            if (e == hipSuccess) e = hipEventSynchronize(ctx->ev1);
            float ms = 0;
            if (e == hipSuccess) e = hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
            fprintf(stderr, "avk label tallies: %u labels, %llu regions, %llu list entries: kernels %.3f ms (%.1f GB/s of per-region blocks per launch)\n", n_labels,
                    (unsigned long long)n, (unsigned long long)n_idx, ms,
                    ms > 0 ? (double)n * AVK_GM_WORDS * 4 * ((n_labels + AVK_LABEL_BLOCK - 1) / AVK_LABEL_BLOCK) / (ms * 1e6) : 0.0);
        }
        if (e == hipSuccess) e = hipMemcpyAsync(host.data(), d_out, host.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    }
    if (d_off) (void)hipFree(d_off);
    if (d_idx) (void)hipFree(d_idx);
    if (d_out) (void)hipFree(d_out);
    if (rc) return rc;
    if (e != hipSuccess) return fail(ctx, AVK_E_HIP, "label tallies failed: %s", hipGetErrorString(e));
    for (size_t k = 0; k < host.size(); ++k) out[k] += host[k];
    return 0;
}

uint32_t avk_label_block(const avk_ctx *ctx) {
    if (!ctx) return 0;
    (void)hipSetDevice(ctx->device);
    return label_block(const_cast<avk_ctx *>(ctx));
}

/* the label lists into pool buffers on the context's stream, the sums cleared */
static int labels_upload(avk_ctx *ctx, uint64_t n, const avk_region_labels *lab, void **d_off, void **d_idx, void **d_out) {
    const uint64_t n_idx = lab->label_off[n];
    const size_t words = (size_t)lab->n_labels * AVK_TALLY_LEN;
    int rc = pool_alloc(ctx, d_off, (n + 1) * 8);
    if (!rc) rc = pool_alloc(ctx, d_idx, n_idx * 4);
    if (!rc) rc = pool_alloc(ctx, d_out, words * 8);
    if (rc) return rc;
    hipError_t e = hipMemcpyAsync(*d_off, lab->label_off, (n + 1) * 8, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess && n_idx) e = hipMemcpyAsync(*d_idx, lab->label_idx, n_idx * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(*d_out, 0, words * 8, ctx->stream);
    if (e != hipSuccess) return fail(ctx, AVK_E_HIP, "label lists: %s", hipGetErrorString(e));
    return 0;
}

int avk_label_tallies_compact(avk_ctx *ctx, avk_dev_batch *db, const avk_region_labels *lab, uint64_t *out) {
    if (!ctx || !db || !lab) return AVK_E_ARG;
    {
        const int rl = labels_check(ctx, db->n_regions, lab, out);
        if (rl) return rl;
    }
    if (lab->n_labels == 0) return 0;
    if (!db->dev_packed) return fail(ctx, AVK_E_STATE, "label sums from the compact results need a device-packed batch: the option device_pack was 0 at its upload");
    if (!db->has_run || db->last_mode != 0) return fail(ctx, AVK_E_STATE, "label sums from the compact results need a batch that avk_compare_resident has solved");
    if (!db->bp_valid) return fail(ctx, AVK_E_STATE, "the batch has no BASEPAIR groups on the device: set emit_bp_groups before avk_compare_resident");
    AVK_HIP(ctx, hipSetDevice(ctx->device));
    const uint64_t n = db->n_regions;
    const size_t words = (size_t)lab->n_labels * AVK_TALLY_LEN;
    void *d_off = nullptr, *d_idx = nullptr, *d_out = nullptr;
    std::vector<uint64_t> host(words, 0);
    int rc = labels_upload(ctx, n, lab, &d_off, &d_idx, &d_out);
    if (!rc) rc = label_sums_queue(ctx, db, d_off, d_idx, lab->n_labels, d_out, false, host.data()); /* (labels_upload cleared the sums) */
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    pool_release(ctx, d_off), pool_release(ctx, d_idx), pool_release(ctx, d_out);
    if (rc) return rc;
    if (e != hipSuccess) return fail(ctx, AVK_E_HIP, "label tallies failed: %s", hipGetErrorString(e));
    labels_timing_print(ctx, "resident", lab->n_labels, n, lab->label_off[n]);
    for (size_t k = 0; k < words; ++k) out[k] += host[k];
    return 0;
}

int avk_compare_packed_submit_labels(avk_ctx *ctx, const avk_packed_batch *batch, const avk_packed_escapes *esc, const avk_region_labels *lab, const avk_compare_config *cfg,
                                     avk_result_batch *out, uint64_t *label_tallies, avk_ticket **ticket) {
    return submit_impl(ctx, batch, cfg, out, ticket, nullptr, nullptr, esc, lab, label_tallies);
}

/* ---- stratification sets resident on the device, containment lists by kernel (avk_strata.inl) ------------------------------------------------------ */
/* the refusals of avk_strata_upload, before any allocation (no device involved: with ctx == NULL the text is avk_last_error(NULL)'s) */
static int strata_check(avk_ctx *ctx, uint32_t n_labels, uint32_t n_contigs, const uint64_t *tree_off, const uint32_t *start, const uint32_t *end_max) {
    const uint64_t n_trees = (uint64_t)n_labels * n_contigs;
    if (n_trees && !tree_off) return fail(ctx, AVK_E_ARG, "strata: tree_off missing");
    if (!n_trees) return 0;
    for (uint64_t k = 0; k < n_trees; ++k)
        if (tree_off[k + 1] < tree_off[k]) return fail(ctx, AVK_E_ARG, "strata: tree_off must not decrease (tree %llu)", (unsigned long long)k);
    const uint64_t total = tree_off[n_trees];
    if (total && (!start || !end_max)) return fail(ctx, AVK_E_ARG, "strata: start / end_max missing: tree_off names %llu intervals", (unsigned long long)total);
    for (uint64_t k = 0; k < n_trees; ++k)
        for (uint64_t i = tree_off[k] + 1; i < tree_off[k + 1]; ++i) {
            if (start[i] < start[i - 1]) return fail(ctx, AVK_E_ARG, "strata: the starts of tree %llu are not sorted", (unsigned long long)k);
            if (end_max[i] < end_max[i - 1]) return fail(ctx, AVK_E_ARG, "strata: end_max of tree %llu decreases", (unsigned long long)k);
        }
    return 0;
}

/* the refusals of a context spec (avk_strata_upload_context, avk_context_label_name): no device involved */
static int context_spec_check(avk_ctx *ctx, const avk_context_spec *sp) {
    if (sp->n_gc_edges > AVK_CONTEXT_GC_EDGES_MAX || sp->n_hp_edges > AVK_CONTEXT_HP_EDGES_MAX)
        return fail(ctx, AVK_E_ARG, "context labels: at most %d GC edges and %d run edges", AVK_CONTEXT_GC_EDGES_MAX, AVK_CONTEXT_HP_EDGES_MAX);
    if (sp->n_gc_edges == 0 && sp->n_hp_edges == 0) return fail(ctx, AVK_E_ARG, "context labels: both families are empty");
    if (sp->n_gc_edges == 1) return fail(ctx, AVK_E_ARG, "context labels: one GC edge makes no label");
    if ((sp->n_gc_edges && sp->gc_pad > AVK_CONTEXT_PAD_MAX) || (sp->n_hp_edges && sp->hp_pad > AVK_CONTEXT_PAD_MAX))
        return fail(ctx, AVK_E_ARG, "context labels: a pad above %d", AVK_CONTEXT_PAD_MAX);
    for (uint32_t i = 0; i < sp->n_gc_edges; ++i) {
        if (sp->gc_edges[i] > 101u) return fail(ctx, AVK_E_ARG, "context labels: GC edge %u is above 101", sp->gc_edges[i]);
        if (i && sp->gc_edges[i] <= sp->gc_edges[i - 1]) return fail(ctx, AVK_E_ARG, "context labels: the GC edges are not strictly ascending");
    }
    for (uint32_t i = 0; i < sp->n_hp_edges; ++i) {
        if (sp->hp_edges[i] == 0) return fail(ctx, AVK_E_ARG, "context labels: a run edge of 0");
        if (i && sp->hp_edges[i] <= sp->hp_edges[i - 1]) return fail(ctx, AVK_E_ARG, "context labels: the run edges are not strictly ascending");
    }
    return 0;
}
static_assert(sizeof(avk_context_spec) == sizeof(avk::cx::CxSpec) && AVK_CONTEXT_PAD_MAX == AVK_CX_PAD_MAX && AVK_CONTEXT_GC_EDGES_MAX == AVK_CX_GC_EDGES_MAX &&
                  AVK_CONTEXT_HP_EDGES_MAX == AVK_CX_HP_EDGES_MAX,
              "avk_context_spec is avk::cx::CxSpec, field for field");

int avk_context_label_name(const avk_context_spec *sp, uint32_t j, char *buf, size_t cap) {
    if (!sp || !buf || !cap) return fail(nullptr, AVK_E_ARG, "context label name: spec or buffer missing");
    if (context_spec_check(nullptr, sp)) return AVK_E_ARG;
    const uint32_t n_gc = sp->n_gc_edges ? sp->n_gc_edges - 1u : 0u;
    if (j >= n_gc + sp->n_hp_edges) return fail(nullptr, AVK_E_ARG, "context label name: the spec has %u labels", n_gc + sp->n_hp_edges);
    int len;
    if (j < n_gc) len = snprintf(buf, cap, "ctx_gc_%u_%u", sp->gc_edges[j], sp->gc_edges[j + 1]);
    else if (j - n_gc + 1 == sp->n_hp_edges) len = snprintf(buf, cap, "ctx_hp_ge%u", sp->hp_edges[j - n_gc]);
    else len = snprintf(buf, cap, "ctx_hp_%u_%u", sp->hp_edges[j - n_gc], sp->hp_edges[j - n_gc + 1] - 1u);
    if (len < 0 || (size_t)len >= cap) return fail(nullptr, AVK_E_ARG, "context label name: %d bytes of room needed", len + 1);
    return 0;
}

int avk_strata_upload(avk_ctx *ctx, uint32_t n_labels, uint32_t n_contigs, const uint64_t *tree_off, const uint32_t *start, const uint32_t *end_max, avk_strata **out) {
    return avk_strata_upload_context(ctx, n_labels, n_contigs, tree_off, start, end_max, nullptr, out);
}

int avk_strata_upload_context(avk_ctx *ctx, uint32_t n_labels, uint32_t n_contigs, const uint64_t *tree_off, const uint32_t *start, const uint32_t *end_max,
                              const avk_context_spec *spec, avk_strata **out) {
    if (!out) return fail(ctx, AVK_E_ARG, "strata: out missing");
    *out = nullptr;
    {
        int rc = strata_check(ctx, n_labels, n_contigs, tree_off, start, end_max);
        if (!rc && spec) rc = context_spec_check(ctx, spec);
        if (!rc && spec && !n_contigs) rc = fail(ctx, AVK_E_ARG, "context labels: n_contigs missing");
        if (rc) return rc;
    }
    if (!ctx) return fail(ctx, AVK_E_ARG, "strata: context missing");
    AVK_HIP(ctx, hipSetDevice(ctx->device));
    const uint64_t n_trees = (uint64_t)n_labels * n_contigs, first = n_trees ? tree_off[0] : 0, total = n_trees ? tree_off[n_trees] : 0;
    avk_strata *st = new avk_strata();
    st->ctx = ctx, st->n_bed_labels = n_labels, st->n_labels = n_labels, st->n_contigs = n_contigs, st->n_intervals = total - first;
    if (spec) { /* (a family without edges does not exist: its pad and edges are not kept) */
        if (spec->n_gc_edges) st->spec.gc_pad = spec->gc_pad, st->spec.n_gc_edges = spec->n_gc_edges, memcpy(st->spec.gc_edges, spec->gc_edges, sizeof(uint32_t) * spec->n_gc_edges);
        if (spec->n_hp_edges) st->spec.hp_pad = spec->hp_pad, st->spec.n_hp_edges = spec->n_hp_edges, memcpy(st->spec.hp_edges, spec->hp_edges, sizeof(uint32_t) * spec->n_hp_edges);
        st->n_ctx_labels = avk::cx::cx_n_labels(st->spec), st->n_labels = n_labels + st->n_ctx_labels;
    }
    int rc = dev_alloc(ctx, &st->d_tree_off, (size_t)n_trees + 1);
    if (!rc) rc = dev_alloc(ctx, &st->d_start, (size_t)total);
    if (!rc) rc = dev_alloc(ctx, &st->d_end_max, (size_t)total);
    hipError_t e = hipSuccess;
    if (!rc && n_trees) e = hipMemcpy(st->d_tree_off, tree_off, (size_t)(n_trees + 1) * 8, hipMemcpyHostToDevice);
    if (!rc && !n_trees) e = hipMemset(st->d_tree_off, 0, 8);
    if (!rc && e == hipSuccess && total) e = hipMemcpy(st->d_start, start, (size_t)total * 4, hipMemcpyHostToDevice);
    if (!rc && e == hipSuccess && total) e = hipMemcpy(st->d_end_max, end_max, (size_t)total * 4, hipMemcpyHostToDevice);
    if (!rc && e != hipSuccess) rc = fail(ctx, AVK_E_HIP, "strata upload failed: %s", hipGetErrorString(e));
    if (rc) {
        avk_strata_free(ctx, st);
        return rc;
    }
    *out = st;
    return 0;
}
void avk_strata_free(avk_ctx *ctx, avk_strata *st) {
    if (!st) return;
    if (ctx) (void)hipSetDevice(ctx->device);
    if (st->use->in_flight) /* batches submitted with the handle are not waited for yet: their mask passes, the only readers of the trees, must be over */
        for (const hipStream_t ms : st->use->streams) (void)hipStreamSynchronize(ms);
    if (st->d_tree_off) (void)hipFree(st->d_tree_off);
    if (st->d_start) (void)hipFree(st->d_start);
    if (st->d_end_max) (void)hipFree(st->d_end_max);
    delete st;
}
uint32_t avk_strata_n_labels(const avk_strata *st) { return st ? st->n_labels : 0; }
uint32_t avk_strata_n_context_labels(const avk_strata *st) { return st ? st->n_ctx_labels : 0; }

/* the lists of a resident batch in pool buffers, on the context's stream; the number of entries is read back (the resident forms size the index array with it) */
struct StrataLists {
    void *d_mask = nullptr, *d_sums = nullptr, *d_off = nullptr, *d_idx = nullptr;
    uint64_t total = 0;
};
static void strata_lists_release(avk_ctx *ctx, StrataLists &L) {
    pool_release(ctx, L.d_mask), pool_release(ctx, L.d_sums), pool_release(ctx, L.d_off), pool_release(ctx, L.d_idx);
    L = StrataLists();
}
static int strata_lists_alloc(avk_ctx *ctx, const avk_strata *st, uint64_t n, StrataLists &L) {
    int rc = pool_alloc(ctx, &L.d_mask, (size_t)n * strata_words(st) * 4 + 16);
    if (!rc) rc = pool_alloc(ctx, &L.d_sums, ((size_t)strata_blocks(n) + 1) * 8);
    if (!rc) rc = pool_alloc(ctx, &L.d_off, (size_t)(n + 1) * 8);
    return rc;
}
static int strata_lists_make(avk_ctx *ctx, avk_dev_batch *db, const avk_strata *st, bool want_idx, StrataLists &L) {
    const uint64_t n = db->n_regions;
    int rc = strata_lists_alloc(ctx, st, n, L);
    if (rc) return rc;
    hipError_t e = strata_count_launch(st, db->dp_args.in, n, (uint32_t *)L.d_mask, (uint64_t *)L.d_sums, ctx->stream);
    if (e == hipSuccess && n) e = hipMemcpyAsync(&L.total, (uint64_t *)L.d_sums + strata_blocks(n), 8, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(ctx, AVK_E_HIP, "strata lists failed: %s", hipGetErrorString(e));
    if (want_idx) rc = pool_alloc(ctx, &L.d_idx, (size_t)L.total * 4 + 16);
    if (rc) return rc;
    e = strata_fill_launch(st, n, (const uint32_t *)L.d_mask, (const uint64_t *)L.d_sums, (uint64_t *)L.d_off, want_idx ? (uint32_t *)L.d_idx : nullptr, L.total, ctx->stream);
    if (e != hipSuccess) return fail(ctx, AVK_E_HIP, "strata lists failed: %s", hipGetErrorString(e));
    return 0;
}
static int strata_handle_check(avk_ctx *ctx, const avk_strata *st) {
    if (st->ctx != ctx) return fail(ctx, AVK_E_ARG, "strata: the handle was uploaded to another context");
    if (st->n_ctx_labels) { /* the context kernel reads the reference as it is at launch time */
        if (!ctx->d_ref || !ctx->d_ref2b || !ctx->d_refexc || !ctx->d_contig_tab) return fail(ctx, AVK_E_ARG, "context labels: avk_ref_upload has not been called");
        if (ctx->contig_len.size() != st->n_contigs)
            return fail(ctx, AVK_E_ARG, "context labels: the reference has %llu contigs, the handle %u", (unsigned long long)ctx->contig_len.size(), st->n_contigs);
    }
    return 0;
}

int avk_strata_region_labels(avk_ctx *ctx, avk_dev_batch *db, const avk_strata *st, uint64_t *label_off, uint32_t *label_idx, uint64_t cap) {
    if (!ctx || !db || !st || !label_off) return AVK_E_ARG;
    if (strata_handle_check(ctx, st)) return AVK_E_ARG;
    if (!db->dev_packed) return fail(ctx, AVK_E_STATE, "strata lists need a device-packed batch: the option device_pack was 0 at its upload");
    AVK_HIP(ctx, hipSetDevice(ctx->device));
    const uint64_t n = db->n_regions;
    if (st->n_labels == 0) {
        memset(label_off, 0, (size_t)(n + 1) * 8);
        return 0;
    }
    StrataLists L;
    const bool want_idx = label_idx != nullptr;
    int rc = strata_lists_make(ctx, db, st, want_idx, L);
    hipError_t e = hipSuccess;
    if (!rc) e = hipMemcpyAsync(label_off, L.d_off, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, ctx->stream);
    const bool fits = L.total <= cap;
    if (!rc && e == hipSuccess && want_idx && fits && L.total) e = hipMemcpyAsync(label_idx, L.d_idx, (size_t)L.total * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (hipStreamSynchronize(ctx->stream) != hipSuccess && e == hipSuccess) e = hipGetLastError();
    strata_lists_release(ctx, L);
    if (rc) return rc;
    if (e != hipSuccess) return fail(ctx, AVK_E_HIP, "strata lists failed: %s", hipGetErrorString(e));
    if (want_idx && !fits) return fail(ctx, AVK_E_ARG, "strata lists: label_idx holds %llu entries, %llu are needed", (unsigned long long)cap, (unsigned long long)label_off[n]);
    return 0;
}

int avk_label_tallies_strata(avk_ctx *ctx, avk_dev_batch *db, const avk_strata *st, uint64_t *out) {
    if (!ctx || !db || !st) return AVK_E_ARG;
    if (!out) return fail(ctx, AVK_E_ARG, "label_tallies missing");
    if (strata_handle_check(ctx, st)) return AVK_E_ARG;
    if (st->n_labels == 0) return 0;
    if (!db->dev_packed) return fail(ctx, AVK_E_STATE, "label sums from the compact results need a device-packed batch: the option device_pack was 0 at its upload");
    if (!db->has_run || db->last_mode != 0) return fail(ctx, AVK_E_STATE, "label sums from the compact results need a batch that avk_compare_resident has solved");
    if (!db->bp_valid) return fail(ctx, AVK_E_STATE, "the batch has no BASEPAIR groups on the device: set emit_bp_groups before avk_compare_resident");
    AVK_HIP(ctx, hipSetDevice(ctx->device));
    const uint64_t n = db->n_regions;
    const size_t words = (size_t)st->n_labels * AVK_TALLY_LEN;
    std::vector<uint64_t> host(words, 0);
    StrataLists L;
    void *d_out = nullptr;
    int rc = strata_lists_make(ctx, db, st, true, L);
    if (!rc) rc = pool_alloc(ctx, &d_out, words * 8);
    if (!rc) rc = label_sums_queue(ctx, db, L.d_off, L.d_idx, st->n_labels, d_out, true, host.data());
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    const uint64_t n_idx = L.total;
    strata_lists_release(ctx, L);
    pool_release(ctx, d_out);
    if (rc) return rc;
    if (e != hipSuccess) return fail(ctx, AVK_E_HIP, "label tallies failed: %s", hipGetErrorString(e));
    labels_timing_print(ctx, "resident, device lists", st->n_labels, n, n_idx);
    for (size_t k = 0; k < words; ++k) out[k] += host[k];
    return 0;
}

/* AVK_TIMING: the packed call on the device's clock, free-running (no profiler): events on the context's stream */
static void packed_timeline_print(avk_ctx *ctx) {
    if (!ctx->ev_tl[4] || !ctx->ev_valid) return;
    float c1 = 0, c2 = 0, c3 = 0, c4 = 0, c5 = 0, c6 = 0, c7 = 0;
    if (!ctx->tl_region_valid || !ctx->ev_tl[5] || hipEventElapsedTime(&c7, ctx->ev_tl[0], ctx->ev_tl[5]) != hipSuccess) c7 = -1.f, (void)hipGetLastError(); /* (-1: this call recorded none) */
    if (hipEventElapsedTime(&c1, ctx->ev_tl[0], ctx->ev_tl[1]) == hipSuccess && hipEventElapsedTime(&c2, ctx->ev_tl[0], ctx->ev_tl[2]) == hipSuccess &&
        hipEventElapsedTime(&c3, ctx->ev_tl[0], ctx->ev_tl[3]) == hipSuccess && hipEventElapsedTime(&c4, ctx->ev_tl[0], ctx->ev0) == hipSuccess &&
        hipEventElapsedTime(&c5, ctx->ev_tl[0], ctx->ev1) == hipSuccess && hipEventElapsedTime(&c6, ctx->ev_tl[0], ctx->ev_tl[4]) == hipSuccess)
        fprintf(stderr, "avk compare packed, device clock from the first copy: copies in done %.3f ms, region pass done %.3f, work order done %.3f, record writers done %.3f, solver launches %.3f .. %.3f, results out %.3f\n",
                c1, c7, c2, c3, c4, c5, c6);
    else
        (void)hipGetLastError();
    /* where each chain of the launch graph ended, from the first solver launch (events of this call only when the batch used the chain) */
    fprintf(stderr, "avk compare packed, chains end (ms after the first solver launch):");
    for (int id = 0; id < AVK_N_ENDS; ++id) {
        float t = 0;
        const bool none = id == AVK_END_DONE && ctx->last_step_chains; /* (a step with hand-back chains records no such end) */
        if (!none && hipEventElapsedTime(&t, ctx->ev0, ctx->ev_end[id]) == hipSuccess) fprintf(stderr, " %s %.3f;", AVK_STEP_END_NAME[id], t);
        else (void)hipGetLastError();
    }
    fprintf(stderr, " all %.3f\n", c5 - c4);
}

/* ---- the synchronous one-call forms ------------------------------------------------------------------------------------------------------------
 * One driver: upload (the form's own), solve, download, free — with the label kernel and the copy of its sums between solve and download for the two forms with
 * labels.  Their lists are the caller's arrays, uploaded behind the batch (lab), or made on the device: counted inside the upload, filled behind it (st). */
struct LabelStage {
    const avk_region_labels *lab;
    const avk_strata *st;
    uint64_t *sums; /* the caller's [n_labels * AVK_TALLY_LEN]: gains the sums */
};
/* ... and the bootstrap replicates behind the download (avk_compare_packed_boot): the capacity retry has patched the device view by then, so the regions it
 * repaired are counted by the same kernel; the scopes' masks are those of the upload's count pass */
struct BootStage {
    const avk_boot_spec *spec;
    uint64_t *sums; /* the caller's [(1 + n_labels) * replicates * AVK_TALLY_LEN]: gains the sums */
};
static int boot_sums_run(avk_ctx *ctx, avk_dev_batch *db, const avk_boot_spec *bs, uint32_t n_labels, const uint32_t *d_mask, uint64_t *out);
/* ... and the size-bin tallies, behind the download for the same reason (avk_compare_packed_size); they read no BASEPAIR groups, and the scopes' masks are made
 * from the resident batch when a handle is given */
struct SizeStage {
    const avk_size_spec *spec;
    const avk_strata *st;
    uint64_t *sums; /* the caller's [(1 + n_labels) * n_bins * AVK_N_GROUPS * AVK_SIZE_FIELDS]: gains the sums */
};
static int size_resident_run(avk_ctx *ctx, avk_dev_batch *db, const avk_size_spec *sp, const avk_strata *st, uint64_t *out);
/* ... and the curve by query score (avk_compare_packed_score), likewise */
struct ScoreStage {
    const avk_score_spec *spec;
    const float *scores; /* the caller's [n_variants] */
    const avk_strata *st;
    uint64_t *sums; /* the caller's [(1 + n_labels) * n_points * AVK_N_GROUPS * AVK_SCORE_FIELDS]: gains the sums */
};
static int score_resident_run(avk_ctx *ctx, avk_dev_batch *db, const avk_score_spec *sp, const float *scores, const avk_strata *st, uint64_t *out);
/* ... and the tallies by call kind (avk_compare_packed_kind), likewise */
struct KindStage {
    const avk_strata *st;
    uint64_t *sums; /* the caller's [(1 + n_labels) * AVK_N_KINDS * AVK_N_GROUPS * AVK_SIZE_FIELDS]: gains the sums */
};
static int kind_resident_run(avk_ctx *ctx, avk_dev_batch *db, const avk_strata *st, uint64_t *out);
static int compare_one_call(avk_ctx *ctx, const avk_compare_config *cfg, avk_result_batch *out, uint64_t n, const char *timed_as,
                            const std::function<int(const CallSpec &, avk_dev_batch **)> &upload, const LabelStage *ls = nullptr, const BootStage *boot = nullptr,
                            const SizeStage *size = nullptr, const ScoreStage *score = nullptr, const KindStage *kind = nullptr) {
    ctx->last_one_shot = 0;
    CallSpec spec = call_spec(ctx, out, ls != nullptr || boot != nullptr); /* (the groups are what the label kernel reads, whether the caller asked for them or not) */
    const uint32_t n_labels = !ls ? 0 : ls->st ? ls->st->n_labels : ls->lab->n_labels;
    std::vector<uint64_t> host((size_t)n_labels * AVK_TALLY_LEN, 0);
    avk_dev_batch *db = nullptr;
    StrataLists L; /* (the caller's lists use d_off and d_idx only) */
    void *d_out = nullptr;
    StrataJob job{ls ? ls->st : nullptr, nullptr, nullptr};
    int rc = 0;
    if (job.st) { /* pass 1 of the lists runs inside the upload, behind the packer's region passes; their size comes back with the plan */
        rc = strata_lists_alloc(ctx, job.st, n, L);
        if (!rc) rc = pool_alloc(ctx, &d_out, host.size() * 8);
        job.d_mask = (uint32_t *)L.d_mask, job.d_sums = (uint64_t *)L.d_sums;
        spec.strata = &job;
    }
    const auto t0 = std::chrono::steady_clock::now();
    if (!rc) rc = upload(spec, &db);
    const auto t1 = std::chrono::steady_clock::now();
    if (!rc && job.st) {
        if (n && !job.counted) rc = fail(ctx, AVK_E_STATE, "strata lists: the upload did not count them");
        L.total = job.total;
        if (!rc) rc = pool_alloc(ctx, &L.d_idx, (size_t)L.total * 4 + 16);
        if (!rc) {
            hipError_t e = hipMemsetAsync(d_out, 0, host.size() * 8, ctx->stream);
            if (e == hipSuccess) e = strata_fill_launch(job.st, n, (const uint32_t *)L.d_mask, (const uint64_t *)L.d_sums, (uint64_t *)L.d_off, (uint32_t *)L.d_idx, L.total, ctx->stream);
            if (e != hipSuccess) rc = fail(ctx, AVK_E_HIP, "strata lists failed: %s", hipGetErrorString(e));
        }
    } else if (!rc && ls)
        rc = labels_upload(ctx, n, ls->lab, &L.d_off, &L.d_idx, &d_out);
    if (!rc) rc = run_internal(ctx, spec, db, cfg, nullptr, 0);
    const auto t2 = std::chrono::steady_clock::now();
    if (!rc && ls) rc = label_sums_queue(ctx, db, L.d_off, L.d_idx, n_labels, d_out, false, host.data());
    if (!rc) { /* (the download waits for the stream; a region its capacity retry repairs is added on the host: it was not solved when the label kernel ran) */
        LabelFix lf{ls ? ls->lab : nullptr, ls ? ls->sums : nullptr}; /* the caller's lists; device lists: a repaired region's entries are fetched from there */
        if (job.st) lf.d_off = (const uint64_t *)L.d_off, lf.d_idx = (const uint32_t *)L.d_idx, lf.n = n;
        if (ls) spec.label_fix = &lf;
        rc = results_download_impl(ctx, spec, db, out, nullptr, nullptr);
        if (!rc && lf.err != hipSuccess) rc = fail(ctx, AVK_E_HIP, "label tallies: the lists of the regions the capacity retry repaired could not be fetched: %s", hipGetErrorString(lf.err));
    }
    const auto t3 = std::chrono::steady_clock::now();
    const uint64_t n_strata_idx = L.total;
    if (ls) (void)hipStreamSynchronize(ctx->stream);
    if (!rc && boot) rc = boot_sums_run(ctx, db, boot->spec, job.st ? job.st->n_labels : 0, (const uint32_t *)L.d_mask, boot->sums);
    if (!rc && size) rc = size_resident_run(ctx, db, size->spec, size->st, size->sums);
    if (!rc && score) rc = score_resident_run(ctx, db, score->spec, score->scores, score->st, score->sums);
    if (!rc && kind) rc = kind_resident_run(ctx, db, kind->st, kind->sums);
    strata_lists_release(ctx, L);
    pool_release(ctx, d_out);
    if (db) {
        ctx->last_one_shot = db->dev_packed ? 1 : 0;
        avk_batch_free(ctx, db);
    }
    if (timed_as && getenv("AVK_TIMING")) {
        auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        fprintf(stderr, "avk compare %s: upload %.3f ms, launches %.3f ms, download %.3f ms, free %.3f ms\n", timed_as, ms(t0, t1), ms(t1, t2), ms(t2, t3),
                ms(t3, std::chrono::steady_clock::now()));
    }
    if (rc || !ls) return rc;
    labels_timing_print(ctx, job.st ? "one call, device lists" : "one call", n_labels, n, job.st ? n_strata_idx : ls->lab->label_off[n]);
    for (size_t k = 0; k < host.size(); ++k) ls->sums[k] += host[k];
    return 0;
}

int avk_compare_packed_esc(avk_ctx *ctx, const avk_packed_batch *batch, const avk_packed_escapes *esc, const avk_compare_config *cfg, avk_result_batch *out) {
    if (!ctx || !batch || !cfg || !out || !(out->status || out->region_packed)) return AVK_E_ARG;
    ctx->last_one_shot = 0;
    if (!esc_present(esc)) esc = nullptr;
    if (ctx->split_parts > 1 && ctx->d_ref && !esc) { /* (the split cuts the narrow arrays by their own running sums: a batch with escapes runs whole) */
        const int rs = compare_packed_split(ctx, batch, cfg, out);
        if (rs >= 0) return rs;
    }
    const int rc = compare_one_call(ctx, cfg, out, batch->n_regions, "packed", [&](const CallSpec &spec, avk_dev_batch **db) { return upload_packed(ctx, spec, batch, esc, db); });
    if (!rc && getenv("AVK_TIMING")) packed_timeline_print(ctx);
    return rc;
}

int avk_compare_compact(avk_ctx *ctx, const avk_compact_batch *batch, const avk_compare_config *cfg, avk_result_batch *out) {
    if (!ctx || !batch || !cfg || !out || !(out->status || out->region_packed)) return AVK_E_ARG;
    return compare_one_call(ctx, cfg, out, batch->n_regions, nullptr, [&](const CallSpec &spec, avk_dev_batch **db) { return upload_compact(ctx, spec, batch, db); });
}

int avk_compare_batch(avk_ctx *ctx, const avk_region_batch *batch, const avk_compare_config *cfg, avk_result_batch *out) {
    if (!ctx || !batch || !cfg || !out || !(out->status || out->region_packed)) return AVK_E_ARG;
    if (!ctx->d_ref) return fail(ctx, AVK_E_STATE, "avk_ref_upload has not been called");
    return compare_one_call(ctx, cfg, out, batch->n_regions, "batch", [&](const CallSpec &spec, avk_dev_batch **db) { return upload_internal(ctx, spec, batch, false, db); });
}

int avk_compare_packed_labels(avk_ctx *ctx, const avk_packed_batch *batch, const avk_packed_escapes *esc, const avk_region_labels *lab, const avk_compare_config *cfg,
                              avk_result_batch *out, uint64_t *label_tallies) {
    if (!lab || lab->n_labels == 0) return avk_compare_packed_esc(ctx, batch, esc, cfg, out); /* the call without labels, launch for launch */
    if (!batch) return AVK_E_ARG;
    { /* (first of all: these refusals need no device, avk_last_error(NULL) has their text when ctx is NULL) */
        const int rl = labels_check(ctx, batch->n_regions, lab, label_tallies);
        if (rl) return rl;
    }
    if (!ctx || !cfg || !out || !(out->status || out->region_packed)) return AVK_E_ARG;
    if (!esc_present(esc)) esc = nullptr;
    const LabelStage ls{lab, nullptr, label_tallies};
    return compare_one_call(ctx, cfg, out, batch->n_regions, nullptr, [&](const CallSpec &spec, avk_dev_batch **db) { return upload_packed(ctx, spec, batch, esc, db); }, &ls);
}

int avk_compare_packed_strata(avk_ctx *ctx, const avk_packed_batch *batch, const avk_packed_escapes *esc, const avk_strata *st, const avk_compare_config *cfg, avk_result_batch *out,
                              uint64_t *label_tallies) {
    if (!st || st->n_labels == 0) return avk_compare_packed_esc(ctx, batch, esc, cfg, out); /* the call without labels, launch for launch */
    if (!batch) return AVK_E_ARG;
    if (!label_tallies) return fail(ctx, AVK_E_ARG, "label_tallies missing");
    if (!ctx || !cfg || !out || !(out->status || out->region_packed)) return AVK_E_ARG;
    if (strata_handle_check(ctx, st)) return AVK_E_ARG;
    AVK_HIP(ctx, hipSetDevice(ctx->device));
    if (!esc_present(esc)) esc = nullptr;
    const LabelStage ls{nullptr, st, label_tallies};
    return compare_one_call(ctx, cfg, out, batch->n_regions, nullptr, [&](const CallSpec &spec, avk_dev_batch **db) { return upload_packed(ctx, spec, batch, esc, db); }, &ls);
}

/* ---- bootstrap replicates of the tallies (avk_boot.h, avk_boot.inl) ----------------------------------------------------------------------------------- */
static_assert(AVK_BT_REPS * AVK_BT_SLOT <= AVK_BT_THREADS && AVK_BT_SLOT >= AVK_N_FIELDS + 1 && AVK_N_GROUPS <= 32, "a workgroup of avk_boot_tally_kernel holds its lanes and a slot its words");
/* the refusals of every entry point with a spec, before anything is queued (no device involved) */
static int boot_spec_check(avk_ctx *ctx, const avk_boot_spec *bs, uint32_t n_labels, const uint64_t *out) {
    if (bs->replicates < 1 || bs->replicates > AVK_BOOT_MAX_REPLICATES) return fail(ctx, AVK_E_ARG, "bootstrap: %u replicates, 1 to %u are possible", bs->replicates, AVK_BOOT_MAX_REPLICATES);
    if (((uint64_t)n_labels + 1) * bs->replicates > AVK_BOOT_MAX_BLOCKS)
        return fail(ctx, AVK_E_ARG, "bootstrap: %u replicates of 1 + %u scopes are more than %u blocks", bs->replicates, n_labels, AVK_BOOT_MAX_BLOCKS);
    if (!out) return fail(ctx, AVK_E_ARG, "boot_tallies missing");
    return 0;
}
/* the kernel over the scopes and the blocks of replicates, on stream s behind whatever wrote the batch's results: d_out[(1 + n_labels) * B * AVK_TALLY_LEN] gains the sums */
static int boot_launch(avk_ctx *ctx, avk_dev_batch *db, const avk_boot_spec *bs, uint32_t n_labels, const uint32_t *d_mask, uint64_t *d_out, hipStream_t s) {
    const uint64_t n = db->n_regions;
    if (!n) return 0;
    avk::lb::LbView v;
    memset(&v, 0, sizeof(v));
    v.in = db->dp_args.in, v.vinfo = db->dp_args.vinfo, v.region_out = db->d_region_out, v.var_out = db->d_var_out, v.v_off = db->d_voff, v.bp_off = db->d_bp_off, v.bp = db->d_bp;
    /* as many workgroups as a CU keeps resident (avk_boot.inl: one, at 131 registers a lane); more would only add flushes */
    uint64_t blocks = (n + AVK_BT_TILE - 1) / AVK_BT_TILE;
    if (blocks > (uint64_t)ctx->n_cus * AVK_BT_WG_PER_CU) blocks = (uint64_t)ctx->n_cus * AVK_BT_WG_PER_CU;
    const unsigned long long seed_mix = avk_boot_mix(bs->seed);
    const uint32_t B = bs->replicates;
    for (uint32_t scope = 0; scope <= (d_mask ? n_labels : 0u); ++scope)
        for (uint32_t lo = 0; lo < B; lo += AVK_BT_REPS) {
            const uint32_t hi = B - lo > AVK_BT_REPS ? lo + AVK_BT_REPS : B;
            hipLaunchKernelGGL(avk_boot_tally_kernel, dim3((unsigned)blocks), dim3(AVK_BT_THREADS), 0, s, v, d_mask, (uint32_t)n, scope, seed_mix, B, lo, hi, (unsigned long long *)d_out);
            AVK_HIP(ctx, hipGetLastError());
        }
    return 0;
}
/* sums cleared, kernels, copy back, wait, added to the caller's: on the context's stream */
static int boot_sums_run(avk_ctx *ctx, avk_dev_batch *db, const avk_boot_spec *bs, uint32_t n_labels, const uint32_t *d_mask, uint64_t *out) {
    if (!d_mask) n_labels = 0;
    const size_t words = ((size_t)n_labels + 1) * bs->replicates * AVK_TALLY_LEN;
    std::vector<uint64_t> host(words, 0);
    void *d_out = nullptr;
    int rc = pool_alloc(ctx, &d_out, words * 8);
    hipError_t e = hipSuccess;
    if (!rc) e = hipMemsetAsync(d_out, 0, words * 8, ctx->stream);
    if (!rc && e == hipSuccess) rc = boot_launch(ctx, db, bs, n_labels, d_mask, (uint64_t *)d_out, ctx->stream);
    if (!rc && e == hipSuccess) e = hipMemcpyAsync(host.data(), d_out, words * 8, hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t es = hipStreamSynchronize(ctx->stream);
    pool_release(ctx, d_out);
    if (rc) return rc;
    if (e != hipSuccess || es != hipSuccess) return fail(ctx, AVK_E_HIP, "bootstrap tallies failed: %s", hipGetErrorString(e != hipSuccess ? e : es));
    for (size_t k = 0; k < words; ++k) out[k] += host[k];
    return 0;
}

uint32_t avk_boot_block(const avk_ctx *ctx) { return ctx ? AVK_BT_REPS : 0; }

int avk_boot_tallies(avk_ctx *ctx, avk_dev_batch *db, const avk_boot_spec *bs, const avk_strata *st, uint64_t *out) {
    if (!ctx || !db || !bs) return AVK_E_ARG;
    {
        const int rb = boot_spec_check(ctx, bs, st ? st->n_labels : 0, out);
        if (rb) return rb;
    }
    if (st && strata_handle_check(ctx, st)) return AVK_E_ARG;
    if (!db->dev_packed) return fail(ctx, AVK_E_STATE, "bootstrap tallies on the device need a device-packed batch: the option device_pack was 0 at its upload (host route: avk_boot_tallies_host)");
    if (!db->has_run || db->last_mode != 0) return fail(ctx, AVK_E_STATE, "bootstrap tallies need a batch that avk_compare_resident has solved");
    if (!db->bp_valid) return fail(ctx, AVK_E_STATE, "the batch has no BASEPAIR groups on the device: set emit_bp_groups before avk_compare_resident");
    AVK_HIP(ctx, hipSetDevice(ctx->device));
    const uint64_t n = db->n_regions;
    StrataLists L;
    int rc = 0;
    if (st && st->n_labels && n) { /* the scopes' membership: the strata pass's masks, nothing else of the lists */
        rc = strata_lists_alloc(ctx, st, n, L);
        if (!rc) {
            const hipError_t e = strata_mask_launch(st, db->dp_args.in, n, (uint32_t *)L.d_mask, (uint64_t *)L.d_sums, ctx->stream);
            if (e != hipSuccess) rc = fail(ctx, AVK_E_HIP, "strata masks failed: %s", hipGetErrorString(e));
        }
    }
    if (!rc) rc = boot_sums_run(ctx, db, bs, L.d_mask ? st->n_labels : 0, (const uint32_t *)L.d_mask, out);
    else (void)hipStreamSynchronize(ctx->stream);
    strata_lists_release(ctx, L);
    return rc;
}

int avk_compare_packed_boot(avk_ctx *ctx, const avk_packed_batch *batch, const avk_packed_escapes *esc, const avk_strata *st, const avk_compare_config *cfg, avk_result_batch *out,
                            uint64_t *label_tallies, const avk_boot_spec *bs, uint64_t *boot_tallies) {
    if (!bs || bs->replicates == 0) return avk_compare_packed_strata(ctx, batch, esc, st, cfg, out, label_tallies); /* the call without a spec, launch for launch */
    if (!batch) return AVK_E_ARG;
    if (st && st->n_labels == 0) st = nullptr;
    {
        const int rb = boot_spec_check(ctx, bs, st ? st->n_labels : 0, boot_tallies);
        if (rb) return rb;
    }
    if (st && !label_tallies) return fail(ctx, AVK_E_ARG, "label_tallies missing");
    if (!ctx || !cfg || !out || !(out->status || out->region_packed)) return AVK_E_ARG;
    if (st && strata_handle_check(ctx, st)) return AVK_E_ARG;
    AVK_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->device_pack) return fail(ctx, AVK_E_STATE, "bootstrap tallies on the device need the option device_pack (host route: avk_boot_tallies_host)");
    if (!esc_present(esc)) esc = nullptr;
    const LabelStage ls{nullptr, st, label_tallies};
    const BootStage boot{bs, boot_tallies};
    return compare_one_call(ctx, cfg, out, batch->n_regions, nullptr, [&](const CallSpec &spec, avk_dev_batch **db) { return upload_packed(ctx, spec, batch, esc, db); }, st ? &ls : nullptr,
                            &boot);
}

int avk_boot_tallies_host(const avk_region_batch *b, const avk_result_batch *res, const avk_boot_spec *bs, const avk_region_labels *lab, uint32_t threads, uint64_t *out) {
    if (!b || !res || !bs) return fail(nullptr, AVK_E_ARG, "bootstrap: batch, results or spec missing");
    const uint32_t n_labels = lab ? lab->n_labels : 0;
    {
        const int rb = boot_spec_check(nullptr, bs, n_labels, out);
        if (rb) return rb;
        if (lab && n_labels) {
            const int rl = labels_check(nullptr, b->n_regions, lab, out);
            if (rl) return rl;
        }
    }
    if (!(res->status || res->region_packed)) return fail(nullptr, AVK_E_ARG, "bootstrap: the results have neither status nor region_packed");
    if (b->n_regions && !b->start) return fail(nullptr, AVK_E_ARG, "bootstrap: the batch has no start array");
    const uint64_t n = b->n_regions;
    const uint32_t B = bs->replicates;
    const size_t words = ((size_t)n_labels + 1) * B * AVK_TALLY_LEN;
    /* every thread sums into a block of its own: at most 64 of them, and no more than keep those blocks within 1 GiB */
    uint32_t T = threads < 1 ? 1u : (threads > 64u ? 64u : threads);
    while (T > 1 && (uint64_t)T * words * 8 > (1ull << 30)) --T;
    std::vector<std::vector<uint64_t>> part(T);
    std::vector<int> bad(T, 0);
    auto work = [&](uint32_t t) {
        std::vector<uint64_t> &acc = part[t];
        acc.assign(words, 0);
        uint32_t blk[AVK_N_GROUPS * AVK_N_FIELDS];
        std::vector<uint8_t> w(B);
        for (uint64_t r = n * t / T; r < n * (t + 1) / T; ++r) {
            const uint32_t status = res->status ? (uint32_t)res->status[r] : avk_rp_status(res->region_packed[r]);
            if (status != 0) continue;
            if (avk_group_metrics_from_compact(b, r, res, blk)) {
                bad[t] = 1;
                return;
            }
            const uint64_t h = avk_boot_region_hash(bs->seed, avk_boot_key(b->contig_idx ? b->contig_idx[r] : 0u, (uint32_t)b->start[r]));
            for (uint32_t k = 0; k < B; ++k) w[k] = (uint8_t)avk_boot_weight_of_hash(h, k);
            auto add = [&](uint32_t scope) {
                for (uint32_t k = 0; k < B; ++k) {
                    if (!w[k]) continue;
                    uint64_t *dst = acc.data() + ((size_t)scope * B + k) * AVK_TALLY_LEN;
                    for (int i = 0; i < AVK_N_GROUPS * AVK_N_FIELDS; ++i) dst[i] += (uint64_t)w[k] * blk[i];
                    dst[AVK_TALLY_SOLVED] += w[k];
                }
            };
            add(0);
            if (n_labels)
                for (uint64_t q = lab->label_off[r]; q < lab->label_off[r + 1]; ++q) add(1u + lab->label_idx[q]);
        }
    };
    std::vector<std::thread> pool;
    for (uint32_t t = 1; t < T; ++t) pool.emplace_back(work, t);
    work(0);
    for (std::thread &th : pool) th.join();
    for (uint32_t t = 0; t < T; ++t)
        if (bad[t]) return fail(nullptr, AVK_E_ARG, "bootstrap: avk_group_metrics_from_compact refused a region (per-call outputs and BASEPAIR groups are needed)");
    for (uint32_t t = 0; t < T; ++t)
        for (size_t k = 0; k < words; ++k) out[k] += part[t][k];
    return 0;
}

/* ---- per-call tallies by size bin (avk_sizebin.h, avk_sizebin.inl) ------------------------------------------------------------------------------------ */
/* (included here, behind the kernels of the solver step and the packer: the code of the headline call lies where it lay) */
} /* extern "C" */
#include "avk_sizebin.inl"
extern "C" {
static_assert(AVK_SIZE_FIELDS == AVK_F_WHAP_QUERY_FP + 1 && AVK_F_GT_TRUTH_TP == 0, "the size block's fields are the first fourteen of a group");
static_assert(AVK_SZ_BLOCK_WORDS(AVK_SIZE_EDGES_MAX + 1) * 8 <= AVK_SZ_LDS_BYTES && AVK_SZ_THREADS % 64 == 0 && AVK_N_VARIANT_TYPES < 15,
              "a workgroup of avk_size_tally_kernel holds one scope's block of the widest spec, whole waves, and a key its type");
using avk::cbh::host_call_values; /* (avk_callboot_host.h: the per-call contribution every per-call host route shares) */
/* the refusals of every entry point with a spec, before anything is queued (no device involved) */
static int size_spec_check(avk_ctx *ctx, const avk_size_spec *sp, const uint64_t *out) {
    if (!sp) return fail(ctx, AVK_E_ARG, "size bins: spec missing");
    if (!avk_size_spec_ok(sp)) return fail(ctx, AVK_E_ARG, "size bins: 1 to %d edges, the first at least 1, strictly ascending", AVK_SIZE_EDGES_MAX);
    if (!out) return fail(ctx, AVK_E_ARG, "size_tallies missing");
    return 0;
}
uint32_t avk_size_n_bins(const avk_size_spec *sp) { return avk_size_spec_ok(sp) ? sp->n_edges + 1u : 0u; }
uint32_t avk_size_block(const avk_ctx *ctx) { return ctx ? AVK_SZ_THREADS : 0; }
int avk_size_bin_name(const avk_size_spec *sp, uint32_t j, char *buf, size_t cap) {
    if (!avk_size_spec_ok(sp) || j > sp->n_edges || !buf || !cap) return fail(nullptr, AVK_E_ARG, "size bins: invalid spec, bin or buffer");
    uint32_t lo, hi;
    avk_size_bin_bounds(sp, j, &lo, &hi);
    const int k = j == sp->n_edges ? snprintf(buf, cap, "len_ge%u", lo) : lo == hi ? snprintf(buf, cap, "len_%u", lo) : snprintf(buf, cap, "len_%u_%u", lo, hi);
    return k > 0 && (size_t)k < cap ? 0 : fail(nullptr, AVK_E_ARG, "size bins: the name buffer is too small");
}
/* the kernel over blocks of scopes, on stream s behind whatever wrote the batch's results: d_out[(1 + n_labels) * AVK_SZ_BLOCK_WORDS(n_bins)] gains the sums */
static int size_launch(avk_ctx *ctx, avk_dev_batch *db, const avk_size_spec *sp, uint32_t n_labels, const uint32_t *d_mask, uint64_t *d_out, hipStream_t s) {
    const uint64_t n = db->n_regions;
    if (!n) return 0;
    avk::lb::LbView v;
    memset(&v, 0, sizeof(v));
    v.in = db->dp_args.in, v.vinfo = db->dp_args.vinfo, v.region_out = db->d_region_out, v.var_out = db->d_var_out, v.v_off = db->d_voff;
    const uint32_t block_bytes = AVK_SZ_BLOCK_WORDS(sp->n_edges + 1u) * 8u, n_scopes = 1u + (d_mask ? n_labels : 0u);
    uint32_t per_launch = AVK_SZ_LDS_BYTES / block_bytes;
    if (per_launch > AVK_SZ_SCOPES_MAX) per_launch = AVK_SZ_SCOPES_MAX;
    /* four workgroups a CU (their LDS), and no more workgroups than tiles: each flushes its block once */
    uint64_t blocks = (n + AVK_SZ_THREADS - 1) / AVK_SZ_THREADS;
    if (blocks > (uint64_t)ctx->n_cus * 4u) blocks = (uint64_t)ctx->n_cus * 4u;
    for (uint32_t lo = 0; lo < n_scopes; lo += per_launch) {
        const uint32_t hi = n_scopes - lo > per_launch ? lo + per_launch : n_scopes;
        hipLaunchKernelGGL(avk_size_tally_kernel, dim3((unsigned)blocks), dim3(AVK_SZ_THREADS), (size_t)(hi - lo) * block_bytes, s, v, d_mask, (uint32_t)n, *sp, lo, hi,
                           (unsigned long long *)d_out);
        AVK_HIP(ctx, hipGetLastError());
    }
    return 0;
}
/* sums cleared, kernels, copy back, wait, added to the caller's: on the context's stream */
static int size_sums_run(avk_ctx *ctx, avk_dev_batch *db, const avk_size_spec *sp, uint32_t n_labels, const uint32_t *d_mask, uint64_t *out) {
    if (!d_mask) n_labels = 0;
    const size_t words = ((size_t)n_labels + 1) * AVK_SZ_BLOCK_WORDS(sp->n_edges + 1u);
    std::vector<uint64_t> host(words, 0);
    void *d_out = nullptr;
    int rc = pool_alloc(ctx, &d_out, words * 8);
    hipError_t e = hipSuccess;
    if (!rc) e = hipMemsetAsync(d_out, 0, words * 8, ctx->stream);
    if (!rc && e == hipSuccess) rc = size_launch(ctx, db, sp, n_labels, d_mask, (uint64_t *)d_out, ctx->stream);
    if (!rc && e == hipSuccess) e = hipMemcpyAsync(host.data(), d_out, words * 8, hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t es = hipStreamSynchronize(ctx->stream);
    pool_release(ctx, d_out);
    if (rc) return rc;
    if (e != hipSuccess || es != hipSuccess) return fail(ctx, AVK_E_HIP, "size-bin tallies failed: %s", hipGetErrorString(e != hipSuccess ? e : es));
    for (size_t k = 0; k < words; ++k) out[k] += host[k];
    return 0;
}
/* a solved resident batch: the scopes' membership (the strata pass's masks, nothing else of the lists), then the sums */
static int size_resident_run(avk_ctx *ctx, avk_dev_batch *db, const avk_size_spec *sp, const avk_strata *st, uint64_t *out) {
    const uint64_t n = db->n_regions;
    StrataLists L;
    int rc = 0;
    if (st && st->n_labels && n) {
        rc = strata_lists_alloc(ctx, st, n, L);
        if (!rc) {
            const hipError_t e = strata_mask_launch(st, db->dp_args.in, n, (uint32_t *)L.d_mask, (uint64_t *)L.d_sums, ctx->stream);
            if (e != hipSuccess) rc = fail(ctx, AVK_E_HIP, "strata masks failed: %s", hipGetErrorString(e));
        }
    }
    if (!rc) rc = size_sums_run(ctx, db, sp, L.d_mask ? st->n_labels : 0, (const uint32_t *)L.d_mask, out);
    else (void)hipStreamSynchronize(ctx->stream);
    strata_lists_release(ctx, L);
    return rc;
}

int avk_size_tallies(avk_ctx *ctx, avk_dev_batch *db, const avk_size_spec *sp, const avk_strata *st, uint64_t *out) {
    if (!ctx || !db) return AVK_E_ARG;
    {
        const int rs = size_spec_check(ctx, sp, out);
        if (rs) return rs;
    }
    if (st && strata_handle_check(ctx, st)) return AVK_E_ARG;
    if (!db->dev_packed) return fail(ctx, AVK_E_STATE, "size-bin tallies on the device need a device-packed batch: the option device_pack was 0 at its upload (host route: avk_size_tallies_host)");
    if (!db->has_run || db->last_mode != 0) return fail(ctx, AVK_E_STATE, "size-bin tallies need a batch that avk_compare_resident has solved");
    AVK_HIP(ctx, hipSetDevice(ctx->device));
    return size_resident_run(ctx, db, sp, st, out);
}

int avk_compare_packed_size(avk_ctx *ctx, const avk_packed_batch *batch, const avk_packed_escapes *esc, const avk_strata *st, const avk_compare_config *cfg,
                            const avk_size_spec *sp, avk_result_batch *out, uint64_t *size_out) {
    if (!batch) return AVK_E_ARG;
    if (st && st->n_labels == 0) st = nullptr;
    {
        const int rs = size_spec_check(ctx, sp, size_out);
        if (rs) return rs;
    }
    if (!ctx || !cfg || !out || !(out->status || out->region_packed)) return AVK_E_ARG;
    if (st && strata_handle_check(ctx, st)) return AVK_E_ARG;
    AVK_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->device_pack) return fail(ctx, AVK_E_STATE, "size-bin tallies on the device need the option device_pack (host route: avk_size_tallies_host)");
    if (!esc_present(esc)) esc = nullptr;
    const SizeStage size{sp, st, size_out};
    return compare_one_call(ctx, cfg, out, batch->n_regions, nullptr, [&](const CallSpec &spec, avk_dev_batch **db) { return upload_packed(ctx, spec, batch, esc, db); }, nullptr, nullptr,
                            &size);
}

int avk_size_tallies_host(const avk_region_batch *b, const avk_result_batch *res, const avk_size_spec *sp, const avk_region_labels *lab, uint32_t threads, uint64_t *out) {
    if (!b || !res) return fail(nullptr, AVK_E_ARG, "size bins: batch or results missing");
    const uint32_t n_labels = lab ? lab->n_labels : 0;
    {
        const int rs = size_spec_check(nullptr, sp, out);
        if (rs) return rs;
        if (lab && n_labels) {
            const int rl = labels_check(nullptr, b->n_regions, lab, out);
            if (rl) return rl;
        }
    }
    if (!(res->status || res->region_packed)) return fail(nullptr, AVK_E_ARG, "size bins: the results have neither status nor region_packed");
    const bool wide_calls = res->var_expected && res->var_observed;
    if (!wide_calls && !res->var_packed) return fail(nullptr, AVK_E_ARG, "size bins: the results have no per-call outputs");
    const uint64_t n = b->n_regions;
    const uint32_t n_bins = sp->n_edges + 1u;
    const size_t block = AVK_SZ_BLOCK_WORDS(n_bins), words = ((size_t)n_labels + 1) * block;
    const uint32_t T = threads < 1 ? 1u : (threads > 64u ? 64u : threads); /* every thread sums into a block of its own */
    std::vector<std::vector<uint64_t>> part(T);
    std::vector<int> bad(T, 0);
    auto work = [&](uint32_t t) {
        std::vector<uint64_t> &acc = part[t];
        acc.assign(words, 0);
        for (uint64_t r = n * t / T; r < n * (t + 1) / T; ++r) {
            const uint32_t status = res->status ? (uint32_t)res->status[r] : avk_rp_status(res->region_packed[r]);
            if (status != 0) continue;
            for (int side = 0; side < 2; ++side) {
                const uint64_t off = side == 0 ? b->t_off[r] : b->q_off[r];
                const uint32_t cnt = side == 0 ? b->t_cnt[r] : b->q_cnt[r];
                if (off > b->n_variants || cnt > b->n_variants - off) {
                    bad[t] = 1;
                    return;
                }
                for (uint32_t i = 0; i < cnt; ++i) {
                    const uint64_t v = off + i;
                    const uint32_t vt = b->var_type[v];
                    const uint64_t w = avk::host_edit_distance(b->allele_bytes + b->a0_off[v], b->a0_len[v], b->allele_bytes + b->a1_off[v], b->a1_len[v]); /* Variant::alt_ed */
                    uint32_t val[AVK_SIZE_VALUES];
                    host_call_values(res, wide_calls, v, side, w, val);
                    const uint32_t bin = avk_size_bin_of(sp, avk_size_of(b->a0_len[v], b->a1_len[v]));
                    auto add = [&](uint32_t scope) {
                        for (uint32_t g : {0u, 1u + vt}) {
                            if (g >= AVK_N_GROUPS) continue;
                            uint64_t *dst = acc.data() + (size_t)scope * block + ((size_t)bin * AVK_N_GROUPS + g) * AVK_SIZE_FIELDS;
                            for (uint32_t k = 0; k < AVK_SIZE_VALUES; ++k) dst[avk_size_field_of(k, side)] += val[k];
                        }
                    };
                    add(0);
                    if (n_labels)
                        for (uint64_t q = lab->label_off[r]; q < lab->label_off[r + 1]; ++q) add(1u + lab->label_idx[q]);
                }
            }
        }
    };
    std::vector<std::thread> pool;
    for (uint32_t t = 1; t < T; ++t) pool.emplace_back(work, t);
    work(0);
    for (std::thread &th : pool) th.join();
    for (uint32_t t = 0; t < T; ++t)
        if (bad[t]) return fail(nullptr, AVK_E_ARG, "size bins: a region's calls lie outside the batch");
    for (uint32_t t = 0; t < T; ++t)
        for (size_t k = 0; k < words; ++k) out[k] += part[t][k];
    return 0;
}

/* ---- precision-recall curve by query score (avk_score.h, avk_score.inl) -------------------------------------------------------------------------------- */
} /* extern "C" */
#include "avk_score.inl"
#include "avk_score_host.h"
extern "C" {
static_assert(AVK_SCORE_FIELDS == AVK_SIZE_FIELDS && AVK_SCORE_FIELDS == AVK_F_WHAP_QUERY_FP + 1, "the score block's fields are the size block's");
static_assert(AVK_SC_BLOCK_WORDS(AVK_SCORE_THRESHOLDS_MAX + 1) * 8 <= AVK_SC_LDS_BYTES && AVK_SC_THREADS % 64 == 0 && AVK_N_VARIANT_TYPES < 15 && AVK_SCORE_THRESHOLDS_MAX < 32,
              "a workgroup of avk_score_hist_kernel holds one scope's block of the widest spec, whole waves, and a key its bin and type");
/* the refusals of every entry point with a spec, before anything is queued (no device involved) */
static int score_spec_check(avk_ctx *ctx, const avk_score_spec *sp, const float *scores, const uint64_t *out) {
    if (!sp) return fail(ctx, AVK_E_ARG, "score curve: spec missing");
    if (!avk_score_spec_ok(sp)) return fail(ctx, AVK_E_ARG, "score curve: 1 to %d thresholds, every one finite, strictly ascending", AVK_SCORE_THRESHOLDS_MAX);
    if (!scores) return fail(ctx, AVK_E_ARG, "score curve: scores missing");
    if (!out) return fail(ctx, AVK_E_ARG, "score_tallies missing");
    return 0;
}
uint32_t avk_score_n_points(const avk_score_spec *sp) { return avk_score_spec_ok(sp) ? sp->n_thresholds + 1u : 0u; }
uint32_t avk_score_block(const avk_ctx *ctx) { return ctx ? AVK_SC_THREADS : 0; }
int avk_score_point_name(const avk_score_spec *sp, uint32_t k, char *buf, size_t cap) {
    if (!avk_score_spec_ok(sp) || k > sp->n_thresholds || !buf || !cap) return fail(nullptr, AVK_E_ARG, "score curve: invalid spec, point or buffer");
    const int w = k == 0 ? snprintf(buf, cap, "score_all") : snprintf(buf, cap, "score_ge_%g", (double)sp->t[k - 1]);
    return w > 0 && (size_t)w < cap ? 0 : fail(nullptr, AVK_E_ARG, "score curve: the name buffer is too small");
}
/* scores in, histograms cleared, the histogram kernel over blocks of scopes, the curve kernel, copy back, wait, added to the caller's: on the context's stream */
static int score_sums_run(avk_ctx *ctx, avk_dev_batch *db, const avk_score_spec *sp, const float *scores, uint32_t n_labels, const uint32_t *d_mask, uint64_t *out) {
    if (!d_mask) n_labels = 0;
    const uint64_t n = db->n_regions, nv = db->dp_args.in.n_variants;
    const uint32_t n_points = sp->n_thresholds + 1u, n_scopes = 1u + n_labels;
    const size_t hist_words = (size_t)n_scopes * AVK_SC_BLOCK_WORDS(n_points), curve_words = (size_t)n_scopes * AVK_SC_H_WORDS(n_points);
    if (!n) return 0;
    /* one pool block: the curve, the error word (in a 64-bit slot), the histograms; the scores in a second */
    std::vector<uint64_t> host(curve_words + 1, 0);
    void *d_blk = nullptr, *d_scores = nullptr;
    int rc = pool_alloc(ctx, &d_blk, (curve_words + 1 + hist_words) * 8);
    if (!rc) rc = pool_alloc(ctx, &d_scores, (size_t)nv * 4 + 16);
    hipError_t e = hipSuccess;
    if (!rc) e = hipMemsetAsync(d_blk, 0, (curve_words + 1 + hist_words) * 8, ctx->stream);
    if (!rc && e == hipSuccess && nv) e = hipMemcpyAsync(d_scores, scores, (size_t)nv * 4, hipMemcpyHostToDevice, ctx->stream);
    if (!rc && e == hipSuccess) {
        uint64_t *d_curve = (uint64_t *)d_blk, *d_hist = d_curve + curve_words + 1;
        uint32_t *d_err = (uint32_t *)(d_curve + curve_words);
        avk::lb::LbView v;
        memset(&v, 0, sizeof(v));
        v.in = db->dp_args.in, v.vinfo = db->dp_args.vinfo, v.region_out = db->d_region_out, v.var_out = db->d_var_out, v.v_off = db->d_voff;
        const uint32_t block_bytes = AVK_SC_BLOCK_WORDS(n_points) * 8u;
        uint32_t per_launch = AVK_SC_LDS_BYTES / block_bytes;
        if (per_launch > AVK_SC_SCOPES_MAX) per_launch = AVK_SC_SCOPES_MAX;
        const uint64_t tiles = (n + AVK_SC_THREADS - 1) / AVK_SC_THREADS;
        for (uint32_t lo = 0; lo < n_scopes && e == hipSuccess; lo += per_launch) {
            const uint32_t hi = n_scopes - lo > per_launch ? lo + per_launch : n_scopes;
            const uint32_t lds_words = (hi - lo) * AVK_SC_BLOCK_WORDS(n_points);
            /* as many workgroups a CU as this launch's blocks fit its 160 KB of LDS beside each other — two for a 32-point scope, eight (the CU's 2,048
             * work-items) for one scope of a few thresholds —, and no more workgroups than tiles: each flushes its block once */
            uint32_t per_cu = (uint32_t)(AVK_SC_CU_LDS_BYTES / ((size_t)lds_words * 8));
            per_cu = per_cu < 1u ? 1u : per_cu > 2048u / AVK_SC_THREADS ? 2048u / AVK_SC_THREADS : per_cu;
            const uint64_t blocks = tiles < (uint64_t)ctx->n_cus * per_cu ? tiles : (uint64_t)ctx->n_cus * per_cu;
            hipLaunchKernelGGL(avk_score_hist_kernel, dim3((unsigned)blocks), dim3(AVK_SC_THREADS), (size_t)lds_words * 8, ctx->stream, v, d_mask, (uint32_t)n, *sp,
                               (const float *)d_scores, lo, hi, lds_words, (unsigned long long *)d_hist, d_err);
            e = hipGetLastError();
        }
        if (e == hipSuccess) {
            hipLaunchKernelGGL(avk_score_curve_kernel, dim3(n_scopes * AVK_N_GROUPS), dim3(64), 0, ctx->stream, (const unsigned long long *)d_hist, n_points, n_scopes,
                               (const uint32_t *)d_err, (unsigned long long *)d_curve);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(host.data(), d_curve, (curve_words + 1) * 8, hipMemcpyDeviceToHost, ctx->stream);
    }
    const hipError_t es = hipStreamSynchronize(ctx->stream);
    pool_release(ctx, d_blk), pool_release(ctx, d_scores);
    if (rc) return rc;
    if (e != hipSuccess || es != hipSuccess) return fail(ctx, AVK_E_HIP, "score curve failed: %s", hipGetErrorString(e != hipSuccess ? e : es));
    if (host[curve_words]) return fail(ctx, AVK_E_HIP, "score curve: the kernel refused its launch (error word %llu); nothing was added", (unsigned long long)host[curve_words]);
    for (size_t k = 0; k < curve_words; ++k) out[k] += host[k];
    return 0;
}
/* a solved resident batch: the scopes' membership (the strata pass's masks, nothing else of the lists), then the sums */
static int score_resident_run(avk_ctx *ctx, avk_dev_batch *db, const avk_score_spec *sp, const float *scores, const avk_strata *st, uint64_t *out) {
    const uint64_t n = db->n_regions;
    StrataLists L;
    int rc = 0;
    if (st && st->n_labels && n) {
        rc = strata_lists_alloc(ctx, st, n, L);
        if (!rc) {
            const hipError_t e = strata_mask_launch(st, db->dp_args.in, n, (uint32_t *)L.d_mask, (uint64_t *)L.d_sums, ctx->stream);
            if (e != hipSuccess) rc = fail(ctx, AVK_E_HIP, "strata masks failed: %s", hipGetErrorString(e));
        }
    }
    if (!rc) rc = score_sums_run(ctx, db, sp, scores, L.d_mask ? st->n_labels : 0, (const uint32_t *)L.d_mask, out);
    else (void)hipStreamSynchronize(ctx->stream);
    strata_lists_release(ctx, L);
    return rc;
}

int avk_score_tallies(avk_ctx *ctx, avk_dev_batch *db, const avk_score_spec *sp, const float *scores, const avk_strata *st, uint64_t *out) {
    if (!ctx || !db) return AVK_E_ARG;
    {
        const int rs = score_spec_check(ctx, sp, scores, out);
        if (rs) return rs;
    }
    if (st && strata_handle_check(ctx, st)) return AVK_E_ARG;
    if (!db->dev_packed) return fail(ctx, AVK_E_STATE, "the score curve on the device needs a device-packed batch: the option device_pack was 0 at its upload (host route: avk_score_tallies_host)");
    if (!db->has_run || db->last_mode != 0) return fail(ctx, AVK_E_STATE, "the score curve needs a batch that avk_compare_resident has solved");
    AVK_HIP(ctx, hipSetDevice(ctx->device));
    return score_resident_run(ctx, db, sp, scores, st, out);
}

int avk_compare_packed_score(avk_ctx *ctx, const avk_packed_batch *batch, const avk_packed_escapes *esc, const avk_strata *st, const avk_compare_config *cfg,
                             const avk_score_spec *sp, const float *scores, avk_result_batch *out, uint64_t *score_out) {
    if (!batch) return AVK_E_ARG;
    if (st && st->n_labels == 0) st = nullptr;
    {
        const int rs = score_spec_check(ctx, sp, scores, score_out);
        if (rs) return rs;
    }
    if (!ctx || !cfg || !out || !(out->status || out->region_packed)) return AVK_E_ARG;
    if (st && strata_handle_check(ctx, st)) return AVK_E_ARG;
    AVK_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->device_pack) return fail(ctx, AVK_E_STATE, "the score curve on the device needs the option device_pack (host route: avk_score_tallies_host)");
    if (!esc_present(esc)) esc = nullptr;
    const ScoreStage score{sp, scores, st, score_out};
    return compare_one_call(ctx, cfg, out, batch->n_regions, nullptr, [&](const CallSpec &spec, avk_dev_batch **db) { return upload_packed(ctx, spec, batch, esc, db); }, nullptr, nullptr,
                            nullptr, &score);
}

int avk_score_tallies_host(const avk_region_batch *b, const avk_result_batch *res, const avk_score_spec *sp, const float *scores, const avk_region_labels *lab, uint32_t threads,
                           uint64_t *out) {
    if (!b || !res) return fail(nullptr, AVK_E_ARG, "score curve: batch or results missing");
    const uint32_t n_labels = lab ? lab->n_labels : 0;
    {
        const int rs = score_spec_check(nullptr, sp, scores, out);
        if (rs) return rs;
        if (lab && n_labels) {
            const int rl = labels_check(nullptr, b->n_regions, lab, out);
            if (rl) return rl;
        }
    }
    if (!(res->status || res->region_packed)) return fail(nullptr, AVK_E_ARG, "score curve: the results have neither status nor region_packed");
    const bool wide_calls = res->var_expected && res->var_observed;
    if (!wide_calls && !res->var_packed) return fail(nullptr, AVK_E_ARG, "score curve: the results have no per-call outputs");
    /* the sums themselves: plain C++ in a header of its own, which the sanitizer program of the tests includes as well */
    if (avk_score_host_sum(b, res, sp, scores, lab && n_labels ? lab : nullptr, threads, avk::host_edit_distance, out))
        return fail(nullptr, AVK_E_ARG, "score curve: a region's calls lie outside the batch, or a label is not one of the labels");
    return 0;
}

/* ---- per-call tallies by call kind: het / hom x Ti / Tv (avk_callkind.h, avk_callkind.inl) ---------------------------------------------------------------- */
} /* extern "C" */
#include "avk_callkind.inl"
extern "C" {
static_assert(AVK_ZYG_UNPHASED_HET == 2 && AVK_ZYG_PHASED_HET01 == 3 && AVK_ZYG_PHASED_HET10 == 4 && AVK_ZYG_HOM_ALT == 5, "avk_kind_gt_of reads these numbers");
static_assert(AVK_N_KINDS == AVK_KIND_N_GT * AVK_KIND_N_SUB && AVK_N_KINDS <= 16, "a kind is a genotype and a substitution class, and a key holds it in four bits");
static_assert(AVK_CK_SCOPES >= 1 && AVK_CK_SCOPES <= AVK_SZ_SCOPES_MAX && AVK_CK_THREADS % 64 == 0 && AVK_N_VARIANT_TYPES < 15,
              "a workgroup of avk_kind_tally_kernel holds a scope's block, whole waves, and a key its type");
uint32_t avk_kind_n(void) { return AVK_N_KINDS; }
uint32_t avk_kind_block(const avk_ctx *ctx) { return ctx ? AVK_CK_THREADS : 0; }
int avk_kind_name(uint32_t k, char *buf, size_t cap) {
    const char *name = avk_kind_name_of(k);
    if (!name || !buf || !cap) return fail(nullptr, AVK_E_ARG, "call kinds: invalid kind or buffer");
    const int len = snprintf(buf, cap, "%s", name);
    return len > 0 && (size_t)len < cap ? 0 : fail(nullptr, AVK_E_ARG, "call kinds: the name buffer is too small");
}
/* the kernel over blocks of scopes, on stream s behind whatever wrote the batch's results: d_out[(1 + n_labels) * AVK_CK_BLOCK_WORDS] gains the sums */
static int kind_launch(avk_ctx *ctx, avk_dev_batch *db, uint32_t n_labels, const uint32_t *d_mask, uint64_t *d_out, hipStream_t s) {
    const uint64_t n = db->n_regions;
    if (!n) return 0;
    avk::lb::LbView v;
    memset(&v, 0, sizeof(v));
    v.in = db->dp_args.in, v.vinfo = db->dp_args.vinfo, v.region_out = db->d_region_out, v.var_out = db->d_var_out, v.v_off = db->d_voff;
    const uint32_t n_scopes = 1u + (d_mask ? n_labels : 0u);
    /* four workgroups a CU (their LDS), and no more workgroups than tiles: each flushes its block once */
    uint64_t blocks = (n + AVK_CK_THREADS - 1) / AVK_CK_THREADS;
    if (blocks > (uint64_t)ctx->n_cus * 4u) blocks = (uint64_t)ctx->n_cus * 4u;
    for (uint32_t lo = 0; lo < n_scopes; lo += AVK_CK_SCOPES) {
        const uint32_t hi = n_scopes - lo > AVK_CK_SCOPES ? lo + AVK_CK_SCOPES : n_scopes;
        hipLaunchKernelGGL(avk_kind_tally_kernel, dim3((unsigned)blocks), dim3(AVK_CK_THREADS), (size_t)(hi - lo) * AVK_CK_BLOCK_WORDS * 8u, s, v, d_mask, (uint32_t)n, lo, hi,
                           (unsigned long long *)d_out);
        AVK_HIP(ctx, hipGetLastError());
    }
    return 0;
}
/* sums cleared, kernels, copy back, wait, added to the caller's: on the context's stream */
static int kind_sums_run(avk_ctx *ctx, avk_dev_batch *db, uint32_t n_labels, const uint32_t *d_mask, uint64_t *out) {
    if (!d_mask) n_labels = 0;
    const size_t words = ((size_t)n_labels + 1) * AVK_CK_BLOCK_WORDS;
    std::vector<uint64_t> host(words, 0);
    void *d_out = nullptr;
    int rc = pool_alloc(ctx, &d_out, words * 8);
    hipError_t e = hipSuccess;
    if (!rc) e = hipMemsetAsync(d_out, 0, words * 8, ctx->stream);
    if (!rc && e == hipSuccess) rc = kind_launch(ctx, db, n_labels, d_mask, (uint64_t *)d_out, ctx->stream);
    if (!rc && e == hipSuccess) e = hipMemcpyAsync(host.data(), d_out, words * 8, hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t es = hipStreamSynchronize(ctx->stream);
    pool_release(ctx, d_out);
    if (rc) return rc;
    if (e != hipSuccess || es != hipSuccess) return fail(ctx, AVK_E_HIP, "call-kind tallies failed: %s", hipGetErrorString(e != hipSuccess ? e : es));
    for (size_t k = 0; k < words; ++k) out[k] += host[k];
    return 0;
}
/* a solved resident batch: the scopes' membership (the strata pass's masks, nothing else of the lists), then the sums */
static int kind_resident_run(avk_ctx *ctx, avk_dev_batch *db, const avk_strata *st, uint64_t *out) {
    const uint64_t n = db->n_regions;
    StrataLists L;
    int rc = 0;
    if (st && st->n_labels && n) {
        rc = strata_lists_alloc(ctx, st, n, L);
        if (!rc) {
            const hipError_t e = strata_mask_launch(st, db->dp_args.in, n, (uint32_t *)L.d_mask, (uint64_t *)L.d_sums, ctx->stream);
            if (e != hipSuccess) rc = fail(ctx, AVK_E_HIP, "strata masks failed: %s", hipGetErrorString(e));
        }
    }
    if (!rc) rc = kind_sums_run(ctx, db, L.d_mask ? st->n_labels : 0, (const uint32_t *)L.d_mask, out);
    else (void)hipStreamSynchronize(ctx->stream);
    strata_lists_release(ctx, L);
    return rc;
}

int avk_kind_tallies(avk_ctx *ctx, avk_dev_batch *db, const avk_strata *st, uint64_t *out) {
    if (!ctx || !db) return AVK_E_ARG;
    if (!out) return fail(ctx, AVK_E_ARG, "kind_tallies missing");
    if (st && strata_handle_check(ctx, st)) return AVK_E_ARG;
    if (!db->dev_packed) return fail(ctx, AVK_E_STATE, "call-kind tallies on the device need a device-packed batch: the option device_pack was 0 at its upload (host route: avk_kind_tallies_host)");
    if (!db->has_run || db->last_mode != 0) return fail(ctx, AVK_E_STATE, "call-kind tallies need a batch that avk_compare_resident has solved");
    AVK_HIP(ctx, hipSetDevice(ctx->device));
    return kind_resident_run(ctx, db, st, out);
}

int avk_compare_packed_kind(avk_ctx *ctx, const avk_packed_batch *batch, const avk_packed_escapes *esc, const avk_strata *st, const avk_compare_config *cfg,
                            avk_result_batch *out, uint64_t *kind_out) {
    if (!batch) return AVK_E_ARG;
    if (st && st->n_labels == 0) st = nullptr;
    if (!kind_out) return fail(ctx, AVK_E_ARG, "kind_tallies missing");
    if (!ctx || !cfg || !out || !(out->status || out->region_packed)) return AVK_E_ARG;
    if (st && strata_handle_check(ctx, st)) return AVK_E_ARG;
    AVK_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->device_pack) return fail(ctx, AVK_E_STATE, "call-kind tallies on the device need the option device_pack (host route: avk_kind_tallies_host)");
    if (!esc_present(esc)) esc = nullptr;
    const KindStage kind{st, kind_out};
    return compare_one_call(ctx, cfg, out, batch->n_regions, nullptr, [&](const CallSpec &spec, avk_dev_batch **db) { return upload_packed(ctx, spec, batch, esc, db); }, nullptr, nullptr,
                            nullptr, nullptr, &kind);
}

int avk_kind_tallies_host(const avk_region_batch *b, const avk_result_batch *res, const avk_region_labels *lab, uint32_t threads, uint64_t *out) {
    if (!b || !res) return fail(nullptr, AVK_E_ARG, "call kinds: batch or results missing");
    const uint32_t n_labels = lab ? lab->n_labels : 0;
    if (!out) return fail(nullptr, AVK_E_ARG, "kind_tallies missing");
    if (lab && n_labels) {
        const int rl = labels_check(nullptr, b->n_regions, lab, out);
        if (rl) return rl;
    }
    if (!(res->status || res->region_packed)) return fail(nullptr, AVK_E_ARG, "call kinds: the results have neither status nor region_packed");
    const bool wide_calls = res->var_expected && res->var_observed;
    if (!wide_calls && !res->var_packed) return fail(nullptr, AVK_E_ARG, "call kinds: the results have no per-call outputs");
    const uint64_t n = b->n_regions;
    const size_t block = AVK_CK_BLOCK_WORDS, words = ((size_t)n_labels + 1) * block;
    const uint32_t T = threads < 1 ? 1u : (threads > 64u ? 64u : threads); /* every thread sums into a block of its own */
    std::vector<std::vector<uint64_t>> part(T);
    std::vector<int> bad(T, 0);
    auto work = [&](uint32_t t) {
        std::vector<uint64_t> &acc = part[t];
        acc.assign(words, 0);
        for (uint64_t r = n * t / T; r < n * (t + 1) / T; ++r) {
            const uint32_t status = res->status ? (uint32_t)res->status[r] : avk_rp_status(res->region_packed[r]);
            if (status != 0) continue;
            for (int side = 0; side < 2; ++side) {
                const uint64_t off = side == 0 ? b->t_off[r] : b->q_off[r];
                const uint32_t cnt = side == 0 ? b->t_cnt[r] : b->q_cnt[r];
                if (off > b->n_variants || cnt > b->n_variants - off) {
                    bad[t] = 1;
                    return;
                }
                for (uint32_t i = 0; i < cnt; ++i) {
                    const uint64_t v = off + i;
                    const uint32_t vt = b->var_type[v], l0 = b->a0_len[v], l1 = b->a1_len[v];
                    const uint64_t w = avk::host_edit_distance(b->allele_bytes + b->a0_off[v], l0, b->allele_bytes + b->a1_off[v], l1); /* Variant::alt_ed */
                    uint32_t val[AVK_SIZE_VALUES];
                    host_call_values(res, wide_calls, v, side, w, val);
                    const bool bytes = l0 == 1u && l1 == 1u && b->a0_off[v] < b->allele_bytes_len && b->a1_off[v] < b->allele_bytes_len;
                    const uint32_t sub = bytes ? avk_kind_sub_of(1u, 1u, b->allele_bytes[b->a0_off[v]], b->allele_bytes[b->a1_off[v]]) : (uint32_t)AVK_KIND_SUB_OTHER;
                    const uint32_t kind = avk_kind_of(avk_kind_gt_of(b->var_zyg[v]), sub);
                    auto add = [&](uint32_t scope) {
                        for (uint32_t g : {0u, 1u + vt}) {
                            if (g >= AVK_N_GROUPS) continue;
                            uint64_t *dst = acc.data() + (size_t)scope * block + ((size_t)kind * AVK_N_GROUPS + g) * AVK_SIZE_FIELDS;
                            for (uint32_t k = 0; k < AVK_SIZE_VALUES; ++k) dst[avk_size_field_of(k, side)] += val[k];
                        }
                    };
                    add(0);
                    if (n_labels)
                        for (uint64_t q = lab->label_off[r]; q < lab->label_off[r + 1]; ++q) add(1u + lab->label_idx[q]);
                }
            }
        }
    };
    std::vector<std::thread> pool;
    for (uint32_t t = 1; t < T; ++t) pool.emplace_back(work, t);
    work(0);
    for (std::thread &th : pool) th.join();
    for (uint32_t t = 0; t < T; ++t)
        if (bad[t]) return fail(nullptr, AVK_E_ARG, "call kinds: a region's calls lie outside the batch");
    for (uint32_t t = 0; t < T; ++t)
        for (size_t k = 0; k < words; ++k) out[k] += part[t][k];
    return 0;
}

/* ---- bootstrap replicates of the per-call blocks: size bins and call kinds (avk_callboot.h, avk_callboot.inl) ------------------------------------------------ */
} /* extern "C" */
#include "avk_callboot.inl"
extern "C" {
static_assert(AVK_CALLBOOT_KEY_WORDS * 8 == 1456 && AVK_CB_SLOTS * AVK_CB_REPS_MAX <= AVK_CB_THREADS && AVK_CB_TILE <= AVK_CB_THREADS && AVK_CB_RECS <= AVK_CB_THREADS,
              "a workgroup of avk_callboot_tally_kernel holds its lane teams, a staging lane per region and one per record");
static_assert(AVK_CB_LDS_BYTES(AVK_SIZE_EDGES_MAX + 1, 1) <= 64 * 1024 && AVK_N_KINDS <= 16 && AVK_SIZE_EDGES_MAX + 1 <= 16,
              "one replicate of the widest family fits the LDS every device grants; a key fits four bits");
static_assert((uint64_t)1000 * AVK_N_KINDS * 17 <= AVK_CALLBOOT_MAX_BLOCKS, "the cap admits 1000 replicates of the kinds in 17 scopes");
static int64_t callboot_lds(avk_ctx *ctx) { /* the LDS a launch really gets: the whole CU's where the runtime grants it */
    if (!ctx->callboot_lds_bytes) {
        int64_t b = 64 * 1024;
        if (hipFuncSetAttribute((const void *)avk_callboot_tally_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, AVK_CB_LDS_MAX) == hipSuccess) b = AVK_CB_LDS_MAX;
        else {
            (void)hipGetLastError();
            int attr = 0;
            if (hipDeviceGetAttribute(&attr, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device) == hipSuccess && attr > 0 && attr < b) b = attr;
            else (void)hipGetLastError();
        }
        ctx->callboot_lds_bytes = b - 1024; /* (the kernel's static words, the barrier's among them, lie beside the dynamic part: 256 bytes by the compiler's count) */
    }
    return ctx->callboot_lds_bytes;
}
/* the refusals of every entry point, before anything is queued (no device involved): the family's spec, the replicates, the cap, out */
static int callboot_check(avk_ctx *ctx, int family, const avk_size_spec *sp, const avk_boot_spec *bs, uint32_t n_labels, const uint64_t *out, const char *out_name) {
    if (family == AVK_CALLBOOT_SIZE) {
        if (!sp) return fail(ctx, AVK_E_ARG, "size bins: spec missing");
        if (!avk_size_spec_ok(sp)) return fail(ctx, AVK_E_ARG, "size bins: 1 to %d edges, the first at least 1, strictly ascending", AVK_SIZE_EDGES_MAX);
    }
    if (bs->replicates < 1 || bs->replicates > AVK_BOOT_MAX_REPLICATES) return fail(ctx, AVK_E_ARG, "bootstrap: %u replicates, 1 to %u are possible", bs->replicates, AVK_BOOT_MAX_REPLICATES);
    const uint32_t n_keys = avk_callboot_n_keys(family, sp);
    if (!avk_callboot_blocks_ok((uint64_t)n_labels + 1, bs->replicates, n_keys))
        return fail(ctx, AVK_E_ARG, "per-call bootstrap: %u replicates of 1 + %u scopes and %u keys are more than %u blocks", bs->replicates, n_labels, n_keys, AVK_CALLBOOT_MAX_BLOCKS);
    if (!out) return fail(ctx, AVK_E_ARG, "%s missing", out_name);
    return 0;
}
uint32_t avk_callboot_block(avk_ctx *ctx, uint32_t n_keys) {
    if (!ctx || n_keys < 1 || n_keys > 16) return 0;
    if (hipSetDevice(ctx->device) != hipSuccess) return 0;
    return avk::cb::cb_reps(n_keys, (uint64_t)callboot_lds(ctx));
}
/* the kernel over the scopes and the blocks of replicates, on stream s behind whatever wrote the batch's results: d_out[(1 + n_labels) * B * n_keys * 182] gains the sums */
static int callboot_launch(avk_ctx *ctx, avk_dev_batch *db, int family, const avk_size_spec *sp, const avk_boot_spec *bs, uint32_t n_labels, const uint32_t *d_mask,
                           uint64_t *d_out, hipStream_t s) {
    const uint64_t n = db->n_regions;
    if (!n) return 0;
    avk::lb::LbView v;
    memset(&v, 0, sizeof(v));
    v.in = db->dp_args.in, v.vinfo = db->dp_args.vinfo, v.region_out = db->d_region_out, v.var_out = db->d_var_out, v.v_off = db->d_voff;
    avk_size_spec spec;
    memset(&spec, 0, sizeof(spec));
    if (family == AVK_CALLBOOT_SIZE) spec = *sp;
    const uint32_t n_keys = avk_callboot_n_keys(family, sp), B = bs->replicates;
    const uint32_t R = avk::cb::cb_reps(n_keys, (uint64_t)callboot_lds(ctx));
    const size_t lds = AVK_CB_LDS_BYTES(n_keys, R);
    if ((int64_t)lds > callboot_lds(ctx)) return fail(ctx, AVK_E_HIP, "per-call bootstrap: a launch needs %zu bytes of LDS, the device grants %lld", lds, (long long)callboot_lds(ctx));
    /* one workgroup a CU (its LDS), and no more workgroups than tiles: each flushes its accumulators once */
    uint64_t blocks = (n + AVK_CB_TILE - 1) / AVK_CB_TILE;
    if (blocks > (uint64_t)ctx->n_cus) blocks = (uint64_t)ctx->n_cus;
    const unsigned long long seed_mix = avk_boot_mix(bs->seed);
    for (uint32_t scope = 0; scope <= (d_mask ? n_labels : 0u); ++scope)
        for (uint32_t lo = 0; lo < B; lo += R) {
            const uint32_t hi = B - lo > R ? lo + R : B;
            hipLaunchKernelGGL(avk_callboot_tally_kernel, dim3((unsigned)blocks), dim3(AVK_CB_THREADS), lds, s, v, d_mask, (uint32_t)n, family, spec, n_keys, scope, seed_mix, B, lo, hi,
                               R, (unsigned long long *)d_out);
            AVK_HIP(ctx, hipGetLastError());
        }
    return 0;
}
/* a solved resident batch: the scopes' membership (the strata pass's masks), sums cleared, kernels, copy back, wait, added to the caller's: on the context's stream */
static int callboot_resident_run(avk_ctx *ctx, avk_dev_batch *db, int family, const avk_size_spec *sp, const avk_boot_spec *bs, const avk_strata *st, uint64_t *out) {
    const uint64_t n = db->n_regions;
    StrataLists L;
    int rc = 0;
    if (st && st->n_labels && n) {
        rc = strata_lists_alloc(ctx, st, n, L);
        if (!rc) {
            const hipError_t e = strata_mask_launch(st, db->dp_args.in, n, (uint32_t *)L.d_mask, (uint64_t *)L.d_sums, ctx->stream);
            if (e != hipSuccess) rc = fail(ctx, AVK_E_HIP, "strata masks failed: %s", hipGetErrorString(e));
        }
    }
    if (rc) {
        (void)hipStreamSynchronize(ctx->stream);
        strata_lists_release(ctx, L);
        return rc;
    }
    const uint32_t n_labels = L.d_mask ? st->n_labels : 0;
    const size_t words = ((size_t)n_labels + 1) * bs->replicates * avk_callboot_n_keys(family, sp) * AVK_CALLBOOT_KEY_WORDS;
    std::vector<uint64_t> host(words, 0);
    void *d_out = nullptr;
    rc = pool_alloc(ctx, &d_out, words * 8);
    hipError_t e = hipSuccess;
    if (!rc) e = hipMemsetAsync(d_out, 0, words * 8, ctx->stream);
    if (!rc && e == hipSuccess) rc = callboot_launch(ctx, db, family, sp, bs, n_labels, (const uint32_t *)L.d_mask, (uint64_t *)d_out, ctx->stream);
    if (!rc && e == hipSuccess) e = hipMemcpyAsync(host.data(), d_out, words * 8, hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t es = hipStreamSynchronize(ctx->stream);
    pool_release(ctx, d_out);
    strata_lists_release(ctx, L);
    if (rc) return rc;
    if (e != hipSuccess || es != hipSuccess) return fail(ctx, AVK_E_HIP, "per-call bootstrap tallies failed: %s", hipGetErrorString(e != hipSuccess ? e : es));
    for (size_t k = 0; k < words; ++k) out[k] += host[k];
    return 0;
}
static int callboot_tallies(avk_ctx *ctx, avk_dev_batch *db, int family, const avk_size_spec *sp, const avk_boot_spec *bs, const avk_strata *st, uint64_t *out, const char *out_name) {
    if (!ctx || !db || !bs) return AVK_E_ARG;
    if (st && strata_handle_check(ctx, st)) return AVK_E_ARG; /* (before anything of the handle is read) */
    {
        const int rb = callboot_check(ctx, family, sp, bs, st ? st->n_labels : 0, out, out_name);
        if (rb) return rb;
    }
    if (!db->dev_packed)
        return fail(ctx, AVK_E_STATE, "per-call bootstrap tallies on the device need a device-packed batch: the option device_pack was 0 at its upload (host route: avk_%s_boot_tallies_host)",
                    family == AVK_CALLBOOT_KIND ? "kind" : "size");
    if (!db->has_run || db->last_mode != 0) return fail(ctx, AVK_E_STATE, "per-call bootstrap tallies need a batch that avk_compare_resident has solved");
    AVK_HIP(ctx, hipSetDevice(ctx->device));
    return callboot_resident_run(ctx, db, family, sp, bs, st, out);
}
int avk_size_boot_tallies(avk_ctx *ctx, avk_dev_batch *db, const avk_size_spec *sp, const avk_boot_spec *bs, const avk_strata *st, uint64_t *out) {
    return callboot_tallies(ctx, db, AVK_CALLBOOT_SIZE, sp, bs, st, out, "size_boot_tallies");
}
int avk_kind_boot_tallies(avk_ctx *ctx, avk_dev_batch *db, const avk_boot_spec *bs, const avk_strata *st, uint64_t *out) {
    return callboot_tallies(ctx, db, AVK_CALLBOOT_KIND, nullptr, bs, st, out, "kind_boot_tallies");
}

/* host only: the checks here, the sums in avk_callboot_host.h (X_r from the wide batch and its results, weighted with avk_boot.h's rule) */
static int callboot_tallies_host(const avk_region_batch *b, const avk_result_batch *res, int family, const avk_size_spec *sp, const avk_boot_spec *bs, const avk_region_labels *lab,
                                 uint32_t threads, uint64_t *out, const char *out_name) {
    if (!b || !res || !bs) return fail(nullptr, AVK_E_ARG, "per-call bootstrap: batch, results or spec missing");
    const uint32_t n_labels = lab ? lab->n_labels : 0;
    {
        const int rb = callboot_check(nullptr, family, sp, bs, n_labels, out, out_name);
        if (rb) return rb;
        if (lab && n_labels) {
            const int rl = labels_check(nullptr, b->n_regions, lab, out);
            if (rl) return rl;
        }
    }
    if (!(res->status || res->region_packed)) return fail(nullptr, AVK_E_ARG, "per-call bootstrap: the results have neither status nor region_packed");
    const bool wide_calls = res->var_expected && res->var_observed;
    if (!wide_calls && !res->var_packed) return fail(nullptr, AVK_E_ARG, "per-call bootstrap: the results have no per-call outputs");
    if (b->n_regions && !b->start) return fail(nullptr, AVK_E_ARG, "per-call bootstrap: the batch has no start array");
    if (avk::cbh::callboot_host_sum(b, res, family, sp, bs, lab && n_labels ? lab : nullptr, threads, out, avk::host_edit_distance))
        return fail(nullptr, AVK_E_ARG, "per-call bootstrap: a region's calls lie outside the batch");
    return 0;
}
int avk_size_boot_tallies_host(const avk_region_batch *b, const avk_result_batch *res, const avk_size_spec *sp, const avk_boot_spec *bs, const avk_region_labels *lab, uint32_t threads,
                               uint64_t *out) {
    return callboot_tallies_host(b, res, AVK_CALLBOOT_SIZE, sp, bs, lab, threads, out, "size_boot_tallies");
}
int avk_kind_boot_tallies_host(const avk_region_batch *b, const avk_result_batch *res, const avk_boot_spec *bs, const avk_region_labels *lab, uint32_t threads, uint64_t *out) {
    return callboot_tallies_host(b, res, AVK_CALLBOOT_KIND, nullptr, bs, lab, threads, out, "kind_boot_tallies");
}

int avk_compare_packed_submit_strata(avk_ctx *ctx, const avk_packed_batch *batch, const avk_packed_escapes *esc, const avk_strata *st, const avk_compare_config *cfg,
                                     avk_result_batch *out, uint64_t *label_tallies, avk_ticket **ticket) {
    if (!st || st->n_labels == 0) return submit_impl(ctx, batch, cfg, out, ticket, nullptr, nullptr, esc); /* the submit without labels, launch for launch */
    if (!ctx) return AVK_E_ARG;
    if (!label_tallies) return fail(ctx, AVK_E_ARG, "label_tallies missing");
    if (strata_handle_check(ctx, st)) return AVK_E_ARG;
    return submit_impl(ctx, batch, cfg, out, ticket, nullptr, nullptr, esc, nullptr, label_tallies, st);
}

/* solve_merge_region's pairwise test (merge_solver.rs:128-147) for every region of the batch: the "truth"
 * range is input i, the "query" range input j */
int avk_optimize_pairs_batch(avk_ctx *ctx, const avk_region_batch *batch, uint32_t max_branch_factor, int32_t *status, uint8_t *is_exact_match) {
    if (!ctx || !batch || !status || !is_exact_match) return AVK_E_ARG;
    if (!ctx->d_ref) return fail(ctx, AVK_E_STATE, "avk_ref_upload has not been called");
    avk_compare_config cfg;
    cfg.max_branch_factor = max_branch_factor;
    cfg.enable_sequences = 0;
    cfg.enable_exact_shortcut = 0;
    avk_dev_batch *db = nullptr;
    CallSpec spec = call_spec(ctx);
    spec.emit_gm = false; /* the pair solve writes no metric blocks */
    int rc = upload_internal(ctx, spec, batch, true, &db);
    if (rc) return rc;
    rc = run_internal(ctx, spec, db, &cfg, nullptr, 1);
    if (!rc && db->dev_packed) { /* status and the exact-match flag in the caller's layout come from dp_unpack */
        avk_result_batch ro;
        memset(&ro, 0, sizeof(ro));
        ro.status = status;
        std::vector<uint64_t> tally((size_t)AVK_TALLY_STRIDE);
        rc = download_device_packed(ctx, spec, db, &ro, is_exact_match, tally.data());
        ctx->last_one_shot = rc == 0;
        memcpy(ctx->last_tiers, tally.data() + AVK_TALLY_LEN, 5 * sizeof(uint64_t));
        ctx->last_lane_solved = tally[AVK_TALLY_LANE_SOLVED];
        ctx->last_wide_solved = tally[AVK_TALLY_WIDE_SOLVED];
    } else if (!rc) {
        std::vector<uint32_t> rout(db->n_regions * 4 + 4);
        hipError_t e = hipMemcpyAsync(rout.data(), db->d_region_out, db->n_regions * 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) rc = fail(ctx, AVK_E_HIP, "pairs download failed: %s", hipGetErrorString(e));
        else
            for (uint64_t r = 0; r < db->n_regions; ++r) {
                status[r] = (int32_t)rout[4 * r];
                is_exact_match[r] = status[r] == 0 && rout[4 * r + 1] ? 1 : 0;
            }
    }
    avk_batch_free(ctx, db);
    return rc;
}

/* solve_merge_region's classification (merge_solver.rs:149-199) on top of the pair matrix */
int avk_merge_classify(uint64_t n_regions, uint32_t k, const uint32_t *in_cnt, const uint8_t *has_unknown_zyg, const int32_t *pair_status,
                       const uint8_t *pair_exact, const avk_merge_config *cfg, int32_t *status, uint8_t *classification, uint64_t *members) {
    if (!in_cnt || !cfg || !status || !classification || !members || (n_regions && (!pair_status || !pair_exact))) return AVK_E_ARG;
    if (k < 1 || k > 64) return AVK_E_ARG;
    const uint64_t ppr = (uint64_t)k * (k - 1) / 2;
    for (uint64_t m = 0; m < n_regions; ++m) {
        const int32_t *pst = pair_status + m * ppr;
        const uint8_t *pex = pair_exact + m * ppr;
        avk::dp::merge_classify_one<64>(k, in_cnt + m * k, has_unknown_zyg && has_unknown_zyg[m], [pst, pex](uint64_t p, int32_t &st, bool &ex) {
            st = pst[p];
            ex = pex[p] != 0;
        }, cfg->no_conflict_enabled, cfg->majority_voting_enabled, cfg->conflict_selection, status + m, classification + m, members + m);
    }
    return 0;
}

static bool merge_on_device(const avk_ctx *ctx, uint64_t n_regions, uint32_t k) {
    return ctx->device_pack && k >= 2 && k <= (uint32_t)avk::dp::DP_MERGE_KMAX && n_regions && n_regions * (uint64_t)(k * (k - 1) / 2) <= 0x7FFFFFFFull;
}
/* n_sweep = 0: the one config *cfg, the launches of avk_merge_packed_counts.  n_sweep >= 1 (avk_merge_packed_sweep): cfg[n_sweep] with one max_branch_factor, decided on
 * top of ONE pair solve; classification / members are config-major and counts holds a block per config. */
static int merge_batch_internal(avk_ctx *ctx, const avk_multi_batch *mb, const avk_packed_multi_batch *pm, const avk_merge_config *cfg, int32_t *status, uint8_t *classification,
                                uint64_t *members, const avk_packed_escapes *esc = nullptr, uint64_t *counts = nullptr, uint32_t n_sweep = 0);
static int merge_packed_internal(avk_ctx *ctx, const avk_packed_multi_batch *pm, const avk_packed_escapes *esc, const avk_merge_config *cfg, int32_t *status, uint8_t *classification,
                                 uint64_t *members, uint64_t *counts, uint32_t n_sweep = 0);
/* the LDS a launch of the count kernel really gets (as for the label kernel: the whole CU's where the runtime grants it) */
static int64_t mergecount_lds(avk_ctx *ctx) {
    if (!ctx->mergecount_lds_bytes) {
        int64_t b = 64 * 1024;
        if (hipFuncSetAttribute((const void *)avk_merge_count_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess) b = 160 * 1024;
        else {
            (void)hipGetLastError();
            int attr = 0;
            if (hipDeviceGetAttribute(&attr, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device) == hipSuccess && attr > 0 && attr < b) b = attr;
            else (void)hipGetLastError();
        }
        ctx->mergecount_lds_bytes = b;
    }
    return ctx->mergecount_lds_bytes;
}
int avk_merge_counts_in_lds(avk_ctx *ctx, uint32_t n_inputs) {
    if (!ctx || avk_merge_counts_len(n_inputs) == 0) return 0;
    (void)hipSetDevice(ctx->device);
    return avk::mc::mc_fits_lds(n_inputs, (uint64_t)mergecount_lds(ctx)) ? 1 : 0;
}
int avk_last_merge_counts_on_device(avk_ctx *ctx) { return ctx ? ctx->last_merge_counts_on_device : 0; }

/* The merge call with MergeSummaryWriter's counters: the batch's dense block is ADDED to counts[avk_merge_counts_len(k)].  On the device route the count kernel
 * runs behind the classification kernel and its block comes back with the three result arrays; a batch without a device route is counted by
 * avk_merge_counts_esc after the solve.  Either way a batch the host function refuses — or one with a call whose type nibble is no VariantType, in whatever
 * region — is AVK_E_ARG with counts untouched (status / classification / members are then what the call without counters leaves). */
int avk_merge_packed_counts(avk_ctx *ctx, const avk_packed_multi_batch *pm, const avk_packed_escapes *esc, const avk_merge_config *cfg, int32_t *status, uint8_t *classification,
                            uint64_t *members, uint64_t *counts) {
    if (!counts) return avk_merge_packed_esc(ctx, pm, esc, cfg, status, classification, members);
    if (!ctx || !pm || !cfg || !status || !classification || !members) return AVK_E_ARG;
    ctx->last_merge_counts_on_device = 0;
    if (avk_merge_counts_len(pm->n_inputs) == 0) return fail(ctx, AVK_E_ARG, "summary counters exist for 2 to %d inputs (n_inputs %u)", AVK_MERGE_COUNTS_MAX_INPUTS, pm->n_inputs);
    return merge_packed_internal(ctx, pm, esc, cfg, status, classification, members, counts);
}

int avk_merge_packed(avk_ctx *ctx, const avk_packed_multi_batch *pm, const avk_merge_config *cfg, int32_t *status, uint8_t *classification, uint64_t *members) {
    return avk_merge_packed_esc(ctx, pm, nullptr, cfg, status, classification, members);
}
int avk_merge_packed_esc(avk_ctx *ctx, const avk_packed_multi_batch *pm, const avk_packed_escapes *esc, const avk_merge_config *cfg, int32_t *status, uint8_t *classification,
                         uint64_t *members) {
    return merge_packed_internal(ctx, pm, esc, cfg, status, classification, members, nullptr);
}
/* the decisions of several configs on top of one pair matrix (avk_mergesweep.inl) */
int avk_merge_classify_sweep(uint64_t n_regions, uint32_t k, const uint32_t *in_cnt, const uint8_t *has_unknown_zyg, const int32_t *pair_status, const uint8_t *pair_exact,
                             uint32_t n_cfgs, const avk_merge_config *cfgs, int32_t *status, uint8_t *classification, uint64_t *members) {
    return avk::ms::merge_classify_sweep_host(n_regions, k, in_cnt, has_unknown_zyg, pair_status, pair_exact, n_cfgs, cfgs, status, classification, members);
}
/* One pair solve, n_cfgs decisions (include/aardvark_amd.h).  Everything that can be refused from the arguments alone is refused here, before anything is queued. */
int avk_merge_packed_sweep(avk_ctx *ctx, const avk_packed_multi_batch *pm, const avk_packed_escapes *esc, uint32_t n_cfgs, const avk_merge_config *cfgs, int32_t *status,
                           uint8_t *classification, uint64_t *members, uint64_t *counts) {
    if (!ctx || !pm || !cfgs || !status || !classification || !members) return AVK_E_ARG;
    ctx->last_merge_counts_on_device = 0;
    if (n_cfgs < 1 || n_cfgs > (uint32_t)AVK_MERGE_SWEEP_MAX) return fail(ctx, AVK_E_ARG, "a sweep takes 1 to %d configs (n_cfgs %u)", AVK_MERGE_SWEEP_MAX, n_cfgs);
    if (pm->n_inputs < 1 || pm->n_inputs > 64) return fail(ctx, AVK_E_ARG, "n_inputs must be in [1, 64]");
    for (uint32_t c = 0; c < n_cfgs; ++c) {
        if (cfgs[c].max_branch_factor != cfgs[0].max_branch_factor)
            return fail(ctx, AVK_E_ARG, "the configs of a sweep share one pair solve: config %u has max_branch_factor %u, config 0 has %u", c, cfgs[c].max_branch_factor, cfgs[0].max_branch_factor);
        if (!avk::ms::merge_sweep_cfg_ok(pm->n_inputs, cfgs[c]))
            return fail(ctx, AVK_E_ARG, "config %u: conflict_selection %d is not -1 or one of the %u inputs", c, cfgs[c].conflict_selection, pm->n_inputs);
    }
    if (counts && avk_merge_counts_len(pm->n_inputs) == 0)
        return fail(ctx, AVK_E_ARG, "summary counters exist for 2 to %d inputs (n_inputs %u)", AVK_MERGE_COUNTS_MAX_INPUTS, pm->n_inputs);
    return merge_packed_internal(ctx, pm, esc, cfgs, status, classification, members, counts, n_cfgs);
}
static int merge_packed_internal(avk_ctx *ctx, const avk_packed_multi_batch *pm, const avk_packed_escapes *esc, const avk_merge_config *cfg, int32_t *status, uint8_t *classification,
                                 uint64_t *members, uint64_t *counts, uint32_t n_sweep) {
    if (!ctx || !pm || !cfg || !status || !classification || !members) return AVK_E_ARG;
    if (!esc_present(esc)) esc = nullptr;
    const uint32_t k = pm->n_inputs;
    if (k < 1 || k > 64) return fail(ctx, AVK_E_ARG, "n_inputs must be in [1, 64]");
    const uint64_t n = pm->n_regions, nv = pm->n_variants;
    if (n && (!pm->start || !pm->len || !pm->in_cnt)) return fail(ctx, AVK_E_ARG, "region arrays missing");
    if (nv && (!pm->var_rel_pos || !pm->var_type_zyg || !pm->a0_len || !pm->a1_len || !pm->allele_bytes)) return fail(ctx, AVK_E_ARG, "variant arrays missing");
    avk_multi_batch mb;
    memset(&mb, 0, sizeof(mb));
    mb.n_regions = n, mb.n_inputs = k, mb.n_variants = nv, mb.allele_bytes = pm->allele_bytes, mb.allele_bytes_len = pm->allele_bytes_len;
    if (merge_on_device(ctx, n, k)) return merge_batch_internal(ctx, &mb, pm, cfg, status, classification, members, esc, counts, n_sweep);
    if (counts) { /* no device route: the solve as it is, then the host's count into a block of its own (nothing reaches counts[] of a batch that is refused) */
        int rc = merge_packed_internal(ctx, pm, esc, cfg, status, classification, members, nullptr, n_sweep);
        if (rc) return rc;
        for (uint64_t v = 0; v < nv; ++v)
            if ((pm->var_type_zyg[v] & 15u) >= AVK_N_VARIANT_TYPES) return fail(ctx, AVK_E_ARG, "summary counters: call %llu has the unknown type %u", (unsigned long long)v, pm->var_type_zyg[v] & 15u);
        const uint32_t nc = n_sweep ? n_sweep : 1u; /* (a sweep: a block per config, and none of them reaches counts[] unless all are made) */
        const size_t len = (size_t)avk_merge_counts_len(k);
        std::vector<uint64_t> block(len * nc, 0);
        for (uint32_t c = 0; c < nc && !rc; ++c) rc = avk_merge_counts_esc(pm, esc, status, classification + (size_t)c * n, members + (size_t)c * n, block.data() + c * len);
        if (rc) return fail(ctx, AVK_E_ARG, "summary counters: the batch and its results do not fit together (call counts, escape lists, classifications)");
        for (size_t w = 0; w < block.size(); ++w) counts[w] += block[w];
        return AVK_E_OK;
    }
    PackedWideHost wh;
    if (!packed_widen_host(pm->len, n, pm->in_cnt, nullptr, n * k, pm->var_rel_pos, pm->a0_len, pm->a1_len, nv, esc, wh))
        return fail(ctx, AVK_E_ARG, "packed batch: an escape list is not ascending, names an entry outside the batch, or lists an entry whose narrow field is not 0");
    /* no device path for this batch (more than DP_MERGE_KMAX inputs, an empty batch, device_pack = 0): the wide form, made here, through avk_merge_batch */
    std::vector<uint64_t> start(n), end(n), in_off(n * k), pos(nv), a0_off(nv), a1_off(nv);
    std::vector<uint32_t> contig(n), in_cnt(n * k), a0_len(nv), a1_len(nv), raw(nv);
    std::vector<uint8_t> type(nv + 1), zyg(nv + 1);
    uint64_t v = 0, ab = 0;
    for (uint64_t m = 0; m < n; ++m) {
        contig[m] = pm->contig_idx ? pm->contig_idx[m] : 0u, start[m] = pm->start[m], end[m] = (uint64_t)pm->start[m] + wh.len[m];
        for (uint32_t i = 0; i < k; ++i) {
            in_off[m * k + i] = v, in_cnt[m * k + i] = wh.cnt[m * k + i];
            for (uint32_t q = 0; q < wh.cnt[m * k + i]; ++q, ++v) {
                if (v >= nv) return fail(ctx, AVK_E_ARG, "packed batch: the call counts sum to more than n_variants %llu", (unsigned long long)nv);
                pos[v] = start[m] + wh.rel[v];
            }
        }
    }
    if (v != nv) return fail(ctx, AVK_E_ARG, "packed batch: the call counts sum to %llu (n_variants %llu)", (unsigned long long)v, (unsigned long long)nv);
    for (v = 0; v < nv; ++v) {
        a0_off[v] = ab, a0_len[v] = wh.a0[v], a1_off[v] = ab + a0_len[v], a1_len[v] = wh.a1[v], ab += (uint64_t)a0_len[v] + a1_len[v];
        raw[v] = pm->var_raw_space ? pm->var_raw_space[v] : (a0_len[v] > a1_len[v] ? a0_len[v] : a1_len[v]);
        type[v] = pm->var_type_zyg[v] & 15u, zyg[v] = pm->var_type_zyg[v] >> 4;
    }
    if (ab != pm->allele_bytes_len && nv) return fail(ctx, AVK_E_ARG, "packed batch: the allele lengths sum to %llu (allele_bytes_len %llu)", (unsigned long long)ab, (unsigned long long)pm->allele_bytes_len);
    mb.contig_idx = contig.data(), mb.start = start.data(), mb.end = end.data(), mb.in_off = in_off.data(), mb.in_cnt = in_cnt.data(), mb.var_pos = pos.data(), mb.var_type = type.data(),
    mb.var_zyg = zyg.data(), mb.var_raw_space = raw.data(), mb.a0_off = a0_off.data(), mb.a0_len = a0_len.data(), mb.a1_off = a1_off.data(), mb.a1_len = a1_len.data();
    return merge_batch_internal(ctx, &mb, nullptr, cfg, status, classification, members, nullptr, nullptr, n_sweep);
}

int avk_merge_batch(avk_ctx *ctx, const avk_multi_batch *mb, const avk_merge_config *cfg, int32_t *status, uint8_t *classification, uint64_t *members) {
    return merge_batch_internal(ctx, mb, nullptr, cfg, status, classification, members);
}

static int merge_batch_internal(avk_ctx *ctx, const avk_multi_batch *mb, const avk_packed_multi_batch *pm, const avk_merge_config *cfg, int32_t *status, uint8_t *classification,
                                uint64_t *members, const avk_packed_escapes *esc, uint64_t *counts, uint32_t n_sweep) {
    if (!ctx || !mb || !cfg || !status || !classification || !members) return AVK_E_ARG;
    const uint32_t k = mb->n_inputs;
    const uint32_t nc = n_sweep ? n_sweep : 1u; /* decisions per region */
    if (k < 1 || k > 64) return fail(ctx, AVK_E_ARG, "n_inputs must be in [1, 64]");
    if (merge_on_device(ctx, mb->n_regions, k)) {
        /* all of solve_merge_region on the device: the MultiRegions as they are over PCIe, one region per input pair made by a kernel, the pair solve (mode 1),
         * the decision on top of the pair matrix by a kernel; status / classification / members come back */
        if (!ctx->d_ref) return fail(ctx, AVK_E_STATE, "avk_ref_upload has not been called");
        AVK_HIP(ctx, hipSetDevice(ctx->device));
        avk_dev_batch *db = nullptr;
        CallSpec spec = call_spec(ctx);
        spec.emit_gm = false; /* the pair solve writes no metric blocks */
        int rc = upload_device_packed(ctx, spec, pm ? UploadSource::of(pm, *mb, esc) : UploadSource::of(mb), nullptr, &db);
        if (rc) return rc;
        avk_compare_config pcfg;
        pcfg.max_branch_factor = cfg->max_branch_factor, pcfg.enable_sequences = 0, pcfg.enable_exact_shortcut = 0;
        rc = run_internal(ctx, spec, db, &pcfg, nullptr, 1);
        const uint64_t nm = mb->n_regions;
        void *d_st = nullptr, *d_cl = nullptr, *d_mem = nullptr;
        if (!rc) rc = pool_alloc(ctx, &d_st, (nm + 1) * 4);
        if (!rc) rc = pool_alloc(ctx, &d_cl, nc * nm + 16);
        if (!rc) rc = pool_alloc(ctx, &d_mem, (nc * nm + 1) * 8);
        if (!rc && n_sweep) { /* every config's decision by one kernel: the pair records are read once */
            avk::ms::MsSweep c;
            memset(&c, 0, sizeof(c));
            c.region_out = db->d_region_out, c.in_off = db->d_m_in_off, c.in_cnt = db->d_m_in_cnt, c.var_zyg = db->d_in_zyg, c.n_multi = nm, c.n_variants = mb->n_variants, c.k = k,
            c.ppr = k * (k - 1) / 2, c.n_cfgs = nc;
            for (uint32_t q = 0; q < nc; ++q)
                c.cfg[q].no_conflict_enabled = cfg[q].no_conflict_enabled, c.cfg[q].majority_voting_enabled = cfg[q].majority_voting_enabled, c.cfg[q].conflict_selection = cfg[q].conflict_selection;
            c.status = (int32_t *)d_st, c.classification = (uint8_t *)d_cl, c.members = (uint64_t *)d_mem;
            hipLaunchKernelGGL(avk_merge_sweep_kernel, dim3((unsigned)((nm + 255) / 256)), dim3(256), 0, ctx->stream, c);
            hipError_t e = hipGetLastError();
            if (e != hipSuccess) rc = fail(ctx, AVK_E_HIP, "merge sweep failed: %s", hipGetErrorString(e));
        } else if (!rc) {
            avk::dp::DpMerge c;
            memset(&c, 0, sizeof(c));
            c.region_out = db->d_region_out, c.in_off = db->d_m_in_off, c.in_cnt = db->d_m_in_cnt, c.var_zyg = db->d_in_zyg, c.n_multi = nm, c.n_variants = mb->n_variants, c.k = k,
            c.ppr = k * (k - 1) / 2, c.no_conflict_enabled = cfg->no_conflict_enabled, c.majority_voting_enabled = cfg->majority_voting_enabled, c.conflict_selection = cfg->conflict_selection;
            c.status = (int32_t *)d_st, c.classification = (uint8_t *)d_cl, c.members = (uint64_t *)d_mem;
            hipLaunchKernelGGL(avk_dp_merge_classify_kernel, dim3((unsigned)((nm + 255) / 256)), dim3(256), 0, ctx->stream, c);
            hipError_t e = hipGetLastError();
            if (e != hipSuccess) rc = fail(ctx, AVK_E_HIP, "merge classification failed: %s", hipGetErrorString(e));
        }
        /* the summary counters (avk_merge_packed_counts): a cleared block and its error word behind it, the count kernel behind the classification — of a sweep: a block
         * and an error word per config, the count kernel once per config on that config's slices */
        const size_t words = counts ? (size_t)avk::mc::merge_counts_words(k) : 0;
        void *d_cnt = nullptr;
        std::vector<uint64_t> h_cnt(counts ? nc * (words + 1) : 0);
        if (!rc && counts) rc = pool_alloc(ctx, &d_cnt, nc * (words + 1) * 8);
        if (!rc && counts) {
            const int64_t lds_max = mergecount_lds(ctx);
            const bool in_lds = avk::mc::mc_fits_lds(k, (uint64_t)lds_max);
            const size_t lds = in_lds ? words * 8 : 0;
            avk::mc::McView v;
            memset(&v, 0, sizeof(v));
            v.status = (const int32_t *)d_st, v.classification = (const uint8_t *)d_cl, v.members = (const uint64_t *)d_mem, v.in_off = db->d_m_in_off, v.in_cnt = db->d_m_in_cnt,
            v.var_type = db->d_in_type, v.n_regions = nm, v.n_variants = mb->n_variants, v.k = k;
            /* a CU runs 2,048 work-items: two workgroups where their blocks fit beside each other (and where there are none) */
            const uint32_t per_cu = lds * 2 <= (size_t)lds_max ? 2u : 1u;
            uint64_t blocks = (nm * k + 1023) / 1024;
            if (blocks > (uint64_t)ctx->n_cus * per_cu) blocks = (uint64_t)ctx->n_cus * per_cu;
            hipError_t e = hipMemsetAsync(d_cnt, 0, nc * (words + 1) * 8, ctx->stream);
            for (uint32_t q = 0; q < nc && e == hipSuccess; ++q) {
                uint64_t *block = (uint64_t *)d_cnt + q * (words + 1);
                v.classification = (const uint8_t *)d_cl + (size_t)q * nm, v.members = (const uint64_t *)d_mem + (size_t)q * nm;
                hipLaunchKernelGGL(avk_merge_count_kernel, dim3((unsigned)blocks), dim3(1024), lds, ctx->stream, v, (uint32_t)(in_lds ? words : 0), (unsigned long long *)block,
                                   (uint32_t *)(block + words));
                e = hipGetLastError();
            }
            if (e != hipSuccess) rc = fail(ctx, AVK_E_HIP, "merge counting failed: %s", hipGetErrorString(e));
        }
        if (!rc) {
            std::vector<CopySeg> segs = {{status, d_st, nm * 4}, {classification, d_cl, nc * nm}, {members, d_mem, nc * nm * 8}};
            if (counts) segs.push_back({h_cnt.data(), d_cnt, nc * (words + 1) * 8});
            CopyOut co;
            rc = copy_out(ctx, segs, &co);
            if (!rc) rc = finish_copy_out(ctx, co);
        }
        (void)hipStreamSynchronize(ctx->stream);
        pool_release(ctx, d_st), pool_release(ctx, d_cl), pool_release(ctx, d_mem), pool_release(ctx, d_cnt);
        if (!rc && counts) { /* the error words first: nothing of a refused batch reaches counts[], of whichever config */
            uint32_t err = 0;
            for (uint32_t q = 0; q < nc; ++q) err |= (uint32_t)h_cnt[q * (words + 1) + words];
            if (err)
                rc = fail(ctx, AVK_E_ARG, "summary counters: %s", err & avk::mc::MC_ERR_TYPE    ? "a call's type is none of the variant types"
                                                                  : err & avk::mc::MC_ERR_RANGE ? "an input's calls are not inside the batch"
                                                                                                : "a solved region's classification is not a merge classification");
            else {
                for (uint32_t q = 0; q < nc; ++q)
                    for (size_t w = 0; w < words; ++w) counts[q * words + w] += h_cnt[q * (words + 1) + w];
                ctx->last_merge_counts_on_device = 1;
            }
        }
        ctx->last_one_shot = rc == 0;
        avk_batch_free(ctx, db);
        return rc;
    }
    const uint64_t n = mb->n_regions, ppr = (uint64_t)k * (k - 1) / 2, np = n * ppr;
    /* one CompareRegion-shaped item per (i < j) pair: input i plays the truth side, input j the query side */
    std::vector<uint64_t> rid(np), st(np), en(np), t_off(np), q_off(np);
    std::vector<uint32_t> cidx(np), t_cnt(np), q_cnt(np);
    std::vector<uint8_t> unknown(n, 0);
    uint64_t p = 0;
    for (uint64_t m = 0; m < n; ++m) {
        for (uint32_t i = 0; i < k; ++i) {
            const uint64_t off = mb->in_off[m * k + i];
            const uint32_t cnt = mb->in_cnt[m * k + i];
            if (off > mb->n_variants || cnt > mb->n_variants - off) return fail(ctx, AVK_E_ARG, "variant range of a region exceeds n_variants");
            for (uint32_t v = 0; v < cnt; ++v)
                if (mb->var_zyg[off + v] == AVK_ZYG_UNKNOWN) unknown[m] = 1;
        }
        for (uint32_t i = 0; i < k; ++i)
            for (uint32_t j = i + 1; j < k; ++j, ++p) {
                rid[p] = mb->region_id ? mb->region_id[m] : m;
                cidx[p] = mb->contig_idx ? mb->contig_idx[m] : 0;
                st[p] = mb->start[m];
                en[p] = mb->end[m];
                t_off[p] = mb->in_off[m * k + i];
                t_cnt[p] = mb->in_cnt[m * k + i];
                q_off[p] = mb->in_off[m * k + j];
                q_cnt[p] = mb->in_cnt[m * k + j];
            }
    }
    avk_region_batch b;
    memset(&b, 0, sizeof(b));
    b.n_regions = np;
    b.region_id = rid.data();
    b.contig_idx = cidx.data();
    b.start = st.data();
    b.end = en.data();
    b.t_off = t_off.data();
    b.t_cnt = t_cnt.data();
    b.q_off = q_off.data();
    b.q_cnt = q_cnt.data();
    b.n_variants = mb->n_variants;
    b.var_pos = mb->var_pos;
    b.var_type = mb->var_type;
    b.var_zyg = mb->var_zyg;
    b.var_raw_space = mb->var_raw_space;
    b.a0_off = mb->a0_off;
    b.a0_len = mb->a0_len;
    b.a1_off = mb->a1_off;
    b.a1_len = mb->a1_len;
    b.allele_bytes = mb->allele_bytes;
    b.allele_bytes_len = mb->allele_bytes_len;
    std::vector<int32_t> pst(np ? np : 1, 0);
    std::vector<uint8_t> pex(np ? np : 1, 0);
    if (np) {
        const int rc = avk_optimize_pairs_batch(ctx, &b, cfg->max_branch_factor, pst.data(), pex.data());
        if (rc) return rc;
    }
    if (n_sweep) return avk_merge_classify_sweep(n, k, mb->in_cnt, unknown.data(), pst.data(), pex.data(), n_sweep, cfg, status, classification, members);
    return avk_merge_classify(n, k, mb->in_cnt, unknown.data(), pst.data(), pex.data(), cfg, status, classification, members);
}

} /* extern "C" */
