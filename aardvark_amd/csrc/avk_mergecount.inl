/*
 * avk_mergecount.inl — MergeSummaryWriter's counters of a solved merge batch, by kernel.
 *
 * MergeSummaryWriter::add_merge_benchmark (src/writers/merge_summary.rs:57-81) adds every call of a solved region to the key (merge reason with its indices,
 * variant type, input) -> (pass, fail).  avk_merge_counts_esc (avk_shard_host.inl) makes the dense block of these sums on the host, after status,
 * classification and members have come back: one thread over every region, slot and call of the batch.  Everything it reads is on the device when
 * avk_dp_merge_classify_kernel ends — its three outputs, the slots' call ranges (in_off / in_cnt, widened already when the batch came with escapes) and the
 * calls' type bytes — so mc_slot below states the same rule for ONE slot (region, input), and the kernel runs one lane per slot behind the classification.
 *
 * Where the sums are kept.  A genome's merge puts most of its calls on a handful of keys (BasepairIdentical x Snv x input), so global atomics per call would
 * queue up on a few addresses.
 *   - mc_fits_lds(k, lds): the dense block of k inputs, avk::mc::merge_counts_words(k) 64-bit words, fits the LDS of the launch.  The workgroup clears a copy
 *     of the block in its LDS, its lanes add there (LDS atomics), and the words that are not zero are added to the global block once per workgroup.
 *     The block has 576 words for k = 2, 1,512 for 3, 3,648 for 4, 8,520 for 5, 19,584 (153 KB) for 6: with the 160 KB a gfx950 workgroup can get that is
 *     k <= 6, with 64 KB k <= 4.
 *   - beyond (k = 7 and 8 of the device route: 44,520 and 100,224 words): no staging.  The lanes of a wave that add to the same entry at the same time are
 *     found with the whole wave in step (ballot, shuffle, a butterfly sum), and one of them adds their sum to the global block — one 64-bit global atomic per
 *     distinct entry and step of a wave.
 * The rule is a function of k and the launch's LDS size alone.
 *
 * mc_open / mc_next / mc_slot are one-lane code without cross-lane primitives, so tests/emu/mergecount_emu.cpp runs the SAME function on the CPU against avk_merge_counts_esc.
 */
#ifndef AVK_MERGECOUNT_INL
#define AVK_MERGECOUNT_INL

#include "avk_merge_reason.h"
#include "avk_wave.h"

namespace avk {
namespace mc {

/* the error word of a launch */
enum { MC_ERR_TYPE = 1u /* a call's type nibble is not a VariantType */, MC_ERR_RANGE = 2u /* a slot's calls are not inside the batch */,
       MC_ERR_CLASS = 4u /* a solved region's classification is none of AVK_MERGE_*, or its ConflictSelection index is not an input */ };

/* the device view of a classified merge batch */
struct McView {
    const int32_t *status;         /* [n_regions] */
    const uint8_t *classification; /* [n_regions] */
    const uint64_t *members;       /* [n_regions] a mask, or the index of a ConflictSelection */
    const uint64_t *in_off;        /* [n_regions * k] first call of a slot */
    const uint32_t *in_cnt;        /* [n_regions * k] its calls (wide: the escapes applied) */
    const uint8_t *var_type;       /* [n_variants] the calls' types; the low nibble is read (the packed form's type | zygosity << 4 bytes serve as well) */
    uint64_t n_regions, n_variants;
    uint32_t k;
};

/* is_passing (merge_summary.rs:61-72): every input of a BasepairIdentical region, the selected one of a ConflictSelection (members is an INDEX there), the
 * listed ones of NoConflict / MajorityAgree (members is a mask), none of a Different region */
AVK_MR_HD bool mc_input_passes(uint8_t classification, uint64_t members, uint32_t input) {
    if (classification == AVK_MERGE_IDENTICAL) return true;
    if (classification == AVK_MERGE_CONFLICT_SELECTION) return members == input;
    return classification != AVK_MERGE_DIFFERENT && ((members >> input) & 1ull) != 0;
}

AVK_MR_HD bool mc_fits_lds(uint32_t k, uint64_t lds_bytes) { return merge_counts_words(k) * 8ull <= lds_bytes; }

/* One lane: slot s = region * k + input, in two steps so that the kernel can take a wave's slots through their additions side by side.  mc_open looks at the
 * slot (err(bits) sets bits of the error word); mc_next hands out the slot's next addition — entry e of the block gains n — until there is none.  Calls of one type
 * that follow each other are one addition.  A slot of an unsolved region adds nothing, but its calls' types are looked at like any other's: a batch with a call of
 * no VariantType is refused whatever became of the call's region.  Nothing is added for a slot that sets an error bit. */
struct McRun {
    uint64_t off;      /* the slot's first call */
    uint32_t cnt, j;   /* its calls, and how many of them have been handed out */
    uint32_t base;     /* (reason * AVK_N_VARIANT_TYPES) * k + input: the entry is (base + type * k) * 2 + fail */
    uint32_t fail;
};
template <class Err>
AVK_DEV McRun mc_open(const McView &v, uint64_t s, Err &&err) {
    McRun run;
    run.off = 0, run.cnt = 0, run.j = 0, run.base = 0, run.fail = 0;
    const uint64_t r = s / v.k;
    const uint32_t i = (uint32_t)(s % v.k);
    const uint64_t off = v.in_off[s];
    const uint32_t cnt = v.in_cnt[s];
    if (off > v.n_variants || (uint64_t)cnt > v.n_variants - off) {
        err((uint32_t)MC_ERR_RANGE);
        return run;
    }
    const bool solved = v.status[r] == 0;
    const uint8_t cls = v.classification[r];
    const uint64_t mem = v.members[r];
    if (solved && (cls > AVK_MERGE_CONFLICT_SELECTION || (cls == AVK_MERGE_CONFLICT_SELECTION && mem >= v.k))) {
        err((uint32_t)MC_ERR_CLASS);
        return run;
    }
    bool bad = false;
    for (uint32_t j = 0; j < cnt; ++j) bad = bad || (v.var_type[off + j] & 15u) >= (uint32_t)AVK_N_VARIANT_TYPES;
    if (bad) {
        err((uint32_t)MC_ERR_TYPE);
        return run;
    }
    if (!solved) return run;
    run.off = off, run.cnt = cnt;
    run.base = merge_reason(v.k, cls, mem) * (uint32_t)AVK_N_VARIANT_TYPES * v.k + i;
    run.fail = mc_input_passes(cls, mem, i) ? 0u : 1u;
    return run;
}
AVK_DEV bool mc_next(const McView &v, McRun &run, uint32_t &e, uint32_t &n) {
    if (run.j >= run.cnt) return false;
    const uint32_t vt = v.var_type[run.off + run.j] & 15u;
    uint32_t len = 1;
    while (run.j + len < run.cnt && (v.var_type[run.off + run.j + len] & 15u) == vt) ++len;
    e = (run.base + vt * v.k) * 2u + run.fail;
    n = len;
    run.j += len;
    return true;
}
/* the two together: every addition of slot s through add(e, n) */
template <class Add, class Err>
AVK_DEV void mc_slot(const McView &v, uint64_t s, Add &&add, Err &&err) {
    McRun run = mc_open(v, s, err);
    uint32_t e, n;
    while (mc_next(v, run, e, n)) add(e, n);
}

} // namespace mc
} // namespace avk

#ifndef AVK_EMU
/* The launch of one batch: `lds_words` is merge_counts_words(k) where mc_fits_lds said yes (the dynamic LDS of the launch holds that many 64-bit words), 0 beyond.
 * out[0 .. words) is the block, cleared by the host before the launch; err_word is cleared with it. */
__global__ void __launch_bounds__(1024) avk_merge_count_kernel(avk::mc::McView v, uint32_t lds_words, unsigned long long *out, uint32_t *err_word) {
    extern __shared__ __attribute__((aligned(16))) unsigned char avk_smem[];
    unsigned long long *acc = (unsigned long long *)avk_smem;
    const uint64_t n_slots = v.n_regions * v.k, step = (uint64_t)gridDim.x * blockDim.x;
    auto err = [err_word](uint32_t bits) { atomicOr(err_word, bits); };
    if (lds_words) {
        for (unsigned w = threadIdx.x; w < lds_words; w += blockDim.x) acc[w] = 0;
        __syncthreads();
        for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n_slots; s += step)
            avk::mc::mc_slot(v, s, [acc, lds_words](uint32_t e, uint32_t n) {
                if (e < lds_words) atomicAdd(acc + e, (unsigned long long)n);
            }, err);
        __syncthreads();
        for (unsigned w = threadIdx.x; w < lds_words; w += blockDim.x) {
            const unsigned long long x = acc[w];
            if (x) atomicAdd(out + w, x);
        }
        return;
    }
    /* beyond the LDS rule.  Every cross-lane step runs with the whole wave in it: the loop over the wave's slots goes by the wave's FIRST slot, the lanes take
     * their slots' additions side by side (lanes that have none left wait with have == false), and per round the entries that are met are taken one after the
     * other — the lowest lane that still has one names it, the lanes with the same entry are summed over the wave, that lane adds the sum. */
    const uint32_t words = (uint32_t)avk::mc::merge_counts_words(v.k);
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s - lane < n_slots; s += step) {
        avk::mc::McRun run;
        run.off = 0, run.cnt = 0, run.j = 0, run.base = 0, run.fail = 0;
        if (s < n_slots) run = avk::mc::mc_open(v, s, err);
        uint32_t e = 0, n = 0;
        bool have = avk::mc::mc_next(v, run, e, n);
        for (unsigned long long pending = __ballot(have); pending; pending = __ballot(have)) {
            while (pending) {
                const int leader = __builtin_ctzll(pending);
                const uint32_t le = (uint32_t)__shfl((int)e, leader);
                const bool mine = have && e == le;
                const unsigned long long group = __ballot(mine);
                unsigned long long sum = mine ? (unsigned long long)n : 0ull;
                for (int d = 32; d; d >>= 1) sum += __shfl_xor(sum, d);
                if (lane == (uint32_t)leader && le < words) atomicAdd(out + le, sum);
                pending &= ~group;
            }
            have = avk::mc::mc_next(v, run, e, n);
        }
    }
}
#endif

#endif /* AVK_MERGECOUNT_INL */
