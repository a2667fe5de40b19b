/*
 * mergecount_emu.cpp — the per-slot rule of the merge summary counters (aardvark_amd/csrc/avk_mergecount.inl) on the CPU.
 *
 * Test infrastructure like label_emu.cpp and strata_emu.cpp, and a translation unit of its own: mc_slot is one-lane code (no cross-lane primitive), so the SAME
 * source the gfx950 kernel runs is called here slot by slot on the arrays the device holds behind the classification kernel — status, classification, members,
 * the slots' wide call ranges, the calls' type bytes — and the block is compared with avk_merge_counts_esc's (tests/test_merge_counts_emu.py).  Built by
 * tests/mergecount_emu_lib.py with the flags of tests/emu/Makefile.
 */
#define AVK_EMU 1
#include <string.h>

#include "../../aardvark_amd/csrc/avk_mergecount.inl"

extern "C" {

struct mergecount_emu_view {
    uint64_t n_regions, n_variants;
    uint32_t k;
    const int32_t *status;
    const uint8_t *classification;
    const uint64_t *members;
    const uint64_t *in_off;
    const uint32_t *in_cnt;
    const uint8_t *var_type;
};

/* every slot of the batch through mc_slot: counts[merge_counts_words(k)] is ADDED to (as the kernel adds to its block), the return value is the error word */
uint32_t mergecount_emu_counts(const mergecount_emu_view *e, uint64_t *counts) {
    avk::mc::McView v;
    memset(&v, 0, sizeof(v));
    v.status = e->status, v.classification = e->classification, v.members = e->members, v.in_off = e->in_off, v.in_cnt = e->in_cnt, v.var_type = e->var_type;
    v.n_regions = e->n_regions, v.n_variants = e->n_variants, v.k = e->k;
    const uint64_t words = avk::mc::merge_counts_words(e->k);
    uint32_t err = 0;
    for (uint64_t s = 0; s < e->n_regions * e->k; ++s)
        avk::mc::mc_slot(v, s, [&](uint32_t entry, uint32_t n) {
            if (entry < words) counts[entry] += n;
            else err |= 0x80000000u; /* (an entry outside the block: never, whatever the inputs) */
        }, [&](uint32_t bits) { err |= bits; });
    return err;
}

uint32_t mergecount_emu_reason(uint32_t k, uint8_t classification, uint64_t members) { return avk::mc::merge_reason(k, classification, members); }
uint64_t mergecount_emu_words(uint32_t k) { return avk::mc::merge_counts_words(k); }
int mergecount_emu_fits_lds(uint32_t k, uint64_t lds_bytes) { return avk::mc::mc_fits_lds(k, lds_bytes) ? 1 : 0; }

} /* extern "C" */
