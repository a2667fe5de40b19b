/*
 * strata_emu.cpp — the containment rule of the device-made label lists (aardvark_amd/csrc/avk_strata.inl) on the CPU.
 *
 * Test infrastructure like label_emu.cpp, and a translation unit of its own: sx_region_in_label is one-lane code (no cross-lane primitive), so the SAME source
 * the gfx950 kernels run is called here region by region and label by label, on the arrays the device would hold — the wide arrays of a batch or the packed
 * source, and the exported interval sets — and the lists are compared with the host's (tests/test_strata.py).  Built by tests/strata_emu_lib.py with the flags
 * of tests/emu/Makefile.
 */
#define AVK_EMU 1
#include <string.h>

#include "../../aardvark_amd/csrc/avk_strata.inl"

extern "C" {

/* the device view, array by array (names of avk::dp::DpIn); wide arrays, or — pk_start != NULL — the packed source */
struct strata_emu_view {
    uint64_t n_regions, n_variants;
    const uint32_t *contig_idx;
    const uint64_t *start, *t_off, *q_off;
    const uint32_t *t_cnt, *q_cnt;
    const uint64_t *var_pos;
    const uint32_t *a0_len;
    const uint32_t *pk_start;
    const uint16_t *pk_contig, *pk_rel;
    const uint8_t *pk_tc, *pk_qc, *pk_a0;
    const uint64_t *pk_voff;
    /* the exported sets (avf_strat_export) */
    uint32_t n_labels, n_contigs;
    const uint64_t *tree_off;
    const uint32_t *tree_start, *tree_end_max;
};

/* label_off[n + 1] and, when label_idx is not NULL, the indices: ascending within a region, the order of the kernels' bit masks */
int strata_emu_lists(const strata_emu_view *e, uint64_t *label_off, uint32_t *label_idx) {
    avk::dp::DpIn in;
    memset(&in, 0, sizeof(in));
    in.n_regions = e->n_regions, in.n_variants = e->n_variants;
    in.contig_idx = e->contig_idx, in.start = e->start, in.t_off = e->t_off, in.q_off = e->q_off, in.t_cnt = e->t_cnt, in.q_cnt = e->q_cnt, in.var_pos = e->var_pos, in.a0_len = e->a0_len;
    in.pk_start = e->pk_start, in.pk_contig = e->pk_contig, in.pk_rel = e->pk_rel, in.pk_tc = e->pk_tc, in.pk_qc = e->pk_qc, in.pk_a0 = e->pk_a0, in.pk_voff = e->pk_voff;
    avk::sx::SxTrees t;
    t.tree_off = e->tree_off, t.start = e->tree_start, t.end_max = e->tree_end_max, t.n_labels = e->n_labels, t.n_contigs = e->n_contigs;
    /* the kernels' passes with the kernels' own per-lane functions: a word of answers per 32 labels into word-major masks (sx_mask_word, the labels in the
     * kernel's chunks of 256), then offsets by a running sum and the lists from the masks (sx_fill_region) */
    const uint64_t n = e->n_regions;
    const uint32_t n_words = (e->n_labels + 31u) / 32u;
    uint32_t *mask = new uint32_t[(size_t)n * n_words + 1];
    for (uint64_t r = 0; r < n; ++r) {
        const avk::sx::SxSpan sp = avk::sx::sx_region_span(in, r, t.n_contigs);
        for (uint32_t lb = 0; lb < t.n_labels; lb += 256u) {
            const uint32_t chunk = t.n_labels - lb < 256u ? t.n_labels - lb : 256u;
            for (uint32_t j0 = 0; j0 < chunk; j0 += 32u)
                mask[avk::sx::sx_mask_at((lb + j0) >> 5, r, n)] = avk::sx::sx_mask_word(t, sp, lb + j0, chunk - j0 < 32u ? chunk - j0 : 32u, [&](uint32_t l, uint64_t &a, uint64_t &b) {
                    const uint64_t at = (uint64_t)l * t.n_contigs + sp.contig;
                    a = t.tree_off[at], b = t.tree_off[at + 1];
                });
        }
    }
    uint64_t at = 0;
    int bad = 0;
    for (uint64_t r = 0; r < n; ++r) {
        label_off[r] = at;
        const uint32_t k = avk::sx::sx_fill_region(mask, r, n, n_words, label_idx, at, ~0ull);
        /* the rule asked label by label says the same */
        uint32_t direct = 0;
        for (uint32_t l = 0; l < e->n_labels; ++l) direct += avk::sx::sx_region_in_label(in, t, r, l) ? 1u : 0u;
        if (direct != k) bad = 1;
        at += k;
    }
    label_off[n] = at;
    delete[] mask;
    return bad;
}

/* one query on the exported arrays: is [first, last] (inclusive) of contig c contained in label l — avf_strat_containments' question */
int strata_emu_contains(const strata_emu_view *e, uint32_t l, uint32_t c, uint64_t first, uint64_t last) {
    avk::sx::SxTrees t;
    t.tree_off = e->tree_off, t.start = e->tree_start, t.end_max = e->tree_end_max, t.n_labels = e->n_labels, t.n_contigs = e->n_contigs;
    if (l >= t.n_labels || c >= t.n_contigs) return 0;
    const uint64_t at = (uint64_t)l * t.n_contigs + c;
    return avk::sx::sx_tree_hit(t, t.tree_off[at], t.tree_off[at + 1], first, last) ? 1 : 0;
}

} /* extern "C" */
