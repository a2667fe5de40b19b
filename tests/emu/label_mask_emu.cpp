/*
 * label_mask_emu.cpp — the stratified tally that reads a region's labels from the strata pass's BIT MASKS (lb_region_labels_mask, aardvark_amd/csrc/avk_labels.inl)
 * on the CPU, beside the tally that reads lists made from the same masks (sx_fill_region of avk_strata.inl, then lb_region_labels).
 *
 * Test infrastructure like label_emu.cpp, whose device view it shares, and a translation unit of its own: both functions are one-lane code (no cross-lane
 * primitive), so the SAME source the gfx950 kernels run is called here region by region, label block by label block (tests/test_label_mask.py).  Built by
 * tests/label_mask_emu_lib.py with the flags of tests/emu/Makefile.
 */
#define AVK_EMU 1
#include <string.h>

#include "../../aardvark_amd/csrc/avk_labels.inl"
#include "../../aardvark_amd/csrc/avk_strata.inl"

extern "C" {

/* label_emu_view of label_emu.cpp, field for field */
struct label_mask_emu_view {
    uint64_t n_regions, n_variants;
    const uint64_t *t_off, *q_off;
    const uint32_t *t_cnt, *q_cnt;
    const uint8_t *var_type, *var_zyg;
    const uint32_t *var_raw; /* may be NULL */
    const uint32_t *a0_len, *a1_len;
    const uint32_t *pk_start;
    const uint8_t *pk_tc, *pk_qc, *pk_tz, *pk_a0, *pk_a1;
    const uint64_t *pk_voff;
    const uint32_t *alt_ed;     /* [n_variants] */
    const uint32_t *region_out; /* [n][4] */
    const uint32_t *var_out, *v_off, *bp_off, *bp;
};

static void make_view(const label_mask_emu_view *e, avk::lb::LbView &v, avk::dp::DpVarInfo *vinfo) {
    memset(&v, 0, sizeof(v));
    v.in.n_regions = e->n_regions, v.in.n_variants = e->n_variants;
    v.in.t_off = e->t_off, v.in.q_off = e->q_off, v.in.t_cnt = e->t_cnt, v.in.q_cnt = e->q_cnt, v.in.var_type = e->var_type, v.in.var_zyg = e->var_zyg, v.in.var_raw = e->var_raw;
    v.in.a0_len = e->a0_len, v.in.a1_len = e->a1_len;
    v.in.pk_start = e->pk_start, v.in.pk_tc = e->pk_tc, v.in.pk_qc = e->pk_qc, v.in.pk_tz = e->pk_tz, v.in.pk_a0 = e->pk_a0, v.in.pk_a1 = e->pk_a1, v.in.pk_voff = e->pk_voff;
    for (uint64_t i = 0; i < e->n_variants; ++i) vinfo[i].alt_ed = e->alt_ed[i], vinfo[i].flags = 0, vinfo[i].a1lo = vinfo[i].a1hi = 0;
    v.vinfo = vinfo;
    v.region_out = e->region_out, v.var_out = e->var_out, v.v_off = e->v_off, v.bp_off = e->bp_off, v.bp = e->bp;
}

int label_mask_emu_block_max(void) { return AVK_LB_MASK_BLOCK_MAX; }

/* the lists sx_fill_region makes from word-major masks (mask[w * n + r], n_words words a region): label_off[n + 1], and with label_idx the indices */
int label_mask_emu_lists(const uint32_t *mask, uint64_t n, uint32_t n_words, uint64_t *label_off, uint32_t *label_idx) {
    uint64_t at = 0;
    for (uint64_t r = 0; r < n; ++r) {
        label_off[r] = at;
        at += avk::sx::sx_fill_region(mask, r, n, n_words, label_idx, at, ~0ull);
    }
    label_off[n] = at;
    return 0;
}

/* ONE launch's accumulator for the block [label_lo, label_hi), as the kernel's lanes fill it: acc[(label_hi - label_lo) * AVK_LB_WORDS], set here.
 * label_off == NULL: lb_region_labels_mask on the masks; otherwise lb_region_labels on the lists. */
int label_mask_emu_block(const label_mask_emu_view *e, const uint32_t *mask, const uint64_t *label_off, const uint32_t *label_idx, uint32_t label_lo, uint32_t label_hi,
                         uint64_t *acc) {
    if (label_hi < label_lo || label_hi - label_lo > AVK_LB_MASK_BLOCK_MAX) return -1;
    avk::dp::DpVarInfo *vinfo = new avk::dp::DpVarInfo[e->n_variants + 1];
    avk::lb::LbView v;
    make_view(e, v, vinfo);
    memset(acc, 0, sizeof(uint64_t) * (size_t)(label_hi - label_lo) * AVK_LB_WORDS);
    auto add = [](uint64_t *p, uint32_t x) { *p += x; };
    for (uint64_t r = 0; r < e->n_regions; ++r) {
        if (label_off) avk::lb::lb_region_labels(v, r, label_off, label_idx, label_lo, label_hi, acc, add);
        else avk::lb::lb_region_labels_mask(v, r, mask, e->n_regions, label_lo, label_hi, acc, add);
    }
    delete[] vinfo;
    return 0;
}

} /* extern "C" */
