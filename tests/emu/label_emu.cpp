/*
 * label_emu.cpp — the per-region rule of the compact stratified tallies (aardvark_amd/csrc/avk_labels.inl) on the CPU.
 *
 * Test infrastructure like wave_emu.cpp, and a translation unit of its own: lb_region_groups / lb_region_labels are one-lane code (no cross-lane primitive),
 * so the SAME source the gfx950 kernel runs is called here region by region, on a device view the tests fill from the oracle's results
 * (tests/test_label_compact.py).  Built by tests/label_emu_lib.py with the flags of tests/emu/Makefile.
 */
#define AVK_EMU 1
#include <string.h>

#include "../../aardvark_amd/csrc/avk_labels.inl"

extern "C" {

/* the device view, array by array (names of avk::dp::DpIn and avk::lb::LbView); wide arrays, or — pk_start != NULL — the packed source */
struct label_emu_view {
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

static void make_view(const label_emu_view *e, avk::lb::LbView &v, avk::dp::DpVarInfo *vinfo) {
    memset(&v, 0, sizeof(v));
    v.in.n_regions = e->n_regions, v.in.n_variants = e->n_variants;
    v.in.t_off = e->t_off, v.in.q_off = e->q_off, v.in.t_cnt = e->t_cnt, v.in.q_cnt = e->q_cnt, v.in.var_type = e->var_type, v.in.var_zyg = e->var_zyg, v.in.var_raw = e->var_raw;
    v.in.a0_len = e->a0_len, v.in.a1_len = e->a1_len;
    v.in.pk_start = e->pk_start, v.in.pk_tc = e->pk_tc, v.in.pk_qc = e->pk_qc, v.in.pk_tz = e->pk_tz, v.in.pk_a0 = e->pk_a0, v.in.pk_a1 = e->pk_a1, v.in.pk_voff = e->pk_voff;
    for (uint64_t i = 0; i < e->n_variants; ++i) vinfo[i].alt_ed = e->alt_ed[i], vinfo[i].flags = 0, vinfo[i].a1lo = vinfo[i].a1hi = 0;
    v.vinfo = vinfo;
    v.region_out = e->region_out, v.var_out = e->var_out, v.v_off = e->v_off, v.bp_off = e->bp_off, v.bp = e->bp;
}

/* lb_region_groups for every region with status 0: blocks[r][AVK_N_GROUPS * AVK_N_FIELDS] (the others stay as they are) */
int label_emu_blocks(const label_emu_view *e, uint32_t *blocks) {
    avk::dp::DpVarInfo *vinfo = new avk::dp::DpVarInfo[e->n_variants + 1];
    avk::lb::LbView v;
    make_view(e, v, vinfo);
    for (uint64_t r = 0; r < e->n_regions; ++r) {
        if (e->region_out[4 * r] != 0) continue;
        uint32_t *block = blocks + r * AVK_LB_WORDS;
        avk::lb::lb_region_groups(v, r, [&](uint32_t g, const uint32_t(&F)[AVK_N_FIELDS]) {
            for (int f = 0; f < AVK_N_FIELDS; ++f) block[g * AVK_N_FIELDS + f] = F[f];
        });
    }
    delete[] vinfo;
    return 0;
}

/* lb_region_labels as the kernel's launches call it: labels in blocks of `block`, an accumulator per block, flushed into out[n_labels][AVK_TALLY_LEN] (ADDED) */
int label_emu_tally(const label_emu_view *e, uint32_t n_labels, const uint64_t *label_off, const uint32_t *label_idx, uint32_t block, uint64_t *out) {
    if (!block) return -1;
    avk::dp::DpVarInfo *vinfo = new avk::dp::DpVarInfo[e->n_variants + 1];
    avk::lb::LbView v;
    make_view(e, v, vinfo);
    uint64_t *acc = new uint64_t[(size_t)block * AVK_LB_WORDS];
    for (uint32_t lo = 0; lo < n_labels; lo += block) {
        const uint32_t hi = n_labels - lo > block ? lo + block : n_labels;
        memset(acc, 0, sizeof(uint64_t) * (size_t)block * AVK_LB_WORDS);
        for (uint64_t r = 0; r < e->n_regions; ++r)
            avk::lb::lb_region_labels(v, r, label_off, label_idx, lo, hi, acc, [](uint64_t *p, uint32_t x) { *p += x; });
        for (size_t k = 0; k < (size_t)(hi - lo) * AVK_LB_WORDS; ++k) out[(size_t)(lo + k / AVK_LB_WORDS) * AVK_TALLY_LEN + k % AVK_LB_WORDS] += acc[k];
    }
    delete[] acc;
    delete[] vinfo;
    return 0;
}

} /* extern "C" */
