/*
 * score_emu.cpp — the score curve's wave code (sc_wave_tile and sc_wave_curve of aardvark_amd/csrc/avk_score.inl, with the lane functions under them) on the CPU,
 * driven the way the two kernels and their host loop drive it: a launch of the histogram kernel holds a block of scopes sized from AVK_SC_LDS_BYTES, workgroups
 * take tiles of AVK_SC_THREADS regions in grid-stride order, the four waves of a workgroup add to one block, a workgroup flushes its non-zero words once; then one
 * wave per (scope, group) row turns the histogram bins into curve points.
 *
 * Test infrastructure like size_emu.cpp, whose device view it shares.  A wave's 64 lanes run as 64 threads that meet in every primitive (wave_threads.h); the
 * SAME source the gfx950 kernels run is what they execute (tests/test_score_emu.py).
 */
#define AVK_EMU 1
#include <string.h>

#include <vector>

#include "wave_threads.h"

#include "../../aardvark_amd/csrc/avk_score.inl"

extern "C" {

/* label_emu_view of label_emu.cpp, field for field */
struct score_emu_view {
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

int score_emu_threads(void) { return AVK_SC_THREADS; }
int score_emu_lds_bytes(void) { return AVK_SC_LDS_BYTES; }
int score_emu_spec_ok(const avk_score_spec *s) { return avk_score_spec_ok(s); }
uint32_t score_emu_bin(const avk_score_spec *s, float score) { return avk_score_bin_of(s, score); }

/* Every launch of a call: out[(1 + n_labels) * n_points * AVK_N_GROUPS * AVK_SCORE_FIELDS] gains the curve.  mask: word-major (sx_mask_at), may be NULL with
 * n_labels == 0.  grid: workgroups of a histogram launch. */
int score_emu_run(const score_emu_view *e, const uint32_t *mask, uint32_t n_labels, const avk_score_spec *spec, const float *scores, uint32_t grid, uint64_t *out) {
    if (!grid || !avk_score_spec_ok(spec)) return -1;
    std::vector<avk::dp::DpVarInfo> vinfo(e->n_variants + 1);
    avk::lb::LbView v;
    memset(&v, 0, sizeof(v));
    v.in.n_regions = e->n_regions, v.in.n_variants = e->n_variants;
    v.in.t_off = e->t_off, v.in.q_off = e->q_off, v.in.t_cnt = e->t_cnt, v.in.q_cnt = e->q_cnt, v.in.var_type = e->var_type, v.in.var_zyg = e->var_zyg, v.in.var_raw = e->var_raw;
    v.in.a0_len = e->a0_len, v.in.a1_len = e->a1_len;
    v.in.pk_start = e->pk_start, v.in.pk_tc = e->pk_tc, v.in.pk_qc = e->pk_qc, v.in.pk_tz = e->pk_tz, v.in.pk_a0 = e->pk_a0, v.in.pk_a1 = e->pk_a1, v.in.pk_voff = e->pk_voff;
    for (uint64_t i = 0; i < e->n_variants; ++i) vinfo[i].alt_ed = e->alt_ed[i], vinfo[i].flags = 0, vinfo[i].a1lo = vinfo[i].a1hi = 0;
    v.vinfo = vinfo.data();
    v.region_out = e->region_out, v.var_out = e->var_out, v.v_off = e->v_off; /* (no BASEPAIR groups: the kernels read none) */

    const uint64_t n = e->n_regions;
    const uint32_t n_tiles = (uint32_t)((n + AVK_SC_THREADS - 1) / AVK_SC_THREADS);
    const uint32_t n_points = spec->n_thresholds + 1u, block_words = AVK_SC_BLOCK_WORDS(n_points), n_scopes = 1u + (mask ? n_labels : 0u);
    uint32_t per_launch = AVK_SC_LDS_BYTES / (block_words * 8u);
    if (per_launch > AVK_SC_SCOPES_MAX) per_launch = AVK_SC_SCOPES_MAX;
    if (!per_launch) return -1;
    std::vector<uint64_t> hist((size_t)n_scopes * block_words, 0); /* the cleared pool block */
    auto add = [](uint64_t *p, uint64_t x) { __atomic_fetch_add(p, x, __ATOMIC_RELAXED); };
    for (uint32_t lo = 0; lo < n_scopes; lo += per_launch) {
        const uint32_t hi = n_scopes - lo > per_launch ? lo + per_launch : n_scopes;
        for (uint32_t wg = 0; wg < grid; ++wg) {
            std::vector<uint64_t> acc((size_t)(hi - lo) * block_words, 0); /* the workgroup's LDS, exactly as long as the launch makes it */
            for (uint32_t tile = wg; tile < n_tiles; tile += grid)
                for (uint32_t wave = 0; wave < AVK_SC_THREADS / 64; ++wave)
                    avk_emu::run_wave([&](int lane) {
                        avk::sc::sc_wave_tile(v, (uint64_t)tile * AVK_SC_THREADS + wave * 64u + (uint32_t)lane, n, mask, *spec, scores, lo, hi, acc.data(), add);
                    });
            for (size_t k = 0; k < acc.size(); ++k)
                if (acc[k]) hist[(size_t)lo * block_words + k] += acc[k];
        }
    }
    for (uint32_t row = 0; row < n_scopes * AVK_N_GROUPS; ++row) { /* avk_score_curve_kernel: a wave a row */
        const uint32_t scope = row / AVK_N_GROUPS, g = row % AVK_N_GROUPS;
        avk_emu::run_wave([&](int) { avk::sc::sc_wave_curve(hist.data() + (size_t)scope * block_words, n_points, g, out + (size_t)scope * AVK_SC_H_WORDS(n_points)); });
    }
    return 0;
}

} /* extern "C" */
