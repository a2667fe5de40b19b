/*
 * kind_emu.cpp — the call-kind tally's wave code (ck_wave_tile of aardvark_amd/csrc/avk_callkind.inl, with the lane functions under it) on the CPU, driven the way
 * avk_kind_tally_kernel and its host loop drive it: a launch holds AVK_CK_SCOPES scopes, workgroups take tiles of AVK_CK_THREADS regions in grid-stride order, the
 * four waves of a workgroup add to one block, a workgroup flushes its non-zero words once.
 *
 * Test infrastructure like size_emu.cpp.  ck_wave_tile uses cross-lane primitives, so a wave's 64 lanes run as 64 threads that meet in every primitive
 * (wave_threads.h); the SAME source the gfx950 kernel runs is what they execute (tests/test_kind_emu.py).
 */
#define AVK_EMU 1
#include <string.h>

#include <vector>

#include "wave_threads.h"

#include "../../aardvark_amd/csrc/avk_callkind.inl"

extern "C" {

/* label_emu_view of label_emu.cpp, field for field, then the allele bytes and their offsets */
struct kind_emu_view {
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
    const uint64_t *a0_off, *a1_off, *pk_aoff;
    const uint8_t *alleles;
    uint64_t alleles_len;
};

int kind_emu_threads(void) { return AVK_CK_THREADS; }
int kind_emu_scopes(void) { return AVK_CK_SCOPES; }
int kind_emu_lds_bytes(void) { return AVK_CK_LDS_BYTES; }

/* The launches of a call that hold the scopes [scope_lo, scope_hi), the first starting at scope_lo: out[(1 + n_labels) * AVK_CK_BLOCK_WORDS] gains the sums.  mask:
 * word-major (sx_mask_at), may be NULL with n_labels == 0.  grid: workgroups of a launch. */
int kind_emu_run(const kind_emu_view *e, const uint32_t *mask, uint32_t n_labels, uint32_t grid, uint32_t scope_lo, uint32_t scope_hi, uint64_t *out) {
    const uint32_t n_scopes = 1u + (mask ? n_labels : 0u);
    if (!grid || scope_lo >= scope_hi || scope_hi > n_scopes) return -1;
    std::vector<avk::dp::DpVarInfo> vinfo(e->n_variants + 1);
    avk::lb::LbView v;
    memset(&v, 0, sizeof(v));
    v.in.n_regions = e->n_regions, v.in.n_variants = e->n_variants;
    v.in.t_off = e->t_off, v.in.q_off = e->q_off, v.in.t_cnt = e->t_cnt, v.in.q_cnt = e->q_cnt, v.in.var_type = e->var_type, v.in.var_zyg = e->var_zyg, v.in.var_raw = e->var_raw;
    v.in.a0_len = e->a0_len, v.in.a1_len = e->a1_len, v.in.a0_off = e->a0_off, v.in.a1_off = e->a1_off, v.in.alleles = e->alleles, v.in.alleles_len = e->alleles_len;
    v.in.pk_start = e->pk_start, v.in.pk_tc = e->pk_tc, v.in.pk_qc = e->pk_qc, v.in.pk_tz = e->pk_tz, v.in.pk_a0 = e->pk_a0, v.in.pk_a1 = e->pk_a1, v.in.pk_voff = e->pk_voff;
    v.in.pk_aoff = e->pk_aoff;
    for (uint64_t i = 0; i < e->n_variants; ++i) vinfo[i].alt_ed = e->alt_ed[i], vinfo[i].flags = 0, vinfo[i].a1lo = vinfo[i].a1hi = 0;
    v.vinfo = vinfo.data();
    v.region_out = e->region_out, v.var_out = e->var_out, v.v_off = e->v_off; /* (no BASEPAIR groups: the kernel reads none) */

    const uint64_t n = e->n_regions;
    const uint32_t n_tiles = (uint32_t)((n + AVK_CK_THREADS - 1) / AVK_CK_THREADS);
    auto add = [](uint64_t *p, uint64_t x) { __atomic_fetch_add(p, x, __ATOMIC_RELAXED); };
    for (uint32_t lo = scope_lo; lo < scope_hi; lo += AVK_CK_SCOPES) {
        const uint32_t hi = scope_hi - lo > AVK_CK_SCOPES ? lo + AVK_CK_SCOPES : scope_hi;
        for (uint32_t wg = 0; wg < grid; ++wg) {
            std::vector<uint64_t> acc((size_t)(hi - lo) * AVK_CK_BLOCK_WORDS, 0); /* the workgroup's LDS, exactly as long as the launch makes it */
            for (uint32_t tile = wg; tile < n_tiles; tile += grid)
                for (uint32_t wave = 0; wave < AVK_CK_THREADS / 64; ++wave)
                    avk_emu::run_wave([&](int lane) {
                        avk::ck::ck_wave_tile(v, (uint64_t)tile * AVK_CK_THREADS + wave * 64u + (uint32_t)lane, n, mask, lo, hi, acc.data(), add);
                    });
            for (size_t k = 0; k < acc.size(); ++k)
                if (acc[k]) out[(size_t)lo * AVK_CK_BLOCK_WORDS + k] += acc[k];
        }
    }
    return 0;
}

} /* extern "C" */
