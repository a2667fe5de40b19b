/*
 * boot_emu.cpp — the bootstrap tally's lane functions (bt_stage_region, bt_weight_entry, bt_lane_region, bt_lane_flush of aardvark_amd/csrc/avk_boot.inl) on the
 * CPU, driven the way avk_boot_tally_kernel drives them: workgroups take tiles in grid-stride order, a workgroup's lanes keep their sums across its tiles and
 * flush once; a launch holds AVK_BT_REPS replicates of one scope, the host loops over scopes and blocks of replicates.
 *
 * Test infrastructure like label_mask_emu.cpp, whose device view it shares (plus the regions' contigs and starts, which the rule's key reads).  All four functions
 * are one-lane code, so the SAME source the gfx950 kernel runs is called here lane by lane (tests/test_boot_emu.py).
 */
#define AVK_EMU 1
#include <string.h>

#include <vector>

#include "../../aardvark_amd/csrc/avk_boot.inl"

extern "C" {

/* label_emu_view of label_emu.cpp, field for field */
struct boot_emu_view {
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

int boot_emu_tile(void) { return AVK_BT_TILE; }
int boot_emu_reps(void) { return AVK_BT_REPS; }
uint32_t boot_emu_weight(uint64_t seed, uint32_t contig_idx, uint32_t start, uint32_t b) { return avk_boot_weight(seed, contig_idx, start, b); }
uint32_t boot_emu_threshold(int k) {
    static const uint32_t T[AVK_BOOT_N_THRESHOLDS] = {AVK_BOOT_T0, AVK_BOOT_T1, AVK_BOOT_T2, AVK_BOOT_T3, AVK_BOOT_T4, AVK_BOOT_T5,
                                                      AVK_BOOT_T6, AVK_BOOT_T7, AVK_BOOT_T8, AVK_BOOT_T9, AVK_BOOT_T10, AVK_BOOT_T11};
    return k >= 0 && k < AVK_BOOT_N_THRESHOLDS ? T[k] : 0u;
}

/* Every launch of a call: out[(1 + n_labels) * B * AVK_TALLY_LEN] gains the sums.  contig / start: the regions' key parts — wide arrays, or with pk16 != 0 the
 * packed source's (start32 as pk_start, contig16 as pk_contig).  mask: word-major (sx_mask_at), may be NULL with n_labels == 0.  grid: workgroups of a launch. */
int boot_emu_run(const boot_emu_view *e, const uint32_t *contig32, const uint64_t *start64, const uint16_t *contig16, const uint32_t *start32, const uint32_t *mask,
                 uint32_t n_labels, uint64_t seed, uint32_t B, uint32_t grid, uint64_t *out) {
    if (!grid) return -1;
    std::vector<avk::dp::DpVarInfo> vinfo(e->n_variants + 1);
    avk::lb::LbView v;
    memset(&v, 0, sizeof(v));
    v.in.n_regions = e->n_regions, v.in.n_variants = e->n_variants;
    v.in.t_off = e->t_off, v.in.q_off = e->q_off, v.in.t_cnt = e->t_cnt, v.in.q_cnt = e->q_cnt, v.in.var_type = e->var_type, v.in.var_zyg = e->var_zyg, v.in.var_raw = e->var_raw;
    v.in.a0_len = e->a0_len, v.in.a1_len = e->a1_len;
    v.in.pk_tc = e->pk_tc, v.in.pk_qc = e->pk_qc, v.in.pk_tz = e->pk_tz, v.in.pk_a0 = e->pk_a0, v.in.pk_a1 = e->pk_a1, v.in.pk_voff = e->pk_voff;
    if (e->pk_start) v.in.pk_start = start32, v.in.pk_contig = contig16;
    else v.in.contig_idx = contig32, v.in.start = start64;
    for (uint64_t i = 0; i < e->n_variants; ++i) vinfo[i].alt_ed = e->alt_ed[i], vinfo[i].flags = 0, vinfo[i].a1lo = vinfo[i].a1hi = 0;
    v.vinfo = vinfo.data();
    v.region_out = e->region_out, v.var_out = e->var_out, v.v_off = e->v_off, v.bp_off = e->bp_off, v.bp = e->bp;

    const uint64_t n = e->n_regions;
    const uint32_t n_tiles = (uint32_t)((n + AVK_BT_TILE - 1) / AVK_BT_TILE);
    const uint64_t seed_mix = avk_boot_mix(seed);
    std::vector<uint32_t> blk((size_t)AVK_BT_TILE_SLOTS * AVK_BT_SLOT), gm(AVK_BT_TILE);
    std::vector<uint64_t> h(AVK_BT_TILE);
    std::vector<uint8_t> w((size_t)AVK_BT_TILE * AVK_BT_REPS);
    avk::bt::BtTile t;
    t.blk = blk.data(), t.h = h.data(), t.gm = gm.data(), t.w = w.data();
    auto add = [](uint64_t *p, uint64_t x) { *p += x; };
    for (uint32_t scope = 0; scope <= n_labels; ++scope)
        for (uint32_t lo = 0; lo < B; lo += AVK_BT_REPS) {
            const uint32_t hi = B - lo > AVK_BT_REPS ? lo + AVK_BT_REPS : B;
            for (uint32_t wg = 0; wg < grid; ++wg) {
                std::vector<uint64_t> acc((size_t)AVK_BT_THREADS * AVK_N_GROUPS, 0); /* the lanes' registers */
                for (uint32_t tile = wg; tile < n_tiles; tile += grid) {
                    /* (LDS is not cleared between tiles on the device either: what a tile leaves behind must not be read) */
                    uint32_t any = 0;
                    for (uint32_t tid = 0; tid < AVK_BT_TILE; ++tid) any |= avk::bt::bt_stage_region(v, (uint64_t)tile * AVK_BT_TILE + tid, n, mask, scope, seed_mix, tid, t);
                    if (!any) continue;
                    for (uint32_t en = 0; en < AVK_BT_TILE * AVK_BT_REPS; ++en) avk::bt::bt_weight_entry(t, en, lo, hi);
                    for (uint32_t tid = 0; tid < AVK_BT_THREADS; ++tid) {
                        const uint32_t bl = tid / AVK_BT_SLOT, f = tid % AVK_BT_SLOT;
                        if (bl >= AVK_BT_REPS) continue;
                        uint64_t(&a)[AVK_N_GROUPS] = *(uint64_t(*)[AVK_N_GROUPS])(acc.data() + (size_t)tid * AVK_N_GROUPS);
                        for (uint32_t rt = 0; rt < AVK_BT_TILE; ++rt)
                            if (t.gm[rt]) avk::bt::bt_lane_region(t, rt, t.gm[rt], bl, f, a);
                    }
                }
                for (uint32_t tid = 0; tid < AVK_BT_THREADS; ++tid) {
                    const uint32_t bl = tid / AVK_BT_SLOT, f = tid % AVK_BT_SLOT;
                    if (bl >= AVK_BT_REPS || lo + bl >= hi) continue;
                    const uint64_t(&a)[AVK_N_GROUPS] = *(const uint64_t(*)[AVK_N_GROUPS])(acc.data() + (size_t)tid * AVK_N_GROUPS);
                    avk::bt::bt_lane_flush(a, scope, B, lo + bl, f, out, add);
                }
            }
        }
    return 0;
}

} /* extern "C" */
