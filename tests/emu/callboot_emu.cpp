/*
 * callboot_emu.cpp — the per-call bootstrap's lane functions (cb_stage_region, cb_ranges, cb_weight_entry, cb_stage_record, cb_lane_piece, cb_flush_word of
 * aardvark_amd/csrc/avk_callboot.inl) on the CPU, driven the way avk_callboot_tally_kernel and its host loop drive them: a launch holds R replicates of one scope,
 * workgroups take tiles of AVK_CB_TILE regions in grid-stride order, a tile's calls are walked in pieces of `cap` records, a workgroup keeps its accumulators
 * across its tiles and flushes once; the host loops over scopes and blocks of replicates.
 *
 * Test infrastructure like boot_emu.cpp and kind_emu.cpp, whose device view it shares (kind_emu_view, plus the regions' contigs and starts, which the rule's key
 * reads).  All functions are one-lane code, so the SAME source the gfx950 kernel runs is called here lane by lane (tests/test_callboot_emu.py).  The buffer behind a
 * workgroup's tile is laid out by cb_tile_at, exactly as long as AVK_CB_LDS_BYTES makes it, and is not cleared between tiles: what a tile leaves behind must not
 * be read.
 */
#define AVK_EMU 1
#include <string.h>

#include <vector>

#include "../../aardvark_amd/csrc/avk_callboot.inl"

extern "C" {

/* kind_emu_view of kind_emu.cpp, field for field */
struct callboot_emu_view {
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

int callboot_emu_tile(void) { return AVK_CB_TILE; }
int callboot_emu_recs(void) { return AVK_CB_RECS; }
int callboot_emu_threads(void) { return AVK_CB_THREADS; }
int callboot_emu_reps_max(void) { return AVK_CB_REPS_MAX; }
uint32_t callboot_emu_reps(uint32_t n_keys, uint64_t lds_bytes) { return avk::cb::cb_reps(n_keys, lds_bytes); }
uint64_t callboot_emu_lds_bytes(uint32_t n_keys, uint32_t R) { return AVK_CB_LDS_BYTES(n_keys, R); }

/* Every launch of a call: out[(1 + n_labels) * B * n_keys * 182] gains the sums.  contig / start: the regions' key parts — wide arrays, or with the view's pk_start
 * set the packed source's (start32 as pk_start, contig16 as pk_contig).  mask: word-major (sx_mask_at), may be NULL with n_labels == 0.  R: replicates of a launch
 * (1 .. AVK_CB_REPS_MAX); cap: records of a piece (1 .. AVK_CB_RECS; the kernel's is AVK_CB_RECS); grid: workgroups of a launch. */
int callboot_emu_run(const callboot_emu_view *e, const uint32_t *contig32, const uint64_t *start64, const uint16_t *contig16, const uint32_t *start32, const uint32_t *mask,
                     uint32_t n_labels, int family, const avk_size_spec *sp, uint64_t seed, uint32_t B, uint32_t R, uint32_t cap, uint32_t grid, uint64_t *out) {
    const uint32_t n_keys = avk_callboot_n_keys(family, sp);
    if (!grid || !n_keys || R < 1 || R > AVK_CB_REPS_MAX || cap < 1 || cap > AVK_CB_RECS || !avk_callboot_blocks_ok((uint64_t)n_labels + 1, B, n_keys)) return -1;
    avk_size_spec spec;
    memset(&spec, 0, sizeof(spec));
    if (family == AVK_CALLBOOT_SIZE) spec = *sp;
    std::vector<avk::dp::DpVarInfo> vinfo(e->n_variants + 1);
    avk::lb::LbView v;
    memset(&v, 0, sizeof(v));
    v.in.n_regions = e->n_regions, v.in.n_variants = e->n_variants;
    v.in.t_off = e->t_off, v.in.q_off = e->q_off, v.in.t_cnt = e->t_cnt, v.in.q_cnt = e->q_cnt, v.in.var_type = e->var_type, v.in.var_zyg = e->var_zyg, v.in.var_raw = e->var_raw;
    v.in.a0_len = e->a0_len, v.in.a1_len = e->a1_len, v.in.a0_off = e->a0_off, v.in.a1_off = e->a1_off, v.in.alleles = e->alleles, v.in.alleles_len = e->alleles_len;
    v.in.pk_tc = e->pk_tc, v.in.pk_qc = e->pk_qc, v.in.pk_tz = e->pk_tz, v.in.pk_a0 = e->pk_a0, v.in.pk_a1 = e->pk_a1, v.in.pk_voff = e->pk_voff, v.in.pk_aoff = e->pk_aoff;
    if (e->pk_start) v.in.pk_start = start32, v.in.pk_contig = contig16;
    else v.in.contig_idx = contig32, v.in.start = start64;
    for (uint64_t i = 0; i < e->n_variants; ++i) vinfo[i].alt_ed = e->alt_ed[i], vinfo[i].flags = 0, vinfo[i].a1lo = vinfo[i].a1hi = 0;
    v.vinfo = vinfo.data();
    v.region_out = e->region_out, v.var_out = e->var_out, v.v_off = e->v_off; /* (no BASEPAIR groups: the kernel reads none) */

    const uint64_t n = e->n_regions;
    const uint32_t n_tiles = (uint32_t)((n + AVK_CB_TILE - 1) / AVK_CB_TILE);
    const uint64_t seed_mix = avk_boot_mix(seed), acc_words = AVK_CB_ACC_WORDS(n_keys, R);
    auto add = [](uint64_t *p, uint64_t x) { *p += x; };
    for (uint32_t scope = 0; scope <= (mask ? n_labels : 0u); ++scope)
        for (uint32_t lo = 0; lo < B; lo += R) {
            const uint32_t hi = B - lo > R ? lo + R : B;
            for (uint32_t wg = 0; wg < grid; ++wg) {
                std::vector<uint64_t> lds((AVK_CB_LDS_BYTES(n_keys, R) + 7) / 8, 0xA5A5A5A5A5A5A5A5ull); /* the workgroup's LDS: garbage until written */
                const avk::cb::CbTile t = avk::cb::cb_tile_at((unsigned char *)lds.data(), n_keys, R);
                for (uint64_t q = 0; q < acc_words; ++q) t.acc[q] = 0;
                for (uint32_t tile = wg; tile < n_tiles; tile += grid) {
                    uint32_t any = 0;
                    for (uint32_t tid = 0; tid < AVK_CB_TILE; ++tid) any |= avk::cb::cb_stage_region(v, (uint64_t)tile * AVK_CB_TILE + tid, n, mask, scope, seed_mix, tid, t);
                    if (!any) continue;
                    const uint32_t total = avk::cb::cb_ranges(t);
                    for (uint32_t en = 0; en < AVK_CB_TILE * R; ++en) avk::cb::cb_weight_entry(t, en, R, lo, hi);
                    for (uint32_t piece = 0; piece < total; piece += cap) {
                        for (uint32_t tid = 0; tid < cap; ++tid)
                            if (piece + tid < total) avk::cb::cb_stage_record(v, t, family, spec, piece + tid, tid);
                        for (uint32_t tid = 0; tid < AVK_CB_THREADS; ++tid) {
                            const uint32_t bl = tid % R, s = tid / R;
                            if (s < AVK_CB_SLOTS) avk::cb::cb_lane_piece(t, piece, cap, R, bl, s);
                        }
                    }
                }
                for (uint64_t q = 0; q < acc_words; ++q) avk::cb::cb_flush_word(t, q, R, n_keys, scope, B, lo, hi, out, add);
            }
        }
    return 0;
}

} /* extern "C" */
