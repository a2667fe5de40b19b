/* The arithmetic of a solver step (avk_step.inl): how many workgroups each launch gets, how the per-wave HBM slices of the context's workspace are shared out among
 * the launches that run side by side, and the LDS and grid of a lane launch.
 *
 * The workspace is one array of slices of ws_bytes, a slice per wave, four waves per workgroup.  Four launches of a step may hold slices at the same time, so each has
 * a share of its own, handed out here and nowhere else (two launches once met on a slice: profiles/r04_gpu_fuzz_classc.txt):
 *
 *   [ main: hbm_blocks | solo: hbm_solo_max (the side launch takes its workgroups from the END of this share) | early hand-backs: hbm_early_max ]
 *
 * Plain C++, no HIP types: tests/native/step_geometry_check.cpp compiles this header for the CPU. */
#ifndef AVK_STEP_GEOMETRY_H
#define AVK_STEP_GEOMETRY_H

#include <cstddef>
#include <cstdint>

/* workgroups (x 4 waves x ws_bytes_per_wave of HBM) of the main HBM-tier launch of a batch that has lane launches.  Every wave of the grid needs a slice, and fresh device
 * memory is scrubbed when it is handed out (75 ms per GB): n_cus x 3 workgroups were 3 of the 4.8 GB a process's first whole-genome call waited 0.39 s for
 * (profiles/r05_first_solve.txt); the step does not notice the difference (profiles/r05_quad_sweeps.txt) */
#define AVK_HBM_BLOCKS_BESIDE_LANES 192u
enum { AVK_WAVES_PER_BLOCK = 4 };

/* a tile width (1 .. 64 records a wave takes at a time) as a power of two */
static inline uint32_t avk_width_log2(int64_t w) { return w <= 1 ? 0u : (w <= 2 ? 1u : (w <= 4 ? 2u : (w <= 8 ? 3u : (w <= 16 ? 4u : (w <= 32 ? 5u : 6u))))); }

struct AvkStepGeometryIn {
    int n_cus;
    int64_t waves_per_cu;
    uint64_t n;      /* regions of the batch */
    uint32_t n_fast; /* of them, the lane launches' */
    bool lanes;      /* the step has lane launches */
    int64_t ws_bytes, ws_budget_bytes;
    int64_t hbm_solo_blocks, hbm_early_blocks; /* options: 0 or less selects 128 / 64 */
    int64_t big_waves, big_bytes;
};

struct AvkStepGeometry {
    uint32_t blocks;        /* workgroups that cover the records of the wave-per-region launches */
    uint32_t hbm_blocks;    /* the main HBM launch: no more workgroups than can be resident (three per CU at the kernel's register count) — later ones would find the
                             * work list empty anyway, and every wave of the grid needs a slice of HBM (fresh device memory is scrubbed when it is handed out: 13 GB of
                             * workspaces cost 0.25 s at the first call of a process, 4 GB a third of that) */
    uint32_t hbm_solo_max;  /* the HBM solo launch runs beside the main stream's HBM launch: its workgroups have slices of their own, after the others */
    uint32_t hbm_early_max; /* workgroups of the launch behind the three-call lane class (its hand-backs), slices of their own too */
    bool shrunk;            /* the shares were cut to fit ws_budget_bytes */
    bool floored;           /* a share was kept at eight workgroups (or all it had) where the budget asked for fewer: ws_need may exceed the budget */
    uint32_t n_waves;       /* waves of the main launch */
    int64_t ws_bytes;
    size_t ws_need;
    uint32_t big_blocks;
    size_t big_need;

    /* the shares of the workspace, as the first wave of each */
    uint32_t main_wave() const { return 0u; }
    uint32_t solo_wave() const { return n_waves; }
    uint32_t side_wave(uint32_t xb) const { return n_waves + (hbm_solo_max - xb) * AVK_WAVES_PER_BLOCK; } /* the last xb workgroups of the solo share (avk_side_split) */
    uint32_t early_wave() const { return n_waves + hbm_solo_max * AVK_WAVES_PER_BLOCK; }
    uint32_t end_wave() const { return n_waves + (hbm_solo_max + hbm_early_max) * AVK_WAVES_PER_BLOCK; }
    /* ... and as a pointer into the workspace */
    uint8_t *share(uint8_t *d_ws, uint32_t wave) const { return d_ws + (size_t)wave * (size_t)ws_bytes; }
};

static inline AvkStepGeometry avk_step_geometry(const AvkStepGeometryIn &in) {
    AvkStepGeometry g;
    uint64_t want_waves = (uint64_t)in.n_cus * (uint64_t)in.waves_per_cu;
    if (want_waves > in.n - in.n_fast) want_waves = in.n - in.n_fast;
    g.blocks = (uint32_t)((want_waves + AVK_WAVES_PER_BLOCK - 1) / AVK_WAVES_PER_BLOCK);
    if (g.blocks == 0) g.blocks = 1;
    g.hbm_blocks = (uint32_t)in.n_cus * 3u;
    /* lane launches that leave the other kernels a few thousand regions leave this tier a few dozen (a genome: 27) */
    if (in.lanes && in.n - in.n_fast <= 16384 && g.hbm_blocks > AVK_HBM_BLOCKS_BESIDE_LANES) g.hbm_blocks = AVK_HBM_BLOCKS_BESIDE_LANES;
    if (g.hbm_blocks > g.blocks) g.hbm_blocks = g.blocks;
    g.hbm_solo_max = (uint32_t)(in.hbm_solo_blocks > 0 ? in.hbm_solo_blocks : 128);
    g.hbm_early_max = (uint32_t)(in.hbm_early_blocks > 0 ? in.hbm_early_blocks : 64);
    /* large slices mean fewer waves per launch (option ws_budget_bytes) */
    g.shrunk = g.floored = false;
    g.ws_bytes = in.ws_bytes;
    const double total = (double)(g.hbm_blocks + g.hbm_solo_max + g.hbm_early_max) * AVK_WAVES_PER_BLOCK * (double)in.ws_bytes;
    if (total > (double)in.ws_budget_bytes) {
        const double f = (double)in.ws_budget_bytes / total;
        g.shrunk = true;
        uint32_t *shares[3] = {&g.hbm_blocks, &g.hbm_solo_max, &g.hbm_early_max};
        for (uint32_t *b : shares) {
            const uint32_t x = (uint32_t)(*b * f);
            if (x < 8) g.floored = true;
            *b = x < 8 ? (*b < 8 ? *b : 8u) : x;
        }
    }
    g.n_waves = g.hbm_blocks * AVK_WAVES_PER_BLOCK;
    g.ws_need = (size_t)g.end_wave() * (size_t)in.ws_bytes;
    g.big_blocks = (uint32_t)((in.big_waves + AVK_WAVES_PER_BLOCK - 1) / AVK_WAVES_PER_BLOCK);
    g.big_need = (size_t)g.big_blocks * AVK_WAVES_PER_BLOCK * (size_t)in.big_bytes;
    return g;
}

/* workgroups of the HBM solo launch for n_c records of class C: a wave per record, as far as its share goes */
static inline uint32_t avk_solo_blocks(uint32_t n_c, uint32_t hbm_solo_max) {
    const uint32_t b = (n_c + 3) / 4;
    return b < hbm_solo_max ? b : hbm_solo_max;
}

/* The side launch (the class C records that are not the wide kernel's, or a team launch for the head of the class) takes `want` workgroups from the END of the solo
 * launch's share, which keeps at least half of it — a batch with large per-wave slices (adaptive_ws under its budget) may have a share of eight workgroups, and the two
 * launches must never meet on a slice (they did: a side launch of hbm_solo_max workgroups left the solo launch one workgroup ON the other's first slices — wrong results
 * in a fuzz case where every region was planned as class C, profiles/r04_gpu_fuzz_classc.txt).  Returns the side launch's workgroups and trims *hbm_solo to the rest. */
static inline uint32_t avk_side_split(uint32_t want, uint32_t hbm_solo_max, uint32_t *hbm_solo) {
    const uint32_t xb = want > hbm_solo_max / 2u ? hbm_solo_max / 2u : want;
    if (*hbm_solo > hbm_solo_max - xb) *hbm_solo = hbm_solo_max - xb;
    return xb;
}

/* ---- a lane launch: one-wave workgroups, the per-lane arrays of `1 << lanes_log2` lanes plus a tally of its own in LDS ---- */
struct AvkLaneShape {
    uint32_t W, nm, ed_max, qcap, pool, lanes_log2, n_tiles;
    bool quad; /* four lanes per region (avk_quad.inl) */
};
struct AvkLaneCaps {
    int n_cus;
    int64_t waves_per_cu; /* option lane_waves_per_cu (0 or less: 12) */
    int64_t waves_three;  /* lane_waves_three: the three-call class, when positive */
};
/* LDS bytes of the workgroup (0: does not fit) and the grid that fills the machine: as many workgroups per CU as the LDS and the wave slots hold */
static inline size_t avk_lane_geometry(const AvkLaneShape &la, const AvkLaneCaps &c, uint32_t *grid) {
    const uint32_t rows = (1 + 2 * (la.nm - 1)) * (la.W + 1) + ((la.quad ? 4 : 3) + 2 * la.pool) * ((2 * la.ed_max + 2 + 3) / 4) + la.qcap + (la.nm == 2 ? 4 : 8); /* lane_rows / quad_rows */
    const size_t lds = (size_t)rows * (4u << la.lanes_log2) + 288 * 4;
    uint32_t per_cu = (uint32_t)((160 * 1024) / lds);
    if (per_cu < 1) return 0;
    uint32_t cap = la.lanes_log2 < 4 ? 32u : (uint32_t)(c.waves_per_cu > 0 ? c.waves_per_cu : 12); /* very narrow tiles: every wave slot */
    if (la.nm > 4 && c.waves_three > 0) cap = (uint32_t)c.waves_three; /* the three-call class: 17 KB per wave */
    if (per_cu > cap) per_cu = cap;
    const uint32_t claims = la.n_tiles * (64u >> la.lanes_log2);
    uint32_t g = (uint32_t)c.n_cus * per_cu;
    if (g > claims) g = claims;
    *grid = g;
    return lds;
}

#endif
