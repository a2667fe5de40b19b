// The step's arithmetic (csrc/avk_step_geometry.h) swept over a grid, for tests/test_step_geometry.py.  Every point is checked here (a failed check prints a line
// that starts with FAIL and the program exits 1); printed for pytest:
//   points <n> floored <n>
//   floor cus <c> rest <n - n_fast> lanes <0|1> ws <bytes> budget <bytes> solo_opt <o> : main <b> solo <b> early <b> need <bytes> over <0|1>     a point where the floor of eight holds (over: past the budget)
//   pin <name> : main <b> solo <b> early <b>                                                                                          points the tests name
//   lane class <k> width <w> quad <0|1> pool <p> : lds <bytes> grid <g>
//   log2 <w> <l>
#include <cinttypes>
#include <cstdio>
#include <initializer_list>

#include "../../aardvark_amd/csrc/avk_dev_types.h"
#include "../../aardvark_amd/csrc/avk_step_geometry.h"

static int g_fail = 0;
#define CHECK(cond, ...)              \
    do {                              \
        if (!(cond)) {                \
            printf("FAIL " #cond ": "); \
            printf(__VA_ARGS__);      \
            printf("\n");             \
            g_fail = 1;               \
        }                             \
    } while (0)

struct Span {
    uint64_t lo, hi; /* waves [lo, hi) */
};
static bool disjoint(Span a, Span b) { return a.hi <= b.lo || b.hi <= a.lo || a.lo == a.hi || b.lo == b.hi; }

static AvkStepGeometryIn point(int cus, uint64_t rest, bool lanes, int64_t ws, int64_t budget, int64_t solo_opt) {
    const uint32_t n_fast = lanes ? 100000u : 0u;
    return AvkStepGeometryIn{cus, 16, rest + n_fast, n_fast, lanes, ws, budget, solo_opt, 64, 8, 8ll << 20};
}

int main() {
    const int cus[] = {8, 256};
    const uint64_t rest[] = {1, 3, 4, 5, 16384, 16385, 1000000};
    const int64_t ws[] = {256ll << 10, 1ll << 20, 4ll << 20, 4000000ll, 64ll << 20};
    const int64_t budget[] = {1ll << 30, 4ll << 30, 96ll << 30};
    const int64_t solo_opt[] = {64, 0}; /* the context's value; 0: the 128 the step takes without one */
    long points = 0, floored = 0;
    static uint8_t base[1];
    for (int c : cus)
        for (uint64_t r : rest)
            for (int lanes = 0; lanes < 2; ++lanes)
                for (int64_t w : ws)
                    for (int64_t b : budget)
                        for (int64_t so : solo_opt) {
                            const AvkStepGeometryIn in = point(c, r, lanes != 0, w, b, so);
                            const AvkStepGeometry g = avk_step_geometry(in);
                            const char *at = "cus %d rest %" PRIu64 " lanes %d ws %" PRId64 " budget %" PRId64 " solo_opt %" PRId64;
#define AT c, r, lanes, w, b, so
                            CHECK(g.blocks >= 1 && g.hbm_blocks >= 1 && g.hbm_blocks <= g.blocks && g.hbm_solo_max >= 1 && g.hbm_early_max >= 1, at, AT);
                            CHECK(g.n_waves == g.hbm_blocks * 4u, at, AT);
                            CHECK(g.ws_need == (size_t)g.end_wave() * (size_t)w, at, AT);
                            CHECK(g.share(base, g.main_wave()) == base, at, AT);
                            /* total slice bytes stay within the budget, except through the floor of eight workgroups per share */
                            CHECK(g.floored || (double)g.ws_need <= (double)b, at, AT);
                            if (g.floored) {
                                floored += 1;
                                CHECK(g.hbm_blocks <= 8 || g.hbm_solo_max <= 8 || g.hbm_early_max <= 8, at, AT);
                                printf("floor cus %d rest %" PRIu64 " lanes %d ws %" PRId64 " budget %" PRId64 " solo_opt %" PRId64 " : main %u solo %u early %u need %zu over %d\n", AT, g.hbm_blocks,
                                       g.hbm_solo_max, g.hbm_early_max, g.ws_need, (double)g.ws_need > (double)b ? 1 : 0);
                            }
                            const uint32_t share = g.hbm_solo_max;
                            const uint32_t n_cs[] = {1, 7, 4 * share};
                            const uint32_t n_nws[] = {0, 1, share / 2, share, 2 * share};
                            for (uint32_t n_c : n_cs)
                                for (uint32_t nw : n_nws)
                                    for (int team = 0; team < 2; ++team) {
                                        /* as the step asks: the companion of the wide launch (a workgroup per record that is not the wide kernel's, at most 64 and no
                                         * more than the solo launch has), or a team launch (up to half of the class, here: as many as nw) */
                                        uint32_t hbm_solo = avk_solo_blocks(n_c, share);
                                        const uint32_t before = hbm_solo;
                                        uint32_t want = team ? (n_c / 2u < nw ? n_c / 2u : nw) : (nw < n_c ? nw : n_c);
                                        if (!team) want = want < hbm_solo ? want : hbm_solo, want = want < 64u ? want : 64u;
                                        const uint32_t xb = avk_side_split(want, share, &hbm_solo);
                                        points += 1;
                                        CHECK(before >= 1 && before <= share, at, AT);
                                        CHECK(xb <= share / 2u && xb <= want, at, AT);
                                        CHECK(hbm_solo >= 1 && hbm_solo <= before, at, AT); /* the solo launch keeps a workgroup of its own */
                                        const Span main_s = {g.main_wave(), (uint64_t)g.main_wave() + g.hbm_blocks * 4u};
                                        const Span solo_s = {g.solo_wave(), (uint64_t)g.solo_wave() + hbm_solo * 4u};
                                        const Span side_s = {g.side_wave(xb), (uint64_t)g.side_wave(xb) + xb * 4u};
                                        const uint32_t eb = g.hbm_blocks < g.hbm_early_max ? g.hbm_blocks : g.hbm_early_max;
                                        const Span early_s = {g.early_wave(), (uint64_t)g.early_wave() + eb * 4u};
                                        const Span all[4] = {main_s, solo_s, side_s, early_s};
                                        for (int i = 0; i < 4; ++i) {
                                            CHECK(all[i].lo <= all[i].hi && all[i].hi * (uint64_t)w <= g.ws_need, at, AT);
                                            for (int j = i + 1; j < 4; ++j) CHECK(disjoint(all[i], all[j]), at, AT);
                                        }
                                        CHECK(side_s.hi == early_s.lo, at, AT); /* the side launch's are the LAST slices of the solo share */
                                    }
#undef AT
                        }
    printf("points %ld floored %ld\n", points, floored);
    {
        /* tests/test_gpu_wide.py::test_small_slice_shares_do_not_overlap: 256 CUs, slices of 4 MB, 1 GiB */
        AvkStepGeometry g = avk_step_geometry(point(256, 1000000, false, 4000000, 1ll << 30, 0)); /* 960 workgroups x 4 waves x 4,000,000 bytes */
        printf("pin decimal_4mb_128 : main %u solo %u early %u\n", g.hbm_blocks, g.hbm_solo_max, g.hbm_early_max);
        g = avk_step_geometry(point(256, 1000000, false, 4ll << 20, 1ll << 30, 64)); /* the options as the test sets them, the context's 64 + 64 workgroups */
        printf("pin binary_4mb_64 : main %u solo %u early %u\n", g.hbm_blocks, g.hbm_solo_max, g.hbm_early_max);
        g = avk_step_geometry(point(256, 16384, true, 4ll << 20, 1ll << 30, 64)); /* ... beside lane launches: 192 + 64 + 64 */
        printf("pin binary_4mb_64_lanes : main %u solo %u early %u\n", g.hbm_blocks, g.hbm_solo_max, g.hbm_early_max);
    }
    const AvkLaneCaps caps = {256, 12, 0};
    for (int k = 0; k < AVK_FAST_CLASSES; ++k)
        for (uint32_t l2 : {6u, 4u}) {
            const AvkFastClass &cl = AVK_FAST_CLASS[k];
            const bool quad = l2 <= 4;
            const uint32_t pool = cl.maxv > 2 ? 6u : 0u;
            const AvkLaneShape s = {cl.W, 1u << cl.maxv, cl.ed_max, cl.qcap, pool, l2, 100000u, quad};
            uint32_t grid = 0;
            const size_t lds = avk_lane_geometry(s, caps, &grid);
            printf("lane class %d width %u quad %d pool %u : lds %zu grid %u\n", k, 1u << l2, quad ? 1 : 0, pool, lds, grid);
        }
    {
        const AvkLaneShape s = {12, 8, 6, 32, 6, 6, 100000u, false}; /* the three-call class: its own cap, then a grid no larger than its claims, then an LDS that does not fit */
        uint32_t grid = 0;
        const AvkLaneCaps three = {256, 12, 1};
        avk_lane_geometry(s, three, &grid);
        printf("lane three_cap grid %u\n", grid);
        AvkLaneShape few = s;
        few.n_tiles = 5, few.lanes_log2 = 4;
        avk_lane_geometry(few, caps, &grid);
        printf("lane few_tiles grid %u\n", grid);
        AvkLaneShape big = s;
        big.pool = 60;
        printf("lane too_big lds %zu\n", avk_lane_geometry(big, caps, &grid));
    }
    const int widths[] = {-1, 0, 1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65};
    for (int w : widths) printf("log2 %d %u\n", w, avk_width_log2(w));
    printf(g_fail ? "step_geometry_check: FAILED\n" : "step_geometry_check: ok\n");
    return g_fail;
}
