/*
 * pack_chunks_check.cpp — the chunk plan of avk_pack_chunks.h on the CPU, a program of its own (tests/test_pack_chunks_plan.py builds it with
 * -fsanitize=address,undefined and runs it).
 *
 * Over a sweep of n_regions, n_variants and K:
 *   - the groups' segments tile every per-region and every per-call array exactly once, in order, inside the array;
 *   - region ranges are whole 256-region blocks (the last block of the batch may be short);
 *   - a plan with k > 0 keeps the floor in every segment of every array, a plan that could not has k = 0;
 *   - with the running sums of random counts: every block is run by exactly one launch 0 .. K, a group launch only ever takes a block whose region range and
 *     whose calls have arrived with that group or before, and is the FIRST such launch; only counts that overrun n_variants reach the catch-all.
 */
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../aardvark_amd/csrc/avk_pack_chunks.h"

using namespace avk::pc;

static int failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (failures < 20) {                          \
                fprintf(stderr, "FAIL %s: ", #cond);      \
                fprintf(stderr, __VA_ARGS__);             \
                fprintf(stderr, "\n");                    \
            }                                             \
            ++failures;                                   \
        }                                                 \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
    return rng_state;
}

/* entry widths of the arrays a group copies: start 4, len 2, contig_idx 2 per region; var_rel_pos 2, var_type_zyg 1, var_raw_space 4 per call */
static const uint64_t REGION_WIDTHS[] = {4, 2, 2}, CALL_WIDTHS[] = {2, 1, 4};

static void check_tiling(uint64_t n, uint64_t nv, int64_t want, uint64_t floor_bytes) {
    const ChunkPlan p = plan_chunks(n, nv, want, floor_bytes);
    if (!p.k) {
        /* refused: an empty batch, K out of range, or some segment under the floor */
        if (want >= 2 && want <= PC_MAX_GROUPS && n && nv) {
            const ChunkPlan q = plan_chunks(n, nv, want, 0);
            CHECK(q.k == (uint32_t)want, "n %llu nv %llu K %lld: no plan without a floor", (unsigned long long)n, (unsigned long long)nv, (long long)want);
            bool under = false;
            for (uint32_t j = 0; j < q.k; ++j) under = under || pc_region_range(q, j).count * 2 < floor_bytes || pc_call_range(q, j).count < floor_bytes;
            CHECK(under, "n %llu nv %llu K %lld floor %llu: refused although every segment keeps the floor", (unsigned long long)n, (unsigned long long)nv, (long long)want,
                  (unsigned long long)floor_bytes);
        }
        return;
    }
    CHECK(p.k == (uint32_t)want, "k %u want %lld", p.k, (long long)want);
    CHECK(p.block_cut[0] == 0 && p.block_cut[p.k] == pc_blocks(n), "blocks 0 .. %u, plan %u .. %u", pc_blocks(n), p.block_cut[0], p.block_cut[p.k]);
    CHECK(p.call_cut[0] == 0 && p.call_cut[p.k] == nv, "calls");
    /* real arrays of the real sizes, one byte a touched entry: the sanitizer sees every index */
    std::vector<uint8_t> seen_r(n, 0), seen_v(nv, 0);
    uint64_t next_r = 0, next_v = 0;
    for (uint32_t j = 0; j < p.k; ++j) {
        const Range rr = pc_region_range(p, j), cr = pc_call_range(p, j);
        CHECK(rr.first == next_r && cr.first == next_v, "group %u starts at region %llu (expected %llu), call %llu (expected %llu)", j, (unsigned long long)rr.first,
              (unsigned long long)next_r, (unsigned long long)cr.first, (unsigned long long)next_v);
        CHECK(rr.first + rr.count <= n && cr.first + cr.count <= nv, "group %u out of bounds", j);
        CHECK(rr.first % PC_BLOCK == 0 && (rr.count % PC_BLOCK == 0 || rr.first + rr.count == n), "group %u is not whole blocks", j);
        for (uint64_t w : REGION_WIDTHS) CHECK(rr.count * w >= floor_bytes, "group %u: %llu bytes of a per-region array under the floor %llu", j, (unsigned long long)(rr.count * w), (unsigned long long)floor_bytes);
        for (uint64_t w : CALL_WIDTHS) CHECK(cr.count * w >= floor_bytes, "group %u: %llu bytes of a per-call array under the floor %llu", j, (unsigned long long)(cr.count * w), (unsigned long long)floor_bytes);
        for (uint64_t r = rr.first; r < rr.first + rr.count && r < n; ++r) seen_r[r] += 1;
        for (uint64_t v = cr.first; v < cr.first + cr.count && v < nv; ++v) seen_v[v] += 1;
        next_r = rr.first + rr.count, next_v = cr.first + cr.count;
    }
    CHECK(next_r == n && next_v == nv, "the groups end at region %llu of %llu, call %llu of %llu", (unsigned long long)next_r, (unsigned long long)n, (unsigned long long)next_v, (unsigned long long)nv);
    for (uint64_t r = 0; r < n; ++r) CHECK(seen_r[r] == 1, "region %llu copied %u times", (unsigned long long)r, seen_r[r]);
    for (uint64_t v = 0; v < nv; ++v) CHECK(seen_v[v] == 1, "call %llu copied %u times", (unsigned long long)v, seen_v[v]);
}

/* shape: 0 uniform counts, 1 every call in the last region, 2 none in the first half, 3 all in the first tenth, 4 counts that overrun nv */
static void check_ownership(uint64_t n, uint64_t nv, int64_t want, int shape) {
    const ChunkPlan p = plan_chunks(n, nv, want, 0);
    if (!p.k) return;
    std::vector<uint64_t> cnt(n, 0);
    uint64_t left = nv;
    if (shape == 1) cnt[n - 1] = left, left = 0;
    const uint64_t lo = shape == 2 ? n / 2 : 0, hi = shape == 3 ? (n / 10 ? n / 10 : 1) : n;
    while (left) {
        const uint64_t r = lo + rnd() % (hi - lo), c = 1 + rnd() % 3;
        const uint64_t take = c < left ? c : left;
        cnt[r] += take, left -= take;
    }
    if (shape == 4) cnt[rnd() % n] += 1 + rnd() % 1000;
    std::vector<uint64_t> voff(n + 1, 0);
    for (uint64_t r = 0; r < n; ++r) voff[r + 1] = voff[r] + cnt[r];
    const uint32_t nb = pc_blocks(n);
    for (uint32_t b = 0; b < nb; ++b) {
        const uint64_t r_end = ((uint64_t)b + 1) * PC_BLOCK < n ? ((uint64_t)b + 1) * PC_BLOCK : n;
        const uint64_t calls_end = voff[r_end];
        uint32_t ran = 0, first_possible = p.k;
        for (uint32_t j = 0; j <= p.k; ++j) {
            const bool in_grid = j == p.k || b < p.block_cut[j + 1]; /* launch j covers the blocks of ranges 0 .. j */
            const bool arrived = j < p.k && b < p.block_cut[j + 1] && calls_end <= p.call_cut[j + 1];
            if (arrived && first_possible == p.k) first_possible = j;
            if (pc_launch_of_block(p, b, calls_end) == j) {
                ran += 1;
                CHECK(in_grid, "block %u is launch %u's, whose grid ends at block %u", b, j, j < p.k ? p.block_cut[j + 1] : nb);
                if (j < p.k) CHECK(arrived, "block %u runs in launch %u before its arrays are there (calls end %llu, chunk ends %llu)", b, j, (unsigned long long)calls_end, (unsigned long long)p.call_cut[j + 1]);
                CHECK(j == first_possible, "block %u runs in launch %u, could have run in %u", b, j, first_possible);
                if (j == p.k) CHECK(calls_end > nv, "block %u left to the catch-all although its calls end at %llu of %llu", b, (unsigned long long)calls_end, (unsigned long long)nv);
            }
        }
        CHECK(ran == 1, "block %u runs %u times", b, ran);
    }
}

int main() {
    const uint64_t ns[] = {1, 2, 255, 256, 257, 511, 512, 513, 1000, 2047, 2048, 4097, 9999, 65536, 100001, 300007};
    const uint64_t nvs[] = {1, 2, 7, 8, 9, 255, 1000, 4099, 65537, 300000, 1048576};
    const uint64_t floors[] = {0, 64, 4096, 1u << 20};
    for (uint64_t n : ns)
        for (uint64_t nv : nvs)
            for (int64_t want = -1; want <= PC_MAX_GROUPS + 1; ++want)
                for (uint64_t fl : floors) check_tiling(n, nv, want, fl);
    /* the flagship's size: four groups keep the 1 MiB floor, eight do not (var_type_zyg: one byte a call) */
    CHECK(plan_chunks(3570000, 7800000, 4, 1u << 20).k == 4, "a genome in four groups");
    CHECK(plan_chunks(3570000, 7800000, 8, 1u << 20).k == 0, "a genome in eight groups would copy less than 1 MiB of some array");
    CHECK(plan_chunks(0, 0, 4, 0).k == 0 && plan_chunks(100, 0, 4, 0).k == 0 && plan_chunks(0, 100, 4, 0).k == 0, "an empty batch has no plan");
    for (uint64_t n : ns)
        for (uint64_t nv : {(uint64_t)1, (uint64_t)100, (uint64_t)5000, (uint64_t)250000})
            for (int64_t want = 2; want <= PC_MAX_GROUPS; ++want)
                for (int shape = 0; shape < 5; ++shape) check_ownership(n, nv, want, shape);
    if (failures) {
        fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    printf("pack_chunks_check: ok\n");
    return 0;
}
