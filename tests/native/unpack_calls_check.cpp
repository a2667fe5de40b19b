/*
 * unpack_calls_check.cpp — dp_unpack_calls (aardvark_amd/csrc/avk_devpack.inl: the per-call outputs of a dense batch read from its packed source, four calls per
 * lane) against dp_unpack (one lane per region) under AddressSanitizer and UBSan, as a program of its own.  Every array a lane may read or write is a heap block
 * EXACTLY as long as its contents: var_out has n_calls words (16-byte aligned, as the pool's buffers are) and every per-call output n_calls bytes, so a load or store
 * past call n_calls - 1 stops the program.  (The library's own buffers are 16 bytes longer; the kernel must not need that.)  The lanes are driven as
 * avk_dp_unpack_calls_kernel drives them: whole workgroups of 256, lanes beyond the last call included.
 *
 * The batches: 1, 255, 256 and 257 regions of 0 to 3 calls a side (regions without calls on one side and on both among them); totals of 1, 3, 4 and 5 calls; a last
 * region of 1, 2 or 3 calls behind a multiple of four.  Every combination of the five outputs being wanted or NULL.  The per-call words are random in all 32 bits:
 * the map must be exact for any word.  Both routes start from outputs filled with a sentinel and must leave the same bytes.
 *
 * Built and run by tests/test_unpack_calls_native.py; never loaded into Python.
 */
#define AVK_EMU 1
#include <stdio.h>
#include <string.h>

#include <memory>
#include <new>
#include <vector>

#include "../emu/wave_threads.h"

#include "../../aardvark_amd/csrc/avk_devpack.inl"

typedef uint8_t u8;
typedef uint32_t u32;
typedef uint64_t u64;
namespace dpk = avk::dp;

static u64 rng_state = 0x9E3779B97F4A7C15ull;
static u32 rnd32() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (u32)(rng_state >> 29);
}

struct Outputs {
    std::unique_ptr<u8[]> a[5];
    Outputs(u64 n, u32 wanted) {
        for (int k = 0; k < 5; ++k)
            if (wanted >> k & 1u) {
                a[k].reset(new u8[n]);
                memset(a[k].get(), 0xEE, n);
            }
    }
    void name(dpk::DpOut &o) const { o.var_expected = a[0].get(), o.var_observed = a[1].get(), o.var_class = a[2].get(), o.var_zyg = a[3].get(), o.var_packed = a[4].get(); }
};

static int check(const std::vector<std::pair<u32, u32>> &counts, u32 wanted, const char *what) {
    const u64 n = counts.size();
    std::unique_ptr<u8[]> tc(new u8[n]), qc(new u8[n]);
    std::unique_ptr<u64[]> pk_voff(new u64[n]);
    std::unique_ptr<u32[]> v_off(new u32[n]), region_out(new u32[4 * n]);
    u64 nv = 0;
    for (u64 r = 0; r < n; ++r) {
        tc[r] = (u8)counts[r].first, qc[r] = (u8)counts[r].second;
        pk_voff[r] = nv, v_off[r] = (u32)nv; /* the two exclusive running sums of the same counts */
        nv += counts[r].first + counts[r].second;
        for (int k = 0; k < 4; ++k) region_out[4 * r + k] = rnd32();
    }
    struct Aligned16 {
        void operator()(u32 *p) const { ::operator delete[](p, std::align_val_t(16)); }
    };
    std::unique_ptr<u32[], Aligned16> var_out(new (std::align_val_t(16)) u32[nv]);
    for (u64 v = 0; v < nv; ++v) var_out[v] = rnd32();
    dpk::DpOut o;
    memset(&o, 0, sizeof(o));
    o.region_out = region_out.get(), o.var_out = var_out.get(), o.v_off = v_off.get(), o.n_regions = n, o.n_variants = nv, o.v_lo = 0, o.mode = 0;
    o.pk_voff = pk_voff.get(), o.pk_tc = tc.get(), o.pk_qc = qc.get();
    std::unique_ptr<int32_t[]> status(new int32_t[n]);
    o.status = status.get();
    Outputs by_region(nv, wanted), by_element(nv, wanted);
    dpk::DpOut o_r = o, o_e = o;
    by_region.name(o_r), by_element.name(o_e);
    for (u64 r = 0; r < ((n + 255) / 256) * 256; ++r) dpk::dp_unpack(o_r, r);
    const u64 lanes = ((nv + 1023) / 1024) * 256;
    for (u64 q = 0; q < lanes; ++q) dpk::dp_unpack_calls(o_e, nv, q);
    for (int k = 0; k < 5; ++k)
        if ((wanted >> k & 1u) && nv && memcmp(by_region.a[k].get(), by_element.a[k].get(), nv) != 0) {
            printf("unpack_calls_check: %s, outputs %u: output %d differs\n", what, wanted, k);
            return 1;
        }
    return 0;
}

int main() {
    struct Case {
        const char *what;
        std::vector<std::pair<u32, u32>> counts;
    };
    std::vector<Case> cases;
    for (u32 n : {1u, 255u, 256u, 257u, 1500u}) {
        Case c{"random counts", {}};
        for (u32 r = 0; r < n; ++r) c.counts.push_back({r % 7 == 2 ? 0u : rnd32() % 4u, r % 5 == 1 ? 0u : rnd32() % 4u});
        cases.push_back(c);
    }
    cases.push_back({"1 call", {{1, 0}}});
    cases.push_back({"3 calls", {{1, 2}}});
    cases.push_back({"4 calls", {{2, 2}}});
    cases.push_back({"5 calls", {{3, 2}}});
    cases.push_back({"tail of 1", {{2, 2}, {1, 3}, {1, 0}}});
    cases.push_back({"tail of 2", {{2, 2}, {1, 3}, {0, 2}}});
    cases.push_back({"tail of 3", {{2, 2}, {1, 3}, {2, 1}}});
    cases.push_back({"empty regions", {{0, 2}, {3, 0}, {0, 0}, {1, 1}, {0, 0}, {0, 3}, {0, 0}}});
    cases.push_back({"large counts", {{255, 255}, {0, 0}, {200, 1}, {3, 250}}});
    int bad = 0;
    for (const Case &c : cases)
        for (u32 wanted = 1; wanted < 32; ++wanted) bad += check(c.counts, wanted, c.what);
    if (bad) return 1;
    printf("unpack_calls_check: ok (%zu batches, 31 sets of outputs each)\n", cases.size());
    return 0;
}
