/*
 * merge_sweep_check.cpp — the header functions of aardvark_amd/csrc/avk_mergesweep.inl on the CPU, a program of its own (tests/test_merge_sweep_host.py builds it
 * with -fsanitize=address,undefined and runs it; it is never loaded into another process).
 *
 * For k in {1, 2, 3, 8, 9, 33, 64} and random pair matrices of the kinds tests/test_merge_sweep_host.py uses — dense and sparse ones that are not transitive,
 * groups of equal inputs, empty inputs, an unknown zygosity, a pair that is not solved first, in the middle and last — merge_classify_sweep_host (the body of
 * avk_merge_classify_sweep) decides under the four strategies x conflict_selection in {-1, 0, k - 1}, eight configs at a time with duplicates, and every answer is
 * compared with a restatement of solve_merge_region's decision (src/merge_solver.rs:149-199) written here with sets of indices.  For k <= 8 the kernel's lane
 * function ms_sweep_lane (the 8-input form of the match sets: one word for all rows) runs on the same matrices laid out as the pair solve's records.
 * The arrays are exactly as long as the functions may read or write, so that an access outside them is an error of the run.
 */
#define AVK_EMU 1
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../aardvark_amd/csrc/avk_mergesweep.inl"

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() { /* xorshift64* */
    rng_state ^= rng_state >> 12, rng_state ^= rng_state << 25, rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}

struct Want {
    int32_t status;
    uint8_t cls;
    uint64_t members;
};
/* the rule, stated with vectors of indices */
Want restated(uint32_t k, const uint32_t *cnt, bool unknown, const int32_t *pst, const uint8_t *pex, const avk_merge_config &cfg) {
    Want w = {0, AVK_MERGE_DIFFERENT, 0};
    if (unknown) {
        w.status = AVK_ST_BAD_ZYGOSITY;
        return w;
    }
    std::vector<std::vector<uint32_t>> sets(k);
    for (uint32_t i = 0; i < k; ++i) sets[i].push_back(i);
    bool identical = true, no_conflict = true;
    size_t p = 0;
    for (uint32_t i = 0; i < k; ++i)
        for (uint32_t j = i + 1; j < k; ++j, ++p) {
            if (pst[p]) {
                w.status = pst[p];
                return w;
            }
            const bool e = pex[p] != 0;
            identical = identical && e;
            if (cnt[i] && cnt[j] && !e) no_conflict = false;
            if (e) sets[i].push_back(j), sets[j].push_back(i);
        }
    auto mask = [](const std::vector<uint32_t> &s) {
        uint64_t m = 0;
        for (uint32_t i : s) m |= 1ull << i;
        return m;
    };
    if (identical) w.cls = AVK_MERGE_IDENTICAL;
    else if (cfg.no_conflict_enabled && no_conflict) {
        w.cls = AVK_MERGE_NO_CONFLICT;
        for (uint32_t i = 0; i < k; ++i)
            if (cnt[i]) w.members |= 1ull << i;
    } else {
        const std::vector<uint32_t> *maj = nullptr;
        for (uint32_t i = 0; i < k && !maj; ++i)
            if (sets[i].size() >= k / 2 + 1) maj = &sets[i];
        if (cfg.majority_voting_enabled && maj) w.cls = AVK_MERGE_MAJORITY_AGREE, w.members = mask(*maj);
        else if (cfg.conflict_selection >= 0) w.cls = AVK_MERGE_CONFLICT_SELECTION, w.members = (uint64_t)cfg.conflict_selection;
    }
    return w;
}

int check(uint32_t k, uint64_t n) {
    const uint64_t ppr = (uint64_t)k * (k - 1) / 2;
    std::vector<uint32_t> cnt(n * k);
    std::vector<uint8_t> unknown(n, 0), pex(ppr ? n * ppr : 1); /* (one input: no pairs; the pointers are there and never read) */
    std::vector<int32_t> pst(ppr ? n * ppr : 1, 0);
    for (uint64_t m = 0; m < n; ++m) {
        for (uint32_t i = 0; i < k; ++i) cnt[m * k + i] = rnd() % 10 < 3 ? 0u : rnd() % 4;
        if (m % 3 == 0) { /* groups of equal inputs */
            std::vector<uint32_t> g(k);
            for (uint32_t i = 0; i < k; ++i) g[i] = rnd() % (1 + m % 4);
            uint64_t p = 0;
            for (uint32_t i = 0; i < k; ++i)
                for (uint32_t j = i + 1; j < k; ++j, ++p) pex[m * ppr + p] = g[i] == g[j];
        } else {
            const uint32_t density[6] = {0, 30, 60, 90, 97, 100};
            for (uint64_t p = 0; p < ppr; ++p) pex[m * ppr + p] = rnd() % 100 < density[m % 6];
        }
    }
    for (uint32_t i = 0; i < k; ++i) cnt[5 * k + i] = 0, cnt[6 * k + i] = 1;
    for (uint64_t p = 0; p < ppr; ++p) pex[6 * ppr + p] = 1;
    unknown[7] = 1, cnt[7 * k] = 1;
    if (ppr) {
        pst[8 * ppr] = 3, pst[9 * ppr + ppr / 2] = 7, pst[10 * ppr + ppr - 1] = 21;
        pst[11 * ppr + ppr - 1] = 21, pst[11 * ppr] = 2;
        unknown[12] = 1, cnt[12 * k] = 2, pst[12 * ppr] = 3;
    }
    if (k >= 3) { /* the last input in a majority set and in a NoConflict set */
        for (uint32_t i = 0; i < k; ++i) cnt[13 * k + i] = 1, cnt[14 * k + i] = i + 2 >= k ? 2u : 0u;
        for (uint64_t p = 0; p < ppr; ++p) pex[13 * ppr + p] = p != 0, pex[14 * ppr + p] = p == ppr - 1;
    }
    std::vector<avk_merge_config> all;
    for (uint32_t s = 0; s < 4; ++s)
        for (int32_t cs : {-1, 0, (int32_t)k - 1}) all.push_back({50u + s /* (not read) */, s & 1u, s >> 1, cs});
    int bad = 0;
    uint64_t last_bit_seen = 0;
    for (int round = 0; round < 6; ++round) {
        const uint32_t nc = round == 0 ? 1u : (uint32_t)AVK_MERGE_SWEEP_MAX;
        std::vector<avk_merge_config> cfgs(nc);
        for (uint32_t c = 0; c < nc; ++c) cfgs[c] = round == 1 ? all[c] : round == 2 ? all[all.size() - nc + c] : round == 3 ? all[(c / 2) * 5 % all.size()] : all[rnd() % all.size()];
        std::vector<int32_t> st(n, -9);
        std::vector<uint8_t> cl(nc * n, 9);
        std::vector<uint64_t> mem(nc * n, 9);
        if (avk::ms::merge_classify_sweep_host(n, k, cnt.data(), unknown.data(), pst.data(), pex.data(), nc, cfgs.data(), st.data(), cl.data(), mem.data()) != AVK_E_OK) {
            printf("k %u: the sweep refused a good call\n", k);
            return 1;
        }
        /* the kernel's lane function on the same matrices (records of four words: status, exact; calls with a zygosity byte each) */
        std::vector<int32_t> d_st(n, -9);
        std::vector<uint8_t> d_cl(nc * n, 9);
        std::vector<uint64_t> d_mem(nc * n, 9);
        if (k >= 2 && k <= (uint32_t)avk::ms::MS_KMAX) {
            std::vector<uint32_t> ro(n * ppr * 4);
            for (uint64_t p = 0; p < n * ppr; ++p) ro[4 * p] = (uint32_t)pst[p], ro[4 * p + 1] = pex[p], ro[4 * p + 2] = 0xDEADu, ro[4 * p + 3] = 0xBEEFu;
            std::vector<uint64_t> in_off(n * k);
            uint64_t nv = 0;
            for (uint64_t s = 0; s < n * k; ++s) in_off[s] = nv, nv += cnt[s];
            std::vector<uint8_t> zyg(nv, AVK_ZYG_HOM_ALT);
            for (uint64_t m = 0; m < n; ++m)
                if (unknown[m]) zyg[in_off[m * k]] = AVK_ZYG_UNKNOWN; /* (the first input of such a region has a call) */
            avk::ms::MsSweep c;
            memset(&c, 0, sizeof(c));
            c.region_out = ro.data(), c.in_off = in_off.data(), c.in_cnt = cnt.data(), c.var_zyg = zyg.data(), c.n_multi = n, c.n_variants = nv, c.k = k, c.ppr = (uint32_t)ppr, c.n_cfgs = nc;
            for (uint32_t q = 0; q < nc; ++q)
                c.cfg[q].no_conflict_enabled = cfgs[q].no_conflict_enabled, c.cfg[q].majority_voting_enabled = cfgs[q].majority_voting_enabled, c.cfg[q].conflict_selection = cfgs[q].conflict_selection;
            c.status = d_st.data(), c.classification = d_cl.data(), c.members = d_mem.data();
            for (uint64_t m = 0; m < n + 3; ++m) avk::ms::ms_sweep_lane(c, m); /* (lanes behind the last region write nothing) */
        }
        for (uint32_t c = 0; c < nc; ++c)
            for (uint64_t m = 0; m < n; ++m) {
                const Want w = restated(k, cnt.data() + m * k, unknown[m] != 0, pst.data() + m * ppr, pex.data() + m * ppr, cfgs[c]);
                if (st[m] != w.status || cl[c * n + m] != w.cls || mem[c * n + m] != w.members) {
                    if (bad++ < 5) printf("k %u config %u region %llu: host sweep (%d, %u, %llx), restated (%d, %u, %llx)\n", k, c, (unsigned long long)m, st[m], cl[c * n + m],
                                          (unsigned long long)mem[c * n + m], w.status, w.cls, (unsigned long long)w.members);
                }
                if (k >= 2 && k <= (uint32_t)avk::ms::MS_KMAX && (d_st[m] != w.status || d_cl[c * n + m] != w.cls || d_mem[c * n + m] != w.members)) {
                    if (bad++ < 5) printf("k %u config %u region %llu: lane function (%d, %u, %llx), restated (%d, %u, %llx)\n", k, c, (unsigned long long)m, d_st[m], d_cl[c * n + m],
                                          (unsigned long long)d_mem[c * n + m], w.status, w.cls, (unsigned long long)w.members);
                }
                if (w.cls == AVK_MERGE_NO_CONFLICT || w.cls == AVK_MERGE_MAJORITY_AGREE) last_bit_seen |= w.members >> (k - 1) & 1ull;
            }
    }
    if (k >= 3 && !last_bit_seen) {
        printf("k %u: no member set held the last input\n", k);
        return 1;
    }
    /* refusals write nothing */
    std::vector<int32_t> st(n, -9);
    std::vector<uint8_t> cl(9 * n, 9);
    std::vector<uint64_t> mem(9 * n, 9);
    std::vector<avk_merge_config> nine(9, all[0]);
    int refused = 0;
    refused += avk::ms::merge_classify_sweep_host(n, k, cnt.data(), unknown.data(), pst.data(), pex.data(), 0, nine.data(), st.data(), cl.data(), mem.data()) == AVK_E_ARG;
    refused += avk::ms::merge_classify_sweep_host(n, k, cnt.data(), unknown.data(), pst.data(), pex.data(), 9, nine.data(), st.data(), cl.data(), mem.data()) == AVK_E_ARG;
    nine[1].conflict_selection = (int32_t)k;
    refused += avk::ms::merge_classify_sweep_host(n, k, cnt.data(), unknown.data(), pst.data(), pex.data(), 2, nine.data(), st.data(), cl.data(), mem.data()) == AVK_E_ARG;
    refused += avk::ms::merge_classify_sweep_host(n, k, cnt.data(), unknown.data(), pst.data(), pex.data(), 2, nullptr, st.data(), cl.data(), mem.data()) == AVK_E_ARG;
    for (uint64_t m = 0; m < n; ++m) bad += st[m] != -9;
    for (uint64_t i = 0; i < 9 * n; ++i) bad += cl[i] != 9 || mem[i] != 9;
    if (refused != 4) {
        printf("k %u: %d of 4 bad calls refused\n", k, refused);
        return 1;
    }
    if (bad) printf("k %u: %d differences\n", k, bad);
    return bad != 0;
}

} // namespace

int main() {
    int bad = 0;
    for (uint32_t k : {1u, 2u, 3u, 8u, 9u, 33u, 64u}) bad += check(k, 96);
    bad += check(3, 15); /* a batch that ends with the special regions */
    if (bad) return 1;
    printf("merge_sweep_check: ok\n");
    return 0;
}
