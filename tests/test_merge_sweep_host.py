"""One pair matrix decided under several strategies, without a GPU: avk_merge_classify_sweep (merge_facts_one + merge_decide of aardvark_amd/csrc/avk_mergesweep.inl)
against the single-config avk_merge_classify (merge_classify_one of avk_devpack.inl) on random pair matrices, its refusals, the reference's known answers of
tests/golden/merge_solver.json, the new exports, and tests/native/merge_sweep_check.cpp — a program of its own that runs the same header functions under the address
and undefined-behaviour sanitizers against a restatement of the rule.  All comparisons are exact."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import aardvark_amd
import oracle_lib
from aardvark_amd import _abi
from aardvark_amd.merge import AvkMergeConfig, MergeConfig, MergeResult, merge_classify_sweep, pair_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "merge_solver.json")))
KS = [1, 2, 3, 8, 9, 33, 64]
P = lambda a, t: a.ctypes.data_as(C.POINTER(t))


@pytest.fixture(scope="module")
def lib():
    return aardvark_amd.load_library()


def random_matrices(k, seed, n=96):
    """(in_cnt[n * k], unknown[n], pair_status[n * ppr], pair_exact[n * ppr]) — pair matrices of every density (most of them not transitive), matrices made from
    groups of equal inputs (transitive), regions with empty inputs and with nothing but empty inputs, one unknown zygosity, a non-zero pair status at the first, a
    middle and the last pair; for k >= 3 a region whose first majority set and one whose NoConflict set hold the LAST input (bit k - 1: bit 63 of members at k = 64)"""
    rng = np.random.default_rng(seed)
    pairs = [(i, j) for i in range(k) for j in range(i + 1, k)]
    ppr = len(pairs)
    cnt = rng.integers(0, 4, (n, k)) * (rng.random((n, k)) > 0.3)
    ex = np.zeros((n, max(ppr, 1)), np.uint8)
    st = np.zeros((n, max(ppr, 1)), np.int32)
    unknown = np.zeros(n, np.uint8)
    for m in range(n):
        if m % 3 == 0:  # groups of equal inputs
            g = rng.integers(0, 1 + m % 4, k)
            ex[m, :ppr] = [g[i] == g[j] for i, j in pairs]
        else:
            ex[m, :ppr] = rng.random(ppr) < (0.0, 0.3, 0.6, 0.9, 0.97, 1.0)[m % 6]
    cnt[5] = 0  # nothing but empty inputs
    cnt[6], ex[6] = 1, 1  # identical
    unknown[7] = 1
    if ppr:
        st[8, 0], st[9, ppr // 2], st[10, ppr - 1] = 3, 7, 21
        st[11, ppr - 1], st[11, 0] = 21, 2  # two of them: the first one in pair order is the answer
        unknown[12], st[12, 0] = 1, 3  # the zygosity comes first
    if k >= 3:
        cnt[13], ex[13] = 1, 1
        ex[13, 0] = 0  # all but the pair (0, 1): input 0's set is everything but input 1
        cnt[14], ex[14] = 0, 0
        cnt[14, k - 2:], ex[14, ppr - 1] = 2, 1  # the last two inputs alone, equal
    if not ppr:  # (one input: no pairs; the arrays are there but never read)
        st, ex = np.zeros(1, np.int32), np.zeros(1, np.uint8)
    return cnt.astype(np.uint32).reshape(-1), unknown, st.reshape(-1), ex.reshape(-1)


def all_configs(k):
    """the four strategies x conflict_selection in {-1, 0, k - 1}"""
    return [MergeConfig(no_conflict_enabled=nc, majority_voting_enabled=mv, conflict_selection=cs)
            for nc, mv in ((False, False), (True, False), (False, True), (True, True)) for cs in sorted({None, 0, k - 1}, key=lambda x: -1 if x is None else x)]


def single(lib, k, cnt, unknown, pst, pex, config):
    """avk_merge_classify"""
    n = cnt.size // k
    cfg = AvkMergeConfig(config.max_branch_factor, int(config.no_conflict_enabled), int(config.majority_voting_enabled), -1 if config.conflict_selection is None else int(config.conflict_selection))
    st, cl, mem = np.full(n, -9, np.int32), np.full(n, 9, np.uint8), np.full(n, 9, np.uint64)
    assert lib.avk_merge_classify(n, k, P(cnt, C.c_uint32), P(unknown, C.c_uint8), P(pst, C.c_int32), P(pex, C.c_uint8), C.byref(cfg), P(st, C.c_int32), P(cl, C.c_uint8),
                                  P(mem, C.c_uint64)) == 0
    return MergeResult(st, cl, mem, k)


def same(a, b):
    return np.array_equal(a.status, b.status) and np.array_equal(a.classification, b.classification) and np.array_equal(a.members, b.members)


@pytest.mark.parametrize("k", KS)
def test_every_config_of_a_sweep_decides_what_the_single_call_decides(lib, k):
    cnt, unknown, pst, pex = random_matrices(k, 500 + k)
    configs = all_configs(k)
    assert len(configs) == (12 if k > 1 else 8)
    want = [single(lib, k, cnt, unknown, pst, pex, c) for c in configs]
    # what the matrices are there to show
    ppr = k * (k - 1) // 2
    if ppr:
        assert want[0].status[[8, 9, 10, 11, 12]].tolist() == [3, 7, 21, 2, 6] and want[0].status[7] == 6
    if k >= 3:
        full = want[-1]  # both strategies on, conflict_selection k - 1
        assert set(full.classification[full.status == 0].tolist()) == {1, 2, 3, 4} and set(want[6].classification[want[6].status == 0].tolist()) == {0, 1, 3}
        last = np.uint64(1) << np.uint64(k - 1)
        assert want[6].classification[13] == 3 and want[6].members[13] & last and want[3].classification[14] == 2 and want[3].members[14] == last | (last >> np.uint64(1))
    # one at a time
    for c, w in zip(configs, want):
        got = merge_classify_sweep(lib, k, cnt, unknown, pst, pex, [c])
        assert len(got) == 1 and same(got[0], w)
    # eight at a time: every config in some sweep, duplicates side by side and apart
    rng = np.random.default_rng(k)
    picks = [list(range(8)), list(range(len(configs) - 8, len(configs))), [3, 3, 0, len(configs) - 1, 3, 0, 5, 5]] + [rng.integers(0, len(configs), 8).tolist() for _ in range(3)]
    for pick in picks:
        got = merge_classify_sweep(lib, k, cnt, unknown, pst, pex, [configs[i] for i in pick])
        assert len(got) == 8
        for i, g in zip(pick, got):
            assert same(g, want[i]), (k, pick, i)


def raw_sweep(lib, n, k, cnt, unknown, pst, pex, cfgs, n_cfgs, st, cl, mem):
    lib.avk_merge_classify_sweep.argtypes = [C.c_uint64, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.c_uint32,
                                             C.POINTER(AvkMergeConfig), C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)]
    ptr = lambda a, t: None if a is None else P(a, t)
    return lib.avk_merge_classify_sweep(n, k, ptr(cnt, C.c_uint32), ptr(unknown, C.c_uint8), ptr(pst, C.c_int32), ptr(pex, C.c_uint8), n_cfgs, cfgs, ptr(st, C.c_int32),
                                        ptr(cl, C.c_uint8), ptr(mem, C.c_uint64))


def test_refusals_write_nothing(lib):
    k, n = 3, 40
    cnt, unknown, pst, pex = random_matrices(k, 1, n)
    nine = (AvkMergeConfig * 9)(*[AvkMergeConfig(50, 1, 1, -1)] * 9)
    outs = lambda: (np.full(n, -77, np.int32), np.full(9 * n, 0xAB, np.uint8), np.full(9 * n, 0xABCD, np.uint64))
    untouched = lambda st, cl, mem: (st == -77).all() and (cl == 0xAB).all() and (mem == 0xABCD).all()
    st, cl, mem = outs()
    assert raw_sweep(lib, n, k, cnt, unknown, pst, pex, nine, 8, st, cl, mem) == 0 and (st != -77).all() and (cl[:8 * n] != 0xAB).all() and (cl[8 * n:] == 0xAB).all()
    for n_cfgs in (0, 9, 2 ** 31):
        st, cl, mem = outs()
        assert raw_sweep(lib, n, k, cnt, unknown, pst, pex, nine, n_cfgs, st, cl, mem) == -1 and untouched(st, cl, mem)  # AVK_E_ARG
    for bad, ok in ((k, False), (64, False), (-2, False), (k - 1, True), (-1, True)):
        cfgs = (AvkMergeConfig * 2)(AvkMergeConfig(50, 1, 1, 0), AvkMergeConfig(50, 0, 0, bad))  # (the refused config is the LAST one: nothing of the first is written)
        st, cl, mem = outs()
        rc = raw_sweep(lib, n, k, cnt, unknown, pst, pex, cfgs, 2, st, cl, mem)
        assert (rc == 0 and not untouched(st, cl, mem)) if ok else (rc == -1 and untouched(st, cl, mem)), bad
    for bad_k in (0, 65):
        st, cl, mem = outs()
        assert raw_sweep(lib, n, bad_k, cnt, unknown, pst, pex, nine, 2, st, cl, mem) == -1 and untouched(st, cl, mem)
    for missing in ("cnt", "pst", "pex", "cfgs", "st", "cl", "mem"):
        st, cl, mem = outs()
        a = dict(cnt=cnt, pst=pst, pex=pex, cfgs=nine, st=st, cl=cl, mem=mem)
        a[missing] = None
        assert raw_sweep(lib, n, k, a["cnt"], unknown, a["pst"], a["pex"], a["cfgs"], 2, a["st"], a["cl"], a["mem"]) == -1 and untouched(st, cl, mem), missing
    # has_unknown_zyg may be NULL, as for avk_merge_classify; no regions: nothing to write
    st, cl, mem = outs()
    assert raw_sweep(lib, n, k, cnt, None, pst, pex, nine, 2, st, cl, mem) == 0 and not untouched(st, cl, mem)
    st, cl, mem = outs()
    assert raw_sweep(lib, 0, k, cnt, unknown, None, None, nine, 2, st, cl, mem) == 0 and untouched(st, cl, mem)


def test_reference_known_answers_through_the_sweep(lib, oracle):
    """src/merge_solver.rs:243-370 and its doc-test: eight regions of three inputs under the three configs the file carries — ONE pair matrix (the oracle's),
    one sweep, every region's answer under its own config"""
    regions = [{"start": r["start"], "end": r["end"], "inputs": r["inputs"]} for r in GOLD["regions"]]
    carried = []
    for r in GOLD["regions"]:
        if r["config"] not in carried:
            carried.append(r["config"])
    assert len(carried) == 3 and len(regions) == 8
    batch, _ = pair_batch(regions)
    pst, pex = oracle_lib.optimize_pairs(oracle, batch, [GOLD["contig"].encode()], 50)
    cnt = np.array([[len(v) for v in r["inputs"]] for r in regions], np.uint32).reshape(-1)
    got = merge_classify_sweep(lib, 3, cnt, np.zeros(len(regions), np.uint8), pst, pex, [MergeConfig(**c) for c in carried])
    for m, r in enumerate(GOLD["regions"]):
        want = (0, tuple(r["expect"]) if len(r["expect"]) == 1 else (r["expect"][0], r["expect"][1]))
        assert got[carried.index(r["config"])].decoded()[m] == want, r["name"]
    # the strategies side by side, as a sweep is meant to be read: test_noconflict_mode_a is NoConflict, MajorityAgree or Different depending on the switches
    m = [r["name"] for r in GOLD["regions"]].index("test_noconflict_mode_a")
    assert {carried.index(c): got[carried.index(c)].decoded()[m][1][0] for c in carried} == {carried.index({}): "different", carried.index({"no_conflict_enabled": True}): "no_conflict",
                                                                                               carried.index({"majority_voting_enabled": True}): "majority"}


def test_the_new_exports_and_their_constant(lib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "aardvark_amd.h")).read(), flags=re.S)
    assert int(re.search(r"#define\s+AVK_MERGE_SWEEP_MAX\s+(\d+)", src).group(1)) == _abi.MERGE_SWEEP_MAX == 8
    for name in ("avk_merge_packed_sweep", "avk_merge_classify_sweep"):
        assert re.search(r"\b%s\s*\(" % name, src) and hasattr(lib, name), name
    assert C.sizeof(AvkMergeConfig) == 16  # (the kernel takes the three switches of each, 12 bytes; max_branch_factor belongs to the pair solve)


def test_the_header_functions_under_the_sanitizers(tmp_path):
    """tests/native/merge_sweep_check.cpp: merge_facts_one / merge_decide in both template forms (64 inputs: a word per input; 8: the kernel's, one word for all
    rows) and the body of avk_merge_classify_sweep, built with -fsanitize=address,undefined and run as a program of its own"""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no C++ compiler for tests/native/merge_sweep_check.cpp")
    exe = str(tmp_path / "merge_sweep_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(ROOT, "tests", "native", "merge_sweep_check.cpp")])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(out.stdout)
    assert out.returncode == 0 and "merge_sweep_check: ok" in out.stdout
