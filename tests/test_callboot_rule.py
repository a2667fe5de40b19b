"""The rule of the per-call bootstrap (aardvark_amd/csrc/avk_callboot.h) without a GPU: the header's layout macro and cap as the text states
them, and the host routes (avk_size_boot_tallies_host, avk_kind_boot_tallies_host) against the restatement of tests/callboot_lib.py on the ORACLE's per-call outputs —
without labels, with labels, with a label named twice in a region's list, with 1 and 16 threads — and their refusals.  Every comparison is exact."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import aardvark_amd
import callboot_lib as cbl
import kind_lib
import oracle_lib
import size_lib
from aardvark_amd import BootSpec, SizeSpec, _abi, kind_boot_tallies_host, size_boot_tallies_host

SEED = 77
KIND, DEFAULT, FIFTEEN = cbl.KIND, cbl.size(size_lib.DEFAULT), cbl.size(size_lib.FIFTEEN)
HEADER = os.path.join(cbl.CSRC, "avk_callboot.h")


@pytest.fixture(scope="module")
def job():
    j = kind_lib.build_case(oracle_lib.load())
    j["keys"] = (np.asarray(j["batch"].contig_idx, np.uint64), np.asarray(j["batch"].start, np.uint64))
    return j


def host(j, family, B, labels=None, threads=1, out=None, seed=SEED):
    if family == KIND:
        return kind_boot_tallies_host(j["batch"], j["want"], BootSpec(B, seed), labels=labels, threads=threads, out=out)
    return size_boot_tallies_host(j["batch"], j["want"], SizeSpec(list(family[1])), BootSpec(B, seed), labels=labels, threads=threads, out=out)


def test_the_header_states_the_layout_and_the_cap():
    src = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"#define AVK_CALLBOOT_AT\(scope, B, b, n_keys, key, g, f\)\s*\\\n\s*(.*)", code)
    assert m, "the layout macro"
    expr = m.group(1).replace("(uint64_t)", "").replace("AVK_N_GROUPS", "13").replace("AVK_SIZE_FIELDS", "14")
    rng = np.random.default_rng(1)
    for _ in range(50):
        B, K = int(rng.integers(1, 4097)), int(rng.integers(1, 17))
        scope, b, key, g, f = int(rng.integers(0, 50)), int(rng.integers(0, B)), int(rng.integers(0, K)), int(rng.integers(0, 13)), int(rng.integers(0, 14))
        assert eval(expr, {}, dict(scope=scope, B=B, b=b, n_keys=K, key=key, g=g, f=f)) == cbl.at(scope, B, b, K, key, g, f)
    cap = int(re.search(r"#define AVK_CALLBOOT_MAX_BLOCKS (\d+)u", code).group(1))
    assert cap == cbl.MAX_BLOCKS == _abi.CALLBOOT_MAX_BLOCKS and cap >= 1000 * 9 * 17 and cbl.BLOCK_BYTES == 13 * 14 * 8
    assert "AVK_CALLBOOT_SIZE = 0" in code and "AVK_CALLBOOT_KIND = 1" in code and "avk_boot_weight" in src


@pytest.mark.parametrize("family", [KIND, DEFAULT, FIFTEEN], ids=["kind", "size5", "size16"])
def test_host_route_equals_the_restatement(job, family):
    n, B = job["batch"].n_regions, 5
    got = host(job, family, B)
    want = cbl.expected(job["calls"], n, None, B, SEED, family, keys=job["keys"])
    assert got.shape == want.shape and np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert all(got[0, b].any() for b in range(B)) and not np.array_equal(got[0, 0], got[0, 1])
    twice = host(job, family, B, out=got.copy())
    assert np.array_equal(twice, 2 * want)
    assert not np.array_equal(host(job, family, B, seed=SEED + 1), want)


def test_threads_1_against_16(job):
    for family in (KIND, DEFAULT):
        assert np.array_equal(host(job, family, 7, threads=1), host(job, family, 7, threads=16))


def test_unweighted_replicates_are_the_plain_blocks(job):
    """the restatement's own anchor: with every weight 1 it is kind_lib's / size_lib's block"""
    n = job["batch"].n_regions
    X = cbl.region_blocks(job["calls"], n, KIND).sum(axis=0)
    assert np.array_equal(X, kind_lib.expected(job["calls"], n)[0])
    X = cbl.region_blocks(job["calls"], n, DEFAULT).sum(axis=0)
    assert np.array_equal(X, size_lib.expected(job["calls"], size_lib.DEFAULT, n)[0])


@pytest.mark.parametrize("family", [KIND, DEFAULT], ids=["kind", "size"])
def test_host_route_with_labels_and_a_label_named_twice(job, family):
    n, B = job["batch"].n_regions, 4
    rng = np.random.default_rng(2)
    m = [np.ones(n, bool), np.zeros(n, bool), rng.random(n) < 0.3, rng.random(n) < 0.05]
    lists = [[l for l in range(4) if m[l][r]] for r in range(n)]
    solved = np.flatnonzero(job["solved"])
    twice_in = [int(r) for r in solved[5:25]]
    for r in twice_in:
        lists[r] = lists[r] + [2, 2] if 2 not in lists[r] else lists[r] + [2]  # label 2 named twice in these regions' lists
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint64)
    idx = np.array([l for x in lists for l in x] + [0], np.uint32)
    got = host(job, family, B, labels=(4, off, idx), threads=3)
    want = cbl.expected_lists(job["calls"], n, (4, off, idx), B, SEED, family, job["keys"])
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert np.array_equal(got[1], got[0]) and not got[2].any() and got[3].any() and got[4].any()
    members = [m[0], m[1], m[2].copy(), m[3]]
    members[2][twice_in] = True
    once = cbl.expected(job["calls"], n, members, B, SEED, family, keys=job["keys"])
    assert np.array_equal(got[[0, 1, 2, 4]], once[[0, 1, 2, 4]]) and not np.array_equal(got[3], once[3]), "named twice counts twice"


def test_refusals_leave_out_untouched(job):
    lib = aardvark_amd.load_library()
    u64p = C.POINTER(C.c_uint64)
    out = np.zeros((1, 2, 9, _abi.N_GROUPS, 14), np.uint64)
    o = out.ctypes.data_as(u64p)
    cb, ro = job["batch"].c_struct(), job["want"].c_struct()
    err = lambda: lib.avk_last_error(None).decode()
    spec = lambda B: C.byref(BootSpec(B, 1).c_struct())
    assert lib.avk_kind_boot_tallies_host(C.byref(cb), C.byref(ro), spec(2), None, 1, None) == -1 and "kind_boot_tallies missing" in err()
    assert lib.avk_kind_boot_tallies_host(C.byref(cb), C.byref(ro), spec(0), None, 1, o) == -1 and "replicates" in err()
    assert lib.avk_kind_boot_tallies_host(C.byref(cb), C.byref(ro), spec(4097), None, 1, o) == -1 and "replicates" in err()
    assert lib.avk_kind_boot_tallies_host(None, C.byref(ro), spec(2), None, 1, o) == -1
    bad = size_lib.c_spec([5, 3])
    assert lib.avk_size_boot_tallies_host(C.byref(cb), C.byref(ro), C.byref(bad), spec(2), None, 1, o) == -1 and "edges" in err()
    ok = size_lib.c_spec(list(size_lib.FIFTEEN))
    assert lib.avk_size_boot_tallies_host(C.byref(cb), C.byref(ro), C.byref(ok), spec(2), None, 1, None) == -1 and "size_boot_tallies missing" in err()
    # over the cap: 4096 replicates x 16 bins x 5 scopes = 327,680 blocks; within it, 4096 x 16 x 4 = 262,144 is not refused for that (the labels are then looked at)
    n = job["batch"].n_regions
    lab, keep = _abi.region_labels(4, np.zeros(n + 1, np.uint64), np.zeros(1, np.uint32))
    assert lib.avk_size_boot_tallies_host(C.byref(cb), C.byref(ro), C.byref(ok), spec(4096), C.byref(lab), 1, o) == -1 and "blocks" in err()
    assert lib.avk_callboot_block(None, 9) == 0
    assert not out.any()
