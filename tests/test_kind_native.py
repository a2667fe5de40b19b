"""The host route of the call kinds (avk_kind_tallies_host) without a GPU: against the restatement of tests/kind_lib.py on the ORACLE's per-call outputs of the
fixture every kind test shares — with 1 and 4 threads, with labels — the refusals, and the conservation law against the oracle's summed group_metrics.  Every
comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import aardvark_amd
import kind_lib
import oracle_lib
from aardvark_amd import _abi, kind_tallies_host


@pytest.fixture(scope="module")
def job():
    return kind_lib.build_case(oracle_lib.load())


@pytest.mark.parametrize("threads", [1, 4])
def test_host_route_equals_the_restatement(job, threads):
    got = kind_tallies_host(job["batch"], job["want"], threads=threads)
    want = kind_lib.expected(job["calls"], job["batch"].n_regions)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert all(got[0, k, 0, kind_lib.TRUTH_F[:2]].sum() > 0 and got[0, k, 0, kind_lib.QUERY_F[:2]].sum() > 0 for k in range(6))
    twice = kind_tallies_host(job["batch"], job["want"], threads=threads, out=got.copy())
    assert np.array_equal(twice, 2 * want)


def test_host_route_with_labels(job):
    n = job["batch"].n_regions
    rng = np.random.default_rng(2)
    m = [np.ones(n, bool), np.zeros(n, bool), rng.random(n) < 0.3, rng.random(n) < 0.05]
    lists = [[l for l in range(4) if m[l][r]] for r in range(n)]
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint64)
    got = kind_tallies_host(job["batch"], job["want"], labels=(4, off, np.array([l for x in lists for l in x] + [0], np.uint32)), threads=3)
    assert np.array_equal(got, kind_lib.expected(job["calls"], n, m))
    assert np.array_equal(got[1], got[0]) and not got[2].any() and got[3].any() and got[4].any()


def test_conservation_law_against_the_oracle(job):
    """for every group and f < 14 the sum over the kinds is the word of the oracle's tally: its group_metrics summed over the solved regions"""
    got = kind_tallies_host(job["batch"], job["want"])
    tally = np.asarray(job["want"].group_metrics).reshape(job["batch"].n_regions, _abi.N_GROUPS, _abi.N_FIELDS)[job["solved"]].astype(np.uint64).sum(axis=0)
    assert np.array_equal(got[0].sum(axis=0), tally[:, :14]) and tally[:, :14].any()


def test_refusals(job):
    lib = aardvark_amd.load_library()
    out = np.zeros((1, 9, _abi.N_GROUPS, 14), np.uint64)
    cb, ro = job["batch"].c_struct(), job["want"].c_struct()
    assert lib.avk_kind_tallies_host(C.byref(cb), C.byref(ro), None, 1, None) == -1 and "kind_tallies missing" in lib.avk_last_error(None).decode()
    assert lib.avk_kind_tallies_host(None, C.byref(ro), None, 1, out.ctypes.data_as(kind_lib.u64p)) == -1
    assert lib.avk_kind_tallies(None, None, None, out.ctypes.data_as(kind_lib.u64p)) == -1 and not out.any()


def test_nogt_rows_from_a_synthetic_batch(job):
    """no solved region of the oracle holds a nogt_* call: the rows are reached with every third input zygosity replaced by Unknown, HomozygousReference, 6 or 7"""
    import copy
    b = copy.copy(job["batch"])
    z = np.asarray(b.var_zyg, np.uint8).copy()
    z[::3] = np.resize(np.array([0, 1, 6, 7], np.uint8), z[::3].size)
    b.var_zyg = z
    got = kind_tallies_host(b, job["want"], threads=3)
    want = kind_lib.expected(kind_lib.calls_of(b, job["want"]), b.n_regions)
    assert np.array_equal(got, want) and all(got[0, k].any() for k in range(9))
