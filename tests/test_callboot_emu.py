"""The per-call bootstrap kernel's own lane functions (aardvark_amd/csrc/avk_callboot.inl) on the CPU — tests/emu/callboot_emu.cpp drives them the way the kernel and
its host loop do: R replicates of one scope a launch, tiles in grid-stride order, a tile's calls in pieces of the record capacity, accumulators kept across a
workgroup's tiles, one flush — against the restatement of the rule (tests/callboot_lib.py) on the ORACLE's per-call outputs.  Every comparison is exact.

Tiles of 1, T - 1, T, T + 1 and 2 T + 1 regions; replicates 1, R, R + 1 and 2 R + 1 around a launch's count R for either family; the regions of more calls than
a piece holds (kind_lib.build_case's escaped batch: sides of 255, 256 and 300 calls against a capacity of 256), and every region in pieces at capacities of 1 and
7; a tile with no counting region; scopes in the second mask word; both key sources."""
import numpy as np
import pytest

import callboot_lib as cbl
import kind_lib
import oracle_lib
import size_lib

SEED = 0x5EED0002
LDS = 160 * 1024
KIND, DEFAULT, FIFTEEN = cbl.KIND, cbl.size(size_lib.DEFAULT), cbl.size(size_lib.FIFTEEN)


@pytest.fixture(scope="module")
def job():
    """the kind tests' fixture, the oracle's results as the device view: shared, never changed"""
    j = kind_lib.build_case(oracle_lib.load())
    solved = np.flatnonzero(j["solved"])
    j["starved"] = [int(r) for r in solved[10:12]]  # shown as AVK_ST_CAPACITY: they must not count
    j["calls"] = j["calls"][~np.isin(j["calls"][:, 0], j["starved"])]
    j["view"] = kind_lib.device_view(j["batch"], j["want"], starved=j["starved"])
    j["keys"] = (np.asarray(j["batch"].contig_idx, np.uint64), np.asarray(j["batch"].start, np.uint64))
    lib = cbl.load()
    j["T"], j["cap"] = lib.callboot_emu_tile(), lib.callboot_emu_recs()
    per_region = np.asarray(j["batch"].t_cnt, np.int64) + np.asarray(j["batch"].q_cnt, np.int64)
    j["long"] = [int(r) for r in np.flatnonzero((per_region > j["cap"]) & j["solved"])]
    assert j["long"], "a solved region holds more calls than a piece: the escaped batch's dense regions"
    assert j["batch"].n_regions > 2 * j["T"] + 1
    return j


def reps(family):
    return int(cbl.load().callboot_emu_reps(cbl.n_keys_of(family), LDS))


def run(j, n, B, family=KIND, members=None, grid=3, R=None, cap=None, view=None, seed=SEED, first=0):
    view = (view or j["view"])[0]
    full = int(view.n_regions)
    view.n_regions = n  # (a batch of the first n regions: the arrays behind them are not read)
    try:
        L = 0 if members is None else len(members)
        mask = None if members is None else size_lib.mask_of_members([m[:n] for m in members], n)
        got = cbl.emu_run(view, (j["keys"][0][:n], j["keys"][1][:n]), family, seed, B, reps(family) if R is None else R, cap=cap, mask=mask, n_labels=L, grid=grid)
    finally:
        view.n_regions = full
    return got, cbl.expected(j["calls"], n, members, B, seed, family, keys=j["keys"])


def test_geometry():
    lib = cbl.load()
    assert lib.callboot_emu_tile() == 64 and lib.callboot_emu_recs() == 256 and lib.callboot_emu_threads() == 256 and lib.callboot_emu_reps_max() == 18
    # the replicates of a launch follow from the LDS: 9 kinds, the 5 default bins (bounded by the lane teams), 16 bins and 2 bins, at 160 KB and at 64 KB
    assert [reps(f) for f in (KIND, DEFAULT, FIFTEEN, cbl.size((2,)))] == [11, 18, 6, 18]
    assert [int(lib.callboot_emu_reps(k, 64 * 1024)) for k in (9, 5, 16)] == [4, 7, 2]
    for k, lds in ((9, LDS), (16, LDS), (16, 64 * 1024), (5, 64 * 1024)):
        R = int(lib.callboot_emu_reps(k, lds))
        assert lib.callboot_emu_lds_bytes(k, R) <= lds and (R == 18 or lib.callboot_emu_lds_bytes(k, R + 1) > lds)
        assert lib.callboot_emu_lds_bytes(k, R) >= k * 13 * 14 * 8 * R + 256 * 32


@pytest.mark.parametrize("family", [KIND, DEFAULT], ids=["kind", "size"])
@pytest.mark.parametrize("n", ["1", "T-1", "T", "T+1", "2T+1"])
def test_tiles(job, n, family):
    T = job["T"]
    n = {"1": 1, "T-1": T - 1, "T": T, "T+1": T + 1, "2T+1": 2 * T + 1}[n]
    got, want = run(job, n, 3, family=family)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert want.any()


@pytest.mark.parametrize("family", [KIND, DEFAULT, FIFTEEN], ids=["kind", "size5", "size16"])
@pytest.mark.parametrize("B", ["1", "R", "R+1", "2R+1"])
def test_replicate_blocks(job, B, family):
    R = reps(family)
    B = {"1": 1, "R": R, "R+1": R + 1, "2R+1": 2 * R + 1}[B]
    got, want = run(job, 2 * job["T"] + 1, B, family=family, grid=2)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert all(want[0, b].any() for b in range(B))


@pytest.mark.parametrize("family", [KIND, DEFAULT], ids=["kind", "size"])
def test_whole_batch_with_the_regions_over_the_record_capacity(job, family):
    """every region, those of 510, 511 and 555 calls among them: walked in two and three pieces of 256 records; the replicates differ, and a replicate summed over
    its keys does not depend on the family"""
    n = job["batch"].n_regions
    got, want = run(job, n, 4, family=family)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    long_only = job["calls"][np.isin(job["calls"][:, 0], job["long"])]
    assert cbl.expected(long_only, n, None, 4, SEED, family, keys=job["keys"]).any(), "the long regions add to these replicates"
    assert not np.array_equal(got[0, 0], got[0, 1])
    other, _ = run(job, n, 4, family=DEFAULT if family == KIND else KIND)
    assert np.array_equal(got.sum(axis=2), other.sum(axis=2))


@pytest.mark.parametrize("cap", [1, 7, 255])
def test_small_pieces(job, cap):
    """the same walk at other capacities: every region of more than `cap` calls is cut, ranges begin and end inside pieces"""
    n = 2 * job["T"] + 1
    got, want = run(job, n, 3, cap=cap, grid=1)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    n = job["batch"].n_regions
    got, want = run(job, n, 2, family=DEFAULT, cap=255 if cap == 255 else 64, grid=3)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]


def test_a_tile_with_no_counting_region(job):
    """the scope of a label that holds no region of the second tile, and one that holds no region at all: the tile is skipped, what the tile before left is not read"""
    T, n = job["T"], 3 * job["T"] + 5
    hole = np.ones(n, bool)
    hole[T:2 * T] = False
    members = [hole, np.zeros(n, bool)]
    got, want = run(job, n, 3, members=members, grid=1)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert got[1].any() and not got[2].any() and not np.array_equal(got[1], got[0])


def test_scopes_in_the_second_mask_word(job):
    n = 2 * job["T"] + 1
    rng = np.random.default_rng(7)
    members = [np.ones(n, bool), np.zeros(n, bool)] + [rng.random(n) < 0.4 for _ in range(2)] + [np.zeros(n, bool)] * 29 + [rng.random(n) < 0.5]
    got, want = run(job, n, 2, family=DEFAULT, members=members)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert np.array_equal(got[1], got[0]) and not got[2].any() and got[3].any() and got[34].any() and not got[5:34].any()


def test_packed_source_and_another_seed(job):
    """the calls and the key through the packed source's arrays; another seed gives other replicates under the same rule"""
    b = job["plain"]  # (no escapes: lengths fit a byte)
    res = oracle_lib.compare_batch(oracle_lib.load(), b, job["contigs"], threads=8)
    view = kind_lib.device_view(b, res, packed_source=True)
    n = b.n_regions
    keys = (np.asarray(b.contig_idx, np.uint64), np.asarray(b.start, np.uint64))
    calls = kind_lib.calls_of(b, res)
    got = cbl.emu_run(view[0], keys, KIND, SEED, 3, reps(KIND), grid=2)
    assert np.array_equal(got, cbl.expected(calls, n, None, 3, SEED, KIND, keys=keys))
    other = cbl.emu_run(view[0], keys, KIND, SEED + 1, 3, reps(KIND), grid=2)
    assert np.array_equal(other, cbl.expected(calls, n, None, 3, SEED + 1, KIND, keys=keys)) and not np.array_equal(got, other)


def test_nogt_rows_from_a_synthetic_batch(job):
    """the oracle solves no region with a call outside het / hom: the nogt kinds are reached as in tests/test_kind_emu.py"""
    import copy
    b = copy.copy(job["batch"])
    z = np.asarray(b.var_zyg, np.uint8).copy()
    z[::3] = np.resize(np.array([0, 1, 6, 7], np.uint8), z[::3].size)
    b.var_zyg = z
    calls = kind_lib.calls_of(b, job["want"])
    calls = calls[~np.isin(calls[:, 0], job["starved"])]
    view = kind_lib.device_view(b, job["want"], starved=job["starved"])
    n = b.n_regions
    got = cbl.emu_run(view[0], job["keys"], KIND, SEED, 2, reps(KIND), grid=3)
    want = cbl.expected(calls, n, None, 2, SEED, KIND, keys=job["keys"])
    assert np.array_equal(got, want) and all(got[0, :, k].any() for k in range(9))
