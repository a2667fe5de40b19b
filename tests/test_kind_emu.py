"""The call-kind kernel's own wave code (ck_wave_tile of aardvark_amd/csrc/avk_callkind.inl) on the CPU — tests/emu/kind_emu.cpp drives it the way the kernel and its
host loop do: three scopes a launch, tiles in grid-stride order, four waves on one block, one flush per workgroup; a wave's lanes are 64 threads that meet in every
cross-lane primitive — against the restatement of the rule (tests/kind_lib.py) on the ORACLE's per-call outputs.  Every comparison is exact.

Region counts 1, 63, 64, 65 (around the wave) and T - 1, T, T + 1, 2T + 1 (around the workgroup's tile); grids of 1 and 3; 0, 1, 33 and 49 labels (the second mask
word); a launch whose block of scopes starts at a scope > 0; the allele bytes through one 2-byte read (allele 1 behind allele 0), through two offsets, and through
the packed source's running offset."""
import copy

import numpy as np
import pytest

import kind_lib
import oracle_lib

T = 256


@pytest.fixture(scope="module")
def job():
    """the shared fixture, the oracle's results as the device view: never changed"""
    j = kind_lib.build_case(oracle_lib.load())
    solved = np.flatnonzero(j["solved"])
    j["starved"] = [int(r) for r in solved[10:12]]  # shown as AVK_ST_CAPACITY: they must not count
    j["calls"] = j["calls"][~np.isin(j["calls"][:, 0], j["starved"])]
    j["view"] = kind_lib.device_view(j["batch"], j["want"], starved=j["starved"])
    assert j["batch"].n_regions > 2 * T + 1 and np.array_equal(j["batch"].a1_off, j["batch"].a0_off + j["batch"].a0_len.astype(np.uint64))
    return j


def run(j, n, members=None, grid=3, view=None, **kw):
    view = (view or j["view"])[0]
    full = int(view.n_regions)
    view.n_regions = n  # (a batch of the first n regions: the arrays behind them are not read)
    try:
        L = 0 if members is None else len(members)
        mask = None if members is None else kind_lib.size_lib.mask_of_members([m[:n] for m in members], n)
        got = kind_lib.emu_run(view, mask=mask, n_labels=L, grid=grid, **kw)
    finally:
        view.n_regions = full
    return got, kind_lib.expected(j["calls"], j["batch"].n_regions, members, lo=0, hi=n)


def test_geometry():
    lib = kind_lib.load()
    assert lib.kind_emu_threads() == T and lib.kind_emu_scopes() == 3 and lib.kind_emu_lds_bytes() == 40960 >= 3 * 9 * 13 * 14 * 8


@pytest.mark.parametrize("grid", [1, 3])
@pytest.mark.parametrize("n", [1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1])
def test_region_counts(job, n, grid):
    got, want = run(job, n, grid=grid)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert want.any()


def test_whole_batch_and_the_law(job):
    """every region, the hand-written ones and the injected long alleles among them; summed over the kinds the block is the oracle's tally"""
    n = job["batch"].n_regions
    got, want = run(job, n, grid=3)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert all(want[0, k, 0].any() for k in range(6))  # (the oracle refuses a region with a call of unknown zygosity: no solved region holds a nogt_* call)
    solved = job["solved"].copy()
    solved[job["starved"]] = False
    tally = np.asarray(job["want"].group_metrics).reshape(n, 13, 22)[solved].astype(np.uint64).sum(axis=0)
    assert np.array_equal(got[0].sum(axis=0), tally[:, :14])


def members_of(job, n_labels, seed):
    n = job["batch"].n_regions
    rng = np.random.default_rng(seed)
    m = [rng.random(n) < p for p in rng.random(n_labels) * 0.6]
    if n_labels > 2:
        m[0], m[1] = np.ones(n, bool), np.zeros(n, bool)
    return m


@pytest.mark.parametrize("grid", [1, 3])
@pytest.mark.parametrize("n_labels", [1, 33, 49])
def test_labels(job, n_labels, grid):
    """1 label: one launch of two scopes; 33 and 49: twelve and seventeen launches, the last labels in the second mask word"""
    members = members_of(job, n_labels, 5 + n_labels)
    got, want = run(job, T + 1, members=members, grid=grid)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert got[n_labels].any() and not np.array_equal(got[n_labels], got[0])
    if n_labels > 2:
        assert np.array_equal(got[1], got[0]) and not got[2].any()


def test_a_launch_that_starts_at_a_scope_above_0(job):
    """the launch of scopes 36 .. 38 alone (labels 35, 36, 37: the second mask word), and the launches of scopes 4 .. 7 (two launches, the second of one scope)"""
    members = members_of(job, 49, 9)
    for lo, hi in ((36, 39), (4, 8)):
        got, want = run(job, 2 * T + 1, members=members, grid=3, scope_lo=lo, scope_hi=hi)
        want[:lo], want[hi:] = 0, 0
        assert np.array_equal(got, want), np.argwhere(got != want)[:8]
        assert all(got[s].any() for s in range(lo, hi))


def test_two_offsets(job):
    """the wide form's two offsets: allele 1 of every call lies in a second copy of the arena, so no call takes the 2-byte read"""
    b = copy.copy(job["batch"])
    arena = np.asarray(b.allele_bytes, np.uint8)
    b.allele_bytes = np.concatenate([arena, arena])
    b.a1_off = np.asarray(b.a1_off, np.uint64) + np.uint64(arena.size)
    assert np.array_equal(kind_lib.kinds_of(b), kind_lib.kinds_of(job["batch"]))
    view = kind_lib.device_view(b, job["want"], starved=job["starved"])
    got, want = run(job, job["batch"].n_regions, grid=3, view=view)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    # an allele offset outside the allele array: such a call is `other`, and nothing is read
    view[0].alleles_len = arena.size
    got, _ = run(job, job["batch"].n_regions, grid=1, view=view)
    moved = job["calls"].copy()
    one_one = (np.asarray(b.a0_len)[moved[:, 12]] == 1) & (np.asarray(b.a1_len)[moved[:, 12]] == 1)
    moved[one_one, 11] = moved[one_one, 11] // 3 * 3 + 2
    assert np.array_equal(got, kind_lib.expected(moved, job["batch"].n_regions)) and not got[0, [0, 1, 3, 4]].any()


def test_packed_source(job):
    """the calls through the packed source's arrays: type and zygosity from one byte, the alleles at the running offset"""
    b = job["plain"]  # (no escapes: lengths fit a byte)
    res = oracle_lib.compare_batch(oracle_lib.load(), b, job["contigs"], threads=8)
    view = kind_lib.device_view(b, res, packed_source=True)
    n = b.n_regions
    members = [np.arange(n) % 3 == 0]
    got = kind_lib.emu_run(view[0], mask=kind_lib.size_lib.mask_of_members(members, n), n_labels=1, grid=1)
    want = kind_lib.expected(kind_lib.calls_of(b, res), n, members)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert got[1].any() and all(got[0, k].any() for k in range(6))


def test_nogt_rows_from_a_synthetic_batch(job):
    """the oracle solves no region with a call outside het / hom, so the nogt rows are reached with a batch that is not the oracle's: the fixture's calls with every
    third input zygosity replaced by Unknown, HomozygousReference, 6 or 7, under the oracle's results of the original batch"""
    b = copy.copy(job["batch"])
    z = np.asarray(b.var_zyg, np.uint8).copy()
    z[::3] = np.resize(np.array([0, 1, 6, 7], np.uint8), z[::3].size)
    b.var_zyg = z
    calls = kind_lib.calls_of(b, job["want"])
    calls = calls[~np.isin(calls[:, 0], job["starved"])]
    view = kind_lib.device_view(b, job["want"], starved=job["starved"])
    n = b.n_regions
    members = [np.arange(n) % 2 == 0]
    got = kind_lib.emu_run(view[0], mask=kind_lib.size_lib.mask_of_members(members, n), n_labels=1, grid=3)
    want = kind_lib.expected(calls, n, members)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert all(got[s, k].any() for s in (0, 1) for k in range(9))
