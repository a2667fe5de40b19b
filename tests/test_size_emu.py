"""The size-bin kernel's own wave code (sz_wave_tile of aardvark_amd/csrc/avk_sizebin.inl) on the CPU — tests/emu/size_emu.cpp drives it the way the kernel and its
host loop do: blocks of scopes sized from the LDS budget, tiles in grid-stride order, four waves on one block, one flush per workgroup; a wave's lanes are 64
threads that meet in every cross-lane primitive — against the restatement of the rule (tests/size_lib.py) on the ORACLE's per-call outputs.  Every comparison is
exact.

Grid sizes 1 and 3; region counts 1, 63, 64, 65 (around the wave) and the whole batch (six tiles of 256 regions); 1, 4 and 15 edges; with and without masks, a
label in the second mask word; both sources of the calls' arrays (wide, the packed source)."""
import numpy as np
import pytest

import label_emu_lib
import oracle_lib
import scenarios
import size_lib
from aardvark_amd import synth


def make(contigs, batch):
    res = oracle_lib.compare_batch(oracle_lib.load(), batch, contigs, threads=8)
    solved = np.flatnonzero(np.asarray(res.status) == 0)
    starved = [int(r) for r in solved[10:12]]  # shown as AVK_ST_CAPACITY: they must not count
    calls = size_lib.calls_of(batch, res)
    calls = calls[~np.isin(calls[:, 0], starved)]
    return dict(batch=batch, res=res, calls=calls, starved=starved)


@pytest.fixture(scope="module")
def job():
    """indels of every default bin with the invalid regions behind them (unsolved), the oracle's results as the device view: shared, never changed"""
    contigs, base = scenarios.indel_small(1500)
    _, bad = scenarios.invalid_regions()
    j = make(contigs, synth.concat_batches([base, bad]))
    assert (np.asarray(j["res"].status) != 0).any() and j["batch"].n_regions > 5 * 256
    j["view"] = label_emu_lib.device_view(j["batch"], j["res"], starved=j["starved"])
    return j


@pytest.fixture(scope="module")
def packed_job():
    """fuzzed regions whose calls the lanes read through the packed source's arrays"""
    contigs, batch = scenarios.fuzz_regions(341, 130, max_vars=9, max_len=12)
    j = make(contigs, batch)
    j["view"] = label_emu_lib.device_view(batch, j["res"], packed_source=True, starved=j["starved"])
    return j


def run(j, n, edges, members=None, grid=3):
    view = j["view"][0]
    full = int(view.n_regions)
    view.n_regions = n  # (a batch of the first n regions: the arrays behind them are not read)
    try:
        L = 0 if members is None else len(members)
        mask = None if members is None else size_lib.mask_of_members([m[:n] for m in members], n)
        got = size_lib.emu_run(view, edges, mask=mask, n_labels=L, grid=grid)
    finally:
        view.n_regions = full
    return got, size_lib.expected(j["calls"], edges, j["batch"].n_regions, members, lo=0, hi=n)


def test_geometry():
    lib = size_lib.load()
    assert lib.size_emu_threads() == 256 and lib.size_emu_lds_bytes() >= 16 * 13 * 14 * 8


@pytest.mark.parametrize("grid", [1, 3])
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_around_the_wave(job, n, grid):
    got, want = run(job, n, size_lib.DEFAULT, grid=grid)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert want.any()


@pytest.mark.parametrize("edges", size_lib.EDGE_SETS)
def test_whole_batch(job, edges):
    got, want = run(job, job["batch"].n_regions, edges, grid=3)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert sum(bool(want[0, b, 0].any()) for b in range(len(edges) + 1)) >= min(len(edges) + 1, 4)  # (sizes 0 .. 17 occur)
    # the conservation law, against the oracle's blocks
    solved = np.asarray(job["res"].status) == 0
    solved[job["starved"]] = False
    tally = np.asarray(job["res"].group_metrics).reshape(job["batch"].n_regions, 13, 22)[solved].astype(np.uint64).sum(axis=0)
    assert np.array_equal(got[0].sum(axis=0), tally[:, :14])


def test_scopes(job):
    """scope 0, a label on every region, one on none, runs of regions; the unsolved regions are under every label and count under none"""
    n = job["batch"].n_regions
    rng = np.random.default_rng(5)
    runs = np.zeros(n, bool)
    for s in rng.integers(0, n, 6):
        runs[s:s + int(rng.integers(1, 300))] = True
    unsolved = np.asarray(job["res"].status) != 0
    members = [np.ones(n, bool), np.zeros(n, bool), runs | unsolved]
    got, want = run(job, n, size_lib.DEFAULT, members=members, grid=1)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert np.array_equal(got[1], got[0]) and not got[2].any() and got[3].any() and not np.array_equal(got[3], got[0])


def test_a_label_in_the_second_mask_word(job):
    """34 labels over 65 regions and 16 bins: one scope a launch, label 33 in the second word"""
    n = 65
    rng = np.random.default_rng(6)
    members = [np.ones(n, bool)] + [np.zeros(n, bool)] * 31 + [rng.random(n) < 0.5, rng.random(n) < 0.5]
    got, want = run(job, n, size_lib.FIFTEEN, members=members, grid=1)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert got[33].any() and got[34].any() and not got[2:33].any() and not np.array_equal(got[33], got[34])


@pytest.mark.parametrize("edges", [size_lib.DEFAULT, (2,)])
def test_packed_source(packed_job, edges):
    n = packed_job["batch"].n_regions
    members = [np.arange(n) % 3 == 0]
    got, want = run(packed_job, n, edges, members=members, grid=1)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert got[1].any()
