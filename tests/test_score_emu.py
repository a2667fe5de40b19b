"""Both score kernels' own wave code (sc_wave_tile and sc_wave_curve of aardvark_amd/csrc/avk_score.inl) on the CPU — tests/emu/score_emu.cpp drives them the way the
kernels and their host loop do: blocks of scopes sized from the LDS budget, tiles in grid-stride order, four waves on one block, one flush per workgroup, then a
wave per (scope, group) row for the scans; a wave's lanes are 64 threads that meet in every cross-lane primitive — against the restatement of the rule
(tests/score_lib.py) on the ORACLE's per-call outputs.  Every comparison is exact.

Grid sizes 1 and 3 (six tiles of 256 regions: strides past the first); region counts 1, 63, 64, 65 and the whole batch; K = 1, 2, 10 and 31; with and without
masks, a label in the second mask word; both sources of the calls' arrays (wide, the packed source)."""
import numpy as np
import pytest

import label_emu_lib
import oracle_lib
import scenarios
import score_lib
import size_lib
from aardvark_amd import synth


def make(contigs, batch):
    res = oracle_lib.compare_batch(oracle_lib.load(), batch, contigs, threads=8)
    solved = np.flatnonzero(np.asarray(res.status) == 0)
    starved = [int(r) for r in solved[10:12]]  # shown as AVK_ST_CAPACITY: they must not count
    calls, vidx = size_lib.calls_of(batch, res), score_lib.call_index(batch, res)
    keep = ~np.isin(calls[:, 0], starved)
    return dict(batch=batch, res=res, calls=calls[keep], vidx=vidx[keep], alt_ed=size_lib.alt_eds(batch), starved=starved)


@pytest.fixture(scope="module")
def job():
    """indels with the invalid regions behind them (unsolved), the oracle's results as the device view: shared, never changed"""
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


def run(j, n, thresholds, members=None, grid=3, seed=7):
    view = j["view"][0]
    full = int(view.n_regions)
    scores = score_lib.scores_for(j["batch"].n_variants, thresholds, seed)
    view.n_regions = n  # (a batch of the first n regions: the arrays behind them are not read)
    try:
        L = 0 if members is None else len(members)
        mask = None if members is None else size_lib.mask_of_members([m[:n] for m in members], n)
        got = score_lib.emu_run(view, thresholds, scores, mask=mask, n_labels=L, grid=grid)
    finally:
        view.n_regions = full
    return got, score_lib.expected(j["calls"], j["vidx"], j["alt_ed"], thresholds, scores, j["batch"].n_regions, members, lo=0, hi=n)


def test_geometry():
    lib = score_lib.load()
    assert lib.score_emu_threads() == 256 and lib.score_emu_lds_bytes() >= 32 * 13 * 17 * 8


@pytest.mark.parametrize("grid", [1, 3])
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_around_the_wave(job, n, grid):
    got, want = run(job, n, score_lib.DEFAULT, grid=grid)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert want.any()


@pytest.mark.parametrize("thresholds", score_lib.SPECS)
def test_whole_batch(job, thresholds):
    """six tiles on three workgroups: every workgroup strides past its first tile"""
    got, want = run(job, job["batch"].n_regions, thresholds, grid=3)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    solved = np.asarray(job["res"].status) == 0
    solved[job["starved"]] = False
    tally = np.asarray(job["res"].group_metrics).reshape(job["batch"].n_regions, 13, 22)[solved].astype(np.uint64).sum(axis=0)
    score_lib.check_invariants(got, tally[:, :14][None])
    assert not np.array_equal(got[0, 0], got[0, -1]) and got[0, -1, 0].any()


def test_scopes(job):
    """scope 0, a label on every region, one on none, runs of regions; the unsolved regions are under every label and count under none"""
    n = job["batch"].n_regions
    rng = np.random.default_rng(5)
    runs = np.zeros(n, bool)
    for s in rng.integers(0, n, 6):
        runs[s:s + int(rng.integers(1, 300))] = True
    unsolved = np.asarray(job["res"].status) != 0
    members = [np.ones(n, bool), np.zeros(n, bool), runs | unsolved]
    got, want = run(job, n, score_lib.DEFAULT, members=members, grid=1)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert np.array_equal(got[1], got[0]) and not got[2].any() and got[3].any() and not np.array_equal(got[3], got[0])


def test_a_label_in_the_second_mask_word(job):
    """34 labels over 65 regions and 32 points: one scope a launch, label 33 in the second word"""
    n = 65
    rng = np.random.default_rng(6)
    members = [np.ones(n, bool)] + [np.zeros(n, bool)] * 31 + [rng.random(n) < 0.5, rng.random(n) < 0.5]
    got, want = run(job, n, score_lib.THIRTY_ONE, members=members, grid=1)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert got[33].any() and got[34].any() and not got[2:33].any() and not np.array_equal(got[33], got[34])


@pytest.mark.parametrize("thresholds", [score_lib.DEFAULT, (20.0,)])
def test_packed_source(packed_job, thresholds):
    n = packed_job["batch"].n_regions
    members = [np.arange(n) % 3 == 0]
    got, want = run(packed_job, n, thresholds, members=members, grid=1)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert got[1].any()
