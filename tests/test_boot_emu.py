"""The bootstrap tally kernel's own lane functions (aardvark_amd/csrc/avk_boot.inl) on the CPU (tests/emu/boot_emu.cpp drives them the way the kernel does: tiles in
grid-stride order, sums kept across a workgroup's tiles, one flush) against the ORACLE's per-region blocks times weights from the numpy restatement of the rule
(tests/boot_lib.py).  Every comparison is exact.

Region counts 1, T - 1, T, T + 1 and 2 T + 1 around the kernel's tile T; replicate counts 1, R - 1, R, R + 1 and 2 R + 1 around a launch's block R; a scope on every
region, one on none, interval-like scopes (runs of regions), one scope in a second mask word; both key sources (wide arrays, the packed source)."""
import numpy as np
import pytest

import boot_lib
import label_emu_lib
import oracle_lib
import scenarios
from aardvark_amd import synth

WORDS = boot_lib.WORDS
SEED = 0x5EED0001


@pytest.fixture(scope="module")
def fuzz():
    """the fuzzed regions of tests/test_label_mask.py (with the invalid ones: unsolved), the oracle's results as the device view: shared, never changed"""
    contigs, batch = scenarios.fuzz_regions(341, 400, max_vars=9, max_len=12)
    _, bad = scenarios.invalid_regions()
    batch = synth.concat_batches([batch, bad])
    res = oracle_lib.compare_batch(oracle_lib.load(), batch, contigs, threads=8)
    solved = np.asarray(res.status) == 0
    assert solved.sum() > 300 and (~solved).sum() >= 1
    starved = [int(r) for r in np.flatnonzero(solved)[10:12]]  # shown as AVK_ST_CAPACITY: they must not count
    counts = solved.copy()
    counts[starved] = False
    views = {ps: label_emu_lib.device_view(batch, res, packed_source=ps, starved=starved) for ps in (False, True)}
    blocks = np.asarray(res.group_metrics).reshape(batch.n_regions, WORDS)
    return dict(batch=batch, views=views, counts=counts, blocks=blocks, contig=np.asarray(batch.contig_idx, np.uint64), start=np.asarray(batch.start, np.uint64))


def run(fuzz, n, B, packed=False, members=None, grid=3, seed=SEED):
    view = fuzz["views"][packed][0]
    full = int(view.n_regions)
    view.n_regions = n  # (a batch of the first n regions: the arrays behind them are not read)
    try:
        L = 0 if members is None else len(members)
        mask = None if members is None else boot_lib.mask_of_members(members, n)
        got = boot_lib.emu_run(view, fuzz["contig"][:n], fuzz["start"][:n], seed, B, mask=mask, n_labels=L, grid=grid)
    finally:
        view.n_regions = full
    w = boot_lib.weights(seed, fuzz["contig"][:n], fuzz["start"][:n], np.arange(B))
    want = boot_lib.expected(fuzz["blocks"][:n], fuzz["counts"][:n], w, members)
    return got, want


def test_geometry():
    lib = boot_lib.load()
    assert lib.boot_emu_tile() == 32 and lib.boot_emu_reps() == 21 and lib.boot_emu_reps() * 24 <= 512


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("n", ["1", "T-1", "T", "T+1", "2T+1", "all"])
def test_tiles(fuzz, n, packed):
    T, R = boot_lib.load().boot_emu_tile(), boot_lib.load().boot_emu_reps()
    n = {"1": 1, "T-1": T - 1, "T": T, "T+1": T + 1, "2T+1": 2 * T + 1, "all": fuzz["batch"].n_regions}[n]
    got, want = run(fuzz, n, R + 1, packed=packed)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert want[0, :, boot_lib.SOLVED].any() and not got[:, :, boot_lib.ERRORS].any()


@pytest.mark.parametrize("B", ["1", "R-1", "R", "R+1", "2R+1"])
@pytest.mark.parametrize("grid", [1, 2])
def test_replicate_blocks(fuzz, B, grid):
    T, R = boot_lib.load().boot_emu_tile(), boot_lib.load().boot_emu_reps()
    B = {"1": 1, "R-1": R - 1, "R": R, "R+1": R + 1, "2R+1": 2 * R + 1}[B]
    got, want = run(fuzz, 2 * T + 1, B, grid=grid)
    assert np.array_equal(got, want) and want[0, :, :WORDS].any()


def test_scopes(fuzz):
    """scope 0, a label on every region, one on none, runs of regions (what an interval set gives on sorted regions), single regions at tile edges, and label 33 in
    the second mask word; the unsolved regions are under every label and count under none"""
    T, R = boot_lib.load().boot_emu_tile(), boot_lib.load().boot_emu_reps()
    n = fuzz["batch"].n_regions
    rng = np.random.default_rng(5)
    members = [np.ones(n, bool), np.zeros(n, bool)]
    for _ in range(3):
        m = np.zeros(n, bool)
        for s in rng.integers(0, n, 4):
            m[s:s + int(rng.integers(1, 3 * T))] = True
        members.append(m)
    edge = np.zeros(n, bool)
    edge[[T - 1, T, 2 * T - 1, n - 1]] = True
    members.append(edge)
    members += [np.zeros(n, bool)] * (33 - len(members)) + [rng.random(n) < 0.5]
    for m in members[2:]:
        m |= ~fuzz["counts"]
    members[1] = np.zeros(n, bool)
    got, want = run(fuzz, n, R + 1, members=members)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert np.array_equal(got[1], got[0]) and not got[2].any() and got[3].any() and got[6].any() and got[34].any() and not got[8:34].any()


def test_another_seed_gives_other_replicates(fuzz):
    """the same regions under another seed: other weights, the same rule"""
    T, R = boot_lib.load().boot_emu_tile(), boot_lib.load().boot_emu_reps()
    n = 2 * T + 1
    a, want = run(fuzz, n, R)
    b, _ = run(fuzz, n, R, seed=SEED + 1)
    assert np.array_equal(a, want) and not np.array_equal(a, b)
    assert np.array_equal(a[0, :, boot_lib.SOLVED] > 0, want[0, :, boot_lib.SOLVED] > 0)
