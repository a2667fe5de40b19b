"""The stratified tally of a batch in flight reads a region's labels from the strata pass's bit masks (lb_region_labels_mask, aardvark_amd/csrc/avk_labels.inl),
without a GPU: the lane function of the gfx950 kernel runs on the CPU (tests/emu/label_mask_emu.cpp), launch block by launch block, against lb_region_labels over
the lists sx_fill_region makes from the SAME masks — the route of the one-call form, pinned against the oracle's blocks by tests/test_label_compact.py.  The
accumulators are compared word for word.

Label counts 6, 32, 33, 71, 72 and 143 with blocks of 28 and of 71 labels (avk_label_block with 64 KB and with 160 KB of LDS): a block's edge falls on a word's
first bit (0, 32, 64 ..), on its last bit (a block that ends at 32: 32 labels, or block [28, 56) ending at bit 23 and [56, 84) starting at bit 24 — and hi = 71,
142: bits 6 and 13), in its middle, and one block lies wholly inside one word ([33, 40)).

Also here: the refusal of avk_compare_packed_submit_strata that needs no device, and the Python declaration against the header."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import aardvark_amd
import label_emu_lib
import label_mask_emu_lib as lm
import oracle_lib
import scenarios
import strata_emu_lib as sx
from aardvark_amd import _abi, feeder, synth
from aardvark_amd._abi import AvkCompareConfig

WORDS = label_emu_lib.WORDS
LABEL_COUNTS = [6, 32, 33, 71, 72, 143]
BLOCKS = [28, 71]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def launches(n_labels, block):
    """the blocks [lo, hi) of the label kernel's launches, plus the block inside one word where the labels reach it"""
    out = [(lo, min(n_labels, lo + block)) for lo in range(0, n_labels, block)]
    if n_labels >= 40:
        out.append((33, 40))
    return out


@pytest.fixture(scope="module")
def fuzz():
    """the fuzzed regions of tests/test_label_compact.py (with the invalid ones: unsolved) and the oracle's results, as the device view: shared, never changed"""
    contigs, batch = scenarios.fuzz_regions(341, 400, max_vars=9, max_len=12)
    _, bad = scenarios.invalid_regions()
    batch = synth.concat_batches([batch, bad])
    res = oracle_lib.compare_batch(oracle_lib.load(), batch, contigs, threads=8)
    solved = np.asarray(res.status) == 0
    assert solved.sum() > 300 and (~solved).sum() >= 1
    # two solved regions are shown as AVK_ST_CAPACITY (words and groups in place): like the unsolved ones they must add nothing, whatever their masks say
    starved = [int(r) for r in np.flatnonzero(solved & np.asarray(res.group_metrics).reshape(batch.n_regions, -1).any(axis=1))[10:12]]
    view, keep = label_emu_lib.device_view(batch, res, starved=starved)
    counts = solved.copy()
    counts[starved] = False
    return dict(view=view, keep=keep, n=batch.n_regions, counts=counts)


def random_masks(n, n_labels, seed, counts):
    """word-major masks: a third of the regions without any label, one region under every label, the unsolved regions under all of them; no bit beyond n_labels"""
    rng = np.random.default_rng(seed)
    nw = lm.n_words(n_labels)
    mask = rng.integers(0, 2 ** 32, (nw, n), dtype=np.uint64).astype(np.uint32)
    mask &= rng.integers(0, 2 ** 32, (nw, n), dtype=np.uint64).astype(np.uint32)  # a quarter of the bits
    mask[:, rng.random(n) < 0.33] = 0
    mask[:, n // 2] = 0xFFFFFFFF
    mask[:, ~counts] = 0xFFFFFFFF
    if n_labels & 31:
        mask[nw - 1] &= np.uint32((1 << (n_labels & 31)) - 1)
    return mask


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("n_labels", LABEL_COUNTS)
def test_random_masks_give_the_accumulators_of_their_lists(fuzz, n_labels, block):
    view, n = fuzz["view"], fuzz["n"]
    assert block <= lm.load().label_mask_emu_block_max()
    mask = random_masks(n, n_labels, 7 * n_labels + block, fuzz["counts"])
    off, idx = lm.lists_of_masks(mask, n, n_labels)
    assert np.array_equal(lm.masks_of_lists(n, n_labels, off, idx), mask) and len(idx) and int(idx.max()) == n_labels - 1
    some = 0
    for lo, hi in launches(n_labels, block):
        got, want = lm.block_from_masks(view, mask, lo, hi), lm.block_from_lists(view, off, idx, lo, hi)
        assert np.array_equal(got, want), (lo, hi, np.flatnonzero(got != want)[:8])
        some += int(want.any())
    assert some == len(launches(n_labels, block))


@pytest.mark.parametrize("n_labels", [33, 143])
def test_zero_masks_and_unsolved_regions_add_nothing(fuzz, n_labels):
    """regions without a bit add nothing; regions that do not count (status != 0, AVK_ST_CAPACITY) add nothing under every label; one region that counts, alone
    under one label, adds its block to that label's sums and to no other word"""
    view, n, counts = fuzz["view"], fuzz["n"], fuzz["counts"]
    nw = lm.n_words(n_labels)
    blocks = label_emu_lib.blocks(view, n)
    for lo, hi in launches(n_labels, 28):
        assert not lm.block_from_masks(view, np.zeros((nw, n), np.uint32), lo, hi).any()
        only_unsolved = np.zeros((nw, n), np.uint32)
        only_unsolved[:, ~counts] = 0xFFFFFFFF
        assert not lm.block_from_masks(view, only_unsolved, lo, hi).any()
        r = int(np.flatnonzero(counts & blocks.any(axis=1))[3])
        for l in (lo, hi - 1):
            one = np.zeros((nw, n), np.uint32)
            one[l >> 5, r] = 1 << (l & 31)
            for outside in (lo - 1, hi):  # the neighbours just outside the block must not count
                if 0 <= outside < n_labels:
                    one[outside >> 5, r] |= np.uint32(1 << (outside & 31))
            acc = lm.block_from_masks(view, one, lo, hi).reshape(hi - lo, WORDS)
            assert np.array_equal(acc[l - lo], blocks[r].astype(np.uint64)) and not np.delete(acc, l - lo, axis=0).any()


@pytest.fixture(scope="module")
def shared_job():
    """the job of strata_emu_lib — every edge of the containment rule plus 600 random regions on three contigs — on a reference its calls fit, with the oracle's
    results as the device view: shared, never changed"""
    batch = sx.batch_of(sx.edge_regions() + sx.random_regions(600))
    contigs = [b"A" * (sx.SPAN + 2_000)] * 3
    res = oracle_lib.compare_batch(oracle_lib.load(), batch, contigs, threads=8)
    assert (np.asarray(res.status) == 0).sum() > 400
    view, keep = label_emu_lib.device_view(batch, res)
    return dict(batch=batch, view=view, keep=keep)


@pytest.mark.parametrize("n_labels", LABEL_COUNTS)
def test_shared_job_masks_of_the_rule(shared_job, tmp_path, n_labels):
    """the masks the containment rule gives for 6 .. 143 label sets (sx_mask_word, through the lists of tests/emu/strata_emu.cpp) tallied both ways, blocks of 28
    and of 71"""
    from test_feeder import write_text
    folder = str(tmp_path)
    genome = feeder.Genome(sx.write_genome(folder, write_text))
    strat = feeder.Stratifications(sx.write_sets(folder, write_text, n_many=500, extra_labels=n_labels - 6))
    assert len(strat.labels) == n_labels
    batch, view, n = shared_job["batch"], shared_job["view"], shared_job["batch"].n_regions
    sview, _keep = sx.view_of(batch, strat.export(genome))
    rule_off, rule_idx = sx.lists(sview, n)
    strat.close()
    mask = lm.masks_of_lists(n, n_labels, rule_off, rule_idx)
    off, idx = lm.lists_of_masks(mask, n, n_labels)
    assert np.array_equal(off, rule_off) and np.array_equal(idx, rule_idx)  # (ascending within a region: the masks lose nothing)
    assert (np.diff(off.astype(np.int64)) == 0).any() and np.bincount(idx, minlength=n_labels)[0] > 500
    for block in BLOCKS:
        total = np.zeros(n_labels * WORDS, np.uint64)
        for k, (lo, hi) in enumerate(launches(n_labels, block)):
            got, want = lm.block_from_masks(view, mask, lo, hi), lm.block_from_lists(view, off, idx, lo, hi)
            assert np.array_equal(got, want), (block, lo, hi)
            if k < -(-n_labels // block):  # (the launches proper, not the extra block inside one word)
                total[lo * WORDS:hi * WORDS] += got
        # ... and together the launches give the sums label_emu's flush gives for the whole set
        assert np.array_equal(total, label_emu_lib.tally(view, n_labels, off, idx, block)[:, :WORDS].reshape(-1)) and total.any()


# ---- the entry point: what needs no device --------------------------------------------------------------------------------------------------------------
def test_submit_strata_with_a_null_context_is_an_argument_error():
    lib = aardvark_amd.load_library()
    contigs, batch = scenarios.fuzz_regions(2, 12, max_vars=2)
    pb = aardvark_amd.PackedBatch.from_compact(aardvark_amd.CompactBatch.from_region_batch(batch))
    st, cfg = pb.c_struct(), AvkCompareConfig(50, 0, 0)
    res = aardvark_amd.ResultBatch(pb, sequences=False, group_metrics=False)
    ro = res.c_struct()
    sums = np.zeros((4, _abi.TALLY_LEN), np.uint64)
    ticket = C.c_void_p()
    rc = lib.avk_compare_packed_submit_strata(None, C.byref(st), None, None, C.byref(cfg), C.byref(ro), sums.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(ticket))
    assert rc == -1 and not ticket.value and not sums.any()


def test_python_declaration_agrees_with_the_header():
    """the prototype in include/aardvark_amd.h, parameter by parameter, against the argtypes aardvark_amd/_abi.py declares"""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "aardvark_amd.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+avk_compare_packed_submit_strata\s*\(([^)]*)\)\s*;", src)
    assert m, "the header does not declare avk_compare_packed_submit_strata"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    types = [re.sub(r"\s*\b[a-z_]+$", "", p).replace("const ", "").strip() for p in params]
    assert types == ["avk_ctx *", "avk_packed_batch *", "avk_packed_escapes *", "avk_strata *", "avk_compare_config *", "avk_result_batch *", "uint64_t *", "avk_ticket **"]
    lib = aardvark_amd.load_library()
    fn = lib.avk_compare_packed_submit_strata
    P, vp = C.POINTER, C.c_void_p
    assert fn.restype is C.c_int
    assert list(fn.argtypes) == [vp, P(_abi.AvkPackedBatch), P(_abi.AvkPackedEscapes), vp, P(_abi.AvkCompareConfig), P(_abi.AvkResultBatch), P(C.c_uint64), P(vp)]
    import inspect
    assert "strata" in inspect.signature(aardvark_amd.Context.submit_packed).parameters
