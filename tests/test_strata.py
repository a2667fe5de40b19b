"""The containment rule of the device-made label lists (aardvark_amd/csrc/avk_strata.inl) on the CPU, against the host's lists (avf_strat_batch_labels, itself
pinned by the reference's example_stratification fixture in tests/test_feeder.py), the export of the sets (avf_strat_export) and the refusals of
avk_strata_upload that need no device.  Every comparison is exact."""
import ctypes as C
import os

import numpy as np
import pytest

import strata_emu_lib as sx
from aardvark_amd import CompactBatch, PackedBatch, feeder
from test_feeder import write_text


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    folder = str(tmp_path_factory.mktemp("strata"))
    genome = feeder.Genome(sx.write_genome(folder, write_text))
    strat = feeder.Stratifications(sx.write_sets(folder, write_text, extra_labels=34))
    exported = strat.export(genome)
    yield dict(genome=genome, strat=strat, exported=exported)
    strat.close()


def host_lists(sets, batch):
    return sets["strat"].batch_labels(sets["genome"], batch)


def same_lists(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_export_layout(sets):
    n_labels, n_contigs, tree_off, start, end_max = sets["exported"]
    strat = sets["strat"]
    assert n_labels == len(strat.labels) == 40 and n_contigs == 3 and strat.labels[:6] == ["a_every", "b_none", "c_nested", "d_many", "e_touch", "f_mid"]
    assert tree_off[0] == 0 and (np.diff(tree_off.astype(np.int64)) >= 0).all() and int(tree_off[-1]) == len(start) == len(end_max)
    sizes = np.diff(tree_off.astype(np.int64)).reshape(n_labels, n_contigs)
    # trees with 0, 1 and several thousand intervals; chrZ and the interval that starts at 2^32 or beyond are left out, the e == 0 interval is kept
    assert sizes[3].tolist() == [4000, 1, 0] and sizes[1].tolist() == [2, 0, 0] and sizes[4].tolist() == [0, 1, 0]
    for l in range(n_labels):
        for c in range(n_contigs):
            lo, hi = int(tree_off[l * n_contigs + c]), int(tree_off[l * n_contigs + c + 1])
            assert hi - lo == strat.n_intervals(l, sx.NAMES[c]) or (l, c) == (1, 1)
            assert (np.diff(start[lo:hi].astype(np.int64)) >= 0).all() and (np.diff(end_max[lo:hi].astype(np.int64)) >= 0).all()
    lo = int(tree_off[1 * n_contigs + 0])
    assert start[lo] == 0 and end_max[lo] == 0  # "chrA 0 0": an exclusive end of 0 contains nothing


def test_export_round_trips_on_random_points(sets):
    """queries on the exported arrays equal avf_strat_containments"""
    strat, exported = sets["strat"], sets["exported"]
    view, _keep = sx.view_of(sx.batch_of([]), exported)
    lib = sx.load()
    rng = np.random.default_rng(21)
    n_labels = exported[0]
    hits = 0
    for _ in range(3000):
        c = int(rng.integers(0, 3))
        first = int(rng.integers(0, sx.SPAN + 5_000))
        last = first + int(rng.integers(0, 400 if rng.random() < 0.8 else 40_000))
        want = strat.containments(sx.NAMES[c], first, last)
        got = [l for l in range(n_labels) if lib.strata_emu_contains(C.byref(view), l, c, first, last)]
        assert got == want, (c, first, last)
        hits += len(got)
    assert hits > 6000
    # the edges of the one interval of e_touch, and beyond the last interval of a tree
    lo, hi = sx.TOUCH
    for first, last in ((lo, hi - 1), (lo - 1, hi - 1), (lo, hi), (hi - 1, hi - 1), (hi, hi), (0, 0), (2 ** 32 - 2, 2 ** 32 - 2)):
        assert [l for l in range(n_labels) if lib.strata_emu_contains(C.byref(view), l, 1, first, last)] == strat.containments("chrB", first, last)


@pytest.mark.parametrize("packed_source", [False, True], ids=["wide", "packed"])
def test_lists_equal_the_hosts(sets, packed_source):
    """every edge of the rule plus random regions on three contigs, through the wide arrays and through the packed source"""
    batch = sx.batch_of(sx.edge_regions() + sx.random_regions(3000))
    want = host_lists(sets, batch)
    view, _keep = sx.view_of(batch, sets["exported"], packed_source=packed_source)
    got = sx.lists(view, batch.n_regions)
    assert same_lists(got, want)
    off, idx = want
    per_label = np.bincount(idx, minlength=40)
    assert per_label[1] == 0 and (per_label[[0, 2, 3, 4, 5]] > 0).all() and per_label[6:].sum() > 0
    # (a_every holds every region that has a span at all; the region without calls has no label)
    assert per_label[0] == batch.n_regions - sum(1 for r in range(batch.n_regions) if batch.t_cnt[r] + batch.q_cnt[r] == 0)


def test_more_labels_than_a_staging_chunk(tmp_path):
    """300 labels: the kernels' label loop runs a second time (256 labels are staged at a time), mask words 8 and 9 come from it, the last one 12 labels wide"""
    folder = str(tmp_path)
    genome = feeder.Genome(sx.write_genome(folder, write_text))
    strat = feeder.Stratifications(sx.write_sets(folder, write_text, n_many=500, extra_labels=294))
    assert len(strat.labels) == 300
    exported = strat.export(genome)
    batch = sx.batch_of(sx.edge_regions() + sx.random_regions(700, seed=4))
    want = strat.batch_labels(genome, batch)
    assert (np.bincount(want[1], minlength=300)[256:] > 0).all()
    for packed_source in (False, True):
        view, _keep = sx.view_of(batch, exported, packed_source=packed_source)
        assert same_lists(sx.lists(view, batch.n_regions), want)
    strat.close()


def test_edges_one_by_one(sets):
    """the edge regions alone, in the order edge_regions() lists them: which of them label e_touch (4), c_nested (2), d_many (3) contain"""
    regions = sx.edge_regions()
    batch = sx.batch_of(regions)
    order = sorted(range(len(regions)), key=lambda k: (regions[k]["contig"], regions[k]["start"]))
    view, _keep = sx.view_of(batch, sets["exported"])
    off, idx = sx.lists(view, batch.n_regions)
    assert same_lists((off, idx), host_lists(sets, batch))
    labels = {k: idx[int(off[at]):int(off[at + 1])].tolist() for at, k in enumerate(order)}
    touch = [4 in labels[k] for k in range(11)]
    assert touch == [True, False, True, False, True, False, True, True, True, False, False]
    assert labels[10] == [] and 2 in labels[11] and 2 not in labels[12]
    assert 3 not in labels[13] and 2 in labels[13] and 2 in labels[14]


def test_escaped_batch(sets):
    """a window over 65,535 bases and an allele over 255 bases as a side's last call: the batch needs escapes, the device sees it widened"""
    batch = sx.batch_of(sx.escape_regions() + sx.random_regions(200, seed=5))
    pb = PackedBatch.from_compact(CompactBatch.from_region_batch(batch), escapes=True)
    assert len(pb.escapes.esc_region) >= 1 and len(pb.escapes.esc_call) >= 2
    widened = pb.to_compact().widen()  # what dp_widen_packed_esc leaves on the device
    assert np.array_equal(widened.a0_len, batch.a0_len) and np.array_equal(widened.var_pos, batch.var_pos)
    want = host_lists(sets, batch)
    view, _keep = sx.view_of(widened, sets["exported"])
    got = sx.lists(view, batch.n_regions)
    assert same_lists(got, want)
    off, idx = got
    # the two regions around the end of f_mid's chrB interval (60,000): the long allele alone decides
    r_in = [r for r in range(batch.n_regions) if int(batch.start[r]) == 30_000 and int(batch.contig_idx[r]) == 1][0]
    r_out = [r for r in range(batch.n_regions) if int(batch.start[r]) == 59_000 and int(batch.contig_idx[r]) == 1][0]
    assert 5 in idx[int(off[r_in]):int(off[r_in + 1])] and 5 not in idx[int(off[r_out]):int(off[r_out + 1])]


def test_regions_outside_the_batch_or_the_sets_have_no_labels(sets):
    batch = sx.batch_of(sx.random_regions(60, seed=2))
    n_labels, n_contigs, tree_off, start, end_max = sets["exported"]
    view, keep = sx.view_of(batch, sets["exported"])
    full = sx.lists(view, batch.n_regions)
    assert full[0][-1] > 0
    keep["contig_idx"][:] = 3  # a contig the sets do not know
    assert sx.lists(view, batch.n_regions)[0][-1] == 0
    view, keep = sx.view_of(batch, sets["exported"])
    keep["t_off"][5] = batch.n_variants + 1  # a call range outside the batch
    keep["q_cnt"][7] = batch.n_variants + 1
    off, idx = sx.lists(view, batch.n_regions)
    assert off[6] == off[5] and off[8] == off[7]
    others = [r for r in range(batch.n_regions) if r not in (5, 7)]
    assert all(np.array_equal(idx[int(off[r]):int(off[r + 1])], full[1][int(full[0][r]):int(full[0][r + 1])]) for r in others)


def upload_refusal(lib, n_labels, n_contigs, tree_off, start, end_max):
    u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    lib.avk_strata_upload.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, u64p, u32p, u32p, C.POINTER(C.c_void_p)]
    lib.avk_last_error.restype = C.c_char_p
    lib.avk_last_error.argtypes = [C.c_void_p]
    h = C.c_void_p()
    p = lambda a, t: None if a is None else a.ctypes.data_as(t)
    rc = lib.avk_strata_upload(None, n_labels, n_contigs, p(tree_off, u64p), p(start, u32p), p(end_max, u32p), C.byref(h))
    assert not h.value
    return rc, lib.avk_last_error(None).decode()


def test_upload_refusals_need_no_device():
    """the array checks come before anything else: AVK_E_ARG with their text even without a context; sound arrays get as far as the missing context"""
    import aardvark_amd
    lib = aardvark_amd.load_library()
    off = np.array([0, 2, 2, 5], np.uint64)
    start, end = np.array([1, 5, 3, 3, 9], np.uint32), np.array([4, 8, 6, 6, 12], np.uint32)
    assert upload_refusal(lib, 1, 3, off, start, end) == (-1, "strata: context missing")
    assert upload_refusal(lib, 0, 3, None, None, None) == (-1, "strata: context missing")  # an empty set is sound
    rc, text = upload_refusal(lib, 1, 3, np.array([0, 2, 1, 5], np.uint64), start, end)
    assert rc == -1 and "tree_off must not decrease" in text
    bad = start.copy()
    bad[1] = 0
    rc, text = upload_refusal(lib, 1, 3, off, bad, end)
    assert rc == -1 and "starts of tree 0 are not sorted" in text
    bad = end.copy()
    bad[4] = 5
    rc, text = upload_refusal(lib, 1, 3, off, start, bad)
    assert rc == -1 and "end_max of tree 2 decreases" in text
    # (a new tree may start below the last one's values)
    assert upload_refusal(lib, 3, 1, off, start, end)[1] == "strata: context missing"
    for s, e in ((None, end), (start, None), (None, None)):
        rc, text = upload_refusal(lib, 1, 3, off, s, e)
        assert rc == -1 and "start / end_max missing" in text
    rc, text = upload_refusal(lib, 1, 3, None, start, end)
    assert rc == -1 and "tree_off missing" in text
