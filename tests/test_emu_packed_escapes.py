"""The widening of packed batches with escapes (avk_packed_escapes) on CPU lanes: dp_widen_packed_esc, dp_widen_packed_multi_esc and dp_esc_lower of
aardvark_amd/csrc/avk_devpack.inl, run through the emulator for every lane, against the numpy statement of what a packed batch with escapes stands for
(PackedBatch._wide_fields plus exclusive cumulative sums).  The lists are long here — up to every entry of the batch — and sit where a search, a running sum or
a block edge can be off by one: entry 0, the last entry, both sides of the 4096-element blocks of the narrow sums, dense runs, both count slots of a region with its
window, with the truly oversize regions first, in the middle and last.  No GPU involved.

What is NOT run here: avk_esc_scan_kernel (avk_devpack_host.inl), the one-workgroup kernel that checks a list and writes its exclusive sums in chunks of 1024 with a
carry.  It is a __global__ with LDS in the host file and the emulator does not build it; the sums it writes are made with numpy here, and its chunks, its carry and
its order check across a chunk edge are covered by tests/test_gpu_packed_escapes.py on the device.  Its per-entry check IS run here: dp_esc_entry_bad, a plain
function of avk_devpack.inl the kernel calls for every entry.

Bad lists.  The widening runs on a list before the error word of the scan is read, so a list that breaks the form must not be able to index outside an allocation:
 * dp_esc_lower(list, n, key) returns a p in [0, n] whatever the list holds (lo and hi stay inside [0, n]; no order is assumed for termination);
 * cnt_before[] / bytes_before[] have n + 1 entries, so [p] is inside; list[p] and the values at p are read only behind `p < n`;
 * every write goes to index i of the lane itself (i < n_regions / n_variants, i * k + j < n_regions * k) except the positions: dp_esc_positions writes
   w_pos[v] and reads rel_pos[v] only for v < n_variants, whatever the (possibly wrong) first call and count of the region are;
 * what comes out wrong — offsets, counts, lengths — is validated by dp_region / dp_variant like any wide batch's before anything is read through it.
test_a_bad_list_is_refused_and_writes_nothing_outside checks this argument: the same bad lists the GPU tests hand in run through the same functions here, with
guard words behind every output array (emu_lib.widen_packed_esc asserts them)."""
import functools

import numpy as np
import pytest

import emu_lib
import escapes_lib as el
from aardvark_amd.merge import PackedMultiBatch

SCALE = 0.01  # of the genome job: about 35,000 regions and 80,000 calls, nine blocks of the narrow sums over the regions and twenty over the calls
JOBS = ("genome", "indel_mix_v2", "merge")


@functools.lru_cache(maxsize=None)
def packed_job(job, where):
    """the escaped packed batch of a job (a PackedBatch, or a PackedMultiBatch for "merge") with its injected regions `where`"""
    if job == "merge":
        return PackedMultiBatch.from_multi(el.merge_job(where=where)[1], escapes=True)
    batch = el.genome_job(SCALE, where)[1] if job == "genome" else el.indel_mix_job(where=where)[1]
    return el.escaped(batch)[1]


def excl(x, total=False):
    out = np.concatenate([[0], np.cumsum(x.astype(np.int64))])
    return (out if total else out[:-1]).astype(np.uint64)


def device_sums(pb):
    """what the kernels in front of the widening hand it: the exclusive sums over the NARROW counts and allele lengths (avk_ps_*), and over the lists' values
    (avk_esc_scan_kernel), the latter with the total as entry n"""
    e = pb.escapes
    calls = excl(pb.in_cnt) if hasattr(pb, "n_inputs") else excl(pb.t_cnt.astype(np.int64) + pb.q_cnt)
    return calls, excl(pb.a0_len.astype(np.int64) + pb.a1_len), excl(e.esc_cnt, True), excl(e.esc_a0_len.astype(np.int64) + e.esc_a1_len, True)


def stands_for(pb):
    """the wide arrays `pb` stands for, by numpy"""
    n, multi = pb.n_regions, hasattr(pb, "n_inputs")
    per = pb.n_inputs if multi else 2
    length, cnt, rel, a0, a1 = pb._wide_fields()
    off = excl(cnt).astype(np.int64)
    per_region = cnt.reshape(n, per).sum(axis=1)
    start, aoff = pb.start.astype(np.int64), excl(a0 + a1).astype(np.int64)
    want = {"start": start, "end": start + length, "pos": np.repeat(start, per_region) + rel, "a0_off": aoff, "a1_off": aoff + a0, "a0_len": a0, "a1_len": a1,
            "type": pb.var_type_zyg & 15, "zyg": pb.var_type_zyg >> 4, "raw": pb.var_raw_space if pb.var_raw_space is not None else np.maximum(a0, a1)}
    if pb.contig_idx is not None:
        want["contig"] = pb.contig_idx
    if multi:
        want.update(in_off=off, in_cnt=cnt)
    else:
        want.update(t_off=off[0::2], q_off=off[1::2], t_cnt=cnt[0::2], q_cnt=cnt[1::2])
    return want


def differing(pb, expect_refused=0):
    got, refused = emu_lib.widen_packed_esc(pb, device_sums(pb))
    assert refused == expect_refused
    want = stands_for(pb)
    return [f for f in want if not np.array_equal(got[f].astype(np.int64), np.asarray(want[f]).astype(np.int64))]


def test_the_table_is_the_one_the_cases_are_made_from():
    for job in JOBS:
        assert tuple(el.promotion_table(packed_job(job, "last"))) == el.PROMOTIONS


@pytest.mark.parametrize("where", el.WHERE)
@pytest.mark.parametrize("job", JOBS)
def test_the_jobs_as_they_are(job, where):
    pb = packed_job(job, where)
    e = pb.escapes
    assert e.esc_region.size and e.esc_slot.size and e.esc_call.size
    if where == "first":  # the oversize values precede every ordinary entry
        assert int(e.esc_call[-1]) < pb.n_variants // 4 and int(e.esc_slot[-1]) < pb.n_regions // 4
    if where == "middle":
        assert pb.n_variants // 4 < int(e.esc_call[0]) and int(e.esc_call[-1]) < 3 * pb.n_variants // 4
    assert differing(pb) == []


@pytest.mark.parametrize("name", el.PROMOTIONS)
@pytest.mark.parametrize("where", el.WHERE)
@pytest.mark.parametrize("job", JOBS)
def test_promoted_lists(job, where, name):
    pb = packed_job(job, where)
    regions, slots, calls = el.promotion(pb, name)
    promoted = el.promote(pb, regions, slots, calls)
    e = promoted.escapes
    # the promoted batch stands for the batch it was made from, and its lists hold what was asked for
    before, after = stands_for(pb), stands_for(promoted)
    assert [f for f in before if not np.array_equal(before[f], after[f])] == []
    for lst, first, asked in ((e.esc_region, e.first_region, regions), (e.esc_slot, e.first_slot, slots), (e.esc_call, e.first_call, calls)):
        assert np.all(np.diff(lst.astype(np.int64)) > 0) and np.isin(np.asarray(asked, np.uint64) + np.uint64(first), lst).all()
    if name.startswith("draw_"):
        size = int(name.rsplit("_", 1)[1])
        per = promoted.n_inputs if job == "merge" else 2
        assert (e.esc_region.size, e.esc_slot.size, e.esc_call.size) == (min(size, pb.n_regions), min(size, pb.n_regions * per), min(size, pb.n_variants))
    if job == "genome":  # large enough for every index and size of the table, whatever becomes of the workload
        assert pb.n_regions > 8192 and pb.n_variants > 8192
        if name == "block_edges":
            assert all(np.isin(np.asarray(el.BLOCK_EDGES, np.uint64), lst).all() for lst in (e.esc_region, e.esc_slot, e.esc_call))
        if name == "every_second":
            assert e.esc_call.size > 10_000 and e.esc_region.size > 10_000 and e.esc_slot.size > 10_000
            for edge in (4096, 8192):  # listed entries on both sides of two block edges of the narrow sums
                assert (np.isin(np.asarray([edge - 2, edge, edge + 2], np.uint64), e.esc_call).all() and np.isin(np.asarray([edge - 2, edge], np.uint64), e.esc_region).all())
        if name.startswith("draw_"):
            assert e.esc_call.size == int(name.rsplit("_", 1)[1])
    assert differing(promoted) == []


@pytest.mark.parametrize("where", el.WHERE)
def test_slices_of_a_densely_promoted_batch(where):
    """split(7): first_region / first_slot / first_call are non-zero and a part's lists are a range of the whole's"""
    pb = packed_job("genome", where)
    tab = el.promotion_table(pb)
    regions, slots, calls = (np.union1d(a, b) for a, b in zip(tab["every_second"], tab["draw_1_of_3000"]))
    whole = el.promote(pb, regions, slots, calls)
    parts = whole.split(7)
    assert len(parts) == 7 and all(p.escapes.esc_call.size > 1024 and p.escapes.esc_slot.size > 1024 and p.escapes.esc_region.size > 1024 for p in parts)
    assert all(p.escapes.first_region > 0 and p.escapes.first_call > 0 and p.escapes.first_slot == 2 * p.escapes.first_region for p in parts[1:])
    assert all(p.escapes.esc_call.base is not None for p in parts)
    want, r0, v0 = stands_for(whole), 0, 0
    for p in parts:
        assert differing(p) == []
        got = stands_for(p)
        assert np.array_equal(got["end"], want["end"][r0:r0 + p.n_regions]) and np.array_equal(got["t_cnt"], want["t_cnt"][r0:r0 + p.n_regions])
        assert np.array_equal(got["pos"], want["pos"][v0:v0 + p.n_variants]) and np.array_equal(got["a1_len"], want["a1_len"][v0:v0 + p.n_variants])
        r0, v0 = r0 + p.n_regions, v0 + p.n_variants
    assert (r0, v0) == (whole.n_regions, whole.n_variants)


def test_esc_lower_is_searchsorted_left():
    rng = np.random.default_rng(4)
    lists = [np.zeros(0, np.uint64), np.array([7], np.uint64), np.array([3, 9], np.uint64), np.arange(10, 1034, dtype=np.uint64) * np.uint64(3),
             np.sort(rng.choice(1 << 20, 4097, replace=False)).astype(np.uint64) + np.uint64(5)]
    for lst in lists:
        keys = {0, 1, 1 << 40}  # below all, above all
        if lst.size:
            first, last = int(lst[0]), int(lst[-1])
            keys |= {first - 1, first, first + 1, last - 1, last, last + 1} | {int(x) for x in lst[:: max(1, lst.size // 97)]} | {int(x) + 1 for x in lst[:: max(1, lst.size // 89)]}
        for key in sorted(k for k in keys if k >= 0):
            assert emu_lib.esc_lower(lst, key) == int(np.searchsorted(lst, np.uint64(key), side="left")), (lst.size, key)


# ---- batches that break the form -----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def long_lists(job):
    """three lists of 2,048 entries each, with non-zero bases: for the compare form the second of two slices; the multi form, which has no slicing in Python, as a
    slice of a larger batch by shifted bases and indices (escapes_lib.rebased)"""
    pb = packed_job(job, "middle")
    if job == "merge":
        good = el.rebased(el.promote(pb, *el.exact_promotion(pb, (2048, 2048, 2048))))
        assert good.escapes.first_region > 0 and good.escapes.first_call > 0 and good.escapes.first_slot > 0
        return good
    part = pb.split(2)[1]
    assert part.escapes.first_region > 0 and part.escapes.first_call > 0 and part.escapes.first_slot > 0
    return el.promote(part, *el.exact_promotion(part, (2048, 2048, 2048)))


BAD_LISTS = [(job, which, how) for job in ("genome", "merge") for which in el.LISTS for how in el.SPOILS]


@pytest.mark.parametrize("job,which,how", BAD_LISTS)
def test_a_bad_list_is_refused_and_writes_nothing_outside(job, which, how):
    good = long_lists(job)
    assert all(getattr(good.escapes, f).size >= 2048 for f in ("esc_region", "esc_slot", "esc_call"))
    assert differing(good) == []
    bad = el.spoiled(good, which, how)
    got, refused = emu_lib.widen_packed_esc(bad, device_sums(bad))  # (the guard words behind every output array are asserted inside)
    assert refused == 1


@pytest.mark.parametrize("job", ("genome", "merge"))
def test_a_non_zero_narrow_field_under_a_listed_entry_is_refused(job):
    good = long_lists(job)
    for field in el.narrow_fields(good):
        bad = el.nonzero_under_a_listed_entry(good, field)
        assert int(np.count_nonzero(getattr(bad, field) != getattr(good, field))) == 1
        got, refused = emu_lib.widen_packed_esc(bad, device_sums(bad))
        assert refused == 1, field
