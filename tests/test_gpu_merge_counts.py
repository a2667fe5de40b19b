"""The merge summary counters with the merge call (avk_merge_packed_counts; the count kernel of aardvark_amd/csrc/avk_mergecount.inl) on the GPU.

Every case compares the counters word for word with avk_merge_counts_esc on the same results, and status / classification / members with avk_merge_packed_esc on
the same context.  The jobs are the small merge job of tests/test_merge_shard.py (synth.config_genome_merge at scale 0.0008) with 2 to 9 call sets, its first
1, 255, 256 and 257 regions (the edges of the 256-lane classification launch; the count launch has 1,024 lanes for k slots a region), and the escaped job of
tests/escapes_lib.py."""
import ctypes as C
import functools
import gzip
import os
import subprocess

import numpy as np
import pytest

import aardvark_amd
import escapes_lib as el
import mergecount_emu_lib as mc
from aardvark_amd import synth
from aardvark_amd._abi import AvkPackedEscapes
from aardvark_amd.api import AardvarkAmdError
from aardvark_amd.merge import (AvkMergeConfig, AvkPackedMultiBatch, MergeConfig, MergeResult, PackedMultiBatch, counts_in_lds, counts_on_device, merge_counts, merge_counts_len,
                                merge_multi_batch, shard_packed_multi)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = MergeConfig(no_conflict_enabled=True, majority_voting_enabled=True, conflict_selection=1)


@functools.lru_cache(maxsize=None)
def job(k, regions=None):
    """(contigs, MultiBatch) of the small job with k call sets; regions: its first so many MultiRegions"""
    contigs, mb = synth.config_genome_merge(scale=0.0008, k=k, threads=4)
    if regions is not None:
        mb = el.reordered_multi(mb, np.arange(regions))
    return contigs, mb


@pytest.fixture(scope="module")
def ctx():
    c = aardvark_amd.Context(0)
    try:
        c.upload_reference(job(3)[0])  # (the contigs of the small job do not depend on k)
        yield c
    finally:
        c.close()


def same(a, b):
    return np.array_equal(a.status, b.status) and np.array_equal(a.classification, b.classification) and np.array_equal(a.members, b.members)


def counted(ctx, pm, cfg, on_device=True, start=None):
    """one call with counters, checked against the plain call and the host function -> (MergeResult, the batch's block)"""
    n = merge_counts_len(ctx.lib, pm.n_inputs)
    counts = np.zeros(n, np.uint64) if start is None else start.copy()
    got = merge_multi_batch(ctx, pm, cfg, counts=counts)
    assert counts_on_device(ctx) == on_device
    plain = merge_multi_batch(ctx, pm, cfg)
    assert same(got, plain)
    want = merge_counts(ctx.lib, pm, plain)
    block = counts if start is None else counts - start
    assert np.array_equal(block, want)
    # the calls of the solved regions, no more and no less
    _, cnt, _, _, _ = pm._wide_fields()
    assert int(block.sum()) == int(cnt.reshape(-1, pm.n_inputs)[plain.status == 0].sum())
    return plain, block


@pytest.mark.parametrize("regions", [1, 255, 256, 257, None])
def test_counts_at_the_edges_of_the_launches(ctx, regions):
    _, mb = job(3, regions)
    assert regions is None or mb.n_regions == regions
    res, block = counted(ctx, PackedMultiBatch.from_multi(mb), MergeConfig(majority_voting_enabled=True))
    if regions is None:
        assert mb.n_regions * 3 > 4 * 1024 and block.sum() > 0 and {1, 3} <= set(res.classification.tolist())


@pytest.mark.parametrize("which", ["2", "3", "last_in_lds", "first_beyond"])
def test_counts_on_either_side_of_the_lds_rule(ctx, which):
    """k = 2 and 3, the largest k whose block the count kernel keeps in LDS on this context and the next one (6 and 7 where a workgroup gets 160 KB)"""
    inside = [k for k in range(2, 9) if counts_in_lds(ctx, k)]
    assert inside == list(range(2, inside[-1] + 1)) and 3 <= inside[-1] < 8
    k = {"2": 2, "3": 3, "last_in_lds": inside[-1], "first_beyond": inside[-1] + 1}[which]
    assert counts_in_lds(ctx, k) == (which != "first_beyond")
    _, mb = job(k, None if k <= 3 else 1500)
    assert mb.n_regions * k > 2 * 1024  # more than one workgroup
    res, block = counted(ctx, PackedMultiBatch.from_multi(mb), ALL)
    assert len(set(res.classification[res.status == 0].tolist())) >= 3 and np.count_nonzero(block) > 8


def test_nine_inputs_are_counted_by_the_host_function(ctx):
    _, mb = job(9, 300)
    counted(ctx, PackedMultiBatch.from_multi(mb), ALL, on_device=False)
    # ... and so is any batch with device packing off
    _, mb = job(3, 300)
    ctx.set_option("device_pack", 0)
    try:
        counted(ctx, PackedMultiBatch.from_multi(mb), ALL, on_device=False)
    finally:
        ctx.set_option("device_pack", 1)
    counted(ctx, PackedMultiBatch.from_multi(mb), ALL, on_device=True)


@pytest.mark.parametrize("cfg", [MergeConfig(), MergeConfig(no_conflict_enabled=True), MergeConfig(majority_voting_enabled=True),
                                 MergeConfig(no_conflict_enabled=True, majority_voting_enabled=True), MergeConfig(conflict_selection=2), ALL],
                         ids=["exact", "no_conflict", "majority", "all", "select_2", "all_select_1"])
def test_counts_under_every_strategy(ctx, cfg):
    _, mb = job(3)
    res, _ = counted(ctx, PackedMultiBatch.from_multi(mb), cfg)
    if cfg.conflict_selection is not None:
        assert 4 in res.classification.tolist()


def test_a_region_with_an_unknown_zygosity_is_not_counted(ctx):
    _, mb = job(3, 400)
    pm = PackedMultiBatch.from_multi(mb)
    r = int(np.flatnonzero(pm.in_cnt.reshape(-1, 3).sum(axis=1) >= 3)[5])
    v = int(pm.in_cnt[:3 * r].astype(np.int64).sum())
    before, _ = counted(ctx, pm, ALL)
    assert before.status[r] == 0
    pm.var_type_zyg = pm.var_type_zyg.copy()
    pm.var_type_zyg[v] &= 15  # zygosity 0: Unknown
    after, block = counted(ctx, pm, ALL)
    assert after.status[r] != 0 and (after.status == 0).sum() == (before.status == 0).sum() - 1


def test_an_escaped_slot_of_more_than_255_calls(ctx):
    contigs, mb = el.merge_job()
    pm = PackedMultiBatch.from_multi(mb, escapes=True)
    _, cnt, _, _, _ = pm._wide_fields()
    long_slots = pm.escapes.esc_slot[pm.escapes.esc_cnt > 255].astype(np.int64)
    assert long_slots.size >= 1 and pm.c_escapes() is not None
    res, block = counted(ctx, pm, MergeConfig(majority_voting_enabled=True, no_conflict_enabled=True))
    assert all(res.status[s // 3] == 0 for s in long_slots)  # the dense region is solved: its 260 calls are among the counters


def test_counts_are_added_and_the_device_block_is_cleared_between_calls(ctx):
    _, mb = job(3, 700)
    pm = PackedMultiBatch.from_multi(mb)
    n = merge_counts_len(ctx.lib, 3)
    start = np.arange(n, dtype=np.uint64) * np.uint64(7) + np.uint64(2 ** 33)
    _, block = counted(ctx, pm, ALL, start=start)
    # two calls in a row into one array: twice the block
    twice = np.zeros(n, np.uint64)
    merge_multi_batch(ctx, pm, ALL, counts=twice)
    merge_multi_batch(ctx, pm, ALL, counts=twice)
    assert np.array_equal(twice, block * np.uint64(2))
    # ... and a smaller batch behind a larger one sees nothing of it
    _, small = job(3, 1)
    counted(ctx, PackedMultiBatch.from_multi(small), ALL)


@pytest.mark.parametrize("world", [2, 3])
def test_the_shards_counters_add_up_to_the_jobs(ctx, world):
    _, mb = job(3)
    pm = PackedMultiBatch.from_multi(mb)
    _, whole = counted(ctx, pm, ALL)
    total = np.zeros_like(whole)
    for rank in range(world):
        shard, idx = shard_packed_multi(ctx.lib, pm, mb.region_id, rank, world)
        assert 0 < idx.size < mb.n_regions
        merge_multi_batch(ctx, shard, ALL, counts=total)
        assert counts_on_device(ctx)
    assert np.array_equal(total, whole)


def raw_call(ctx, pm, cfg, counts):
    """avk_merge_packed_counts itself (counts may be None: a NULL pointer)"""
    n = pm.n_regions
    c = AvkMergeConfig(cfg.max_branch_factor, int(cfg.no_conflict_enabled), int(cfg.majority_voting_enabled), -1 if cfg.conflict_selection is None else int(cfg.conflict_selection))
    st, cl, mem = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint64)
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    f = ctx.lib.avk_merge_packed_counts
    f.argtypes = [C.c_void_p, C.POINTER(AvkPackedMultiBatch), C.POINTER(AvkPackedEscapes), C.POINTER(AvkMergeConfig), C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_uint64),
                  C.POINTER(C.c_uint64)]
    cb, esc = pm.c_struct(), pm.c_escapes()
    rc = f(ctx.handle, C.byref(cb), C.byref(esc) if esc is not None else None, C.byref(c), P(st, C.c_int32), P(cl, C.c_uint8), P(mem, C.c_uint64),
           None if counts is None else P(counts, C.c_uint64))
    return rc, MergeResult(st[:n], cl[:n], mem[:n], pm.n_inputs)


def test_without_counts_it_is_the_plain_call(ctx):
    _, mb = job(3, 700)
    pm = PackedMultiBatch.from_multi(mb)
    rc, got = raw_call(ctx, pm, ALL, None)
    assert rc == 0 and same(got, merge_multi_batch(ctx, pm, ALL))
    contigs, emb = el.merge_job()
    epm = PackedMultiBatch.from_multi(emb, escapes=True)
    rc, got = raw_call(ctx, epm, ALL, None)
    assert rc == 0 and same(got, merge_multi_batch(ctx, epm, ALL))


def test_refusals_leave_counts_untouched_and_the_context_goes_on(ctx):
    _, mb = job(3, 700)
    pm = PackedMultiBatch.from_multi(mb)
    n = merge_counts_len(ctx.lib, 3)
    start = np.arange(n, dtype=np.uint64) + np.uint64(5)
    # a type nibble of 12
    bad = PackedMultiBatch.from_multi(mb)
    bad.var_type_zyg = bad.var_type_zyg.copy()
    v = bad.n_variants // 2
    bad.var_type_zyg[v] = (bad.var_type_zyg[v] & 0xF0) | 12
    counts = start.copy()
    rc, _ = raw_call(ctx, bad, ALL, counts)
    assert rc == -1 and np.array_equal(counts, start)  # AVK_E_ARG
    with pytest.raises(AardvarkAmdError):
        merge_multi_batch(ctx, bad, ALL, counts=counts)
    assert np.array_equal(counts, start)
    counted(ctx, pm, ALL, start=start)
    # ... the same on the host route
    ctx.set_option("device_pack", 0)
    try:
        rc, _ = raw_call(ctx, bad, ALL, counts)
        assert rc == -1 and np.array_equal(counts, start)
    finally:
        ctx.set_option("device_pack", 1)
    # more call sets than the dense block exists for: refused before anything is queued
    eleven = mc.packed_batch(11, [0] * 11, [])
    counts = np.full(8, 3, np.uint64)
    rc, _ = raw_call(ctx, eleven, ALL, counts)
    assert rc == -1 and counts.tolist() == [3] * 8
    counted(ctx, pm, ALL)


def merge_cli():
    return os.path.join(ROOT, "aardvark_amd", "bin", "aardvark_amd_merge")


def test_the_tool_writes_the_same_files_with_either_summary_route(tmp_path):
    """aardvark_amd_merge --summary-counts device against host, on one context (two batches, both workers) and on --devices 0,0: the summary byte for byte, the
    other outputs equal; -v says which route counted"""
    from test_merge_outputs import write_case
    p, _ = write_case(tmp_path, 1500, 600_000)
    runs = {}
    for name, extra in (("one_device", ["--summary-counts", "device", "--batch-regions", "400", "-v"]), ("one_host", ["--summary-counts", "host", "--batch-regions", "400", "-v"]),
                        ("one_default", []), ("two_device", ["--devices", "0,0", "--summary-counts", "device", "-v"]), ("two_host", ["--devices", "0,0", "--summary-counts", "host", "-v"])):
        out, summary = str(tmp_path / ("out_" + name)), str(tmp_path / (name + ".csv"))
        cmd = [merge_cli(), "-r", p["fa"]] + [x for v in p["vcfs"] for x in ("-i", v)] + ["-b", p["bed"], "-o", out, "--output-summary", summary, "--merge-strategy", "all",
                                                                                           "--conflict-select", "1"] + extra
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        runs[name] = (out, summary, r.stderr)
    assert "--summary-counts device" in runs["one_device"][2] and "0 by the host function" in runs["one_device"][2] and "counted by kernel" in runs["one_device"][2]
    assert "region by region on the host" in runs["one_host"][2]
    assert "--summary-counts device; 2 batches counted by kernel" in runs["two_device"][2]
    assert "--summary-counts host; 0 batches counted by kernel with the merge call, 2 by the host function" in runs["two_host"][2]
    strip = lambda x: b"\n".join(l for l in x.split(b"\n") if not l.startswith(b"##aardvark_command"))
    for other in ("one_device", "one_default", "two_device", "two_host"):
        for name in ("passing.vcf.gz", "regions.bed.gz", "failed_regions.bed.gz"):
            x, y = (gzip.open(os.path.join(runs[n][0], name), "rb").read() for n in ("one_host", other))
            assert strip(x) == strip(y), (other, name)
        assert open(runs["one_host"][1], "rb").read() == open(runs[other][1], "rb").read() != b"", other
        solved = [l for l in runs["one_host"][2].splitlines() if l.startswith("Solved:error")]
        assert solved and solved == [l for l in runs[other][2].splitlines() if l.startswith("Solved:error")]
    r = subprocess.run([merge_cli(), "-r", p["fa"], "-i", p["vcfs"][0], "-o", str(tmp_path / "x"), "--summary-counts", "gpu"], capture_output=True, text=True)
    assert r.returncode == 78
