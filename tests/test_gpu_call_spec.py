"""What a call wants — metric blocks, BASEPAIR groups, the upload's streams, a strata job, a label fix — travels by argument (CallSpec, avk_host.hip), never through
the context: the options a caller set are the same after every form of call, after a call that failed, and between a submit and its wait.

The batch and the labels are those of tests/test_gpu_label_compact.py (SNVs and indels, some unsolved regions; random interval labels); the starved-workspace
context is its capacity-retry one.  Every comparison is exact: statuses and the 286 tally sums against the oracle, every result array against a plain packed
call on the same context, label sums against sums of the oracle's per-region blocks.
"""
import ctypes as C
import os

import numpy as np
import pytest

import escapes_lib
import oracle_lib
import scenarios
from aardvark_amd import CompactBatch, CompareConfig, PackedBatch, ResultBatch
from aardvark_amd._abi import TALLY_LEN, AvkCompareConfig, AvkPackedEscapes
from test_gpu_label_compact import WORDS, agrees, interval_labels, oracle_sums

pytestmark = pytest.mark.gpu
CPUS = min(os.cpu_count() or 1, 16)
N_LABELS = 9
P = C.POINTER


def new_results(pb):
    return ResultBatch(pb, sequences=False, group_metrics=False)


def three_strata(ctx):
    """label 0: every region of contig 0; label 1: nothing; label 2: the first 2,000 bases"""
    return ctx.upload_strata(3, 1, np.array([0, 1, 1, 2], np.uint64), np.array([0, 0], np.uint32), np.array([100_000_000, 2_000], np.uint32))


@pytest.fixture(scope="module")
def job(oracle):
    """one context with DEFAULT options, one call set, the oracle's results and label sums: shared, never changed"""
    import aardvark_amd
    from aardvark_amd import synth
    contigs, base = scenarios.indel_small(1500)
    _, bad = scenarios.invalid_regions()
    batch = synth.concat_batches([base, bad])
    want = oracle_lib.compare_batch(oracle, batch, contigs, threads=CPUS)
    ctx = aardvark_amd.Context(0)
    ctx.upload_reference(contigs)
    cb = CompactBatch.from_region_batch(batch)
    pb = PackedBatch.from_compact(cb)
    off, idx, lists = interval_labels(batch, N_LABELS, 77, max(len(c) for c in contigs))
    yield dict(ctx=ctx, contigs=contigs, batch=batch, cb=cb, pb=pb, want=want, labels=(N_LABELS, off, idx), sums=oracle_sums(want, lists, N_LABELS))
    ctx.close()


def options_are_the_defaults(job, ctx=None):
    """the two resident checks: emit_group_metrics is still 1 (the downloaded blocks are the oracle's), emit_bp_groups still 0 (the compact label sums refuse)"""
    import aardvark_amd
    ctx, pb, want = ctx or job["ctx"], job["pb"], job["want"]
    rb = ctx.upload(pb)
    try:
        ctx.compare_resident(rb)
        res = ctx.download(rb, group_metrics=True)
        assert agrees(res, want)
        assert np.array_equal(np.asarray(res.group_metrics).reshape(-1), np.asarray(want.group_metrics).reshape(-1))
        with pytest.raises(aardvark_amd.AardvarkAmdError, match="error -4.*no BASEPAIR groups on the device"):
            ctx.label_tallies_compact(rb, *job["labels"])
    finally:
        rb.free()


def test_the_options_survive_every_form(job):
    ctx, batch, cb, pb, want = job["ctx"], job["batch"], job["cb"], job["pb"], job["want"]
    esc = escapes_lib.promote(pb, regions=[1, 7, pb.n_regions - 1], slots=[0, 5, 2 * pb.n_regions - 2], calls=[0, 3, pb.n_variants - 1])
    strata = three_strata(ctx)
    try:
        assert agrees(ctx.solve_compare_regions(batch, CompareConfig(enable_sequences=False), group_metrics=False), want)
        assert agrees(ctx.solve_compact(cb), want)
        plain = ctx.solve_packed(pb, res=new_results(pb))
        assert agrees(plain, want)
        assert ctx.solve_packed(esc, res=new_results(esc)).diff(plain) == []
        got = ctx.solve_packed(pb, res=new_results(pb), labels=job["labels"])  # forces the groups on
        assert got.diff(plain) == [] and np.array_equal(got.label_tallies, job["sums"])
        got = ctx.solve_packed(pb, res=new_results(pb), strata=strata)  # and so does this one
        assert got.diff(plain) == [] and not got.label_tallies[1].any()
        assert np.array_equal(got.label_tallies[0, :WORDS], want.tally[:WORDS])  # (a label on every region of the one contig)
    finally:
        strata.free()
    options_are_the_defaults(job)


def test_the_options_survive_a_failing_call(job):
    import aardvark_amd
    ctx, pb = job["ctx"], job["pb"]
    lib = ctx.lib
    st, cfg, res = pb.c_struct(), AvkCompareConfig(50, 0, 0), new_results(pb)
    ro = res.c_struct()
    esc = AvkPackedEscapes()
    esc.n_esc_regions = 2  # counts, and no arrays
    assert lib.avk_compare_packed_esc(ctx.handle, C.byref(st), C.byref(esc), C.byref(cfg), C.byref(ro)) == -1
    assert "escape arrays missing" in lib.avk_last_error(ctx.handle).decode()
    options_are_the_defaults(job)
    bare = aardvark_amd.Context(0)  # no reference: the labels form fails at its upload, the groups already forced on
    try:
        with pytest.raises(aardvark_amd.AardvarkAmdError, match="error -4"):
            bare.solve_packed(pb, res=new_results(pb), labels=job["labels"])
        bare.upload_reference(job["contigs"])
        options_are_the_defaults(job, bare)
    finally:
        bare.close()


def submit_then_solve_then_wait(ctx, pb, labels):
    """a submit with labels, a synchronous packed call without groups and without metric blocks before its wait -> (waited results, synchronous results)"""
    pinned = ctx.pinned_packed(pb)
    n_labels, off, idx = labels
    poff, pidx = ctx.host_array(off.shape, np.uint64), ctx.host_array(idx.shape, np.uint32)
    poff[...], pidx[...] = off, idx
    ticket = ctx.submit_packed(pinned, res=ctx.pinned_results(pinned), labels=(n_labels, poff, pidx))
    between = ctx.solve_packed(pb, res=new_results(pb))
    return ticket.wait(), between


def test_a_synchronous_call_between_submit_and_wait(job):
    ctx, pb, want = job["ctx"], job["pb"], job["want"]
    plain = ctx.solve_packed(pb, res=new_results(pb))
    waited, between = submit_then_solve_then_wait(ctx, pb, job["labels"])
    assert agrees(plain, want) and between.diff(plain) == [] and waited.diff(plain) == []
    assert np.array_equal(waited.label_tallies, job["sums"])
    options_are_the_defaults(job)


def test_the_same_with_a_capacity_retry_in_the_wait(oracle):
    """the starved-workspace context: the wait repairs regions that came back AVK_ST_CAPACITY and adds their blocks to the label's sums (LabelFix)"""
    import aardvark_amd
    ctx = aardvark_amd.Context(0)
    try:
        for k, v in dict(lds_bytes_per_wave=2048, lds2_bytes_per_wave=0, ws_bytes_per_wave=0, big_ws_bytes=4096).items():
            ctx.set_option(k, v)
        contigs, batch = scenarios.fuzz_regions(341, 400, max_vars=9, max_len=12)
        ctx.upload_reference(contigs)
        want = oracle_lib.compare_batch(oracle, batch, contigs, threads=CPUS)
        pb = PackedBatch.from_compact(CompactBatch.from_region_batch(batch))
        n = batch.n_regions
        ctx.set_option("capacity_retry", 0)
        assert (ctx.solve_packed(pb, res=new_results(pb)).status == 21).any()  # some regions do exhaust the last tier on the first try
        ctx.set_option("capacity_retry", 1)
        plain = ctx.solve_packed(pb, res=new_results(pb))
        waited, between = submit_then_solve_then_wait(ctx, pb, (1, np.arange(n + 1, dtype=np.uint64), np.zeros(n, np.uint32)))
        assert agrees(plain, want) and between.diff(plain) == [] and waited.diff(plain) == []
        assert np.array_equal(waited.label_tallies[0, :WORDS], want.tally[:WORDS])
    finally:
        ctx.close()


def test_the_strata_forms_upload_counts_its_lists_once(oracle):
    """a batch with escapes and one call whose edit distance is left to the host: the packer's region passes run twice inside the upload, the lists are counted
    in the first round only — the one-call form's sums are the resident form's"""
    import aardvark_amd
    from test_gpu_pack_chunks import snv_job, spread
    contigs, batch = snv_job(spread(400, lambda r: True, 7), 17, long_call_at=200)
    pb = PackedBatch.from_compact(CompactBatch.from_region_batch(batch))
    src = escapes_lib.promote(pb, regions=[1, 7, pb.n_regions - 1], slots=[0, 5, 2 * pb.n_regions - 2], calls=[0, 3, pb.n_variants - 1])
    assert not src.escapes.empty()
    want = oracle_lib.compare_batch(oracle, batch, contigs, threads=4)
    ctx = aardvark_amd.Context(0)
    try:
        for opt in ("lane_min_regions", "lane_min_batch"):
            ctx.set_option(opt, 0)
        ctx.upload_reference(contigs)
        strata = three_strata(ctx)
        got = ctx.solve_packed(src, res=new_results(src), strata=strata)
        assert ctx.last_region_launches() == 2, "the passes did not run a second round"
        assert agrees(got, want)
        ctx.set_option("emit_bp_groups", 1)
        rb = ctx.upload(src)
        ctx.compare_resident(rb)
        sums = ctx.label_tallies_strata(rb, strata)
        rb.free()
        strata.free()
        assert np.array_equal(got.label_tallies, sums)
        assert np.array_equal(sums[0, :WORDS], want.tally[:WORDS]) and not sums[1].any() and 0 < sums[2].sum() < sums[0].sum()
    finally:
        ctx.close()
