"""Packed batches with escapes (avk_packed_escapes) on a real MI355X: a batch whose long alleles, long windows and dense sides are listed in the escape lists gives,
through every packed entry point, what the oracle gives for the same batch in the wide form — every region, every output array, statuses included — and is planned
exactly like the same batch handed in wide; a batch that lists nothing is untouched by the new entry points.

Long lists (the second half of this file).  escapes_lib.promote moves entries of a batch into its escape lists without changing the batch it stands for, so the
oracle's result of a job is the expected result of every promoted variant: lists of 1,023 to 2,049 entries and of more than 10,000 (avk_esc_scan_kernel works in
chunks of 1024 with a carry), listed entries at entry 0, at the last entry, on both sides of the 4096-element blocks of the narrow prefix sums, with the truly
oversize regions first, in the middle and last, through every route.  Every comparison is bit for bit, over all regions.

Refusals.  A list that is not ascending or leaves the batch, a missing array, and a listed entry whose narrow field is not 0 are AVK_E_ARG by contract
(include/aardvark_amd.h: avk_packed_escapes); each is handed in once per entry point, and the same context must solve the good batch straight afterwards.  The
widening kernels run on such a list before the scan's error word is read, so before any of them went to a GPU it was established that a bad list cannot index
outside an allocation: dp_esc_lower is bounded by n whatever the list holds; before[] has n + 1 entries; list[p] and its values are read behind p < n only; every
write goes to the lane's own index except the positions, and dp_esc_positions clips both its w_pos writes and its rel_pos reads by n_variants; the widened offsets,
counts and lengths are validated by dp_region / dp_variant like any wide batch's before anything is read through them.  tests/test_emu_packed_escapes.py runs the
same bad lists (escapes_lib.spoiled) through the same functions on the CPU with guard words behind every output array.  The merge form has no submit entry point
in the library: its refusals go through avk_merge_packed_esc alone; it has no slicing in Python either, so its batch gets the bases of a slice by shifting them and
the listed indices (escapes_lib.rebased)."""
import ctypes as C
import os

import numpy as np
import pytest

import escapes_lib as el
import oracle_lib
from aardvark_amd import CompactBatch, PackedBatch, RegionBatch, ResultBatch, synth
from aardvark_amd._abi import AvkPackedEscapes, PackedEscapes

pytestmark = pytest.mark.gpu
CPUS = min(os.cpu_count() or 1, 16)
ST_CAPACITY = 21
JOBS = {"genome": lambda: el.genome_job(scale=0.01), "indel_mix_v2": el.indel_mix_job}


@pytest.fixture(scope="module", params=sorted(JOBS))
def job(request, oracle):
    import aardvark_amd
    contigs, batch = JOBS[request.param]()
    cb, pb = el.escaped(batch)
    assert pb.c_escapes() is not None
    ctx = aardvark_amd.Context(0)
    ctx.set_option("lane_min_regions", 0)
    ctx.set_option("lane_min_batch", 0)
    ctx.upload_reference(contigs)
    want = oracle_lib.compare_batch(oracle, batch, contigs, threads=CPUS)
    yield ctx, contigs, batch, pb, want
    ctx.close()


def no_capacity(res):
    st = res.status if res.status is not None else (res.region_packed & np.uint64(0x7F)).astype(np.int32)
    return int((st == ST_CAPACITY).sum()) == 0


def test_the_wide_form_of_the_workload_has_no_capacity_failure_and_is_the_oracles(job):
    """the ground the other tests stand on: handed in wide, the injected regions are solved (no AVK_ST_CAPACITY) and equal the oracle's"""
    ctx, contigs, batch, pb, want = job
    got = ctx.solve_compare_regions(batch, aardvark_amd_config(), group_metrics=True)
    print("statuses of the wide call:", np.unique(got.status, return_counts=True))
    assert no_capacity(got)
    assert got.diff(want) == []


def aardvark_amd_config():
    from aardvark_amd import CompareConfig
    return CompareConfig(enable_sequences=False)


def test_compare_packed_with_escapes_equals_the_oracle_in_every_result_form(job):
    from aardvark_amd.api import group_metrics_from_compact
    ctx, contigs, batch, pb, want = job
    wide = ctx.solve_packed(pb, res=ResultBatch(pb, sequences=False, group_metrics=True))  # the wide arrays with the 13 x 22 blocks
    assert no_capacity(wide) and wide.diff(want) == []
    both = ctx.solve_packed(pb, res=ResultBatch(pb, sequences=False, group_metrics=False, packed=True))
    assert both.diff(want) == [] and both.expanded(ctx.lib, batch).diff(want) == []
    only = ctx.solve_packed(pb, res=ResultBatch(pb, sequences=False, group_metrics=False, packed="only"))
    assert np.array_equal(only.region_packed, both.region_packed) and np.array_equal(only.var_packed, both.var_packed)
    assert only.expanded(ctx.lib, batch).diff(want) == []
    for form in (True, "packed"):  # the compact BASEPAIR groups, and their packed form
        res = ctx.solve_packed(pb, res=ResultBatch(pb, sequences=False, group_metrics=False, bp_groups=form))
        assert res.diff(want) == []
        assert np.array_equal(group_metrics_from_compact(batch, res), want.group_metrics), form
    # ... and with the packer's other source route switched on or off (an escaped batch is widened either way)
    ctx.set_option("packed_source", 0)
    try:
        assert ctx.solve_packed(pb, res=ResultBatch(pb, sequences=False, group_metrics=True)).diff(want) == []
    finally:
        ctx.set_option("packed_source", 1)


def test_submit_and_wait_with_two_batches_in_flight(job):
    ctx, contigs, batch, pb, want = job
    parts = [ctx.pinned_packed(p) for p in pb.split(2)]
    assert len(parts) == 2 and parts[1].c_escapes() is not None
    tickets = [ctx.submit_packed(p, res=ctx.pinned_results(p, packed=True)) for p in parts]  # both in flight
    got = [tickets[1].wait(), tickets[0].wait()][::-1]
    assert ctx.last_compare_was_one_shot()
    for f in ("status", "ed_h1", "ed_h2", "n_optima", "type_present"):
        assert np.array_equal(np.concatenate([getattr(g, f) for g in got]), getattr(want, f)), f
    for f in ("var_expected", "var_observed", "var_class", "var_zyg"):
        assert np.array_equal(np.concatenate([getattr(g, f)[:p.n_variants] for g, p in zip(got, parts)]), getattr(want, f)[:batch.n_variants]), f
    assert np.array_equal(sum(g.tally.astype(np.uint64) for g in got), want.tally)
    assert all(no_capacity(g) for g in got)
    # pageable escape lists: solved at the submit, same results
    loose = pb.split(2)[1]
    t = ctx.submit_packed(loose, res=ResultBatch(loose, sequences=False, group_metrics=False, packed=True))
    assert np.array_equal(t.wait().region_packed, got[1].region_packed)


def test_upload_resident_download_and_the_plan_of_the_wide_form(job):
    ctx, contigs, batch, pb, want = job
    rb, rw = ctx.upload(pb), ctx.upload(batch)
    try:
        order_e, plan_e = ctx.work_order(rb)
        order_w, plan_w = ctx.work_order(rw)
        # the same regions to the same launches (inside a bucket of the counting sort the order is that of the scatter's atomics, from run to run)
        assert plan_e == plan_w and np.array_equal(np.sort(order_e), np.sort(order_w))
        for first, regions, head in plan_e["fast"]:
            assert np.array_equal(np.sort(order_e[first:first + regions]), np.sort(order_w[first:first + regions]))
        ctx.compare_resident(rb, aardvark_amd_config())
        got = ctx.download(rb, group_metrics=True, packed=True)
        tiers_e = ctx.last_tier_counts()
        ctx.compare_resident(rw, aardvark_amd_config())
        wide = ctx.download(rw, group_metrics=True, packed=True)
        assert tiers_e == ctx.last_tier_counts() and tiers_e[4] == 0
        assert got.diff(want) == [] and wide.diff(want) == [] and np.array_equal(got.region_packed, wide.region_packed) and np.array_equal(got.var_packed, wide.var_packed)
    finally:
        rb.free(), rw.free()


def test_a_batch_that_lists_nothing_is_untouched_by_the_new_entry_points(job):
    ctx = job[0]
    contig, batch = synth.config_indel_mix_v2(n_truth=3000, contig_len=1_200_000)
    ctx.upload_reference([contig])
    try:
        pb = PackedBatch.from_compact(CompactBatch.from_region_batch(batch))
        old = ctx.solve_packed(pb, res=ResultBatch(pb, sequences=False, group_metrics=True, packed=True))
        st, cfg = pb.c_struct(), aardvark_amd_config().c_struct()
        empty = PackedEscapes().c_struct()
        for esc in (None, C.byref(empty)):
            res = ResultBatch(pb, sequences=False, group_metrics=True, packed=True)
            ro = res.c_struct()
            ctx._check(ctx.lib.avk_compare_packed_esc(ctx.handle, C.byref(st), esc, C.byref(cfg), C.byref(ro)))
            assert res.diff(old) == [] and np.array_equal(res.region_packed, old.region_packed) and np.array_equal(res.var_packed, old.var_packed)
    finally:
        ctx.upload_reference(job[1])


def test_an_escape_list_out_of_order_is_an_argument_error(job):
    import aardvark_amd
    ctx, contigs, batch, pb, want = job
    bad = PackedBatch(escapes=PackedEscapes(**{f: getattr(pb.escapes, f).copy() for f in PackedEscapes.FIELDS}), **{f: getattr(pb, f) for f in PackedBatch.FIELDS})
    bad.escapes.esc_call[:2] = bad.escapes.esc_call[:2][::-1].copy()
    with pytest.raises(aardvark_amd.AardvarkAmdError):
        ctx.solve_packed(bad)
    assert ctx.solve_packed(pb, res=ResultBatch(pb, sequences=False, group_metrics=True)).diff(want) == []  # the context is fine


def merge_oracle(oracle, contigs, mb):
    """(status, classification, members) of a MultiBatch from the oracle's pairs (input i as truth, input j as query, i < j) and the library's host classification on top"""
    import aardvark_amd
    from aardvark_amd.merge import AvkMergeConfig
    k, n = mb.n_inputs, mb.n_regions
    pairs = [(i, j) for i in range(k) for j in range(i + 1, k)]
    io, ic = mb.in_off.reshape(n, k), mb.in_cnt.reshape(n, k)
    rep = lambda a: np.repeat(a, len(pairs))
    pb = RegionBatch(np.arange(n * len(pairs)), rep(mb.contig_idx), rep(mb.start), rep(mb.end), np.stack([io[:, i] for i, j in pairs], 1).reshape(-1),
                     np.stack([ic[:, i] for i, j in pairs], 1).reshape(-1), np.stack([io[:, j] for i, j in pairs], 1).reshape(-1), np.stack([ic[:, j] for i, j in pairs], 1).reshape(-1),
                     mb.var_pos, mb.var_type, mb.var_zyg, mb.var_raw_space, mb.a0_off, mb.a0_len, mb.a1_off, mb.a1_len, mb.allele_bytes)
    pst, pex = oracle_lib.optimize_pairs(oracle, pb, contigs, 50, threads=CPUS)
    unknown = np.array([bool((mb.var_zyg[int(io[m, 0]):int(io[m, 0]) + int(ic[m].sum())] == 0).any()) for m in range(n)], np.uint8)
    cfg = AvkMergeConfig(50, 1, 1, -1)
    st, cls, mem = np.zeros(n, np.int32), np.zeros(n, np.uint8), np.zeros(n, np.uint64)
    P = lambda a, t: np.ascontiguousarray(a).ctypes.data_as(C.POINTER(t))
    lib = aardvark_amd.load_library()
    pst, pex, cnt32 = np.ascontiguousarray(pst, np.int32), np.ascontiguousarray(pex, np.uint8), np.ascontiguousarray(mb.in_cnt, np.uint32)
    assert lib.avk_merge_classify(C.c_uint64(n), C.c_uint32(k), P(cnt32, C.c_uint32), P(unknown, C.c_uint8), P(pst, C.c_int32), P(pex, C.c_uint8), C.byref(cfg),
                                  P(st, C.c_int32), P(cls, C.c_uint8), P(mem, C.c_uint64)) == 0
    return st, cls, mem


def merge_is_the_wide_merge_and_the_oracles(got, wide, st, cls, mem):
    print("merge statuses:", np.unique(got.status, return_counts=True))
    assert int((got.status == ST_CAPACITY).sum()) == 0
    for name, a, b, c in (("status", got.status, wide.status, st), ("classification", got.classification, wide.classification, cls), ("members", got.members, wide.members, mem)):
        assert np.array_equal(a, b), name
        ok = c == a if name == "status" else (c == a) | (st != 0)  # (classification and members mean nothing for an unsolved region)
        assert bool(np.all(ok)), name


def test_merge_packed_with_escapes_equals_the_wide_merge_and_the_oracle(oracle):
    import aardvark_amd
    from aardvark_amd.merge import MergeConfig, PackedMultiBatch, merge_multi_batch
    contigs, mb = el.merge_job()
    pm = PackedMultiBatch.from_multi(mb, escapes=True)
    assert pm.c_escapes() is not None
    st, cls, mem = merge_oracle(oracle, contigs, mb)
    config = MergeConfig(majority_voting_enabled=True, no_conflict_enabled=True)
    ctx = aardvark_amd.Context(0)
    try:
        ctx.upload_reference(contigs)
        got = merge_multi_batch(ctx, pm, config)
        wide = merge_multi_batch(ctx, mb, config)
    finally:
        ctx.close()
    merge_is_the_wide_merge_and_the_oracles(got, wide, st, cls, mem)


# ---- long lists: lengths across the scan's chunks, every position, every route ----------------------------------------------------------------------------

PLACED_SCALE = 0.004  # of the genome job, for the promoted variants (at 0.01 this file took 4.5 times what it took before them; measured on one MI355X)


@pytest.fixture(scope="module", params=el.WHERE)
def placed(request, oracle):
    """(ctx, contigs, batch, pb, want, plain): the genome job with its injected regions last, first or in the middle, the oracle's result, and the result of the
    batch as the packer made it (one context alive at a time: each holds its workspaces)"""
    import aardvark_amd
    contigs, batch = el.genome_job(scale=PLACED_SCALE, where=request.param)
    cb, pb = el.escaped(batch)
    assert pb.n_regions > 8192 and pb.n_variants > 24_000  # two block edges inside every list, and room for 12,000 listed calls
    ctx = aardvark_amd.Context(0)
    try:
        ctx.set_option("lane_min_regions", 0)
        ctx.set_option("lane_min_batch", 0)
        ctx.upload_reference(contigs)
        want = oracle_lib.compare_batch(oracle, batch, contigs, threads=CPUS)
        plain = ctx.solve_packed(pb, res=ResultBatch(pb, sequences=False, group_metrics=False, packed=True))
        assert no_capacity(plain) and plain.diff(want) == []
        yield ctx, contigs, batch, pb, want, plain
    finally:
        ctx.close()


def same_as_the_oracle(ctx, promoted, want, plain):
    """all regions, bit for bit, no AVK_ST_CAPACITY; the packed words those of the unpromoted batch"""
    res = ctx.solve_packed(promoted, res=ResultBatch(promoted, sequences=False, group_metrics=False, packed=True))
    assert res.status.size == want.status.size == promoted.n_regions and no_capacity(res)
    assert res.diff(want) == []
    assert np.array_equal(res.region_packed, plain.region_packed) and np.array_equal(res.var_packed, plain.var_packed)
    return res


LENGTHS = {"1023": (1023,) * 3, "1024": (1024,) * 3, "1025": (1025,) * 3, "2048": (2048,) * 3, "2049": (2049,) * 3, "calls_12000": (1025, 1025, 12_000)}


@pytest.mark.parametrize("name", sorted(LENGTHS))
def test_list_lengths_across_the_chunks_of_the_scan(placed, name):
    ctx, contigs, batch, pb, want, plain = placed
    sizes = LENGTHS[name]
    promoted = el.promote(pb, *el.exact_promotion(pb, sizes))
    e = promoted.escapes
    assert (e.esc_region.size, e.esc_slot.size, e.esc_call.size) == sizes
    if name == "calls_12000":
        assert e.esc_call.size > 10_000
    same_as_the_oracle(ctx, promoted, want, plain)


IN_THE_MIDDLE = pytest.mark.parametrize("placed", ["middle"], indirect=True)  # what runs at one placement: the seeded draws (the CPU file runs them at all three), the refusals
BY_RULE = tuple(n for n in el.PROMOTIONS if not n.startswith("draw_"))
DRAWN = tuple(n for n in el.PROMOTIONS if n.startswith("draw_"))


@pytest.mark.parametrize("name", BY_RULE)
def test_listed_entries_at_every_position(placed, name):
    listed_entries_solve_like_the_oracle(placed, name)


@IN_THE_MIDDLE
@pytest.mark.parametrize("name", DRAWN)
def test_drawn_lists_of_1023_to_3000_entries(placed, name):
    assert len(DRAWN) == 12 and len(BY_RULE) + len(DRAWN) == len(el.PROMOTIONS)
    listed_entries_solve_like_the_oracle(placed, name)


def listed_entries_solve_like_the_oracle(placed, name):
    ctx, contigs, batch, pb, want, plain = placed
    promoted = el.promote(pb, *el.promotion(pb, name))
    e = promoted.escapes
    if name == "every_second":  # the dense case
        assert e.esc_call.size > 10_000
        for edge in (4096, 8192):
            assert np.isin(np.asarray([edge - 2, edge, edge + 2], np.uint64), e.esc_call).all() and np.isin(np.asarray([edge - 2, edge], np.uint64), e.esc_region).all()
    if name == "block_edges":
        assert all(np.isin(np.asarray(el.BLOCK_EDGES, np.uint64), lst).all() for lst in (e.esc_region, e.esc_slot, e.esc_call))
    if name.startswith("draw_"):
        assert e.esc_region.size == e.esc_slot.size == e.esc_call.size == int(name.rsplit("_", 1)[1])
    same_as_the_oracle(ctx, promoted, want, plain)


def dense(pb):
    out = el.promote(pb, *(np.union1d(a, b) for a, b in zip(el.promotion(pb, "every_second"), el.promotion(pb, "draw_1_of_3000"))))
    assert out.escapes.esc_call.size > 10_000 and out.escapes.esc_slot.size > 8192 and out.escapes.esc_region.size > 4096
    return out


def test_a_dense_batch_through_submit_and_wait_with_two_parts_in_flight(placed):
    ctx, contigs, batch, pb, want, plain = placed
    parts = [ctx.pinned_packed(p) for p in dense(pb).split(2)]
    assert len(parts) == 2 and all(min(p.escapes.esc_region.size, p.escapes.esc_slot.size, p.escapes.esc_call.size) > 1024 for p in parts)
    assert parts[1].escapes.first_region > 0 and parts[1].escapes.first_call > 0
    tickets = [ctx.submit_packed(p, res=ctx.pinned_results(p, packed=True)) for p in parts]  # both in flight
    got = [tickets[1].wait(), tickets[0].wait()][::-1]
    assert ctx.last_compare_was_one_shot()
    for f in ("status", "ed_h1", "ed_h2", "n_optima", "type_present", "region_packed"):
        assert np.array_equal(np.concatenate([getattr(g, f) for g in got]), getattr(plain if f == "region_packed" else want, f)), f
    for f in ("var_expected", "var_observed", "var_class", "var_zyg", "var_packed"):
        assert np.array_equal(np.concatenate([getattr(g, f)[:p.n_variants] for g, p in zip(got, parts)]), getattr(plain if f == "var_packed" else want, f)[:batch.n_variants]), f
    assert np.array_equal(sum(g.tally.astype(np.uint64) for g in got), want.tally)
    assert all(no_capacity(g) for g in got)


def test_a_dense_batch_resident_and_planned_like_the_wide_form(placed):
    ctx, contigs, batch, pb, want, plain = placed
    rb, rw = ctx.upload(dense(pb)), ctx.upload(batch)
    try:
        order_e, plan_e = ctx.work_order(rb)
        order_w, plan_w = ctx.work_order(rw)
        assert plan_e == plan_w and np.array_equal(np.sort(order_e), np.sort(order_w))
        for first, regions, head in plan_e["fast"]:
            assert np.array_equal(np.sort(order_e[first:first + regions]), np.sort(order_w[first:first + regions]))
        ctx.compare_resident(rb, aardvark_amd_config())
        got = ctx.download(rb, group_metrics=True, packed=True)
        assert no_capacity(got) and got.diff(want) == []
        assert np.array_equal(got.region_packed, plain.region_packed) and np.array_equal(got.var_packed, plain.var_packed)
    finally:
        rb.free(), rw.free()


def test_a_dense_batch_with_either_source_route(placed):
    ctx, contigs, batch, pb, want, plain = placed
    try:
        for value in (0, 1):
            ctx.set_option("packed_source", value)
            same_as_the_oracle(ctx, dense(pb), want, plain)
    finally:
        ctx.set_option("packed_source", 1)


@pytest.mark.parametrize("world", [2, 3])
def test_shards_of_a_dense_batch_solved_and_scattered_back(placed, world):
    from test_packed_escapes import shard_api, shard_as_python
    ctx, contigs, batch, pb, want, plain = placed
    lib = shard_api()
    whole_pb = dense(pb)
    st, esc = whole_pb.c_struct(), whole_pb.c_escapes()
    ids = np.ascontiguousarray(batch.region_id, np.uint64)
    whole = ResultBatch(whole_pb, sequences=False, group_metrics=False, packed=True)
    whole.region_packed[:] = np.uint64(0x7F)  # (no region may keep what it starts with)
    seen, tally = 0, np.zeros_like(want.tally, dtype=np.uint64)
    for rank in range(world):
        h = C.c_void_p()
        assert lib.avk_packed_shard_make_esc(C.byref(st), C.byref(esc), ids.ctypes.data_as(C.POINTER(C.c_uint64)), 0, rank, world, C.byref(h)) == 0
        try:
            shard, idx = shard_as_python(lib, h)
            assert shard.escapes.esc_call.size > 1024 and shard.escapes.esc_slot.size > 1024 and shard.escapes.esc_region.size > 1024
            res = ctx.solve_packed(shard, res=ResultBatch(shard, sequences=False, group_metrics=False, packed=True))
            assert no_capacity(res)
            a, b = res.c_struct(), whole.c_struct()
            assert lib.avk_packed_shard_scatter(h, C.byref(a), C.byref(b)) == 0
            seen += idx.size
            tally += res.tally.astype(np.uint64)  # (the sums over a batch's regions are the caller's to add up: the scatter moves per-region and per-call results)
        finally:
            lib.avk_packed_shard_free(h)
    assert seen == pb.n_regions
    assert np.array_equal(whole.region_packed[:pb.n_regions], plain.region_packed[:pb.n_regions]) and np.array_equal(whole.var_packed[:pb.n_variants], plain.var_packed[:pb.n_variants])
    assert np.array_equal(whole.status, want.status) and np.array_equal(whole.var_zyg[:pb.n_variants], want.var_zyg[:pb.n_variants])
    assert np.array_equal(tally, want.tally)
    assert [f for f in whole.expanded(ctx.lib, batch).diff(want) if f != "tally"] == []


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------------------

class LongPart:
    """the second half of the job (non-zero bases) with 2,048 entries in each list; ONE set of pinned arrays for it, into which a bad batch is written for its
    submit and the good one for the submit that follows; the checks that the context still solves the good batch, synchronously and through submit / wait"""

    def __init__(self, placed):
        self.ctx, contigs, batch, pb, self.want, self.plain = placed
        part = pb.split(2)[1]
        self.r0, self.v0 = part.escapes.first_region, part.escapes.first_call
        assert self.r0 > 0 and self.v0 > 0 and part.escapes.first_slot == 2 * self.r0
        self.good = el.promote(part, *el.exact_promotion(part, (2048, 2048, 2048)))
        self.pinned = self.ctx.pinned_packed(self.good)
        self.pinned_res = self.ctx.pinned_results(self.pinned, packed=True)

    def load(self, src):
        """src's arrays and lists into the pinned ones (a spoiled copy has the good batch's sizes and bases)"""
        for f in PackedBatch.FIELDS:
            if getattr(self.pinned, f) is not None:
                getattr(self.pinned, f)[...] = getattr(src, f)
        for f in PackedEscapes.FIELDS:
            getattr(self.pinned.escapes, f)[...] = getattr(src.escapes, f)
        e, g = self.pinned.escapes, src.escapes
        assert (e.first_region, e.first_slot, e.first_call) == (g.first_region, g.first_slot, g.first_call)
        return self.pinned

    def is_the_good_result(self, res):
        n, nv, r0, v0 = self.good.n_regions, self.good.n_variants, self.r0, self.v0
        assert no_capacity(res) and res.region_packed.size >= n
        assert np.array_equal(res.region_packed[:n], self.plain.region_packed[r0:r0 + n]) and np.array_equal(res.var_packed[:nv], self.plain.var_packed[v0:v0 + nv])
        for f in ("status", "ed_h1", "ed_h2", "n_optima", "type_present"):
            assert np.array_equal(getattr(res, f)[:n], getattr(self.want, f)[r0:r0 + n]), f

    def still_fine(self):
        self.is_the_good_result(self.ctx.solve_packed(self.good, res=ResultBatch(self.good, sequences=False, group_metrics=False, packed=True)))

    def still_fine_through_submit(self):
        """a staging slot that a refused submit kept would be missing here sooner or later (there are four)"""
        self.pinned_res.region_packed[:] = 0
        res = self.ctx.submit_packed(self.load(self.good), res=self.pinned_res).wait()
        assert self.ctx.last_compare_was_one_shot()
        self.is_the_good_result(res)

    def refused_by_both_entry_points(self, bad):
        import aardvark_amd
        with pytest.raises(aardvark_amd.AardvarkAmdError):
            self.ctx.solve_packed(bad)
        self.still_fine()
        with pytest.raises(aardvark_amd.AardvarkAmdError):
            self.ctx.submit_packed(self.load(bad), res=self.pinned_res)
        self.still_fine_through_submit()


@pytest.fixture(scope="module")
def long_part(placed):
    lp = LongPart(placed)
    lp.still_fine()
    lp.still_fine_through_submit()
    return lp


@IN_THE_MIDDLE
@pytest.mark.parametrize("how", el.SPOILS)
@pytest.mark.parametrize("which", sorted(el.LISTS))
def test_a_list_that_breaks_the_form_is_an_argument_error_and_the_context_goes_on(long_part, which, how):
    long_part.refused_by_both_entry_points(el.spoiled(long_part.good, which, how))


@IN_THE_MIDDLE
def test_a_missing_escape_array_is_an_argument_error(long_part):
    ctx, good = long_part.ctx, long_part.good
    cfg = aardvark_amd_config().c_struct()
    pinned = long_part.load(good)
    for name in PackedEscapes.FIELDS:
        for src, res in ((good, ResultBatch(good, sequences=False, group_metrics=False, packed=True)), (pinned, long_part.pinned_res)):
            st, esc, ro, ticket = src.c_struct(), src.escapes.c_struct(), res.c_struct(), C.c_void_p()
            setattr(esc, name, None)  # n_esc_* > 0 with a NULL array
            assert ctx.lib.avk_compare_packed_esc(ctx.handle, C.byref(st), C.byref(esc), C.byref(cfg), C.byref(ro)) == -1, name
            assert ctx.lib.avk_compare_packed_submit_esc(ctx.handle, C.byref(st), C.byref(esc), C.byref(cfg), C.byref(ro), C.byref(ticket)) == -1 and not ticket.value, name
    long_part.still_fine()
    long_part.still_fine_through_submit()


@IN_THE_MIDDLE
@pytest.mark.parametrize("field", ("len", "t_cnt", "q_cnt", "var_rel_pos", "a0_len", "a1_len"))
def test_a_listed_entry_whose_narrow_field_is_not_zero_is_an_argument_error(long_part, field):
    """the rule next to "MUST be written as 0" (include/aardvark_amd.h), all five narrow fields; tests/test_packed_escapes.py hands the same batches to
    avk_packed_shard_make_esc on the host"""
    good = long_part.good
    assert field in el.narrow_fields(good) and len(el.narrow_fields(good)) == 6
    bad = el.nonzero_under_a_listed_entry(good, field)
    assert int(np.count_nonzero(getattr(bad, field) != getattr(good, field))) == 1
    long_part.refused_by_both_entry_points(bad)


# ---- the merge form: long lists at every placement, every refusal ------------------------------------------------------------------------------------------------

class Merged:
    def __init__(self, oracle, where):
        import aardvark_amd
        from aardvark_amd.merge import MergeConfig, PackedMultiBatch, merge_multi_batch
        self.contigs, self.mb = el.merge_job(where=where)
        self.pm = PackedMultiBatch.from_multi(self.mb, escapes=True)
        assert self.pm.c_escapes() is not None and self.pm.n_regions * self.pm.n_inputs > 2049 and self.pm.n_variants > 8192
        self.config = MergeConfig(majority_voting_enabled=True, no_conflict_enabled=True)
        self.lib = aardvark_amd.load_library()
        self.ctx = aardvark_amd.Context(0)
        try:
            self.ctx.upload_reference(self.contigs)
            self.got = self.merge(self.pm)
            # the ground the promoted variants stand on: the wide merge and the oracle-derived classification
            merge_is_the_wide_merge_and_the_oracles(self.got, merge_multi_batch(self.ctx, self.mb, self.config), *merge_oracle(oracle, self.contigs, self.mb))
        except BaseException:
            self.ctx.close()
            raise

    def merge(self, batch):
        from aardvark_amd.merge import merge_multi_batch
        return merge_multi_batch(self.ctx, batch, self.config)

    def same_merge_and_counts(self, promoted):
        """every MultiRegion: status, classification, members; and the summary counters of avk_merge_counts_esc"""
        from aardvark_amd.merge import merge_counts
        res = self.merge(promoted)
        assert res.status.size == self.got.status.size == promoted.n_regions and int((res.status == ST_CAPACITY).sum()) == 0
        assert np.array_equal(res.status, self.got.status) and np.array_equal(res.classification, self.got.classification) and np.array_equal(res.members, self.got.members)
        assert np.array_equal(merge_counts(self.lib, promoted, self.got), merge_counts(self.lib, self.pm, self.got))


@pytest.fixture(scope="module", params=el.WHERE)
def merged(request, oracle):
    m = Merged(oracle, request.param)
    yield m
    m.ctx.close()


MERGE_LENGTHS = {"1025": (1025, 1025, 1025), "2049": (2049, 2049, 2049), "calls_9000": (1030, 1030, 9000)}


@pytest.mark.parametrize("name", sorted(MERGE_LENGTHS))
def test_merge_list_lengths_with_all_slots_of_one_multiregion(merged, name):
    pm, k, sizes = merged.pm, merged.pm.n_inputs, MERGE_LENGTHS[name]
    regions, slots, calls = el.exact_promotion(pm, sizes)
    m = int(regions[regions.size // 2])
    promoted = el.promote(pm, regions, np.union1d(slots, np.arange(m * k, (m + 1) * k)), calls)
    e = promoted.escapes
    assert e.esc_region.size == sizes[0] and sizes[1] <= e.esc_slot.size <= sizes[1] + k and e.esc_call.size == sizes[2]
    assert np.isin(np.arange(m * k, (m + 1) * k).astype(np.uint64) + np.uint64(e.first_slot), e.esc_slot).all() and m in regions
    merged.same_merge_and_counts(promoted)


@pytest.mark.parametrize("name", ("entry_0", "last_entry", "block_edges", "every_second", "every_second_odd", "everything"))
def test_merge_listed_entries_at_every_position(merged, name):
    promoted = el.promote(merged.pm, *el.promotion(merged.pm, name))
    if name == "block_edges":
        assert all(np.isin(np.asarray(el.BLOCK_EDGES, np.uint64), lst).all() for lst in (promoted.escapes.esc_slot, promoted.escapes.esc_call))
    merged.same_merge_and_counts(promoted)


MERGE_IN_THE_MIDDLE = pytest.mark.parametrize("merged", ["middle"], indirect=True)


@pytest.fixture(scope="module")
def merged_long(merged):
    """(merged, the batch with 2,048 entries in each list and the bases of a slice of a larger batch): avk_packed_escapes carries the bases for both forms"""
    good = el.rebased(el.promote(merged.pm, *el.exact_promotion(merged.pm, (2048, 2048, 2048))))
    assert good.escapes.first_region > 0 and good.escapes.first_slot > 0 and good.escapes.first_call > 0
    merged.same_merge_and_counts(good)
    return merged, good


@MERGE_IN_THE_MIDDLE
@pytest.mark.parametrize("how", el.SPOILS)
@pytest.mark.parametrize("which", sorted(el.LISTS))
def test_merge_a_list_that_breaks_the_form_is_an_argument_error_and_the_context_goes_on(merged_long, which, how):
    import aardvark_amd
    merged, good = merged_long
    with pytest.raises(aardvark_amd.AardvarkAmdError):
        merged.merge(el.spoiled(good, which, how))
    merged.same_merge_and_counts(good)


@MERGE_IN_THE_MIDDLE
@pytest.mark.parametrize("field", ("len", "in_cnt", "var_rel_pos", "a0_len", "a1_len"))
def test_merge_a_listed_entry_whose_narrow_field_is_not_zero_is_an_argument_error(merged_long, field):
    import aardvark_amd
    merged, good = merged_long
    assert field in el.narrow_fields(good) and len(el.narrow_fields(good)) == 5
    with pytest.raises(aardvark_amd.AardvarkAmdError):
        merged.merge(el.nonzero_under_a_listed_entry(good, field))
    merged.same_merge_and_counts(good)


@MERGE_IN_THE_MIDDLE
@pytest.mark.parametrize("name", PackedEscapes.FIELDS)
def test_merge_a_missing_escape_array_is_an_argument_error(merged_long, name):
    from aardvark_amd.merge import AvkMergeConfig, AvkPackedMultiBatch
    merged, good = merged_long
    ctx, n = merged.ctx, good.n_regions
    entry = ctx.lib.avk_merge_packed_esc
    entry.argtypes = [C.c_void_p, C.POINTER(AvkPackedMultiBatch), C.POINTER(AvkPackedEscapes), C.POINTER(AvkMergeConfig), C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)]
    st, cls, mem = np.zeros(n, np.int32), np.zeros(n, np.uint8), np.zeros(n, np.uint64)
    cb, esc, cfg = good.c_struct(), good.escapes.c_struct(), AvkMergeConfig(50, 1, 1, -1)
    setattr(esc, name, None)  # n_esc_* > 0 with a NULL array
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    assert entry(ctx.handle, C.byref(cb), C.byref(esc), C.byref(cfg), P(st, C.c_int32), P(cls, C.c_uint8), P(mem, C.c_uint64)) == -1  # AVK_E_ARG
    merged.same_merge_and_counts(good)


# ---- the two tools ----------------------------------------------------------------------------------------------------------------------------

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _files(folder):
    out = {}
    for base, _, names in os.walk(folder):
        for name in names:
            out[os.path.relpath(os.path.join(base, name), folder)] = open(os.path.join(base, name), "rb").read()
    return out


def _same_outputs(a, b, want):
    """every file of the two output folders byte for byte; the VCFs' one header line that quotes the command is compared without the command"""
    import gzip
    fa, fb = _files(a), _files(b)
    assert sorted(fa) == sorted(fb) and set(want) <= set(fa), (sorted(fa), sorted(fb))
    strip = lambda x: b"\n".join(l for l in x.split(b"\n") if not l.startswith(b"##aardvark_command"))
    for name in fa:
        if name.endswith(".vcf.gz"):
            assert strip(gzip.decompress(fa[name])) == strip(gzip.decompress(fb[name])), name
            assert len(gzip.decompress(fa[name])) == len(gzip.decompress(fb[name])), name  # (the two commands are written to be equally long, for the indexes' offsets)
        else:
            assert fa[name] == fb[name], name
        assert len(fa[name]) > 20, name


def test_compare_tool_shards_an_escaped_job_and_writes_the_files_of_the_wide_form(tmp_path):
    import subprocess
    p = el.write_feeder_case(tmp_path)
    tool = os.path.join(ROOT, "aardvark_amd", "bin", "aardvark_amd_compare")
    base = [tool, "-r", p["fa"], "-t", p["t"], "-q", p["q"], "-b", p["bed"], "--min-variant-gap", str(el.GAP), "-o"]
    wide = subprocess.run(base + [str(tmp_path / "w"), "--batch-form", "wide"], capture_output=True, text=True)
    assert wide.returncode == 0, wide.stderr
    two = subprocess.run(base + [str(tmp_path / "dd"), "--devices", "0,0", "-v"], capture_output=True, text=True)
    assert two.returncode == 0, two.stderr
    line = [l for l in two.stderr.splitlines() if l.startswith("Batch form:")]
    print(line)
    assert len(line) == 1 and "packed with escapes" in line[0] and "1 escaped counts" in line[0] and "2 contexts solve the job" in line[0] and " 0 escaped calls" not in line[0]
    _same_outputs(str(tmp_path / "w"), str(tmp_path / "dd"), ["summary.tsv", "truth.vcf.gz", "truth.vcf.gz.tbi", "query.vcf.gz", "query.vcf.gz.tbi"])
    solved = [l for l in wide.stderr.splitlines() if l.startswith("Solved:error")]
    assert solved and solved == [l for l in two.stderr.splitlines() if l.startswith("Solved:error")] and solved[0].rstrip().endswith(": 0")
    # one context, escapes: the line says so
    one = subprocess.run(base + [str(tmp_path / "o"), "-v"], capture_output=True, text=True)
    assert one.returncode == 0 and "packed with escapes" in one.stderr and "1 context solves the job" in one.stderr, one.stderr


def test_merge_tool_runs_an_escaped_job_on_every_listed_context(tmp_path):
    import subprocess
    p = el.write_feeder_case(tmp_path)
    tool = os.path.join(ROOT, "aardvark_amd", "bin", "aardvark_amd_merge")
    base = [tool, "-r", p["fa"]] + [x for v in p["vcfs"] for x in ("-i", v)] + ["-b", p["bed"], "--min-variant-gap", str(el.GAP), "--merge-strategy", "all", "--conflict-select", "1"]
    runs = {}
    for name, extra in (("ww", ["--batch-form", "wide"]), ("d", ["--devices", "0,0,0", "-v"])):
        os.makedirs(str(tmp_path / ("s" + name[0])))
        r = subprocess.run(base + ["--output-summary", str(tmp_path / ("s" + name[0]) / "merge_summary.tsv"), "-o", str(tmp_path / name)] + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        runs[name] = r.stderr
    line = [l for l in runs["d"].splitlines() if l.startswith("Batch form:")]
    print(line)
    assert len(line) == 1 and "packed with escapes" in line[0] and "3 contexts solve the job" in line[0]  # (before escapes: one context)
    assert "3 contexts, regions sharded by hash(region_id) % 3" in runs["d"]
    _same_outputs(str(tmp_path / "ww"), str(tmp_path / "d"), ["passing.vcf.gz", "passing.vcf.gz.tbi", "regions.bed.gz", "regions.bed.gz.tbi", "failed_regions.bed.gz"])
    _same_outputs(str(tmp_path / "sw"), str(tmp_path / "sd"), ["merge_summary.tsv"])
    solved = [l for l in runs["ww"].splitlines() if l.startswith("Solved:error")]
    assert solved and solved == [l for l in runs["d"].splitlines() if l.startswith("Solved:error")]
