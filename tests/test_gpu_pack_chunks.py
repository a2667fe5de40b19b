"""The chunked route of a packed compare call (context option pack_chunks, csrc/avk_pack_chunks.h) on a real MI355X: with the per-region and per-call arrays
copied in N groups and the region pass run group by group under the copies, a call returns what it returns with pack_chunks = 0 — every output array and the tally
byte for byte, the same plan and the same regions in every segment of the work order (inside a bucket of the counting sort the order is that of the scatter's
atomics, from run to run) — for N in {2, 4, 8}, and one run per batch equals the oracle.

The batches have a few thousand regions (several 256-region blocks) and a few hundred to a few thousand calls; pack_chunk_floor = 0 lifts the 1 MiB floor so that
they chunk.  avk_last_region_launches says which route a call took: N + 1 launches of the region pass on the chunked route (the groups and the catch-all), 1 on the
old one, one more where calls were left to the host's edit distance.

Shapes (block = 256 regions; the cuts of the call arrays are n_variants * j / N):
  mix          a synthetic indel mix: regions whose calls straddle the cuts, 11.7 blocks
  empty_front  no call in the first three quarters of the regions: those blocks' call chunk is 0, their region ranges arrive later (taken by the range's own group)
  giant_first  region 0 holds most calls, its block's calls end in the last chunk: the early groups own no block
  zero_border  runs of regions without calls on both sides of every cut, and a region whose calls straddle the first cut
  one_block    200 regions;  odd_tail  1,111 regions (4.3 blocks);  two_blocks  300 regions: fewer blocks than groups for N = 4 and 8
Counts that overrun n_variants reach the catch-all launch (no group owns such a block) and are refused like on the old route."""
import numpy as np
import pytest

import oracle_lib
from aardvark_amd import CompactBatch, CompareConfig, PackedBatch, RegionBatch, ResultBatch, synth
from aardvark_amd.api import AardvarkAmdError

pytestmark = pytest.mark.gpu
GROUPS = (2, 4, 8)
RESULT_FIELDS = ("status", "ed_h1", "ed_h2", "n_optima", "type_present", "var_expected", "var_observed", "var_class", "var_zyg", "region_packed", "var_packed",
                 "bp_off", "bp_groups", "tally")
BASES = b"ACGT"


def snv_job(counts, seed, long_call_at=None):
    """(contigs, RegionBatch): region r has counts[r] = (truth calls, query calls), SNVs four bases apart from the window's start, the shared ones equal on both
    sides; long_call_at: that region gets one more call on both sides whose two alleles are 90 unlike bases — its edit distance is left to the host"""
    rng = np.random.default_rng(seed)
    widths = [max(40, 4 * max(t, q) + 12) + (100 if r == long_call_at else 0) for r, (t, q) in enumerate(counts)]
    starts = 100 + np.concatenate([[0], np.cumsum(np.asarray(widths) + 10)])
    ref = rng.integers(0, 4, int(starts[-1]) + 200).astype(np.uint8)
    contig = bytes(BASES[b] for b in ref)
    zygs = ("HomozygousAlternate", "HomozygousAlternate", "UnphasedHeterozygous", "PhasedHet01")
    regions = []
    for r, (t, q) in enumerate(counts):
        s = int(starts[r])

        def call(i, small):
            p = s + 4 + 4 * i
            alt = BASES[(ref[p] + 1 + (i + r) % 3) % 4]
            return (p, contig[p:p + 1], bytes([alt]), "Snv", zygs[(i + r) % 4] if small else "HomozygousAlternate")
        small = max(t, q) <= 3
        truth, query = [call(i, small) for i in range(t)], [call(i, small) for i in range(q)]
        if r == long_call_at:
            p = s + 4 + 4 * max(t, q) + 2
            alt = bytes(BASES[(ref[p + k] + 2) % 4] for k in range(90))
            long_call = (p, contig[p:p + 90], alt, "Indel", "HomozygousAlternate")
            truth.append(long_call), query.append(long_call)
        regions.append({"start": s, "end": s + widths[r], "truth": truth, "query": query})
    return [contig], RegionBatch.from_regions(regions)


def spread(n, where, seed):
    """counts for n regions: (1..2, 0..2) calls in the regions `where` selects, none elsewhere"""
    rng = np.random.default_rng(seed)
    return [((int(rng.integers(1, 3)), int(rng.integers(0, 3))) if where(r) else (0, 0)) for r in range(n)]


def zero_border_counts():
    n = 1536
    counts = spread(n, lambda r: True, 5)
    total = sum(t + q for t, q in counts)
    run = 0
    for r in range(n):  # 40 regions without calls around every quarter of the calls, and in front of the first cut a region with six calls that straddles it
        before = run
        run += sum(counts[r])
        for j in (1, 2, 3):
            if before <= total * j // 4 < run:
                for x in range(max(r - 20, 0), min(r + 20, n)):
                    counts[x] = (0, 0)
                if j == 1:
                    counts[r] = (3, 3)
    return counts


def mix_job():
    contig, batch = synth.config_indel_mix_v2(n_truth=3000, contig_len=1_200_000)
    return [contig], batch


JOBS = {
    "mix": mix_job,
    "empty_front": lambda: snv_job(spread(2048, lambda r: r >= 1536, 1), 11),
    "giant_first": lambda: snv_job([(100, 100)] + spread(1499, lambda r: r % 20 == 0, 2), 12),
    "zero_border": lambda: snv_job(zero_border_counts(), 13),
    "one_block": lambda: snv_job(spread(200, lambda r: True, 3), 14),
    "odd_tail": lambda: snv_job(spread(1111, lambda r: r % 3 != 1, 4), 15),
    "two_blocks": lambda: snv_job(spread(300, lambda r: True, 6), 16),
    "host_edit_distance": lambda: snv_job(spread(1300, lambda r: True, 7), 17, long_call_at=700),
}


@pytest.fixture(scope="module")
def ctx():
    import aardvark_amd
    c = aardvark_amd.Context(0)
    for opt in ("lane_min_regions", "lane_min_batch", "pack_chunk_floor"):
        c.set_option(opt, 0)
    yield c
    c.close()


@pytest.fixture(scope="module", params=sorted(JOBS))
def job(request, ctx, oracle):
    contigs, batch = JOBS[request.param]()
    pb = ctx.pinned_packed(PackedBatch.from_compact(CompactBatch.from_region_batch(batch)))
    want = oracle_lib.compare_batch(oracle, batch, contigs, threads=4)
    ctx.upload_reference(contigs)
    ctx.set_option("pack_chunks", 0)
    base, base_launches = solve(ctx, pb)
    return request.param, contigs, batch, pb, want, base, base_launches


def solve(ctx, pb):
    res = ctx.solve_packed(pb, res=ctx.pinned_results(pb, bp_groups=True, packed=True))
    return res, ctx.last_region_launches()


def same(a, b):
    return [f for f in RESULT_FIELDS if not np.array_equal(getattr(a, f), getattr(b, f))]


def test_the_old_route_equals_the_oracle(job):
    name, contigs, batch, pb, want, base, base_launches = job
    print(name, "regions", pb.n_regions, "calls", pb.n_variants, "region launches", base_launches)
    assert base_launches == (2 if name == "host_edit_distance" else 1)
    assert base.diff(want) == []


@pytest.mark.parametrize("groups", GROUPS)
def test_chunked_call_equals_the_old_route_byte_for_byte(ctx, job, groups):
    name, contigs, batch, pb, want, base, base_launches = job
    ctx.upload_reference(contigs)
    ctx.set_option("pack_chunks", groups)
    try:
        got, launches = solve(ctx, pb)
    finally:
        ctx.set_option("pack_chunks", 0)
    assert launches == groups + base_launches, "the call did not take the chunked route"  # N groups + the catch-all (+ the whole-range second round)
    assert same(got, base) == []
    if groups == 4:
        assert got.diff(want) == []


@pytest.mark.parametrize("groups", GROUPS)
def test_chunked_upload_plans_like_the_old_route(ctx, job, groups):
    name, contigs, batch, pb, want, base, base_launches = job
    ctx.upload_reference(contigs)
    plans = []
    for k in (0, groups):
        ctx.set_option("pack_chunks", k)
        try:
            rb = ctx.upload(pb)
        finally:
            ctx.set_option("pack_chunks", 0)
        try:
            assert ctx.last_region_launches() == (k + base_launches if k else base_launches)
            plans.append(ctx.work_order(rb))
        finally:
            rb.free()
    (order0, plan0), (order1, plan1) = plans
    assert plan0 == plan1
    n_fast = sum(regions for first, regions, head in plan0["fast"])
    edges = [0, plan0["class_c"], plan0["class_c"] + plan0["class_b"], pb.n_regions - n_fast] + [first + regions for first, regions, head in plan0["fast"] if regions]
    edges = sorted(set(edges + [pb.n_regions]))
    for lo, hi in zip(edges[:-1], edges[1:]):
        assert np.array_equal(np.sort(order0[lo:hi]), np.sort(order1[lo:hi])), (lo, hi)


def test_an_empty_batch(ctx):
    contigs, batch = snv_job(spread(10, lambda r: True, 8), 18)
    ctx.upload_reference(contigs)
    empty = ctx.pinned_packed(PackedBatch(**{f: np.zeros(0, dt) for f, dt in zip(PackedBatch.FIELDS, PackedBatch.DTYPES)}))
    assert empty.n_regions == 0 and empty.n_variants == 0
    out = []
    for k in (0, 4):
        ctx.set_option("pack_chunks", k)
        try:
            out.append(ctx.solve_packed(empty, res=ctx.pinned_results(empty, packed=True)))
        finally:
            ctx.set_option("pack_chunks", 0)
    assert np.array_equal(out[0].tally, out[1].tally) and int(out[1].tally.sum()) == 0


def test_escapes_submit_pageable_and_kernel_copies_keep_the_old_route(ctx):
    """everything the chunked route is not for runs launch for launch as with pack_chunks = 0: one launch of the region pass, the same results"""
    import escapes_lib as el
    contigs, batch = mix_job()
    ctx.upload_reference(contigs)
    loose = PackedBatch.from_compact(CompactBatch.from_region_batch(batch))
    pb = ctx.pinned_packed(loose)
    ctx.set_option("pack_chunks", 0)
    base, _ = solve(ctx, pb)
    contigs_e, batch_e = el.indel_mix_job()  # the same mix with oversize regions injected: its packed form lists escapes
    esc_pb = ctx.pinned_packed(el.escaped(batch_e)[1])
    assert esc_pb.c_escapes() is not None
    ctx.upload_reference(contigs_e)
    esc_base, esc_launches = solve(ctx, esc_pb)
    ctx.set_option("pack_chunks", 4)
    try:
        got, launches = solve(ctx, esc_pb)
    finally:
        ctx.set_option("pack_chunks", 0)
    assert launches == esc_launches == 1 and same(got, esc_base) == []
    ctx.upload_reference(contigs)
    ctx.set_option("pack_chunks", 4)
    try:
        got, launches = solve(ctx, pb)
        assert launches == 5 and same(got, base) == []  # (the ground: this batch does chunk)
        got = ctx.submit_packed(pb, res=ctx.pinned_results(pb, bp_groups=False, packed=True)).wait()  # a submitted batch: the staging slot
        assert ctx.last_region_launches() == 1
        assert np.array_equal(got.region_packed, base.region_packed) and np.array_equal(got.var_packed, base.var_packed) and np.array_equal(got.tally, base.tally)
        got = ctx.solve_packed(loose, res=ResultBatch(loose, sequences=False, group_metrics=False, bp_groups=True, packed=True))  # pageable arrays
        assert ctx.last_region_launches() == 1 and same(got, base) == []
        ctx.set_option("kernel_copies", 2)  # a context that copies by kernel
        try:
            got, launches = solve(ctx, pb)
        finally:
            ctx.set_option("kernel_copies", 1)
        assert launches == 1 and same(got, base) == []
        ctx.set_option("pack_chunks", 0)  # the old order of the copies with the side stream's steps queued early or late: one launch, the same bytes
        for early in (0, 1):
            ctx.set_option("pack_queue_early", early)
            try:
                got, launches = solve(ctx, pb)
            finally:
                ctx.set_option("pack_queue_early", 1)
            assert launches == 1 and same(got, base) == [], early
        ctx.set_option("pack_chunks", 4)
        ctx.set_option("pack_chunk_floor", 1 << 20)  # the floor: a batch this small keeps the old order
        try:
            got, launches = solve(ctx, pb)
        finally:
            ctx.set_option("pack_chunk_floor", 0)
        assert launches == 1 and same(got, base) == []
    finally:
        ctx.set_option("pack_chunks", 0)


def test_counts_that_overrun_the_calls_are_refused_on_both_routes(ctx):
    """no group owns a block whose calls end beyond n_variants: the catch-all launch runs it, dp_region sees the range, the batch is refused as before — and the
    context solves a good batch straight afterwards"""
    contigs, batch = snv_job(spread(1000, lambda r: True, 9), 19)
    ctx.upload_reference(contigs)
    good = ctx.pinned_packed(PackedBatch.from_compact(CompactBatch.from_region_batch(batch)))
    ctx.set_option("pack_chunks", 0)
    base, _ = solve(ctx, good)
    bad = ctx.pinned_packed(good)
    bad.t_cnt[400] += 7
    for k in (0, 4):
        ctx.set_option("pack_chunks", k)
        try:
            with pytest.raises(AardvarkAmdError):
                ctx.solve_packed(bad, res=ctx.pinned_results(bad, packed=True))
            got, launches = solve(ctx, good)
        finally:
            ctx.set_option("pack_chunks", 0)
        assert launches == (5 if k else 1) and same(got, base) == []
