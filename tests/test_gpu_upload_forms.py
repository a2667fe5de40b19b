"""Every form a batch reaches the upload in (csrc/avk_upload.inl, csrc/avk_upload_forms.h) on a real MI355X, on one small job per path.

The compare job: 513 regions (three 256-region blocks, the last one with a single region) on two contigs; call counts of 0 to 3 per side (the lane classes), 6 to 12
and 20 to 100 per side (class C by their size) and of 5 or 6 in all (class B, the wave-per-region kernels; class_c_below is 0); one truth call whose two alleles
are 90 unlike bases, which dp_variant leaves to the host's edit distance (n_pending = 1: the region passes run twice).  It goes in wide, compact, packed from pinned and from pageable arrays,
packed through submit / wait (the staging slot) and packed with pack_chunks on: every form returns the oracle's results, and the resident forms the same plan and the
same regions in every segment of the work order (inside a bucket of the counting sort the order is that of the scatter's atomics, from run to run).  The same job
with three more regions — a window of 70,000 bases, a side of 256 calls, an allele of 300 bases: one entry in each escape list — goes in packed with escapes and
equals its own wide form.

The merge job: three call sets over 257 MultiRegions, wide and packed, equal each other and the oracle.

The writers' side-stream clearing starts at 262,144 regions: a packed batch of single-SNV regions one region below and one at that size, one after the other on one
context (the pooled counters and partials the second one clears were the first one's), each equal to the wide form of the same batch."""
import numpy as np
import pytest

import oracle_lib
from aardvark_amd import CompactBatch, CompareConfig, PackedBatch, RegionBatch, ResultBatch
from aardvark_amd.merge import MergeConfig, PackedMultiBatch, merge_multi_batch

pytestmark = pytest.mark.gpu
BASES = b"ACGT"
N_REGIONS = 513
CONTIG_CHANGE = 300  # regions from here on lie on contig 1
LONG_CALL_AT = 400
RESULT_FIELDS = ("status", "ed_h1", "ed_h2", "n_optima", "type_present", "var_expected", "var_observed", "var_class", "var_zyg", "region_packed", "var_packed",
                 "bp_off", "bp_groups", "tally")
UNESCAPED = ("wide", "compact", "packed_pinned", "packed_pageable", "packed_submit", "packed_chunks")


def small_counts():
    rng = np.random.default_rng(21)
    counts = []
    for r in range(N_REGIONS):
        if r % 37 == 5:
            counts.append((int(rng.integers(6, 13)), int(rng.integers(6, 13))))
        elif r % 53 == 11:
            counts.append([(4, 1), (4, 2), (5, 0), (0, 6)][(r // 53) % 4])
        elif r % 101 == 7:
            counts.append([(100, 100), (40, 40), (20, 0), (0, 25), (60, 3)][(r // 101) % 5])
        else:
            counts.append((int(rng.integers(0, 4)), int(rng.integers(0, 4))))
    return counts


def small_job(escapes=False):
    """(contigs, RegionBatch): SNVs four bases apart from each window's start, the shared ones equal on both sides; escapes: three more regions, each beyond one of
    the packed form's narrow fields"""
    rng = np.random.default_rng(22)
    counts = small_counts()
    widths = [max(40, 4 * max(t, q) + 12) + (100 if r == LONG_CALL_AT else 0) for r, (t, q) in enumerate(counts)]
    zygs = ("HomozygousAlternate", "HomozygousAlternate", "UnphasedHeterozygous", "PhasedHet01")
    refs = [rng.integers(0, 4, 120_000).astype(np.uint8) for _ in range(2)]
    contigs = [bytes(BASES[b] for b in ref) for ref in refs]
    regions, cursor = [], [100, 100]

    def snv(c, p, i, r, small=False):
        return (p, contigs[c][p:p + 1], bytes([BASES[(refs[c][p] + 1 + (i + r) % 3) % 4]]), "Snv", zygs[(i + r) % 4] if small else "HomozygousAlternate")

    def add(c, width, t, q, r, extra_truth=()):
        s = cursor[c]
        small = max(t, q) <= 3
        regions.append({"start": s, "end": s + width, "contig": c, "truth": [snv(c, s + 4 + 4 * i, i, r, small) for i in range(t)] + list(extra_truth),
                        "query": [snv(c, s + 4 + 4 * i, i, r, small) for i in range(q)]})
        cursor[c] = s + width + 10

    for r, (t, q) in enumerate(counts):
        c = 0 if r < CONTIG_CHANGE else 1
        extra = ()
        if r == LONG_CALL_AT:  # one call with two long unrelated alleles, on the truth side only
            p = cursor[c] + 4 + 4 * max(t, q) + 2
            extra = [(p, contigs[c][p:p + 90], bytes(BASES[(refs[c][p + k] + 2) % 4] for k in range(90)), "Indel", "HomozygousAlternate")]
        add(c, widths[r], t, q, r, extra)
    if escapes:
        add(1, 70_000, 2, 2, N_REGIONS)  # a long window
        add(1, 4 * 256 + 40, 256, 3, N_REGIONS + 1)  # a count above 255
        p = cursor[1] + 20
        add(1, 400, 1, 1, N_REGIONS + 2, [(p, contigs[1][p:p + 1], contigs[1][p:p + 1] + bytes(BASES[x] for x in rng.integers(0, 4, 299)), "Insertion", "HomozygousAlternate")])
    return contigs, RegionBatch.from_regions(regions)


@pytest.fixture(scope="module")
def ctx():
    import aardvark_amd
    c = aardvark_amd.Context(0)
    for opt in ("lane_min_regions", "lane_min_batch", "pack_chunk_floor", "class_c_below"):  # (class_c_below: a batch this small would plan every region outside the lanes as class C)
        c.set_option(opt, 0)
    yield c
    c.close()


def result_of(form):
    return ResultBatch(form, sequences=False, group_metrics=False, bp_groups=True, packed=True)


def solve_form(ctx, name, batch, packed):
    """one call of the small job in the form `name` -> (ResultBatch, launches of the region pass)"""
    if name == "wide":
        res = ctx.solve_compare_regions(batch, CompareConfig(enable_sequences=False), group_metrics=False, bp_groups=True, packed=True)
    elif name == "compact":
        res = ctx.solve_compact(CompactBatch.from_region_batch(batch), res=result_of(batch))
    elif name == "packed_pageable":
        res = ctx.solve_packed(packed, res=result_of(packed))
    elif name == "packed_submit":
        pinned = ctx.pinned_packed(packed)
        res = ctx.submit_packed(pinned, res=ctx.pinned_results(pinned, bp_groups=True, packed=True)).wait()
    else:
        pinned = ctx.pinned_packed(packed)
        ctx.set_option("pack_chunks", 2 if name == "packed_chunks" else 0)
        try:
            res = ctx.solve_packed(pinned, res=ctx.pinned_results(pinned, bp_groups=True, packed=True))
        finally:
            ctx.set_option("pack_chunks", 0)
    return res, ctx.last_region_launches()


def same(a, b):
    return [f for f in RESULT_FIELDS if not np.array_equal(getattr(a, f), getattr(b, f))]


@pytest.fixture(scope="module")
def small(oracle):
    contigs, batch = small_job()
    assert batch.n_regions == N_REGIONS and np.count_nonzero(np.diff(batch.contig_idx.astype(np.int64))) == 1
    return contigs, batch, PackedBatch.from_compact(CompactBatch.from_region_batch(batch)), oracle_lib.compare_batch(oracle, batch, contigs, threads=4)


@pytest.mark.parametrize("name", UNESCAPED)
def test_small_job_in_every_form_equals_the_oracle(ctx, small, name):
    contigs, batch, packed, want = small
    ctx.upload_reference(contigs)
    got, launches = solve_form(ctx, name, batch, packed)
    print(name, "region launches", launches)
    assert got.diff(want) == []
    if name != "wide":  # (the wide call may solve in one shot, off the resident path's counters)
        assert launches == (4 if name == "packed_chunks" else 2)  # twice: one call was left to the host's edit distance; chunked: two groups and the catch-all first


def test_small_job_plans_alike_in_every_resident_form(ctx, small):
    contigs, batch, packed, want = small
    ctx.upload_reference(contigs)
    compact, pinned = CompactBatch.from_region_batch(batch), ctx.pinned_packed(packed)
    plans = {}
    for name, form, chunks in (("wide", batch, 0), ("compact", compact, 0), ("packed_pageable", packed, 0), ("packed_pinned", pinned, 0), ("packed_chunks", pinned, 2)):
        ctx.set_option("pack_chunks", chunks)
        try:
            rb = ctx.upload(form)
        finally:
            ctx.set_option("pack_chunks", 0)
        try:
            assert ctx.last_region_launches() == (4 if chunks else 2), name
            plans[name] = ctx.work_order(rb)
        finally:
            rb.free()
    order0, plan0 = plans["wide"]
    print(plan0)
    n_fast = sum(regions for first, regions, head in plan0["fast"])
    assert n_fast > 0 and plan0["class_c"] > 0 and plan0["class_b"] > 0  # the lane, class C and wave classes all occur
    edges = [0, plan0["class_c"], plan0["class_c"] + plan0["class_b"], N_REGIONS - n_fast] + [first + regions for first, regions, head in plan0["fast"] if regions]
    edges = sorted(set(edges + [N_REGIONS]))
    for name, (order, plan) in plans.items():
        assert plan == plan0, name
        for lo, hi in zip(edges[:-1], edges[1:]):
            assert np.array_equal(np.sort(order0[lo:hi]), np.sort(order[lo:hi])), (name, lo, hi)


def test_escaped_job_equals_its_wide_form(ctx):
    contigs, batch = small_job(escapes=True)
    packed = PackedBatch.from_compact(CompactBatch.from_region_batch(batch), escapes=True)
    e = packed.escapes
    assert (e.esc_region.size, e.esc_slot.size, e.esc_call.size) == (1, 1, 1)  # one entry in each list
    ctx.upload_reference(contigs)
    wide, _ = solve_form(ctx, "wide", batch, None)
    for name in ("packed_pinned", "packed_pageable", "packed_submit"):
        got, launches = solve_form(ctx, name, batch, packed)
        assert launches == 2 and same(got, wide) == [], name


def test_merge_forms_agree_with_each_other_and_the_oracle(ctx, oracle):
    from merge_lib import oracle_merge, same as same_merge, small_job as merge_job
    contigs, mb = merge_job(3, 257)
    assert mb.n_regions == 257 and mb.n_inputs == 3
    ctx.upload_reference(contigs)
    cfg = MergeConfig(majority_voting_enabled=True)
    wide, packed = merge_multi_batch(ctx, mb, cfg), merge_multi_batch(ctx, PackedMultiBatch.from_multi(mb), cfg)
    assert same_merge(wide, packed) and same_merge(wide, oracle_merge(oracle, mb, contigs, cfg))


def snv_batch(n, contig, ref):
    """n regions of 12 bases with one SNV on both sides each (the query's allele differs in every third region)"""
    start = 50 + 14 * np.arange(n, dtype=np.uint64)
    pos = np.repeat(start + 5, 2)
    base = ref[(start + 5).astype(np.int64)]
    letters = np.frombuffer(BASES, np.uint8)
    alleles = np.empty((n, 4), np.uint8)  # truth: allele0, allele1; query: allele0, allele1
    alleles[:, 0] = alleles[:, 2] = letters[base]
    alleles[:, 1] = letters[(base + 1) % 4]
    alleles[:, 3] = letters[np.where(np.arange(n) % 3 == 0, (base + 2) % 4, (base + 1) % 4)]
    voff, aoff = 2 * np.arange(n, dtype=np.uint64), 2 * np.arange(2 * n, dtype=np.uint64)
    one = np.ones(n, np.uint32)
    return RegionBatch(np.arange(n, dtype=np.uint64), np.zeros(n, np.uint32), start, start + 12, voff, one, voff + 1, one, pos, np.zeros(2 * n, np.uint8), np.full(2 * n, 5, np.uint8),
                       np.ones(2 * n, np.uint32), aoff, np.ones(2 * n, np.uint32), aoff + 1, np.ones(2 * n, np.uint32), alleles.reshape(-1))


def test_both_sides_of_the_side_stream_clearing(ctx):
    """262,143 regions: the counters and partials are cleared on the context's stream in front of the solver launches; 262,144: beside the writers on the side
    stream.  The second batch follows the first on the same context: what it clears was the first batch's.  (No oracle at this size: wide against packed.)"""
    n_max = 262_144
    ref = np.random.default_rng(23).integers(0, 4, 14 * n_max + 200).astype(np.uint8)
    contig = np.frombuffer(BASES, np.uint8)[ref].tobytes()
    ctx.upload_reference([contig])
    whole = snv_batch(n_max, contig, ref)
    for n in (n_max - 1, n_max):
        batch = whole if n == n_max else snv_batch(n, contig, ref)
        pinned = ctx.pinned_packed(PackedBatch.from_compact(CompactBatch.from_region_batch(batch)))
        got = ctx.solve_packed(pinned, res=ctx.pinned_results(pinned, bp_groups=True, packed=True))
        wide, _ = solve_form(ctx, "wide", batch, None)
        assert got.n_regions == n and same(got, wide) == [], n
        assert int(np.count_nonzero(got.status)) == 0 and int(got.tally.sum()) > 0  # the regions were solved
