"""The per-call results of a packed call by element (avk_dp_unpack_calls_kernel, csrc/avk_devpack.inl: dp_unpack_calls) on a real MI355X.

A dense batch read from its packed source has word j of the solver's per-call words at call j of the caller's arrays, so its per-call outputs are made four calls
per lane; every other batch keeps the region-by-region route (dp_unpack).  The jobs here are tiny and sit on the edges of that kernel: 1, 255, 256 and 257 regions;
1, 3, 4, 5 and 10 calls in all; regions without calls on one side and on both; a last region of 1, 2 or 3 calls behind a multiple of four (the tail lane).  Every
job is solved in the packed form (the element route) and in the compact form of the same batch (the region route) with each result form — the packed form alone,
the wide arrays, both — and both must equal the oracle bit for bit, and each other in every array they share.

Further: slices of the wide form that share the call arrays with their batch (one dense, one with holes; both start past call 0 and take the region route) leave
every byte they do not own as the caller filled it; a batch with escapes (widened first: the region route) equals its wide form; the packed form through
submit / wait; and a batch in which the tiers are so small that regions are repaired by the capacity retry behind the download."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib
import scenarios
from aardvark_amd import CompactBatch, CompareConfig, PackedBatch, RegionBatch, ResultBatch

pytestmark = pytest.mark.gpu
BASES = b"ACGT"
FORMS = ("only", False, True)  # ResultBatch(packed=...): the packed form alone, the wide arrays, both
REGION_FIELDS = ("status", "ed_h1", "ed_h2", "n_optima", "type_present", "region_packed")
CALL_FIELDS = ("var_expected", "var_observed", "var_class", "var_zyg", "var_packed")
SENTINEL = 0xEE


def mixed_counts(n, seed):
    """(truth, query) call counts of n regions: 0 to 3 per side, every 17th region 4 to 6 per side"""
    rng = np.random.default_rng(seed)
    return [(int(rng.integers(4, 7)), int(rng.integers(4, 7))) if r % 17 == 3 else (int(rng.integers(0, 4)), int(rng.integers(0, 4))) for r in range(n)]


CASES = {
    "one_region": [(2, 1)],
    "regions_255": mixed_counts(255, 1),
    "regions_256": mixed_counts(256, 2),
    "regions_257": mixed_counts(257, 3),
    "calls_1": [(1, 0)],
    "calls_3": [(1, 2)],
    "calls_4": [(2, 2)],
    "calls_5": [(3, 2)],
    "calls_10": [(3, 3), (2, 2)],
    "empty_sides": [(0, 2), (3, 0), (0, 0), (1, 1), (0, 0), (0, 3), (0, 0)],
    "tail_1": [(2, 2), (1, 3), (1, 0)],
    "tail_2": [(2, 2), (1, 3), (0, 2)],
    "tail_3": [(2, 2), (1, 3), (2, 1)],
}


def job(counts, seed=31):
    """(contigs, RegionBatch): region r has counts[r] SNVs per side, four bases apart from the window's start; a query call has the truth call's allele except where
    (i + r) % 4 == 0, and the zygosities cycle, so that the four per-call bytes differ from call to call"""
    rng = np.random.default_rng(seed)
    widths = [max(24, 4 * max(t, q) + 12) for t, q in counts]
    ref = rng.integers(0, 4, sum(widths) + 10 * len(widths) + 200).astype(np.uint8)
    contig = bytes(BASES[b] for b in ref)
    zygs = ("HomozygousAlternate", "UnphasedHeterozygous", "HomozygousAlternate", "PhasedHet01")
    regions, s = [], 100
    for r, (t, q) in enumerate(counts):
        def snv(i, query):
            p = s + 4 + 4 * i
            alt = (ref[p] + 1 + (i + r) % 3 + (1 if query and (i + r) % 4 == 0 else 0)) % 4
            if alt == ref[p]:
                alt = (alt + 1) % 4
            return (p, contig[p:p + 1], bytes([BASES[alt]]), "Snv", zygs[(i + r + (1 if query and i % 3 == 1 else 0)) % 4] if max(t, q) <= 3 else "HomozygousAlternate")
        regions.append({"start": s, "end": s + widths[r], "truth": [snv(i, False) for i in range(t)], "query": [snv(i, True) for i in range(q)]})
        s += widths[r] + 10
    return [contig], RegionBatch.from_regions(regions)


@pytest.fixture(scope="module")
def ctx():
    import aardvark_amd
    c = aardvark_amd.Context(0)
    for opt in ("lane_min_regions", "lane_min_batch", "class_c_below"):
        c.set_option(opt, 0)
    yield c
    c.close()


_jobs = {}


@pytest.fixture
def case(request, oracle):
    """(contigs, RegionBatch, PackedBatch, CompactBatch, the oracle's results) of CASES[name], made once"""
    name = request.param
    if name not in _jobs:
        contigs, batch = job(CASES[name])
        cb = CompactBatch.from_region_batch(batch)
        _jobs[name] = (contigs, batch, PackedBatch.from_compact(cb), cb, oracle_lib.compare_batch(oracle, batch, contigs, threads=4))
    return _jobs[name]


def differing(a, b):
    """the arrays both results hold that are not equal"""
    return [f for f in REGION_FIELDS + CALL_FIELDS + ("tally",) if getattr(a, f) is not None and getattr(b, f) is not None and not np.array_equal(getattr(a, f), getattr(b, f))]


def against_oracle(ctx, got, batch, want, form):
    wide = got.expanded(ctx.lib, batch) if form == "only" else got
    return wide.diff(want)


@pytest.mark.parametrize("form", FORMS, ids=("packed_only", "wide", "both"))
@pytest.mark.parametrize("case", sorted(CASES), indirect=True)
def test_element_route_equals_the_oracle_and_the_region_route(ctx, case, form):
    contigs, batch, pb, cb, want = case
    assert pb.n_variants == sum(int(t) + int(q) for t, q in zip(batch.t_cnt, batch.q_cnt))
    ctx.upload_reference(contigs)
    pinned = ctx.pinned_packed(pb)
    by_element = ctx.solve_packed(pinned, res=ctx.pinned_results(pinned, packed=form))
    pageable = ctx.solve_packed(pb, res=ResultBatch(pb, sequences=False, group_metrics=False, packed=form))
    by_region = ctx.solve_compact(cb, res=ResultBatch(cb, sequences=False, group_metrics=False, packed=form))
    assert against_oracle(ctx, by_element, batch, want, form) == []
    assert against_oracle(ctx, by_region, batch, want, form) == []
    assert differing(by_element, by_region) == [] and differing(pageable, by_region) == []
    if form is True:  # the packed form of a call is a function of its wide bytes
        v = pb.n_variants
        made = (by_element.var_expected[:v] & 3) | ((by_element.var_observed[:v] & 3) << 2) | ((by_element.var_zyg[:v] & 7) << 4)
        assert np.array_equal(by_element.var_packed[:v], made)


def compare_into(ctx, batch, res):
    """avk_compare_batch into a ResultBatch the caller has filled"""
    cb, cfg, ro = batch.c_struct(), CompareConfig(enable_sequences=False).c_struct(), res.c_struct()
    ctx._check(ctx.lib.avk_compare_batch(ctx.handle, C.byref(cb), C.byref(cfg), C.byref(ro)))
    return res


@pytest.mark.parametrize("holes", (False, True), ids=("dense_slice", "slice_with_holes"))
@pytest.mark.parametrize("case", ["regions_257"], indirect=True)
def test_a_slice_leaves_the_calls_it_does_not_own(ctx, case, holes):
    contigs, batch, pb, cb, want = case
    ctx.upload_reference(contigs)
    whole = ctx.solve_packed(pb, res=ResultBatch(pb, sequences=False, group_metrics=False, packed=True))
    assert whole.diff(want) == []
    if holes:  # every third region left out: calls inside the slice's range that no region of it owns
        idx = np.array([r for r in range(40, 200) if r % 3 != 1])
        sub = RegionBatch(batch.region_id[idx], batch.contig_idx[idx], batch.start[idx], batch.end[idx], batch.t_off[idx], batch.t_cnt[idx], batch.q_off[idx], batch.q_cnt[idx],
                          batch.var_pos, batch.var_type, batch.var_zyg, batch.var_raw_space, batch.a0_off, batch.a0_len, batch.a1_off, batch.a1_len, batch.allele_bytes)
    else:
        idx = np.arange(40, 200)
        sub = batch.slice(40, 200)
    assert int(sub.t_off[0]) > 0 and sub.n_variants == batch.n_variants
    owned = np.zeros(batch.n_variants, bool)
    for r in idx:
        owned[int(batch.t_off[r]):int(batch.t_off[r]) + int(batch.t_cnt[r])] = True
        owned[int(batch.q_off[r]):int(batch.q_off[r]) + int(batch.q_cnt[r])] = True
    assert owned.any() and not owned.all() and (not holes or not owned[int(sub.t_off[0]):int(sub.q_off[-1])].all())
    res = ResultBatch(sub, sequences=False, group_metrics=False, packed=True)
    for f in CALL_FIELDS:
        getattr(res, f)[...] = SENTINEL
    compare_into(ctx, sub, res)
    for f in REGION_FIELDS:
        assert np.array_equal(getattr(res, f), getattr(whole, f)[idx]), f
    for f in CALL_FIELDS:
        got = getattr(res, f)
        assert np.array_equal(got[owned], getattr(whole, f)[owned]), f
        assert (got[~owned] == SENTINEL).all(), f


@pytest.mark.parametrize("form", FORMS, ids=("packed_only", "wide", "both"))
@pytest.mark.parametrize("case", ["regions_257", "tail_3"], indirect=True)
def test_submit_and_wait(ctx, case, form):
    contigs, batch, pb, cb, want = case
    ctx.upload_reference(contigs)
    pinned = ctx.pinned_packed(pb)
    tickets = [ctx.submit_packed(pinned, res=ctx.pinned_results(pinned, packed=form)) for _ in range(2)]
    for t in tickets:
        assert against_oracle(ctx, t.wait(), batch, want, form) == []


def test_escaped_batch_equals_its_wide_form(ctx):
    """a batch with escapes is widened on the device and unpacked region by region, whatever the result form"""
    from test_gpu_upload_forms import small_job
    contigs, batch = small_job(escapes=True)
    pb = PackedBatch.from_compact(CompactBatch.from_region_batch(batch), escapes=True)
    assert not pb.escapes.empty()
    ctx.upload_reference(contigs)
    wide = ctx.solve_compare_regions(batch, CompareConfig(enable_sequences=False), group_metrics=False, packed=True)
    for form in FORMS:
        pinned = ctx.pinned_packed(pb)
        got = ctx.solve_packed(pinned, res=ctx.pinned_results(pinned, packed=form))
        assert differing(got, wide) == [], form


def test_capacity_retry_behind_the_element_route(oracle):
    """tiers so small that regions come back as capacity failures and are solved again behind the download: the repaired calls land where the element route put
    the others"""
    import aardvark_amd
    c = aardvark_amd.Context(0)
    try:
        for k, v in dict(lds_bytes_per_wave=2048, lds2_bytes_per_wave=0, ws_bytes_per_wave=0, big_ws_bytes=4096).items():
            c.set_option(k, v)
        contigs, batch = scenarios.fuzz_regions(341, 400, max_vars=9, max_len=12)
        c.upload_reference(contigs)
        want = oracle_lib.compare_batch(oracle, batch, contigs, threads=4)
        cb = CompactBatch.from_region_batch(batch)
        pb = PackedBatch.from_compact(cb)
        c.set_option("capacity_retry", 0)
        starved = c.solve_packed(pb, res=ResultBatch(pb, sequences=False, group_metrics=False, packed=True))
        assert (starved.status == 21).any()  # some regions do exhaust the last tier on the first try
        c.set_option("capacity_retry", 1)
        got = c.solve_packed(pb, res=ResultBatch(pb, sequences=False, group_metrics=False, packed=True))
        assert got.diff(want) == []
        by_region = c.solve_compact(cb, res=ResultBatch(cb, sequences=False, group_metrics=False, packed=True))
        assert differing(got, by_region) == []
    finally:
        c.close()
