"""Packed batches with escapes (avk_packed_escapes) on a real MI355X: a batch whose long alleles, long windows and dense sides are listed in the escape lists gives,
through every packed entry point, what the oracle gives for the same batch in the wide form — every region, every output array, statuses included — and is planned
exactly like the same batch handed in wide; a batch that lists nothing is untouched by the new entry points."""
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


def test_merge_packed_with_escapes_equals_the_wide_merge_and_the_oracle(oracle):
    import aardvark_amd
    from aardvark_amd.merge import AvkMergeConfig, MergeConfig, PackedMultiBatch, merge_multi_batch
    contigs, mb = el.merge_job()
    pm = PackedMultiBatch.from_multi(mb, escapes=True)
    assert pm.c_escapes() is not None
    k, n = 3, mb.n_regions
    # the oracle's pairs (input i as truth, input j as query, i < j) and the library's host classification on top
    pairs = [(i, j) for i in range(k) for j in range(i + 1, k)]
    io, ic = mb.in_off.reshape(n, k), mb.in_cnt.reshape(n, k)
    rep = lambda a: np.repeat(a, len(pairs))
    pb = RegionBatch(np.arange(n * len(pairs)), rep(mb.contig_idx), rep(mb.start), rep(mb.end), np.stack([io[:, i] for i, j in pairs], 1).reshape(-1),
                     np.stack([ic[:, i] for i, j in pairs], 1).reshape(-1), np.stack([io[:, j] for i, j in pairs], 1).reshape(-1), np.stack([ic[:, j] for i, j in pairs], 1).reshape(-1),
                     mb.var_pos, mb.var_type, mb.var_zyg, mb.var_raw_space, mb.a0_off, mb.a0_len, mb.a1_off, mb.a1_len, mb.allele_bytes)
    pst, pex = oracle_lib.optimize_pairs(oracle, pb, contigs, 50, threads=CPUS)
    unknown = np.array([bool((mb.var_zyg[int(io[m, 0]):int(io[m, 0]) + int(ic[m].sum())] == 0).any()) for m in range(n)], np.uint8)
    config = MergeConfig(majority_voting_enabled=True, no_conflict_enabled=True)
    cfg = AvkMergeConfig(50, 1, 1, -1)
    st, cls, mem = np.zeros(n, np.int32), np.zeros(n, np.uint8), np.zeros(n, np.uint64)
    P = lambda a, t: np.ascontiguousarray(a).ctypes.data_as(C.POINTER(t))
    lib = aardvark_amd.load_library()
    pst, pex, cnt32 = np.ascontiguousarray(pst, np.int32), np.ascontiguousarray(pex, np.uint8), np.ascontiguousarray(mb.in_cnt, np.uint32)
    assert lib.avk_merge_classify(C.c_uint64(n), C.c_uint32(k), P(cnt32, C.c_uint32), P(unknown, C.c_uint8), P(pst, C.c_int32), P(pex, C.c_uint8), C.byref(cfg),
                                  P(st, C.c_int32), P(cls, C.c_uint8), P(mem, C.c_uint64)) == 0
    ctx = aardvark_amd.Context(0)
    try:
        ctx.upload_reference(contigs)
        got = merge_multi_batch(ctx, pm, config)
        wide = merge_multi_batch(ctx, mb, config)
    finally:
        ctx.close()
    print("merge statuses:", np.unique(got.status, return_counts=True))
    assert int((got.status == ST_CAPACITY).sum()) == 0
    for name, a, b, c in (("status", got.status, wide.status, st), ("classification", got.classification, wide.classification, cls), ("members", got.members, wide.members, mem)):
        assert np.array_equal(a, b), name
        ok = c == a if name == "status" else (c == a) | (st != 0)  # (classification and members mean nothing for an unsolved region)
        assert bool(np.all(ok)), name


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
