"""The precision-recall curve by query score on a real MI355X (avk_score_hist_kernel, avk_score_curve_kernel): the resident form, the one-call form, scopes from a
strata handle, slices, score patterns, every upload form, shards, the refusals and the tool, against the restatement of the rule (tests/score_lib.py: no code
under test) on the ORACLE's per-call outputs, and the invariants against the size block and the tally.  Every comparison is exact.

Slices straddle the wave (1, 63, 64, 65 regions) and the kernel's regions-per-workgroup constant T = Context.score_block().  Scores are drawn per call of the wide
batch; an upload in the packed order gets them in that order (score_lib.packed_order)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import context_lib as cl
import escapes_lib
import oracle_lib
import scenarios
import score_lib
import size_lib
from aardvark_amd import CompactBatch, PackedBatch, ResultBatch, ScoreSpec, SizeSpec
from aardvark_amd._abi import N_GROUPS, AvkCompareConfig, AvkPackedBatch, AvkResultBatch

pytestmark = pytest.mark.gpu
CPUS = min(os.cpu_count() or 1, 16)
P = C.POINTER
u64p, f32p = P(C.c_uint64), P(C.c_float)
DEFAULT = score_lib.DEFAULT
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def job(oracle):
    """one context, one call set (indels, the invalid regions, the injected long alleles packed through the escape lists), the oracle's results: shared, never
    changed"""
    import aardvark_amd
    from aardvark_amd import synth
    contigs, base = scenarios.indel_small(1500)
    _, bad = scenarios.invalid_regions()
    plain = synth.concat_batches([base, bad])  # (packs without escapes)
    batch = escapes_lib.with_injections(contigs, plain)
    want = oracle_lib.compare_batch(oracle, batch, contigs, threads=CPUS)
    solved = np.asarray(want.status) == 0
    calls, vidx = size_lib.calls_of(batch, want), score_lib.call_index(batch, want)
    assert (~solved).any() and solved.sum() > 500
    assert ((calls[:, 1] == 0) & (calls[:, 5] == 1) & (calls[:, 7] > 0)).any(), "a truth FN with observed > 0"
    order = score_lib.packed_order(batch)
    assert len(order) == batch.n_variants
    ctx = aardvark_amd.Context(0)
    ctx.set_option("lane_min_regions", 0)
    ctx.set_option("lane_min_batch", 0)
    ctx.upload_reference(contigs)
    cb = CompactBatch.from_region_batch(batch)
    pe = PackedBatch.from_compact(cb, escapes=True)
    assert pe.c_escapes() is not None
    pp = PackedBatch.from_compact(CompactBatch.from_region_batch(plain))
    j = dict(contigs=contigs, batch=batch, plain=plain, want=want, solved=solved, calls=calls, vidx=vidx, alt_ed=size_lib.alt_eds(batch), order=order, ctx=ctx, cb=cb, pe=pe,
             pp=pp, T=ctx.score_block(), n=batch.n_regions, n_plain=plain.n_regions, scores={})
    yield j
    ctx.close()


def scores_of(job, thresholds=DEFAULT):
    """the seeded scores of a spec, per call of the wide batch (made once)"""
    if thresholds not in job["scores"]:
        job["scores"][thresholds] = score_lib.scores_for(job["batch"].n_variants, thresholds, 3)
    return job["scores"][thresholds]


def packed_scores(job, scores, plain=False):
    sc = np.ascontiguousarray(scores[job["order"]])
    return sc[:job["pp"].n_variants] if plain else sc


def want_of(job, thresholds=DEFAULT, scores=None, lo=0, hi=None, members=None):
    scores = scores_of(job, thresholds) if scores is None else scores
    return score_lib.expected(job["calls"], job["vidx"], job["alt_ed"], thresholds, scores, job["n"], members, lo=lo, hi=hi)


def resident(ctx, src, spec, scores, strata=None, out=None):
    rb = ctx.upload(src)
    try:
        ctx.compare_resident(rb)
        return ctx.score_tallies(rb, spec, scores, strata=strata, out=out)
    finally:
        rb.free()


def test_score_block(job):
    assert job["T"] == score_lib.load().score_emu_threads() == 256


@pytest.mark.parametrize("thresholds", score_lib.SPECS)
def test_resident_scope_0(job, thresholds):
    """K = 1, 2, 10 and 31: the curve equals the restatement's; a second call doubles `out`; words of other scopes are untouched; the invariants"""
    ctx = job["ctx"]
    want = want_of(job, thresholds)
    sc = packed_scores(job, scores_of(job, thresholds))
    rb = ctx.upload(job["pe"])
    try:
        ctx.compare_resident(rb)
        out = np.zeros((3, len(thresholds) + 1, N_GROUPS, 14), np.uint64)
        out[1:] = 7
        ctx.score_tallies(rb, ScoreSpec(thresholds), sc, out=out)
        assert np.array_equal(out[:1], want), np.argwhere(out[:1] != want)[:8]
        assert (out[1:] == 7).all()
        ctx.score_tallies(rb, ScoreSpec(thresholds), sc, out=out)
        assert np.array_equal(out[:1], 2 * want) and (out[1:] == 7).all()
    finally:
        rb.free()
    tally = np.asarray(job["want"].group_metrics).reshape(job["n"], N_GROUPS, 22)[job["solved"]].astype(np.uint64).sum(axis=0)
    score_lib.check_invariants(want, tally[:, :14][None])
    assert not np.array_equal(want[0, 0], want[0, -1]) and want[0, -1, 0].any()


def reorder_trees(tree_off, start, end_max, n_contigs, order):
    """the interval sets of the labels `order` (None: a label without intervals), in that order"""
    off, s, e = [0], [], []
    for l in order:
        for c in range(n_contigs):
            if l is not None:
                a, b = int(tree_off[l * n_contigs + c]), int(tree_off[l * n_contigs + c + 1])
                s += start[a:b].tolist()
                e += end_max[a:b].tolist()
            off.append(len(s))
    return np.array(off, np.uint64), np.array(s, np.uint32), np.array(e, np.uint32)


@pytest.fixture(scope="module")
def strata_job(job):
    """a handle of 33 labels: 28 without intervals, four of random intervals, and label 32 — the second mask word — every contig whole; which regions each holds"""
    ctx, contigs = job["ctx"], job["contigs"]
    n_bed, n_contigs, tree_off, start, end_max = cl.bed_trees(5, contigs)
    tree_off, start, end_max = reorder_trees(tree_off, start, end_max, n_contigs, [None] * 28 + [1, 2, 3, 4, 0])
    st = ctx.upload_strata(33, n_contigs, tree_off, start, end_max)
    assert st.n_labels == 33
    rb = ctx.upload(job["pe"])
    off, idx = ctx.strata_region_labels(rb, st)
    rb.free()
    n = job["n"]
    members = size_lib.members_of_lists(off, idx, 33, n)
    has_calls = (np.asarray(job["batch"].t_cnt) + np.asarray(job["batch"].q_cnt)) > 0
    assert np.array_equal(members[32] & job["solved"], has_calls & job["solved"]) and not members[:28].any() and members[28:32].any()
    yield dict(st=st, members=list(members), L=33)
    st.free()


def test_scopes_from_a_strata_handle(job, strata_job):
    """empty labels, interval labels and a whole-contig label in the second mask word"""
    ctx, st, members = job["ctx"], strata_job["st"], strata_job["members"]
    got = resident(ctx, job["pe"], ScoreSpec(), packed_scores(job, scores_of(job)), strata=st)
    want = want_of(job, members=members)
    assert got.shape == (34, 11, N_GROUPS, 14) and np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert np.array_equal(got[33], got[0]) and not got[1:29].any() and got[29:33].any()
    score_lib.check_invariants(got)


def test_scopes_with_31_thresholds(job, strata_job):
    """32 points: one scope a launch, 34 launches"""
    got = resident(job["ctx"], job["pe"], ScoreSpec(score_lib.THIRTY_ONE), packed_scores(job, scores_of(job, score_lib.THIRTY_ONE)), strata=strata_job["st"])
    assert np.array_equal(got, want_of(job, score_lib.THIRTY_ONE, members=strata_job["members"]))


def packed_slice(pb, lo, hi):
    """regions [lo, hi) of a packed batch without escapes as a packed batch of their own, and the range of its calls"""
    cnt = pb.t_cnt.astype(np.int64) + pb.q_cnt
    v0, v1 = int(cnt[:lo].sum()), int(cnt[:hi].sum())
    alen = pb.a0_len.astype(np.int64) + pb.a1_len
    a0, a1 = int(alen[:v0].sum()), int(alen[:v1].sum())
    reg, var = np.s_[lo:hi], np.s_[v0:v1]
    return PackedBatch(contig_idx=pb.contig_idx[reg], start=pb.start[reg], len=pb.len[reg], t_cnt=pb.t_cnt[reg], q_cnt=pb.q_cnt[reg], var_rel_pos=pb.var_rel_pos[var],
                       var_type_zyg=pb.var_type_zyg[var], a0_len=pb.a0_len[var], a1_len=pb.a1_len[var],
                       var_raw_space=None if pb.var_raw_space is None else pb.var_raw_space[var], allele_bytes=pb.allele_bytes[a0:a1]), v0, v1


@pytest.mark.parametrize("n", ["1", "63", "64", "65", "T-1", "T", "T+1", "2T+1"])
def test_slices(job, n):
    T = job["T"]
    n = {"T-1": T - 1, "T": T, "T+1": T + 1, "2T+1": 2 * T + 1}.get(n) or int(n)
    lo = 3
    part, v0, v1 = packed_slice(job["pp"], lo, lo + n)
    got = resident(job["ctx"], part, ScoreSpec(), np.ascontiguousarray(packed_scores(job, scores_of(job))[v0:v1]))
    want = want_of(job, lo=lo, hi=lo + n)
    assert np.array_equal(got, want) and want.any()


@pytest.mark.parametrize("pattern", ["nan", "below", "above"])
def test_score_patterns(job, pattern):
    """every score missing or below t[0]: the query side is empty beyond point 0 and every supported truth call is lost; every score above: a flat curve"""
    value = {"nan": NAN, "below": 4.75, "above": 1e9}[pattern]
    scores = np.full(job["batch"].n_variants, value, np.float32)
    got = resident(job["ctx"], job["pe"], ScoreSpec(), scores)
    want = want_of(job, scores=scores)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    if pattern == "above":
        assert (got[0] == got[0, :1]).all() and got[0, 0].any()
    else:
        assert not got[0, 1:, :, size_lib.QUERY_F].any() and got[0, 0, 0, size_lib.QUERY_F].any() and (got[0, 1:] == got[0, 1:2]).all()


def test_point_0_is_the_size_block_and_the_tally(job):
    ctx = job["ctx"]
    ctx_scores = packed_scores(job, scores_of(job))
    rb = ctx.upload(job["pe"])
    try:
        ctx.compare_resident(rb)
        curve = ctx.score_tallies(rb, ScoreSpec(), ctx_scores)
        size = ctx.size_tallies(rb, SizeSpec())
    finally:
        rb.free()
    res = ctx.solve_packed(job["pe"], res=ResultBatch(job["pe"], sequences=False, group_metrics=False, packed="only"))
    assert np.array_equal(curve[0, 0], size[0].sum(axis=0))
    assert np.array_equal(curve[0, 0], size_lib.tally14(np.asarray(res.tally))) and curve[0, 0].any()


@pytest.mark.parametrize("form", ["wide", "compact", "packed", "packed_source=0", "packed + escapes"])
def test_upload_forms(job, form):
    ctx = job["ctx"]
    whole = form in ("wide", "compact", "packed + escapes")
    src = {"wide": job["batch"], "compact": job["cb"], "packed": job["pp"], "packed_source=0": job["pp"], "packed + escapes": job["pe"]}[form]
    wide = scores_of(job)
    # the wide and the compact form keep the batch's own call order (its t_off / q_off); the packed forms their own
    sc = wide if form in ("wide", "compact") else packed_scores(job, wide, plain=not whole)
    ctx.set_option("packed_source", 0 if form == "packed_source=0" else 1)
    try:
        got = resident(ctx, src, ScoreSpec(), sc)
    finally:
        ctx.set_option("packed_source", 1)
    assert np.array_equal(got, want_of(job, hi=None if whole else job["n_plain"]))


def same(a, b):
    return np.array_equal(a.region_packed, b.region_packed) and np.array_equal(a.var_packed, b.var_packed) and np.array_equal(a.tally, b.tally)


def test_one_call_form(job, strata_job):
    """the block is the resident form's and the restatement's; results and tally bit-identical to a plain solve_packed"""
    ctx, pe, st, members = job["ctx"], job["pe"], strata_job["st"], strata_job["members"]
    sc = packed_scores(job, scores_of(job))
    new = lambda: ResultBatch(pe, sequences=False, group_metrics=False, packed="only")
    bare = ctx.solve_packed(pe, res=new())
    alone = ctx.solve_packed(pe, res=new(), score=ScoreSpec(), scores=sc)
    assert same(alone, bare) and np.array_equal(alone.score_tallies, want_of(job)) and bare.tally.any()
    assert np.array_equal(alone.tally[:N_GROUPS * 22].reshape(N_GROUPS, 22)[:, :14], alone.score_tallies[0, 0])
    got = ctx.solve_packed(pe, res=new(), strata=st, score=ScoreSpec(), scores=sc)
    assert same(got, bare) and np.array_equal(got.score_tallies, want_of(job, members=members))
    twice = ctx.solve_packed(pe, res=new(), score=ScoreSpec(), scores=sc, score_tallies=alone.score_tallies.copy())
    assert np.array_equal(twice.score_tallies, 2 * want_of(job))
    with pytest.raises(ValueError):
        ctx.solve_packed(pe, res=new(), score=ScoreSpec(), scores=sc, size=SizeSpec())


def test_shards_add_up(job):
    """the hash-sharded halves of the batch add up to the whole: each shard's scores are its regions' calls in its own order"""
    ctx, pb = job["ctx"], job["pp"]
    lib = ctx.lib
    lib.avk_packed_shard_make.argtypes = [P(AvkPackedBatch), u64p, C.c_uint64, C.c_uint32, C.c_uint32, P(C.c_void_p)]
    lib.avk_packed_shard_batch.restype = P(AvkPackedBatch)
    lib.avk_packed_shard_batch.argtypes = [C.c_void_p]
    lib.avk_packed_shard_free.argtypes = [C.c_void_p]
    lib.avk_packed_shard_regions.restype = C.c_uint64
    lib.avk_packed_shard_regions.argtypes = [C.c_void_p, P(P(C.c_uint64))]
    st, ids = pb.c_struct(), np.arange(pb.n_regions, dtype=np.uint64)
    sc = packed_scores(job, scores_of(job), plain=True)
    cnt = pb.t_cnt.astype(np.int64) + pb.q_cnt
    voff = np.concatenate([[0], np.cumsum(cnt)])
    total = np.zeros((1, 11, N_GROUPS, 14), np.uint64)
    cfg, ss = AvkCompareConfig(50, 0, 0), ScoreSpec().c_struct()
    taken = 0
    for rank in range(2):
        h = C.c_void_p()
        assert lib.avk_packed_shard_make(C.byref(st), ids.ctypes.data_as(u64p), 0, rank, 2, C.byref(h)) == 0
        sb = lib.avk_packed_shard_batch(h).contents
        m = int(sb.n_regions)
        assert 0 < m < pb.n_regions
        index = P(C.c_uint64)()
        assert int(lib.avk_packed_shard_regions(h, C.byref(index))) == m  # which regions of the whole the shard holds, in its order
        regions = [int(index[i]) for i in range(m)]
        part = np.ascontiguousarray(np.concatenate([sc[voff[r]:voff[r + 1]] for r in regions] + [np.zeros(1, np.float32)]))
        assert part.size - 1 == int(sb.n_variants)
        taken += m
        status = np.full(m + 1, -1, np.int32)
        ro = AvkResultBatch()
        ro.status = status.ctypes.data_as(P(C.c_int32))
        ctx._check(lib.avk_compare_packed_score(ctx.handle, C.byref(sb), None, None, C.byref(cfg), C.byref(ss), part.ctypes.data_as(f32p), C.byref(ro), total.ctypes.data_as(u64p)))
        lib.avk_packed_shard_free(h)
    assert taken == pb.n_regions and np.array_equal(total, want_of(job, hi=job["n_plain"]))


def test_refusals_then_a_correct_solve(job):
    """a bad spec, null scores, device_pack 0: each leaves `out` untouched and the context solves the next call correctly"""
    import aardvark_amd
    ctx, pp = job["ctx"], job["pp"]
    sc = packed_scores(job, scores_of(job), plain=True)
    scp = sc.ctypes.data_as(f32p)
    out = np.zeros((1, 32, N_GROUPS, 14), np.uint64)
    outp = out.ctypes.data_as(u64p)
    rb = ctx.upload(pp)
    try:
        good = ScoreSpec().c_struct()
        assert ctx.lib.avk_score_tallies(ctx.handle, rb.handle, C.byref(good), scp, None, outp) == -4  # not solved yet: AVK_E_STATE
        assert "avk_compare_resident has solved" in ctx.lib.avk_last_error(ctx.handle).decode()
        ctx.compare_resident(rb)
        assert ctx.lib.avk_score_tallies(ctx.handle, rb.handle, None, scp, None, outp) == -1 and "spec missing" in ctx.lib.avk_last_error(ctx.handle).decode()
        for t in [(), tuple(range(32)), (NAN,), (1.0, INF), (3.0, 3.0), (6.0, 1.0)]:
            bad = score_lib.c_spec(t[:31], n=len(t))
            assert ctx.lib.avk_score_tallies(ctx.handle, rb.handle, C.byref(bad), scp, None, outp) == -1, t
            assert "strictly ascending" in ctx.lib.avk_last_error(ctx.handle).decode()
        assert ctx.lib.avk_score_tallies(ctx.handle, rb.handle, C.byref(good), None, None, outp) == -1 and "scores missing" in ctx.lib.avk_last_error(ctx.handle).decode()
        assert ctx.lib.avk_score_tallies(ctx.handle, rb.handle, C.byref(good), scp, None, None) == -1
        assert not out.any()
        assert np.array_equal(ctx.score_tallies(rb, ScoreSpec(), sc), want_of(job, hi=job["n_plain"]))
    finally:
        rb.free()
    new = lambda: ResultBatch(pp, sequences=False, group_metrics=False)
    with pytest.raises(aardvark_amd.AardvarkAmdError, match="strictly ascending"):
        ctx.solve_packed(pp, res=new(), score=ScoreSpec((5.0, 5.0)), scores=sc, score_tallies=out)
    with pytest.raises(aardvark_amd.AardvarkAmdError, match="scores missing"):
        ctx.solve_packed(pp, res=new(), score=ScoreSpec(), scores=None, score_tallies=out)
    ctx.set_option("device_pack", 0)
    try:
        with pytest.raises(aardvark_amd.AardvarkAmdError, match="error -4.*device_pack"):
            ctx.solve_packed(pp, res=new(), score=ScoreSpec(), scores=sc, score_tallies=out)
    finally:
        ctx.set_option("device_pack", 1)
    assert not out.any()
    got = ctx.solve_packed(pp, res=new(), score=ScoreSpec(), scores=sc)
    assert np.array_equal(np.asarray(got.status)[:job["n_plain"]], job["want"].status[:job["n_plain"]]) and np.array_equal(got.score_tallies, want_of(job, hi=job["n_plain"]))


# ---- the tool ---------------------------------------------------------------------------------------------------------------------------------------------
CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "aardvark_amd", "bin", "aardvark_amd_compare")
QUALS = ["3", "10", "17.5", "20", ".", "45", "61", "9.99", "30"]


def test_tool_writes_the_curve_beside_an_unchanged_summary(oracle, tmp_path):
    """aardvark_amd_compare --roc QUAL on a small job: summary_roc.tsv is the writer fed with the restatement's block on the oracle's results, summary.tsv is
    byte-identical to a run without --roc"""
    import gzip
    from aardvark_amd import feeder
    case = escapes_lib.write_feeder_case(tmp_path)
    lines = gzip.decompress(open(case["q"], "rb").read()).decode().split("\n")
    k = 0
    for i, line in enumerate(lines):
        if line and not line.startswith("#"):
            cells = line.split("\t")
            cells[5] = QUALS[k % len(QUALS)]
            lines[i], k = "\t".join(cells), k + 1
    open(case["q"], "wb").write(gzip.compress("\n".join(lines).encode()))

    def run(name, *extra):
        out = str(tmp_path / name)
        r = subprocess.run([CLI, "-r", case["fa"], "-t", case["t"], "-q", case["q"], "-b", case["bed"], "--min-variant-gap", str(escapes_lib.GAP), "-o", out, "-v",
                            "--enable-haplotype-metrics", "--enable-weighted-haplotype-metrics"] + list(extra), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        read = lambda f: open(os.path.join(out, f), "rb").read() if os.path.exists(os.path.join(out, f)) else None
        return read("summary.tsv"), read("summary_roc.tsv"), r.stderr

    plain, none, _ = run("plain")
    summary, roc, err = run("roc", "--roc", "QUAL")
    assert none is None and summary == plain and roc is not None and "avk_compare_packed_score" in err
    g = feeder.Genome(case["fa"])
    feed = feeder.feed_compare(case["t"], case["q"], case["bed"], g, min_variant_gap=escapes_lib.GAP, score_field="QUAL")
    want = oracle_lib.compare_batch(oracle, feed.batch, [bytes(c) for c in g.contigs()], threads=CPUS)
    calls, vidx = size_lib.calls_of(feed.batch, want), score_lib.call_index(feed.batch, want)
    block = score_lib.expected(calls, vidx, size_lib.alt_eds(feed.batch), DEFAULT, feed.scores, feed.batch.n_regions)
    assert not np.array_equal(block[0, 0], block[0, -1]) and block[0, -1].any()
    ref = str(tmp_path / "want_roc.tsv")
    feeder.write_summary_roc(ref, score_lib.names_of(DEFAULT), [], block)
    assert roc == open(ref, "rb").read()
    s2, r2, err2 = run("wide", "--roc", "QUAL", "--batch-form", "wide")
    assert s2 == plain and r2 == roc and "avk_score_tallies_host" in err2
    s3, r3, err3 = run("both", "--roc", "QUAL", "--size-strata", "--devices", "0,0", "--batch-regions", "100")
    assert s3 == plain and r3 == roc and "avk_score_tallies)" in err3
