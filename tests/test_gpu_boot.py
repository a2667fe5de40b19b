"""Bootstrap replicates of the tallies on a real MI355X (avk_boot_tally_kernel): the resident form, the one-call form, scopes from a strata handle, slices, every
upload form, the capacity retry, shards and the refusals, against the ORACLE's per-region blocks times weights from the numpy restatement of the rule
(tests/boot_lib.py: no code under test).  Every comparison is exact.

Replicate counts straddle a launch's block R = Context.boot_block(): 1, R - 1, R, R + 1, 2 R + 1; slices straddle the kernel's tile T of 32 regions.  Which regions a
label of a strata handle holds is asked of Context.strata_region_labels — the lists of the same masks, pinned against the host's lists by tests/test_gpu_strata.py
and against the rule of the context labels by tests/test_gpu_context_strata.py; label 0 (whole contigs) and the empty label are checked by hand."""
import ctypes as C
import os

import numpy as np
import pytest

import boot_lib
import context_lib as cl
import escapes_lib
import oracle_lib
import scenarios
from aardvark_amd import BootSpec, CompactBatch, ContextSpec, PackedBatch, ResultBatch
from aardvark_amd._abi import TALLY_LEN, AvkBootSpec, AvkCompareConfig, AvkPackedBatch, AvkResultBatch

pytestmark = pytest.mark.gpu
CPUS = min(os.cpu_count() or 1, 16)
WORDS, SOLVED, ERRORS = boot_lib.WORDS, boot_lib.SOLVED, boot_lib.ERRORS
TILE = 32
P = C.POINTER
SEED = 20260101


@pytest.fixture(scope="module")
def job(oracle):
    """one context, one call set (SNVs and indels, several call types per region, some unsolved regions), the oracle's results: shared, never changed"""
    import aardvark_amd
    from aardvark_amd import synth
    contigs, base = scenarios.indel_small(1500)
    _, bad = scenarios.invalid_regions()
    batch = synth.concat_batches([base, bad])
    want = oracle_lib.compare_batch(oracle, batch, contigs, threads=CPUS)
    solved = np.asarray(want.status) == 0
    assert (~solved).any() and solved.sum() > 500
    ctx = aardvark_amd.Context(0)
    ctx.set_option("lane_min_regions", 0)
    ctx.set_option("lane_min_batch", 0)
    ctx.upload_reference(contigs)
    pb = PackedBatch.from_compact(CompactBatch.from_region_batch(batch))
    n = batch.n_regions
    yield dict(ctx=ctx, contigs=contigs, batch=batch, pb=pb, want=want, solved=solved, blocks=np.asarray(want.group_metrics).reshape(n, WORDS), R=ctx.boot_block(),
               contig=np.asarray(batch.contig_idx), start=np.asarray(batch.start))
    ctx.close()


def want_of(job, B, seed=SEED, lo=0, hi=None, members=None):
    hi = job["batch"].n_regions if hi is None else hi
    w = boot_lib.weights(seed, job["contig"][lo:hi], job["start"][lo:hi], np.arange(B))
    return boot_lib.expected(job["blocks"][lo:hi], job["solved"][lo:hi], w, None if members is None else [m[lo:hi] for m in members])


def packed_slice(pb, lo, hi):
    """regions [lo, hi) of a packed batch as a packed batch of their own"""
    cnt = pb.t_cnt.astype(np.int64) + pb.q_cnt
    v0, v1 = int(cnt[:lo].sum()), int(cnt[:hi].sum())
    alen = pb.a0_len.astype(np.int64) + pb.a1_len
    a0, a1 = int(alen[:v0].sum()), int(alen[:v1].sum())
    reg, var = np.s_[lo:hi], np.s_[v0:v1]
    return PackedBatch(contig_idx=pb.contig_idx[reg], start=pb.start[reg], len=pb.len[reg], t_cnt=pb.t_cnt[reg], q_cnt=pb.q_cnt[reg], var_rel_pos=pb.var_rel_pos[var],
                       var_type_zyg=pb.var_type_zyg[var], a0_len=pb.a0_len[var], a1_len=pb.a1_len[var],
                       var_raw_space=None if pb.var_raw_space is None else pb.var_raw_space[var], allele_bytes=pb.allele_bytes[a0:a1])


def resident(ctx, src, spec, strata=None, out=None):
    ctx.set_option("emit_bp_groups", 1)
    rb = ctx.upload(src)
    try:
        ctx.compare_resident(rb)
        return ctx.boot_tallies(rb, spec, strata=strata, out=out)
    finally:
        rb.free()
        ctx.set_option("emit_bp_groups", 0)


def test_boot_block(job):
    assert job["R"] == boot_lib.load().boot_emu_reps() == 21


@pytest.mark.parametrize("which", range(5))
def test_resident_scope_0(job, which):
    """the sums equal the restatement's; a second call doubles `out`; word AVK_TALLY_ERRORS stays; word AVK_TALLY_SOLVED is the sum of the weights"""
    ctx, R = job["ctx"], job["R"]
    B = [1, R - 1, R, R + 1, 2 * R + 1][which]
    want = want_of(job, B)
    assert want[0, :, :WORDS].any()
    ctx.set_option("emit_bp_groups", 1)
    rb = ctx.upload(job["pb"])
    try:
        ctx.compare_resident(rb)
        out = np.zeros((1, B, TALLY_LEN), np.uint64)
        out[:, :, ERRORS] = 7
        ctx.boot_tallies(rb, BootSpec(B, SEED), out=out)
        assert np.array_equal(out[:, :, :ERRORS], want[:, :, :ERRORS]), np.argwhere(out[:, :, :ERRORS] != want[:, :, :ERRORS])[:8]
        assert (out[:, :, ERRORS] == 7).all()
        w = boot_lib.weights(SEED, job["contig"], job["start"], np.arange(B))
        assert np.array_equal(out[0, :, SOLVED], w[job["solved"]].sum(axis=0))
        ctx.boot_tallies(rb, BootSpec(B, SEED), out=out)
        assert np.array_equal(out[:, :, :ERRORS], 2 * want[:, :, :ERRORS])
        other = ctx.boot_tallies(rb, BootSpec(B, SEED + 1))
        assert not np.array_equal(other, want)
    finally:
        rb.free()
        ctx.set_option("emit_bp_groups", 0)


@pytest.fixture(scope="module")
def strata_job(job):
    """a handle of 5 BED labels (label 0: every contig whole), one label without intervals and the 16 default context labels; which regions each holds"""
    ctx, contigs = job["ctx"], job["contigs"]
    n_bed, n_contigs, tree_off, start, end_max = cl.bed_trees(5, contigs)
    tree_off = np.concatenate([tree_off, np.full(n_contigs, tree_off[-1], np.uint64)])  # label 5: no interval on any contig
    spec = ContextSpec()
    st = ctx.upload_strata(n_bed + 1, n_contigs, tree_off, start, end_max, context=spec)
    L = st.n_labels
    assert L == 6 + spec.n_labels
    rb = ctx.upload(job["pb"])
    off, idx = ctx.strata_region_labels(rb, st)
    rb.free()
    n = job["batch"].n_regions
    members = np.zeros((L, n), bool)
    members[idx, np.repeat(np.arange(n), np.diff(off.astype(np.int64)))] = True
    has_calls = (np.asarray(job["batch"].t_cnt) + np.asarray(job["batch"].q_cnt)) > 0
    assert np.array_equal(members[0] & job["solved"], has_calls & job["solved"]) and not members[5].any() and members[1:5].any() and members[6:].any()
    yield dict(st=st, members=list(members), L=L)
    st.free()


def test_resident_with_a_strata_handle(job, strata_job):
    """a label on every region, one on none, interval labels and context labels: (1 + L) * B blocks, B one more than a launch holds"""
    ctx, st, members, L = job["ctx"], strata_job["st"], strata_job["members"], strata_job["L"]
    B = job["R"] + 1
    got = resident(ctx, job["pb"], BootSpec(B, SEED), strata=st)
    want = want_of(job, B, members=members)
    assert got.shape == (1 + L, B, TALLY_LEN) and np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert got[1].any() and not got[6].any() and sum(int(got[1 + l].any()) for l in range(6, L)) >= 2


@pytest.mark.parametrize("n", [1, TILE - 1, TILE, TILE + 1])
def test_slices(job, n):
    lo = 3
    got = resident(job["ctx"], packed_slice(job["pb"], lo, lo + n), BootSpec(job["R"] + 1, SEED))
    assert np.array_equal(got, want_of(job, job["R"] + 1, lo=lo, hi=lo + n))


@pytest.mark.parametrize("form", ["packed_source=0", "escaped", "wide"])
def test_other_sources(job, form):
    ctx, pb = job["ctx"], job["pb"]
    ctx.set_option("packed_source", 0 if form == "packed_source=0" else 1)
    src = pb
    if form == "escaped":
        src = escapes_lib.promote(pb, regions=[1, 7, pb.n_regions - 1], slots=[0, 5, 2 * pb.n_regions - 2], calls=[0, 3, pb.n_variants - 1])
        assert not src.escapes.empty()
    if form == "wide":
        src = job["batch"]
    try:
        got = resident(ctx, src, BootSpec(5, SEED))
        assert np.array_equal(got, want_of(job, 5))
    finally:
        ctx.set_option("packed_source", 1)


def test_capacity_retry_counts_repaired_regions(oracle):
    """tiny tiers: regions come back AVK_ST_CAPACITY and are repaired by the download; the resident form called after the download and the one-call form count them"""
    import aardvark_amd
    ctx = aardvark_amd.Context(0)
    try:
        for k, v in dict(lds_bytes_per_wave=2048, lds2_bytes_per_wave=0, ws_bytes_per_wave=0, big_ws_bytes=4096).items():
            ctx.set_option(k, v)
        contigs, batch = scenarios.fuzz_regions(341, 400, max_vars=9, max_len=12)
        ctx.upload_reference(contigs)
        want = oracle_lib.compare_batch(oracle, batch, contigs, threads=CPUS)
        pb = PackedBatch.from_compact(CompactBatch.from_region_batch(batch))
        ctx.set_option("capacity_retry", 0)
        starved = ctx.solve_packed(pb, res=ResultBatch(pb, sequences=False, group_metrics=False))
        assert (starved.status == 21).any()
        ctx.set_option("capacity_retry", 1)
        B = 7
        w = boot_lib.weights(SEED, batch.contig_idx, batch.start, np.arange(B))
        sums = boot_lib.expected(np.asarray(want.group_metrics).reshape(batch.n_regions, WORDS), np.asarray(want.status) == 0, w)
        ctx.set_option("emit_bp_groups", 1)
        rb = ctx.upload(pb)
        ctx.compare_resident(rb)
        res = ctx.download(rb, group_metrics=False)
        assert np.array_equal(np.asarray(res.status)[:batch.n_regions], want.status)
        assert np.array_equal(ctx.boot_tallies(rb, BootSpec(B, SEED)), sums)
        rb.free()
        ctx.set_option("emit_bp_groups", 0)
        one = ctx.solve_packed(pb, res=ResultBatch(pb, sequences=False, group_metrics=False), boot=BootSpec(B, SEED))
        assert np.array_equal(one.boot_tallies, sums)
    finally:
        ctx.close()


def same(a, b):
    return np.array_equal(a.region_packed, b.region_packed) and np.array_equal(a.var_packed, b.var_packed) and np.array_equal(a.tally, b.tally)


def test_one_call_form(job, strata_job):
    """results, tally and label sums bit-identical to the call without a spec; the replicates are the resident form's and the restatement's; replicates = 0 is the old call"""
    ctx, pb, st, members = job["ctx"], job["pb"], strata_job["st"], strata_job["members"]
    B = job["R"] + 1
    new = lambda: ResultBatch(pb, sequences=False, group_metrics=False, packed="only")
    plain = ctx.solve_packed(pb, res=new(), strata=st)
    got = ctx.solve_packed(pb, res=new(), strata=st, boot=BootSpec(B, SEED))
    assert same(got, plain) and np.array_equal(got.label_tallies, plain.label_tallies) and plain.label_tallies.any()
    assert np.array_equal(got.boot_tallies, want_of(job, B, members=members))
    assert np.array_equal(got.boot_tallies, resident(ctx, pb, BootSpec(B, SEED), strata=st))
    bare = ctx.solve_packed(pb, res=new())
    alone = ctx.solve_packed(pb, res=new(), boot=BootSpec(B, SEED))
    assert same(alone, bare) and np.array_equal(alone.boot_tallies, want_of(job, B))
    # replicates = 0 through the C entry point: the call without a spec, boot_tallies not read
    res = new()
    st_pb, cfg, ro, bs = pb.c_struct(), AvkCompareConfig(50, 0, 0), res.c_struct(), AvkBootSpec(0, SEED)
    sums = np.zeros((st.n_labels, TALLY_LEN), np.uint64)
    ctx._check(ctx.lib.avk_compare_packed_boot(ctx.handle, C.byref(st_pb), None, st.handle, C.byref(cfg), C.byref(ro), sums.ctypes.data_as(P(C.c_uint64)), C.byref(bs), None))
    assert same(res, plain) and np.array_equal(sums, plain.label_tallies)


@pytest.mark.parametrize("world", [2, 3])
def test_shards_add_up(job, world):
    import aardvark_amd
    ctx, pb = job["ctx"], job["pb"]
    lib = ctx.lib
    lib.avk_packed_shard_make.argtypes = [P(AvkPackedBatch), P(C.c_uint64), C.c_uint64, C.c_uint32, C.c_uint32, P(C.c_void_p)]
    lib.avk_packed_shard_batch.restype = P(AvkPackedBatch)
    lib.avk_packed_shard_batch.argtypes = [C.c_void_p]
    lib.avk_packed_shard_free.argtypes = [C.c_void_p]
    B = job["R"] + 1
    st, ids = pb.c_struct(), np.arange(pb.n_regions, dtype=np.uint64)
    total = np.zeros((1, B, TALLY_LEN), np.uint64)
    cfg, bs = AvkCompareConfig(50, 0, 0), AvkBootSpec(B, SEED)
    for rank in range(world):
        h = C.c_void_p()
        assert lib.avk_packed_shard_make(C.byref(st), ids.ctypes.data_as(P(C.c_uint64)), 0, rank, world, C.byref(h)) == 0
        sb = lib.avk_packed_shard_batch(h).contents
        status = np.full(int(sb.n_regions) + 1, -1, np.int32)
        ro = AvkResultBatch()
        ro.status = status.ctypes.data_as(P(C.c_int32))
        ctx._check(lib.avk_compare_packed_boot(ctx.handle, C.byref(sb), None, None, C.byref(cfg), C.byref(ro), None, C.byref(bs), total.ctypes.data_as(P(C.c_uint64))))
        lib.avk_packed_shard_free(h)
    assert np.array_equal(total, want_of(job, B))


def test_refusals_then_a_correct_solve(job, strata_job):
    """each refusal leaves `out` untouched and the context solves the next call correctly"""
    import aardvark_amd
    ctx, pb, st = job["ctx"], job["pb"], strata_job["st"]
    u64p = P(C.c_uint64)
    out = np.zeros(64, np.uint64)

    def after():
        assert not out.any()
        got = ctx.solve_packed(pb, res=ResultBatch(pb, sequences=False, group_metrics=False), boot=BootSpec(2, SEED))
        assert np.array_equal(np.asarray(got.status)[:len(job["want"].status)], job["want"].status) and np.array_equal(got.boot_tallies, want_of(job, 2))

    other = aardvark_amd.Context(0)
    try:
        ctx.set_option("emit_bp_groups", 1)
        rb = ctx.upload(pb)
        ctx.compare_resident(rb)
        cases = [("4097 replicates", AvkBootSpec(4097, 1), None, out.ctypes.data_as(u64p)), ("more than 16384 blocks", AvkBootSpec(4096, 1), st.handle, out.ctypes.data_as(u64p)),
                 ("boot_tallies missing", AvkBootSpec(4, 1), None, None), ("0 replicates", AvkBootSpec(0, 1), None, out.ctypes.data_as(u64p))]
        for text, bs, handle, o in cases:
            assert ctx.lib.avk_boot_tallies(ctx.handle, rb.handle, C.byref(bs), handle, o) == -1, text
            assert text in ctx.lib.avk_last_error(ctx.handle).decode(), text
            after()
        # a handle of another context
        n_bed, n_contigs, tree_off, start, end_max = cl.bed_trees(2, job["contigs"])
        foreign = other.upload_strata(n_bed, n_contigs, tree_off, start, end_max)
        bs = AvkBootSpec(4, 1)
        assert ctx.lib.avk_boot_tallies(ctx.handle, rb.handle, C.byref(bs), foreign.handle, out.ctypes.data_as(u64p)) == -1
        assert "another context" in ctx.lib.avk_last_error(ctx.handle).decode()
        foreign.free()
        after()
        rb.free()
        # emit_bp_groups off: AVK_E_STATE
        ctx.set_option("emit_bp_groups", 0)
        rb = ctx.upload(pb)
        ctx.compare_resident(rb)
        with pytest.raises(aardvark_amd.AardvarkAmdError, match="error -4.*emit_bp_groups"):
            ctx.boot_tallies(rb, BootSpec(4, 1), out=out.reshape(-1))
        rb.free()
        after()
        # the one-call form refuses the same specs before anything is queued
        with pytest.raises(aardvark_amd.AardvarkAmdError, match="4097 replicates"):
            ctx.solve_packed(pb, res=ResultBatch(pb, sequences=False, group_metrics=False), boot=BootSpec(4097, 1), boot_tallies=out)
        after()
    finally:
        ctx.set_option("emit_bp_groups", 0)
        other.close()


def test_the_tool(tmp_path, oracle):
    """aardvark_amd_compare --bootstrap 64 --bootstrap-seed 7 -s strat.tsv: summary.tsv byte-identical to the run without the option; summary_ci.tsv equal, cell by
    cell, to the restated interval rule (tests/test_boot_writer.py) on the restated replicates of the ORACLE's blocks under the host's label lists; byte-identical
    across --batch-regions 900, --devices 0,0 and the wide feed (the host route); another seed gives another file; -v names the route"""
    import subprocess
    import test_boot_writer as tw
    from aardvark_amd import feeder
    from test_feeder import cli_path, write_case_files, write_text
    p, contig, want_batch = write_case_files(tmp_path, 2500, 1_200_000)
    rng = np.random.default_rng(8)
    names = ["s%02d" % i for i in range(6)]
    for i, name in enumerate(names):
        iv = sorted((int(s), int(s) + int(w)) for s, w in zip(rng.integers(0, 1_190_000, 30 + 10 * i), rng.integers(200, 40_000, 30 + 10 * i)))
        write_text(str(tmp_path / (name + ".bed")), "".join("chr20\t%d\t%d\n" % x for x in iv))
    write_text(str(tmp_path / "strat.tsv"), "".join("%s\t%s.bed\n" % (n, n) for n in names))
    strat = feeder.Stratifications(str(tmp_path / "strat.tsv"))
    genome = feeder.Genome(p["fa"])
    feed = feeder.feed_compare(p["t"], p["q"], p["bed"], genome, enable_trimming=False)
    batch = feed.batch
    n = batch.n_regions
    res = oracle_lib.compare_batch(oracle, batch, genome.contigs(), threads=CPUS)
    off, idx = strat.batch_labels(genome, batch)
    members = np.zeros((len(names), n), bool)
    members[idx, np.repeat(np.arange(n), np.diff(np.asarray(off).astype(np.int64)))] = True
    B, level = 64, 95
    w = boot_lib.weights(7, batch.contig_idx, batch.start, np.arange(B))
    reps = boot_lib.expected(np.asarray(res.group_metrics).reshape(n, WORDS), np.asarray(res.status) == 0, w, list(members))
    assert reps[1:].any()

    def run(name, *extra):
        out = str(tmp_path / name)
        r = subprocess.run([cli_path(), "-r", p["fa"], "-t", p["t"], "-q", p["q"], "-b", p["bed"], "-o", out, "--disable-variant-trimming", "-s", str(tmp_path / "strat.tsv"), "-v"]
                           + list(extra), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        ci = os.path.join(out, "summary_ci.tsv")
        return open(os.path.join(out, "summary.tsv")).read(), open(ci).read() if os.path.exists(ci) else None, r.stderr

    plain, none, _ = run("plain")
    assert none is None
    boot = ("--bootstrap", str(B), "--bootstrap-seed", "7")
    summary, ci, err = run("boot", *boot)
    assert summary == plain and "avk_compare_packed_boot" in err
    # every cell against the restatement
    head, rows = tw.read(os.path.join(str(tmp_path / "boot"), "summary_ci.tsv"))
    shead, srows = tw.read(os.path.join(str(tmp_path / "boot"), "summary.tsv"))
    assert [r[:5] for r in rows] == [r[:5] for r in srows] and len(rows) > 10
    scope = {"ALL": 0, **{name: 1 + l for l, name in enumerate(names)}}
    some = 0
    for r in rows:
        per_rep = [tw.ratios(reps[scope[r[2]], b], r[1], r[4]) for b in range(B)]
        for q in range(3):
            lo, hi, m = tw.interval([x[q] for x in per_rep if x[q] is not None], level)
            if m == 0:
                assert (r[6 + 3 * q], r[7 + 3 * q]) == ("", "")
            else:
                assert (float(r[6 + 3 * q]), float(r[7 + 3 * q])) == (lo, hi), (r[:5], q)
                some += lo < hi
        assert int(r[14]) == tw.interval([x[2] for x in per_rep if x[2] is not None], level)[2]
    assert some > 10
    for name, extra in (("batches", ("--batch-regions", "900")), ("two", ("--devices", "0,0")), ("wide", ("--batch-form", "wide"))):
        s2, ci2, err2 = run(name, *boot, *extra)
        assert s2 == plain and ci2 == ci, name
        assert ("avk_boot_tallies_host" in err2) == (name == "wide")
    _, other, _ = run("seed8", "--bootstrap", str(B), "--bootstrap-seed", "8")
    assert other != ci and other.split("\n")[0] == ci.split("\n")[0]
    _, l99, _ = run("l99", *boot, "--bootstrap-level", "99")
    assert l99 != ci
    strat.close()
