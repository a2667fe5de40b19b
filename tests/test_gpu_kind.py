"""Per-call tallies by call kind on a real MI355X (avk_kind_tally_kernel): the resident form, the one-call form, scopes from a strata handle, slices, every upload
form, shards and the refusals, against the restatement of the rule (tests/kind_lib.py: no code under test) on the ORACLE's per-call outputs, and the conservation
law against the oracle's tally, the library's own label sums and its size bins.  Every comparison is exact.

Slices straddle the wave (1, 63, 64, 65 regions) and the kernel's regions-per-workgroup constant T = Context.kind_block().  Which regions a label of a strata handle
holds is asked of Context.strata_region_labels, as tests/test_gpu_size.py does."""
import ctypes as C
import os

import numpy as np
import pytest

import context_lib as cl
import kind_lib
import size_lib
from aardvark_amd import CompactBatch, ContextSpec, PackedBatch, ResultBatch, SizeSpec
from aardvark_amd._abi import N_GROUPS, AvkCompareConfig, AvkPackedBatch, AvkResultBatch

pytestmark = pytest.mark.gpu
CPUS = min(os.cpu_count() or 1, 16)
P = C.POINTER
u64p = P(C.c_uint64)


@pytest.fixture(scope="module")
def job(oracle):
    """one context, one call set, the oracle's results: shared, never changed"""
    import aardvark_amd
    j = kind_lib.build_case(oracle, threads=CPUS)
    ctx = aardvark_amd.Context(0)
    ctx.set_option("lane_min_regions", 0)
    ctx.set_option("lane_min_batch", 0)
    ctx.upload_reference(j["contigs"])
    cb = CompactBatch.from_region_batch(j["batch"])
    pe = PackedBatch.from_compact(cb, escapes=True)
    assert pe.c_escapes() is not None
    pp = PackedBatch.from_compact(CompactBatch.from_region_batch(j["plain"]))
    j.update(ctx=ctx, cb=cb, pe=pe, pp=pp, T=ctx.kind_block(), n=j["batch"].n_regions, n_plain=j["plain"].n_regions)
    yield j
    ctx.close()


def want_of(job, lo=0, hi=None, members=None):
    return kind_lib.expected(job["calls"], job["n"], members, lo=lo, hi=hi)


def resident(ctx, src, strata=None, out=None):
    rb = ctx.upload(src)
    try:
        ctx.compare_resident(rb)
        return ctx.kind_tallies(rb, strata=strata, out=out)
    finally:
        rb.free()


def packed_slice(pb, lo, hi):
    """regions [lo, hi) of a packed batch without escapes as a packed batch of their own"""
    cnt = pb.t_cnt.astype(np.int64) + pb.q_cnt
    v0, v1 = int(cnt[:lo].sum()), int(cnt[:hi].sum())
    alen = pb.a0_len.astype(np.int64) + pb.a1_len
    a0, a1 = int(alen[:v0].sum()), int(alen[:v1].sum())
    reg, var = np.s_[lo:hi], np.s_[v0:v1]
    return PackedBatch(contig_idx=pb.contig_idx[reg], start=pb.start[reg], len=pb.len[reg], t_cnt=pb.t_cnt[reg], q_cnt=pb.q_cnt[reg], var_rel_pos=pb.var_rel_pos[var],
                       var_type_zyg=pb.var_type_zyg[var], a0_len=pb.a0_len[var], a1_len=pb.a1_len[var],
                       var_raw_space=None if pb.var_raw_space is None else pb.var_raw_space[var], allele_bytes=pb.allele_bytes[a0:a1])


def same(a, b):
    return np.array_equal(a.region_packed, b.region_packed) and np.array_equal(a.var_packed, b.var_packed) and np.array_equal(a.tally, b.tally)


def test_kind_block(job):
    assert job["T"] == 256


def test_resident_scope_0(job):
    """the sums equal the restatement's; a second call doubles `out`; words of other scopes are untouched; the sum over the kinds is the oracle's tally and the
    library's size bins summed"""
    ctx = job["ctx"]
    want = want_of(job)
    rb = ctx.upload(job["pe"])
    try:
        ctx.compare_resident(rb)
        out = np.zeros((3, 9, N_GROUPS, 14), np.uint64)
        out[1:] = 7
        ctx.kind_tallies(rb, out=out)
        assert np.array_equal(out[:1], want), np.argwhere(out[:1] != want)[:8]
        assert (out[1:] == 7).all()
        ctx.kind_tallies(rb, out=out)
        assert np.array_equal(out[:1], 2 * want) and (out[1:] == 7).all()
        sizes = ctx.size_tallies(rb, SizeSpec())
    finally:
        rb.free()
    n = job["n"]
    tally = np.asarray(job["want"].group_metrics).reshape(n, N_GROUPS, 22)[job["solved"]].astype(np.uint64).sum(axis=0)
    assert np.array_equal(want[0].sum(axis=0), tally[:, :14]) and tally[:, :14].any()
    assert np.array_equal(want[0].sum(axis=0), sizes[0].sum(axis=0)), "summed over the kinds the block is size_tallies summed over the bins"
    assert all(want[0, k, 0].any() for k in range(6))


@pytest.fixture(scope="module")
def strata_job(job):
    """a handle of 5 BED labels (label 0: every contig whole), 28 labels without intervals and the 16 default context labels (33 .. 48: the second mask word);
    which regions each holds"""
    ctx, contigs = job["ctx"], job["contigs"]
    n_bed, n_contigs, tree_off, start, end_max = cl.bed_trees(5, contigs)
    tree_off = np.concatenate([tree_off, np.full(28 * n_contigs, tree_off[-1], np.uint64)])
    spec = ContextSpec()
    st = ctx.upload_strata(n_bed + 28, n_contigs, tree_off, start, end_max, context=spec)
    L = st.n_labels
    assert L == 33 + spec.n_labels
    rb = ctx.upload(job["pe"])
    off, idx = ctx.strata_region_labels(rb, st)
    rb.free()
    n = job["n"]
    members = size_lib.members_of_lists(off, idx, L, n)
    has_calls = (np.asarray(job["batch"].t_cnt) + np.asarray(job["batch"].q_cnt)) > 0
    assert np.array_equal(members[0] & job["solved"], has_calls & job["solved"]) and not members[5:33].any() and members[1:5].any() and members[33:].any()
    yield dict(st=st, members=list(members), L=L)
    st.free()


def test_scopes_from_a_strata_handle(job, strata_job):
    """a whole-contig label, empty labels, interval labels and context labels in the second mask word (17 launches of three scopes); the conservation law against
    label_tallies_strata and size_tallies"""
    ctx, st, members, L = job["ctx"], strata_job["st"], strata_job["members"], strata_job["L"]
    ctx.set_option("emit_bp_groups", 1)
    rb = ctx.upload(job["pe"])
    try:
        ctx.compare_resident(rb)
        got = ctx.kind_tallies(rb, strata=st)
        sums = ctx.label_tallies_strata(rb, st)
        sizes = ctx.size_tallies(rb, SizeSpec(), strata=st)
    finally:
        rb.free()
        ctx.set_option("emit_bp_groups", 0)
    want = want_of(job, members=members)
    assert got.shape == (1 + L, 9, N_GROUPS, 14) and np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert np.array_equal(got[1], got[0]) and not got[6:34].any() and sum(int(got[1 + l].any()) for l in range(33, L)) >= 2 and got[2:6].any()
    assert np.array_equal(got[1:].sum(axis=1), size_lib.tally14(sums)), "the sum over the kinds is the label's tally"
    assert np.array_equal(got.sum(axis=1), sizes.sum(axis=1))


@pytest.mark.parametrize("n", ["1", "63", "64", "65", "T-1", "T", "T+1", "2T+1"])
def test_slices(job, n):
    T = job["T"]
    n = {"T-1": T - 1, "T": T, "T+1": T + 1, "2T+1": 2 * T + 1}.get(n) or int(n)
    lo = 3
    got = resident(job["ctx"], packed_slice(job["pp"], lo, lo + n))
    want = want_of(job, lo=lo, hi=lo + n)
    assert np.array_equal(got, want) and want.any()


@pytest.mark.parametrize("form", ["wide", "compact", "packed", "packed_source=0", "packed + escapes"])
def test_upload_forms(job, form):
    ctx = job["ctx"]
    whole = form in ("wide", "compact", "packed + escapes")
    src = {"wide": job["batch"], "compact": job["cb"], "packed": job["pp"], "packed_source=0": job["pp"], "packed + escapes": job["pe"]}[form]
    ctx.set_option("packed_source", 0 if form == "packed_source=0" else 1)
    try:
        got = resident(ctx, src)
    finally:
        ctx.set_option("packed_source", 1)
    want = want_of(job, hi=None if whole else job["n_plain"])
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    # the hand-written calls (a -> g, C -> a, an N ALT, a -> A) lie in the plain part: every form reads their bytes
    assert job["hand_first"] + 6 <= job["n_plain"]


def test_one_call_form(job, strata_job):
    """the block is the resident form's and the restatement's; results and tally bit-identical to a plain solve_packed"""
    ctx, pe, st, members = job["ctx"], job["pe"], strata_job["st"], strata_job["members"]
    new = lambda: ResultBatch(pe, sequences=False, group_metrics=False, packed="only")
    bare = ctx.solve_packed(pe, res=new())
    alone = ctx.solve_packed(pe, res=new(), kinds=True)
    assert same(alone, bare) and np.array_equal(alone.kind_tallies, want_of(job)) and bare.tally.any()
    assert np.array_equal(alone.tally[:N_GROUPS * 22].reshape(N_GROUPS, 22)[:, :14], alone.kind_tallies[0].sum(axis=0))
    got = ctx.solve_packed(pe, res=new(), strata=st, kinds=True)
    assert same(got, bare) and np.array_equal(got.kind_tallies, want_of(job, members=members))
    assert np.array_equal(got.kind_tallies, resident(ctx, pe, strata=st))
    twice = ctx.solve_packed(pe, res=new(), kinds=True, kind_tallies=alone.kind_tallies.copy())
    assert np.array_equal(twice.kind_tallies, 2 * want_of(job))
    assert not hasattr(bare, "kind_tallies")


@pytest.mark.parametrize("world", [2])
def test_shards_add_up(job, world):
    """the hash-sharded halves of the batch add up to the whole"""
    ctx, pb = job["ctx"], job["pp"]
    lib = ctx.lib
    lib.avk_packed_shard_make.argtypes = [P(AvkPackedBatch), u64p, C.c_uint64, C.c_uint32, C.c_uint32, P(C.c_void_p)]
    lib.avk_packed_shard_batch.restype = P(AvkPackedBatch)
    lib.avk_packed_shard_batch.argtypes = [C.c_void_p]
    lib.avk_packed_shard_free.argtypes = [C.c_void_p]
    st, ids = pb.c_struct(), np.arange(pb.n_regions, dtype=np.uint64)
    total = np.zeros((1, 9, N_GROUPS, 14), np.uint64)
    cfg = AvkCompareConfig(50, 0, 0)
    for rank in range(world):
        h = C.c_void_p()
        assert lib.avk_packed_shard_make(C.byref(st), ids.ctypes.data_as(u64p), 0, rank, world, C.byref(h)) == 0
        sb = lib.avk_packed_shard_batch(h).contents
        assert 0 < int(sb.n_regions) < pb.n_regions
        status = np.full(int(sb.n_regions) + 1, -1, np.int32)
        ro = AvkResultBatch()
        ro.status = status.ctypes.data_as(P(C.c_int32))
        ctx._check(lib.avk_compare_packed_kind(ctx.handle, C.byref(sb), None, None, C.byref(cfg), C.byref(ro), total.ctypes.data_as(u64p)))
        lib.avk_packed_shard_free(h)
    assert np.array_equal(total, want_of(job, hi=job["n_plain"]))


def test_refusals_then_a_correct_solve(job):
    """each refusal leaves `out` untouched and the context solves the next call correctly"""
    import aardvark_amd
    ctx, pp = job["ctx"], job["pp"]
    out = np.zeros((1, 9, N_GROUPS, 14), np.uint64)
    rb = ctx.upload(pp)
    try:
        assert ctx.lib.avk_kind_tallies(ctx.handle, rb.handle, None, out.ctypes.data_as(u64p)) == -4  # not solved yet: AVK_E_STATE
        assert "avk_compare_resident has solved" in ctx.lib.avk_last_error(ctx.handle).decode()
        ctx.compare_resident(rb)
        assert ctx.lib.avk_kind_tallies(ctx.handle, rb.handle, None, None) == -1 and "kind_tallies missing" in ctx.lib.avk_last_error(ctx.handle).decode()
        assert not out.any()
        assert np.array_equal(ctx.kind_tallies(rb), want_of(job, hi=job["n_plain"]))
    finally:
        rb.free()
    cfg, ro = AvkCompareConfig(50, 0, 0), ResultBatch(pp, sequences=False, group_metrics=False)
    pb, cro = pp.c_struct(), ro.c_struct()
    assert ctx.lib.avk_compare_packed_kind(ctx.handle, C.byref(pb), None, None, C.byref(cfg), C.byref(cro), None) == -1
    ctx.set_option("device_pack", 0)
    try:
        with pytest.raises(aardvark_amd.AardvarkAmdError, match="error -4.*device_pack"):
            ctx.solve_packed(pp, res=ResultBatch(pp, sequences=False, group_metrics=False), kinds=True, kind_tallies=out)
    finally:
        ctx.set_option("device_pack", 1)
    assert not out.any()
    with pytest.raises(ValueError):
        ctx.solve_packed(pp, kinds=True, size=SizeSpec())
    got = ctx.solve_packed(pp, res=ResultBatch(pp, sequences=False, group_metrics=False), kinds=True)
    assert np.array_equal(np.asarray(got.status)[:job["n_plain"]], job["want"].status[:job["n_plain"]]) and np.array_equal(got.kind_tallies, want_of(job, hi=job["n_plain"]))
