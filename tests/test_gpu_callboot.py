"""Bootstrap replicates of the per-call blocks on a real MI355X (avk_callboot_tally_kernel): both families, the resident forms against the restatement of the rule
(tests/callboot_lib.py: no code under test) on the ORACLE's per-call outputs, conservation against Context.boot_tallies and between the families, scopes from a
strata handle, slices, replicate counts around a launch's, every upload form, the host routes bit for bit, and the refusals.  Every comparison is exact.

Slices of 1, 63, 64 and 65 regions straddle the wave and the kernel's tile alike (T = 64: T - 1, T, T + 1), and 2 T + 1; replicate counts straddle R = Context.callboot_block(n_keys).  The
fixture's escaped batch holds regions of 510, 511 and 555 calls: more than the 256 records of a piece."""
import ctypes as C
import os

import numpy as np
import pytest

import callboot_lib as cbl
import context_lib as cl
import kind_lib
import size_lib
from aardvark_amd import BootSpec, CompactBatch, ContextSpec, PackedBatch, SizeSpec, kind_boot_tallies_host, size_boot_tallies_host
from aardvark_amd._abi import N_GROUPS

pytestmark = pytest.mark.gpu
CPUS = min(os.cpu_count() or 1, 16)
u64p = C.POINTER(C.c_uint64)
SEED, T = 4242, 64
KIND, DEFAULT, ONE, FIFTEEN = cbl.KIND, cbl.size(size_lib.DEFAULT), cbl.size((2,)), cbl.size(size_lib.FIFTEEN)
FAMILIES = pytest.mark.parametrize("family", [KIND, DEFAULT], ids=["kind", "size"])


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
    per_region = np.asarray(j["batch"].t_cnt, np.int64) + np.asarray(j["batch"].q_cnt, np.int64)
    assert ((per_region > 256) & j["solved"]).sum() >= 2, "solved regions of more calls than a piece holds"
    j.update(ctx=ctx, cb=cb, pe=pe, pp=pp, n=j["batch"].n_regions, n_plain=j["plain"].n_regions,
             keys=(np.asarray(j["batch"].contig_idx, np.uint64), np.asarray(j["batch"].start, np.uint64)))
    yield j
    ctx.close()


def want_of(job, family, B, members=None, lo=0, hi=None, seed=SEED):
    return cbl.expected(job["calls"], job["n"], members, B, seed, family, keys=job["keys"], lo=lo, hi=hi)


def tallies(ctx, rb, family, B, strata=None, out=None, seed=SEED):
    if family == KIND:
        return ctx.kind_boot_tallies(rb, BootSpec(B, seed), strata=strata, out=out)
    return ctx.size_boot_tallies(rb, SizeSpec(list(family[1])), BootSpec(B, seed), strata=strata, out=out)


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


def resident(ctx, src, family, B, strata=None):
    rb = ctx.upload(src)
    try:
        ctx.compare_resident(rb)
        return tallies(ctx, rb, family, B, strata=strata)
    finally:
        rb.free()


def test_block_sizes(job):
    """R follows from the LDS the runtime grants a launch (less 1 KB for the kernel's static words): in 160 KB 11 replicates of the kinds, 6 of sixteen bins and the
    lane teams' 18 for the default bins; in 64 KB 4, 2 and 7 — as Context.label_block() is 71 or 28"""
    ctx = job["ctx"]
    got = [ctx.callboot_block(k) for k in (9, 5, 16, 2)]
    lib = cbl.load()
    assert got in ([int(lib.callboot_emu_reps(k, lds - 1024)) for k in (9, 5, 16, 2)] for lds in (160 * 1024, 64 * 1024)) and got in ([11, 18, 6, 18], [4, 7, 2, 17])
    assert ctx.callboot_block(0) == 0 and ctx.callboot_block(17) == 0


@FAMILIES
def test_resident_scope_0(job, family):
    """the block equals the restatement; a second call doubles `out`; words of other scopes and of replicates >= B are untouched"""
    ctx, B, K = job["ctx"], 3, cbl.n_keys_of(family)
    want = want_of(job, family, B)
    rb = ctx.upload(job["pe"])
    try:
        ctx.compare_resident(rb)
        out = np.zeros((2, B, K, N_GROUPS, 14), np.uint64)
        out[1] = 7
        tallies(ctx, rb, family, B, out=out)
        assert np.array_equal(out[:1], want), np.argwhere(out[:1] != want)[:8]
        assert (out[1] == 7).all()
        tallies(ctx, rb, family, B, out=out)
        assert np.array_equal(out[:1], 2 * want) and (out[1] == 7).all()
        # a caller's array of B + 2 replicates' room behind a call with B: as one scope of B replicates the call writes the first B blocks only
        wide = np.full((B + 2) * K * N_GROUPS * 14, 9, np.uint64)
        ctx._check(ctx.lib.avk_kind_boot_tallies(ctx.handle, rb.handle, C.byref(BootSpec(B, SEED).c_struct()), None, wide.ctypes.data_as(u64p)) if family == KIND else
                   ctx.lib.avk_size_boot_tallies(ctx.handle, rb.handle, C.byref(SizeSpec(list(family[1])).c_struct()), C.byref(BootSpec(B, SEED).c_struct()), None,
                                                 wide.ctypes.data_as(u64p)))
        words = B * K * N_GROUPS * 14
        assert np.array_equal(wide[:words] - np.uint64(9), want.reshape(-1)) and (wide[words:] == 9).all()
    finally:
        rb.free()
    assert all(want[0, b].any() for b in range(B)) and not np.array_equal(want[0, 0], want[0, 1])


def test_conservation_across_kernels(job):
    """replicate b summed over its keys is the 14 GT / HAP / WEIGHTED_HAP fields of every group of boot_tallies' replicate b for the same seed; the size family
    summed over its bins is the kind family summed over its kinds"""
    ctx, B = job["ctx"], 13
    ctx.set_option("emit_bp_groups", 1)
    rb = ctx.upload(job["pe"])
    try:
        ctx.compare_resident(rb)
        reps = ctx.boot_tallies(rb, BootSpec(B, SEED))
        kinds = tallies(ctx, rb, KIND, B)
        sizes = tallies(ctx, rb, DEFAULT, B)
    finally:
        rb.free()
        ctx.set_option("emit_bp_groups", 0)
    assert np.array_equal(kinds.sum(axis=2), size_lib.tally14(reps)) and kinds.any()
    assert np.array_equal(sizes.sum(axis=2), kinds.sum(axis=2))
    assert np.array_equal(kinds, want_of(job, KIND, B)) and np.array_equal(sizes, want_of(job, DEFAULT, B))


@pytest.fixture(scope="module")
def strata_job(job):
    """test_gpu_kind.py's handle: 5 BED labels (label 0: every contig whole), 28 labels without intervals and the 16 default context labels (33 .. 48: the second
    mask word); which regions each holds"""
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
    members = size_lib.members_of_lists(off, idx, L, job["n"])
    assert not members[5:33].any() and members[1:5].any() and members[33:].any()
    yield dict(st=st, members=list(members), L=L, lists=(L, off, idx))
    st.free()


@FAMILIES
def test_scopes_from_a_strata_handle_and_the_host_route(job, strata_job, family):
    """a whole-contig label, empty labels, interval labels and context labels in the second mask word; the GPU equals the host route bit for bit"""
    ctx, st, members, L = job["ctx"], strata_job["st"], strata_job["members"], strata_job["L"]
    B = 2
    got = resident(ctx, job["pe"], family, B, strata=st)
    want = want_of(job, family, B, members=members)
    assert got.shape == (1 + L, B, cbl.n_keys_of(family), N_GROUPS, 14) and np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert np.array_equal(got[1], got[0]) and not got[6:34].any() and sum(int(got[1 + l].any()) for l in range(33, L)) >= 2 and got[2:6].any()
    if family == KIND:
        host = kind_boot_tallies_host(job["batch"], job["want"], BootSpec(B, SEED), labels=strata_job["lists"], threads=CPUS)
    else:
        host = size_boot_tallies_host(job["batch"], job["want"], SizeSpec(list(family[1])), BootSpec(B, SEED), labels=strata_job["lists"], threads=CPUS)
    assert np.array_equal(got, host)


@pytest.mark.parametrize("n", [1, T - 1, T, T + 1, 2 * T + 1])
def test_slices(job, n):
    """a slice's replicates are the whole's restricted to its regions: weights depend on contig and start alone"""
    lo = 3
    got = resident(job["ctx"], packed_slice(job["pp"], lo, lo + n), KIND, 2)
    want = want_of(job, KIND, 2, lo=lo, hi=lo + n)
    assert np.array_equal(got, want) and want.any()


def test_slices_add_up_to_the_whole(job):
    ctx, pp, n = job["ctx"], job["pp"], job["n_plain"]
    total = np.zeros((1, 3, 5, N_GROUPS, 14), np.uint64)
    for lo, hi in ((0, T), (T, 2 * T + 1), (2 * T + 1, n)):
        total += resident(ctx, packed_slice(pp, lo, hi), DEFAULT, 3)
    assert np.array_equal(total, want_of(job, DEFAULT, 3, hi=n)) and np.array_equal(total, resident(ctx, pp, DEFAULT, 3))


@pytest.mark.parametrize("family", [KIND, DEFAULT, ONE, FIFTEEN], ids=["kind", "size5", "size2", "size16"])
def test_replicate_counts_around_a_launch(job, family):
    """B = 1, R, R + 1 and 2 R + 1 for the family's R; a spec of 1 edge and one of 15 edges, the latter with a smaller R"""
    ctx = job["ctx"]
    R = ctx.callboot_block(cbl.n_keys_of(family))
    assert R in {KIND: (11, 4), DEFAULT: (18, 7), ONE: (18, 17), FIFTEEN: (6, 2)}[family]
    rb = ctx.upload(job["pe"])
    try:
        ctx.compare_resident(rb)
        got = {B: tallies(ctx, rb, family, B) for B in (1, R, R + 1, 2 * R + 1)}
    finally:
        rb.free()
    want = want_of(job, family, 2 * R + 1)
    for B, g in got.items():
        assert np.array_equal(g, want[:, :B]), (B, np.argwhere(g != want[:, :B])[:8])
    assert all(want[0, b].any() for b in range(2 * R + 1))


@pytest.mark.parametrize("form", ["wide", "compact", "packed", "packed + escapes"])
def test_upload_forms(job, form):
    ctx = job["ctx"]
    whole = form != "packed"
    src = {"wide": job["batch"], "compact": job["cb"], "packed": job["pp"], "packed + escapes": job["pe"]}[form]
    for family in (KIND, DEFAULT):
        got = resident(ctx, src, family, 2)
        want = want_of(job, family, 2, hi=None if whole else job["n_plain"])
        assert np.array_equal(got, want), np.argwhere(got != want)[:8]


def test_refusals_then_a_correct_call(job):
    """each refusal leaves `out` untouched, and the context serves the next call correctly"""
    ctx, pp, lib = job["ctx"], job["pp"], job["ctx"].lib
    out = np.zeros((1, 2, 9, N_GROUPS, 14), np.uint64)
    o = out.ctypes.data_as(u64p)
    err = lambda: lib.avk_last_error(ctx.handle).decode()
    spec = lambda B: C.byref(BootSpec(B, SEED).c_struct())
    import aardvark_amd
    other = aardvark_amd.Context(0)
    rb = ctx.upload(pp)
    try:
        assert lib.avk_kind_boot_tallies(ctx.handle, rb.handle, spec(2), None, o) == -4 and "avk_compare_resident has solved" in err()  # unsolved: AVK_E_STATE
        ctx.compare_resident(rb)
        assert lib.avk_kind_boot_tallies(ctx.handle, rb.handle, spec(2), None, None) == -1 and "kind_boot_tallies missing" in err()
        ss = SizeSpec().c_struct()
        assert lib.avk_size_boot_tallies(ctx.handle, rb.handle, C.byref(ss), spec(2), None, None) == -1 and "size_boot_tallies missing" in err()
        assert lib.avk_kind_boot_tallies(ctx.handle, rb.handle, spec(0), None, o) == -1 and "replicates" in err()
        assert lib.avk_kind_boot_tallies(ctx.handle, rb.handle, spec(4097), None, o) == -1 and "replicates" in err()
        n_bed, n_contigs, tree_off, start, end_max = cl.bed_trees(5, job["contigs"])
        foreign = other.upload_strata(n_bed, n_contigs, tree_off, start, end_max)
        assert lib.avk_kind_boot_tallies(ctx.handle, rb.handle, spec(2), foreign.handle, o) == -1  # a handle of another context
        foreign.free()
        mine = ctx.upload_strata(n_bed, n_contigs, tree_off, start, end_max)
        wide = SizeSpec(list(size_lib.FIFTEEN)).c_struct()
        assert lib.avk_size_boot_tallies(ctx.handle, rb.handle, C.byref(wide), spec(4096), mine.handle, o) == -1 and "blocks" in err()  # 6 x 4096 x 16 over the cap
        mine.free()
        assert not out.any()
        assert np.array_equal(ctx.kind_boot_tallies(rb, BootSpec(2, SEED)), want_of(job, KIND, 2, hi=job["n_plain"]))
    finally:
        rb.free()
        other.close()
