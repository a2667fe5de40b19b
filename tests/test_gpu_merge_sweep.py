"""One pair solve decided under several strategies on the GPU (avk_merge_packed_sweep; the kernel of aardvark_amd/csrc/avk_mergesweep.inl and the count kernel once per
config behind it).

What a sweep has to equal never comes from the sweep: every config's slice is compared with the EXISTING single-config call on the same context
(merge_multi_batch(ctx, pm, cfg, counts=...)), every block with avk_merge_counts_esc on that call's results (merge_counts), and for one config per k with the C
oracle's pairs under the restated rule (oracle/merge_oracle.py).  The jobs are those of tests/test_gpu_merge_counts.py: synth.config_genome_merge at scale 0.0008
with 2 to 9 call sets, its first 1, 255, 256 and 257 regions (the edges of the 256-lane launch) and the escaped job of tests/escapes_lib.py."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

import aardvark_amd
import escapes_lib as el
import mergecount_emu_lib as mc
import oracle_lib
from aardvark_amd import synth
from aardvark_amd._abi import AvkPackedEscapes
from aardvark_amd.api import AardvarkAmdError
from aardvark_amd.merge import (AvkMergeConfig, AvkPackedMultiBatch, MergeConfig, MergeResult, MultiBatch, PackedMultiBatch, counts_in_lds, counts_on_device, merge_counts, merge_counts_len,
                                merge_multi_batch, merge_multi_batch_sweep)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import merge_oracle as mo  # noqa: E402

pytestmark = pytest.mark.gpu
FOUR = [MergeConfig(), MergeConfig(no_conflict_enabled=True), MergeConfig(majority_voting_enabled=True),
        MergeConfig(no_conflict_enabled=True, majority_voting_enabled=True, conflict_selection=1)]  # exact, no_conflict, majority, all + select 1


def eight(k):
    """eight configs: the four strategies, each without and with a ConflictSelection (the first and the last input in turn); the last one is "all" """
    return [MergeConfig(no_conflict_enabled=nc, majority_voting_enabled=mv, conflict_selection=cs)
            for cs, (nc, mv) in [(None, (False, False)), (0, (True, False)), (None, (False, True)), (k - 1, (False, False)), (None, (True, False)), (0, (False, True)), (None, (True, True)),
                                 (k - 1, (True, True))]]


@functools.lru_cache(maxsize=None)
def job(k, regions=None):
    """(contigs, MultiBatch) of the small job with k call sets; regions: its first so many MultiRegions"""
    contigs, mb = synth.config_genome_merge(scale=0.0008, k=k, threads=4)
    if regions is not None:
        mb = el.reordered_multi(mb, np.arange(regions))
    return contigs, mb


@pytest.fixture(scope="module")
def ctx():
    c = aardvark_amd.Context(0)
    try:
        c.upload_reference(job(3)[0])  # (the contigs of the small job do not depend on k)
        yield c
    finally:
        c.close()


def same(a, b):
    return np.array_equal(a.status, b.status) and np.array_equal(a.classification, b.classification) and np.array_equal(a.members, b.members)


def solved_calls(pm, status):
    _, cnt, _, _, _ = pm._wide_fields()
    return int(cnt.reshape(-1, pm.n_inputs)[status == 0].sum())


def swept(ctx, pm, configs, on_device=True, start=None):
    """one sweep with counters, every config checked against the single call with counters and the host's count of ITS results -> (single results, single blocks)"""
    n = merge_counts_len(ctx.lib, pm.n_inputs)
    counts = np.zeros((len(configs), n), np.uint64) if start is None else start.copy()
    got = merge_multi_batch_sweep(ctx, pm, configs, counts=counts)
    assert counts_on_device(ctx) == on_device and len(got) == len(configs)
    singles, blocks = [], []
    for c, cfg in enumerate(configs):
        block = np.zeros(n, np.uint64)
        one = merge_multi_batch(ctx, pm, cfg, counts=block)
        assert counts_on_device(ctx) == on_device
        assert same(got[c], one), c
        assert np.shares_memory(got[c].status, got[0].status)  # one status array for all of them
        assert np.array_equal(block, merge_counts(ctx.lib, pm, one))
        assert np.array_equal(counts[c] if start is None else counts[c] - start[c], block), c
        assert int(block.sum()) == solved_calls(pm, one.status)
        singles.append(one), blocks.append(block)
    return singles, blocks


def oracle_merge(oracle, mb, contigs, cfg, threads=4):
    """solve_merge_region for a MultiBatch of any number of inputs: pairs from the C oracle, the decision from the restated rule (oracle/merge_oracle.py: classify) —
    tests/test_merge_shard.py's helper, for every k and config"""
    import bench
    k, n = mb.n_inputs, mb.n_regions
    ppr = k * (k - 1) // 2
    st, ex = oracle_lib.optimize_pairs(oracle, bench.pair_batch_of(mb), contigs, cfg.max_branch_factor, threads=threads)
    st, ex = np.asarray(st).reshape(n, ppr), np.asarray(ex).reshape(n, ppr)
    index = {(i, j): p for p, (i, j) in enumerate((i, j) for i in range(k) for j in range(i + 1, k))}
    cnt = mb.in_cnt.astype(np.int64).reshape(n, k)
    unknown = np.zeros(n, bool)
    np.logical_or.at(unknown, np.repeat(np.arange(n), cnt.sum(axis=1)), mb.var_zyg == 0)
    status, cls, members = np.zeros(n, np.int32), np.zeros(n, np.uint8), np.zeros(n, np.uint64)
    code = {"different": 0, "identical": 1, "no_conflict": 2, "majority": 3, "conflict_select": 4}
    for m in range(n):
        if unknown[m] or st[m].any():
            status[m] = 6 if unknown[m] else int(st[m][np.flatnonzero(st[m])[0]])
            continue
        got = mo.classify(cnt[m].tolist(), lambda i, j: ex[m, index[(i, j)]], cfg.no_conflict_enabled, cfg.majority_voting_enabled, cfg.conflict_selection)
        cls[m] = code[got[0]]
        members[m] = 0 if len(got) == 1 else (got[1] if got[0] == "conflict_select" else sum(1 << i for i in got[1]))
    return MergeResult(status, cls, members, k)


@pytest.mark.parametrize("regions", [1, 255, 256, 257, None])
def test_sweep_at_the_edges_of_the_launch(ctx, regions):
    _, mb = job(3, regions)
    assert regions is None or mb.n_regions == regions
    singles, blocks = swept(ctx, PackedMultiBatch.from_multi(mb), FOUR)
    if regions is None:
        assert mb.n_regions > 4 * 256 and {1, 3} <= set(singles[2].classification.tolist()) and 4 in singles[3].classification.tolist()
        assert len({b.tobytes() for b in blocks}) == 4  # the four strategies do count differently on this job


@pytest.mark.parametrize("which", ["2", "last_in_lds", "first_beyond", "8", "9"])
def test_sweep_of_eight_for_every_route(ctx, oracle, which):
    """k = 2, the largest k whose block the count kernel keeps in LDS, the next one (reduced within the wave), DP_MERGE_KMAX = 8, and 9 (no device route: one solve
    through the host route, avk_merge_classify_sweep, the host's count per config)"""
    inside = [k for k in range(2, 9) if counts_in_lds(ctx, k)]
    assert inside == list(range(2, inside[-1] + 1)) and 3 <= inside[-1] < 8
    k = {"2": 2, "last_in_lds": inside[-1], "first_beyond": inside[-1] + 1, "8": 8, "9": 9}[which]
    contigs, mb = job(k, None if k <= 3 else (300 if k == 9 else 1500))
    pm = PackedMultiBatch.from_multi(mb)
    configs = eight(k)
    singles, blocks = swept(ctx, pm, configs, on_device=k <= 8)
    everything = singles[-1]
    assert len(set(everything.classification[everything.status == 0].tolist())) >= 3 and np.count_nonzero(blocks[-1]) > 8
    # ... and one config against the oracle's pairs under the restated rule
    pick = 6 if k > 2 else 1  # "all" (of two call sets a majority is identity: NoConflict with ConflictSelection there)
    want = oracle_merge(oracle, mb, contigs, configs[pick])
    assert same(merge_multi_batch_sweep(ctx, pm, configs)[pick], want)


def test_one_config_is_the_single_call_word_for_word(ctx):
    _, mb = job(3, 700)
    pm = PackedMultiBatch.from_multi(mb)
    n = merge_counts_len(ctx.lib, 3)
    for cfg in FOUR:
        a, b = np.zeros((1, n), np.uint64), np.zeros(n, np.uint64)
        got = merge_multi_batch_sweep(ctx, pm, [cfg], counts=a)
        assert counts_on_device(ctx)
        want = merge_multi_batch(ctx, pm, cfg, counts=b)
        assert len(got) == 1 and same(got[0], want) and np.array_equal(a[0], b) and b.sum() > 0


def test_counts_are_added_to(ctx):
    _, mb = job(3, 700)
    pm = PackedMultiBatch.from_multi(mb)
    n = merge_counts_len(ctx.lib, 3)
    start = (np.arange(4 * n, dtype=np.uint64) * np.uint64(7) + np.uint64(2 ** 33)).reshape(4, n)
    _, blocks = swept(ctx, pm, FOUR, start=start)
    # two sweeps in a row into one array: twice the blocks; duplicates of one config get the same block each
    twice = np.zeros((4, n), np.uint64)
    merge_multi_batch_sweep(ctx, pm, FOUR, counts=twice)
    merge_multi_batch_sweep(ctx, pm, FOUR, counts=twice)
    assert np.array_equal(twice, np.stack(blocks) * np.uint64(2))
    dup = np.zeros((3, n), np.uint64)
    got = merge_multi_batch_sweep(ctx, pm, [FOUR[3], FOUR[0], FOUR[3]], counts=dup)
    assert np.array_equal(dup, np.stack([blocks[3], blocks[0], blocks[3]])) and same(got[0], got[2])
    # ... and a smaller batch behind a larger one sees nothing of it
    _, small = job(3, 1)
    swept(ctx, PackedMultiBatch.from_multi(small), FOUR)


def test_without_counts_the_three_arrays_are_the_same(ctx):
    _, mb = job(3, 700)
    pm = PackedMultiBatch.from_multi(mb)
    with_counts = merge_multi_batch_sweep(ctx, pm, FOUR, counts=np.zeros((4, merge_counts_len(ctx.lib, 3)), np.uint64))
    without = merge_multi_batch_sweep(ctx, pm, FOUR)
    assert len(without) == 4 and all(same(a, b) for a, b in zip(with_counts, without))
    assert all(same(without[c], merge_multi_batch(ctx, pm, FOUR[c])) for c in range(4))
    # a batch beyond the counters' inputs can be swept without them
    _, mb = job(9, 100)
    pm = PackedMultiBatch.from_multi(mb)
    assert all(same(g, merge_multi_batch(ctx, pm, c)) for g, c in zip(merge_multi_batch_sweep(ctx, pm, eight(9)), eight(9)))


def test_the_escaped_job(ctx):
    contigs, mb = el.merge_job()
    pm = PackedMultiBatch.from_multi(mb, escapes=True)
    long_slots = pm.escapes.esc_slot[pm.escapes.esc_cnt > 255].astype(np.int64)
    assert long_slots.size >= 1 and pm.c_escapes() is not None
    singles, _ = swept(ctx, pm, FOUR)
    assert all(singles[0].status[s // 3] == 0 for s in long_slots)  # the dense region is solved: its 260 calls are among every config's counters


def raw_sweep(ctx, pm, configs, counts):
    """avk_merge_packed_sweep itself -> (return code, status, classification, members) with the outputs pre-filled"""
    n, nc = pm.n_regions, len(configs)
    cfgs = (AvkMergeConfig * max(nc, 1))(*[AvkMergeConfig(c.max_branch_factor, int(c.no_conflict_enabled), int(c.majority_voting_enabled), -1 if c.conflict_selection is None else int(c.conflict_selection))
                                            for c in configs])
    st, cl, mem = np.full(max(n, 1), -77, np.int32), np.full(max(nc * n, 1), 0xAB, np.uint8), np.full(max(nc * n, 1), 0xABCD, np.uint64)
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    f = ctx.lib.avk_merge_packed_sweep
    f.argtypes = [C.c_void_p, C.POINTER(AvkPackedMultiBatch), C.POINTER(AvkPackedEscapes), C.c_uint32, C.POINTER(AvkMergeConfig), C.POINTER(C.c_int32), C.POINTER(C.c_uint8),
                  C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    cb, esc = pm.c_struct(), pm.c_escapes()
    rc = f(ctx.handle, C.byref(cb), C.byref(esc) if esc is not None else None, nc, cfgs, P(st, C.c_int32), P(cl, C.c_uint8), P(mem, C.c_uint64), None if counts is None else P(counts, C.c_uint64))
    return rc, st, cl, mem


def test_refusals_leave_everything_untouched_and_the_context_goes_on(ctx):
    _, mb = job(3, 700)
    pm = PackedMultiBatch.from_multi(mb)
    n = merge_counts_len(ctx.lib, 3)
    start = (np.arange(9 * n, dtype=np.uint64) + np.uint64(5)).reshape(9, n)
    untouched = lambda st, cl, mem: (st == -77).all() and (cl == 0xAB).all() and (mem == 0xABCD).all()
    # refused from the arguments, before anything is queued: nothing is written at all
    for configs in ([MergeConfig(), MergeConfig(max_branch_factor=49)], [MergeConfig()] * 9, [], [MergeConfig(), MergeConfig(conflict_selection=3)], [MergeConfig(conflict_selection=-2)]):
        counts = start.copy()
        rc, st, cl, mem = raw_sweep(ctx, pm, configs, counts)
        assert rc == -1 and untouched(st, cl, mem) and np.array_equal(counts, start), len(configs)  # AVK_E_ARG
    with pytest.raises(AardvarkAmdError):
        merge_multi_batch_sweep(ctx, pm, [MergeConfig(), MergeConfig(max_branch_factor=1)])
    eleven = mc.packed_batch(11, [0] * 11, [])
    counts = np.full(16, 3, np.uint64)
    rc, st, cl, mem = raw_sweep(ctx, eleven, FOUR[:2], counts)
    assert rc == -1 and untouched(st, cl, mem) and counts.tolist() == [3] * 16
    swept(ctx, pm, FOUR)
    # a type nibble of 15, in a region that is not solved because of it: the count kernel of EVERY config refuses the batch; no block reaches counts
    bad = PackedMultiBatch.from_multi(mb)
    bad.var_type_zyg = bad.var_type_zyg.copy()
    r = int(np.flatnonzero(bad.in_cnt.reshape(-1, 3).sum(axis=1) >= 2)[7])
    v = int(bad.in_cnt[:3 * r].astype(np.int64).sum())
    bad.var_type_zyg[v] |= 15  # (no VariantType: the call leaves its region unsolved)
    counts = start.copy()
    rc, st, _, _ = raw_sweep(ctx, bad, FOUR, counts)
    assert rc == -1 and np.array_equal(counts, start) and st[r] != 0
    with pytest.raises(AardvarkAmdError):
        merge_multi_batch_sweep(ctx, bad, FOUR, counts=counts)
    assert np.array_equal(counts, start)
    assert all(same(g, merge_multi_batch(ctx, bad, c)) for g, c in zip(merge_multi_batch_sweep(ctx, bad, FOUR), FOUR))  # (without counters the batch is a batch like any other)
    swept(ctx, pm, FOUR, start=start[:4])
    # ... the same on the host route
    ctx.set_option("device_pack", 0)
    try:
        rc, _, _, _ = raw_sweep(ctx, bad, FOUR, counts)
        assert rc == -1 and np.array_equal(counts, start)
        swept(ctx, PackedMultiBatch.from_multi(job(3, 300)[1]), FOUR, on_device=False)
    finally:
        ctx.set_option("device_pack", 1)
    swept(ctx, pm, FOUR)


def het_cluster_job():
    """(contigs, MultiBatch of three inputs): clusters of heterozygous calls, where the search does branch — input 0 and 1 are the two sides of a compare region, input 2
    is one of them again (tests/test_merge.py builds its regions the same way)"""
    from test_wide_parity import het_cluster_regions
    contigs, b = het_cluster_regions(9, 300, n_sites=(3, 9), indel=0.3)
    ab = b.allele_bytes.tobytes()

    def variants(off, cnt):
        return [(int(b.var_pos[v]), ab[int(b.a0_off[v]):int(b.a0_off[v]) + int(b.a0_len[v])], ab[int(b.a1_off[v]):int(b.a1_off[v]) + int(b.a1_len[v])], int(b.var_type[v]), int(b.var_zyg[v]),
                 int(b.var_raw_space[v])) for v in range(off, off + cnt)]
    multi = []
    for q in range(b.n_regions):
        t, qv = variants(int(b.t_off[q]), int(b.t_cnt[q])), variants(int(b.q_off[q]), int(b.q_cnt[q]))
        multi.append({"start": int(b.start[q]), "end": int(b.end[q]), "contig": int(b.contig_idx[q]), "inputs": [t, qv, t if q % 2 else qv]})
    return contigs, MultiBatch.from_regions(multi)


def test_the_shared_solve_honours_the_branch_factor_and_leaves_no_state(ctx, oracle):
    contigs, mb = het_cluster_job()
    pm = PackedMultiBatch.from_multi(mb)
    cfg = MergeConfig(majority_voting_enabled=True)
    ones = [MergeConfig(c.no_conflict_enabled, c.majority_voting_enabled, c.conflict_selection, max_branch_factor=1) for c in FOUR]
    ctx.upload_reference(contigs)
    try:
        before = merge_multi_batch(ctx, pm, cfg)
        singles, _ = swept(ctx, pm, ones)  # every slice equals the single call at a branch factor of 1 ...
        assert not same(singles[2], before)  # ... which is not the answer at 50: a pair or two are no exact match with one branch per bucket
        assert same(singles[2], oracle_merge(oracle, mb, contigs, ones[2])) and same(before, oracle_merge(oracle, mb, contigs, cfg))
        assert same(merge_multi_batch(ctx, pm, cfg), before)  # nothing of the sweep stays with the context
        swept(ctx, pm, FOUR)
        assert same(merge_multi_batch(ctx, pm, cfg), before)
    finally:
        ctx.upload_reference(job(3)[0])
    _, small = job(3, 700)
    spm = PackedMultiBatch.from_multi(small)
    first = merge_multi_batch(ctx, spm, cfg)
    swept(ctx, spm, ones)
    assert same(merge_multi_batch(ctx, spm, cfg), first)
