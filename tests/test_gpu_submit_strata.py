"""The stratified packed call in two halves on a real MI355X (avk_compare_packed_submit_strata -> avk_wait): batches in flight whose per-label sums come from the
resident sets — the strata mask pass on the batch's own packing streams, avk_label_tally_mask_kernel on the masks behind the solve — against the one-call form of
the same build, against sums of the ORACLE's per-region blocks over the HOST's lists (avf_strat_batch_labels), and with result arrays bit-identical to a plain
submit.  Every comparison is exact.

The job: 900 regions of the first two contigs of a genome slice (scale 0.003) and 401 fuzz regions on a third contig, 1,301 regions (two workgroups of the tally,
six of the mask pass, the last ones partly filled), and a 700-region selection of them as a second batch.  Label sets of 5, 33, label_block + 1 and
2 * label_block + 33 labels (label_block: 71 with 160 KB of LDS, 28 with 64 KB — one launch; a second mask word; a second launch of one label; three launches whose
blocks start and end inside words), and of 75 labels for the tickets in flight: one label on every region, one on none, one whose intervals end mid-batch, the rest
random intervals."""
import ctypes as C
import os

import numpy as np
import pytest

import escapes_lib
import oracle_lib
import scenarios
import strata_emu_lib as sx
from aardvark_amd import CompactBatch, PackedBatch, ResultBatch, feeder, synth
from aardvark_amd._abi import TALLY_LEN, AvkCompareConfig

pytestmark = pytest.mark.gpu
CPUS = min(os.cpu_count() or 1, 16)
WORDS = 13 * 22
N_ALL, N_SMALL = 1301, 700
u64p = C.POINTER(C.c_uint64)


def write_label_sets(folder, n_labels, lens, seed):
    from test_feeder import write_text
    rng = np.random.default_rng(seed)
    beds = {"a_every": [(c, 0, 10_000_000) for c in sx.NAMES], "b_none": [("chrZ", 0, 10_000_000)], "c_mid": [("chrA", 0, 10_000_000), ("chrB", 0, lens[1] // 2)]}
    for x in range(n_labels - 3):
        iv = []
        for c in range(3):
            k = 20 + 9 * (x % 40)
            width = (2_000, 90_000) if lens[c] > 100_000 else (40, 1_500)
            iv += [(sx.NAMES[c], int(s), int(s) + int(w)) for s, w in zip(rng.integers(0, lens[c], k), rng.integers(width[0], width[1], k))]
        beds["x%03d" % x] = sorted(iv)
    sub = os.path.join(folder, "sets%d" % n_labels)
    os.makedirs(sub)
    for name, iv in beds.items():
        write_text(os.path.join(sub, name + ".bed"), "".join("%s\t%d\t%d\n" % x for x in iv))
    write_text(os.path.join(sub, "strat.tsv"), "".join("%s\t%s.bed\n" % (n, n) for n in beds))
    return os.path.join(sub, "strat.tsv")


def oracle_sums(res, off, idx, n_labels):
    want = np.zeros((n_labels, TALLY_LEN), np.uint64)
    blocks = np.asarray(res.group_metrics).reshape(-1, WORDS).astype(np.uint64)
    n = len(off) - 1
    region = np.repeat(np.arange(n), np.diff(np.asarray(off).astype(np.int64)))
    solved = np.asarray(res.status)[:n][region] == 0
    region, label = region[solved], np.asarray(idx)[solved]
    for l in range(n_labels):
        want[l, :WORDS] = blocks[region[label == l]].sum(axis=0, dtype=np.uint64)
    return want


def same(a, b):
    return np.array_equal(a.region_packed, b.region_packed) and np.array_equal(a.var_packed, b.var_packed) and np.array_equal(a.tally, b.tally)


def agrees(res, want):
    n = len(want.status)
    return np.array_equal(np.asarray(res.status)[:n], want.status) and np.array_equal(np.asarray(res.tally, np.uint64)[:WORDS], np.asarray(want.tally, np.uint64)[:WORDS])


@pytest.fixture(scope="module")
def job(oracle, tmp_path_factory):
    """one context, the two batches (pageable and pinned), the oracle's results, the label sets with their handles, the HOST's lists and the sums they give,
    the plain submit's results: shared, never changed"""
    import aardvark_amd
    from test_feeder import write_text
    folder = str(tmp_path_factory.mktemp("gpu_submit_strata"))
    gcontigs, gbatch = synth.config_genome(scale=0.003, threads=4)
    n_two = int((gbatch.contig_idx < 2).sum())
    n_one = int((gbatch.contig_idx < 1).sum())
    assert n_one >= 450 and n_two - n_one >= 450
    fcontigs, fuzz = scenarios.fuzz_regions(77, N_ALL - 900, max_vars=4)
    fuzz.contig_idx[:] = 2
    batch = synth.concat_batches([escapes_lib.reordered(gbatch, np.r_[0:450, n_two - 450:n_two]), fuzz])
    contigs = [gcontigs[0], gcontigs[1], fcontigs[0]]
    assert batch.n_regions == N_ALL
    small = escapes_lib.reordered(batch, np.r_[0:300, 700:900, N_ALL - 200:N_ALL])
    assert small.n_regions == N_SMALL and len(set(small.contig_idx.tolist())) == 3
    batches = {N_ALL: batch, N_SMALL: small}
    wants = {n: oracle_lib.compare_batch(oracle, b, contigs, threads=CPUS) for n, b in batches.items()}
    assert (np.asarray(wants[N_ALL].status) == 0).sum() > 1000
    genome = feeder.Genome(sx.write_genome(folder, write_text))
    ctx = aardvark_amd.Context(0)
    ctx.set_option("lane_min_regions", 0)
    ctx.set_option("lane_min_batch", 0)
    ctx.upload_reference(contigs)
    B = ctx.label_block()
    assert B in (28, 71)
    lens = [len(c) for c in contigs]
    sets = {}
    for n_labels in sorted({5, 33, 75, B + 1, 2 * B + 33}):
        strat = feeder.Stratifications(write_label_sets(folder, n_labels, lens, 100 + n_labels))
        assert len(strat.labels) == n_labels
        lists = {n: strat.batch_labels(genome, b) for n, b in batches.items()}
        sums = {n: oracle_sums(wants[n], *lists[n], n_labels) for n in batches}
        assert sums[N_ALL][0].any() and not sums[N_ALL][1].any() and sums[N_ALL][3:].any(axis=1).all()
        sets[n_labels] = dict(strata=ctx.upload_strata(*strat.export(genome)), lists=lists, sums=sums)
        strat.close()
    pbs = {n: PackedBatch.from_compact(CompactBatch.from_region_batch(b)) for n, b in batches.items()}
    pinned = {n: ctx.pinned_packed(pb) for n, pb in pbs.items()}
    plain, plain_launches = {}, {}
    for n, p in pinned.items():
        plain[n] = ctx.submit_packed(p, res=ctx.pinned_results(p, packed="only")).wait()
        plain_launches[n] = ctx.last_region_launches()
    yield dict(ctx=ctx, B=B, contigs=contigs, pbs=pbs, pinned=pinned, wants=wants, sets=sets, plain=plain, plain_launches=plain_launches, genome=genome, folder=folder, lens=lens)
    for s in sets.values():
        s["strata"].free()
    ctx.close()


def submit(job, n, n_labels, **kw):
    ctx, p = job["ctx"], job["pinned"][n]
    return ctx.submit_packed(p, res=ctx.pinned_results(p, packed="only"), strata=job["sets"][n_labels]["strata"], **kw)


def label_counts(job):
    return [5, 33, job["B"] + 1, 2 * job["B"] + 33]


@pytest.mark.parametrize("which", range(4))
def test_parity(job, which):
    """the submitted sums equal the one-call form's of this build, the sums of the oracle's blocks over the host's lists; the results equal the plain submit's"""
    ctx, n_labels = job["ctx"], label_counts(job)[which]
    s, pb = job["sets"][n_labels], job["pbs"][N_ALL]
    got = submit(job, N_ALL, n_labels).wait()
    one_call = ctx.solve_packed(pb, res=ResultBatch(pb, sequences=False, group_metrics=False, packed="only"), strata=s["strata"])
    assert same(got, job["plain"][N_ALL]) and same(one_call, got)
    assert np.array_equal(got.label_tallies, one_call.label_tallies)
    assert np.array_equal(got.label_tallies, s["sums"][N_ALL])
    wide = ctx.submit_packed(job["pinned"][N_ALL], res=ctx.pinned_results(job["pinned"][N_ALL]), strata=s["strata"]).wait()
    assert agrees(wide, job["wants"][N_ALL]) and np.array_equal(wide.label_tallies, got.label_tallies)


def test_four_tickets_two_handles_two_batches(job):
    """four in flight — (batch, handle) all different — waited for in reverse order: every ticket's sums and results are its own"""
    plan = [(N_ALL, 5), (N_SMALL, 75), (N_ALL, 75), (N_SMALL, 5)]
    tickets = [submit(job, n, n_labels) for n, n_labels in plan]
    for k in (3, 2, 1, 0):
        n, n_labels = plan[k]
        got = tickets[k].wait()
        assert same(got, job["plain"][n]), k
        assert np.array_equal(got.label_tallies, job["sets"][n_labels]["sums"][n]), k


def test_sums_are_added_and_the_last_two_words_stay(job):
    n_labels = job["B"] + 1
    sums = job["sets"][n_labels]["sums"][N_ALL]
    out = np.full((n_labels, TALLY_LEN), 3, np.uint64)
    out[:, WORDS:] = 7
    got = submit(job, N_ALL, n_labels, label_tallies=out).wait()
    assert got.label_tallies is out
    assert np.array_equal(out[:, :WORDS], sums[:, :WORDS] + np.uint64(3)) and (out[:, WORDS:] == 7).all()
    submit(job, N_ALL, n_labels, label_tallies=out).wait()
    assert np.array_equal(out[:, :WORDS], 2 * sums[:, :WORDS] + np.uint64(3)) and (out[:, WORDS:] == 7).all()


def test_no_strata_is_the_plain_submit(job):
    """a NULL handle and a handle without labels: the results of the plain submit, label_tallies untouched, the region pass launched as often"""
    ctx, p = job["ctx"], job["pinned"][N_ALL]
    empty = ctx.upload_strata(0, 3, np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint32))
    try:
        for handle in (None, empty.handle):
            res = ctx.pinned_results(p, packed="only")
            pb, cfg, ro = p.c_struct(), AvkCompareConfig(50, 0, 0), res.c_struct()
            sums = np.full((4, TALLY_LEN), 9, np.uint64)
            ticket = C.c_void_p()
            assert ctx.lib.avk_compare_packed_submit_strata(ctx.handle, C.byref(pb), None, handle, C.byref(cfg), C.byref(ro), sums.ctypes.data_as(u64p), C.byref(ticket)) == 0
            assert ctx.last_region_launches() == job["plain_launches"][N_ALL]
            assert ctx.lib.avk_wait(ctx.handle, ticket) == 0
            assert same(res, job["plain"][N_ALL]) and (sums == 9).all()
        got = ctx.submit_packed(p, res=ctx.pinned_results(p, packed="only"), strata=empty).wait()
        assert same(got, job["plain"][N_ALL]) and got.label_tallies.size == 0
        # ... and with labels the region pass is launched as often as without: the mask pass rides behind it
        submit(job, N_ALL, 5).wait()
        assert ctx.last_region_launches() == job["plain_launches"][N_ALL]
    finally:
        empty.free()
    with pytest.raises(ValueError, match="exclude each other"):
        off, idx = job["sets"][5]["lists"][N_ALL]
        ctx.submit_packed(p, labels=(5, off, idx), strata=job["sets"][5]["strata"])


def test_pageable_arrays_are_solved_at_submit(job):
    ctx, pb, s = job["ctx"], job["pbs"][N_SMALL], job["sets"][33]
    out = np.zeros((33, TALLY_LEN), np.uint64)
    t = ctx.submit_packed(pb, res=ResultBatch(pb, sequences=False, group_metrics=False, packed="only"), strata=s["strata"], label_tallies=out)
    assert np.array_equal(out, s["sums"][N_SMALL])  # the ticket is complete: the sums are there before the wait
    got = t.wait()
    assert same(got, job["plain"][N_SMALL]) and np.array_equal(out, s["sums"][N_SMALL])


def test_promoted_escapes_take_the_same_sums(job):
    """the batch with some of its regions, count slots and calls moved into the escape lists (the same values): the escaped packing route, the same masks and sums"""
    ctx, pb, s = job["ctx"], job["pbs"][N_ALL], job["sets"][33]
    src = ctx.pinned_packed(escapes_lib.promote(pb, regions=[1, 7, pb.n_regions - 1], slots=[0, 5, 2 * pb.n_regions - 2], calls=[0, 3, pb.n_variants - 1]))
    assert not src.escapes.empty()
    got = ctx.submit_packed(src, res=ctx.pinned_results(src), strata=s["strata"]).wait()
    assert agrees(got, job["wants"][N_ALL]) and np.array_equal(got.label_tallies, s["sums"][N_ALL])


def test_batch_with_escapes(oracle, tmp_path):
    """strata_emu_lib's escape regions — a window over 65,535 bases, alleles over 255 bases that alone decide whether the region ends inside label f_mid — among 300
    random ones, on a reference their calls fit: submitted, against the one-call form and the oracle's blocks over the host's lists"""
    import aardvark_amd
    from test_feeder import write_text
    batch = sx.batch_of(sx.escape_regions() + sx.random_regions(300, seed=5))
    contigs = [b"A" * (sx.SPAN + 2_000)] * 3
    want = oracle_lib.compare_batch(oracle, batch, contigs, threads=CPUS)
    assert (np.asarray(want.status) == 0).sum() > 200
    genome = feeder.Genome(sx.write_genome(str(tmp_path), write_text))
    strat = feeder.Stratifications(sx.write_sets(str(tmp_path), write_text, n_many=500, extra_labels=34))
    off, idx = strat.batch_labels(genome, batch)
    sums = oracle_sums(want, off, idx, 40)
    ctx = aardvark_amd.Context(0)
    try:
        ctx.upload_reference(contigs)
        strata = ctx.upload_strata(*strat.export(genome))
        pb = PackedBatch.from_compact(CompactBatch.from_region_batch(batch), escapes=True)
        assert len(pb.escapes.esc_region) >= 1 and len(pb.escapes.esc_call) >= 2
        p = ctx.pinned_packed(pb)
        got = ctx.submit_packed(p, res=ctx.pinned_results(p), strata=strata).wait()
        one_call = ctx.solve_packed(pb, res=ResultBatch(pb, sequences=False, group_metrics=False), strata=strata)
        assert agrees(got, want) and np.array_equal(got.label_tallies, one_call.label_tallies) and np.array_equal(got.label_tallies, sums)
        assert sums[5].any() and sums[0].any()
        strata.free()
    finally:
        strat.close()
        ctx.close()


def test_capacity_retry_counts_repaired_regions_once(oracle):
    """the starved-workspace context of tests/test_gpu_strata.py: regions come back AVK_ST_CAPACITY and are repaired in avk_wait, their labels read back from their
    own mask words; one label on every region sums to the oracle's tally — every repaired region once"""
    import aardvark_amd
    ctx = aardvark_amd.Context(0)
    try:
        for k, v in dict(lds_bytes_per_wave=2048, lds2_bytes_per_wave=0, ws_bytes_per_wave=0, big_ws_bytes=4096).items():
            ctx.set_option(k, v)
        contigs, batch = scenarios.fuzz_regions(341, 400, max_vars=9, max_len=12)
        ctx.upload_reference(contigs)
        want = oracle_lib.compare_batch(oracle, batch, contigs, threads=CPUS)
        pb = PackedBatch.from_compact(CompactBatch.from_region_batch(batch))
        p = ctx.pinned_packed(pb)
        # label 0: every region; label 1: nothing; label 2: the first half of the contig; labels 3 .. 34: every region again (a second mask word)
        n_labels = 35
        tree_off = np.array([0, 1, 1, 2] + [3 + k for k in range(32)], np.uint64)
        start = np.zeros(34, np.uint32)
        end_max = np.array([10_000_000, 2_000] + [10_000_000] * 32, np.uint32)
        strata = ctx.upload_strata(n_labels, 1, tree_off, start, end_max)
        ctx.set_option("capacity_retry", 0)
        starved = ctx.submit_packed(p, res=ctx.pinned_results(p)).wait()
        assert (starved.status == 21).any()
        ctx.set_option("capacity_retry", 1)
        got = ctx.submit_packed(p, res=ctx.pinned_results(p), strata=strata).wait()
        assert agrees(got, want)
        assert np.array_equal(got.label_tallies[0, :WORDS], want.tally[:WORDS]) and not got.label_tallies[1].any()
        assert np.array_equal(got.label_tallies[34, :WORDS], want.tally[:WORDS]) and np.array_equal(got.label_tallies[3], got.label_tallies[0])
        assert 0 < got.label_tallies[2].sum() < got.label_tallies[0].sum()
        one_call = ctx.solve_packed(pb, res=ResultBatch(pb, sequences=False, group_metrics=False), strata=strata)
        assert np.array_equal(got.label_tallies, one_call.label_tallies)
        strata.free()
    finally:
        ctx.close()


def test_refusals(job):
    """a handle of another context and a NULL label_tallies are AVK_E_ARG before anything is queued; a fifth submit is AVK_E_STATE and the four in flight complete"""
    import aardvark_amd
    ctx, p, s = job["ctx"], job["pinned"][N_SMALL], job["sets"][5]
    other = aardvark_amd.Context(0)
    try:
        foreign = other.upload_strata(1, 1, np.array([0, 1], np.uint64), np.array([0], np.uint32), np.array([100], np.uint32))
        with pytest.raises(aardvark_amd.AardvarkAmdError, match="error -1.*another context"):
            ctx.submit_packed(p, res=ctx.pinned_results(p, packed="only"), strata=foreign)
        foreign.free()
    finally:
        other.close()
    res = ctx.pinned_results(p, packed="only")
    pb, cfg, ro = p.c_struct(), AvkCompareConfig(50, 0, 0), res.c_struct()
    ticket = C.c_void_p()
    assert ctx.lib.avk_compare_packed_submit_strata(ctx.handle, C.byref(pb), None, s["strata"].handle, C.byref(cfg), C.byref(ro), None, C.byref(ticket)) == -1
    assert not ticket.value and "label_tallies missing" in ctx.lib.avk_last_error(ctx.handle).decode()
    # both refusals left every staging slot free: four submits go through, the fifth is refused, the four complete
    tickets = [submit(job, N_SMALL, 5) for _ in range(4)]
    with pytest.raises(aardvark_amd.AardvarkAmdError, match="error -4.*four batches are in flight"):
        submit(job, N_SMALL, 5)
    for t in tickets:
        got = t.wait()
        assert same(got, job["plain"][N_SMALL]) and np.array_equal(got.label_tallies, s["sums"][N_SMALL])


def test_the_handle_may_be_freed_before_the_wait(job):
    """Strata.free() between submit and wait: the ticket holds what avk_wait needs; a fresh upload of the same sets and a call with it are right too"""
    ctx, genome = job["ctx"], job["genome"]
    strat = feeder.Stratifications(os.path.join(job["folder"], "sets33", "strat.tsv"))
    exported = strat.export(genome)
    strat.close()
    want = job["sets"][33]["sums"]
    first = ctx.upload_strata(*exported)
    p = job["pinned"][N_ALL]
    t1 = ctx.submit_packed(p, res=ctx.pinned_results(p, packed="only"), strata=first)
    t2 = ctx.submit_packed(job["pinned"][N_SMALL], res=ctx.pinned_results(job["pinned"][N_SMALL], packed="only"), strata=first)
    first.free()
    assert not first.handle
    again = ctx.upload_strata(*exported)  # (may well be handed the memory the first handle's trees lay in)
    t3 = ctx.submit_packed(p, res=ctx.pinned_results(p, packed="only"), strata=again)
    for t, n in ((t2, N_SMALL), (t1, N_ALL), (t3, N_ALL)):
        got = t.wait()
        assert same(got, job["plain"][n]) and np.array_equal(got.label_tallies, want[n])
    again.free()
