"""Stratified tallies from the compact results on a real MI355X (avk_label_tally_compact_kernel): the resident form, the one-call forms, the capacity retry,
shards and the command-line tool, against sums of the ORACLE's per-region blocks.  Every comparison is exact.

Label counts straddle the label block B = Context.label_block() (the labels whose sums one launch holds in LDS): 1, B - 1, B, B + 1, 2 B + 1.  Labels are random
genomic intervals (a region carries a label when an interval contains it, the rule of the stratification BEDs), plus one label on every region, one on none, one
region with an empty list, one region listed under more than B labels, and repeats inside lists.

Measured on one MI355X: the 20 tests of this file take 5.7 s in all; the slowest are the fixture (1.8 s: the context and the oracle's results), the tool (1.7 s, two
processes) and the capacity retry (0.7 s); every other test takes 0.1 s or less.
"""
import ctypes as C
import os

import numpy as np
import pytest

import escapes_lib
import oracle_lib
import scenarios
from aardvark_amd import CompactBatch, PackedBatch, ResultBatch, dist
from aardvark_amd._abi import TALLY_LEN, AvkRegionLabels

pytestmark = pytest.mark.gpu
CPUS = min(os.cpu_count() or 1, 16)
WORDS = 13 * 22
P = C.POINTER


def interval_labels(batch, n_labels, seed, span):
    """-> (off, idx, lists).  Label 0: every region; label 1 (when there is one): no region; labels 2..: 6 + l random intervals each."""
    rng = np.random.default_rng(seed)
    n = batch.n_regions
    start, end = np.asarray(batch.start, np.int64), np.asarray(batch.end, np.int64)
    lists = [[0] for _ in range(n)]
    for l in range(2, n_labels):
        k = 6 + l % 40
        s = rng.integers(0, span, k)
        w = rng.integers(200, max(span // 8, 400), k)
        inside = ((s[None, :] <= start[:, None]) & (end[:, None] <= (s + w)[None, :])).any(axis=1)
        for r in np.flatnonzero(inside):
            lists[int(r)].append(l)
    lists[0] = []                                                                    # a region with an empty list
    lists[n // 3] = [l for l in range(n_labels) if l != 1] * 2 + [0]                 # under every label (more than B of them at the larger counts), each twice
    for r in range(5, n, 23):
        if lists[r]:
            lists[r].append(lists[r][-1])                                            # a label named twice counts twice
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in lists])
    return off, np.array([l for x in lists for l in x], np.uint32), lists


def oracle_sums(res, lists, n_labels):
    want = np.zeros((n_labels, TALLY_LEN), np.uint64)
    blocks = np.asarray(res.group_metrics).reshape(len(lists), WORDS).astype(np.uint64)
    for r, ls in enumerate(lists):
        if int(res.status[r]) == 0:
            for l in ls:
                want[l, :WORDS] += blocks[r]
    return want


@pytest.fixture(scope="module")
def job(oracle):
    """one context, one call set (SNVs and indels, several call types per region, some unsolved regions), the oracle's results: shared, never changed"""
    import aardvark_amd
    contigs, base = scenarios.indel_small(1500)
    _, bad = scenarios.invalid_regions()
    from aardvark_amd import synth
    batch = synth.concat_batches([base, bad])
    want = oracle_lib.compare_batch(oracle, batch, contigs, threads=CPUS)
    assert (np.asarray(want.status) != 0).any() and (np.asarray(want.status) == 0).sum() > 500
    ctx = aardvark_amd.Context(0)
    ctx.set_option("lane_min_regions", 0)
    ctx.set_option("lane_min_batch", 0)
    ctx.upload_reference(contigs)
    pb = PackedBatch.from_compact(CompactBatch.from_region_batch(batch))
    span = max(len(c) for c in contigs)
    yield dict(ctx=ctx, contigs=contigs, batch=batch, pb=pb, want=want, span=span, B=ctx.label_block())
    ctx.close()


def counts(B):
    return [1, B - 1, B, B + 1, 2 * B + 1]


def test_label_block_comes_from_the_launchs_lds(job):
    B = job["B"]
    assert B in (65536 // (WORDS * 8), 163840 // (WORDS * 8)) and B >= 16


@pytest.mark.parametrize("which", range(5))
def test_resident_sums_equal_the_oracles(job, which):
    """emit_group_metrics = 0, packed source: the sums equal the oracle's; a second call doubles `out`; words 286 / 287 stay"""
    ctx, pb, want = job["ctx"], job["pb"], job["want"]
    n_labels = counts(job["B"])[which]
    off, idx, lists = interval_labels(job["batch"], n_labels, 10 + which, job["span"])
    sums = oracle_sums(want, lists, n_labels)
    assert sums[0].any() and (n_labels < 3 or sums[2:].any())
    ctx.set_option("emit_group_metrics", 0)
    ctx.set_option("emit_bp_groups", 1)
    rb = ctx.upload(pb)
    try:
        ctx.compare_resident(rb)
        out = np.zeros((n_labels, TALLY_LEN), np.uint64)
        out[:, WORDS:] = 7
        ctx.label_tallies_compact(rb, n_labels, off, idx, out=out)
        assert np.array_equal(out[:, :WORDS], sums[:, :WORDS]) and (out[:, WORDS:] == 7).all()
        ctx.label_tallies_compact(rb, n_labels, off, idx, out=out)
        assert np.array_equal(out[:, :WORDS], 2 * sums[:, :WORDS])
    finally:
        rb.free()
        ctx.set_option("emit_bp_groups", 0)


@pytest.mark.parametrize("form", ["packed_source=0", "escaped", "wide+blocks"])
def test_resident_other_sources(job, form):
    """the widened packed batch, a batch with escapes, and the wide upload — there also against avk_label_tallies on the same batch (emit_group_metrics = 1)"""
    ctx, pb, want, batch = job["ctx"], job["pb"], job["want"], job["batch"]
    n_labels = job["B"] + 1
    off, idx, lists = interval_labels(batch, n_labels, 3, job["span"])
    sums = oracle_sums(want, lists, n_labels)
    ctx.set_option("emit_bp_groups", 1)
    ctx.set_option("emit_group_metrics", 1 if form == "wide+blocks" else 0)
    ctx.set_option("packed_source", 0 if form == "packed_source=0" else 1)
    src = pb
    if form == "escaped":
        src = escapes_lib.promote(pb, regions=[1, 7, pb.n_regions - 1], slots=[0, 5, 2 * pb.n_regions - 2], calls=[0, 3, pb.n_variants - 1])
        assert not src.escapes.empty()
    if form == "wide+blocks":
        src = batch
    rb = ctx.upload(src)
    try:
        ctx.compare_resident(rb)
        got = ctx.label_tallies_compact(rb, n_labels, off, idx)
        assert np.array_equal(got, sums)
        if form == "wide+blocks":
            assert np.array_equal(ctx.label_tallies(rb, n_labels, off, idx), got)
    finally:
        rb.free()
        ctx.set_option("emit_bp_groups", 0)
        ctx.set_option("emit_group_metrics", 0)
        ctx.set_option("packed_source", 1)


def test_resident_refusals(job):
    import aardvark_amd
    ctx, pb, batch = job["ctx"], job["pb"], job["batch"]
    off, idx, _ = interval_labels(batch, 4, 1, job["span"])
    ctx.set_option("emit_bp_groups", 0)
    rb = ctx.upload(pb)
    ctx.compare_resident(rb)
    with pytest.raises(aardvark_amd.AardvarkAmdError, match="error -4.*emit_bp_groups"):
        ctx.label_tallies_compact(rb, 4, off, idx)
    with pytest.raises(aardvark_amd.AardvarkAmdError, match="label index"):
        ctx.label_tallies_compact(rb, 2, off, idx)
    rb.free()
    ctx.set_option("device_pack", 0)
    ctx.set_option("emit_bp_groups", 1)
    rb = ctx.upload(batch)
    try:
        ctx.compare_resident(rb)
        with pytest.raises(aardvark_amd.AardvarkAmdError, match="error -4.*device_pack"):
            ctx.label_tallies_compact(rb, 4, off, idx)
    finally:
        rb.free()
        ctx.set_option("device_pack", 1)
        ctx.set_option("emit_bp_groups", 0)


def agrees(res, want):
    """statuses and the 286 sums of the tally against the oracle's (per-call arrays are compared bit for bit between the library's own calls)"""
    n = len(want.status)
    return np.array_equal(np.asarray(res.status)[:n], want.status) and np.array_equal(np.asarray(res.tally, np.uint64)[:WORDS], np.asarray(want.tally, np.uint64)[:WORDS])


def same(a, b):
    return np.array_equal(a.region_packed, b.region_packed) and np.array_equal(a.var_packed, b.var_packed) and np.array_equal(a.tally, b.tally)


@pytest.mark.parametrize("which", [0, 3, 4])
def test_one_call_form(job, which):
    """results and tally bit-identical to solve_packed without labels, wide and with only the required arrays; the labels' sums are the oracle's"""
    ctx, pb, want = job["ctx"], job["pb"], job["want"]
    n_labels = counts(job["B"])[which]
    off, idx, lists = interval_labels(job["batch"], n_labels, 20 + which, job["span"])
    sums = oracle_sums(want, lists, n_labels)
    plain = ctx.solve_packed(pb, res=ResultBatch(pb, sequences=False, group_metrics=False))
    got = ctx.solve_packed(pb, res=ResultBatch(pb, sequences=False, group_metrics=False), labels=(n_labels, off, idx))
    assert got.diff(plain) == [] and np.array_equal(got.tally, plain.tally) and np.array_equal(got.label_tallies, sums)
    assert agrees(plain, want)
    plain_only = ctx.solve_packed(pb, res=ResultBatch(pb, sequences=False, group_metrics=False, packed="only"))
    only = ctx.solve_packed(pb, res=ResultBatch(pb, sequences=False, group_metrics=False, packed="only"), labels=(n_labels, off, idx))
    assert same(only, plain_only) and np.array_equal(only.label_tallies, sums)
    # no labels: the old call
    none = ctx.solve_packed(pb, res=ResultBatch(pb, sequences=False, group_metrics=False, packed="only"), labels=(0, off, idx))
    assert same(none, plain_only) and none.label_tallies.size == 0


def test_two_submits_in_flight_with_different_lists(job):
    ctx, pb, want, batch = job["ctx"], job["pb"], job["want"], job["batch"]
    pinned = ctx.pinned_packed(pb)
    plain = ctx.solve_packed(pb, res=ResultBatch(pb, sequences=False, group_metrics=False, packed="only"))
    jobs = []
    for k, n_labels in enumerate((job["B"] + 1, 5)):
        off, idx, lists = interval_labels(batch, n_labels, 40 + k, job["span"])
        poff, pidx = ctx.host_array(off.shape, np.uint64), ctx.host_array(idx.shape, np.uint32)
        poff[...], pidx[...] = off, idx
        jobs.append((n_labels, poff, pidx, oracle_sums(want, lists, n_labels)))
    tickets = [ctx.submit_packed(pinned, res=ctx.pinned_results(pinned, packed="only"), labels=(n, o, i)) for n, o, i, _ in jobs]
    for k in (1, 0):  # waited for in reverse order
        got = tickets[k].wait()
        assert same(got, plain) and np.array_equal(got.label_tallies, jobs[k][3]), k
    # pageable arrays: solved inside the submit, the sums are there all the same
    n, o, i, s = jobs[1]
    t = ctx.submit_packed(pb, res=ResultBatch(pb, sequences=False, group_metrics=False, packed="only"), labels=(n, np.array(o), np.array(i)))
    assert np.array_equal(t.wait().label_tallies, s)


def test_capacity_retry_counts_repaired_regions(oracle):
    """tiny tiers: regions come back AVK_ST_CAPACITY from the kernels and are repaired by the download; one label on every region sums to the oracle's tally, in
    the one-call form (the repaired regions' blocks are added on the host) and in the resident form called after the download (the device view is patched)"""
    import aardvark_amd
    ctx = aardvark_amd.Context(0)
    try:
        for k, v in dict(lds_bytes_per_wave=2048, lds2_bytes_per_wave=0, ws_bytes_per_wave=0, big_ws_bytes=4096).items():
            ctx.set_option(k, v)
        contigs, batch = scenarios.fuzz_regions(341, 400, max_vars=9, max_len=12)
        ctx.upload_reference(contigs)
        want = oracle_lib.compare_batch(oracle, batch, contigs, threads=CPUS)
        pb = PackedBatch.from_compact(CompactBatch.from_region_batch(batch))
        n = batch.n_regions
        off, idx = np.arange(n + 1, dtype=np.uint64), np.zeros(n, np.uint32)
        ctx.set_option("capacity_retry", 0)
        starved = ctx.solve_packed(pb, res=ResultBatch(pb, sequences=False, group_metrics=False))
        assert (starved.status == 21).any()  # some regions do exhaust the last tier on the first try
        ctx.set_option("capacity_retry", 1)
        got = ctx.solve_packed(pb, res=ResultBatch(pb, sequences=False, group_metrics=False), labels=(1, off, idx))
        assert agrees(got, want) and np.array_equal(got.label_tallies[0, :WORDS], want.tally[:WORDS])
        ctx.set_option("emit_bp_groups", 1)
        rb = ctx.upload(pb)
        ctx.compare_resident(rb)
        res = ctx.download(rb, group_metrics=False)
        assert agrees(res, want)
        sums = ctx.label_tallies_compact(rb, 1, off, idx)
        assert np.array_equal(sums[0, :WORDS], want.tally[:WORDS])
        rb.free()
    finally:
        ctx.close()


@pytest.mark.parametrize("world", [2, 3])
def test_shard_sums_add_up(job, world):
    import aardvark_amd
    ctx, pb, want, batch = job["ctx"], job["pb"], job["want"], job["batch"]
    lib = ctx.lib
    n_labels = job["B"] + 1
    off, idx, lists = interval_labels(batch, n_labels, 60, job["span"])
    sums = oracle_sums(want, lists, n_labels)
    lib.avk_packed_shard_make.argtypes = [P(aardvark_amd._abi.AvkPackedBatch), P(C.c_uint64), C.c_uint64, C.c_uint32, C.c_uint32, P(C.c_void_p)]
    lib.avk_packed_shard_batch.restype = P(aardvark_amd._abi.AvkPackedBatch)
    lib.avk_packed_shard_batch.argtypes = [C.c_void_p]
    lib.avk_packed_shard_free.argtypes = [C.c_void_p]
    st = pb.c_struct()
    ids = np.arange(pb.n_regions, dtype=np.uint64)
    total = np.zeros((n_labels, TALLY_LEN), np.uint64)
    cfg = aardvark_amd._abi.AvkCompareConfig(50, 0, 0)
    for rank in range(world):
        h = C.c_void_p()
        assert lib.avk_packed_shard_make(C.byref(st), ids.ctypes.data_as(P(C.c_uint64)), 0, rank, world, C.byref(h)) == 0
        _, soff, sidx = dist.shard_labels(lib, h, n_labels, off, idx)
        sb = lib.avk_packed_shard_batch(h).contents
        m = int(sb.n_regions)
        status = np.full(m + 1, -1, np.int32)
        ro = aardvark_amd._abi.AvkResultBatch()
        ro.status = status.ctypes.data_as(P(C.c_int32))
        lab, keep = aardvark_amd._abi.region_labels(n_labels, soff, sidx)
        ctx._check(lib.avk_compare_packed_labels(ctx.handle, C.byref(sb), None, C.byref(lab), C.byref(cfg), C.byref(ro), total.ctypes.data_as(P(C.c_uint64))))
        lib.avk_packed_shard_free(h)
    assert np.array_equal(total, sums)


def refusal_cases(n):
    good_off = np.arange(n + 1, dtype=np.uint64)
    good_idx = (np.arange(n) % 4).astype(np.uint32)
    down = good_off.copy()
    down[n // 2] = down[n // 2 + 1] + 1
    big = good_idx.copy()
    big[n - 1] = 4
    return [("decreasing label_off", down, good_idx, True, "label_off must not decrease"), ("index out of range", good_off, big, True, "label index 4 of 4"),
            ("label_idx missing", good_off, None, True, "label_idx missing"), ("label_tallies missing", good_off, good_idx, False, "label_tallies missing")]


@pytest.mark.parametrize("entry", ["avk_compare_packed_labels", "avk_compare_packed_submit_labels"])
def test_refusals_then_a_correct_solve(job, entry):
    """each refusal is AVK_E_ARG with its text, nothing is queued, and the same context solves the next batch correctly"""
    ctx, pb, want = job["ctx"], job["pb"], job["want"]
    lib = ctx.lib
    pinned = ctx.pinned_packed(pb)
    st, cfg = pinned.c_struct(), __import__("aardvark_amd")._abi.AvkCompareConfig(50, 0, 0)
    sums = np.zeros((4, TALLY_LEN), np.uint64)
    for name, off, idx, with_sums, text in refusal_cases(pb.n_regions):
        res = ctx.pinned_results(pinned, packed="only")
        ro = res.c_struct()
        lab = AvkRegionLabels(4, off.ctypes.data_as(P(C.c_uint64)), idx.ctypes.data_as(P(C.c_uint32)) if idx is not None else None)
        args = [ctx.handle, C.byref(st), None, C.byref(lab), C.byref(cfg), C.byref(ro), sums.ctypes.data_as(P(C.c_uint64)) if with_sums else None]
        handle = C.c_void_p()
        if entry.endswith("submit_labels"):
            args.append(C.byref(handle))
        assert getattr(lib, entry)(*args) == -1, name
        assert text in lib.avk_last_error(ctx.handle).decode(), name
        assert not handle.value and not sums.any()
        after = ctx.solve_packed(pb, res=ResultBatch(pb, sequences=False, group_metrics=False))
        assert agrees(after, want), name


def test_tool_takes_the_compact_route(tmp_path, oracle):
    """-s on the packed feed: summary.tsv byte-identical to the oracle's text, -v names the compact route; --batch-form wide names the other one"""
    import subprocess
    import test_feeder
    fo = test_feeder.fo  # (oracle/feeder_oracle.py, on the path test_feeder sets up)
    from aardvark_amd import feeder
    from test_feeder import cli_path, write_case_files, write_text
    p, contig, want_batch = write_case_files(tmp_path, 2500, 1_200_000)
    rng = np.random.default_rng(8)
    names = ["s%02d" % i for i in range(20)]
    for i, name in enumerate(names):
        iv = sorted((int(s), int(s) + int(w)) for s, w in zip(rng.integers(0, 1_190_000, 30 + 10 * i), rng.integers(200, 40_000, 30 + 10 * i)))
        write_text(str(tmp_path / (name + ".bed")), "".join("chr20\t%d\t%d\n" % x for x in iv))
    write_text(str(tmp_path / "strat.tsv"), "".join("%s\t%s.bed\n" % (n, n) for n in names))
    strat = feeder.Stratifications(str(tmp_path / "strat.tsv"))
    genome = feeder.Genome(p["fa"])
    feed = feeder.feed_compare(p["t"], p["q"], p["bed"], genome, enable_trimming=False)
    res = oracle_lib.compare_batch(oracle, feed.batch, genome.contigs(), threads=CPUS)
    off, idx = strat.batch_labels(genome, feed.batch)
    blocks = np.zeros((20, 288), np.uint64)
    for r in range(feed.batch.n_regions):
        for l in idx[int(off[r]):int(off[r + 1])]:
            blocks[int(l), :286] += res.group_metrics[r].reshape(-1).astype(np.uint64)
    want = fo.summary_text(res.tally, "compare", ("GT", "BASEPAIR"), strat_blocks=[(l, blocks[i]) for i, l in enumerate(strat.labels)])
    base = [cli_path(), "-r", p["fa"], "-t", p["t"], "-q", p["q"], "-b", p["bed"], "-o", p["out"], "--disable-variant-trimming", "-s", str(tmp_path / "strat.tsv"),
            "--batch-regions", "900", "-v"]
    r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert open(os.path.join(p["out"], "summary.tsv")).read() == want
    assert "Stratified sums: from the compact results" in r.stderr
    r = subprocess.run(base + ["--batch-form", "wide"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert open(os.path.join(p["out"], "summary.tsv")).read() == want
    assert "Stratified sums: from per-region metric blocks on the GPU" in r.stderr
