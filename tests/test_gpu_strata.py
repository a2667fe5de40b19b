"""Stratification sets resident on a real MI355X and the containment lists made there (avk_strata.inl): avk_strata_region_labels against the host's lists
(avf_strat_batch_labels) bit for bit, avk_label_tallies_strata and avk_compare_packed_strata against sums of the ORACLE's per-region blocks over the host's lists,
and the command-line tool with --strat-lists device | host.  Every comparison is exact.

The job: the regions of the first two contigs of a genome slice (scale 0.003) and fuzz regions on a third contig, 4,099 regions in all (not a multiple of 64 or
256: 17 workgroups of the list kernels, the last one partly filled), and 1,000 of them drawn from all three contigs.  Label sets of 5 and of 75 labels (75: one more
than fits a 160 KB label block, several blocks of a 64 KB one; three mask words per region): one label on every region, one on none (a chromosome the genome lacks),
one whose intervals end mid-batch, the rest random intervals."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import escapes_lib
import oracle_lib
import scenarios
import strata_emu_lib as sx
from aardvark_amd import CompactBatch, PackedBatch, ResultBatch, feeder, synth
from aardvark_amd._abi import TALLY_LEN

pytestmark = pytest.mark.gpu
CPUS = min(os.cpu_count() or 1, 16)
WORDS = 13 * 22
N_ALL, N_SMALL = 4099, 1000


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
        beds["x%02d" % x] = sorted(iv)
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


@pytest.fixture(scope="module")
def job(oracle, tmp_path_factory):
    """one context, the 4,099-region batch and its 1,000-region selection, the oracle's results, the two label sets with the HOST's lists: shared, never changed"""
    import aardvark_amd
    from test_feeder import write_text
    folder = str(tmp_path_factory.mktemp("gpu_strata"))
    gcontigs, gbatch = synth.config_genome(scale=0.003, threads=4)
    assert (np.diff(gbatch.contig_idx.astype(np.int64)) >= 0).all()
    n_two = int((gbatch.contig_idx < 2).sum())
    fcontigs, fuzz = scenarios.fuzz_regions(77, N_ALL - n_two, max_vars=4)
    fuzz.contig_idx[:] = 2
    batch = synth.concat_batches([escapes_lib.reordered(gbatch, np.arange(n_two)), fuzz])
    contigs = [gcontigs[0], gcontigs[1], fcontigs[0]]
    assert batch.n_regions == N_ALL
    want = oracle_lib.compare_batch(oracle, batch, contigs, threads=CPUS)
    assert (np.asarray(want.status) == 0).sum() > 3000
    pick = np.r_[0:400, n_two - 300:n_two, N_ALL - 300:N_ALL]
    small = escapes_lib.reordered(batch, pick)
    assert small.n_regions == N_SMALL and len(set(small.contig_idx.tolist())) == 3
    genome = feeder.Genome(sx.write_genome(folder, write_text))
    ctx = aardvark_amd.Context(0)
    ctx.set_option("lane_min_regions", 0)
    ctx.set_option("lane_min_batch", 0)
    ctx.upload_reference(contigs)
    lens = [len(c) for c in contigs]
    sets = {}
    for n_labels in (5, 75, 300):  # (300: more than the 256 labels the mask kernel stages at a time, ten mask words a region, the last one partly filled)
        strat = feeder.Stratifications(write_label_sets(folder, n_labels, lens, 100 + n_labels))
        assert len(strat.labels) == n_labels
        exported = strat.export(genome)
        sets[n_labels] = dict(strat=strat, exported=exported, strata=ctx.upload_strata(*exported), lists={N_ALL: strat.batch_labels(genome, batch), N_SMALL: strat.batch_labels(genome, small)})
    batches = {N_ALL: batch, N_SMALL: small}
    wants = {N_ALL: want, N_SMALL: oracle_lib.compare_batch(oracle, small, contigs, threads=CPUS)}
    pbs = {n: PackedBatch.from_compact(CompactBatch.from_region_batch(b)) for n, b in batches.items()}
    yield dict(ctx=ctx, contigs=contigs, batches=batches, pbs=pbs, wants=wants, sets=sets, genome=genome)
    for s in sets.values():
        s["strata"].free()
    ctx.close()


def same_lists(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_the_label_sets_are_what_the_file_says(job):
    for n_labels, s in job["sets"].items():
        off, idx = s["lists"][N_ALL]
        per = np.bincount(idx, minlength=n_labels)
        batch = job["batches"][N_ALL]
        assert N_ALL - 200 < per[0] <= N_ALL and per[1] == 0  # (a_every: every region that has calls and a span)
        assert per[0] == int(((batch.t_cnt.astype(np.int64) + batch.q_cnt) > 0).sum())
        assert per[1] == 0 and 0 < per[2] < N_ALL and (per[3:] > 0).all()
        on_b = np.flatnonzero(batch.contig_idx == 1)
        inside = [2 in idx[int(off[r]):int(off[r + 1])] for r in on_b]
        assert inside[0] and not inside[-1]  # the label's intervals end in the middle of the batch
    assert job["ctx"].label_block() in (28, 71)


@pytest.mark.parametrize("n", [N_SMALL, N_ALL])
@pytest.mark.parametrize("n_labels", [5, 75])
@pytest.mark.parametrize("form", ["wide", "compact", "packed", "packed_source=0", "escaped"])
def test_region_labels_equal_the_hosts(job, form, n_labels, n):
    ctx, s = job["ctx"], job["sets"][n_labels]
    batch, pb = job["batches"][n], job["pbs"][n]
    src = {"wide": batch, "compact": CompactBatch.from_region_batch(batch), "packed": pb, "packed_source=0": pb}.get(form)
    if form == "escaped":
        src = escapes_lib.promote(pb, regions=[1, 7, pb.n_regions - 1], slots=[0, 5, 2 * pb.n_regions - 2], calls=[0, 3, pb.n_variants - 1])
        assert not src.escapes.empty()
    ctx.set_option("packed_source", 0 if form == "packed_source=0" else 1)
    rb = ctx.upload(src)
    try:
        assert same_lists(ctx.strata_region_labels(rb, s["strata"]), s["lists"][n])
    finally:
        rb.free()
        ctx.set_option("packed_source", 1)


@pytest.mark.parametrize("form", ["wide", "packed", "escaped"])
def test_more_labels_than_a_staging_chunk(job, form):
    """300 labels: the mask kernel stages the tree table's row a second time, writes mask words 8 and 9 from it, the last one 12 labels wide; lists against the
    host's, the one-call sums against the oracle's and the host route's"""
    ctx, s, n = job["ctx"], job["sets"][300], N_ALL
    batch, pb, want = job["batches"][n], job["pbs"][n], job["wants"][n]
    off, idx = s["lists"][n]
    assert (np.bincount(idx, minlength=300)[256:] > 0).all()
    src = {"wide": batch, "packed": pb}.get(form)
    if form == "escaped":
        src = escapes_lib.promote(pb, regions=[1, 7, pb.n_regions - 1], slots=[0, 5, 2 * pb.n_regions - 2], calls=[0, 3, pb.n_variants - 1])
    rb = ctx.upload(src)
    try:
        assert same_lists(ctx.strata_region_labels(rb, s["strata"]), (off, idx))
    finally:
        rb.free()
    if form != "wide":
        got = ctx.solve_packed(src, res=ResultBatch(src, sequences=False, group_metrics=False), strata=s["strata"])
        host = ctx.solve_packed(src, res=ResultBatch(src, sequences=False, group_metrics=False), labels=(300, off, idx))
        assert agrees(got, want) and np.array_equal(got.label_tallies, host.label_tallies) and np.array_equal(got.label_tallies, oracle_sums(want, off, idx, 300))


def test_region_labels_cap_too_small_then_right(job):
    import aardvark_amd
    ctx, s, pb = job["ctx"], job["sets"][75], job["pbs"][N_ALL]
    want_off, want_idx = s["lists"][N_ALL]
    u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    rb = ctx.upload(pb)
    try:
        off = np.zeros(N_ALL + 1, np.uint64)
        idx = np.full(len(want_idx) + 8, 0xABCDEF01, np.uint32)
        rc = ctx.lib.avk_strata_region_labels(ctx.handle, rb.handle, s["strata"].handle, off.ctypes.data_as(u64p), idx.ctypes.data_as(u32p), len(want_idx) - 1)
        assert rc == -1 and "are needed" in ctx.lib.avk_last_error(ctx.handle).decode()
        assert int(off[N_ALL]) == len(want_idx) and (idx == 0xABCDEF01).all()
        rc = ctx.lib.avk_strata_region_labels(ctx.handle, rb.handle, s["strata"].handle, off.ctypes.data_as(u64p), idx.ctypes.data_as(u32p), len(want_idx))
        assert rc == 0 and np.array_equal(off, want_off) and np.array_equal(idx[:len(want_idx)], want_idx) and (idx[len(want_idx):] == 0xABCDEF01).all()
        off[:] = 7  # offsets only
        assert ctx.lib.avk_strata_region_labels(ctx.handle, rb.handle, s["strata"].handle, off.ctypes.data_as(u64p), None, 0) == 0 and np.array_equal(off, want_off)
    finally:
        rb.free()


@pytest.mark.parametrize("n", [N_SMALL, N_ALL])
@pytest.mark.parametrize("n_labels", [5, 75])
def test_resident_sums_equal_the_oracles(job, n_labels, n):
    """sums are ADDED, words 286 / 287 stay; 75 labels: more passes than one"""
    ctx, s, pb = job["ctx"], job["sets"][n_labels], job["pbs"][n]
    sums = oracle_sums(job["wants"][n], *s["lists"][n], n_labels)
    assert sums[0].any() and not sums[1].any() and sums[3:].any()
    ctx.set_option("emit_group_metrics", 0)
    ctx.set_option("emit_bp_groups", 1)
    rb = ctx.upload(pb)
    try:
        ctx.compare_resident(rb)
        out = np.zeros((n_labels, TALLY_LEN), np.uint64)
        out[:, WORDS:] = 7
        ctx.label_tallies_strata(rb, s["strata"], out=out)
        assert np.array_equal(out[:, :WORDS], sums[:, :WORDS]) and (out[:, WORDS:] == 7).all()
        ctx.label_tallies_strata(rb, s["strata"], out=out)
        assert np.array_equal(out[:, :WORDS], 2 * sums[:, :WORDS])
        assert np.array_equal(ctx.label_tallies_compact(rb, n_labels, *s["lists"][n]), sums)
    finally:
        rb.free()
        ctx.set_option("emit_bp_groups", 0)


def agrees(res, want):
    n = len(want.status)
    return np.array_equal(np.asarray(res.status)[:n], want.status) and np.array_equal(np.asarray(res.tally, np.uint64)[:WORDS], np.asarray(want.tally, np.uint64)[:WORDS])


def same(a, b):
    return np.array_equal(a.region_packed, b.region_packed) and np.array_equal(a.var_packed, b.var_packed) and np.array_equal(a.tally, b.tally)


def test_resident_refusals_then_a_correct_solve(job):
    """the refusals of avk_label_tallies_compact hold: no BASEPAIR groups, not device-packed; the same context then solves correctly"""
    import aardvark_amd
    ctx, s, pb, batch, want = job["ctx"], job["sets"][5], job["pbs"][N_SMALL], job["batches"][N_SMALL], job["wants"][N_SMALL]
    ctx.set_option("emit_bp_groups", 0)
    rb = ctx.upload(pb)
    ctx.compare_resident(rb)
    with pytest.raises(aardvark_amd.AardvarkAmdError, match="error -4.*emit_bp_groups"):
        ctx.label_tallies_strata(rb, s["strata"])
    rb.free()
    assert agrees(ctx.solve_packed(pb, res=ResultBatch(pb, sequences=False, group_metrics=False)), want)
    ctx.set_option("device_pack", 0)
    ctx.set_option("emit_bp_groups", 1)
    rb = ctx.upload(batch)
    try:
        ctx.compare_resident(rb)
        with pytest.raises(aardvark_amd.AardvarkAmdError, match="error -4.*device_pack"):
            ctx.label_tallies_strata(rb, s["strata"])
        with pytest.raises(aardvark_amd.AardvarkAmdError, match="error -4.*device_pack"):
            ctx.strata_region_labels(rb, s["strata"])
    finally:
        rb.free()
        ctx.set_option("device_pack", 1)
        ctx.set_option("emit_bp_groups", 0)
    got = ctx.solve_packed(pb, res=ResultBatch(pb, sequences=False, group_metrics=False), strata=s["strata"])
    assert agrees(got, want) and np.array_equal(got.label_tallies, oracle_sums(want, *s["lists"][N_SMALL], 5))


@pytest.mark.parametrize("n", [N_SMALL, N_ALL])
@pytest.mark.parametrize("n_labels", [5, 75])
def test_one_call_form(job, n_labels, n):
    """the sums equal avk_compare_packed_labels fed the host's lists (and the oracle's); the results equal the unlabelled call's; a NULL handle is that call"""
    ctx, s, pb, want = job["ctx"], job["sets"][n_labels], job["pbs"][n], job["wants"][n]
    off, idx = s["lists"][n]
    new = lambda: ResultBatch(pb, sequences=False, group_metrics=False, packed="only")
    plain = ctx.solve_packed(pb, res=new())
    host = ctx.solve_packed(pb, res=new(), labels=(n_labels, off, idx))
    got = ctx.solve_packed(pb, res=new(), strata=s["strata"])
    assert same(got, plain) and np.array_equal(got.label_tallies, host.label_tallies) and np.array_equal(got.label_tallies, oracle_sums(want, off, idx, n_labels))
    wide = ctx.solve_packed(pb, res=ResultBatch(pb, sequences=False, group_metrics=False), strata=s["strata"])
    assert agrees(wide, want) and np.array_equal(wide.label_tallies, got.label_tallies)
    # sums are ADDED to the caller's block
    twice = ctx.solve_packed(pb, res=new(), strata=s["strata"], label_tallies=got.label_tallies.copy())
    assert np.array_equal(twice.label_tallies, 2 * host.label_tallies)
    # a NULL handle: the call without labels
    res = new()
    pbs, cfg, ro = pb.c_struct(), __import__("aardvark_amd")._abi.AvkCompareConfig(50, 0, 0), res.c_struct()
    sums = np.zeros((n_labels, TALLY_LEN), np.uint64)
    assert ctx.lib.avk_compare_packed_strata(ctx.handle, C.byref(pbs), None, None, C.byref(cfg), C.byref(ro), sums.ctypes.data_as(C.POINTER(C.c_uint64))) == 0
    assert same(res, plain) and not sums.any()


def test_one_call_form_with_escapes(job):
    ctx, s, pb, want = job["ctx"], job["sets"][75], job["pbs"][N_SMALL], job["wants"][N_SMALL]
    src = escapes_lib.promote(pb, regions=[1, 7, pb.n_regions - 1], slots=[0, 5, 2 * pb.n_regions - 2], calls=[0, 3, pb.n_variants - 1])
    got = ctx.solve_packed(src, res=ResultBatch(src, sequences=False, group_metrics=False), strata=s["strata"])
    assert agrees(got, want) and np.array_equal(got.label_tallies, oracle_sums(want, *s["lists"][N_SMALL], 75))


def test_consecutive_calls_with_different_handles_do_not_mix(job):
    ctx, pb, want = job["ctx"], job["pbs"][N_ALL], job["wants"][N_ALL]
    a, b = job["sets"][75], job["sets"][5]
    new = lambda: ResultBatch(pb, sequences=False, group_metrics=False, packed="only")
    first = ctx.solve_packed(pb, res=new(), strata=a["strata"])
    second = ctx.solve_packed(pb, res=new(), strata=b["strata"])
    third = ctx.solve_packed(pb, res=new(), strata=a["strata"])
    assert np.array_equal(first.label_tallies, oracle_sums(want, *a["lists"][N_ALL], 75)) and np.array_equal(third.label_tallies, first.label_tallies)
    assert np.array_equal(second.label_tallies, oracle_sums(want, *b["lists"][N_ALL], 5)) and same(first, second)


def test_capacity_retry_counts_repaired_regions(oracle):
    """the starved-workspace context of tests/test_gpu_label_compact.py: regions come back AVK_ST_CAPACITY and are repaired by the download; one label on every
    region sums to the oracle's tally in the one-call form (a repaired region's list is fetched from the device) and in the resident form after the download"""
    import aardvark_amd
    ctx = aardvark_amd.Context(0)
    try:
        for k, v in dict(lds_bytes_per_wave=2048, lds2_bytes_per_wave=0, ws_bytes_per_wave=0, big_ws_bytes=4096).items():
            ctx.set_option(k, v)
        contigs, batch = scenarios.fuzz_regions(341, 400, max_vars=9, max_len=12)
        ctx.upload_reference(contigs)
        want = oracle_lib.compare_batch(oracle, batch, contigs, threads=CPUS)
        pb = PackedBatch.from_compact(CompactBatch.from_region_batch(batch))
        # label 0: every region; label 1: nothing; label 2: the first half of the contig
        strata = ctx.upload_strata(3, 1, np.array([0, 1, 1, 2], np.uint64), np.array([0, 0], np.uint32), np.array([10_000_000, 2_000], np.uint32))
        ctx.set_option("capacity_retry", 0)
        starved = ctx.solve_packed(pb, res=ResultBatch(pb, sequences=False, group_metrics=False))
        assert (starved.status == 21).any()
        ctx.set_option("capacity_retry", 1)
        got = ctx.solve_packed(pb, res=ResultBatch(pb, sequences=False, group_metrics=False), strata=strata)
        assert agrees(got, want) and np.array_equal(got.label_tallies[0, :WORDS], want.tally[:WORDS]) and not got.label_tallies[1].any()
        ctx.set_option("emit_bp_groups", 1)
        rb = ctx.upload(pb)
        ctx.compare_resident(rb)
        assert agrees(ctx.download(rb, group_metrics=False), want)
        sums = ctx.label_tallies_strata(rb, strata)
        off, idx = ctx.strata_region_labels(rb, strata)
        assert np.array_equal(sums[0, :WORDS], want.tally[:WORDS]) and np.array_equal(sums, got.label_tallies) and np.array_equal(sums, oracle_sums(want, off, idx, 3))
        assert 0 < sums[2].sum() < sums[0].sum()
        rb.free()
        strata.free()
    finally:
        ctx.close()


def test_upload_refusals_and_the_empty_set(job):
    import aardvark_amd
    ctx, pb = job["ctx"], job["pbs"][N_SMALL]
    with pytest.raises(aardvark_amd.AardvarkAmdError, match="tree_off must not decrease"):
        ctx.upload_strata(1, 2, np.array([0, 2, 1], np.uint64), np.zeros(2, np.uint32), np.ones(2, np.uint32))
    with pytest.raises(aardvark_amd.AardvarkAmdError, match="not sorted"):
        ctx.upload_strata(1, 1, np.array([0, 2], np.uint64), np.array([5, 4], np.uint32), np.array([9, 9], np.uint32))
    empty = ctx.upload_strata(0, 3, np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint32))
    assert empty.n_labels == 0
    plain = ctx.solve_packed(pb, res=ResultBatch(pb, sequences=False, group_metrics=False, packed="only"))
    got = ctx.solve_packed(pb, res=ResultBatch(pb, sequences=False, group_metrics=False, packed="only"), strata=empty)
    assert same(got, plain) and got.label_tallies.size == 0
    empty.free()


def test_tool_lists_on_the_device_and_on_the_host(tmp_path, oracle):
    """-s with --strat-lists device and host: summary.tsv byte-identical, equal to the oracle's text; -v names the route; --devices 0,0 gives the same file"""
    import test_feeder
    fo = test_feeder.fo
    from test_feeder import cli_path, write_case_files, write_text
    p, contig, want_batch = write_case_files(tmp_path, 2500, 1_200_000)
    rng = np.random.default_rng(8)
    names = ["s%02d" % i for i in range(20)]
    for i, name in enumerate(names):
        iv = sorted((int(s), int(s) + int(w)) for s, w in zip(rng.integers(0, 1_190_000, 30 + 10 * i), rng.integers(200, 40_000, 30 + 10 * i)))
        write_text(str(tmp_path / (name + ".bed")), "".join("chr20\t%d\t%d\n" % x for x in iv) + ("chrQ\t0\t1000\n" if i % 3 == 0 else ""))
    write_text(str(tmp_path / "strat.tsv"), "".join("%s\t%s.bed\n" % (n, n) for n in names))
    strat = feeder.Stratifications(str(tmp_path / "strat.tsv"))
    genome = feeder.Genome(p["fa"])
    feed = feeder.feed_compare(p["t"], p["q"], p["bed"], genome, enable_trimming=False)
    res = oracle_lib.compare_batch(oracle, feed.batch, genome.contigs(), threads=CPUS)
    off, idx = strat.batch_labels(genome, feed.batch)
    want = fo.summary_text(res.tally, "compare", ("GT", "BASEPAIR"), strat_blocks=[(l, b) for l, b in zip(strat.labels, oracle_sums(res, off, idx, 20))])
    base = [cli_path(), "-r", p["fa"], "-t", p["t"], "-q", p["q"], "-b", p["bed"], "-o", p["out"], "--disable-variant-trimming", "-s", str(tmp_path / "strat.tsv"),
            "--batch-regions", "900", "-v"]
    texts = {}
    for route, extra, note in (("default", [], "listed on the GPU"), ("device", ["--strat-lists", "device"], "listed on the GPU"), ("host", ["--strat-lists", "host"], "listed on the host"),
                               ("devices", ["--devices", "0,0"], "listed on the GPU")):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert "Region labels: " + note in r.stderr, r.stderr
        texts[route] = open(os.path.join(p["out"], "summary.tsv"), "rb").read()
        os.remove(os.path.join(p["out"], "summary.tsv"))
    assert texts["device"] == texts["host"] == texts["default"] == texts["devices"] == want.encode()
    assert "intervals of 20 labels uploaded" in r.stderr
    r = subprocess.run(base + ["--strat-lists", "both"], capture_output=True, text=True)
    assert r.returncode != 0 and "--strat-lists takes device or host" in r.stderr
