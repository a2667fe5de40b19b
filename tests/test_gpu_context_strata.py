"""The sequence-context labels of a stratified job on a real MI355X (avk_context_mask_kernel behind avk_strata_mask_kernel): the lists, masks and per-label sums
of handles with GC and homopolymer labels behind 0, 1, 31, 32 and 33 BED labels, against the numpy restatement of the rule (tests/context_lib.py, whose builder
has asserted that the inputs reach every branch of it) and against sums of the unlabelled wide call's per-region blocks added on the host.  Every comparison
is exact.  Batches of at most 513 regions."""

import os

import numpy as np
import pytest

import context_lib as cl
from aardvark_amd import CompactBatch, ContextSpec, PackedBatch, ResultBatch
from aardvark_amd._abi import TALLY_LEN

from test_context_strata import TOOL_REFUSALS

pytestmark = pytest.mark.gpu
WORDS = 13 * 22


def context_spec(spec):
    return ContextSpec(spec.gc_edges, spec.hp_edges, spec.gc_pad, spec.hp_pad)


def per_region(lists):
    off, idx = lists
    return [np.asarray(idx)[int(off[r]):int(off[r + 1])].tolist() for r in range(len(off) - 1)]


def host_sums(res, off, idx, n_labels):
    """the sums of the solved regions' metric blocks under lists, added on the host"""
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
def gpu():
    """one context with the job's reference, the jobs of 1 .. 513 regions under the default spec (numpy labels computed once), their packed batches and the
    unlabelled wide call's results: shared, never changed"""
    import aardvark_amd
    ctx = aardvark_amd.Context(0)
    ctx.set_option("lane_min_regions", 0)
    ctx.set_option("lane_min_batch", 0)
    jobs = {n: cl.Job(cl.DEFAULT, n) for n in (1, 255, 256, 257, 513)}
    assert jobs[513].whole and jobs[257].whole
    ctx.upload_reference(jobs[513].contigs)
    pbs = {n: PackedBatch.from_compact(CompactBatch.from_region_batch(j.batch())) for n, j in jobs.items()}
    wide = {n: ctx.solve_packed(pbs[n], res=ResultBatch(pbs[n], sequences=False)) for n in (257, 513)}
    assert (np.asarray(wide[513].status) == 0).sum() > 400
    yield dict(ctx=ctx, jobs=jobs, pbs=pbs, wide=wide)
    ctx.close()


def handles(ctx, contigs, n_bed, spec):
    """(a handle with n_bed BED labels and the spec's context labels, the BED-only handle of the same sets or None)"""
    trees = cl.bed_trees(n_bed, contigs)
    both = ctx.upload_strata(*trees, context=context_spec(spec))
    assert both.n_labels == n_bed + spec.n_labels and both.n_context_labels == spec.n_labels
    return both, (ctx.upload_strata(*trees) if n_bed else None)


def expected_lists(ctx, rb, job, n_bed, bed_only):
    ctx_lists = cl.lists_of_bits(job.bits, n_bed)
    if not n_bed:
        return ctx_lists
    bed_lists = ctx.strata_region_labels(rb, bed_only)
    assert len(bed_lists[1]) >= job.n - 1  # (label 0 holds every contig whole: every region with a span has it)
    return cl.merge_lists(bed_lists, ctx_lists)


@pytest.mark.parametrize("n_bed", [0, 1, 31, 32, 33])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_region_labels(gpu, n, n_bed):
    """the lists of a resident batch: the BED labels' entries are those of a BED-only handle, the context labels' entries those of the numpy rule, behind them"""
    ctx, job = gpu["ctx"], gpu["jobs"][n]
    both, bed_only = handles(ctx, job.contigs, n_bed, job.spec)
    rb = ctx.upload(gpu["pbs"][n])
    try:
        want = expected_lists(ctx, rb, job, n_bed, bed_only)
        got = ctx.strata_region_labels(rb, both)
        assert np.array_equal(got[0], want[0]) and per_region(got) == per_region(want)
        if job.whole:
            assert set(np.asarray(got[1]).tolist()) >= set(range(n_bed, n_bed + job.spec.n_labels))  # every context label on some region
    finally:
        rb.free()
        both.free()
        if bed_only:
            bed_only.free()


@pytest.mark.parametrize("spec", ["other", "same_pad", "gc_only", "hp_only"])
def test_region_labels_other_specs(gpu, spec):
    """pads of 0 and different pads, one window for both families, one family alone — on a reference of their own (the placed runs follow the spec's edges)"""
    import aardvark_amd
    spec = {"other": cl.OTHER, "same_pad": cl.SAME_PAD, "gc_only": cl.Spec(cl.DEFAULT.gc_edges, (), 50, 0), "hp_only": cl.Spec((), (4, 7, 12, 21), 0, 5)}[spec]
    job = cl.Job(spec, 300)
    assert job.whole
    ctx = aardvark_amd.Context(0)
    try:
        ctx.upload_reference(job.contigs)
        both, bed_only = handles(ctx, job.contigs, 3, spec)
        rb = ctx.upload(PackedBatch.from_compact(CompactBatch.from_region_batch(job.batch())))
        want = expected_lists(ctx, rb, job, 3, bed_only)
        got = ctx.strata_region_labels(rb, both)
        assert np.array_equal(got[0], want[0]) and per_region(got) == per_region(want)
        rb.free(), both.free(), bed_only.free()
    finally:
        ctx.close()


@pytest.mark.parametrize("n_bed", [0, 31])
def test_one_call_sums(gpu, n_bed):
    """solve_packed(strata=..): per-label sums, word for word the sums of the unlabelled wide call's blocks under the numpy labels — a handle of context labels
    only, and one combined with BED labels (the shared word)"""
    ctx, job, pb = gpu["ctx"], gpu["jobs"][513], gpu["pbs"][513]
    both, bed_only = handles(ctx, job.contigs, n_bed, job.spec)
    rb = ctx.upload(pb)
    try:
        off, idx = expected_lists(ctx, rb, job, n_bed, bed_only)
        want = host_sums(gpu["wide"][513], off, idx, both.n_labels)
        assert want[n_bed:].any(axis=1).all()
        got = ctx.solve_packed(pb, res=ResultBatch(pb, sequences=False, group_metrics=False), strata=both)
        assert np.array_equal(got.status, gpu["wide"][513].status) and np.array_equal(got.label_tallies, want)
    finally:
        rb.free()
        both.free()
        if bed_only:
            bed_only.free()


def test_two_tickets_two_specs_handle_freed_before_the_wait(gpu):
    """submit_packed(strata=..): two batches in flight under two specs — the mask tally reads the context bits; both handles are freed before the waits"""
    ctx = gpu["ctx"]
    other = cl.Spec((0, 40, 60, 101), (2, 5), 20, 3)
    plan = [(513, 33, cl.DEFAULT), (257, 1, other)]
    wants, tickets, held = [], [], []
    for n, n_bed, spec in plan:
        job = gpu["jobs"][n]
        bits = job.bits if spec is cl.DEFAULT else cl.bits_of_regions(job.contigs, spec, job.regions)
        both, bed_only = handles(ctx, job.contigs, n_bed, spec)
        rb = ctx.upload(gpu["pbs"][n])
        off, idx = cl.merge_lists(ctx.strata_region_labels(rb, bed_only), cl.lists_of_bits(bits, n_bed))
        rb.free(), bed_only.free()
        wants.append(host_sums(gpu["wide"][n], off, idx, both.n_labels))
        held.append(both)
    for (n, _, _), both in zip(plan, held):
        p = ctx.pinned_packed(gpu["pbs"][n])
        tickets.append(ctx.submit_packed(p, res=ctx.pinned_results(p, packed="only"), strata=both))
    for both in held:
        both.free()
        assert not both.handle
    for k in (1, 0):
        got = tickets[k].wait()
        assert np.array_equal(got.label_tallies, wants[k]), k
        assert wants[k][plan[k][1]:].any()


def test_resident_tallies(gpu):
    """avk_label_tallies_strata on a solved resident batch"""
    ctx, job, pb = gpu["ctx"], gpu["jobs"][257], gpu["pbs"][257]
    both, bed_only = handles(ctx, job.contigs, 32, job.spec)
    ctx.set_option("emit_bp_groups", 1)
    rb = ctx.upload(pb)
    try:
        off, idx = expected_lists(ctx, rb, job, 32, bed_only)
        want = host_sums(gpu["wide"][257], off, idx, both.n_labels)
        ctx.compare_resident(rb)
        got = ctx.label_tallies_strata(rb, both)
        assert np.array_equal(got, want) and want[32:].any()
    finally:
        ctx.set_option("emit_bp_groups", 0)
        rb.free(), both.free(), bed_only.free()


def test_escapes_and_a_long_window():
    """a batch whose packed form needs its escape lists, with a span of 68,000 bases: the long loop on one lane"""
    import aardvark_amd
    job = cl.Job(cl.DEFAULT, 300, long=True)
    pb = PackedBatch.from_compact(CompactBatch.from_region_batch(job.batch()), escapes=True)
    assert len(pb.escapes.esc_region) >= 1
    longest = max(cl.span_of(r)[1] - cl.span_of(r)[0] for r in job.regions if cl.span_of(r))
    assert longest + 1 + 2 * job.spec.gc_pad >= 65_536
    ctx = aardvark_amd.Context(0)
    try:
        ctx.upload_reference(job.contigs)
        both, bed_only = handles(ctx, job.contigs, 2, job.spec)
        rb = ctx.upload(pb)
        want = expected_lists(ctx, rb, job, 2, bed_only)
        got = ctx.strata_region_labels(rb, both)
        assert np.array_equal(got[0], want[0]) and per_region(got) == per_region(want)
        wide = ctx.solve_packed(pb, res=ResultBatch(pb, sequences=False))
        one_call = ctx.solve_packed(pb, res=ResultBatch(pb, sequences=False, group_metrics=False), strata=both)
        assert np.array_equal(one_call.label_tallies, host_sums(wide, want[0], want[1], both.n_labels))
        rb.free(), both.free(), bed_only.free()
    finally:
        ctx.close()


def test_refusals_leave_the_sums_untouched(gpu):
    """no reference uploaded, and a reference with another number of contigs than the handle: AVK_E_ARG from every entry point, the caller's sums as they were"""
    import aardvark_amd
    job, pb = gpu["jobs"][257], gpu["pbs"][257]
    ctx = aardvark_amd.Context(0)
    try:
        zero = np.zeros(1, np.uint64)
        none = np.zeros(0, np.uint32)
        st = ctx.upload_strata(0, 4, zero, none, none, context=context_spec(cl.DEFAULT))  # (uploading the handle needs no reference)
        sums = np.full((st.n_labels, TALLY_LEN), 5, np.uint64)
        with pytest.raises(aardvark_amd.AardvarkAmdError, match="error -1.*avk_ref_upload has not been called"):
            ctx.solve_packed(pb, res=ResultBatch(pb, sequences=False, group_metrics=False), strata=st, label_tallies=sums)
        p = ctx.pinned_packed(pb)
        with pytest.raises(aardvark_amd.AardvarkAmdError, match="error -1.*avk_ref_upload has not been called"):
            ctx.submit_packed(p, res=ctx.pinned_results(p, packed="only"), strata=st, label_tallies=sums)
        ctx.upload_reference(job.contigs[:3])
        rb = ctx.upload(pb)
        for call in (lambda: ctx.solve_packed(pb, res=ResultBatch(pb, sequences=False, group_metrics=False), strata=st, label_tallies=sums),
                     lambda: ctx.submit_packed(p, res=ctx.pinned_results(p, packed="only"), strata=st, label_tallies=sums),
                     lambda: ctx.strata_region_labels(rb, st), lambda: ctx.label_tallies_strata(rb, st, out=sums)):
            with pytest.raises(aardvark_amd.AardvarkAmdError, match="error -1.*the reference has 3 contigs, the handle 4"):
                call()
        assert (sums == 5).all()
        rb.free()
        ctx.upload_reference(job.contigs)  # the same handle, once the reference fits it
        rb = ctx.upload(pb)
        assert per_region(ctx.strata_region_labels(rb, st)) == per_region(cl.lists_of_bits(job.bits))
        rb.free(), st.free()
    finally:
        ctx.close()


def _summary_rows(path):
    rows = [l.split("\t") for l in open(path).read().splitlines()]
    assert rows[0][:5] == ["compare_label", "comparison", "region_label", "filter", "variant_type"]
    return rows[1:]


def test_the_tool(tmp_path):
    """aardvark_amd_compare --context-strata on the tool tests' fixture files: the context rows of summary.tsv against the joint metrics of the tool's own
    per-region table (--output-debug of a run without the flag) summed under the numpy labels; the blocks in front of them byte for byte those of the run
    without the flag, which is the restated writer's file; one handle per --devices worker; every refused combination"""
    import gzip
    import subprocess

    import oracle_lib
    import test_feeder as tf
    from aardvark_amd import feeder
    fo = tf.fo
    p, contig, want_batch = tf.write_case_files(tmp_path, 2500, 1_200_000)
    beds = {"lowhalf": [(0, 600_000)], "highhalf": [(500_000, 1_200_000)], "tiles": [(k * 10_000, k * 10_000 + 4_000) for k in range(120)]}
    for name, iv in beds.items():
        tf.write_text(str(tmp_path / (name + ".bed")), "".join("chr20\t%d\t%d\n" % x for x in iv))
    strat_tsv = str(tmp_path / "strat.tsv")
    tf.write_text(strat_tsv, "".join("%s\t%s.bed\n" % (n, n) for n in beds))
    base = [tf.cli_path(), "-r", p["fa"], "-t", p["t"], "-q", p["q"], "-b", p["bed"], "--disable-variant-trimming"]

    def run(name, *extra, ok=True):
        out = str(tmp_path / name)
        r = subprocess.run(base + ["-o", out] + list(extra), capture_output=True, text=True)
        assert (r.returncode == 0) == ok, r.stderr
        return out, r

    # without the flag: today's file — the restated writer's over the oracle's blocks under the restated containment rule
    plain, _ = run("plain", "-s", strat_tsv, "--batch-regions", "900")
    ostrat = fo.load_stratifications(strat_tsv)
    regions, _ = fo.generate_regions(fo.load_calls(p["t"], "", False), fo.load_calls(p["q"], "", False), fo.read_bed(p["bed"]), fo.read_fasta(p["fa"]))
    res = oracle_lib.compare_batch(oracle_lib.load(), want_batch, [contig], threads=8)
    blocks = np.zeros((3, 288), np.uint64)
    for k, reg in enumerate(regions):
        for l in fo.region_labels(ostrat, reg):
            blocks[l, :286] += res.group_metrics[k].reshape(-1).astype(np.uint64)
    plain_text = open(plain + "/summary.tsv").read()
    assert plain_text == fo.summary_text(res.tally, "compare", ("GT", "BASEPAIR"), strat_blocks=[(l, blocks[i]) for i, (l, _) in enumerate(ostrat)])
    nolabels, _ = run("nolabels")
    # the tool's own per-region table, and the numpy labels of the tool's own regions
    dbg = str(tmp_path / "dbg")
    run("debug", "--output-debug", dbg)
    table = [l.split("\t") for l in gzip.open(dbg + "/region_summary.tsv.gz", "rt").read().splitlines()[1:]]
    genome = feeder.Genome(p["fa"])
    batch = feeder.feed_compare(p["t"], p["q"], p["bed"], genome, enable_trimming=False).batch
    contigs = [bytes(c) for c in genome.contigs()]
    ids = {int(i): r for r, i in enumerate(batch.region_id)}
    spans = []
    for r in range(batch.n_regions):
        lo, hi = None, 0
        for off, cnt in ((batch.t_off, batch.t_cnt), (batch.q_off, batch.q_cnt)):
            if cnt[r]:
                f, l = int(off[r]), int(off[r]) + int(cnt[r]) - 1
                lo = int(batch.var_pos[f]) if lo is None else min(lo, int(batch.var_pos[f]))
                hi = max(hi, int(batch.var_pos[l]) + int(batch.a0_len[l]))
        spans.append(None if lo is None or lo >= hi else (lo, hi - 1))

    def check(out, spec, n_bed):
        rows = _summary_rows(out + "/summary.tsv")
        names = spec.names()
        order = [r[2] for r in rows]
        assert [x for i, x in enumerate(order) if i == 0 or order[i - 1] != x] == ["ALL"] + sorted(beds)[:n_bed] + names  # (the sets' labels come sorted by name)
        bits = [cl.bits_of_span(contigs, spec, int(batch.contig_idx[r]), spans[r]) for r in range(batch.n_regions)]
        want = {(kind, j): np.zeros(6, np.int64) for kind in ("GT", "BASEPAIR") for j in range(spec.n_labels)}
        for t in table:  # region_id, coordinates, comparison, truth_total, truth_tp, truth_fn, query_total, query_tp, query_fp, 3 ratios, truth_fn_gt, query_fp_gt
            cells = np.array([int(t[4]), int(t[5]), int(t[7]), int(t[8]), int(t[12] or 0), int(t[13] or 0)], np.int64)
            for j in range(spec.n_labels):
                if (bits[ids[int(t[0])]] >> j) & 1:
                    want[(t[2], j)] += cells
        seen = 0
        for r in rows:
            if r[2] in names and r[4] == "ALL":
                got = np.array([int(r[6]), int(r[7]), int(r[9]), int(r[10]), int(r[14] or 0), int(r[15] or 0)], np.int64)
                assert np.array_equal(got, want[(r[1], names.index(r[2]))]), r
                seen += int(got.sum() > 0)
        assert seen >= 4
        return bits

    both, r = run("both", "-s", strat_tsv, "--context-strata", "gc,hp", "--batch-regions", "900", "-v")
    assert "Context labels: 16 (12 GC bins with pad 50, 4 homopolymer classes with pad 5)" in r.stderr
    assert open(both + "/summary.tsv").read().startswith(plain_text)  # the ALL block and the sets' blocks, then the derived blocks
    check(both, cl.DEFAULT, 3)
    alone, _ = run("alone", "--context-strata", "gc,hp", "--devices", "0,0", "--batch-regions", "700")
    assert open(alone + "/summary.tsv").read().startswith(open(nolabels + "/summary.tsv").read())
    check(alone, cl.DEFAULT, 0)
    spec = cl.Spec((0, 35, 45, 101), (2, 3, 5), 10, 0)
    other, _ = run("other", "--context-strata", "hp,gc", "--context-gc-edges", "0,35,45,101", "--context-gc-pad", "10", "--context-hp-edges", "2,3,5", "--context-hp-pad", "0")
    check(other, spec, 0)
    only, _ = run("only", "--context-strata", "hp", "-s", strat_tsv)
    check(only, cl.Spec((), cl.DEFAULT.hp_edges, 0, 5), 3)
    for name in ("truth.vcf.gz", "query.vcf.gz"):  # the labels change nothing else
        strip = lambda o: [l for l in gzip.open(o + "/" + name, "rt").read().splitlines() if not l.startswith("##aardvark_command")]
        assert strip(both) == strip(plain) == strip(alone)
    for extra, text in TOOL_REFUSALS:
        out, r = run("refused", *extra, ok=False)
        assert r.returncode == 64 and text in r.stderr and not os.path.exists(out + "/summary.tsv"), (extra, r.stderr)
