"""aardvark_amd_compare --bootstrap-per-call: what the tool refuses, by name and with exit code 64, before it reads a VCF or makes a context, and what --help says (no
GPU needed); then, on a GPU, the runs on tests/escapes_lib.write_feeder_case: the three _ci files are present, every other output is byte-identical to the run
without the option, the files equal the writers fed with the restatement's replicates (tests/callboot_lib.py) on the ORACLE's results of the same feed, and the wide
feed's, --devices' and small batches' files equal the packed feed's."""
import os
import subprocess

import numpy as np
import pytest

import callboot_lib as cbl
import escapes_lib as el
import kind_lib
import size_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "aardvark_amd", "bin", "aardvark_amd_compare")
B, SEED = 23, 7
OPT = "--bootstrap-per-call"
REFUSALS = [([OPT, "--size-strata"], "--bootstrap-per-call needs --bootstrap B"),
            ([OPT, "--bootstrap", "10"], "--bootstrap-per-call needs --size-strata or --kind-strata"),
            ([OPT, "--bootstrap", "10", "--kind-strata", "--output-debug", "/nonexistent/dbg"], "--bootstrap-per-call cannot be combined with --output-debug"),
            ([OPT, "--bootstrap", "10", "--size-strata", "-s", "none.tsv", "--strat-lists", "host"],
             "--bootstrap-per-call on the packed feed reads the labels from the sets on the GPU: it cannot be combined with --strat-lists host"),
            # over the cap with the context labels alone: 4096 replicates x 17 scopes x 9 kinds = 626,688 blocks
            ([OPT, "--bootstrap", "4096", "--kind-strata", "--context-strata", "gc,hp"], "--bootstrap-per-call: replicates x (1 + region labels) x keys")]
NEW = ("summary_size_ci.tsv", "summary_kind_ci.tsv", "kind_ratios_ci.tsv")


def test_tool_refusals_need_no_device(tmp_path):
    for extra, text in REFUSALS:
        r = subprocess.run([CLI, "-r", "none.fa", "-t", "none.vcf", "-q", "none.vcf", "-o", str(tmp_path / "out")] + extra, capture_output=True, text=True)
        assert r.returncode == 64 and text in r.stderr, (extra, r.returncode, r.stderr)
    assert not any(os.path.exists(str(tmp_path / "out" / f)) for f in NEW)


def test_usage_names_the_option():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and all(o in r.stderr for o in (OPT,) + NEW)


# ---- the runs ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case(tmp_path_factory, oracle):
    """the feeder's case, its feed solved by the ORACLE; the restatement's point blocks and replicates, with and without the two BED labels"""
    from aardvark_amd import feeder
    import oracle_lib
    d = tmp_path_factory.mktemp("callboot_tool")
    p = el.write_feeder_case(d)
    open(os.path.join(str(d), "front.bed"), "w").write("chrE\t0\t50000\n")
    open(os.path.join(str(d), "none.bed"), "w").write("chrE\t140000\t140010\n")
    open(os.path.join(str(d), "strat.tsv"), "w").write("front\tfront.bed\nnone\tnone.bed\n")
    p["dir"], p["strat"] = d, os.path.join(str(d), "strat.tsv")
    genome = feeder.Genome(p["fa"])
    feed = feeder.feed_compare(p["t"], p["q"], p["bed"], genome, min_variant_gap=el.GAP)
    batch = feed.batch
    res = oracle_lib.compare_batch(oracle, batch, genome.contigs(), threads=8)
    assert (np.asarray(res.status) == 0).all()
    calls = kind_lib.calls_of(batch, res)
    strat = feeder.Stratifications(p["strat"])
    off, idx = strat.batch_labels(genome, batch)
    members = list(size_lib.members_of_lists(off, idx, 2, batch.n_regions))
    strat.close()
    genome.close()
    n, keys = batch.n_regions, (np.asarray(batch.contig_idx, np.uint64), np.asarray(batch.start, np.uint64))
    size = cbl.size(size_lib.DEFAULT)
    for tag, m in (("plain", None), ("label", members)):
        p[tag] = dict(kind=kind_lib.expected(calls, n, m), size=size_lib.expected(calls, size_lib.DEFAULT, n, m),
                      kind_reps=cbl.expected(calls, n, m, B, SEED, cbl.KIND, keys=keys), size_reps=cbl.expected(calls, n, m, B, SEED, size, keys=keys))
    return p


def want_files(case, tag, names, label, level=95):
    from aardvark_amd import feeder
    d = os.path.join(str(case["dir"]), "want_%s_%d" % (tag, level))
    os.makedirs(d, exist_ok=True)
    w, mask = case[tag], feeder.METRIC_GT | feeder.METRIC_HAP | feeder.METRIC_WEIGHTED_HAP
    feeder.write_summary_size_ci(os.path.join(d, NEW[0]), size_lib.names_of(size_lib.DEFAULT), names, w["size"], w["size_reps"], level, label, mask)
    feeder.write_summary_kind_ci(os.path.join(d, NEW[1]), names, w["kind"], w["kind_reps"], level, label, mask)
    feeder.write_kind_ratios_ci(os.path.join(d, NEW[2]), names, w["kind"], w["kind_reps"], level, label)
    return {f: open(os.path.join(d, f)).read() for f in NEW}


def run(case, name, *extra):
    """-> ({file name: text} of the output folder, stderr)"""
    out = os.path.join(str(case["dir"]), name)
    r = subprocess.run([CLI, "-r", case["fa"], "-t", case["t"], "-q", case["q"], "-b", case["bed"], "--min-variant-gap", str(el.GAP), "-o", out, "-v",
                        "--enable-haplotype-metrics", "--enable-weighted-haplotype-metrics"] + list(extra), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out)) if os.path.isfile(os.path.join(out, f))}, r.stderr


def same_outputs(got, without):
    """every file of the run without the option is there and byte-identical — but for the annotated VCFs, whose header records the run's own command line and
    output folder (##aardvark_command): those are compared decompressed, byte for byte, without that one line, and their .tbi, which indexes the compressed
    offsets behind that header, by presence"""
    import gzip
    bad = []
    for f, data in without.items():
        if f.endswith(".vcf.gz"):
            strip = lambda raw: [l for l in gzip.decompress(raw).split(b"\n") if not l.startswith(b"##aardvark_command")]
            a, b = strip(got[f]), strip(data)
            if a != b or len(a) + 1 != len(gzip.decompress(data).split(b"\n")):
                bad.append(f)
        elif f.endswith(".tbi"):
            if f not in got:
                bad.append(f)
        elif got.get(f) != data:
            bad.append(f)
    return bad


BOTH = ("--bootstrap", str(B), "--bootstrap-seed", str(SEED), "--size-strata", "--kind-strata")


@pytest.mark.gpu
def test_plain_job(case):
    """the new files are present and are the writers' on the restatement's replicates; every other output is byte-identical to the run without the option; the wide
    feed, two contexts and small batches give the same files"""
    without, _ = run(case, "without", *BOTH)
    assert not any(f in without for f in NEW)
    got, err = run(case, "with", *BOTH, OPT)
    assert set(got) == set(without) | set(NEW)
    assert same_outputs(got, without) == []
    assert "avk_size_boot_tallies / avk_kind_boot_tallies" in err
    label = got["summary.tsv"].decode().split("\n")[1].split("\t")[0]
    want = want_files(case, "plain", [], label)
    for f in NEW:
        assert got[f].decode() == want[f], f
    assert got[NEW[0]].count(b"\n") == without["summary_size.tsv"].count(b"\n") and got[NEW[2]].count(b"\n") == without["kind_ratios.tsv"].count(b"\n")
    for name, extra in (("wide", ("--batch-form", "wide")), ("two", ("--devices", "0,0")), ("batches", ("--batch-regions", "100"))):
        g2, err2 = run(case, name, *BOTH, OPT, *extra)
        assert all(g2[f] == got[f] for f in got if f.endswith(".tsv")), (name, [f for f in got if f.endswith(".tsv") and g2[f] != got[f]])
        assert ("avk_size_boot_tallies_host / avk_kind_boot_tallies_host" in err2) == (name == "wide")


@pytest.mark.gpu
def test_with_labels_a_level_and_one_family(case):
    """-s with two BED labels at level 90; the wide feed with labels and two contexts equal the packed feed; one family alone writes its files only"""
    without, _ = run(case, "lwithout", "-s", case["strat"], *BOTH, "--bootstrap-level", "90")
    got, _ = run(case, "lwith", "-s", case["strat"], *BOTH, "--bootstrap-level", "90", OPT)
    assert set(got) == set(without) | set(NEW) and same_outputs(got, without) == []
    label = got["summary.tsv"].decode().split("\n")[1].split("\t")[0]
    want = want_files(case, "label", ["front", "none"], label, level=90)
    for f in NEW:
        assert got[f].decode() == want[f], f
    for name, extra in (("lwide", ("--batch-form", "wide")), ("ltwo", ("--devices", "0,0", "--batch-regions", "100"))):
        g2, _ = run(case, name, "-s", case["strat"], *BOTH, "--bootstrap-level", "90", OPT, *extra)
        assert all(g2[f] == got[f] for f in got if f.endswith(".tsv")), name
    only, _ = run(case, "lsize", "-s", case["strat"], "--bootstrap", str(B), "--bootstrap-seed", str(SEED), "--bootstrap-level", "90", "--size-strata", "--roc", "QUAL", OPT)
    assert NEW[0] in only and NEW[1] not in only and NEW[2] not in only and only[NEW[0]] == got[NEW[0]] and "summary_roc.tsv" in only
