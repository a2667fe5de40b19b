"""aardvark_amd_compare --kind-strata: what the tool refuses, by name and with exit code 64, before it reads a file or makes a context, and what --help says (no GPU
needed); then, on a GPU, the runs on tests/escapes_lib.write_feeder_case: summary.tsv byte-identical with and without the option, and summary_kind.tsv and
kind_ratios.tsv equal to the writers fed with the block of the restatement (tests/kind_lib.py) on the ORACLE's results of the same feed — alone, with -s, with
--size-strata --roc QUAL, on the wide feed and with --devices 0,0."""
import os
import subprocess

import numpy as np
import pytest

import escapes_lib as el
import kind_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "aardvark_amd", "bin", "aardvark_amd_compare")
REFUSALS = [(["--kind-strata", "--output-debug", "/nonexistent/dbg"], "--kind-strata cannot be combined with --output-debug"),
            (["--kind-strata", "-s", "none.tsv", "--strat-lists", "host"], "--kind-strata on the packed feed reads the labels from the sets on the GPU: it cannot be combined with --strat-lists host")]


def test_tool_refusals_need_no_device(tmp_path):
    for extra, text in REFUSALS:
        r = subprocess.run([CLI, "-r", "none.fa", "-t", "none.vcf", "-q", "none.vcf", "-o", str(tmp_path / "out")] + extra, capture_output=True, text=True)
        assert r.returncode == 64 and text in r.stderr, (extra, r.returncode, r.stderr)
    assert not os.path.exists(str(tmp_path / "out" / "summary_kind.tsv"))


def test_usage_names_the_option():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and all(o in r.stderr for o in ("--kind-strata", "summary_kind.tsv", "kind_ratios.tsv"))


# ---- the runs ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case(tmp_path_factory, oracle):
    """the feeder's case, its feed solved by the ORACLE, the restatement's block with and without the two BED labels, written by the writers"""
    from aardvark_amd import feeder
    import oracle_lib
    import size_lib
    d = tmp_path_factory.mktemp("kind_tool")
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
    assert len(set(int(k) for k in calls[:, 11])) >= 3  # (het and hom SNVs, the two long alleles)
    strat = feeder.Stratifications(p["strat"])
    off, idx = strat.batch_labels(genome, batch)
    members = size_lib.members_of_lists(off, idx, 2, batch.n_regions)
    assert members[0].any() and not members[0].all() and not members[1].any()
    strat.close()
    genome.close()
    p["plain_block"], p["label_block"] = kind_lib.expected(calls, batch.n_regions), kind_lib.expected(calls, batch.n_regions, list(members))
    return p


def want_files(case, names, block, label):
    from aardvark_amd import feeder
    d = os.path.join(str(case["dir"]), "want_%d" % len(names))
    os.makedirs(d, exist_ok=True)
    feeder.write_summary_kind(os.path.join(d, "k.tsv"), names, block, label, feeder.METRIC_GT | feeder.METRIC_HAP | feeder.METRIC_WEIGHTED_HAP)
    feeder.write_kind_ratios(os.path.join(d, "r.tsv"), names, block, label)
    return open(os.path.join(d, "k.tsv")).read(), open(os.path.join(d, "r.tsv")).read()


def run(case, name, *extra):
    out = os.path.join(str(case["dir"]), name)
    r = subprocess.run([CLI, "-r", case["fa"], "-t", case["t"], "-q", case["q"], "-b", case["bed"], "--min-variant-gap", str(el.GAP), "-o", out, "-v",
                        "--enable-haplotype-metrics", "--enable-weighted-haplotype-metrics"] + list(extra), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    read = lambda f: open(os.path.join(out, f)).read() if os.path.exists(os.path.join(out, f)) else None
    return read("summary.tsv"), read("summary_kind.tsv"), read("kind_ratios.tsv"), r.stderr


@pytest.mark.gpu
def test_plain_job(case):
    plain, none, none2, _ = run(case, "plain")
    assert none is None and none2 is None
    summary, kinds, ratios, err = run(case, "kind", "--kind-strata")
    assert summary == plain and "avk_compare_packed_kind" in err
    label = summary.split("\n")[1].split("\t")[0]
    want_k, want_r = want_files(case, [], case["plain_block"], label)
    assert kinds == want_k and ratios == want_r
    rows = [l.split("\t") for l in ratios.split("\n")[1:-1]]
    snv = {r[3]: r for r in rows if r[2] == "Snv"}
    assert int(snv["truth_total"][4]) + int(snv["truth_total"][5]) == 330 and int(snv["truth_total"][7]) + int(snv["truth_total"][8]) == 330
    for name, extra in (("wide", ("--batch-form", "wide")), ("two", ("--devices", "0,0")), ("batches", ("--batch-regions", "100"))):
        s2, k2, r2, err2 = run(case, name, "--kind-strata", *extra)
        assert s2 == plain and k2 == kinds and r2 == ratios, name
        assert ("avk_kind_tallies_host" in err2) == (name == "wide")


@pytest.mark.gpu
def test_with_labels(case):
    plain, _, _, _ = run(case, "lplain", "-s", case["strat"])
    summary, kinds, ratios, err = run(case, "lkind", "-s", case["strat"], "--kind-strata")
    assert summary == plain and "avk_kind_tallies)" in err
    label = summary.split("\n")[1].split("\t")[0]
    want_k, want_r = want_files(case, ["front", "none"], case["label_block"], label)
    assert kinds == want_k and ratios == want_r
    s2, k2, r2, _ = run(case, "ltwo", "-s", case["strat"], "--kind-strata", "--devices", "0,0", "--batch-regions", "100")
    assert s2 == plain and k2 == kinds and r2 == ratios


@pytest.mark.gpu
def test_with_size_bins_and_the_curve(case):
    out = lambda name, f: open(os.path.join(str(case["dir"]), name, f)).read()
    plain, _, _, _ = run(case, "splain", "--size-strata", "--roc", "QUAL")
    summary, kinds, ratios, err = run(case, "skind", "--size-strata", "--roc", "QUAL", "--kind-strata")
    assert summary == plain and "avk_kind_tallies)" in err
    assert out("skind", "summary_size.tsv") == out("splain", "summary_size.tsv") and out("skind", "summary_roc.tsv") == out("splain", "summary_roc.tsv")
    label = summary.split("\n")[1].split("\t")[0]
    want_k, want_r = want_files(case, [], case["plain_block"], label)
    assert kinds == want_k and ratios == want_r
