"""aardvark_amd_compare --size-strata [--size-edges a,b,..]: what the tool refuses, by name and with exit code 64, before it reads a file or makes a context, and
what --help says (no GPU needed); then, on a GPU, the runs on tests/escapes_lib.write_feeder_case: summary.tsv byte-identical with and without the option,
summary_size.tsv identical across --batch-form values, batch sizes and --devices 0,0, and — the conservation law through the whole tool — its GT truth_total /
query_total per variant type, summed over the bins, equal to summary.tsv's; the same with -s (label sums from the resident batch) and with --bootstrap
(summary_ci.tsv unchanged)."""
import os
import subprocess

import pytest

import escapes_lib as el

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "aardvark_amd", "bin", "aardvark_amd_compare")
EDGES_TEXT = "1 to 15 strictly ascending sizes"
REFUSALS = [(["--size-strata", "--size-edges", "0,5"], EDGES_TEXT),
            (["--size-strata", "--size-edges", "3,3"], EDGES_TEXT),
            (["--size-strata", "--size-edges", "6,1"], EDGES_TEXT),
            (["--size-strata", "--size-edges", ",".join(str(k) for k in range(1, 17))], EDGES_TEXT),
            (["--size-strata", "--size-edges", "1,x"], "invalid value for --size-edges"),
            (["--size-edges", "1,6"], "--size-edges needs --size-strata"),
            (["--size-strata", "--output-debug", "/nonexistent/dbg"], "--size-strata cannot be combined with --output-debug"),
            (["--size-strata", "-s", "none.tsv", "--strat-lists", "host"], "cannot be combined with --strat-lists host")]


def test_tool_refusals_need_no_device(tmp_path):
    for extra, text in REFUSALS:
        r = subprocess.run([CLI, "-r", "none.fa", "-t", "none.vcf", "-q", "none.vcf", "-o", str(tmp_path / "out")] + extra, capture_output=True, text=True)
        assert r.returncode == 64 and text in r.stderr, (extra, r.returncode, r.stderr)
    assert not os.path.exists(str(tmp_path / "out" / "summary_size.tsv"))


def test_usage_names_the_options():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and all(o in r.stderr for o in ("--size-strata", "--size-edges", "summary_size.tsv"))
    assert "BASEPAIR and RECORD_BP rows are not part of this file" in r.stderr


# ---- the runs ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d = tmp_path_factory.mktemp("size_tool")
    p = el.write_feeder_case(d)
    open(os.path.join(str(d), "front.bed"), "w").write("chrE\t0\t50000\n")
    open(os.path.join(str(d), "none.bed"), "w").write("chrE\t140000\t140010\n")
    open(os.path.join(str(d), "strat.tsv"), "w").write("front\tfront.bed\nnone\tnone.bed\n")
    p["dir"], p["strat"] = d, os.path.join(str(d), "strat.tsv")
    return p


def run(case, name, *extra):
    out = os.path.join(str(case["dir"]), name)
    r = subprocess.run([CLI, "-r", case["fa"], "-t", case["t"], "-q", case["q"], "-b", case["bed"], "--min-variant-gap", str(el.GAP), "-o", out, "-v",
                        "--enable-haplotype-metrics", "--enable-weighted-haplotype-metrics"] + list(extra), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    read = lambda f: open(os.path.join(out, f)).read() if os.path.exists(os.path.join(out, f)) else None
    return read("summary.tsv"), read("summary_size.tsv"), read("summary_ci.tsv"), r.stderr


def rows(text):
    lines = [l.split("\t") for l in text.split("\n")[:-1]]
    return lines[0], lines[1:]


def check_law(summary, size, bins):
    """every (comparison, region_label, variant_type) row of summary.tsv that summary_size.tsv can have: its six counts are the sums over the bins"""
    head, srows = rows(summary)
    zhead, zrows = rows(size)
    assert zhead == head
    i = {h: k for k, h in enumerate(head)}
    counts = ["truth_total", "truth_tp", "truth_fn", "query_total", "query_tp", "query_fp"]
    sums, seen_bins = {}, set()
    for r in zrows:
        key = (r[i["comparison"]], r[i["region_label"]], r[i["variant_type"]])
        seen_bins.add(r[i["filter"]])
        acc = sums.setdefault(key, [0] * 6)
        for k, c in enumerate(counts):
            acc[k] += int(r[i[c]])
    assert seen_bins == set(bins) and {k[0] for k in sums} == {"GT", "HAP", "WEIGHTED_HAP"}
    n = 0
    for r in srows:
        if r[i["comparison"]] in ("BASEPAIR", "RECORD_BP"):
            continue
        key = (r[i["comparison"]], r[i["region_label"]], r[i["variant_type"]])
        assert r[i["filter"]] == "ALL" and sums[key] == [int(r[i[c]]) for c in counts], key
        n += 1
    assert n == len(sums)  # (no row of summary_size.tsv without its row in summary.tsv)
    return n


@pytest.mark.gpu
def test_plain_job(case):
    plain, none, _, _ = run(case, "plain")
    assert none is None
    summary, size, _, err = run(case, "size", "--size-strata")
    assert summary == plain and "avk_compare_packed_size" in err
    bins = ["len_0", "len_1_5", "len_6_15", "len_16_49", "len_ge50"]
    assert check_law(summary, size, bins) >= 9
    head, zrows = rows(size)
    gt = {(r[3], r[4]): int(r[5]) for r in zrows if r[1] == "GT" and r[2] == "ALL"}
    assert gt[("len_0", "Snv")] == 330 and gt[("len_ge50", "ALL")] == 2 and gt[("len_1_5", "ALL")] == 0 and ("len_ge50", "Snv") not in gt
    for name, extra in (("wide", ("--batch-form", "wide")), ("packed", ("--batch-form", "packed")), ("two", ("--devices", "0,0")), ("batches", ("--batch-regions", "100"))):
        s2, z2, _, err2 = run(case, name, "--size-strata", *extra)
        assert s2 == plain and z2 == size, name
        assert ("avk_size_tallies_host" in err2) == (name == "wide")


@pytest.mark.gpu
def test_other_edges_and_labels(case):
    plain, _, _, _ = run(case, "lplain", "-s", case["strat"])
    summary, size, _, err = run(case, "lsize", "-s", case["strat"], "--size-strata", "--size-edges", "300,301")
    assert summary == plain and "avk_size_tallies)" in err
    assert check_law(summary, size, ["len_0_299", "len_300", "len_ge301"]) >= 15
    head, zrows = rows(size)
    assert {r[2] for r in zrows} == {"ALL", "front", "none"}
    gt = {(r[2], r[3], r[4]): int(r[5]) for r in zrows if r[1] == "GT"}
    assert gt[("ALL", "len_300", "ALL")] == 1 and gt[("front", "len_ge301", "ALL")] == 1 and gt[("none", "len_0_299", "ALL")] == 0
    s2, z2, _, _ = run(case, "ltwo", "-s", case["strat"], "--size-strata", "--size-edges", "300,301", "--devices", "0,0", "--batch-regions", "100")
    assert s2 == plain and z2 == size


@pytest.mark.gpu
def test_with_bootstrap(case):
    plain, _, ci, _ = run(case, "bplain", "--bootstrap", "16")
    summary, size, ci2, err = run(case, "bsize", "--bootstrap", "16", "--size-strata")
    assert summary == plain and ci2 == ci and ci is not None and "avk_size_tallies)" in err
    _, alone, _, _ = run(case, "balone", "--size-strata")
    assert size == alone
    s3, z3, ci3, _ = run(case, "bwide", "--bootstrap", "16", "--size-strata", "--batch-form", "wide")
    assert s3 == plain and z3 == size and ci3 == ci
