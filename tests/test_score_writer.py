"""summary_roc.tsv (avf_write_summary_roc / feeder.write_summary_roc) from a hand-made block, without a GPU: byte for byte the expected file, the rows of a point
at which a metric's denominator is 0 written as summary.tsv writes such a metric, and row for row what write_summary_named writes for the zero-padded tally of
each (scope, point)."""
import numpy as np
import pytest

from aardvark_amd import feeder
from aardvark_amd._abi import FIELDS, N_FIELDS, N_GROUPS, TALLY_LEN, VARIANT_TYPES

POINTS = ["score_all", "score_ge_10", "score_ge_30.5"]
F = {name: FIELDS.index(name) for name in FIELDS[:14]}
SNV = 1 + list(VARIANT_TYPES).index("Snv")


def hand_block():
    """one scope, three points, SNVs only: at point 1 a few calls are filtered; at point 2 no query call is left (precision has denominator 0)"""
    b = np.zeros((1, 3, N_GROUPS, 14), np.uint64)
    for k, (ttp, tfn, fngt, qtp, qfp) in enumerate([(8, 2, 1, 8, 2), (6, 4, 1, 6, 1), (0, 10, 0, 0, 0)]):
        for g in (0, SNV):
            b[0, k, g, F["GT_TRUTH_TP"]], b[0, k, g, F["GT_TRUTH_FN"]], b[0, k, g, F["GT_TRUTH_FN_GT"]] = ttp, tfn, fngt
            b[0, k, g, F["GT_QUERY_TP"]], b[0, k, g, F["GT_QUERY_FP"]] = qtp, qfp
    return b


HEAD = "compare_label\tcomparison\tregion_label\tfilter\tvariant_type\ttruth_total\ttruth_tp\ttruth_fn\tquery_total\tquery_tp\tquery_fp\tmetric_recall\tmetric_precision\tmetric_f1\ttruth_fn_gt\tquery_fp_gt\n"
# the whole file for hand_block(): recall 8/10, 6/10, 0/10; precision 8/10, 6/7, undefined (no query call left: an empty cell, with F1, as in summary.tsv);
# F1 = 2rp / (r + p) in doubles, printed with the shortest digits that round-trip, as summary.tsv prints its metrics
WANT = HEAD + "".join("job\tGT\tALL\t%s\t%s\t%s\n" % (point, vtype, cells) for point, cells in (
    ("score_all", "10\t8\t2\t10\t8\t2\t0.8\t0.8\t0.8000000000000002\t1\t0"),
    ("score_ge_10", "10\t6\t4\t7\t6\t1\t0.6\t0.8571428571428571\t0.7058823529411764\t1\t0"),
    ("score_ge_30.5", "10\t0\t10\t0\t0\t0\t0.0\t\t\t0\t0")) for vtype in ("ALL", "Snv"))
assert repr(2 * 0.8 * 0.8 / (0.8 + 0.8)) == "0.8000000000000002" and repr(6 / 7) == "0.8571428571428571" and repr(2 * 0.6 * (6 / 7) / (0.6 + 6 / 7)) == "0.7058823529411764"


def named_rows(tmp_path, block14, name):
    """the rows write_summary_named writes for the zero-padded tally of one (scope, point), `filter` replaced by the point's name"""
    tally = np.zeros(TALLY_LEN, np.uint64)
    tally[:N_GROUPS * N_FIELDS].reshape(N_GROUPS, N_FIELDS)[:, :14] = block14
    ref = str(tmp_path / "ref.tsv")
    feeder.write_summary_named(ref, tally, [], np.zeros(1, np.uint64), "job", feeder.METRIC_GT)
    lines = open(ref).read().split("\n")
    assert lines[0] + "\n" == HEAD and lines[-1] == ""
    cells = [l.split("\t") for l in lines[1:-1]]
    assert all(c[3] == "ALL" for c in cells)
    return ["\t".join(c[:3] + [name] + c[4:]) for c in cells]


def test_byte_for_byte(tmp_path):
    """the whole file against a literal, and every point's rows against summary.tsv's rows for that point's tally"""
    path = str(tmp_path / "summary_roc.tsv")
    feeder.write_summary_roc(path, POINTS, [], hand_block(), "job", feeder.METRIC_GT | feeder.METRIC_BASEPAIR)
    text = open(path).read()
    assert text == WANT
    rows = text.split("\n")[1:-1]
    at = 0
    for k, name in enumerate(POINTS):
        want = named_rows(tmp_path, hand_block()[0, k], name)
        assert rows[at:at + len(want)] == want and len(want) == 2, name
        at += len(want)
    assert at == len(rows)


def test_zero_denominator_rows_are_summary_tsv_s(tmp_path):
    """point 2: no query call left — precision and F1 as summary.tsv writes them for such a tally; a point with no truth call either"""
    b = hand_block()
    b = np.concatenate([b, np.zeros((1, 1, N_GROUPS, 14), np.uint64)], axis=1)
    path = str(tmp_path / "summary_roc.tsv")
    feeder.write_summary_roc(path, POINTS + ["score_ge_99"], [], b, "job", feeder.METRIC_GT)
    rows = [l.split("\t") for l in open(path).read().split("\n")[1:-1]]
    for k, name in ((2, "score_ge_30.5"), (3, "score_ge_99")):
        tally = np.zeros(TALLY_LEN, np.uint64)
        tally[:N_GROUPS * N_FIELDS].reshape(N_GROUPS, N_FIELDS)[:, :14] = b[0, k]
        ref = str(tmp_path / "ref.tsv")
        feeder.write_summary_named(ref, tally, [], np.zeros(1, np.uint64), "job", feeder.METRIC_GT)
        want = [l.split("\t") for l in open(ref).read().split("\n")[1:-1]]
        got = [r for r in rows if r[3] == name]
        assert got == [w[:3] + [name] + w[4:] for w in want] and got
    head = open(path).read().split("\n")[0].split("\t")
    last = [r for r in rows if r[3] == "score_ge_30.5"][0]
    assert last[head.index("query_total")] == "0" and last[head.index("metric_recall")] == repr(0.0) and last[head.index("metric_precision")] == last[head.index("metric_f1")]
    assert last[head.index("metric_precision")] not in ("0.0", "0")  # (undefined, not zero: whatever summary.tsv writes for an undefined metric)


def test_scopes_and_hap_rows(tmp_path):
    rng = np.random.default_rng(1)
    b = np.zeros((3, 3, N_GROUPS, 14), np.uint64)
    b[:, :, [2, 3]] = rng.integers(0, 500, (3, 3, 2, 14))
    b[:, :, 0] = b[:, :, 1:].sum(axis=2)
    path = str(tmp_path / "summary_roc.tsv")
    feeder.write_summary_roc(path, POINTS, ["easy", "ha,rd"], b, "job", 31)
    rows = [l.split("\t") for l in open(path).read().split("\n")[1:-1]]
    assert {r[1] for r in rows} == {"GT", "HAP", "WEIGHTED_HAP"} and {r[2] for r in rows} == {"ALL", "easy", "ha,rd"} and {r[3] for r in rows} == set(POINTS)
    with pytest.raises(ValueError):
        feeder.write_summary_roc(path, POINTS[:2], ["easy", "ha,rd"], b)
    with pytest.raises(feeder.FeederError):
        feeder.write_summary_roc(str(tmp_path / "no" / "dir.tsv"), POINTS, ["easy", "ha,rd"], b)
