"""summary_ci.tsv (avf_write_summary_ci / feeder.write_summary_ci) on hand-made blocks, without a GPU, against a Python restatement of the interval rule: the
percentile interval over the m replicates in which a metric is defined, sorted ascending, lo = x[floor(a/2 m)], hi = x[ceil((1 - a/2) m) - 1] with a = 1 - level/100
(exact fractions here), indices clamped, empty cells when m = 0; the column `replicates` is the m of F1.  Values are compared as doubles: the file's shortest
round-trip text parses back to the very double the restatement computes."""
import math
from fractions import Fraction

import numpy as np
import pytest

from aardvark_amd import feeder
from aardvark_amd._abi import N_FIELDS, TALLY_LEN

BASE = {"GT": 0, "HAP": 6, "WEIGHTED_HAP": 10, "BASEPAIR": 14, "RECORD_BP": 18}
TYPES = ["Snv", "Insertion", "Deletion", "Indel", "SvInsertion", "SvDeletion", "SvDuplication", "SvInversion", "SvBreakend", "TrContraction", "TrExpansion", "Unknown"]
JOINTS = {"JointIndel": ["Insertion", "Deletion", "Indel"], "JointStructuralVariant": ["SvInsertion", "SvDeletion", "SvDuplication", "SvInversion", "SvBreakend"],
          "JointTandemRepeat": ["TrExpansion", "TrContraction"]}
KEYS = ["compare_label", "comparison", "region_label", "filter", "variant_type"]
ALL_METRICS = 31
B = 40


def groups_of(vtype):
    if vtype == "ALL":
        return [0]
    return [1 + TYPES.index(t) for t in JOINTS.get(vtype, [vtype])]


def ratios(block, kind, vtype):
    """(recall, precision, f1) of a block's row, None where undefined — sums in Python integers, ratios in doubles like the writer"""
    m = [sum(int(block[g * N_FIELDS + BASE[kind] + k]) for g in groups_of(vtype)) for k in range(4)]
    ttot, qtot = m[0] + m[1], m[2] + m[3]
    r = m[0] / ttot if ttot else None
    p = m[2] / qtot if qtot else None
    return r, p, (2.0 * r * p / (r + p) if ttot and qtot and r + p > 0 else None)  # (recall = precision = 0: F1 is 0 / 0, not defined)


def interval(xs, level):
    xs = sorted(xs)
    m = len(xs)
    if not m:
        return None, None, 0
    half = (1 - Fraction(level, 100)) / 2
    lo, hi = math.floor(half * m), math.ceil((1 - half) * m) - 1
    clamp = lambda i: min(max(i, 0), m - 1)
    return xs[clamp(lo)], xs[clamp(hi)], m


def make_blocks(seed, n_labels):
    """a tally and label blocks with SNVs, three indel types (a joint row) and one tandem-repeat type; B replicates around them, some with an empty Deletion group
    (smaller m), label 1 with no deletions at all in any replicate but some in the point block (m = 0 beside a row that exists)"""
    rng = np.random.default_rng(seed)
    point = np.zeros((1 + n_labels, TALLY_LEN), np.uint64)
    reps = np.zeros((1 + n_labels, B, TALLY_LEN), np.uint64)
    for s in range(1 + n_labels):
        for t, scale in (("Snv", 4000), ("Insertion", 300), ("Deletion", 3), ("Indel", 40), ("TrExpansion", 25)):
            g = 1 + TYPES.index(t)
            for base in BASE.values():
                vals = rng.integers(scale // 3 + 1, scale + 2, 4)
                point[s, g * N_FIELDS + base:g * N_FIELDS + base + 4] = vals
                reps[s, :, g * N_FIELDS + base:g * N_FIELDS + base + 4] = rng.poisson(vals, (B, 4))
        g = 1 + TYPES.index("Deletion")
        reps[s, 5:5 + 3 * (s + 1), g * N_FIELDS:(g + 1) * N_FIELDS] = 0  # Deletion undefined in some replicates
        if s == 2:
            reps[s, :, g * N_FIELDS:(g + 1) * N_FIELDS] = 0
        for blk in [point[s]] + list(reps[s]):  # the joint group (0) holds everything
            blk[:N_FIELDS] = blk[N_FIELDS:13 * N_FIELDS].reshape(12, N_FIELDS).sum(axis=0)
    return point, reps


def read(path):
    rows = [l.split("\t") for l in open(path).read().split("\n")[:-1]]
    return rows[0], rows[1:]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("ci")
    names = ["easy", "hard"]
    point, reps = make_blocks(1, 2)
    out = {}
    feeder.write_summary_named(str(d / "summary.tsv"), point[0], names, point[1:], "job", ALL_METRICS)
    out["summary"] = read(str(d / "summary.tsv"))
    for level in (90, 95, 99):
        feeder.write_summary_ci(str(d / ("ci%d.tsv" % level)), point[0], names, point[1:], reps, level, "job", ALL_METRICS)
        out[level] = read(str(d / ("ci%d.tsv" % level)))
    out.update(point=point, reps=reps, names=names, dir=d)
    return out


def test_header_keys_and_row_order_equal_summary_tsv(files):
    sh, srows = files["summary"]
    ch, crows = files[95]
    assert ch == KEYS + ["metric_recall", "recall_lo", "recall_hi", "metric_precision", "precision_lo", "precision_hi", "metric_f1", "f1_lo", "f1_hi", "replicates"]
    assert sh[:5] == KEYS and [r[:5] for r in crows] == [r[:5] for r in srows] and len(crows) > 60
    i = {h: k for k, h in enumerate(sh)}
    for s, c in zip(srows, crows):  # the point values, formatted as summary.tsv formats them
        assert (c[5], c[8], c[11]) == (s[i["metric_recall"]], s[i["metric_precision"]], s[i["metric_f1"]])
    assert any(r[4] == "JointIndel" for r in crows) and any(r[2] == "hard" for r in crows) and not any(r[4] == "SvInsertion" for r in crows)


@pytest.mark.parametrize("level", [90, 95, 99])
def test_intervals_equal_the_restatement(files, level):
    _, rows = files[level]
    scope = {"ALL": 0, "easy": 1, "hard": 2}
    smaller, empty = 0, 0
    for r in rows:
        s = scope[r[2]]
        per_rep = [ratios(files["reps"][s, b], r[1], r[4]) for b in range(B)]
        for q in range(3):
            lo, hi, m = interval([x[q] for x in per_rep if x[q] is not None], level)
            got_lo, got_hi = r[6 + 3 * q], r[7 + 3 * q]
            if m == 0:
                assert (got_lo, got_hi) == ("", "")
            else:
                assert (float(got_lo), float(got_hi)) == (lo, hi), (r[:5], q)
                assert lo <= hi
            if q == 2:
                assert int(r[14]) == m
                smaller += 0 < m < B
                empty += m == 0
    assert smaller >= 5 and empty >= 5  # rows whose denominator is 0 in some replicates report the smaller m; label `hard` has Deletion rows without any


def test_level_90_is_nested_in_level_99(files):
    strictly = 0
    for a, b in zip(files[90][1], files[99][1]):
        assert a[:5] == b[:5] and a[14] == b[14]
        for q in range(3):
            if a[6 + 3 * q]:
                lo90, hi90, lo99, hi99 = (float(x) for x in (a[6 + 3 * q], a[7 + 3 * q], b[6 + 3 * q], b[7 + 3 * q]))
                assert lo99 <= lo90 <= hi90 <= hi99
                strictly += lo99 < lo90 or hi90 < hi99
    assert strictly > 50


def test_replicates_equal_to_the_tally_give_lo_hi_point(files, tmp_path):
    point, names = files["point"], files["names"]
    reps = np.repeat(point[:, None, :], 7, axis=1)
    feeder.write_summary_ci(str(tmp_path / "same.tsv"), point[0], names, point[1:], reps, 95, "job", ALL_METRICS)
    _, rows = read(str(tmp_path / "same.tsv"))
    assert len(rows) == len(files[95][1])
    for r in rows:
        for q in range(3):
            assert r[5 + 3 * q] == r[6 + 3 * q] == r[7 + 3 * q] != ""
        assert r[14] == "7"


def test_no_labels_one_replicate_and_refusals(files, tmp_path):
    point, reps = files["point"], files["reps"]
    feeder.write_summary_ci(str(tmp_path / "one.tsv"), point[0], [], None, reps[:1, :1], 99)
    _, rows = read(str(tmp_path / "one.tsv"))
    assert rows and all(r[2] == "ALL" and r[14] in ("0", "1") for r in rows) and all(r[6] == r[7] for r in rows)
    with pytest.raises(feeder.FeederError, match="90, 95 or 99"):
        feeder.write_summary_ci(str(tmp_path / "bad.tsv"), point[0], [], None, reps[:1], 80)
    with pytest.raises(ValueError):
        feeder.write_summary_ci(str(tmp_path / "bad.tsv"), point[0], ["a"], point[1:2], reps[:1], 95)
