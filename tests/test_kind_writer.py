"""summary_kind.tsv and kind_ratios.tsv (avf_write_summary_kind, avf_write_kind_ratios / feeder.write_summary_kind, feeder.write_kind_ratios) without a GPU: both
files from a hand-made block with known ratios, byte for byte; a zero denominator gives an empty cell; label rows in the handle's order; the summary_kind.tsv rows
of one kind equal summary.tsv's GT / HAP / WEIGHTED_HAP rows of a tally that holds only that kind."""
import numpy as np
import pytest

import kind_lib
from aardvark_amd import feeder
from aardvark_amd._abi import FIELDS, N_FIELDS, N_GROUPS, TALLY_LEN

F = {f: FIELDS.index(f) for f in FIELDS[:14]}
K = {n: k for k, n in enumerate(kind_lib.NAMES)}
SNV, INS, DEL = 1, 2, 3  # groups: 1 + type


def hand_block(n_labels=0):
    """SNVs: 30 het transitions (24 truth TP, 6 FN; 25 query TP, 5 FP), 10 het transversions, 20 hom transitions, 4 hom transversions (all TP on both sides);
    insertions: 8 het_other, 2 hom_other; the joint group is their sum.  Ti/Tv of truth_total: 50 / 14; het/hom of truth_total ALL: 48 / 26"""
    b = np.zeros((1 + n_labels, 9, N_GROUPS, 14), np.uint64)
    def put(kind, g, ttp, tfn, qtp, qfp):
        b[0, K[kind], g, [F["GT_TRUTH_TP"], F["GT_TRUTH_FN"], F["GT_QUERY_TP"], F["GT_QUERY_FP"]]] = [ttp, tfn, qtp, qfp]
        b[0, K[kind], g, [F["HAP_TRUTH_TP"], F["HAP_TRUTH_FN"], F["HAP_QUERY_TP"], F["HAP_QUERY_FP"]]] = [2 * ttp, 2 * tfn, 2 * qtp, 2 * qfp]
    put("het_ts", SNV, 24, 6, 25, 5)
    put("het_tv", SNV, 10, 0, 10, 0)
    put("hom_ts", SNV, 20, 0, 20, 0)
    put("hom_tv", SNV, 4, 0, 4, 0)
    put("het_other", INS, 8, 0, 8, 0)
    put("hom_other", INS, 2, 0, 2, 0)
    b[0, :, 0] = b[0, :, 1:].sum(axis=1)
    return b


RATIO_HEAD = "compare_label\tregion_label\tvariant_type\tset\tti\ttv\ttitv_ratio\thet\thom_alt\thet_hom_ratio\n"


def test_ratios_by_hand(tmp_path):
    path = str(tmp_path / "kind_ratios.tsv")
    feeder.write_kind_ratios(path, [], hand_block(), "job")
    text = open(path).read()
    assert text.startswith(RATIO_HEAD)
    rows = [l.split("\t") for l in text.split("\n")[1:-1]]
    assert [r[2] for r in rows[::6]] == ["ALL", "Snv", "Insertion", "JointIndel"] and len(rows) == 24
    assert [r[3] for r in rows[:6]] == ["truth_total", "truth_tp", "truth_fn", "query_total", "query_tp", "query_fp"]
    by = {(r[2], r[3]): r[4:] for r in rows}
    assert by[("ALL", "truth_total")][:2] == ["50", "14"] and by[("ALL", "truth_total")][3:5] == ["48", "26"]
    assert float(by[("ALL", "truth_total")][2]) == pytest.approx(50 / 14, abs=1e-6) and float(by[("ALL", "truth_total")][5]) == pytest.approx(48 / 26, abs=1e-6)
    assert by[("Snv", "truth_tp")][:2] == ["44", "14"] and by[("Snv", "truth_tp")][3:5] == ["34", "24"]
    assert by[("Snv", "query_fp")] == ["5", "0", "", "5", "0", ""], "a zero denominator gives an empty cell"
    assert by[("Snv", "truth_fn")] == ["6", "0", "", "6", "0", ""]
    assert by[("Insertion", "truth_total")][:3] == ["0", "0", ""] and by[("Insertion", "truth_total")][3:5] == ["8", "2"]
    assert float(by[("Insertion", "truth_total")][5]) == 4.0 and by[("JointIndel", "query_tp")] == by[("Insertion", "query_tp")]
    # the ratio cells are formatted as summary.tsv formats a metric: the same quotient there and here
    half = hand_block()
    half[0, K["het_tv"], SNV, F["GT_TRUTH_TP"]] = 60  # ti 50 / tv 60 + 4
    half[0, K["het_tv"], 0, F["GT_TRUTH_TP"]] = 60
    feeder.write_kind_ratios(path, [], half, "job")
    cell = [l.split("\t") for l in open(path).read().split("\n")[1:-1] if l.split("\t")[2:4] == ["Snv", "truth_total"]][0]
    tally = np.zeros(TALLY_LEN, np.uint64)
    tally[[F["GT_TRUTH_TP"], F["GT_TRUTH_FN"]]] = [50, 14]  # recall 50 / 64 = ti / tv of the block above
    spath = str(tmp_path / "summary.tsv")
    feeder.write_summary_named(spath, tally, [], np.zeros(1, np.uint64), "job", feeder.METRIC_GT)
    recall = open(spath).read().split("\n")[1].split("\t")[11]
    assert cell[4:7] == ["50", "64", recall] and recall == "0.78125"


def test_both_files_byte_for_byte(tmp_path):
    """one SNV kind only: every cell can be written down"""
    b = np.zeros((1, 9, N_GROUPS, 14), np.uint64)
    for g in (0, SNV):
        b[0, K["hom_ts"], g, [F["GT_TRUTH_TP"], F["GT_TRUTH_FN"], F["GT_QUERY_TP"], F["GT_QUERY_FP"], F["GT_TRUTH_FN_GT"]]] = [3, 1, 3, 0, 1]
    rp, kp = str(tmp_path / "kind_ratios.tsv"), str(tmp_path / "summary_kind.tsv")
    feeder.write_kind_ratios(rp, [], b, "job")
    feeder.write_summary_kind(kp, [], b, "job", feeder.METRIC_GT)
    counts = [("truth_total", 4), ("truth_tp", 3), ("truth_fn", 1), ("query_total", 3), ("query_tp", 3), ("query_fp", 0)]
    want = RATIO_HEAD + "".join("job\tALL\t%s\t%s\t%d\t0\t\t0\t%d\t0.0\n" % (vt, s, c, c) if c else "job\tALL\t%s\t%s\t0\t0\t\t0\t0\t\n" % (vt, s)
                                for vt in ("ALL", "Snv") for s, c in counts)
    assert open(rp).read() == want
    lines = open(kp).read().split("\n")[:-1]
    assert lines[0].split("\t")[:5] == ["compare_label", "comparison", "region_label", "filter", "variant_type"]
    body = [l.split("\t") for l in lines[1:]]
    assert [r[3] for r in body] == kind_lib.NAMES[:3] + ["hom_ts", "hom_ts"] + kind_lib.NAMES[4:]
    assert body[3][:11] == ["job", "GT", "ALL", "hom_ts", "ALL", "4", "3", "1", "3", "3", "0"] and body[4][4] == "Snv" and body[3][11:13] == ["0.75", "1.0"] and body[3][14:] == ["1", "0"]


def test_label_rows_are_in_the_handles_order(tmp_path):
    names = ["zeta", "alpha", "mid,dle"]
    b = hand_block(3)
    b[2] = b[0]
    b[3, K["hom_tv"]] = b[0, K["hom_tv"]]
    for name, write in (("r.tsv", lambda p: feeder.write_kind_ratios(p, names, b, "job")), ("k.tsv", lambda p: feeder.write_summary_kind(p, names, b, "job"))):
        path = str(tmp_path / name)
        write(path)
        rows = [l.split("\t") for l in open(path).read().split("\n")[1:-1]]
        col = 1 if name == "r.tsv" else 2
        seen = [r[col] for r in rows]
        assert [x for k, x in enumerate(seen) if k == 0 or seen[k - 1] != x] == ["ALL"] + names
    rows = [l.split("\t") for l in open(str(tmp_path / "r.tsv")).read().split("\n")[1:-1]]
    assert [r[2] for r in rows if r[1] == "zeta"] == ["ALL"] * 6 and [r[4:] for r in rows if r[1] == "zeta"] == [["0", "0", "", "0", "0", ""]] * 6
    assert [r[4:] for r in rows if r[1] == "alpha"] == [r[4:] for r in rows if r[1] == "ALL"]
    assert [r[4:] for r in rows if r[1] == "mid,dle" and r[2:4] == ["Snv", "truth_total"]] == [["0", "4", "0.0", "0", "4", "0.0"]]
    with pytest.raises(ValueError):
        feeder.write_kind_ratios(str(tmp_path / "bad.tsv"), ["a"], b)
    with pytest.raises(feeder.FeederError):
        feeder.write_summary_kind(str(tmp_path / "no" / "such" / "dir.tsv"), names, b)


@pytest.mark.parametrize("kind", ["het_ts", "hom_other"])
def test_rows_of_one_kind_equal_the_summary_of_its_tally(tmp_path, kind):
    b = hand_block()
    kp, sp = str(tmp_path / "summary_kind.tsv"), str(tmp_path / "summary.tsv")
    metrics = feeder.METRIC_GT | feeder.METRIC_HAP | feeder.METRIC_WEIGHTED_HAP
    feeder.write_summary_kind(kp, [], b, "job", metrics | feeder.METRIC_BASEPAIR)
    tally = np.zeros(TALLY_LEN, np.uint64)
    tally[:N_GROUPS * N_FIELDS].reshape(N_GROUPS, N_FIELDS)[:, :14] = b[0, K[kind]]
    feeder.write_summary_named(sp, tally, [], np.zeros(1, np.uint64), "job", metrics)
    got = [l.split("\t") for l in open(kp).read().split("\n")[1:-1]]
    want = [l.split("\t") for l in open(sp).read().split("\n")[1:-1]]
    assert [r[:3] + r[4:] for r in got if r[3] == kind] == [r[:3] + r[4:] for r in want] and len(want) >= 5
    assert {r[1] for r in got} == {"GT", "HAP", "WEIGHTED_HAP"}
