"""summary_size_ci.tsv, summary_kind_ci.tsv and kind_ratios_ci.tsv (avf_write_summary_size_ci, avf_write_summary_kind_ci, avf_write_kind_ratios_ci) on hand-made
blocks, without a GPU, against a Python restatement: the key columns, row order and point values are those of summary_size.tsv / summary_kind.tsv / kind_ratios.tsv
for the same tallies; an interval is the percentile interval of tests/test_boot_writer.py's restatement (exact fractions) over the replicates in which the metric or
the ratio is defined; `replicates` is F1's count, or the smaller of the two ratios' counts.  Values are compared as doubles: the file's shortest round-trip text parses
back to the very double the restatement computes."""
import numpy as np
import pytest

from aardvark_amd import feeder
from aardvark_amd._abi import KIND_NAMES, N_GROUPS
from test_boot_writer import BASE, TYPES, groups_of, interval

B = 40
BINS = ["len_0", "len_1_5", "len_ge6"]
NAMES = ["easy", "hard"]
KINDS3 = ["GT", "HAP", "WEIGHTED_HAP"]


def make_blocks(seed, n_scopes, n_keys):
    """point blocks [scopes, keys, 13, 14] with SNVs, three indel types (a joint row) and one tandem-repeat type; B replicates around them.  Key 1 has no Deletion
    calls in some replicates (a smaller m) and, in the last scope, in none (m = 0 beside a row that exists); key 2 of scope 0 is empty (only its ALL rows exist)"""
    rng = np.random.default_rng(seed)
    point = np.zeros((n_scopes, n_keys, N_GROUPS, 14), np.uint64)
    reps = np.zeros((n_scopes, B, n_keys, N_GROUPS, 14), np.uint64)
    for s in range(n_scopes):
        for k in range(n_keys):
            if s == 0 and k == 2:
                continue
            for t, scale in (("Snv", 4000), ("Insertion", 300), ("Deletion", 3), ("Indel", 40), ("TrExpansion", 25)):
                g = 1 + TYPES.index(t)
                vals = rng.integers(scale // 3 + 1, scale + 2, 14)
                point[s, k, g] = vals
                reps[s, :, k, g] = rng.poisson(vals, (B, 14))
            g = 1 + TYPES.index("Deletion")
            if k == 1:
                reps[s, 5:5 + 3 * (s + 1), k, g] = 0
                if s == n_scopes - 1:
                    reps[s, :, k, g] = 0
            point[s, k, 0] = point[s, k, 1:].sum(axis=0)
            reps[s, :, k, 0] = reps[s, :, k, 1:].sum(axis=1)
    return point, reps


def read(path):
    rows = [l.split("\t") for l in open(path).read().split("\n")[:-1]]
    return rows[0], rows[1:]


def ratios14(block, kind, vtype):
    """test_boot_writer.ratios for a keyed block [13, 14]"""
    m = [sum(int(block[g, BASE[kind] + k]) for g in groups_of(vtype)) for k in range(4)]
    ttot, qtot = m[0] + m[1], m[2] + m[3]
    r = m[0] / ttot if ttot else None
    p = m[2] / qtot if qtot else None
    return r, p, (2.0 * r * p / (r + p) if ttot and qtot and r + p > 0 else None)


def cell(x):
    return None if x == "" else float(x)


@pytest.mark.parametrize("level", [90, 95, 99])
@pytest.mark.parametrize("family", ["size", "kind"])
def test_summary_ci_files(tmp_path, family, level):
    keys = BINS if family == "size" else KIND_NAMES
    point, reps = make_blocks(3, 1 + len(NAMES), len(keys))
    plain, ci = str(tmp_path / "plain.tsv"), str(tmp_path / "ci.tsv")
    if family == "size":
        feeder.write_summary_size(plain, BINS, NAMES, point, metrics=31)
        feeder.write_summary_size_ci(ci, BINS, NAMES, point, reps, level=level, metrics=31)
    else:
        feeder.write_summary_kind(plain, NAMES, point, metrics=31)
        feeder.write_summary_kind_ci(ci, NAMES, point, reps, level=level, metrics=31)
    ph, prow = read(plain)
    ch, crow = read(ci)
    assert ch == ph[:5] + ["metric_recall", "recall_lo", "recall_hi", "metric_precision", "precision_lo", "precision_hi", "metric_f1", "f1_lo", "f1_hi", "replicates"]
    assert [r[:5] for r in crow] == [r[:5] for r in prow], "the rows, their order and their key columns are the plain file's"
    assert [(r[5], r[8], r[11]) for r in crow] == [(r[11], r[12], r[13]) for r in prow], "the point values are the plain file's, text for text"
    assert {r[1] for r in crow} == set(KINDS3), "BASEPAIR and RECORD_BP bits are ignored"
    scopes = ["ALL"] + NAMES
    seen_small = seen_none = False
    for r in crow:
        s, k = scopes.index(r[2]), keys.index(r[3])
        per = [ratios14(reps[s, b, k], r[1], r[4]) for b in range(B)]
        for q in range(3):
            lo, hi, m = interval([x[q] for x in per if x[q] is not None], level)
            assert (cell(r[6 + 3 * q]), cell(r[7 + 3 * q])) == (lo, hi), r
            if q == 2:
                assert int(r[14]) == m
        seen_small |= 0 < int(r[14]) < B
        seen_none |= int(r[14]) == 0 and r[5] != ""
    assert seen_small and seen_none
    assert sum(1 for r in crow if r[2] == "ALL" and r[3] == keys[2]) == 3 and all(r[14] == "0" for r in crow if r[2] == "ALL" and r[3] == keys[2])


def ti_tv_het_hom(block, vtype, s):
    """the four counts of set s (truth_total .. query_fp) of a kind block [9, 13, 14]"""
    out = [0, 0, 0, 0]
    for k in range(9):
        m = [sum(int(block[k, g, q]) for g in groups_of(vtype)) for q in range(4)]
        x = [m[0] + m[1], m[0], m[1], m[2] + m[3], m[2], m[3]][s]
        gt, sub = divmod(k, 3)
        out[0] += x if sub == 0 else 0
        out[1] += x if sub == 1 else 0
        out[2] += x if gt == 0 else 0
        out[3] += x if gt == 1 else 0
    return out


@pytest.mark.parametrize("level", [90, 95, 99])
def test_kind_ratios_ci(tmp_path, level):
    point, reps = make_blocks(4, 1 + len(NAMES), 9)
    reps[1, 3:12, [1, 4, 7]] = 0   # no transversion in these replicates of scope 1: Ti/Tv undefined there, het/hom defined
    reps[2, 20:, 3:6] = 0          # no hom call in these replicates of scope 2
    plain, ci = str(tmp_path / "ratios.tsv"), str(tmp_path / "ratios_ci.tsv")
    feeder.write_kind_ratios(plain, NAMES, point)
    feeder.write_kind_ratios_ci(ci, NAMES, point, reps, level=level)
    ph, prow = read(plain)
    ch, crow = read(ci)
    assert ch == ph + ["titv_lo", "titv_hi", "hethom_lo", "hethom_hi", "replicates"]
    assert [r[:10] for r in crow] == prow, "kind_ratios.tsv's rows, text for text"
    sets = ["truth_total", "truth_tp", "truth_fn", "query_total", "query_tp", "query_fp"]
    scopes = ["ALL"] + NAMES
    counts = set()
    for r in crow:
        s, st = scopes.index(r[1]), sets.index(r[3])
        per = [ti_tv_het_hom(reps[s, b], r[2], st) for b in range(B)]
        a = interval([c[0] / c[1] for c in per if c[1]], level)
        h = interval([c[2] / c[3] for c in per if c[3]], level)
        assert (cell(r[10]), cell(r[11]), cell(r[12]), cell(r[13]), int(r[14])) == (a[0], a[1], h[0], h[1], min(a[2], h[2])), r
        counts.add((r[1], a[2], h[2]))
    assert ("easy", B - 9, B) in counts and ("hard", B, 20) in counts, "a ratio undefined in some replicates"


def test_percentile_indices_at_m_0_and_1(tmp_path):
    """one replicate: lo = hi = its value at every level; a metric defined in no replicate: empty cells and replicates 0"""
    point, reps = make_blocks(5, 1, 3)
    one = reps[:, :1].copy()
    for level in (90, 95, 99):
        ci = str(tmp_path / ("one%d.tsv" % level))
        feeder.write_summary_size_ci(ci, BINS, [], point, one, level=level)
        _, rows = read(ci)
        for r in rows:
            v = ratios14(one[0, 0, BINS.index(r[3])], r[1], r[4])
            for q in range(3):
                assert cell(r[6 + 3 * q]) == cell(r[7 + 3 * q]) == v[q]
            assert r[14] == ("0" if v[2] is None else "1")
    none = np.zeros_like(one)
    ci = str(tmp_path / "none.tsv")
    feeder.write_summary_size_ci(ci, BINS, [], point, none, level=95)
    _, rows = read(ci)
    assert rows and all(r[6:8] + r[9:11] + r[12:] == ["", "", "", "", "", "", "0"] for r in rows)
    feeder.write_kind_ratios_ci(ci, [], make_blocks(5, 1, 9)[0], np.zeros((1, 1, 9, N_GROUPS, 14), np.uint64))
    _, rows = read(ci)
    assert rows and all(r[10:] == ["", "", "", "", "0"] for r in rows)


def test_refusals(tmp_path):
    point, reps = make_blocks(6, 1, 3)
    with pytest.raises(Exception, match="90, 95 or 99"):
        feeder.write_summary_size_ci(str(tmp_path / "x.tsv"), BINS, [], point, reps, level=80)
    with pytest.raises(ValueError):
        feeder.write_summary_size_ci(str(tmp_path / "x.tsv"), BINS, [], point, reps[:, :, :2])
    with pytest.raises(ValueError):
        feeder.write_kind_ratios_ci(str(tmp_path / "x.tsv"), [], make_blocks(6, 1, 9)[0], reps)
