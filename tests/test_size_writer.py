"""summary_size.tsv (avf_write_summary_size / feeder.write_summary_size) on random blocks, without a GPU: row for row what write_summary_named writes for the
zero-padded tally of each (scope, bin), with the `filter` column replaced by the bin's name and the BASEPAIR / RECORD_BP rows dropped."""
import numpy as np
import pytest

from aardvark_amd import feeder
from aardvark_amd._abi import N_FIELDS, N_GROUPS, TALLY_LEN

ALL_METRICS = 31
BINS = ["len_0", "len_1_5", "len_6_15", "len_16_49", "len_ge50"]
NAMES = ["easy", "ha,rd"]  # (a name the .csv form has to quote)


def make_blocks(seed, n_labels, n_bins):
    """SNVs only in bin 0, three indel types (a joint row) and an SV type in the others, one (scope, bin) without any call, one with a type that has truth calls only"""
    rng = np.random.default_rng(seed)
    b = np.zeros((1 + n_labels, n_bins, N_GROUPS, 14), np.uint64)
    for s in range(1 + n_labels):
        for k in range(n_bins):
            for g in ([1] if k == 0 else [2, 3, 4, 5]):
                b[s, k, g] = rng.integers(0, 4000 // (1 + k) + 2, 14)
        b[s, 2, 3, [2, 3, 5, 8, 9, 12, 13]] = 0  # deletions of bin 2: no query call
    if n_labels:
        b[1, 3] = 0
    b[:, :, 0] = b[:, :, 1:].sum(axis=2)
    return b


def read(path):
    """(header, rows) as lists of cells; .csv files are parsed as CSV (quoted cells), everything else is split at tabs"""
    import csv
    text = open(path).read()
    assert text.endswith("\n")
    rows = list(csv.reader(text.split("\n")[:-1])) if path.endswith(".csv") else [l.split("\t") for l in text.split("\n")[:-1]]
    return rows[0], rows[1:]


def want_rows(tmp_path, blocks, names, metrics, ext="tsv"):
    """the rows write_summary_named gives for each (scope, bin)'s zero-padded tally, `filter` replaced, BASEPAIR / RECORD_BP rows dropped"""
    out, head = [], None
    scope_names = ["ALL"] + list(names)
    for s in range(blocks.shape[0]):
        for k in range(blocks.shape[1]):
            tally = np.zeros(TALLY_LEN, np.uint64)
            tally[:N_GROUPS * N_FIELDS].reshape(N_GROUPS, N_FIELDS)[:, :14] = blocks[s, k]
            path = str(tmp_path / ("one." + ext))
            if s == 0:
                feeder.write_summary_named(path, tally, [], np.zeros(1, np.uint64), "job", metrics)
            else:  # the label's rows of a stratified file
                feeder.write_summary_named(path, np.zeros(TALLY_LEN, np.uint64), [scope_names[s]], tally[None, :], "job", metrics)
            head, rows = read(path)
            for cells in rows:
                if cells[2] != scope_names[s] or cells[1] in ("BASEPAIR", "RECORD_BP"):
                    continue
                assert cells[3] == "ALL"
                out.append(cells[:3] + [BINS[k]] + cells[4:])
    return head, out


@pytest.mark.parametrize("seed", [1, 2])
def test_rows_equal_write_summary_named(tmp_path, seed):
    blocks = make_blocks(seed, 2, 5)
    path = str(tmp_path / "summary_size.tsv")
    feeder.write_summary_size(path, BINS, NAMES, blocks, "job", ALL_METRICS)
    got_head, cells = read(path)
    head, want = want_rows(tmp_path, blocks, NAMES, ALL_METRICS)
    assert got_head == head and cells == want and len(want) > 100
    assert {c[1] for c in cells} == {"GT", "HAP", "WEIGHTED_HAP"}
    assert any(c[4] == "JointIndel" for c in cells) and any(c[2] == "ha,rd" for c in cells) and {c[3] for c in cells} == set(BINS)
    # the (scope, bin) without a call still has its ALL row per kind, as a tally of zeros has
    assert [c[4] for c in cells if c[2] == "easy" and c[3] == "len_16_49"] == ["ALL"] * 3


def test_csv_paths_are_comma_separated(tmp_path):
    blocks = make_blocks(3, 2, 5)
    path = str(tmp_path / "summary_size.csv")
    feeder.write_summary_size(path, BINS, NAMES, blocks, "job", ALL_METRICS)
    lines = open(path).read().split("\n")[:-1]
    assert "\t" not in "".join(lines) and lines[0].count(",") == 15 and any('"ha,rd"' in l for l in lines)
    got_head, cells = read(path)
    head, want = want_rows(tmp_path, blocks, NAMES, ALL_METRICS, ext="csv")
    assert got_head == head and cells == want and len(want) > 100 and any(c[2] == "ha,rd" for c in cells)


def test_a_mask_without_hap_leaves_the_hap_rows_out(tmp_path):
    blocks = make_blocks(4, 0, 5)
    path = str(tmp_path / "gt.tsv")
    feeder.write_summary_size(path, BINS, [], blocks[:1], "job", feeder.METRIC_GT | feeder.METRIC_BASEPAIR)
    _, rows = read(path)
    assert rows and {r[1] for r in rows} == {"GT"} and {r[2] for r in rows} == {"ALL"}
    feeder.write_summary_size(path, BINS, [], blocks[:1], "job", feeder.METRIC_GT | feeder.METRIC_WEIGHTED_HAP)
    _, rows = read(path)
    assert {r[1] for r in rows} == {"GT", "WEIGHTED_HAP"}
    head, want = want_rows(tmp_path, blocks[:1], [], feeder.METRIC_GT | feeder.METRIC_WEIGHTED_HAP)
    assert rows == want


def test_refusals(tmp_path):
    blocks = make_blocks(5, 1, 5)
    with pytest.raises(ValueError):
        feeder.write_summary_size(str(tmp_path / "bad.tsv"), BINS, ["a", "b"], blocks)
    with pytest.raises(ValueError):
        feeder.write_summary_size(str(tmp_path / "bad.tsv"), BINS[:4], ["a"], blocks)
    with pytest.raises(feeder.FeederError):
        feeder.write_summary_size(str(tmp_path / "no" / "such" / "dir.tsv"), BINS, ["a"], blocks)
