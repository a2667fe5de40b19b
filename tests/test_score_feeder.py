"""The scores of a VCF's records for the curve by query score (avf_vcf_scores, avf_feed_scores; feeder.vcf_scores, feeder.feed_compare(score_field=)) on a small
BGZF VCF the test writes: QUAL and FORMAT/GQ of the chosen sample, '.', an absent key, a value that is no number, a record the parser drops (it still counts as
a data line), and a multi-allelic record whose two calls get its score through var_record.  No GPU."""
import numpy as np
import pytest

from aardvark_amd import feeder
from test_feeder import bgzf_bytes

HEAD = ("##fileformat=VCFv4.2\n##contig=<ID=chrS>\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n"
        "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1\tS2\n")
SEQ = "ACGTTGCAAGCTTAGCCGATCGATTACGGCAT" * 40
NAN = float("nan")


def ref_at(pos0, n=1):
    return SEQ[pos0:pos0 + n]


def other(b):
    return "C" if b != "C" else "G"


# (pos0, alt, QUAL, FORMAT, S1, S2) -> what QUAL, GQ of S1 and GQ of S2 must read
QUERY = [(100, None, "33.5", "GT:GQ", "1/1:20", "0/1:7", 33.5, 20.0, 7.0),
         (200, None, ".", "GT:GQ", "1/1:.", "1/1:99", NAN, NAN, 99.0),
         (300, None, "12", "GT", "0/1", "0/1", 12.0, NAN, NAN),
         (400, None, "abc", "GT:DP:GQ", "1/1:30:4x", "1/1:30:15.25", NAN, NAN, 15.25),
         (500, None, "7e1", "GT:GQ", "./.:3", "1/1:2", 70.0, 3.0, 2.0),     # no call for S1: the parser drops it, the line still counts
         (600, "MULTI", "50", "GQ:GT", "41:1/2", "5:0/1", 50.0, 41.0, 5.0),  # two ALT alleles: two calls, one record
         (700, None, "0", "GT:GQ", "1/1", "1/1", 0.0, NAN, NAN)]              # the sample column ends before GQ


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d = tmp_path_factory.mktemp("score_feeder")
    fa, bed, t, q = (str(d / n) for n in ("s.fa", "s.bed", "t.vcf.gz", "q.vcf.gz"))
    open(fa, "w").write(">chrS\n" + "\n".join(SEQ[i:i + 60] for i in range(0, len(SEQ), 60)) + "\n")
    open(bed, "w").write("chrS\t10\t%d\n" % (len(SEQ) - 10))
    lines = []
    for pos, alt, qual, fmt, s1, s2, *_ in QUERY:
        alts = other(ref_at(pos)) if alt is None else ",".join(b for b in "ACGT" if b != ref_at(pos))[:3]
        lines.append("chrS\t%d\t.\t%s\t%s\t%s\tPASS\t.\t%s\t%s\t%s\n" % (pos + 1, ref_at(pos), alts, qual, fmt, s1, s2))
    open(q, "wb").write(bgzf_bytes((HEAD + "".join(lines)).encode(), block=150))  # (many small blocks: lines cross them)
    truth = "".join("chrS\t%d\t.\t%s\t%s\t88\tPASS\t.\tGT:GQ\t1/1:77\t1/1:77\n" % (pos + 1, ref_at(pos), other(ref_at(pos))) for pos in (100, 200, 250))
    open(t, "wb").write(bgzf_bytes((HEAD + truth).encode(), block=150))
    return dict(fa=fa, bed=bed, t=t, q=q)


def same(a, b):
    return np.array_equal(np.asarray(a, np.float32), np.asarray(b, np.float32), equal_nan=True)


def test_qual_and_gq_per_record(case):
    n = len(QUERY)
    assert same(feeder.vcf_scores(case["q"], "QUAL", n), [r[6] for r in QUERY])
    assert same(feeder.vcf_scores(case["q"], "GQ", n), [r[7] for r in QUERY])          # the first sample
    assert same(feeder.vcf_scores(case["q"], "GQ", n, sample="S1"), [r[7] for r in QUERY])
    assert same(feeder.vcf_scores(case["q"], "GQ", n, sample="S2"), [r[8] for r in QUERY])
    assert same(feeder.vcf_scores(case["q"], "QUAL", 3), [r[6] for r in QUERY[:3]])      # fewer records asked for than the file has
    assert same(feeder.vcf_scores(case["q"], "QUAL", n + 2), [r[6] for r in QUERY] + [NAN, NAN])  # more: missing
    assert feeder.vcf_scores(case["q"], "QUAL", 0).size == 0


def test_refusals(case):
    with pytest.raises(feeder.FeederError, match="QUAL or GQ"):
        feeder.vcf_scores(case["q"], "DP", 3)
    with pytest.raises(feeder.FeederError, match="S9"):
        feeder.vcf_scores(case["q"], "GQ", 3, sample="S9")
    with pytest.raises(feeder.FeederError):
        feeder.vcf_scores(case["q"] + ".missing", "QUAL", 3)


@pytest.mark.parametrize("field,col", [("QUAL", 6), ("GQ", 7)])
def test_scores_in_call_order(case, field, col):
    """every query entry has its record's score, every truth entry NaN; the multi-allelic record's two calls share its score"""
    g = feeder.Genome(case["fa"])
    feed = feeder.feed_compare(case["t"], case["q"], case["bed"], g, score_field=field)
    plain = feeder.feed_compare(case["t"], case["q"], case["bed"], g)
    assert plain.scores is None and np.array_equal(plain.var_record, feed.var_record)
    b, sc = feed.batch, feed.scores
    assert sc.dtype == np.float32 and sc.size == b.n_variants
    is_query = np.zeros(b.n_variants, bool)
    for r in range(b.n_regions):
        is_query[int(b.q_off[r]):int(b.q_off[r]) + int(b.q_cnt[r])] = True
    assert is_query.sum() == 7 and (~is_query).sum() == 3  # six records of S1 with a call, one of them twice; three truth calls
    assert np.isnan(sc[~is_query]).all(), "truth entries carry no score (their own QUAL is 88)"
    want = np.array([QUERY[int(rec)][col] for rec in feed.var_record[is_query]], np.float32)
    assert same(sc[is_query], want)
    multi = np.flatnonzero(is_query & (feed.var_record == 5))
    assert len(multi) == 2 and sorted(feed.var_alt_index[multi]) == [1, 2] and (sc[multi] == QUERY[5][col]).all()
    assert 4 not in set(feed.var_record[is_query])  # (the dropped line left no call, and shifted no index)
    if feed.packed is not None:  # the packed form keeps the feed's call order: one score array serves both
        assert feed.packed.n_variants == b.n_variants
    g.close()
