"""Workloads for the tests of packed batches with escapes (avk_packed_escapes): synthetic batches with a handful of injected regions whose values sit on, just
below and beyond the limits of the narrow packed fields — alleles of 255, 256, 300 and 1,000 to 2,000 bases, windows of 65,535, 65,536 and more bases with
calls at relative positions 65,535 and 65,536, sides of 255, 256 and 300 calls."""
import numpy as np

from aardvark_amd import CompactBatch, PackedBatch, RegionBatch, synth
from aardvark_amd.merge import MultiBatch

SNV, INS, DEL = 0, 1, 2
HOM, HET = 5, 2


def _other(b):
    return b"C" if b != b"C" else b"A"


def _bases(rng, n):
    return bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)])


def _ins(contig, pos, n, rng, zyg=HOM):
    """an insertion whose allele1 has n bases (allele0: the anchor base)"""
    a = bytes(contig[pos:pos + 1])
    return (pos, a, a + _bases(rng, n - 1), INS, zyg)


def _del(contig, pos, n, zyg=HOM):
    """a deletion whose allele0 has n bases"""
    return (pos, bytes(contig[pos:pos + n]), bytes(contig[pos:pos + 1]), DEL, zyg)


def _snv(contig, pos, zyg=HOM):
    a = bytes(contig[pos:pos + 1])
    return (pos, a, _other(a), SNV, zyg)


def injected_regions(contig, at=400_000, seed=5, contig_idx=0, many=300):
    """region dicts on `contig` (bytes-like, ACGT); every region is simple for the search (the same calls on both sides, or one side empty), so that the
    long alleles and windows cost the aligner length, not branching"""
    rng = np.random.default_rng(seed)
    out = []

    def region(start, end, truth, query):
        out.append({"start": start, "end": end, "contig": contig_idx, "truth": truth, "query": query})

    p = at
    for n in (255, 256, 300):  # the border of the 8-bit allele length, on allele1: both sides, truth only, query only
        v = _ins(contig, p + 60, n, rng)
        region(p, p + 200, [v], [v])
        region(p + 1000, p + 1200, [_ins(contig, p + 1060, n, rng)], [])
        region(p + 2000, p + 2200, [], [_ins(contig, p + 2060, n, rng, HET)])
        p += 3000
    for n in (255, 256, 300, 1500):  # ... and on allele0
        v = _del(contig, p + 60, n)
        region(p, p + n + 200, [v], [v])
        region(p + 4000, p + 4000 + n + 200, [_del(contig, p + 4060, n, HET)], [])
        p += 8000
    v = _ins(contig, p + 60, 2000, rng)  # 1,000 to 2,000 bases, on both sides at once
    w = _ins(contig, p + 120, 1000, rng)
    region(p, p + 300, [v, w], [v, w])
    p += 3000
    for length in (65_535, 65_536, 70_000):  # the border of the 16-bit window length; calls at relative positions 65,535 and 65,536
        calls = [_snv(contig, p + 100), _snv(contig, p + 65_000)]
        if length > 65_536 + 50:
            calls += [_snv(contig, p + 65_535), _snv(contig, p + 65_536, HET), _ins(contig, p + 65_600, 256, rng)]
        region(p, p + length, calls, calls)
        p += length + 1000
    for cnt in (255, 256, many):  # the border of the 8-bit call count: the truth side has cnt calls, the query side 255 of them
        calls = [_snv(contig, p + 60 + 12 * i) for i in range(cnt)]
        region(p, p + 60 + 12 * cnt + 60, calls, calls[:255])
        p += 12 * cnt + 1000
    return out


def with_injections(contigs, batch, **kw):
    """`batch` (a RegionBatch on `contigs`) followed by the injected regions on contig 0, region ids running on"""
    extra = RegionBatch.from_regions(injected_regions(np.asarray(contigs[0]).tobytes() if not isinstance(contigs[0], bytes) else contigs[0], **kw))
    extra.region_id = (np.arange(extra.n_regions) + batch.n_regions).astype(np.uint64)
    return synth.concat_batches([batch, extra])


def genome_job(scale=0.004):
    contigs, batch = synth.config_genome(scale=scale, threads=4)
    return contigs, with_injections(contigs, batch, at=60_000)


def indel_mix_job(n_truth=3000, contig_len=1_200_000):
    contig, batch = synth.config_indel_mix_v2(n_truth=n_truth, contig_len=contig_len)
    return [contig], with_injections([contig], batch, at=300_000)


def escaped(batch):
    """(CompactBatch, PackedBatch with escapes) of a RegionBatch"""
    cb = CompactBatch.from_region_batch(batch)
    return cb, PackedBatch.from_compact(cb, escapes=True)


def merge_job(scale=0.0008, at=30_000, many=260):
    """three call sets (synth.config_genome_merge) plus injected MultiRegions: long alleles in one, two or all inputs, a long window, an input with more than
    255 calls -> (contigs, MultiBatch)"""
    contigs, mb = synth.config_genome_merge(scale=scale, k=3, threads=4)
    contig = np.asarray(contigs[0]).tobytes()
    rng = np.random.default_rng(11)
    regions = []
    p = at
    for n in (255, 256, 300, 1200):
        v, d = _ins(contig, p + 60, n, rng), _del(contig, p + 1060, n)
        regions.append({"start": p, "end": p + 200, "contig": 0, "inputs": [[v], [v], [v]]})
        regions.append({"start": p + 1000, "end": p + 1200 + n, "contig": 0, "inputs": [[d], [], [d]]})
        p += 4000
    calls = [_snv(contig, p + 100), _snv(contig, p + 65_535), _snv(contig, p + 65_536)]
    regions.append({"start": p, "end": p + 66_000, "contig": 0, "inputs": [calls, calls, calls[:2]]})
    p += 67_000
    calls = [_snv(contig, p + 60 + 12 * i) for i in range(many)]
    regions.append({"start": p, "end": p + 12 * many + 120, "contig": 0, "inputs": [calls, calls[:255], calls]})
    extra = MultiBatch.from_regions(regions)
    cat = lambda f, sh=0: np.concatenate([getattr(mb, f), getattr(extra, f) + np.asarray(sh, getattr(extra, f).dtype)])
    return contigs, MultiBatch(3, region_id=np.arange(mb.n_regions + extra.n_regions), contig_idx=cat("contig_idx"), start=cat("start"), end=cat("end"),
                               in_off=cat("in_off", mb.n_variants), in_cnt=cat("in_cnt"), var_pos=cat("var_pos"), var_type=cat("var_type"), var_zyg=cat("var_zyg"),
                               var_raw_space=cat("var_raw_space"), a0_off=cat("a0_off", mb.allele_bytes.size if mb.n_variants else 0), a0_len=cat("a0_len"),
                               a1_off=cat("a1_off", mb.allele_bytes.size if mb.n_variants else 0), a1_len=cat("a1_len"),
                               allele_bytes=np.concatenate([mb.allele_bytes[:int((mb.a0_len.astype(np.int64) + mb.a1_len).sum())], extra.allele_bytes]))


def region_contents(b, idx):
    """what regions `idx` of RegionBatch `b` hold, independent of where their calls and alleles lie: per-region fields and, call by call, every field and the allele bytes"""
    idx = np.asarray(idx, np.int64)
    calls = np.concatenate([np.concatenate([np.arange(int(b.t_off[r]), int(b.t_off[r]) + int(b.t_cnt[r])), np.arange(int(b.q_off[r]), int(b.q_off[r]) + int(b.q_cnt[r]))])
                            for r in idx]).astype(np.int64) if idx.size else np.zeros(0, np.int64)
    ab = b.allele_bytes
    alleles = b"".join(ab[int(b.a0_off[v]):int(b.a0_off[v]) + int(b.a0_len[v])].tobytes() + ab[int(b.a1_off[v]):int(b.a1_off[v]) + int(b.a1_len[v])].tobytes() for v in calls)
    return {"contig_idx": b.contig_idx[idx], "start": b.start[idx], "end": b.end[idx], "t_cnt": b.t_cnt[idx], "q_cnt": b.q_cnt[idx], "var_pos": b.var_pos[calls],
            "var_type": b.var_type[calls], "var_zyg": b.var_zyg[calls], "var_raw_space": b.var_raw_space[calls], "a0_len": b.a0_len[calls], "a1_len": b.a1_len[calls],
            "alleles": np.frombuffer(alleles, np.uint8)}


def same_contents(a, b):
    return [f for f in a if not np.array_equal(a[f], b[f])]


# ---- files for the feeder and the two tools: a 300-base insertion, a 2 kbp deletion and — with --min-variant-gap 1000 — one region with 300 calls on a side ----

VCF_HEADER = ("##fileformat=VCFv4.2\n##contig=<ID={c}>\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n"
              "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t{s}\n")
GAP = 1000


def write_feeder_case(folder, length=150_000):
    """-> {"fa", "bed", "t", "q", "vcfs": [three call sets for a merge]} under `folder` (a path), contig chrE"""
    import gzip
    import os
    rng = np.random.default_rng(77)
    seq = _bases(rng, length)
    ins = seq[10_000:10_001] + _bases(rng, 300)
    calls = [(10_000, seq[10_000:10_001], ins, "1/1"), (20_000, seq[20_000:22_001], seq[20_000:20_001], "1/1")]
    dense = [(40_000 + 40 * i, seq[40_000 + 40 * i:40_001 + 40 * i], _other(seq[40_000 + 40 * i:40_001 + 40 * i]), "1/1") for i in range(300)]
    loose = [(60_000 + 2_500 * i, seq[60_000 + 2_500 * i:60_001 + 2_500 * i], _other(seq[60_000 + 2_500 * i:60_001 + 2_500 * i]), "0/1" if i % 3 else "1/1") for i in range(30)]
    sets = {"t": calls + dense + loose, "q": calls + dense[:200] + loose[:25], "third": calls[:1] + dense + loose[5:]}
    p = {k: os.path.join(str(folder), k + ".vcf.gz") for k in sets}
    p["fa"], p["bed"] = os.path.join(str(folder), "e.fa"), os.path.join(str(folder), "e.bed")
    open(p["fa"], "w").write(">chrE\n" + "\n".join(seq[i:i + 80].decode() for i in range(0, length, 80)) + "\n")
    open(p["bed"], "w").write("chrE\t100\t%d\n" % (length - 100))
    for k, cs in sets.items():
        text = VCF_HEADER.format(c="chrE", s="S1") + "".join("chrE\t%d\t.\t%s\t%s\t.\t.\t.\tGT\t%s\n" % (pos + 1, ref.decode(), alt.decode(), gt) for pos, ref, alt, gt in sorted(cs))
        open(p[k], "wb").write(gzip.compress(text.encode()))
    p["vcfs"] = [p["t"], p["q"], p["third"]]
    return p
