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


def reordered(b, order):
    """RegionBatch `b` with its regions in the order `order` (indices into b): calls and allele bytes follow their regions, region ids are renumbered"""
    order = np.asarray(order, np.int64)
    assert np.array_equal(b.q_off, b.t_off + b.t_cnt.astype(np.uint64)) and np.array_equal(b.a1_off, b.a0_off + b.a0_len.astype(np.uint64))
    excl = lambda x: np.concatenate([[0], np.cumsum(x)[:-1]]).astype(np.int64) if x.size else np.zeros(0, np.int64)
    cnt = (b.t_cnt.astype(np.int64) + b.q_cnt)[order]
    voff = excl(cnt)
    calls = np.repeat(b.t_off.astype(np.int64)[order] - voff, cnt) + np.arange(int(cnt.sum()))
    alen = (b.a0_len.astype(np.int64) + b.a1_len)[calls]
    aoff = excl(alen)
    src = np.repeat(b.a0_off.astype(np.int64)[calls] - aoff, alen) + np.arange(int(alen.sum()))
    return RegionBatch(np.arange(order.size).astype(np.uint64), b.contig_idx[order], b.start[order], b.end[order], voff, b.t_cnt[order], voff + b.t_cnt[order], b.q_cnt[order],
                       b.var_pos[calls], b.var_type[calls], b.var_zyg[calls], b.var_raw_space[calls], aoff, b.a0_len[calls], aoff + b.a0_len[calls], b.a1_len[calls],
                       b.allele_bytes[src])


WHERE = ("last", "first", "middle")


def placed(batch, n_injected, where):
    """`batch` whose last `n_injected` regions are the injected ones, with those regions last (as it is), first or in the middle of the ordinary regions: the
    truly oversize values then precede tens of thousands of ordinary entries"""
    n = batch.n_regions - n_injected
    body, extra = np.arange(n), np.arange(n, batch.n_regions)
    if where == "last":
        return batch
    return reordered(batch, np.concatenate([extra, body] if where == "first" else [body[:n // 2], extra, body[n // 2:]]))


def genome_job(scale=0.004, where="last"):
    contigs, batch = synth.config_genome(scale=scale, threads=4)
    return contigs, placed(with_injections(contigs, batch, at=60_000), len(injected_regions(np.asarray(contigs[0]).tobytes(), at=60_000)), where)


def indel_mix_job(n_truth=3000, contig_len=1_200_000, where="last"):
    contig, batch = synth.config_indel_mix_v2(n_truth=n_truth, contig_len=contig_len)
    return [contig], placed(with_injections([contig], batch, at=300_000), len(injected_regions(np.asarray(contig).tobytes(), at=300_000)), where)


def escaped(batch):
    """(CompactBatch, PackedBatch with escapes) of a RegionBatch"""
    cb = CompactBatch.from_region_batch(batch)
    return cb, PackedBatch.from_compact(cb, escapes=True)


def merge_job(scale=0.0008, at=30_000, many=260, where="last"):
    """three call sets (synth.config_genome_merge) plus injected MultiRegions: long alleles in one, two or all inputs, a long window, an input with more than
    255 calls -> (contigs, MultiBatch); where: the injected MultiRegions last, first or in the middle of the others"""
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
    whole = MultiBatch(3, region_id=np.arange(mb.n_regions + extra.n_regions), contig_idx=cat("contig_idx"), start=cat("start"), end=cat("end"),
                       in_off=cat("in_off", mb.n_variants), in_cnt=cat("in_cnt"), var_pos=cat("var_pos"), var_type=cat("var_type"), var_zyg=cat("var_zyg"),
                       var_raw_space=cat("var_raw_space"), a0_off=cat("a0_off", mb.allele_bytes.size if mb.n_variants else 0), a0_len=cat("a0_len"),
                       a1_off=cat("a1_off", mb.allele_bytes.size if mb.n_variants else 0), a1_len=cat("a1_len"),
                       allele_bytes=np.concatenate([mb.allele_bytes[:int((mb.a0_len.astype(np.int64) + mb.a1_len).sum())], extra.allele_bytes]))
    if where == "last":
        return contigs, whole
    n = mb.n_regions
    body, tail = np.arange(n), np.arange(n, whole.n_regions)
    return contigs, reordered_multi(whole, np.concatenate([tail, body] if where == "first" else [body[:n // 2], tail, body[n // 2:]]))


def reordered_multi(mb, order):
    """MultiBatch `mb` with its MultiRegions in the order `order`: calls and allele bytes follow their regions"""
    order, k = np.asarray(order, np.int64), mb.n_inputs
    excl = lambda x: np.concatenate([[0], np.cumsum(x)[:-1]]).astype(np.int64) if x.size else np.zeros(0, np.int64)
    ic = mb.in_cnt.astype(np.int64).reshape(-1, k)[order]
    cnt = ic.sum(axis=1)
    voff = excl(cnt)
    calls = np.repeat(mb.in_off.astype(np.int64).reshape(-1, k)[order, 0] - voff, cnt) + np.arange(int(cnt.sum()))
    alen = (mb.a0_len.astype(np.int64) + mb.a1_len)[calls]
    aoff = excl(alen)
    src = np.repeat(mb.a0_off.astype(np.int64)[calls] - aoff, alen) + np.arange(int(alen.sum()))
    return MultiBatch(k, region_id=np.arange(order.size), contig_idx=mb.contig_idx[order], start=mb.start[order], end=mb.end[order], in_off=excl(ic.reshape(-1)),
                      in_cnt=ic.reshape(-1), var_pos=mb.var_pos[calls], var_type=mb.var_type[calls], var_zyg=mb.var_zyg[calls], var_raw_space=mb.var_raw_space[calls],
                      a0_off=aoff, a0_len=mb.a0_len[calls], a1_off=aoff + mb.a0_len[calls].astype(np.int64), a1_len=mb.a1_len[calls], allele_bytes=mb.allele_bytes[src])


# ---- promotion: the same batch with more of its entries in the escape lists -------------------------------------------------------------------

def promote(pb, regions=(), slots=(), calls=()):
    """A PackedBatch / PackedMultiBatch that stands for the same batch as `pb`, with regions `regions`, count slots `slots` (compare form: 2r / 2r + 1 = t_cnt / q_cnt
    of region r; multi form: m * k + i) and calls `calls` — indices into pb's own arrays — moved into the escape lists: their values go to the lists, their narrow
    fields are zeroed, the lists stay merged and ascending with what pb already lists and keep pb's bases.  A listed entry takes its value from the list whatever
    the value (include/aardvark_amd.h: avk_packed_escapes), so lists of any length cost nothing to solve."""
    from aardvark_amd._abi import PackedEscapes
    length, cnt, rel, a0, a1 = pb._wide_fields()
    e = pb.escapes if pb.escapes is not None else PackedEscapes()
    local = lambda idx, first, more: np.union1d((idx - np.uint64(first)).astype(np.int64), np.asarray(more, np.int64).reshape(-1))
    r, s, v = local(e.esc_region, e.first_region, regions), local(e.esc_slot, e.first_slot, slots), local(e.esc_call, e.first_call, calls)
    assert (r.size == 0 or (r[0] >= 0 and r[-1] < length.size)) and (s.size == 0 or (s[0] >= 0 and s[-1] < cnt.size)) and (v.size == 0 or (v[0] >= 0 and v[-1] < rel.size))
    esc = PackedEscapes(e.first_region, e.first_call, e.first_slot, esc_region=r + e.first_region, esc_len=length[r], esc_slot=s + e.first_slot, esc_cnt=cnt[s],
                        esc_call=v + e.first_call, esc_rel_pos=rel[v], esc_a0_len=a0[v], esc_a1_len=a1[v])
    length[r], cnt[s], rel[v], a0[v], a1[v] = 0, 0, 0, 0, 0
    arrays = {f: getattr(pb, f) for f in type(pb).FIELDS}
    arrays.update(len=length, var_rel_pos=rel, a0_len=a0, a1_len=a1)
    if hasattr(pb, "n_inputs"):
        return type(pb)(pb.n_inputs, escapes=esc, in_cnt=cnt, **{f: x for f, x in arrays.items() if f != "in_cnt"})
    return type(pb)(escapes=esc, t_cnt=cnt[0::2], q_cnt=cnt[1::2], **{f: x for f, x in arrays.items() if f not in ("t_cnt", "q_cnt")})


BLOCK_EDGES = (4095, 4096, 4097, 8191, 8192)  # both sides of the first two edges of the 4096-element blocks the narrow prefix sums run in (AVK_PS_BLOCK)
DRAWS = tuple((seed, size) for seed in (1, 2, 3) for size in (1023, 1024, 1025, 3000))


def promotion_table(pb, draws=True):
    """name -> (regions, slots, calls) to promote, chosen by rule: the places where a search, a running sum or a block edge can be off by one.  A list shorter than
    an index or a draw asks for takes what it has (the tests that need the full size assert it)."""
    n, nv = pb.n_regions, pb.n_variants
    per = pb.n_inputs if hasattr(pb, "n_inputs") else 2
    ns = n * per
    cnt = pb._wide_fields()[1].reshape(n, per).sum(axis=1)
    voff = np.concatenate([[0], np.cumsum(cnt)])
    busy = int(np.argmax(cnt))  # the region with the most calls (an injected one: a listed count among its slots)
    plain = int(np.flatnonzero((cnt >= 2) & (np.arange(n) > n // 3))[0])  # an ordinary region with calls, a third of the way in
    inside = lambda idx, size: [i for i in idx if i < size]
    every = lambda r: np.arange(r * per, (r + 1) * per)
    table = {
        "nothing": ([], [], []),
        "entry_0": ([0], [0], [0]),
        "last_entry": ([n - 1], [ns - 1], [nv - 1]),
        "slots_and_window_of_one_region": ([plain], every(plain), []),
        "slots_and_window_of_the_busiest_region": ([busy], every(busy), []),
        "64_consecutive_calls": ([], [], np.arange(nv // 2, min(nv // 2 + 64, nv))),
        "every_call_of_one_region": ([], [], np.arange(voff[plain], voff[plain + 1])),
        "every_call_of_the_busiest_region": ([busy], every(busy), np.arange(voff[busy], voff[busy + 1])),
        "block_edges": (inside(BLOCK_EDGES, n), inside(BLOCK_EDGES, ns), inside(BLOCK_EDGES, nv)),
        "every_second": (np.arange(0, n, 2), np.arange(0, ns, 2), np.arange(0, nv, 2)),
        "every_second_odd": (np.arange(1, n, 2), np.arange(1, ns, 2), np.arange(1, nv, 2)),
        "all_calls": ([], [], np.arange(nv)),
        "everything": (np.arange(n), np.arange(ns), np.arange(nv)),
    }
    for seed, size in DRAWS if draws else ():
        table["draw_%d_of_%d" % (seed, size)] = exact_promotion(pb, (min(size, n), min(size, ns), min(size, nv)), seed, edges=False)
    return table


def promotion(pb, name):
    """promotion_table(pb)[name] without making the rest of the table's draws"""
    if name.startswith("draw_"):
        seed, size = int(name.split("_")[1]), int(name.rsplit("_", 1)[1])
        per = pb.n_inputs if hasattr(pb, "n_inputs") else 2
        return exact_promotion(pb, (min(size, pb.n_regions), min(size, pb.n_regions * per), min(size, pb.n_variants)), seed, edges=False)
    return promotion_table(pb, draws=False)[name]


def exact_promotion(pb, sizes, seed=0, edges=True):
    """(regions, slots, calls) to promote so that the three lists of the promoted batch have exactly `sizes` entries, what pb lists already included: a seeded
    draw; edges: both ends of the batch and both sides of the block edges first — lists of an exact length for the scan's chunks of 1024"""
    per = pb.n_inputs if hasattr(pb, "n_inputs") else 2
    e, out = pb.escapes, []
    for m, size, idx, first in ((pb.n_regions, sizes[0], e.esc_region, e.first_region), (pb.n_regions * per, sizes[1], e.esc_slot, e.first_slot),
                                (pb.n_variants, sizes[2], e.esc_call, e.first_call)):
        have = (idx - np.uint64(first)).astype(np.int64)
        assert have.size <= size <= m, (have.size, size, m)
        must = np.setdiff1d([i for i in BLOCK_EDGES + (0, m - 1) if i < m] if edges else [], have).astype(np.int64)[:size - have.size]
        rest = np.setdiff1d(np.arange(m), np.concatenate([have, must]))
        rng = np.random.default_rng(1000 * seed + size)
        out.append(np.sort(np.concatenate([must, rng.choice(rest, size - have.size - must.size, replace=False)])))
    return tuple(out)


PROMOTIONS = ("nothing", "entry_0", "last_entry", "slots_and_window_of_one_region", "slots_and_window_of_the_busiest_region", "64_consecutive_calls",
              "every_call_of_one_region", "every_call_of_the_busiest_region", "block_edges", "every_second", "every_second_odd", "all_calls", "everything") + tuple(
                  "draw_%d_of_%d" % d for d in DRAWS)


# ---- batches that break the form: AVK_E_ARG everywhere, by contract ----------------------------------------------------------------------------

LISTS = {"region": ("esc_region", "first_region"), "slot": ("esc_slot", "first_slot"), "call": ("esc_call", "first_call")}
SPOILS = ("duplicate", "swap_0_1", "swap_1023_1024", "last_is_count", "first_below_base")


def copy_of(pb):
    """a deep copy of a PackedBatch / PackedMultiBatch and its escapes"""
    from aardvark_amd._abi import PackedEscapes
    e = pb.escapes
    esc = PackedEscapes(e.first_region, e.first_call, e.first_slot, **{f: getattr(e, f).copy() for f in PackedEscapes.FIELDS})
    arrays = {f: (None if getattr(pb, f) is None else getattr(pb, f).copy()) for f in type(pb).FIELDS}
    return type(pb)(pb.n_inputs, escapes=esc, **arrays) if hasattr(pb, "n_inputs") else type(pb)(escapes=esc, **arrays)


def rebased(pb, regions=1_000, slots=None, calls=77_777):
    """`pb` as a slice of a larger batch that has `regions` regions, `slots` count slots (default: regions times the slots of a region) and `calls` calls in front of
    it: the three bases and every listed index shifted by these constants, nothing else (avk_packed_escapes carries the bases for both forms; a batch that has no
    slicing of its own in Python, the multi form, gets non-zero bases this way)"""
    out = copy_of(pb)
    e = out.escapes
    slots = regions * (pb.n_inputs if hasattr(pb, "n_inputs") else 2) if slots is None else slots
    e.first_region, e.first_slot, e.first_call = e.first_region + regions, e.first_slot + slots, e.first_call + calls
    e.esc_region += np.uint64(regions)
    e.esc_slot += np.uint64(slots)
    e.esc_call += np.uint64(calls)
    return out


def spoiled(pb, which, how):
    """a copy of `pb` whose list `which` (LISTS) breaks the rule `how` (SPOILS): an equal neighbour; a swapped pair at 0 / 1 or across the scan's chunk edge at
    1023 / 1024; a last index equal to first + count; a first index of first - 1 (pb must be a slice with non-zero bases).  Only indices change: every value the
    lists and the batch hold stays a value the good batch holds."""
    bad = copy_of(pb)
    per = pb.n_inputs if hasattr(pb, "n_inputs") else 2
    name, first = LISTS[which]
    idx, first = getattr(bad.escapes, name), getattr(bad.escapes, first)
    count = {"region": pb.n_regions, "slot": pb.n_regions * per, "call": pb.n_variants}[which]
    if how == "duplicate":
        assert idx.size >= 2
        idx[idx.size // 2] = idx[idx.size // 2 - 1]
    elif how == "swap_0_1":
        assert idx.size >= 2
        idx[:2] = idx[:2][::-1].copy()
    elif how == "swap_1023_1024":
        assert idx.size >= 2048
        idx[1023:1025] = idx[1023:1025][::-1].copy()
    elif how == "last_is_count":
        assert idx.size >= 1
        idx[-1] = first + count
    elif how == "first_below_base":
        assert idx.size >= 1 and first > 0
        idx[0] = first - 1
    else:
        raise KeyError(how)
    return bad


def narrow_fields(pb):
    return ("len", "in_cnt", "var_rel_pos", "a0_len", "a1_len") if hasattr(pb, "n_inputs") else ("len", "t_cnt", "q_cnt", "var_rel_pos", "a0_len", "a1_len")


def nonzero_under_a_listed_entry(pb, field):
    """a copy of `pb` with a 1 in narrow field `field` of one LISTED entry (the middle one of its list): the form says that field MUST be 0"""
    bad = copy_of(pb)
    e = bad.escapes
    if field == "len":
        getattr(bad, field)[int(e.esc_region[e.esc_region.size // 2] - e.first_region)] = 1
    elif field in ("var_rel_pos", "a0_len", "a1_len"):
        getattr(bad, field)[int(e.esc_call[e.esc_call.size // 2] - e.first_call)] = 1
    else:
        s = (e.esc_slot - np.uint64(e.first_slot)).astype(np.int64)
        if field != "in_cnt":
            s = s[s % 2 == (0 if field == "t_cnt" else 1)] // 2
        getattr(bad, field)[int(s[s.size // 2])] = 1
    return bad


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
