"""The 2-bit copy of the reference that avk_pack_reference makes at avk_ref_upload, and the kernels' window fetch from it, at word, flag-word and contig
edges, on a real MI355X.  (a) the packed words and the flag bitmap, word for word, against a numpy reference of the layout (ref_edges_lib.py);
(b) windows placed at the edges, with one N or lower-case base in or next to them, bit for bit against the oracle; (c) the same batches once per kernel
class, with the counters showing that the class really solved them and that a flag neither gets lost nor spills into the next word."""
import numpy as np
import pytest

import oracle_lib
import ref_edges_lib as rel
from test_gpu_parity import check

pytestmark = pytest.mark.gpu


def make_ctx(**opts):
    import aardvark_amd
    c = aardvark_amd.Context(0)
    for k, v in opts.items():
        c.set_option(k, v)
    return c


def test_packed_copy_word_for_word():
    """every packed word and every flag word of references whose word counts sit on the edges of the packing launch (a wave packs 64 words and writes two flag
    words from one ballot), the longest uploaded first and the shortest last on one context, then an empty reference and references of one base"""
    import aardvark_amd
    ctx = make_ctx()
    try:
        with pytest.raises(aardvark_amd.AardvarkAmdError):  # no reference yet
            ctx.debug_ref_packed()
        refs = rel.edge_references()
        sizes = [sum(len(c) for c in cs) for cs in refs]
        assert sizes[:-4] == sorted(sizes[:-4], reverse=True) and sizes[0] > 16 * 1024 and sizes[-4:] == [0, 1, 1, 1]
        assert {(s + 15) // 16 for s in sizes} >= set(rel.WORD_COUNTS)
        for contigs in refs:
            ctx.upload_reference(contigs)
            words, flags = ctx.debug_ref_packed()
            want_words, want_flags = rel.pack_reference_np(contigs)
            total = sum(len(c) for c in contigs)
            assert words.size == want_words.size == (total + 15) // 16 and flags.size == want_flags.size
            bad = np.flatnonzero(words != want_words)
            assert bad.size == 0, "%d bases: packed word %d is %08x, not %08x" % (total, bad[0], words[bad[0]], want_words[bad[0]])
            bad = np.flatnonzero(flags != want_flags)  # (the words behind the covered ones are 0 in want_flags)
            assert bad.size == 0, "%d bases, %d packed words: flag word %d is %08x, not %08x" % (total, words.size, bad[0], flags[bad[0]], want_flags[bad[0]])
        # too small a capacity is refused
        ctx.upload_reference(refs[0])
        n_words, n_flags = aardvark_amd._abi.ref_packed_sizes(sizes[0])
        w, f = np.zeros(n_words, np.uint32), np.zeros(n_flags, np.uint32)
        P = lambda a: a.ctypes.data_as(aardvark_amd.api.C.POINTER(aardvark_amd.api.C.c_uint32))
        assert ctx.lib.avk_debug_ref_packed(ctx.handle, P(w), n_words - 1, P(f), n_flags) == -1
        assert ctx.lib.avk_debug_ref_packed(ctx.handle, P(w), n_words, P(f), n_flags - 1) == -1
        assert ctx.lib.avk_debug_ref_packed(ctx.handle, P(w), n_words, P(f), n_flags) == 0
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def variants():
    """the seven variants of the placed windows, each with the oracle's results without sequences (test (c) compares every leg with them)"""
    orc = oracle_lib.load()
    out = {}
    for place in rel.PLACES:
        contigs, batch, info = rel.placed_windows(place)
        out[place] = (contigs, batch, info, oracle_lib.compare_batch(orc, batch, contigs, threads=8))
    return out


def test_placed_windows_against_the_oracle(oracle, variants):
    """every output, haplotype sequences included, of the windows at contig, word and flag-word edges: clean, and with one N or lower-case base in the window's
    first or last base, in the same packed word just before or just after it, and in the neighbouring words"""
    kinds = {(k, cls) for k, cls, *_ in variants["clean"][2]}
    assert kinds == {(k, cls) for k in rel.KINDS for cls in ("pair", "lane", "wide")}
    ctx = make_ctx()
    try:
        for place in rel.PLACES:
            contigs, batch, info, _ = variants[place]
            assert 300 <= batch.n_regions <= 400
            check(ctx, oracle, contigs, batch)
            # the device's flags say what the variant is meant to say
            ctx.upload_reference(contigs)
            flagged = rel.window_flagged(info, ctx.debug_ref_packed()[1])
            assert np.array_equal(flagged, rel.window_flagged(info, rel.pack_reference_np(contigs)[1]))
            if place in ("clean", "word_before", "word_after"):
                assert not flagged.any()
            elif place in ("first", "last"):
                assert flagged.all()
            else:
                assert 0 < flagged.sum() < flagged.size
    finally:
        ctx.close()


LEGS = [("default", {}), ("lane_pairs", {"lane_pairs": 0}), ("lane_quad", {"lane_quad": 0}), ("wide_kernel", {"wide_kernel": 0}), ("lane_kernel", {"lane_kernel": 0}),
        ("use_packed_reference", {"use_packed_reference": 0})]


def run_leg(ctx, contigs, batch, want):
    from aardvark_amd import CompareConfig
    ctx.upload_reference(contigs)
    rb = ctx.upload(batch)
    plan = ctx.work_order(rb, want_order=False)[1]
    ctx.compare_resident(rb, CompareConfig(enable_sequences=False))
    got = ctx.download(rb)
    rb.free()
    assert got.diff(want) == []
    return plan, ctx.last_lane_solved(), ctx.last_wide_solved(), ctx.last_tier_counts()


def test_one_leg_per_kernel_class(variants):
    """The placed windows with the defaults (the lane classes switched on whatever the batch size, as a genome's batch has them), then with the looked-up pairs, the
    quads, the wide kernel, the lanes and the 2-bit reference switched off, one at a time: every leg gives the oracle's outputs, and the counters say that the
    kernels the leg leaves on solved regions.  A flagged word turns its window away from the lanes and the wide kernel (variants first, last: every window has one);
    a flagged word NEXT to a window does not (variants word_before, word_after: as many regions as in the clean variant)."""
    counts = {}
    for leg, opts in LEGS:
        ctx = make_ctx(lane_min_regions=0, lane_min_batch=0, **opts)
        try:
            for place in rel.PLACES:
                contigs, batch, info, want = variants[place]
                plan, lanes, wide, tiers = run_leg(ctx, contigs, batch, want)
                print(leg, place, "lanes", lanes, "wide", wide, "tiers", tiers, "plan", plan)
                counts[leg, place] = (lanes, wide, tiers, plan)
                n = batch.n_regions
                assert lanes + wide + sum(tiers[:4]) == n and tiers[4] == 0  # every region is finished by exactly one kernel
                looked_up = leg in ("default", "lane_quad", "wide_kernel")  # the legs with the pairs' lookup, which reads the word under the call only
                flagged = rel.window_flagged(info, rel.pack_reference_np(contigs)[1], pairs_looked_up=looked_up)
                assert lanes + wide <= int((~flagged).sum())
                counts[leg, place] += (int((~flagged).sum()),)
                if leg == "lane_kernel":
                    assert lanes == 0
                if leg == "wide_kernel":
                    assert wide == 0
                if leg == "use_packed_reference":
                    assert lanes == 0 and wide == 0 and sum(tiers[:4]) == n
        finally:
            ctx.close()
    n = variants["clean"][1].n_regions
    lanes0, wide0, _, plan0 = counts["default", "clean"][:4]
    n_pairs, n_three = plan0["fast"][5][1], plan0["fast"][4][1]
    # the default leg: the lanes, the looked-up pairs and the wide kernel all solved regions (a third of the regions is built for each; the three-call class runs
    # 16 records per wave, that is on quads)
    assert n_pairs >= n // 6 and n_three > 0 and plan0["lanes"] >= n // 2
    assert lanes0 > plan0["lanes"] - n_pairs  # more than the searched classes hold: looked-up pairs among them
    assert lanes0 >= n // 2 and wide0 >= n // 6
    for place in rel.PLACES:
        d_lanes, d_wide = counts["default", place][:2]
        # without the pairs' lookup the same regions are the lanes' where no window has a flag (a lookup hands over what the zygosities alone do not decide; where
        # windows have flags it takes more than the lanes do: it reads the word under its call alone)
        if place in ("clean", "word_before", "word_after"):
            assert counts["lane_pairs", place][0] >= d_lanes
        assert counts["lane_quad", place][:2] == (d_lanes, d_wide)  # one lane per region instead of four: the same regions
        assert counts["wide_kernel", place][0] == d_lanes
    assert counts["lane_kernel", "clean"][1] > 0 and counts["wide_kernel", "clean"][0] > 0 and counts["lane_pairs", "clean"][0] > 0
    for leg, _ in LEGS:
        c_lanes, c_wide = counts[leg, "clean"][:2]
        for place in ("first", "last"):  # a flag in the window: no flag is lost (only a lookup, which reads the word under its call alone, may still take its region)
            assert counts[leg, place][1] == 0
            if leg in ("lane_pairs", "lane_kernel", "use_packed_reference"):
                assert counts[leg, place][0] == 0
        for place in ("word_before", "word_after"):  # a flag in the neighbouring word: it does not spill into the window's
            assert counts[leg, place][:2] == (c_lanes, c_wide), (leg, place)
        for place in ("before", "after"):  # in the window's own first or last word, where the window does not fill it: some regions, not all
            assert counts[leg, place][0] <= c_lanes and counts[leg, place][1] <= c_wide
            if c_wide:
                assert 0 < counts[leg, place][1] < c_wide
            if c_lanes:
                assert 0 < counts[leg, place][0] < c_lanes
