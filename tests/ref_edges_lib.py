"""The 2-bit reference at its word, flag-word and contig edges: a plain numpy reference of the packed layout (written from the description in
include/aardvark_amd.h, not from the packing code), the references test (a) uploads, and the placed windows of tests (b) and (c).
Shared by test_gpu_ref_edges.py (the device packer and the kernels' window fetch) and test_ref_pack_layout.py (the emulator's copy)."""
import numpy as np

from aardvark_amd import RegionBatch

# ---- the layout, in numpy ---------------------------------------------------------------------------------------------------------------

_CODE = np.zeros(256, np.uint32)
_BAD = np.ones(256, bool)
for _i, _ch in enumerate(b"ACGT"):
    _CODE[_ch], _BAD[_ch] = _i, False


def pack_reference_np(contigs):
    """(packed words, flag words) of the concatenated contigs: base p in bits 2 (p % 16) .. of word p / 16, A 0, C 1, G 2, T 3, anything else 0 and bit w % 32 of
    flag word w / 32 set for its word w; positions past the end are 0 and raise no flag.  The flag array has the length avk_debug_ref_packed returns
    (n_words / 32 + 8): the words behind the covered ones are 0."""
    cat = np.concatenate([np.frombuffer(bytes(c), np.uint8) for c in contigs] + [np.zeros(0, np.uint8)])
    n_words = (cat.size + 15) // 16
    code = np.zeros(n_words * 16, np.uint32)
    bad = np.zeros(n_words * 16, bool)
    code[:cat.size], bad[:cat.size] = _CODE[cat], _BAD[cat]
    words = (code.reshape(n_words, 16) << (2 * np.arange(16, dtype=np.uint32))).sum(axis=1, dtype=np.uint64).astype(np.uint32)
    n_flags = n_words // 32 + 8
    bits = np.zeros(n_flags * 32, np.uint64)
    bits[:n_words] = bad.reshape(n_words, 16).any(axis=1)
    flags = (bits.reshape(n_flags, 32) << np.arange(32, dtype=np.uint64)).sum(axis=1, dtype=np.uint64).astype(np.uint32)
    return words, flags


# ---- test (a): references whose word counts sit on the wave (64 words) and flag-word (32 words) edges of the packing launch ---------------

WORD_COUNTS = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1027]
ALPHABET = b"ACGTNacgtRY"
OTHER = b"NacgtRY"


def edge_reference(n_words, extra, seed):
    """three contigs of 16 (n_words - 1) + extra bases in all (extra 1 .. 16; below 16 the last word is partial), no contig base a multiple of 16 where the
    length allows it; sparse other symbols (one base in forty) plus placed ones: the first and last base of every contig and bases 15, 16, 511, 512, 1023,
    1024 of the concatenation"""
    rng = np.random.default_rng(seed)
    total = 16 * (n_words - 1) + extra
    cat = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=total)].copy()
    other = np.frombuffer(OTHER, np.uint8)
    sparse = rng.random(total) < 1 / 40
    cat[sparse] = other[rng.integers(0, other.size, size=int(sparse.sum()))]
    a, b = total // 3, total // 3
    if total >= 40:
        a += (5 - a) % 16  # the second contig starts at a base = 5 (mod 16), the third at 11 (mod 16)
        b += (11 - (a + b)) % 16
    cuts = [0, a, a + b, total]
    placed = [c for c in cuts[:-1]] + [c - 1 for c in cuts[1:]] + [15, 16, 511, 512, 1023, 1024]
    for k, p in enumerate(placed):
        if 0 <= p < total:
            cat[p] = other[k % other.size]
    return [bytes(cat[cuts[i]:cuts[i + 1]]) for i in range(3)]


def edge_references():
    """the references of test (a), longest first and shortest last (each upload on the same context must leave nothing of the one before), then an empty one
    and references of one base"""
    refs = []
    for k, nw in enumerate(sorted(WORD_COUNTS, reverse=True)):
        refs.append(edge_reference(nw, 16, 100 + k))  # the last word full
        refs.append(edge_reference(nw, 1 + (5 * k + 2) % 15, 200 + k))  # 1 .. 15 bases in the last word
    refs.sort(key=lambda cs: -sum(len(c) for c in cs))
    return refs + [[], [b"N"], [b"G"], [b"", b"t", b""]]


# ---- tests (b) and (c): windows placed at the edges, three regions (one per kernel class) on each ------------------------------------------

KINDS = ("contig_start", "contig_end", "shared_word", "flag_bit0", "flag_bit31", "flag_straddle", "len192")
PLACES = ("clean", "first", "last", "before", "after", "word_before", "word_after")
BLOCK = 512  # bases a flag word covers


def placed_sites():
    """-> (contig cuts in the concatenation, sites); a site = (kind, start offset within its word, global start, global end).  Block i of 512 bases has a site of the
    flag-word kinds at its first base (i = 1 .. 48) and, around its middle, a contig boundary with a site of the contig kinds (i = 0 .. 47) or a window of 192
    bases (i = 48 .. 63); sites are at least three packed words apart, so that what one variant writes next to a window touches no other window.  Contig 0
    also has a window at base 0, and the last contig one that ends with the reference, inside a partly filled last word."""
    total = 64 * BLOCK + 41
    cuts, sites = [0], [("contig_start", 0, 0, 44)]
    for i in range(64):
        s, b0, mid = i % 16, BLOCK * i, BLOCK * i + 256
        if 1 <= i <= 16:  # the window's words start at bit 0 of a flag word
            sites.append(("flag_bit0", s, b0 + s, b0 + s + 40))
        elif 17 <= i <= 32:  # ... end at bit 31 of a flag word
            sites.append(("flag_bit31", s, b0 - 48 + s, b0 - s % 5))
        elif 33 <= i <= 48:  # ... straddle two flag words
            sites.append(("flag_straddle", s, b0 - 32 + s, b0 - 32 + s + 56))
        if i < 16:  # the window starts at base 0 of a contig whose base is = s (mod 16)
            cuts.append(mid + s)
            sites.append(("contig_start", s, mid + s, mid + s + 44))
        elif i < 32:  # ... ends at the contig's last base
            cut = mid + 5 + i % 7
            cuts.append(cut)
            sites.append(("contig_end", s, cut - 36 - (cut - 36 - s) % 16, cut))
        elif i < 48:  # ... ends one to three bases before it, in a word the next contig starts in
            cut = mid + 4 + i % 12
            end = cut - 1 - i % 3
            cuts.append(cut)
            sites.append(("shared_word", s, end - 36 - (end - 36 - s) % 16, end))
        else:  # the lane limit: 13 packed words, 14 when shifted
            sites.append(("len192", s, b0 + 160 + s, b0 + 160 + s + 192))
    sites.append(("contig_end", (total - 45) % 16, total - 45, total))
    cuts.append(total)
    for kind, s, g0, g1 in sites:
        assert g0 % 16 == s and 0 <= g0 < g1 <= total, (kind, s, g0, g1)
    return cuts, sites


def dirt_position(place, g0, g1, total):
    """global position of the one byte the variant `place` makes an N or a lower-case base for the window [g0, g1); None where there is no such position"""
    w0, w1 = g0 // 16, (g1 - 1) // 16
    p = {"clean": None, "first": g0, "last": g1 - 1, "before": g0 - 1 if g0 % 16 else None, "after": g1 if g1 % 16 else None,
         "word_before": 16 * (w0 - 1) + 7 if w0 else None, "word_after": 16 * (w1 + 1) + 7}[place]
    return p if p is not None and 0 <= p < total else None


def placed_windows(place, seed=7):
    """-> (contigs, batch, info) of the variant `place`: the same reference and the same regions in every variant but for the one byte per site.
    info: per region, (kind, class the region is built for, first packed word, last packed word, for a 'pair' region the packed word under its call) — 'pair': the same SNV on both sides; 'lane': one to three
    SNVs in the truth, the query's a subset of them; 'wide': a cluster of four to eight unphased heterozygous SNVs on both sides."""
    rng = np.random.default_rng(seed)
    cuts, sites = placed_sites()
    total = cuts[-1]
    acgt = np.frombuffer(b"ACGT", np.uint8)
    cat = acgt[rng.integers(0, 4, size=total)].copy()
    draws = np.random.default_rng(seed + 1)  # the calls: the same in every variant
    regions, info = [], []
    for k, (kind, s, g0, g1) in enumerate(sites):
        p = dirt_position(place, g0, g1, total)
        if p is not None:
            cat[p] = b"NgNaNcNt"[k % 8]
        c = int(np.searchsorted(cuts, g0, side="right")) - 1
        assert cuts[c] <= g0 and g1 <= cuts[c + 1]
        start, end = g0 - cuts[c], g1 - cuts[c]

        def snvs(n, zyg):
            pos = np.sort(draws.choice(np.arange(g0 + 2, g1 - 2), size=n, replace=False))
            out = []
            for q in pos:
                ref = int(cat[q])
                alt = int(acgt[(int(np.flatnonzero(acgt == ref)[0]) + 1 + int(draws.integers(0, 3))) % 4])
                out.append((int(q) - cuts[c], bytes([ref]), bytes([alt]), "Snv", zyg[int(draws.integers(0, len(zyg)))]))
            return out

        one = snvs(1, ["UnphasedHeterozygous", "HomozygousAlternate", "PhasedHet01"])
        pair = {"truth": one, "query": [one[0][:4] + (("UnphasedHeterozygous", "HomozygousAlternate")[k % 2],)]}
        few = snvs(1 + k % 3, ["UnphasedHeterozygous", "HomozygousAlternate", "PhasedHet10"])
        lane = {"truth": few, "query": few[:len(few) - (k // 3) % 2] if len(few) > 1 else []}
        many = snvs(4 + k % 5, ["UnphasedHeterozygous"])
        wide = {"truth": many, "query": [v for j, v in enumerate(many) if j != k % len(many) or k % 4]}
        for cls, calls in (("pair", pair), ("lane", lane), ("wide", wide)):
            regions.append(dict(calls, start=start, end=end, contig=c))
            info.append((kind, cls, g0 // 16, (g1 - 1) // 16, (cuts[c] + one[0][0]) // 16 if cls == "pair" else None))
    contigs = [bytes(cat[cuts[i]:cuts[i + 1]]) for i in range(len(cuts) - 1)]
    return contigs, RegionBatch.from_regions(regions), info


def window_flagged(info, flags, pairs_looked_up=False):
    """per region: does a packed word its window touches have its flag set?  pairs_looked_up: a region with the same SNV on both sides is not searched but looked up
    (avk_pairs.inl), and the lookup reads the base under the call and nothing else of the window: for those regions, the flag of that one word"""
    bit = lambda w: (int(flags[w >> 5]) >> (w & 31)) & 1
    return np.array([bool(bit(wc)) if pairs_looked_up and wc is not None else any(bit(w) for w in range(w0, w1 + 1)) for _, _, w0, w1, wc in info])
