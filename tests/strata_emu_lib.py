"""Loader for tests/emu/libstrata_emu.so: the containment rule of the device-made label lists (aardvark_amd/csrc/avk_strata.inl) run on the CPU, and the small
stratified job (three contigs, six labels, every edge of the rule) that tests/test_strata.py and tests/test_gpu_strata.py share.
Test infrastructure for the GPU-less container; built here, into a library of its own, with the flags of tests/emu/Makefile."""
import ctypes as C
import os
import subprocess

import numpy as np

from aardvark_amd import CompactBatch, PackedBatch, RegionBatch

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aardvark_amd", "csrc")
_lib = None
u8p, u16p, u32p, u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint16), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)


class EmuView(C.Structure):
    """strata_emu_view of tests/emu/strata_emu.cpp"""
    _fields_ = [("n_regions", C.c_uint64), ("n_variants", C.c_uint64), ("contig_idx", u32p), ("start", u64p), ("t_off", u64p), ("q_off", u64p), ("t_cnt", u32p), ("q_cnt", u32p),
                ("var_pos", u64p), ("a0_len", u32p), ("pk_start", u32p), ("pk_contig", u16p), ("pk_rel", u16p), ("pk_tc", u8p), ("pk_qc", u8p), ("pk_a0", u8p), ("pk_voff", u64p),
                ("n_labels", C.c_uint32), ("n_contigs", C.c_uint32), ("tree_off", u64p), ("tree_start", u32p), ("tree_end_max", u32p)]


def load():
    global _lib
    if _lib is None:
        import fcntl
        so = os.path.join(EMU_DIR, "libstrata_emu.so")
        deps = [os.path.join(EMU_DIR, "strata_emu.cpp"), os.path.join(ROOT, "include", "aardvark_amd.h")] + [os.path.join(CSRC, f) for f in (
            "avk_strata.inl", "avk_devpack.inl", "avk_pairs.inl", "avk_wave.h", "avk_dev_types.h")]
        with open(os.path.join(EMU_DIR, ".build.lock"), "w") as lock:  # (pytest-xdist workers: one builds, the others wait)
            fcntl.flock(lock, fcntl.LOCK_EX)
            if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
                subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-g", "-std=c++17", "-fPIC", "-Wall", "-Wextra", "-Wno-unused-function", "-Wno-unknown-pragmas",
                                       "-Wno-strict-aliasing", "-pthread", "-shared", "-o", so, "strata_emu.cpp"], cwd=EMU_DIR)
        lib = C.CDLL(so)
        lib.strata_emu_lists.argtypes = [C.POINTER(EmuView), u64p, u32p]
        lib.strata_emu_contains.argtypes = [C.POINTER(EmuView), C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64]
        _lib = lib
    return _lib


def view_of(batch, exported, packed_source=False):
    """(EmuView, the arrays it points into): the device's view of `batch` — its wide arrays, or (packed_source) the packed arrays with the running sum of the
    counts — and of the exported sets (Stratifications.export)"""
    n_labels, n_contigs, tree_off, start, end_max = exported
    k = dict(tree_off=np.ascontiguousarray(tree_off, np.uint64), tree_start=np.ascontiguousarray(np.append(start, 0), np.uint32),
             tree_end_max=np.ascontiguousarray(np.append(end_max, 0), np.uint32))
    if packed_source:
        pb = PackedBatch.from_compact(CompactBatch.from_region_batch(batch))
        assert pb.escapes is None or pb.escapes.empty()
        calls = pb.t_cnt.astype(np.uint64) + pb.q_cnt.astype(np.uint64)
        k.update(pk_start=pb.start, pk_contig=pb.contig_idx, pk_rel=np.append(pb.var_rel_pos, 0).astype(np.uint16), pk_tc=pb.t_cnt, pk_qc=pb.q_cnt,
                 pk_a0=np.append(pb.a0_len, 0).astype(np.uint8), pk_voff=np.concatenate([[0], np.cumsum(calls)]).astype(np.uint64))
    else:
        k.update(contig_idx=np.ascontiguousarray(batch.contig_idx, np.uint32), start=np.ascontiguousarray(batch.start, np.uint64), t_off=np.ascontiguousarray(batch.t_off, np.uint64),
                 q_off=np.ascontiguousarray(batch.q_off, np.uint64), t_cnt=np.ascontiguousarray(batch.t_cnt, np.uint32), q_cnt=np.ascontiguousarray(batch.q_cnt, np.uint32),
                 var_pos=np.ascontiguousarray(np.append(batch.var_pos, 0), np.uint64), a0_len=np.ascontiguousarray(np.append(batch.a0_len, 0), np.uint32))
    v = EmuView()
    v.n_regions, v.n_variants, v.n_labels, v.n_contigs = batch.n_regions, batch.n_variants, n_labels, n_contigs
    for f, ct in EmuView._fields_:
        if f in k:
            k[f] = np.array(k[f], copy=True, order="C")  # (tests change the view, never the batch)
            setattr(v, f, k[f].ctypes.data_as(ct))
    return v, k


def lists(view, n):
    """the lists the rule gives -> (label_off[n + 1], label_idx), made in the two steps of the kernels: offsets, then indices"""
    off = np.zeros(n + 1, np.uint64)
    assert load().strata_emu_lists(C.byref(view), off.ctypes.data_as(u64p), None) == 0
    idx = np.zeros(int(off[n]) + 1, np.uint32)
    off2 = np.zeros(n + 1, np.uint64)
    assert load().strata_emu_lists(C.byref(view), off2.ctypes.data_as(u64p), idx.ctypes.data_as(u32p)) == 0 and np.array_equal(off, off2)
    return off, idx[:int(off[n])]


# ---- the shared job ---------------------------------------------------------------------------------------------------------------------------------------
NAMES = ("chrA", "chrB", "chrC")
SPAN = 120_000  # the part of each contig the random regions and intervals lie in
TOUCH = (100_000, 100_100)  # the one interval of label e_touch, on chrB


def write_sets(folder, write_text, n_many=4000, extra_labels=0, seed=3):
    """BEDs + strat.tsv under `folder` -> path of the TSV.  Labels (sorted): a_every, b_none, c_nested, d_many, e_touch, f_mid, then x00.. random ones."""
    rng = np.random.default_rng(seed)
    beds = {
        "a_every": [(c, 0, 10_000_000) for c in NAMES],
        # nothing the genome's regions can be in: a chromosome the genome lacks, an interval with e == 0, starts beyond the contig and beyond 2^32
        "b_none": [("chrZ", 0, 10_000_000), ("chrA", 0, 0), ("chrA", 9_000_000, 9_000_100), ("chrB", 5_000_000_000, 5_000_000_100)],
        # one long interval, then short ones that start later and end earlier: only the running maximum of the ends answers for a region behind them
        "c_nested": [("chrA", 1_000, 50_000)] + [("chrA", 2_000 + 40 * k, 2_010 + 40 * k) for k in range(900)] + [("chrC", 500, 90_000), ("chrC", 600, 700), ("chrC", 60_000, 60_010)],
        # thousands of intervals on chrA, ONE on chrB, none on chrC
        "d_many": sorted(("chrA", int(s), int(s) + int(w)) for s, w in zip(rng.integers(0, SPAN, n_many), rng.integers(20, 2_500, n_many))) + [("chrB", 10_000, 70_000)],
        "e_touch": [("chrB",) + TOUCH],
        # intervals that end in the middle of the batch
        "f_mid": [("chrA", 0, 10_000_000), ("chrB", 0, 60_000)],
    }
    for x in range(extra_labels):
        k = 5 + 7 * (x % 40)
        beds["x%02d" % x] = sorted((NAMES[int(c)], int(s), int(s) + int(w)) for c, s, w in zip(rng.integers(0, 3, k), rng.integers(0, SPAN, k), rng.integers(200, 30_000, k)))
    for name, iv in beds.items():
        write_text(os.path.join(folder, name + ".bed"), "".join("%s\t%d\t%d\n" % x for x in iv))
    tsv = os.path.join(folder, "strat.tsv")
    write_text(tsv, "".join("%s\t%s.bed\n" % (n, n) for n in beds))
    return tsv


def _call(pos, ref_len, alt_len=1):
    ref, alt = "A" * ref_len, "C" * alt_len
    return (int(pos), ref, alt, "Snv" if ref_len == alt_len == 1 else ("Deletion" if alt_len == 1 else ("Insertion" if ref_len == 1 else "Indel")), "HomozygousAlternate")


def edge_regions():
    """region dicts for every edge of the rule, on chrB around TOUCH and on chrA / chrC"""
    lo, hi = TOUCH
    R = []

    def reg(contig, truth, query, start=None, end=None):
        calls = truth + query
        s = min(c[0] for c in calls) - 5 if calls else 40_000
        e = max(c[0] + len(c[1]) for c in calls) + 5 if calls else 40_050
        R.append(dict(contig=contig, start=s if start is None else start, end=e if end is None else end, truth=truth, query=query))

    reg(1, [_call(lo, 1)], [_call(lo + 50, 1)])                    # first == start: in
    reg(1, [_call(lo - 1, 1)], [_call(lo + 50, 1)])                # first == start - 1: out
    reg(1, [_call(lo + 10, 1)], [_call(hi - 1, 1)])                # last == end - 1: in
    reg(1, [_call(lo + 10, 1)], [_call(hi, 1)])                    # last == end: out
    reg(1, [_call(lo + 10, 1)], [_call(hi - 3, 3)])                # a deletion that ends at the interval's end: in
    reg(1, [_call(lo + 10, 1)], [_call(hi - 3, 4)])                # ... one base further: out
    reg(1, [], [_call(lo + 20, 1), _call(lo + 30, 2)])             # the truth side empty
    reg(1, [_call(lo + 20, 1), _call(lo + 30, 2)], [])             # the query side empty
    reg(1, [_call(lo + 5, 200), _call(lo + 40, 1)], [])            # the LAST call's end, not the largest end: the 200-base deletion reaches past `hi`, the region is in
    reg(1, [_call(lo + 5, 1), _call(lo + 40, 1)], [_call(lo + 5, 200)])  # here the long call IS a side's last call: out
    reg(1, [], [])                                                 # no calls: no labels
    reg(0, [_call(45_000, 1)], [_call(49_999, 1)])                 # c_nested behind its short intervals: in by the running maximum
    reg(0, [_call(45_000, 1)], [_call(50_000, 1)])                 # ... one base past the long interval: out
    reg(2, [_call(60_002, 1)], [_call(60_005, 1)])                 # chrC: d_many has no intervals there
    reg(2, [_call(89_999, 1)], [])
    return R


def random_regions(n, seed=11, contigs=3):
    rng = np.random.default_rng(seed)
    R = []
    per = [n // contigs + (1 if c < n % contigs else 0) for c in range(contigs)]
    for c in range(contigs):
        for s in sorted(int(x) for x in rng.integers(100, SPAN, per[c])):
            sides = []
            for _ in range(2):
                k = int(rng.integers(0, 4))
                at = s + np.sort(rng.integers(0, 150, k))
                sides.append([_call(int(p), int(rng.integers(1, 31)), 1) for p in at])
            R.append(dict(contig=c, start=s - 10, end=s + 220, truth=sides[0], query=sides[1]))
    return R


def escape_regions():
    """a window over 65,535 bases, and an allele over 255 bases as the LAST call of its side (its a0_len comes from the escape list)"""
    return [dict(contig=0, start=20_000, end=20_000 + 70_000, truth=[_call(20_010, 1), _call(88_000, 1)], query=[_call(20_020, 1)]),
            dict(contig=1, start=30_000, end=31_000, truth=[_call(30_010, 1), _call(30_100, 300)], query=[_call(30_020, 1)]),
            dict(contig=1, start=59_000, end=61_000, truth=[_call(59_100, 1)], query=[_call(59_750, 300)])]  # ends inside / outside f_mid by the long allele alone


def batch_of(regions):
    return RegionBatch.from_regions(sorted(regions, key=lambda r: (r["contig"], r["start"])))


def write_genome(folder, write_text, length=2_000):
    """a FASTA with the three contigs (the rule never reads a base: the contigs only have to exist by name)"""
    path = os.path.join(folder, "g.fa")
    write_text(path, "".join(">%s\n%s\n" % (n, "ACGT" * (length // 4)) for n in NAMES))
    return path
