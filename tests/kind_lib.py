"""Shared by the call-kind tests: a RESTATEMENT of the rule of aardvark_amd/csrc/avk_callkind.h in numpy and plain Python — the kind from the batch's input
zygosity and allele bytes, alt_ed as size_lib's textbook table, the per-call contribution from the ORACLE's var_expected / var_observed / status (size_lib.calls_of,
by import), membership from given region lists; no code under test — the fixture every kind test shares, and the loaders of tests/emu/libkind_emu.so (the kernel's
wave code on the CPU, tests/emu/kind_emu.cpp) and tests/native/libkind_check.so (the header's functions, tests/native/kind_check.cpp).  Test infrastructure; built
here, into libraries of their own, with the flags of tests/emu/Makefile."""
import ctypes as C
import os
import subprocess

import numpy as np

import label_emu_lib
import size_lib
from aardvark_amd._abi import N_GROUPS, RegionBatch

EMU_DIR, ROOT, CSRC = label_emu_lib.EMU_DIR, label_emu_lib.ROOT, label_emu_lib.CSRC
NATIVE_DIR = os.path.join(ROOT, "tests", "native")
N_KINDS = 9
NAMES = ["het_ts", "het_tv", "het_other", "hom_ts", "hom_tv", "hom_other", "nogt_ts", "nogt_tv", "nogt_other"]
TRUTH_F, QUERY_F = size_lib.TRUTH_F, size_lib.QUERY_F
u8p, u32p, u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
_emu = _check = None


# ---- the rule, restated -----------------------------------------------------------------------------------------------------------------------------
def gt_of(zyg):
    """0 het: UnphasedHeterozygous 2, PhasedHet01 3, PhasedHet10 4; 1 hom: HomozygousAlternate 5; 2 nogt: anything else"""
    return 0 if zyg in (2, 3, 4) else 1 if zyg == 5 else 2


def sub_of(a0, a1):
    """a0, a1: the two alleles as bytes -> 0 ts, 1 tv, 2 other"""
    if len(a0) != 1 or len(a1) != 1:
        return 2
    x, y = chr(a0[0] & 0xDF), chr(a1[0] & 0xDF)
    if x not in "ACGT" or y not in "ACGT" or x == y:
        return 2
    return 0 if {x, y} in ({"A", "G"}, {"C", "T"}) else 1


def kinds_of(batch):
    """the kind of every call of the batch, [n_variants]; an allele offset outside the allele array makes the call `other`"""
    arena = bytes(np.asarray(batch.allele_bytes, np.uint8))
    out = np.zeros(batch.n_variants, np.int64)
    for v in range(batch.n_variants):
        o0, l0, o1, l1 = int(batch.a0_off[v]), int(batch.a0_len[v]), int(batch.a1_off[v]), int(batch.a1_len[v])
        inside = o0 < len(arena) and o1 < len(arena)
        out[v] = 3 * gt_of(int(batch.var_zyg[v])) + (sub_of(arena[o0:o0 + l0], arena[o1:o1 + l1]) if inside else 2)
    return out


def call_ids(batch, res):
    """the call index of every row of size_lib.calls_of, in its order"""
    ids = []
    for r in range(batch.n_regions):
        if int(res.status[r]) != 0:
            continue
        for off, cnt in ((batch.t_off, batch.t_cnt), (batch.q_off, batch.q_cnt)):
            ids.extend(int(off[r]) + i for i in range(int(cnt[r])))
    return np.array(ids, np.int64)


def calls_of(batch, res, alt_ed=None):
    """one row per call of a solved region: (region, side, type, size, the seven values, kind, call index) — size_lib.calls_of with two more columns"""
    rows, ids = size_lib.calls_of(batch, res, alt_ed), call_ids(batch, res)
    assert len(rows) == len(ids)
    return np.concatenate([rows, kinds_of(batch)[ids].reshape(-1, 1), ids.reshape(-1, 1)], axis=1)


def expected(calls, n_regions, members=None, lo=0, hi=None):
    """calls (calls_of), the regions [lo, hi), members [L, n_regions] bool or None -> [1 + L, 9, N_GROUPS, 14] uint64"""
    hi = n_regions if hi is None else hi
    scopes = [np.ones(n_regions, bool)] + ([] if members is None else [np.asarray(m, bool) for m in members])
    out = np.zeros((len(scopes), N_KINDS, N_GROUPS, 14), np.uint64)
    for row in calls:
        r, side, vt, kind = int(row[0]), int(row[1]), int(row[2]), int(row[11])
        if not lo <= r < hi:
            continue
        fields = QUERY_F if side else TRUTH_F
        for s, m in enumerate(scopes):
            if m[r]:
                for g in (0, 1 + vt):
                    for k in range(7):
                        out[s, kind, g, fields[k]] += np.uint64(row[4 + k])
    return out


# ---- the fixture ----------------------------------------------------------------------------------------------------------------------------------------
def hand_regions(contig):
    """hand-written regions on the first contig (bytes): a lower-case transition a -> g, a mixed-case transversion C -> a, an N ALT, a 1-base call whose bases are
    equal after folding (a -> A), a 2/2-base substitution typed Indel, a call of unknown zygosity -> (regions, {name: index of the region})"""
    def find(seq, at):
        p = contig.find(seq, at)
        assert p > 100
        return p
    pa, pc = find(b"A", 200_000), find(b"C", 210_000)
    pn, pe, p2, pu = find(b"G", 220_000), find(b"A", 230_000), find(b"AC", 240_000), find(b"T", 250_000)
    hom, het = "HomozygousAlternate", "UnphasedHeterozygous"
    reg = lambda p, t, q: {"start": p - 20, "end": p + 25, "truth": t, "query": q}
    regions = [
        reg(pa, [(pa, b"a", b"g", "Snv", hom)], [(pa, b"a", b"g", "Snv", het)]),
        reg(pc, [(pc, b"C", b"a", "Snv", het)], [(pc, b"C", b"a", "Snv", het)]),
        reg(pn, [(pn, b"G", b"N", "Snv", hom)], [(pn, b"G", b"T", "Snv", hom)]),
        reg(pe, [(pe, b"a", b"A", "Snv", hom)], [(pe, b"A", b"C", "Snv", hom)]),
        reg(p2, [(p2, b"AC", b"GT", "Indel", hom)], [(p2, b"AC", b"GT", "Indel", het)]),
        reg(pu, [(pu, b"T", b"C", "Snv", "Unknown")], [(pu, b"T", b"C", "Snv", hom)]),
    ]
    return regions, dict(lower=0, mixed=1, n_alt=2, folded=3, two_two=4, unknown=5)


def build_case(oracle, threads=8):
    """scenarios.indel_small(1500) (82 % SNVs with random ALT bases and zygosity), the invalid regions (unsolved), the injected long alleles, the hand-written regions;
    the oracle's results; the fixture's adequacy on the ORACLE's output alone, before anything under test runs.

    No nogt_* kind reaches a sum through this fixture: the oracle refuses every region that holds a call of a zygosity outside het / hom — Unknown (the hand-written
    region `unknown` here and the region of scenarios.invalid_regions), HomozygousReference (it panics, scenarios.invalid_regions) — and an unsolved region adds
    nothing by the rule.  The values 6 and 7 name no zygosity.  So the nogt rows of a block are zero wherever the reference solves, and what maps a zygosity to nogt
    is checked on the header (tests/test_kind_rule.py: every value 0 to 7); the nogt rows' addressing in the wave code and the host route is checked with a
    synthetic batch, the fixture's with zygosities replaced under the oracle's results (test_nogt_rows_from_a_synthetic_batch in test_kind_emu and test_kind_native)."""
    import escapes_lib
    import oracle_lib
    import scenarios
    from aardvark_amd import synth
    contigs, base = scenarios.indel_small(1500)
    _, bad = scenarios.invalid_regions()
    contig = np.asarray(contigs[0]).tobytes() if not isinstance(contigs[0], bytes) else contigs[0]
    regions, where = hand_regions(contig)
    hand = RegionBatch.from_regions(regions)
    plain = synth.concat_batches([base, bad, hand])  # (packs without escapes)
    plain.region_id = np.arange(plain.n_regions).astype(np.uint64)
    hand_first = base.n_regions + bad.n_regions
    batch = escapes_lib.with_injections(contigs, plain)
    want = oracle_lib.compare_batch(oracle, batch, contigs, threads=threads)
    solved = np.asarray(want.status) == 0
    calls = calls_of(batch, want)
    kind, truth, query, wrong = calls[:, 11], calls[:, 1] == 0, calls[:, 1] == 1, calls[:, 5] == 1
    for k in range(6):
        assert (truth & (kind == k)).any() and (query & (kind == k)).any(), "%s holds a truth call and a query call" % NAMES[k]
    for k in (0, 1, 3, 4):
        assert (wrong & (kind == k)).any(), "%s holds a call with expected != observed" % NAMES[k]
    assert (truth & (calls[:, 6] == 1)).any(), "a kind holds a FN with observed > 0"
    for name in ("lower", "n_alt", "folded"):
        assert solved[hand_first + where[name]], "the %s call lies in a solved region" % name
    assert (~solved).any() and solved.sum() > 500
    # what the hand-written calls are, by the rule as the issue words it
    first = lambda name: int(batch.t_off[hand_first + where[name]])
    by_hand = kinds_of(batch)
    assert by_hand[first("lower")] == 3 and by_hand[first("lower") + 1] == 0 and by_hand[first("mixed")] == 1 and by_hand[first("n_alt")] == 5
    assert by_hand[first("folded")] == 5 and by_hand[first("two_two")] == 5 and by_hand[first("unknown")] == 6
    return dict(contigs=contigs, batch=batch, plain=plain, want=want, solved=solved, calls=calls, hand_first=hand_first, where=where)


# ---- the emulator -------------------------------------------------------------------------------------------------------------------------------------
class KindView(C.Structure):
    """kind_emu_view of tests/emu/kind_emu.cpp: label_emu_lib.EmuView, then what the kind needs of the allele bytes"""
    _fields_ = label_emu_lib.EmuView._fields_ + [("a0_off", u64p), ("a1_off", u64p), ("pk_aoff", u64p), ("alleles", u8p), ("alleles_len", C.c_uint64)]


def device_view(batch, res, packed_source=False, starved=()):
    """label_emu_lib.device_view with the allele bytes and their offsets (packed_source: one running offset, allele 1 behind allele 0)"""
    base, keep = label_emu_lib.device_view(batch, res, packed_source=packed_source, starved=starved)
    view = KindView()
    for f, _ in label_emu_lib.EmuView._fields_:
        setattr(view, f, getattr(base, f))
    keep["alleles"] = np.ascontiguousarray(batch.allele_bytes, np.uint8)
    view.alleles, view.alleles_len = keep["alleles"].ctypes.data_as(u8p), keep["alleles"].size
    if packed_source:
        assert np.array_equal(batch.a1_off, batch.a0_off + batch.a0_len.astype(np.uint64))
        keep["pk_aoff"] = np.ascontiguousarray(batch.a0_off, np.uint64)
        view.pk_aoff = keep["pk_aoff"].ctypes.data_as(u64p)
    else:
        keep["a0_off"], keep["a1_off"] = np.ascontiguousarray(batch.a0_off, np.uint64), np.ascontiguousarray(batch.a1_off, np.uint64)
        view.a0_off, view.a1_off = keep["a0_off"].ctypes.data_as(u64p), keep["a1_off"].ctypes.data_as(u64p)
    return view, keep


def _build(so, src, deps, cwd):
    import fcntl
    with open(os.path.join(EMU_DIR, ".build.lock"), "w") as lock:  # (pytest-xdist workers: one builds, the others wait)
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
            subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-g", "-std=c++17", "-fPIC", "-Wall", "-Wextra", "-Wno-unused-function", "-Wno-unknown-pragmas",
                                   "-Wno-strict-aliasing", "-pthread", "-shared", "-o", so, src], cwd=cwd)
    return C.CDLL(so)


def load():
    global _emu
    if _emu is None:
        deps = [os.path.join(EMU_DIR, "kind_emu.cpp"), os.path.join(EMU_DIR, "wave_threads.h")] + [os.path.join(CSRC, f) for f in (
            "avk_callkind.inl", "avk_callkind.h", "avk_sizebin.inl", "avk_sizebin.h", "avk_labels.inl", "avk_strata.inl", "avk_devpack.inl", "avk_pairs.inl", "avk_wave.h",
            "avk_dev_types.h")]
        lib = _build(os.path.join(EMU_DIR, "libkind_emu.so"), "kind_emu.cpp", deps, EMU_DIR)
        lib.kind_emu_run.argtypes = [C.POINTER(KindView), u32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, u64p]
        _emu = lib
    return _emu


def load_check():
    """tests/native/kind_check.cpp: the functions of avk_callkind.h behind a C interface"""
    global _check
    if _check is None:
        deps = [os.path.join(NATIVE_DIR, "kind_check.cpp"), os.path.join(CSRC, "avk_callkind.h"), os.path.join(CSRC, "avk_sizebin.h")]
        lib = _build(os.path.join(NATIVE_DIR, "libkind_check.so"), "kind_check.cpp", deps, NATIVE_DIR)
        lib.kind_check_gt.restype = lib.kind_check_sub.restype = lib.kind_check_kind.restype = lib.kind_check_field.restype = C.c_uint32
        lib.kind_check_gt.argtypes = [C.c_uint32]
        lib.kind_check_sub.argtypes = [C.c_uint32] * 4
        lib.kind_check_kind.argtypes = [C.c_uint32] * 2
        lib.kind_check_field.argtypes = [C.c_uint32, C.c_int]
        lib.kind_check_name.restype = C.c_char_p
        lib.kind_check_name.argtypes = [C.c_uint32]
        lib.kind_check_pairs.argtypes = [u8p]
        _check = lib
    return _check


def emu_run(view, mask=None, n_labels=0, grid=3, scope_lo=0, scope_hi=None):
    """the launches of a call on the emulator -> [1 + n_labels, 9, N_GROUPS, 14]; scope_lo, scope_hi: only the launches of these scopes, the first of which starts at
    scope_lo (the words of the other scopes stay 0)"""
    n = int(view.n_regions)
    out = np.zeros((1 + n_labels, N_KINDS, N_GROUPS, 14), np.uint64)
    m = None if mask is None else np.ascontiguousarray(mask, np.uint32)
    assert m is None or m.shape == ((n_labels + 31) // 32, n)
    hi = 1 + (n_labels if m is not None else 0) if scope_hi is None else scope_hi
    rc = load().kind_emu_run(C.byref(view), None if m is None else m.ctypes.data_as(u32p), n_labels, grid, scope_lo, hi, out.ctypes.data_as(u64p))
    assert rc == 0
    return out
