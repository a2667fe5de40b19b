"""Shared by the per-call bootstrap tests: a RESTATEMENT of the rule of aardvark_amd/csrc/avk_callboot.h — out[scope][b][key] = sum over the scope's solved regions of
w(r, b) x X_r[key] — with the weights from tests/boot_lib.py's restatement of avk_boot.h and the per-call contributions from tests/kind_lib.py / tests/size_lib.py
on the ORACLE's outputs; no code under test — and the loaders of tests/emu/libcallboot_emu.so (the kernel's lane functions on the CPU, tests/emu/callboot_emu.cpp)
and of the stand-alone programs of tests/native/callboot_check.cpp.  Test infrastructure; built here with the flags of tests/emu/Makefile."""
import ctypes as C
import os

import numpy as np

import boot_lib
import kind_lib
import size_lib
from aardvark_amd._abi import N_GROUPS, AvkSizeSpec

EMU_DIR, ROOT, CSRC, NATIVE_DIR = kind_lib.EMU_DIR, kind_lib.ROOT, kind_lib.CSRC, kind_lib.NATIVE_DIR
KIND = "kind"
KEY_WORDS, BLOCK_BYTES, MAX_BLOCKS = 13 * 14, 1456, 262144
u16p, u32p, u64p = C.POINTER(C.c_uint16), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
_emu = None


def size(edges):
    """the size family under a spec"""
    return ("size", tuple(edges))


def n_keys_of(family):
    return 9 if family == KIND else len(family[1]) + 1


def at(scope, B, b, n_keys, key, g, f):
    """the layout as the issue words it"""
    return (((scope * B + b) * n_keys + key) * 13 + g) * 14 + f


def region_blocks(calls, n_regions, family):
    """X_r for every region: calls (kind_lib.calls_of) -> [n_regions, n_keys, N_GROUPS, 14] uint64"""
    K = n_keys_of(family)
    X = np.zeros((n_regions, K, N_GROUPS, 14), np.uint64)
    for row in calls:
        r, side, vt = int(row[0]), int(row[1]), int(row[2])
        if r >= n_regions:  # (a batch of the first n_regions regions)
            continue
        key = int(row[11]) if family == KIND else size_lib.bin_of(family[1], int(row[3]))
        fields = size_lib.QUERY_F if side else size_lib.TRUTH_F
        for g in (0, 1 + vt):
            if g < N_GROUPS:
                for k in range(7):
                    X[r, key, g, fields[k]] += np.uint64(row[4 + k])
    return X


def expected(calls, n, members, B, seed, family, keys=None, lo=0, hi=None):
    """calls (kind_lib.calls_of: rows of solved regions only), n regions, members [L, n] bool or None, B replicates drawn with `seed`, family (KIND or size(edges)),
    keys = (contig[n], start[n]) — what a weight depends on; the regions [lo, hi) -> [1 + L, B, n_keys, N_GROUPS, 14] uint64"""
    hi = n if hi is None else hi
    contig, start = keys
    w = boot_lib.weights(seed, np.asarray(contig)[:n], np.asarray(start)[:n], np.arange(B))
    inside = (np.arange(n) >= lo) & (np.arange(n) < hi)
    X = region_blocks(calls, n, family).reshape(n, -1)
    scopes = [np.ones(n, bool)] + ([] if members is None else [np.asarray(m, bool)[:n] for m in members])
    out = np.zeros((len(scopes), B, n_keys_of(family), N_GROUPS, 14), np.uint64)
    for s, m in enumerate(scopes):
        ws = w * (m & inside).astype(np.uint64)[:, None]
        out[s] = (ws.T @ X).reshape(out.shape[1:])
    return out


def expected_lists(calls, n, labels, B, seed, family, keys):
    """the host routes' scopes: labels = (n_labels, label_off, label_idx) — a label named twice in a region's list counts twice"""
    L, off, idx = labels
    contig, start = keys
    w = boot_lib.weights(seed, np.asarray(contig)[:n], np.asarray(start)[:n], np.arange(B))
    X = region_blocks(calls, n, family).reshape(n, -1)
    times = np.zeros((1 + L, n), np.uint64)
    times[0] = 1
    for r in range(n):
        for q in range(int(off[r]), int(off[r + 1])):
            times[1 + int(idx[q]), r] += np.uint64(1)
    out = np.zeros((1 + L, B, n_keys_of(family), N_GROUPS, 14), np.uint64)
    for s in range(1 + L):
        out[s] = ((w * times[s][:, None]).T @ X).reshape(out.shape[1:])
    return out


def c_family(family):
    """-> (the header's family number, an AvkSizeSpec or None)"""
    return (1, None) if family == KIND else (0, size_lib.c_spec(list(family[1])))


# ---- the emulator -------------------------------------------------------------------------------------------------------------------------------------
def load():
    global _emu
    if _emu is None:
        deps = [os.path.join(EMU_DIR, "callboot_emu.cpp")] + [os.path.join(CSRC, f) for f in (
            "avk_callboot.inl", "avk_callboot.h", "avk_boot.h", "avk_callkind.inl", "avk_callkind.h", "avk_sizebin.inl", "avk_sizebin.h", "avk_labels.inl", "avk_strata.inl",
            "avk_devpack.inl", "avk_pairs.inl", "avk_wave.h", "avk_dev_types.h")]
        lib = kind_lib._build(os.path.join(EMU_DIR, "libcallboot_emu.so"), "callboot_emu.cpp", deps, EMU_DIR)
        lib.callboot_emu_reps.restype = C.c_uint32
        lib.callboot_emu_reps.argtypes = [C.c_uint32, C.c_uint64]
        lib.callboot_emu_lds_bytes.restype = C.c_uint64
        lib.callboot_emu_lds_bytes.argtypes = [C.c_uint32, C.c_uint32]
        lib.callboot_emu_run.argtypes = [C.POINTER(kind_lib.KindView), u32p, u64p, u16p, u32p, u32p, C.c_uint32, C.c_int, C.POINTER(AvkSizeSpec), C.c_uint64, C.c_uint32,
                                         C.c_uint32, C.c_uint32, C.c_uint32, u64p]
        _emu = lib
    return _emu


def emu_run(view, keys, family, seed, B, R, cap=None, mask=None, n_labels=0, grid=3):
    """every launch of a call on the emulator -> [1 + n_labels, B, n_keys, N_GROUPS, 14]; the view's pk_start decides which key arrays the lanes read"""
    lib = load()
    n = int(view.n_regions)
    contig, start = keys
    out = np.zeros((1 + n_labels, B, n_keys_of(family), N_GROUPS, 14), np.uint64)
    c32, s64 = np.ascontiguousarray(contig, np.uint32), np.ascontiguousarray(start, np.uint64)
    c16, s32 = np.ascontiguousarray(contig, np.uint16), np.ascontiguousarray(start, np.uint32)
    m = None if mask is None else np.ascontiguousarray(mask, np.uint32)
    assert m is None or m.shape == ((n_labels + 31) // 32, n)
    fam, spec = c_family(family)
    rc = lib.callboot_emu_run(C.byref(view), c32.ctypes.data_as(u32p), s64.ctypes.data_as(u64p), c16.ctypes.data_as(u16p), s32.ctypes.data_as(u32p),
                              None if m is None else m.ctypes.data_as(u32p), n_labels, fam, None if spec is None else C.byref(spec), seed, B, R,
                              lib.callboot_emu_recs() if cap is None else cap, grid, out.ctypes.data_as(u64p))
    assert rc == 0
    return out
