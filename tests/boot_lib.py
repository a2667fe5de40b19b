"""Shared by the bootstrap tests: a RESTATEMENT of the rule of aardvark_amd/csrc/avk_boot.h in numpy (uint64 mixing, thresholds recomputed with `decimal` at 50
digits — no code under test), the expectation built from the ORACLE's per-region blocks with it, and the loader of tests/emu/libboot_emu.so (the kernel's lane
functions on the CPU, tests/emu/boot_emu.cpp).  Test infrastructure; built here, into a library of its own, with the flags of tests/emu/Makefile."""
import ctypes as C
import os
import subprocess
from decimal import ROUND_FLOOR, Decimal, getcontext

import numpy as np

import label_emu_lib
from aardvark_amd._abi import TALLY_LEN

EMU_DIR = label_emu_lib.EMU_DIR
ROOT, CSRC = label_emu_lib.ROOT, label_emu_lib.CSRC
WORDS = label_emu_lib.WORDS
SOLVED, ERRORS = WORDS, WORDS + 1
u16p, u32p, u64p = C.POINTER(C.c_uint16), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
_lib = None


# ---- the rule, restated -----------------------------------------------------------------------------------------------------------------------------
def thresholds():
    """T[k] = floor(2^32 * sum_{j <= k} e^-1 / j!), k = 0 .. 11"""
    getcontext().prec = 50
    e1, s, f, out = Decimal(-1).exp(), Decimal(0), Decimal(1), []
    for k in range(12):
        if k:
            f *= k
        s += e1 / f
        out.append(int((s * Decimal(2 ** 32)).to_integral_value(rounding=ROUND_FLOOR)))
    return out


def mix(x):
    """splitmix64's finaliser on a uint64 array (wraps)"""
    x = np.array(x, np.uint64)
    x ^= x >> np.uint64(30)
    x *= np.uint64(0xBF58476D1CE4E5B9)
    x ^= x >> np.uint64(27)
    x *= np.uint64(0x94D049BB133111EB)
    x ^= x >> np.uint64(31)
    return x


def weights(seed, contig, start, bs):
    """w(r, b) for regions keyed by (contig[r], start[r]) and the replicates `bs` -> [n, len(bs)] uint64"""
    key = (np.asarray(contig, np.uint64) << np.uint64(32)) | (np.asarray(start, np.uint64) & np.uint64(0xFFFFFFFF))
    h = mix(key ^ mix(np.array([seed & 0xFFFFFFFFFFFFFFFF], np.uint64))[0])
    u = mix(h[:, None] + np.asarray(bs, np.uint64)[None, :]) >> np.uint64(32)
    w = np.zeros(u.shape, np.uint64)
    for t in thresholds():
        w += (u >= np.uint64(t)).astype(np.uint64)
    return w


def expected(blocks, solved, w, members=None):
    """blocks [n, 286] (the oracle's), solved [n] bool, w [n, B], members [L, n] bool or None -> [1 + L, B, TALLY_LEN] uint64"""
    n, B = w.shape
    blocks = np.asarray(blocks).reshape(n, WORDS).astype(np.uint64)
    scopes = [np.ones(n, bool)] + ([] if members is None else [np.asarray(m, bool) for m in members])
    out = np.zeros((len(scopes), B, TALLY_LEN), np.uint64)
    for s, m in enumerate(scopes):
        ws = w * (m & np.asarray(solved, bool)).astype(np.uint64)[:, None]
        out[s, :, :WORDS] = ws.T @ blocks
        out[s, :, SOLVED] = ws.sum(axis=0)
    return out


def members_of_mask(mask, n, n_labels):
    """word-major masks (sx_mask_at's layout) -> [n_labels, n] bool"""
    return np.array([(mask[l >> 5, :n] >> np.uint32(l & 31)) & np.uint32(1) for l in range(n_labels)], bool).reshape(n_labels, n)


def mask_of_members(members, n):
    L = len(members)
    mask = np.zeros((max((L + 31) // 32, 1), n), np.uint32)
    for l, m in enumerate(members):
        mask[l >> 5] |= np.asarray(m, bool).astype(np.uint32) << np.uint32(l & 31)
    return mask


# ---- the emulator -------------------------------------------------------------------------------------------------------------------------------------
def load():
    global _lib
    if _lib is None:
        import fcntl
        so = os.path.join(EMU_DIR, "libboot_emu.so")
        deps = [os.path.join(EMU_DIR, "boot_emu.cpp")] + [os.path.join(CSRC, f) for f in (
            "avk_boot.inl", "avk_boot.h", "avk_labels.inl", "avk_strata.inl", "avk_devpack.inl", "avk_pairs.inl", "avk_wave.h", "avk_dev_types.h")]
        with open(os.path.join(EMU_DIR, ".build.lock"), "w") as lock:  # (pytest-xdist workers: one builds, the others wait)
            fcntl.flock(lock, fcntl.LOCK_EX)
            if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
                subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-g", "-std=c++17", "-fPIC", "-Wall", "-Wextra", "-Wno-unused-function", "-Wno-unknown-pragmas",
                                       "-Wno-strict-aliasing", "-pthread", "-shared", "-o", so, "boot_emu.cpp"], cwd=EMU_DIR)
        lib = C.CDLL(so)
        lib.boot_emu_weight.restype = C.c_uint32
        lib.boot_emu_weight.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32]
        lib.boot_emu_threshold.restype = C.c_uint32
        lib.boot_emu_threshold.argtypes = [C.c_int]
        lib.boot_emu_run.argtypes = [C.POINTER(label_emu_lib.EmuView), u32p, u64p, u16p, u32p, u32p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, u64p]
        _lib = lib
    return _lib


def emu_run(view, contig, start, seed, B, mask=None, n_labels=0, grid=3):
    """every launch of a call on the emulator -> [1 + n_labels, B, TALLY_LEN]; the view's pk_start decides which key arrays the lanes read"""
    n = int(view.n_regions)
    out = np.zeros((1 + n_labels, B, TALLY_LEN), np.uint64)
    c32, s64 = np.ascontiguousarray(contig, np.uint32), np.ascontiguousarray(start, np.uint64)
    c16, s32 = np.ascontiguousarray(contig, np.uint16), np.ascontiguousarray(start, np.uint32)
    m = None if mask is None else np.ascontiguousarray(mask, np.uint32)
    assert m is None or m.shape == ((n_labels + 31) // 32, n)
    rc = load().boot_emu_run(C.byref(view), c32.ctypes.data_as(u32p), s64.ctypes.data_as(u64p), c16.ctypes.data_as(u16p), s32.ctypes.data_as(u32p),
                             None if m is None else m.ctypes.data_as(u32p), n_labels, seed, B, grid, out.ctypes.data_as(u64p))
    assert rc == 0
    return out
