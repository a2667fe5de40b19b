"""Loader for tests/emu/libmergecount_emu.so: the per-slot rule of the merge summary counters (aardvark_amd/csrc/avk_mergecount.inl) run on the CPU, the host
function it is compared with, and an independent statement of the rule in Python.
Test infrastructure for the GPU-less container; built here, into a library of its own, with the flags of tests/emu/Makefile."""
import ctypes as C
import os
import subprocess

import numpy as np

from aardvark_amd._abi import PackedEscapes
from aardvark_amd.merge import MergeResult, PackedMultiBatch, merge_counts, merge_counts_len

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aardvark_amd", "csrc")
_lib = None
i32p, u8p, u32p, u64p = C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
N_TYPES = 12
DIFFERENT, IDENTICAL, NO_CONFLICT, MAJORITY, CONFLICT_SELECTION = range(5)
ERR_TYPE, ERR_RANGE, ERR_CLASS = 1, 2, 4


class EmuView(C.Structure):
    """mergecount_emu_view of tests/emu/mergecount_emu.cpp"""
    _fields_ = [("n_regions", C.c_uint64), ("n_variants", C.c_uint64), ("k", C.c_uint32), ("status", i32p), ("classification", u8p), ("members", u64p), ("in_off", u64p),
                ("in_cnt", u32p), ("var_type", u8p)]


def load():
    global _lib
    if _lib is None:
        import fcntl
        so = os.path.join(EMU_DIR, "libmergecount_emu.so")
        deps = [os.path.join(EMU_DIR, "mergecount_emu.cpp"), os.path.join(ROOT, "include", "aardvark_amd.h")] + [os.path.join(CSRC, f) for f in (
            "avk_mergecount.inl", "avk_merge_reason.h", "avk_wave.h")]
        with open(os.path.join(EMU_DIR, ".build.lock"), "w") as lock:  # (pytest-xdist workers: one builds, the others wait)
            fcntl.flock(lock, fcntl.LOCK_EX)
            if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
                subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-g", "-std=c++17", "-fPIC", "-Wall", "-Wextra", "-Wno-unused-function", "-Wno-unknown-pragmas",
                                       "-Wno-strict-aliasing", "-pthread", "-shared", "-o", so, "mergecount_emu.cpp"], cwd=EMU_DIR)
        lib = C.CDLL(so)
        lib.mergecount_emu_counts.restype = C.c_uint32
        lib.mergecount_emu_counts.argtypes = [C.POINTER(EmuView), u64p]
        lib.mergecount_emu_reason.restype = C.c_uint32
        lib.mergecount_emu_reason.argtypes = [C.c_uint32, C.c_uint8, C.c_uint64]
        lib.mergecount_emu_words.restype = C.c_uint64
        lib.mergecount_emu_words.argtypes = [C.c_uint32]
        lib.mergecount_emu_fits_lds.argtypes = [C.c_uint32, C.c_uint64]
        _lib = lib
    return _lib


def packed_batch(k, counts, types, zyg=5):
    """a PackedMultiBatch with counts[n * k] calls per slot and the given type nibble per call; counts of 256 and more go to the escape list (their narrow count
    is 0).  Only what the counters read is meaningful: every call is a one-base allele pair at relative position 0."""
    counts = np.asarray(counts, np.int64)
    n, nv = counts.size // k, int(counts.sum())
    assert counts.size == n * k and len(types) == nv
    length, rel, a0, a1 = np.full(n, 10, np.int64), np.zeros(nv, np.int64), np.ones(nv, np.int64), np.ones(nv, np.int64)
    esc = PackedEscapes.build(length, counts, rel, a0, a1)
    narrow = counts.copy()
    narrow[esc.esc_slot.astype(np.int64)] = 0
    return PackedMultiBatch(k, escapes=esc, contig_idx=np.zeros(n), start=np.arange(n) * 20, len=length, in_cnt=narrow, var_rel_pos=rel,
                            var_type_zyg=np.asarray(types, np.uint8) | np.uint8(zyg << 4), a0_len=a0, a1_len=a1, var_raw_space=None,
                            allele_bytes=np.full(max(2 * nv, 1), 65, np.uint8))


def device_view(pmb, status, classification, members):
    """what the device holds behind the classification kernel -> (EmuView, the arrays it points into)"""
    _, cnt, _, _, _ = pmb._wide_fields()
    k = dict(status=np.ascontiguousarray(status, np.int32), classification=np.ascontiguousarray(classification, np.uint8), members=np.ascontiguousarray(members, np.uint64),
             in_off=np.concatenate([[0], np.cumsum(cnt)])[:-1].astype(np.uint64) if cnt.size else np.zeros(1, np.uint64), in_cnt=np.append(cnt, 0).astype(np.uint32),
             var_type=np.append(pmb.var_type_zyg, 0).astype(np.uint8))
    v = EmuView()
    v.n_regions, v.n_variants, v.k = pmb.n_regions, pmb.n_variants, pmb.n_inputs
    for f, ct in EmuView._fields_[3:]:
        k[f] = np.array(k[f], copy=True, order="C")
        setattr(v, f, k[f].ctypes.data_as(ct))
    return v, k


def emu_counts(view, k, out=None):
    """mc_slot over every slot -> (block, error word)"""
    out = np.zeros(int(load().mergecount_emu_words(k)), np.uint64) if out is None else out
    err = load().mergecount_emu_counts(C.byref(view), out.ctypes.data_as(u64p))
    return out, int(err)


def host_counts(lib, pmb, status, classification, members):
    """avk_merge_counts_esc -> block"""
    return merge_counts(lib, pmb, MergeResult(status, classification, members, pmb.n_inputs))


def python_reason(k, classification, members):
    """the reference's derive(Ord) order of the merge reasons, written from merge_summary.rs:12-18 alone: Different, NoConflict by mask, MajorityAgree by mask,
    ConflictSelection by index, BasepairIdentical"""
    order = [("D", 0)] + [("N", m) for m in range(2 ** k)] + [("M", m) for m in range(2 ** k)] + [("C", i) for i in range(k)] + [("I", 0)]
    key = {DIFFERENT: ("D", 0), IDENTICAL: ("I", 0), NO_CONFLICT: ("N", int(members)), MAJORITY: ("M", int(members)), CONFLICT_SELECTION: ("C", int(members))}[int(classification)]
    return order.index(key)


def python_counts(pmb, status, classification, members):
    """add_merge_benchmark (merge_summary.rs:57-81) region by region -> block"""
    k = pmb.n_inputs
    _, cnt, _, _, _ = pmb._wide_fields()
    out = np.zeros((2 + 2 * 2 ** k + k) * N_TYPES * k * 2, np.uint64)
    v = 0
    for r in range(pmb.n_regions):
        cls, mem = int(classification[r]), int(members[r])
        for i in range(k):
            c = int(cnt[r * k + i])
            if int(status[r]) == 0:
                passing = cls == IDENTICAL or (cls == CONFLICT_SELECTION and mem == i) or (cls in (NO_CONFLICT, MAJORITY) and (mem >> i) & 1 == 1)
                reason = python_reason(k, cls, mem)
                for t in (pmb.var_type_zyg[v:v + c] & 15):
                    out[((reason * N_TYPES + int(t)) * k + i) * 2 + (0 if passing else 1)] += 1
            v += c
    return out


def random_results(rng, n, k, unsolved=0.1):
    """status / classification / members as the classification can leave them: every class, masks of every shape, ConflictSelection indices (NOT masks)"""
    status = np.where(rng.random(n) < unsolved, rng.choice([3, 7, 21], n), 0).astype(np.int32)
    cls = rng.integers(0, 5, n).astype(np.uint8)
    members = np.zeros(n, np.uint64)
    for r in range(n):
        if cls[r] in (NO_CONFLICT, MAJORITY):
            members[r] = int(rng.integers(0, 2 ** k))
        elif cls[r] == CONFLICT_SELECTION:
            members[r] = int(rng.integers(0, k))
    return status, cls, members
