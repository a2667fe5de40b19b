"""Loader for tests/emu/libcontext_emu.so: the sequence-context labels of a stratified job (aardvark_amd/csrc/avk_context.inl) run on the CPU, over the
emulator's copy of the reference layout.  Test infrastructure for the GPU-less container; built here, into a library of its own, with the flags of
tests/emu/Makefile."""
import ctypes as C
import os
import subprocess

import numpy as np

from aardvark_amd._abi import AvkContextSpec

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aardvark_amd", "csrc")
_lib = None
u8p, u32p, u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)


class EmuView(C.Structure):
    """context_emu_view of tests/emu/context_emu.cpp"""
    _fields_ = [("n_regions", C.c_uint64), ("n_variants", C.c_uint64), ("contig_idx", u32p), ("start", u64p), ("t_off", u64p), ("q_off", u64p), ("t_cnt", u32p), ("q_cnt", u32p),
                ("var_pos", u64p), ("a0_len", u32p)]


def load():
    global _lib
    if _lib is None:
        import fcntl
        so = os.path.join(EMU_DIR, "libcontext_emu.so")
        deps = [os.path.join(EMU_DIR, "context_emu.cpp"), os.path.join(ROOT, "include", "aardvark_amd.h")] + [os.path.join(CSRC, f) for f in (
            "avk_context.inl", "avk_strata.inl", "avk_devpack.inl", "avk_pairs.inl", "avk_wave.h", "avk_dev_types.h")]
        with open(os.path.join(EMU_DIR, ".build.lock"), "w") as lock:  # (pytest-xdist workers: one builds, the others wait)
            fcntl.flock(lock, fcntl.LOCK_EX)
            if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
                subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-g", "-std=c++17", "-fPIC", "-Wall", "-Wextra", "-Wno-unused-function", "-Wno-unknown-pragmas",
                                       "-Wno-strict-aliasing", "-pthread", "-shared", "-o", so, "context_emu.cpp"], cwd=EMU_DIR)
        lib = C.CDLL(so)
        seqs = C.POINTER(C.c_char_p)
        lib.context_emu_region_bits.argtypes = [C.POINTER(EmuView), seqs, u64p, C.c_uint32, C.POINTER(AvkContextSpec), u32p]
        lib.context_emu_span_bits.argtypes = [seqs, u64p, C.c_uint32, C.POINTER(AvkContextSpec), C.c_uint64, u32p, u64p, u64p, C.c_int, u32p]
        lib.context_emu_counts.argtypes = [seqs, u64p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int, u64p]
        lib.context_emu_place.restype = C.c_uint64
        lib.context_emu_place.argtypes = [u32p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, u32p]
        assert lib.context_emu_spec_size() == C.sizeof(AvkContextSpec)
        _lib = lib
    return _lib


def c_spec(spec):
    """avk_context_spec of a context_lib.Spec"""
    s = AvkContextSpec()
    s.gc_pad, s.n_gc_edges, s.hp_pad, s.n_hp_edges = spec.gc_pad, len(spec.gc_edges), spec.hp_pad, len(spec.hp_edges)
    for i, x in enumerate(spec.gc_edges):
        s.gc_edges[i] = x
    for i, x in enumerate(spec.hp_edges):
        s.hp_edges[i] = x
    return s


def _ref(contigs):
    seqs = (C.c_char_p * len(contigs))(*[bytes(c) for c in contigs])
    lens = np.array([len(c) for c in contigs], np.uint64)
    return seqs, lens


def region_bits(batch, contigs, spec):
    """cx_region_bits of every region of a RegionBatch (its wide arrays) -> uint32[n]"""
    k = dict(contig_idx=np.ascontiguousarray(batch.contig_idx, np.uint32), start=np.ascontiguousarray(batch.start, np.uint64), t_off=np.ascontiguousarray(batch.t_off, np.uint64),
             q_off=np.ascontiguousarray(batch.q_off, np.uint64), t_cnt=np.ascontiguousarray(batch.t_cnt, np.uint32), q_cnt=np.ascontiguousarray(batch.q_cnt, np.uint32),
             var_pos=np.ascontiguousarray(np.append(batch.var_pos, 0), np.uint64), a0_len=np.ascontiguousarray(np.append(batch.a0_len, 0), np.uint32))
    v = EmuView()
    v.n_regions, v.n_variants = batch.n_regions, batch.n_variants
    for f, ct in EmuView._fields_:
        if f in k:
            setattr(v, f, k[f].ctypes.data_as(ct))
    seqs, lens = _ref(contigs)
    bits = np.full(batch.n_regions + 1, 0xABCD, np.uint32)
    s = c_spec(spec)
    assert load().context_emu_region_bits(C.byref(v), seqs, lens.ctypes.data_as(u64p), len(contigs), C.byref(s), bits.ctypes.data_as(u32p)) == 0
    assert bits[-1] == 0xABCD
    return bits[:-1]


def span_bits(contigs, spec, spans, force_bytes=False):
    """cx_span_bits of explicit (contig, first, last) spans -> uint32[len(spans)]"""
    seqs, lens = _ref(contigs)
    contig = np.array([s[0] for s in spans], np.uint32)
    first, last = np.array([s[1] for s in spans], np.uint64), np.array([s[2] for s in spans], np.uint64)
    bits = np.zeros(len(spans) + 1, np.uint32)
    s = c_spec(spec)
    assert load().context_emu_span_bits(seqs, lens.ctypes.data_as(u64p), len(contigs), C.byref(s), len(spans), contig.ctypes.data_as(u32p), first.ctypes.data_as(u64p),
                                        last.ctypes.data_as(u64p), 1 if force_bytes else 0, bits.ctypes.data_as(u32p)) == 0
    return bits[:-1]


def counts(contigs, lo, hi, force_bytes):
    """(a, g, longest run) of the window [lo, hi) of the concatenated reference, by the 2-bit route (flagged words from the bytes) or by the bytes alone"""
    seqs, lens = _ref(contigs)
    out = np.zeros(3, np.uint64)
    assert load().context_emu_counts(seqs, lens.ctypes.data_as(u64p), len(contigs), lo, hi, 1 if force_bytes else 0, out.ctypes.data_as(u64p)) == 0
    return tuple(int(x) for x in out)


def place(bits, n_bed, n_ctx, mask, fresh):
    """the context kernel's stores into word-major masks [n_words, n] (changed in place) -> the number of context hits"""
    bits = np.ascontiguousarray(bits, np.uint32)
    assert mask.dtype == np.uint32 and mask.flags.c_contiguous and mask.shape[1] == len(bits)
    return int(load().context_emu_place(bits.ctypes.data_as(u32p), len(bits), n_bed, n_ctx, 1 if fresh else 0, mask.ctypes.data_as(u32p)))
