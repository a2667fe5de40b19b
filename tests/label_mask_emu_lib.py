"""Loader for tests/emu/liblabel_mask_emu.so: the stratified tally that reads a region's labels from bit masks (lb_region_labels_mask of
aardvark_amd/csrc/avk_labels.inl) and the tally over lists made from the same masks (sx_fill_region of avk_strata.inl, lb_region_labels), run on the CPU.
Test infrastructure for the GPU-less container; built here, into a library of its own, with the flags of tests/emu/Makefile."""
import ctypes as C
import os
import subprocess

import numpy as np

import label_emu_lib
from label_emu_lib import WORDS, EmuView  # (the device view is label_emu.cpp's, field for field)

EMU_DIR = label_emu_lib.EMU_DIR
ROOT = label_emu_lib.ROOT
CSRC = label_emu_lib.CSRC
_lib = None
u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)


def load():
    global _lib
    if _lib is None:
        import fcntl
        so = os.path.join(EMU_DIR, "liblabel_mask_emu.so")
        deps = [os.path.join(EMU_DIR, "label_mask_emu.cpp"), os.path.join(ROOT, "include", "aardvark_amd.h")] + [os.path.join(CSRC, f) for f in (
            "avk_labels.inl", "avk_strata.inl", "avk_devpack.inl", "avk_pairs.inl", "avk_wave.h", "avk_dev_types.h")]
        with open(os.path.join(EMU_DIR, ".build.lock"), "w") as lock:  # (pytest-xdist workers: one builds, the others wait)
            fcntl.flock(lock, fcntl.LOCK_EX)
            if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
                subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-g", "-std=c++17", "-fPIC", "-Wall", "-Wextra", "-Wno-unused-function", "-Wno-unknown-pragmas",
                                       "-Wno-strict-aliasing", "-pthread", "-shared", "-o", so, "label_mask_emu.cpp"], cwd=EMU_DIR)
        lib = C.CDLL(so)
        lib.label_mask_emu_block_max.restype = C.c_int
        lib.label_mask_emu_lists.argtypes = [u32p, C.c_uint64, C.c_uint32, u64p, u32p]
        lib.label_mask_emu_block.argtypes = [C.POINTER(EmuView), u32p, u64p, u32p, C.c_uint32, C.c_uint32, u64p]
        _lib = lib
    return _lib


def n_words(n_labels):
    return (n_labels + 31) // 32


def masks_of_lists(n, n_labels, off, idx):
    """word-major masks [n_words * n] (mask[w * n + r], the strata mask pass's layout) of lists"""
    mask = np.zeros((n_words(n_labels), n), np.uint32)
    region = np.repeat(np.arange(n), np.diff(np.asarray(off).astype(np.int64)))
    np.bitwise_or.at(mask, (np.asarray(idx) >> 5, region), np.uint32(1) << (np.asarray(idx, np.uint32) & np.uint32(31)))
    return mask


def lists_of_masks(mask, n, n_labels):
    """sx_fill_region's lists of word-major masks -> (label_off[n + 1], label_idx)"""
    mask = np.ascontiguousarray(mask, np.uint32).reshape(-1)
    off = np.zeros(n + 1, np.uint64)
    assert load().label_mask_emu_lists(mask.ctypes.data_as(u32p), n, n_words(n_labels), off.ctypes.data_as(u64p), None) == 0
    idx = np.zeros(int(off[n]) + 1, np.uint32)
    assert load().label_mask_emu_lists(mask.ctypes.data_as(u32p), n, n_words(n_labels), off.ctypes.data_as(u64p), idx.ctypes.data_as(u32p)) == 0
    return off, idx[:int(off[n])]


def block_from_masks(view, mask, lo, hi):
    """lb_region_labels_mask over every region for the block [lo, hi) -> the launch's accumulator [(hi - lo) * 13 * 22] uint64"""
    mask = np.ascontiguousarray(mask, np.uint32).reshape(-1)
    acc = np.full((hi - lo) * WORDS + 1, 0xABCD, np.uint64)
    assert load().label_mask_emu_block(C.byref(view), mask.ctypes.data_as(u32p), None, None, lo, hi, acc.ctypes.data_as(u64p)) == 0
    assert acc[-1] == 0xABCD
    return acc[:-1]


def block_from_lists(view, off, idx, lo, hi):
    """lb_region_labels over every region for the block [lo, hi) -> the launch's accumulator"""
    off = np.ascontiguousarray(off, np.uint64)
    idx = np.ascontiguousarray(idx, np.uint32) if len(idx) else np.zeros(1, np.uint32)
    acc = np.full((hi - lo) * WORDS + 1, 0xABCD, np.uint64)
    assert load().label_mask_emu_block(C.byref(view), None, off.ctypes.data_as(u64p), idx.ctypes.data_as(u32p), lo, hi, acc.ctypes.data_as(u64p)) == 0
    assert acc[-1] == 0xABCD
    return acc[:-1]
