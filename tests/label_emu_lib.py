"""Loader for tests/emu/liblabel_emu.so: the per-region rule of the compact stratified tallies (aardvark_amd/csrc/avk_labels.inl) run on the CPU.
Test infrastructure for the GPU-less container; built here, into a library of its own, with the flags of tests/emu/Makefile."""
import ctypes as C
import os
import subprocess

import numpy as np

import aardvark_amd
from aardvark_amd._abi import N_FIELDS, N_GROUPS, TALLY_LEN

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aardvark_amd", "csrc")
WORDS = N_GROUPS * N_FIELDS
_lib = None
u8p, u32p, u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)


class EmuView(C.Structure):
    """label_emu_view of tests/emu/label_emu.cpp"""
    _fields_ = [("n_regions", C.c_uint64), ("n_variants", C.c_uint64), ("t_off", u64p), ("q_off", u64p), ("t_cnt", u32p), ("q_cnt", u32p), ("var_type", u8p), ("var_zyg", u8p),
                ("var_raw", u32p), ("a0_len", u32p), ("a1_len", u32p), ("pk_start", u32p), ("pk_tc", u8p), ("pk_qc", u8p), ("pk_tz", u8p), ("pk_a0", u8p), ("pk_a1", u8p),
                ("pk_voff", u64p), ("alt_ed", u32p), ("region_out", u32p), ("var_out", u32p), ("v_off", u32p), ("bp_off", u32p), ("bp", u32p)]


def load():
    global _lib
    if _lib is None:
        import fcntl
        so = os.path.join(EMU_DIR, "liblabel_emu.so")
        deps = [os.path.join(EMU_DIR, "label_emu.cpp"), os.path.join(ROOT, "include", "aardvark_amd.h")] + [os.path.join(CSRC, f) for f in (
            "avk_labels.inl", "avk_devpack.inl", "avk_pairs.inl", "avk_wave.h", "avk_dev_types.h")]
        with open(os.path.join(EMU_DIR, ".build.lock"), "w") as lock:  # (pytest-xdist workers: one builds, the others wait)
            fcntl.flock(lock, fcntl.LOCK_EX)
            if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
                subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-g", "-std=c++17", "-fPIC", "-Wall", "-Wextra", "-Wno-unused-function", "-Wno-unknown-pragmas",
                                       "-Wno-strict-aliasing", "-pthread", "-shared", "-o", so, "label_emu.cpp"], cwd=EMU_DIR)
        lib = C.CDLL(so)
        lib.label_emu_blocks.argtypes = [C.POINTER(EmuView), u32p]
        lib.label_emu_tally.argtypes = [C.POINTER(EmuView), C.c_uint32, u64p, u32p, C.c_uint32, u64p]
        _lib = lib
    return _lib


def groups_of(batch, r):
    """the groups of region r's block in the order of its compact BASEPAIR groups: the joint one, then 1 + type for its call types in type order"""
    types = set(int(batch.var_type[int(batch.t_off[r]) + i]) for i in range(int(batch.t_cnt[r]))) | set(int(batch.var_type[int(batch.q_off[r]) + i]) for i in range(int(batch.q_cnt[r])))
    return [0] + [1 + t for t in sorted(types)]


def device_view(batch, res, packed_source=False, starved=()):
    """What a run without metric blocks leaves on the device for `batch`, made from the ORACLE's results `res` (status, expected / observed / class / zygosity per
    call, BASEPAIR counters of its blocks) and avk_edit_distance -> (EmuView, the arrays it points into).  packed_source: the calls through the pk_* stand-ins
    (the batch must keep a region's truth calls, then its query calls, one region after the other).  starved: solved regions that the view shows as
    AVK_ST_CAPACITY (21) — what a region that ran out of workspace looks like: its per-call words and groups are there, its status says it does not count."""
    lib = aardvark_amd.load_library()
    n, nv = batch.n_regions, batch.n_variants
    k = {}
    k["t_off"], k["q_off"] = np.ascontiguousarray(batch.t_off, np.uint64), np.ascontiguousarray(batch.q_off, np.uint64)
    k["t_cnt"], k["q_cnt"] = np.ascontiguousarray(batch.t_cnt, np.uint32), np.ascontiguousarray(batch.q_cnt, np.uint32)
    k["var_type"], k["var_zyg"] = np.ascontiguousarray(batch.var_type, np.uint8), np.ascontiguousarray(batch.var_zyg, np.uint8)
    k["var_raw"] = np.ascontiguousarray(batch.var_raw_space, np.uint32)
    k["a0_len"], k["a1_len"] = np.ascontiguousarray(batch.a0_len, np.uint32), np.ascontiguousarray(batch.a1_len, np.uint32)
    arena = bytes(np.asarray(batch.allele_bytes, np.uint8))
    k["alt_ed"] = np.array([lib.avk_edit_distance(arena[int(batch.a0_off[v]):int(batch.a0_off[v]) + int(batch.a0_len[v])], int(batch.a0_len[v]),
                                                  arena[int(batch.a1_off[v]):int(batch.a1_off[v]) + int(batch.a1_len[v])], int(batch.a1_len[v])) for v in range(nv)] + [0], np.uint32)
    region_out = np.zeros((n + 1, 4), np.uint32)
    region_out[:n, 0] = np.asarray(res.status, np.int64).astype(np.uint32)
    for r in starved:
        assert int(res.status[r]) == 0
        region_out[r, 0] = 21
    k["region_out"] = region_out
    calls = k["t_cnt"].astype(np.int64) + k["q_cnt"].astype(np.int64)
    k["v_off"] = np.concatenate([[0], np.cumsum(calls)[:-1]]).astype(np.uint32) if n else np.zeros(1, np.uint32)
    var_out = np.full(int(calls.sum()) + 1, 0xEEEEEEEE, np.uint32)
    bp_off, bp = np.zeros(n + 1, np.uint32), []
    for r in range(n):
        at = int(k["v_off"][r])
        for side_off, side_cnt in ((batch.t_off, batch.t_cnt), (batch.q_off, batch.q_cnt)):
            for i in range(int(side_cnt[r])):
                v = int(side_off[r]) + i
                var_out[at] = int(res.var_expected[v]) | int(res.var_observed[v]) << 8 | int(res.var_class[v]) << 16 | int(res.var_zyg[v]) << 24
                at += 1
        bp_off[r] = len(bp)
        if int(res.status[r]) == 0:  # (the packer gives every region that passes validation its groups; the rule only reads those of solved regions)
            for g in groups_of(batch, r):
                bp.append(res.group_metrics[r][g][14:18])
    bp_off[n] = len(bp)
    k["var_out"], k["bp_off"] = var_out, bp_off
    k["bp"] = np.ascontiguousarray(np.array(bp, np.uint32).reshape(-1)) if bp else np.zeros(4, np.uint32)
    if packed_source:
        assert np.array_equal(k["t_off"][:n], k["v_off"][:n].astype(np.uint64)) and np.array_equal(k["q_off"][:n], k["t_off"][:n] + k["t_cnt"][:n])
        k["pk_start"] = np.zeros(n + 1, np.uint32)
        k["pk_tc"], k["pk_qc"] = k["t_cnt"].astype(np.uint8), k["q_cnt"].astype(np.uint8)
        k["pk_tz"] = (k["var_type"] | (k["var_zyg"] << 4)).astype(np.uint8)
        k["pk_a0"], k["pk_a1"] = k["a0_len"].astype(np.uint8), k["a1_len"].astype(np.uint8)
        assert np.array_equal(k["pk_a0"], k["a0_len"]) and np.array_equal(k["pk_a1"], k["a1_len"]) and np.array_equal(k["pk_tc"], k["t_cnt"])
        k["pk_voff"] = k["t_off"].copy()
        for f in ("t_off", "q_off", "t_cnt", "q_cnt", "var_type", "var_zyg", "a0_len", "a1_len"):  # the wide arrays do not exist for such a batch
            k[f] = None
    view = EmuView()
    view.n_regions, view.n_variants = n, nv
    for f, ct in EmuView._fields_[2:]:
        a = k.get(f)
        if a is not None:
            setattr(view, f, a.ctypes.data_as(ct))
    return view, k


def blocks(view, n):
    """lb_region_groups for every solved region -> [n, 13 * 22] uint32 (unsolved regions stay 0)"""
    out = np.zeros((n, WORDS), np.uint32)
    assert load().label_emu_blocks(C.byref(view), out.ctypes.data_as(u32p)) == 0
    return out


def tally(view, n_labels, off, idx, block, out=None):
    """lb_region_labels over launches of `block` labels -> [n_labels, TALLY_LEN] uint64 (added to `out`)"""
    out = np.zeros((n_labels, TALLY_LEN), np.uint64) if out is None else out
    off = np.ascontiguousarray(off, np.uint64)
    idx = np.ascontiguousarray(idx, np.uint32) if len(idx) else np.zeros(1, np.uint32)
    assert load().label_emu_tally(C.byref(view), n_labels, off.ctypes.data_as(u64p), idx.ctypes.data_as(u32p), block, out.ctypes.data_as(u64p)) == 0
    return out
