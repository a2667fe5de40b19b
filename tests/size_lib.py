"""Shared by the size-bin tests: a RESTATEMENT of the rule of aardvark_amd/csrc/avk_sizebin.h in numpy and plain Python — size and bin from the batch's allele
lengths, alt_ed as a textbook edit-distance table over the two alleles, the per-call contribution from the ORACLE's var_expected / var_observed / status,
membership from given region lists; no code under test — and the loader of tests/emu/libsize_emu.so (the kernel's wave code on the CPU, tests/emu/size_emu.cpp).
Test infrastructure; built here, into a library of its own, with the flags of tests/emu/Makefile."""
import ctypes as C
import os
import subprocess

import numpy as np

import label_emu_lib
from aardvark_amd._abi import FIELDS, N_FIELDS, N_GROUPS, AvkSizeSpec

EMU_DIR = label_emu_lib.EMU_DIR
ROOT, CSRC = label_emu_lib.ROOT, label_emu_lib.CSRC
N_SIZE_FIELDS = 14
DEFAULT = (1, 6, 16, 50)
FIFTEEN = (1, 2, 3, 4, 5, 6, 8, 11, 16, 21, 31, 50, 100, 1000, 5000)
EDGE_SETS = [(2,), DEFAULT, FIFTEEN]  # the three edge counts: 1, 4 and 15
u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
# where the seven values of a contribution (gt_tp, gt_fn, gt_fn_gt, hap_tp, hap_fn, w_tp, w_fn) land, by the fields' names
TRUTH_F = [FIELDS.index(f) for f in ("GT_TRUTH_TP", "GT_TRUTH_FN", "GT_TRUTH_FN_GT", "HAP_TRUTH_TP", "HAP_TRUTH_FN", "WHAP_TRUTH_TP", "WHAP_TRUTH_FN")]
QUERY_F = [FIELDS.index(f) for f in ("GT_QUERY_TP", "GT_QUERY_FP", "GT_QUERY_FP_GT", "HAP_QUERY_TP", "HAP_QUERY_FP", "WHAP_QUERY_TP", "WHAP_QUERY_FP")]
assert max(TRUTH_F + QUERY_F) == N_SIZE_FIELDS - 1
_lib = None


# ---- the rule, restated -----------------------------------------------------------------------------------------------------------------------------
def bin_of(edges, size):
    """bin 0: size < edges[0]; bin j: edges[j - 1] <= size < edges[j]; the last bin: size >= edges[-1]"""
    for j, e in enumerate(edges):
        if size < e:
            return j
    return len(edges)


def names_of(edges):
    out = []
    for j in range(len(edges) + 1):
        lo = 0 if j == 0 else edges[j - 1]
        if j == len(edges):
            out.append("len_ge%d" % lo)
        elif edges[j] - 1 == lo:
            out.append("len_%d" % lo)
        else:
            out.append("len_%d_%d" % (lo, edges[j] - 1))
    return out


def valid(edges):
    return 1 <= len(edges) <= 15 and edges[0] >= 1 and all(a < b for a, b in zip(edges, edges[1:]))


def edit_distance(a, b):
    """the textbook table: insertions, deletions and substitutions cost 1"""
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y)))
        prev = cur
    return prev[len(b)]


def alt_eds(batch):
    arena = bytes(np.asarray(batch.allele_bytes, np.uint8))
    out = np.zeros(batch.n_variants, np.int64)
    for v in range(batch.n_variants):
        o0, l0, o1, l1 = int(batch.a0_off[v]), int(batch.a0_len[v]), int(batch.a1_off[v]), int(batch.a1_len[v])
        out[v] = edit_distance(arena[o0:o0 + l0], arena[o1:o1 + l1])
    return out


def calls_of(batch, res, alt_ed=None):
    """one row per call of a solved region: (region, side, type, size, the seven values) — the contribution of avk_sizebin.h, values as 32-bit words"""
    alt_ed = alt_eds(batch) if alt_ed is None else alt_ed
    rows = []
    M = 0xFFFFFFFF
    for r in range(batch.n_regions):
        if int(res.status[r]) != 0:
            continue
        for side, off, cnt in ((0, batch.t_off, batch.t_cnt), (1, batch.q_off, batch.q_cnt)):
            for i in range(int(cnt[r])):
                v = int(off[r]) + i
                ea, oa = int(res.var_expected[v]), int(res.var_observed[v])
                exp, obs = (oa, ea) if side else (ea, oa)  # the query entries are stored toggled
                d = (exp - obs) & M
                w = int(alt_ed[v])
                vals = (int(exp == obs), int(exp != obs), int(exp != obs and obs > 0), obs, d, (obs * w) & M, (d * w) & M)
                rows.append((r, side, int(batch.var_type[v]), abs(int(batch.a1_len[v]) - int(batch.a0_len[v]))) + vals)
    return np.array(rows, np.int64).reshape(-1, 11)


def expected(calls, edges, n_regions, members=None, lo=0, hi=None):
    """calls (calls_of), the regions [lo, hi), members [L, n_regions] bool or None -> [1 + L, n_bins, N_GROUPS, 14] uint64"""
    hi = n_regions if hi is None else hi
    scopes = [np.ones(n_regions, bool)] + ([] if members is None else [np.asarray(m, bool) for m in members])
    out = np.zeros((len(scopes), len(edges) + 1, N_GROUPS, N_SIZE_FIELDS), np.uint64)
    for row in calls:
        r, side, vt, size = (int(x) for x in row[:4])
        if not lo <= r < hi:
            continue
        b, fields = bin_of(edges, size), QUERY_F if side else TRUTH_F
        for s, m in enumerate(scopes):
            if m[r]:
                for g in (0, 1 + vt):
                    for k in range(7):
                        out[s, b, g, fields[k]] += np.uint64(row[4 + k])
    return out


def members_of_lists(off, idx, n_labels, n):
    members = np.zeros((n_labels, n), bool)
    members[np.asarray(idx, np.int64), np.repeat(np.arange(n), np.diff(np.asarray(off).astype(np.int64)))] = True
    return members


def mask_of_members(members, n):
    L = len(members)
    mask = np.zeros((max((L + 31) // 32, 1), n), np.uint32)
    for l, m in enumerate(members):
        mask[l >> 5] |= np.asarray(m, bool).astype(np.uint32) << np.uint32(l & 31)
    return mask


def tally14(tally):
    """[.., TALLY_LEN] -> [.., N_GROUPS, 14]: the words of a tally the conservation law speaks of"""
    t = np.asarray(tally, np.uint64)
    return t[..., :N_GROUPS * N_FIELDS].reshape(t.shape[:-1] + (N_GROUPS, N_FIELDS))[..., :N_SIZE_FIELDS]


def c_spec(edges, n_edges=None):
    s = AvkSizeSpec()
    s.n_edges = len(edges) if n_edges is None else n_edges
    for k, e in enumerate(edges[:15]):
        s.edges[k] = e
    return s


# ---- the emulator -------------------------------------------------------------------------------------------------------------------------------------
def load():
    global _lib
    if _lib is None:
        import fcntl
        so = os.path.join(EMU_DIR, "libsize_emu.so")
        deps = [os.path.join(EMU_DIR, "size_emu.cpp"), os.path.join(EMU_DIR, "wave_threads.h")] + [os.path.join(CSRC, f) for f in (
            "avk_sizebin.inl", "avk_sizebin.h", "avk_labels.inl", "avk_strata.inl", "avk_devpack.inl", "avk_pairs.inl", "avk_wave.h", "avk_dev_types.h")]
        with open(os.path.join(EMU_DIR, ".build.lock"), "w") as lock:  # (pytest-xdist workers: one builds, the others wait)
            fcntl.flock(lock, fcntl.LOCK_EX)
            if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
                subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-g", "-std=c++17", "-fPIC", "-Wall", "-Wextra", "-Wno-unused-function", "-Wno-unknown-pragmas",
                                       "-Wno-strict-aliasing", "-pthread", "-shared", "-o", so, "size_emu.cpp"], cwd=EMU_DIR)
        lib = C.CDLL(so)
        P = C.POINTER(AvkSizeSpec)
        lib.size_emu_spec_ok.argtypes = [P]
        lib.size_emu_bin.restype = C.c_uint32
        lib.size_emu_bin.argtypes = [P, C.c_uint32]
        lib.size_emu_size.restype = C.c_uint32
        lib.size_emu_size.argtypes = [C.c_uint32, C.c_uint32]
        lib.size_emu_field.restype = C.c_uint32
        lib.size_emu_field.argtypes = [C.c_uint32, C.c_int]
        lib.size_emu_run.argtypes = [C.POINTER(label_emu_lib.EmuView), u32p, C.c_uint32, P, C.c_uint32, u64p]
        _lib = lib
    return _lib


def emu_run(view, edges, mask=None, n_labels=0, grid=3):
    """every launch of a call on the emulator -> [1 + n_labels, n_bins, N_GROUPS, 14]"""
    n = int(view.n_regions)
    out = np.zeros((1 + n_labels, len(edges) + 1, N_GROUPS, N_SIZE_FIELDS), np.uint64)
    m = None if mask is None else np.ascontiguousarray(mask, np.uint32)
    assert m is None or m.shape == ((n_labels + 31) // 32, n)
    spec = c_spec(edges)
    rc = load().size_emu_run(C.byref(view), None if m is None else m.ctypes.data_as(u32p), n_labels, C.byref(spec), grid, out.ctypes.data_as(u64p))
    assert rc == 0
    return out
