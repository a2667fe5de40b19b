"""Shared by the score-curve tests: a RESTATEMENT of the rule of aardvark_amd/csrc/avk_score.h in numpy and plain Python over size_lib.calls_of — a call's bin from
its float32 score, a truth call's bin from its region's supporting query calls, what a call adds at every POINT of the curve (no histogram, no scan: the direct
statement) — with seeded scores that sit on, and one float32 ulp either side of, every threshold; no code under test — and the loader of
tests/emu/libscore_emu.so (both kernels' wave code on the CPU, tests/emu/score_emu.cpp).  Test infrastructure; built here, into a library of its own."""
import ctypes as C
import os
import subprocess

import numpy as np

import label_emu_lib
import size_lib
from aardvark_amd._abi import N_GROUPS, AvkScoreSpec

EMU_DIR, CSRC = label_emu_lib.EMU_DIR, label_emu_lib.CSRC
N_SCORE_FIELDS = 14
DEFAULT = (5, 10, 15, 20, 25, 30, 35, 40, 50, 60)
THIRTY_ONE = tuple(float(x) for x in range(-5, 57, 2))  # 31 thresholds, negative ones and 0 among them
SPECS = [(20.0,), (10.0, 30.5), DEFAULT, THIRTY_ONE]     # K = 1, 2, 10 and 31
TRUTH_F, QUERY_F = size_lib.TRUTH_F, size_lib.QUERY_F
LOST_F = [TRUTH_F[1], TRUTH_F[4], TRUTH_F[6]]            # GT_TRUTH_FN, HAP_TRUTH_FN, WHAP_TRUTH_FN
assert LOST_F == [1, 7, 11]
M = 0xFFFFFFFF
u32p, u64p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_float)
_lib = None


# ---- the rule, restated -----------------------------------------------------------------------------------------------------------------------------
def valid(thresholds):
    t = np.asarray(thresholds, np.float32)
    return 1 <= len(t) <= 31 and bool(np.isfinite(t).all()) and all(a < b for a, b in zip(t, t[1:]))


def bin_of(thresholds, score):
    """the number of thresholds <= score, both float32; a comparison with NaN is false"""
    s = np.float32(score)
    return sum(1 for t in thresholds if s >= np.float32(t))


def names_of(thresholds):
    return ["score_all"] + ["score_ge_%g" % float(np.float32(t)) for t in thresholds]


def scores_for(n_variants, thresholds, seed):
    """float32 scores for every call (truth entries too: they must not be read): NaN, the infinities, -0.0, every threshold and its two float32 neighbours,
    and values spread below, between and above the thresholds"""
    rng = np.random.default_rng(seed)
    t = np.asarray(thresholds, np.float32)
    special = [np.float32("nan"), np.float32("inf"), np.float32("-inf"), np.float32(-0.0)]
    for x in t:
        special += [x, np.nextafter(x, np.float32("-inf"), dtype=np.float32), np.nextafter(x, np.float32("inf"), dtype=np.float32)]
    special = np.array(special, np.float32)
    lo, hi = float(t[0]) - 10.0, float(t[-1]) + 10.0
    out = rng.uniform(lo, hi, n_variants).astype(np.float32)
    pick = rng.random(n_variants) < 0.45
    out[pick] = special[rng.integers(0, len(special), int(pick.sum()))]
    return out


def call_index(batch, res):
    """the batch's call index of every row of size_lib.calls_of(batch, res), in its order"""
    out = []
    for r in range(batch.n_regions):
        if int(res.status[r]) != 0:
            continue
        out += [int(batch.t_off[r]) + i for i in range(int(batch.t_cnt[r]))] + [int(batch.q_off[r]) + i for i in range(int(batch.q_cnt[r]))]
    return np.array(out, np.int64)


def packed_order(batch):
    """the batch's call indices in the order of the packed form: region after region, a region's truth calls, then its query calls"""
    out = []
    for r in range(batch.n_regions):
        out += [int(batch.t_off[r]) + i for i in range(int(batch.t_cnt[r]))] + [int(batch.q_off[r]) + i for i in range(int(batch.q_cnt[r]))]
    return np.array(out, np.int64)


def bins_of_calls(calls, vidx, thresholds, scores):
    """the bin of every row: a query call's from its score; a truth call's K when observed is 0, else the minimum over its region's query calls with hap_tp > 0"""
    K = len(thresholds)
    qbin = {}
    for row, v in zip(calls, vidx):
        if int(row[1]) == 1:
            qbin[int(v)] = bin_of(thresholds, scores[int(v)])
    support = {}
    for row, v in zip(calls, vidx):
        if int(row[1]) == 1 and int(row[4 + 3]) > 0:
            r = int(row[0])
            support[r] = min(support.get(r, K), qbin[int(v)])
    out = np.zeros(len(calls), np.int64)
    for n, (row, v) in enumerate(zip(calls, vidx)):
        if int(row[1]) == 1:
            out[n] = qbin[int(v)]
        else:
            out[n] = K if int(row[4 + 3]) == 0 else support.get(int(row[0]), K)
    return out


def lost_of(row, w):
    """a truth call's lost values: gt_fn = 1, hap_fn = exp, w_fn = (u32)(exp * alt_ed); exp = hap_tp + hap_fn"""
    exp = (int(row[4 + 3]) + int(row[4 + 4])) & M
    return 1, exp, (exp * int(w)) & M


def expected(calls, vidx, alt_ed, thresholds, scores, n_regions, members=None, lo=0, hi=None):
    """calls (size_lib.calls_of), their call indices, alt_ed per call, the thresholds, scores per call index, the regions [lo, hi), members [L, n_regions] bool or
    None -> [1 + L, n_points, N_GROUPS, 14] uint64: the curve, point by point"""
    hi = n_regions if hi is None else hi
    K = len(thresholds)
    scopes = [np.ones(n_regions, bool)] + ([] if members is None else [np.asarray(m, bool) for m in members])
    out = np.zeros((len(scopes), K + 1, N_GROUPS, N_SCORE_FIELDS), np.uint64)
    bins = bins_of_calls(calls, vidx, thresholds, scores)
    for row, v, b in zip(calls, vidx, bins):
        r, side, vt = int(row[0]), int(row[1]), int(row[2])
        if not lo <= r < hi:
            continue
        add = np.zeros((K + 1, N_SCORE_FIELDS), np.uint64)
        for k in range(K + 1):
            if k <= b:
                for j in range(7):
                    add[k, (QUERY_F if side else TRUTH_F)[j]] = int(row[4 + j])
            elif side == 0:
                for f, x in zip(LOST_F, lost_of(row, alt_ed[int(v)])):
                    add[k, f] = x
        for s, m in enumerate(scopes):
            if m[r]:
                for g in (0, 1 + vt):
                    if g < N_GROUPS:
                        out[s, :, g, :] += add
    return out


def check_invariants(block, tally14=None):
    """what follows from the rule, on a [.., n_points, N_GROUPS, 14] block"""
    b = np.asarray(block, np.uint64).astype(object)
    for tp, fn in ((TRUTH_F[0], TRUTH_F[1]), (TRUTH_F[3], TRUTH_F[4])):
        tot = b[..., tp] + b[..., fn]
        assert (tot == tot[..., :1, :]).all(), "TRUTH_TP + TRUTH_FN is the same at every point"
    for f in [TRUTH_F[0], TRUTH_F[3], TRUTH_F[5]] + QUERY_F:
        col = b[..., f]
        assert (col[..., 1:, :] <= col[..., :-1, :]).all(), "field %d is non-increasing in k" % f
    if tally14 is not None:
        assert np.array_equal(np.asarray(block)[..., 0, :, :], tally14), "point 0 is the tally"


def c_spec(thresholds, n=None):
    s = AvkScoreSpec()
    s.n_thresholds = len(thresholds) if n is None else n
    for k, t in enumerate(thresholds[:31]):
        s.t[k] = t
    return s


# ---- the emulator -------------------------------------------------------------------------------------------------------------------------------------
def load():
    global _lib
    if _lib is None:
        import fcntl
        so = os.path.join(EMU_DIR, "libscore_emu.so")
        deps = [os.path.join(EMU_DIR, "score_emu.cpp"), os.path.join(EMU_DIR, "wave_threads.h")] + [os.path.join(CSRC, f) for f in (
            "avk_score.inl", "avk_score.h", "avk_sizebin.inl", "avk_sizebin.h", "avk_labels.inl", "avk_strata.inl", "avk_devpack.inl", "avk_pairs.inl", "avk_wave.h", "avk_dev_types.h")]
        with open(os.path.join(EMU_DIR, ".build.lock"), "w") as lock:  # (pytest-xdist workers: one builds, the others wait)
            fcntl.flock(lock, fcntl.LOCK_EX)
            if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
                subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-g", "-std=c++17", "-fPIC", "-Wall", "-Wextra", "-Wno-unused-function", "-Wno-unknown-pragmas",
                                       "-Wno-strict-aliasing", "-pthread", "-shared", "-o", so, "score_emu.cpp"], cwd=EMU_DIR)
        lib = C.CDLL(so)
        P = C.POINTER(AvkScoreSpec)
        lib.score_emu_spec_ok.argtypes = [P]
        lib.score_emu_bin.restype = C.c_uint32
        lib.score_emu_bin.argtypes = [P, C.c_float]
        lib.score_emu_run.argtypes = [C.POINTER(label_emu_lib.EmuView), u32p, C.c_uint32, P, f32p, C.c_uint32, u64p]
        _lib = lib
    return _lib


def emu_run(view, thresholds, scores, mask=None, n_labels=0, grid=3):
    """every launch of a call on the emulator -> [1 + n_labels, n_points, N_GROUPS, 14]"""
    n = int(view.n_regions)
    out = np.zeros((1 + n_labels, len(thresholds) + 1, N_GROUPS, N_SCORE_FIELDS), np.uint64)
    m = None if mask is None else np.ascontiguousarray(mask, np.uint32)
    assert m is None or m.shape == ((n_labels + 31) // 32, n)
    spec, sc = c_spec(thresholds), np.ascontiguousarray(scores, np.float32)
    rc = load().score_emu_run(C.byref(view), None if m is None else m.ctypes.data_as(u32p), n_labels, C.byref(spec), sc.ctypes.data_as(f32p), grid, out.ctypes.data_as(u64p))
    assert rc == 0
    return out
