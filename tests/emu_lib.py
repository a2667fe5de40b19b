"""Loader for the kernel-logic emulator (tests/emu/libavk_emu.so): the HIP solver source run
on CPU lanes.  Test infrastructure for the GPU-less container."""
import ctypes as C
import os
import subprocess

from aardvark_amd._abi import AvkCompareConfig, AvkRegionBatch, AvkResultBatch, ResultBatch
from oracle_lib import ContigSet, u8p, u64p

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
_lib = None


def load():
    global _lib
    if _lib is None:
        import fcntl
        with open(os.path.join(EMU_DIR, ".build.lock"), "w") as lock:  # pytest-xdist workers: one of them builds, the others wait (a half-written .so is an OSError)
            fcntl.flock(lock, fcntl.LOCK_EX)
            subprocess.check_call(["make", "-C", EMU_DIR, "libavk_emu.so"], stdout=subprocess.DEVNULL)
        lib = C.CDLL(os.path.join(EMU_DIR, "libavk_emu.so"))
        lib.emu_compare_batch.argtypes = [C.POINTER(AvkRegionBatch), C.POINTER(u8p), u64p, C.c_uint32, C.POINTER(AvkCompareConfig),
                                          C.POINTER(AvkResultBatch), C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64,
                                          C.c_uint32, C.c_int, u64p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]
        lib.emu_optimize_pairs_batch.argtypes = [C.POINTER(AvkRegionBatch), C.POINTER(u8p), u64p, C.c_uint32, C.c_uint32,
                                                 C.POINTER(C.c_int32), u8p, C.c_int]
        lib.emu_set_lane_kernel.argtypes = [C.c_int]
        lib.emu_last_lane_solved.restype = C.c_uint64
        lib.emu_last_wide_solved.restype = C.c_uint64
        lib.emu_set_wide_kernel.argtypes = [C.c_int]
        lib.emu_set_wide_lds_bytes.argtypes = [C.c_uint32]
        lib.emu_set_lane_pool.argtypes = [C.c_int]
        lib.emu_set_lane_quad.argtypes = [C.c_int]
        lib.emu_last_quad_solved.restype = C.c_uint64
        lib.emu_widen_packed_esc.argtypes = [C.c_void_p, C.c_void_p, u64p, u64p, u64p, u64p, C.POINTER(EmuWideArrays)]
        lib.emu_widen_packed_multi_esc.argtypes = [C.c_void_p, C.c_void_p, u64p, u64p, u64p, u64p, C.POINTER(EmuWideArrays)]
        lib.emu_esc_lower.restype = C.c_uint64
        lib.emu_esc_lower.argtypes = [u64p, C.c_uint64, C.c_uint64]
        _lib = lib
    return _lib


class EmuWideArrays(C.Structure):
    """emu_wide_arrays of tests/emu/wave_emu.cpp: the wide arrays the widening functions of avk_devpack.inl write"""
    U32 = ("contig", "t_cnt", "q_cnt", "a0_len", "a1_len", "raw", "in_cnt")
    U64 = ("start", "end", "t_off", "q_off", "pos", "a0_off", "a1_off", "in_off")
    U8 = ("type", "zyg")
    _fields_ = [(f, C.POINTER(C.c_uint32)) for f in U32] + [(f, u64p) for f in U64] + [(f, u8p) for f in U8]


GUARD = 16  # guard elements behind every output array of widen_packed_esc, checked after the run
PER_REGION = ("contig", "t_cnt", "q_cnt", "start", "end", "t_off", "q_off")
PER_SLOT = ("in_cnt", "in_off")


def widen_packed_esc(pb, sums):
    """dp_widen_packed_esc (PackedBatch) / dp_widen_packed_multi_esc (PackedMultiBatch) for every lane i in [0, max(n_regions, n_variants)), on CPU lanes.
    sums = (narrow call offsets [v_off or in_off], narrow allele offsets a_off, cnt_before, bytes_before): uint64 exclusive sums, the last two with the total
    as entry n.  -> (dict of the wide arrays, refused: what the scan of the three lists says).  Every output array has GUARD elements behind it that must
    come back untouched, and starts out as 0xEE bytes."""
    import numpy as np
    lib = load()
    multi = hasattr(pb, "n_inputs")
    n, nv = pb.n_regions, pb.n_variants
    ns = n * pb.n_inputs if multi else 2 * n
    w, out = EmuWideArrays(), {}
    for names, dt, ct in ((EmuWideArrays.U32, np.uint32, C.c_uint32), (EmuWideArrays.U64, np.uint64, C.c_uint64), (EmuWideArrays.U8, np.uint8, C.c_uint8)):
        for f in names:
            size = n if f in PER_REGION else (ns if f in PER_SLOT else nv)
            a = np.empty(size + GUARD, dt)
            a.view(np.uint8)[:] = 0xEE
            out[f] = (a, size)
            setattr(w, f, a.ctypes.data_as(C.POINTER(ct)))
    v_off, a_off, cnt_before, bytes_before = [np.ascontiguousarray(x, np.uint64) for x in sums]
    assert cnt_before.size == pb.escapes.esc_slot.size + 1 and bytes_before.size == pb.escapes.esc_call.size + 1 and v_off.size >= (ns if multi else n) and a_off.size >= nv
    st, esc = pb.c_struct(), pb.escapes.c_struct()
    P = lambda x: x.ctypes.data_as(u64p)
    entry = lib.emu_widen_packed_multi_esc if multi else lib.emu_widen_packed_esc
    refused = entry(C.byref(st), C.byref(esc), P(v_off), P(a_off), P(cnt_before), P(bytes_before), C.byref(w))
    for f, (a, size) in out.items():
        assert np.all(a[size:].view(np.uint8) == 0xEE), "the widening wrote behind the end of " + f
    return {f: a[:size] for f, (a, size) in out.items()}, int(refused)


def esc_lower(lst, key):
    """dp_esc_lower: the first p with lst[p] >= key"""
    import numpy as np
    lst = np.ascontiguousarray(lst, np.uint64)
    return int(load().emu_esc_lower(lst.ctypes.data_as(u64p), lst.size, int(key)))


def compare_batch(batch, contigs, max_branch_factor=50, sequences=False, exact_shortcut=False,
                  lds_bytes=10 * 1024, lds_ed_cap=48, lds2_bytes=40 * 1024, lds2_ed_cap=48, ws_bytes=1 << 20, big_ws_bytes=64 << 20,
                  n_waves=8, threads=8, solo_min_variants=5, lds2_overflow_pass=0, lds_escalation=1, group_metrics=True, lane_kernel=True, bp_groups=False,
                  wide_kernel=True, wide_lds_bytes=16 * 1024, class_c_all=False, packed=False, lane_pool=-1, lane_quad=True, big_slots=2):
    """lane_kernel: small regions go through the lane-per-region code (avk_lane.inl), the rest through the wave-per-region code, as
    avk_compare_resident does; False = everything through the wave-per-region code.  res.lane_solved = regions the lane code finished.
    wide_kernel: class C and what the three-call lane class hands back go through the wave-cooperative code of avk_wide.inl first
    (res.wide_solved = regions it finished); class_c_all = every region outside the lane classes is planned as class C.
    big_slots: the shared big slices an HBM-tier wave escalates into when its own slice (ws_bytes) overflows."""
    lib = load()
    lib.emu_set_lane_kernel(1 if lane_kernel else 0)
    lib.emu_set_wide_kernel(1 if wide_kernel else 0)
    lib.emu_set_wide_lds_bytes(wide_lds_bytes)
    lib.emu_set_lane_quad(1 if lane_quad else 0)  # context option lane_quad: launches of at most 16 records per wave run four lanes per region (avk_quad.inl); res.quad_solved
    lib.emu_set_lane_pool(lane_pool)  # context option lane_pool: node states a lane keeps during its search (-1: by class, in the heads and the three-call class)
    before = os.environ.get("AVK_EMU_CLASS_C")
    if class_c_all:
        os.environ["AVK_EMU_CLASS_C"] = "100000"
    cs = contigs if isinstance(contigs, ContigSet) else ContigSet(contigs)
    res = ResultBatch(batch, sequences=sequences, group_metrics=group_metrics, bp_groups=bp_groups, packed=packed)
    cfg = AvkCompareConfig(max_branch_factor, 1 if sequences else 0, 1 if exact_shortcut else 0)
    cb, ro = batch.c_struct(), res.c_struct()
    tiers = (C.c_uint64 * 5)()
    rc = lib.emu_compare_batch(C.byref(cb), cs.ptrs, cs.lens, cs.n, C.byref(cfg), C.byref(ro), lds_bytes, lds_ed_cap, lds2_bytes, lds2_ed_cap,
                               ws_bytes, big_ws_bytes, n_waves, threads, tiers, solo_min_variants, lds2_overflow_pass, lds_escalation, big_slots)
    assert rc == 0
    res.tier_counts = [int(x) for x in tiers]
    res.lane_solved = int(lib.emu_last_lane_solved())
    res.wide_solved = int(lib.emu_last_wide_solved())
    res.quad_solved = int(lib.emu_last_quad_solved())
    if class_c_all:
        if before is None:
            os.environ.pop("AVK_EMU_CLASS_C", None)
        else:
            os.environ["AVK_EMU_CLASS_C"] = before
    return res


def optimize_pairs(batch, contigs, max_branch_factor=50, threads=8):
    import numpy as np
    lib = load()
    cs = contigs if isinstance(contigs, ContigSet) else ContigSet(contigs)
    status = np.full(batch.n_regions, -1, np.int32)
    exact = np.zeros(max(batch.n_regions, 1), np.uint8)
    cb = batch.c_struct()
    rc = lib.emu_optimize_pairs_batch(C.byref(cb), cs.ptrs, cs.lens, cs.n, max_branch_factor, status.ctypes.data_as(C.POINTER(C.c_int32)),
                                      exact.ctypes.data_as(u8p), threads)
    assert rc == 0
    return status, exact[:batch.n_regions]
