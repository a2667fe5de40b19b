"""The rule of the bootstrap replicates (aardvark_amd/csrc/avk_boot.h) without a GPU: avk_boot_weight as a C program sees it through
include/aardvark_amd.h against the numpy restatement of tests/boot_lib.py, the twelve threshold literals against `decimal` at 50 digits, the distribution of the
weights, and the host route avk_boot_tallies_host against the ORACLE's blocks times restated weights — whole, cut in two, with labels, and every refusal."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import aardvark_amd
import boot_lib
import label_emu_lib
import oracle_lib
import scenarios
from aardvark_amd import _abi, synth

ROOT = boot_lib.ROOT
WORDS, SOLVED, ERRORS = boot_lib.WORDS, boot_lib.SOLVED, boot_lib.ERRORS
u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)

SNIPPET = r'''
#include "aardvark_amd.h"
void weights(uint64_t seed, const uint32_t *contig, const uint32_t *start, const uint32_t *b, uint64_t n, uint32_t *out) {
    for (uint64_t i = 0; i < n; ++i) out[i] = avk_boot_weight(seed, contig[i], start[i], b[i]);
}
uint64_t mixes_agree(uint64_t x) { return avk_boot_mix(x) == avk_region_hash(x); }
unsigned long spec_size(void) { return sizeof(avk_boot_spec); }
'''


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    """avk_boot_weight compiled as plain C from the public header"""
    d = tmp_path_factory.mktemp("boot_rule")
    open(os.path.join(d, "w.c"), "w").write(SNIPPET)
    so = os.path.join(d, "libw.so")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"), "-o", so, os.path.join(d, "w.c")])
    lib = C.CDLL(so)
    lib.weights.argtypes = [C.c_uint64, u32p, u32p, u32p, C.c_uint64, u32p]
    lib.mixes_agree.restype = C.c_uint64
    lib.mixes_agree.argtypes = [C.c_uint64]
    lib.spec_size.restype = C.c_ulong
    return lib


def c_weights(rule, seed, contig, start, b):
    contig, start, b = (np.ascontiguousarray(x, np.uint32) for x in (contig, start, b))
    out = np.zeros(len(b), np.uint32)
    rule.weights(seed, contig.ctypes.data_as(u32p), start.ctypes.data_as(u32p), b.ctypes.data_as(u32p), len(b), out.ctypes.data_as(u32p))
    return out


def test_weight_equals_the_restatement(rule):
    rng = np.random.default_rng(11)
    assert rule.spec_size() == C.sizeof(_abi.AvkBootSpec) == 16
    for x in (0, 1, 2 ** 63, 2 ** 64 - 1, 0x123456789ABCDEF):
        assert rule.mixes_agree(x) == 1
    for seed in [0, 1, 2 ** 64 - 1] + [int(s) for s in rng.integers(0, 2 ** 63, 5)]:
        n = 4000
        contig = rng.integers(0, 65536, n)
        start = rng.integers(0, 2 ** 32, n)
        contig[:4], start[:4] = [0, 0, 65535, 65535], [0, 2 ** 32 - 1, 0, 2 ** 32 - 1]
        for b in (0, 1, 4095):
            got = c_weights(rule, seed, contig, start, np.full(n, b))
            want = boot_lib.weights(seed, contig, start, [b])[:, 0]
            assert np.array_equal(got, want), (seed, b)
            assert np.array_equal(got[:16], [boot_lib.load().boot_emu_weight(seed, int(c), int(s), b) for c, s in zip(contig[:16], start[:16])])


def test_threshold_literals_equal_the_exact_values():
    want = boot_lib.thresholds()
    src = open(os.path.join(boot_lib.CSRC, "avk_boot.h")).read()
    lit = {int(k): int(v) for k, v in re.findall(r"#define AVK_BOOT_T(\d+) (\d+)u", src)}
    assert [lit[k] for k in range(12)] == want and len(lit) == 12
    assert [boot_lib.load().boot_emu_threshold(k) for k in range(12)] == want
    assert all(a < b for a, b in zip(want, want[1:])) and want[11] < 2 ** 32 - 1


def test_weights_are_poisson_1(rule):
    """10^6 (key, b) draws: the mean within 1 +- 0.005 and the share of zeros within e^-1 +- 0.0025 — five standard errors (sd 1: 0.001; sqrt(p (1 - p) / n): 0.00048)"""
    rng = np.random.default_rng(3)
    n = 1_000_000
    w = c_weights(rule, 1, rng.integers(0, 25, n), rng.integers(0, 250_000_000, n), rng.integers(0, 4096, n))
    print("mean %.5f zeros %.5f max %d" % (w.mean(), (w == 0).mean(), w.max()))
    assert abs(w.mean() - 1.0) <= 0.005
    assert abs((w == 0).mean() - np.exp(-1)) <= 0.0025
    assert w.max() <= 12


# ---- the host route -----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def job():
    """an oracle-solved batch (with unsolved regions) whose result batch also carries the compact BASEPAIR groups, made from the oracle's blocks: shared, never changed"""
    contigs, batch = scenarios.fuzz_regions(341, 300, max_vars=9, max_len=12)
    _, bad = scenarios.invalid_regions()
    batch = synth.concat_batches([batch, bad])
    res = oracle_lib.compare_batch(oracle_lib.load(), batch, contigs, threads=8)
    n = batch.n_regions
    bp_off, bp = np.zeros(n + 1, np.uint32), []
    for r in range(n):
        bp_off[r] = len(bp)
        if int(res.status[r]) == 0:
            bp += [res.group_metrics[r][g][14:18] for g in label_emu_lib.groups_of(batch, r)]
    bp_off[n] = len(bp)
    res.bp_off, res.bp_groups = bp_off, np.ascontiguousarray(np.array(bp, np.uint32).reshape(-1, 4))
    solved = np.asarray(res.status) == 0
    assert solved.sum() > 200 and (~solved).any()
    return dict(batch=batch, res=res, solved=solved, blocks=np.asarray(res.group_metrics).reshape(n, WORDS), contig=np.asarray(batch.contig_idx), start=np.asarray(batch.start))


def shifted(ptr, k):
    """ptr + k elements"""
    return C.cast(C.c_void_p(C.cast(ptr, C.c_void_p).value + k * C.sizeof(ptr._type_)), type(ptr))


def host(job, B, seed, lo=0, hi=None, labels=None, threads=1, out=None, rc_want=0, null_out=False):
    lib = aardvark_amd.load_library()
    batch = job["batch"]
    hi = batch.n_regions if hi is None else hi
    cb, ro = batch.c_struct(), job["res"].c_struct()
    for f in ("region_id", "contig_idx", "start", "end", "t_off", "t_cnt", "q_off", "q_cnt"):
        if getattr(cb, f):
            setattr(cb, f, shifted(getattr(cb, f), lo))
    cb.n_regions = hi - lo
    ro.status, ro.bp_off = shifted(ro.status, lo), shifted(ro.bp_off, lo)
    L = 0 if labels is None else labels[0]
    out = np.zeros((1 + L, B if 0 < B <= 4096 else 1, _abi.TALLY_LEN), np.uint64) if out is None else out
    lab, keep = (None, None) if labels is None else _abi.region_labels(*labels)
    spec = _abi.AvkBootSpec(B, seed)
    rc = lib.avk_boot_tallies_host(C.byref(cb), C.byref(ro), C.byref(spec), None if lab is None else C.byref(lab), threads, None if null_out else out.ctypes.data_as(u64p))
    assert rc == rc_want, lib.avk_last_error(None)
    return out


def want_of(job, B, seed, lo=0, hi=None, members=None):
    hi = job["batch"].n_regions if hi is None else hi
    w = boot_lib.weights(seed, job["contig"][lo:hi], job["start"][lo:hi], np.arange(B))
    return boot_lib.expected(job["blocks"][lo:hi], job["solved"][lo:hi], w, members)


@pytest.mark.parametrize("threads", [0, 1, 5, 16])
def test_host_route_equals_the_restatement(job, threads):
    got = host(job, 43, 7, threads=threads)
    assert np.array_equal(got, want_of(job, 43, 7)) and got[0, :, SOLVED].any() and not got[:, :, ERRORS].any()


def test_host_route_adds_and_leaves_the_error_word(job):
    out = np.zeros((1, 3, _abi.TALLY_LEN), np.uint64)
    out[:, :, ERRORS] = 9
    host(job, 3, 2, out=out)
    host(job, 3, 2, out=out)
    assert np.array_equal(out[:, :, :SOLVED + 1], 2 * want_of(job, 3, 2)[:, :, :SOLVED + 1]) and (out[:, :, ERRORS] == 9).all()


def test_two_batches_cut_at_an_odd_place_add_up(job):
    n, cut = job["batch"].n_regions, 137
    whole = host(job, 50, 99)
    parts = host(job, 50, 99, 0, cut)
    host(job, 50, 99, cut, n, out=parts)
    assert np.array_equal(parts, whole) and np.array_equal(whole, want_of(job, 50, 99))


def test_host_route_with_labels(job):
    n = job["batch"].n_regions
    rng = np.random.default_rng(2)
    members = [np.ones(n, bool), np.zeros(n, bool), rng.random(n) < 0.3, rng.random(n) < 0.05]
    lists = [[l for l in range(4) if members[l][r]] for r in range(n)]
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint64)
    idx = np.array([l for x in lists for l in x], np.uint32)
    got = host(job, 20, 5, labels=(4, off, idx), threads=3)
    assert np.array_equal(got, want_of(job, 20, 5, members=members))
    assert np.array_equal(got[1], got[0]) and not got[2].any() and got[4].any()


def test_spec_refusals(job):
    """each is AVK_E_ARG with its text and leaves `out` untouched"""
    lib = aardvark_amd.load_library()
    n = job["batch"].n_regions
    off, idx = np.arange(n + 1, dtype=np.uint64), np.zeros(n, np.uint32)
    out = np.zeros((5, 4096, _abi.TALLY_LEN), np.uint64)
    for B, labels, null_out, text in [(0, None, False, "0 replicates"), (4097, None, False, "4097 replicates"), (4096, (4, off, idx), False, "more than 16384 blocks"),
                                      (3277, (4, off, idx), False, "more than 16384 blocks"), (10, None, True, "boot_tallies missing")]:
        host(job, B, 1, labels=labels, out=out, rc_want=-1, null_out=null_out)
        assert text in lib.avk_last_error(None).decode(), (B, text)
        assert not out.any()
    host(job, 3276, 1, labels=(4, off, idx), out=out)  # (1 + 4) * 3276 = 16380 blocks: allowed
    assert out.reshape(-1)[:5 * 3276 * _abi.TALLY_LEN].reshape(5, 3276, _abi.TALLY_LEN)[1, 3275].any()  # (the block of scope 1, replicate 3275, in the call's own layout)
    spec = _abi.AvkBootSpec(4, 1)
    assert lib.avk_boot_tallies_host(None, None, C.byref(spec), None, 1, out.ctypes.data_as(u64p)) == -1
    assert lib.avk_boot_tallies(None, None, C.byref(spec), None, out.ctypes.data_as(u64p)) == -1
    assert lib.avk_boot_block(None) == 0


def test_python_declarations_agree_with_the_header():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "aardvark_amd.h")).read(), flags=re.S)
    lib = aardvark_amd.load_library()
    P, vp = C.POINTER, C.c_void_p
    want = {"avk_boot_tallies": [vp, vp, P(_abi.AvkBootSpec), vp, u64p],
            "avk_compare_packed_boot": [vp, P(_abi.AvkPackedBatch), P(_abi.AvkPackedEscapes), vp, P(_abi.AvkCompareConfig), P(_abi.AvkResultBatch), u64p, P(_abi.AvkBootSpec), u64p],
            "avk_boot_tallies_host": [P(_abi.AvkRegionBatch), P(_abi.AvkResultBatch), P(_abi.AvkBootSpec), P(_abi.AvkRegionLabels), C.c_uint32, u64p]}
    for name, argtypes in want.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
        assert m and len(m.group(1).split(",")) == len(argtypes), name
        assert list(getattr(lib, name).argtypes) == argtypes and getattr(lib, name).restype is C.c_int
    import inspect
    assert "boot" in inspect.signature(aardvark_amd.Context.solve_packed).parameters and aardvark_amd.BootSpec(5).seed == 1
