"""The rule of the size bins (aardvark_amd/csrc/avk_sizebin.h) without a GPU: the header's bin() at every edge against the restatement of
tests/size_lib.py, the bins' names, every invalid spec, the host route avk_size_tallies_host against the restatement on the ORACLE's per-call outputs — whole, cut
in two, with labels — and the conservation law against the oracle's summed group_metrics.  Every comparison is exact."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import aardvark_amd
import oracle_lib
import scenarios
import size_lib
from aardvark_amd import SizeSpec, _abi, size_tallies_host

u64p = C.POINTER(C.c_uint64)
INVALID = [(), tuple(range(1, 17)), (0, 5), (3, 3), (1, 6, 6, 50), (6, 1), (1, 6, 16, 15)]


@pytest.mark.parametrize("edges", size_lib.EDGE_SETS)
def test_bin_at_every_edge(edges):
    emu, spec = size_lib.load(), size_lib.c_spec(edges)
    assert emu.size_emu_spec_ok(C.byref(spec)) == 1 and aardvark_amd.load_library().avk_size_n_bins(C.byref(spec)) == len(edges) + 1
    sizes = sorted({0, 2 ** 32 - 1} | {s for e in edges for s in (e - 1, e, e + 1)})
    for s in sizes:
        assert emu.size_emu_bin(C.byref(spec), s) == size_lib.bin_of(edges, s), s
    hit = {size_lib.bin_of(edges, s) for s in sizes}
    assert hit == set(range(len(edges) + 1))
    for a0, a1 in ((1, 1), (1, 6), (6, 1), (300, 1), (1, 3001), (0, 0)):
        assert emu.size_emu_size(a0, a1) == abs(a1 - a0)


def test_fields_of_a_contribution():
    emu = size_lib.load()
    assert [emu.size_emu_field(k, 0) for k in range(7)] == size_lib.TRUTH_F and [emu.size_emu_field(k, 1) for k in range(7)] == size_lib.QUERY_F
    assert sorted(size_lib.TRUTH_F + size_lib.QUERY_F) == list(range(14))


def test_names():
    assert SizeSpec().names() == ["len_0", "len_1_5", "len_6_15", "len_16_49", "len_ge50"] == size_lib.names_of(size_lib.DEFAULT)
    one = (1, 2, 10, 11)  # bins of one size: 1, and 10
    assert SizeSpec(one).names() == ["len_0", "len_1", "len_2_9", "len_10", "len_ge11"] == size_lib.names_of(one)
    assert SizeSpec(size_lib.FIFTEEN).names() == size_lib.names_of(size_lib.FIFTEEN) and SizeSpec((2,)).names() == ["len_0_1", "len_ge2"]
    lib, spec = aardvark_amd.load_library(), size_lib.c_spec(size_lib.DEFAULT)
    buf = C.create_string_buffer(8)
    assert lib.avk_size_bin_name(C.byref(spec), 5, buf, 8) == -1 and lib.avk_size_bin_name(C.byref(spec), 3, buf, 8) == -1  # no such bin; "len_16_49" needs 10 bytes
    assert lib.avk_size_bin_name(C.byref(spec), 0, buf, 8) == 0 and buf.value == b"len_0"


@pytest.fixture(scope="module")
def job():
    """three oracle-solved batches (indels of every default bin, unsolved regions, kilobase alleles and SV types), their calls restated: shared, never changed"""
    parts = []
    for contigs, batch in (scenarios.indel_small(1500), scenarios.invalid_regions(), scenarios.long_allele_regions()):
        res = oracle_lib.compare_batch(oracle_lib.load(), batch, contigs, threads=8)
        parts.append(dict(batch=batch, res=res, calls=size_lib.calls_of(batch, res)))
    assert any((np.asarray(p["res"].status) != 0).any() for p in parts)
    return parts


def host_sum(job, edges, threads=1, labels=None):
    out = None
    for k, p in enumerate(job):
        out = size_tallies_host(p["batch"], p["res"], SizeSpec(edges), labels=None if labels is None else labels[k], threads=threads, out=out)
    return out


def want_sum(job, edges, members=None):
    return sum(size_lib.expected(p["calls"], edges, p["batch"].n_regions, None if members is None else members[k]) for k, p in enumerate(job))


@pytest.mark.parametrize("edges", size_lib.EDGE_SETS)
@pytest.mark.parametrize("threads", [0, 5])
def test_host_route_equals_the_restatement(job, edges, threads):
    got, want = host_sum(job, edges, threads), want_sum(job, edges)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    if edges == size_lib.DEFAULT:
        assert all(got[0, b, 0, size_lib.TRUTH_F[:2]].sum() > 0 and got[0, b, 0, size_lib.QUERY_F[:2]].sum() > 0 for b in range(5))


def test_host_route_adds_and_is_additive_over_a_cut(job):
    p = job[0]
    spec = SizeSpec()
    whole = size_tallies_host(p["batch"], p["res"], spec)
    twice = size_tallies_host(p["batch"], p["res"], spec, out=whole.copy())
    assert np.array_equal(twice, 2 * whole)
    # the first 137 regions as a batch of their own, and the rest
    lib, cut, n = aardvark_amd.load_library(), 137, p["batch"].n_regions
    parts = np.zeros_like(whole)
    for lo, hi in ((0, cut), (cut, n)):
        cb, ro, ss = p["batch"].c_struct(), p["res"].c_struct(), spec.c_struct()
        for f in ("region_id", "contig_idx", "start", "end", "t_off", "t_cnt", "q_off", "q_cnt"):
            if getattr(cb, f):
                ptr = getattr(cb, f)
                setattr(cb, f, C.cast(C.c_void_p(C.cast(ptr, C.c_void_p).value + lo * C.sizeof(ptr._type_)), type(ptr)))
        cb.n_regions = hi - lo
        ro.status = C.cast(C.c_void_p(C.cast(ro.status, C.c_void_p).value + lo * 4), type(ro.status))
        assert lib.avk_size_tallies_host(C.byref(cb), C.byref(ro), C.byref(ss), None, 3, parts.ctypes.data_as(u64p)) == 0
    assert np.array_equal(parts, whole)
    assert np.array_equal(size_lib.expected(p["calls"], size_lib.DEFAULT, n, lo=0, hi=cut) + size_lib.expected(p["calls"], size_lib.DEFAULT, n, lo=cut), whole)


def test_host_route_with_labels(job):
    rng = np.random.default_rng(2)
    members, labels = [], []
    for p in job:
        n = p["batch"].n_regions
        m = [np.ones(n, bool), np.zeros(n, bool), rng.random(n) < 0.3, rng.random(n) < 0.05]
        lists = [[l for l in range(4) if m[l][r]] for r in range(n)]
        off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint64)
        members.append(m), labels.append((4, off, np.array([l for x in lists for l in x] + [0], np.uint32)))
    got = host_sum(job, size_lib.DEFAULT, 3, labels)
    assert np.array_equal(got, want_sum(job, size_lib.DEFAULT, members))
    assert np.array_equal(got[1], got[0]) and not got[2].any() and got[3].any() and got[4].any()


@pytest.mark.parametrize("edges", size_lib.EDGE_SETS)
def test_conservation_law_against_the_oracle(job, edges):
    """for every group and f < 14 the sum over the bins is the word of the oracle's tally: its group_metrics summed over the solved regions"""
    got = host_sum(job, edges)
    tally = np.zeros((_abi.N_GROUPS, _abi.N_FIELDS), np.uint64)
    for p in job:
        solved = np.asarray(p["res"].status) == 0
        tally += np.asarray(p["res"].group_metrics).reshape(p["batch"].n_regions, _abi.N_GROUPS, _abi.N_FIELDS)[solved].astype(np.uint64).sum(axis=0)
    assert np.array_equal(got[0].sum(axis=0), tally[:, :14]) and tally[:, :14].any()


def test_invalid_specs_are_refused(job):
    """n_edges 0 and 16, an edge of 0, equal neighbours, descending edges: AVK_E_ARG with its text, `out` untouched; NULL spec and NULL out likewise"""
    lib, emu, p = aardvark_amd.load_library(), size_lib.load(), job[1]
    out = np.zeros((1, 17, _abi.N_GROUPS, 14), np.uint64)
    cb, ro = p["batch"].c_struct(), p["res"].c_struct()
    for edges in INVALID:
        assert not size_lib.valid(edges)
        spec = size_lib.c_spec(edges[:15], n_edges=len(edges))
        assert emu.size_emu_spec_ok(C.byref(spec)) == 0 and lib.avk_size_n_bins(C.byref(spec)) == 0
        assert lib.avk_size_tallies_host(C.byref(cb), C.byref(ro), C.byref(spec), None, 1, out.ctypes.data_as(u64p)) == -1, edges
        assert "strictly ascending" in lib.avk_last_error(None).decode() and not out.any()
        assert lib.avk_size_bin_name(C.byref(spec), 0, C.create_string_buffer(32), 32) == -1
        assert lib.avk_size_tallies(None, None, C.byref(spec), None, out.ctypes.data_as(u64p)) == -1
    good = size_lib.c_spec(size_lib.DEFAULT)
    assert lib.avk_size_tallies_host(C.byref(cb), C.byref(ro), None, None, 1, out.ctypes.data_as(u64p)) == -1 and "spec missing" in lib.avk_last_error(None).decode()
    assert lib.avk_size_tallies_host(C.byref(cb), C.byref(ro), C.byref(good), None, 1, None) == -1 and "size_tallies missing" in lib.avk_last_error(None).decode()
    assert lib.avk_size_n_bins(None) == 0 and lib.avk_size_block(None) == 0 and not out.any()
    for edges in size_lib.EDGE_SETS:
        assert size_lib.valid(edges) and emu.size_emu_spec_ok(C.byref(size_lib.c_spec(edges))) == 1


def test_python_declarations_agree_with_the_header():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(size_lib.ROOT, "include", "aardvark_amd.h")).read(), flags=re.S)
    lib = aardvark_amd.load_library()
    P, vp = C.POINTER, C.c_void_p
    want = {"avk_size_tallies": [vp, vp, P(_abi.AvkSizeSpec), vp, u64p],
            "avk_compare_packed_size": [vp, P(_abi.AvkPackedBatch), P(_abi.AvkPackedEscapes), vp, P(_abi.AvkCompareConfig), P(_abi.AvkSizeSpec), P(_abi.AvkResultBatch), u64p],
            "avk_size_tallies_host": [P(_abi.AvkRegionBatch), P(_abi.AvkResultBatch), P(_abi.AvkSizeSpec), P(_abi.AvkRegionLabels), C.c_uint32, u64p]}
    for name, argtypes in want.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
        assert m and len(m.group(1).split(",")) == len(argtypes), name
        assert list(getattr(lib, name).argtypes) == argtypes and getattr(lib, name).restype is C.c_int
    assert C.sizeof(_abi.AvkSizeSpec) == 64
    import inspect
    assert "size" in inspect.signature(aardvark_amd.Context.solve_packed).parameters and SizeSpec().edges == (1, 6, 16, 50)
