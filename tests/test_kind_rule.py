"""The rule of the call kinds (aardvark_amd/csrc/avk_callkind.h) without a GPU: the header's functions through tests/native/kind_check.cpp
against the restatement of tests/kind_lib.py — all 256 x 256 byte pairs at lengths 1 / 1, lengths 0, 1 and 2 on either side, every zygosity value 0 to 7 — the
names and the field map.  Every comparison is exact."""
import ctypes as C
import os
import re

import numpy as np

import aardvark_amd
import kind_lib
from aardvark_amd import _abi


def test_every_byte_pair():
    got = np.zeros(65536, np.uint8)
    kind_lib.load_check().kind_check_pairs(got.ctypes.data_as(kind_lib.u8p))
    want = np.array([kind_lib.sub_of(bytes([b0]), bytes([b1])) for b0 in range(256) for b1 in range(256)], np.uint8)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    # 4 transitions and 8 transversions among the ordered pairs of ACGT, in each of the 4 case combinations
    assert (want == 0).sum() == 16 and (want == 1).sum() == 32
    at = lambda a, b: int(got[ord(a) * 256 + ord(b)])
    assert at("a", "g") == 0 and at("C", "a") == 1 and at("A", "N") == 2 and at("a", "A") == 2 and at("c", "T") == 0 and at("G", "t") == 1 and at("R", "A") == 2


def test_lengths():
    chk = kind_lib.load_check()
    for l0 in (0, 1, 2):
        for l1 in (0, 1, 2):
            for b0, b1 in ((ord("A"), ord("G")), (ord("A"), ord("C")), (ord("A"), ord("A"))):
                want = kind_lib.sub_of(bytes([b0]) * l0, bytes([b1]) * l1)
                assert chk.kind_check_sub(l0, l1, b0, b1) == want and (want == 2 or (l0, l1) == (1, 1))


def test_every_zygosity():
    chk = kind_lib.load_check()
    assert [chk.kind_check_gt(z) for z in range(8)] == [kind_lib.gt_of(z) for z in range(8)] == [2, 2, 0, 0, 0, 1, 2, 2]
    assert _abi.ZYGOSITIES[2:6] == ["UnphasedHeterozygous", "PhasedHet01", "PhasedHet10", "HomozygousAlternate"]
    assert [chk.kind_check_kind(g, s) for g in range(3) for s in range(3)] == list(range(9)) and chk.kind_check_n() == 9


def test_names():
    chk, lib = kind_lib.load_check(), aardvark_amd.load_library()
    assert [chk.kind_check_name(k).decode() for k in range(9)] == kind_lib.NAMES == aardvark_amd.KIND_NAMES and chk.kind_check_name(9) is None
    assert lib.avk_kind_n() == 9 and lib.avk_kind_block(None) == 0
    for k, name in enumerate(kind_lib.NAMES):
        buf = C.create_string_buffer(16)
        assert lib.avk_kind_name(k, buf, 16) == 0 and buf.value.decode() == name
    buf = C.create_string_buffer(8)
    assert lib.avk_kind_name(9, buf, 8) == -1 and lib.avk_kind_name(8, buf, 8) == -1 and lib.avk_kind_name(0, buf, 8) == 0 and buf.value == b"het_ts"  # "nogt_other" needs 11


def test_fields_of_a_contribution():
    chk = kind_lib.load_check()
    assert [chk.kind_check_field(k, 0) for k in range(7)] == kind_lib.TRUTH_F and [chk.kind_check_field(k, 1) for k in range(7)] == kind_lib.QUERY_F


def test_python_declarations_agree_with_the_header():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(kind_lib.ROOT, "include", "aardvark_amd.h")).read(), flags=re.S)
    lib = aardvark_amd.load_library()
    P, vp, u64p = C.POINTER, C.c_void_p, kind_lib.u64p
    want = {"avk_kind_tallies": [vp, vp, vp, u64p],
            "avk_compare_packed_kind": [vp, P(_abi.AvkPackedBatch), P(_abi.AvkPackedEscapes), vp, P(_abi.AvkCompareConfig), P(_abi.AvkResultBatch), u64p],
            "avk_kind_tallies_host": [P(_abi.AvkRegionBatch), P(_abi.AvkResultBatch), P(_abi.AvkRegionLabels), C.c_uint32, u64p]}
    for name, argtypes in want.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
        assert m and len(m.group(1).split(",")) == len(argtypes), name
        assert list(getattr(lib, name).argtypes) == argtypes and getattr(lib, name).restype is C.c_int
    import inspect
    assert "kinds" in inspect.signature(aardvark_amd.Context.solve_packed).parameters
