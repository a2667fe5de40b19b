"""The layout of the 2-bit reference on the CPU: the emulator's packed copy and flag bitmap (what every emulated parity test reads; emu_ref_packed of
tests/emu/wave_emu.cpp hands out what emu_run builds) against the numpy reference of ref_edges_lib.py, on the references test_gpu_ref_edges.py uploads to the
device — so that the CPU suite pins the layout the GPU test pins — and the placed windows of that test through the emulated kernels against the oracle."""
import ctypes as C

import numpy as np
import pytest

import emu_lib
import oracle_lib
import ref_edges_lib as rel
from aardvark_amd._abi import ref_packed_sizes


def emu_ref_packed(contigs, words_short=0, flags_short=0):
    lib = emu_lib.load()
    cs = oracle_lib.ContigSet(contigs)
    n_words, n_flags = ref_packed_sizes(sum(len(c) for c in contigs))
    words, flags = np.zeros(max(n_words, 1), np.uint32), np.zeros(n_flags, np.uint32)
    u32p = C.POINTER(C.c_uint32)
    lib.emu_ref_packed.argtypes = [C.POINTER(oracle_lib.u8p), oracle_lib.u64p, C.c_uint32, u32p, C.c_uint64, u32p, C.c_uint64]
    rc = lib.emu_ref_packed(cs.ptrs, cs.lens, cs.n, words.ctypes.data_as(u32p), n_words - words_short, flags.ctypes.data_as(u32p), n_flags - flags_short)
    return rc, words[:n_words], flags


def test_numpy_reference_on_a_hand_made_case():
    """the layout as include/aardvark_amd.h words it, on bytes written out by hand: bases 0 .. 7 are ACGTTGNa, 8 .. 16 nine C, 17 .. 32 sixteen T, 33 a G"""
    words, flags = rel.pack_reference_np([b"ACGTT", b"GN", b"a" + b"C" * 9 + b"T" * 16 + b"G"])
    assert words.tolist() == [0 | 1 << 2 | 2 << 4 | 3 << 6 | 3 << 8 | 2 << 10 | 0x5555 << 16, 1 | 0xFFFFFFFC, 3 | 2 << 2]
    assert flags.tolist() == [0b001] + [0] * 7
    words, flags = rel.pack_reference_np([])
    assert words.size == 0 and flags.tolist() == [0] * 8
    words, flags = rel.pack_reference_np([b"A" * (16 * 33 - 1) + b"y"])
    assert not words.any() and flags.tolist() == [0, 1] + [0] * 7


def test_emulator_copy_word_for_word():
    for contigs in rel.edge_references():
        rc, words, flags = emu_ref_packed(contigs)
        want_words, want_flags = rel.pack_reference_np(contigs)
        assert rc == 0 and np.array_equal(words, want_words) and np.array_equal(flags, want_flags), sum(len(c) for c in contigs)
    assert emu_ref_packed(contigs, flags_short=1)[0] == -1 and emu_ref_packed(rel.edge_references()[0], words_short=1)[0] == -1


@pytest.mark.parametrize("place", ["before", "word_after"])
def test_placed_windows_through_the_emulated_kernels(oracle, place):
    """the windows at contig, word and flag-word edges (two of the seven variants: the emulated lanes take their time) through the emulated lane, quad, pair and
    wide code, which reads the copy the test above pins: the oracle's outputs, and a flagged word turns away the windows that touch it and no others"""
    contigs, batch, info = rel.placed_windows(place)
    want = oracle_lib.compare_batch(oracle, batch, contigs, threads=8)
    got = emu_lib.compare_batch(batch, contigs, threads=8)
    assert got.diff(want) == []
    flags = emu_ref_packed(contigs)[2]
    flagged = rel.window_flagged(info, flags)
    assert got.lane_solved + got.wide_solved <= int((~rel.window_flagged(info, flags, pairs_looked_up=True)).sum())
    if place == "word_after":
        assert not flagged.any() and got.lane_solved >= batch.n_regions // 2 and got.wide_solved >= batch.n_regions // 6
    else:
        assert 0 < flagged.sum() < flagged.size and got.lane_solved > 0 and got.wide_solved > 0
