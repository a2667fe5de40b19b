"""The sequence-context labels of a stratified job on the CPU: the lane function of aardvark_amd/csrc/avk_context.inl, run over the emulator's copy of the
reference layout (tests/emu/context_emu.cpp), against the numpy restatement of the rule (tests/context_lib.py) — bit for bit; the 2-bit route against the byte
route; the stores into the masks the BED labels' kernel left; the spec's refusals and the stable names (host-only calls into the library); the summary writer
with names given as an array."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import context_emu_lib as emu
import context_lib as cl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPECS = {"default": cl.DEFAULT, "other": cl.OTHER, "same_pad": cl.SAME_PAD, "gc_only": cl.Spec(cl.DEFAULT.gc_edges, (), 50, 0), "hp_only": cl.Spec((), (4, 7, 12, 21), 0, 5)}


@pytest.fixture(scope="module", params=sorted(SPECS))
def job(request):
    return cl.Job(SPECS[request.param], 513)  # (the builder has asserted that the inputs reach every branch of the rule)


def test_lane_function_equals_the_numpy_rule(job):
    got = emu.region_bits(job.batch(), job.contigs, job.spec)
    assert np.array_equal(got, job.bits), [(r, hex(int(a)), hex(int(b))) for r, (a, b) in enumerate(zip(got, job.bits)) if a != b][:5]


def test_long_window_and_spans_outside_the_contig():
    """a span of 68,000 bases; spans that end beyond their contig or lie outside it are clamped, not read"""
    job = cl.Job(cl.DEFAULT, long=True)
    assert np.array_equal(emu.region_bits(job.batch(), job.contigs, job.spec), job.bits)
    n1 = len(job.contigs[1])
    spans = [(1, n1 - 3, n1 + 5_000), (1, n1 + 50, n1 + 60), (1, n1 + 2_000, n1 + 2_001), (0, 0, 2**63), (3, 0, 0), (2, 0, 63), (1, n1, n1 + 10)]
    want = [cl.bits_of_span(job.contigs, job.spec, c, (a, b)) for c, a, b in spans]
    assert want[1] == want[2] == 0 and want[0] != 0 and want[6] != 0  # (the last one: its pad alone reaches back into the contig)
    assert emu.span_bits(job.contigs, job.spec, spans).tolist() == want
    assert emu.span_bits(job.contigs, job.spec, [(4, 0, 10)]).tolist() == [0]  # a contig the reference lacks


def test_two_bit_route_equals_byte_route():
    """every placement of a window over all-ACGT words (starts and ends at every base offset, inside one word and across words, across the flag-word edge), and
    windows over flagged words: the counts by the 2-bit route are the counts by the bytes, and numpy's"""
    rng = np.random.default_rng(3)
    clean = [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 1100)), bytes(rng.choice(np.frombuffer(b"AACCCGT", np.uint8), 90))]
    dirty = bytearray(clean[0])
    for p in (3, 17, 40, 41, 500, 511, 512, 700):
        dirty[p] = ord("N") if p % 2 else dirty[p] | 0x20
    whole = b"".join(clean)
    windows = [(lo, lo + n) for lo in range(0, 34) for n in range(1, 50)] + [(lo, hi) for lo in (480, 495, 511, 512) for hi in (512, 513, 528, 545)] + [
        (1090, 1100), (1095, 1120), (1100, 1190), (0, 1190)]
    for contigs in ([clean[0], clean[1]], [bytes(dirty), clean[1]]):
        cat = b"".join(contigs)
        for lo, hi in windows:
            if lo < hi:
                packed, by_bytes = emu.counts(contigs, lo, hi, False), emu.counts(contigs, lo, hi, True)
                assert packed == by_bytes == cl.counts(cat[lo:hi]), (lo, hi)
    assert len(whole) == 1190


@pytest.mark.parametrize("n_bed", [0, 1, 31, 32, 33, 64, 70])
def test_stores_into_the_masks(job, n_bed):
    """the shared word is OR-ed into (the BED labels' bits stay), every later word is stored whole, and nothing else is touched"""
    n, n_ctx = job.n, job.spec.n_labels
    n_words = (n_bed + n_ctx + 31) // 32
    rng = np.random.default_rng(n_bed)
    mask = rng.integers(0, 2**32, (n_words + 1, n), dtype=np.uint64).astype(np.uint32)  # (a word of room behind the masks: stays as it is)
    bed_words = n_bed // 32
    if n_bed % 32:
        mask[bed_words] &= np.uint32((1 << (n_bed % 32)) - 1)  # what avk_strata_mask_kernel stores in the last BED word: nothing above the labels
    before = mask.copy()
    hits = emu.place(job.bits, n_bed, n_ctx, mask, fresh=n_bed == 0)
    assert hits == sum(bin(int(b)).count("1") for b in job.bits)
    want = before.copy()
    wide = job.bits.astype(np.uint64) << np.uint64(n_bed % 32)
    for w in range(bed_words, n_words):
        part = ((wide >> np.uint64(32 * (w - bed_words))) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        want[w] = (before[w] | part) if (w == bed_words and n_bed % 32) else part
    assert np.array_equal(mask, want)
    off, idx = cl.lists_of_bits(job.bits, n_bed)
    got = [[32 * w + j for w in range(bed_words, n_words) for j in range(32) if 32 * w + j >= n_bed and (int(mask[w, r]) >> j) & 1] for r in range(n)]
    assert got == [idx[int(off[r]):int(off[r + 1])].tolist() for r in range(n)]


def _lib():
    import aardvark_amd
    return aardvark_amd.load_library()


def test_spec_refusals_need_no_device():
    """AVK_E_ARG with nothing allocated and no context: the checks run in front of everything else"""
    lib = _lib()
    bad = [cl.Spec((0, 50, 50), (), 5, 5), cl.Spec((50, 20), (), 5, 5), cl.Spec((0, 102), (), 5, 5), cl.Spec((), (0, 3), 5, 5), cl.Spec((), (3, 3), 5, 5), cl.Spec((), (5, 4), 5, 5),
           cl.Spec((40,), (), 5, 5), cl.Spec((40,), (4,), 5, 5), cl.Spec((0, 101), (), 1025, 5), cl.Spec((), (4,), 5, 1025), cl.Spec((), (), 5, 5)]
    tree_off = np.zeros(1, np.uint64)
    for spec in bad:
        s, out = emu.c_spec(spec), C.c_void_p(7)
        rc = lib.avk_strata_upload_context(None, 0, 1, tree_off.ctypes.data_as(C.POINTER(C.c_uint64)), None, None, C.byref(s), C.byref(out))
        assert rc == -1 and not out.value, (spec.gc_edges, spec.hp_edges)
        assert b"context labels" in lib.avk_last_error(None)
        assert lib.avk_context_label_name(C.byref(s), 0, C.create_string_buffer(64), 64) == -1
    s = emu.c_spec(cl.DEFAULT)
    s.n_gc_edges = 18
    assert lib.avk_strata_upload_context(None, 0, 1, tree_off.ctypes.data_as(C.POINTER(C.c_uint64)), None, None, C.byref(s), C.byref(C.c_void_p())) == -1
    # a valid spec gets as far as the missing context; no contigs is refused before that
    good, out = emu.c_spec(cl.DEFAULT), C.c_void_p()
    assert lib.avk_strata_upload_context(None, 0, 0, tree_off.ctypes.data_as(C.POINTER(C.c_uint64)), None, None, C.byref(good), C.byref(out)) == -1
    assert b"n_contigs" in lib.avk_last_error(None)
    assert lib.avk_strata_upload_context(None, 0, 4, tree_off.ctypes.data_as(C.POINTER(C.c_uint64)), None, None, C.byref(good), C.byref(out)) == -1
    assert b"context missing" in lib.avk_last_error(None)
    assert lib.avk_strata_n_context_labels(None) == 0


def test_names():
    from aardvark_amd import ContextSpec
    spec = ContextSpec()
    assert (spec.gc_edges, spec.hp_edges, spec.gc_pad, spec.hp_pad) == (cl.DEFAULT.gc_edges, cl.DEFAULT.hp_edges, 50, 5) and spec.n_labels == 16
    assert spec.names() == cl.DEFAULT.names() == ["ctx_gc_0_15", "ctx_gc_15_20", "ctx_gc_20_25", "ctx_gc_25_30", "ctx_gc_30_55", "ctx_gc_55_60", "ctx_gc_60_65", "ctx_gc_65_70",
                                                   "ctx_gc_70_75", "ctx_gc_75_80", "ctx_gc_80_85", "ctx_gc_85_101", "ctx_hp_4_6", "ctx_hp_7_11", "ctx_hp_12_20", "ctx_hp_ge21"]
    for s in (cl.OTHER, cl.SAME_PAD, SPECS["gc_only"], SPECS["hp_only"], cl.Spec((), (9,), 0, 0)):
        assert ContextSpec(s.gc_edges, s.hp_edges, s.gc_pad, s.hp_pad).names() == s.names()
    lib, s = _lib(), emu.c_spec(cl.DEFAULT)
    buf = C.create_string_buffer(64)
    assert lib.avk_context_label_name(C.byref(s), 16, buf, 64) == -1  # beyond the labels
    assert lib.avk_context_label_name(C.byref(s), 0, buf, 11) == -1 and lib.avk_context_label_name(C.byref(s), 0, buf, 12) == 0 and buf.value == b"ctx_gc_0_15"
    with pytest.raises(ValueError):
        ContextSpec((0, 0), ()).names()


def test_summary_named_equals_summary_stratified(tmp_path):
    """the same blocks under the sets' own names: byte for byte the stratified writer's file; further blocks follow under the names given"""
    from aardvark_amd import TALLY_LEN, feeder
    strat = feeder.Stratifications(os.path.join(ROOT, "tests", "golden", "example_stratification", "strat.tsv"))
    try:
        rng = np.random.default_rng(8)
        tally = rng.integers(0, 1000, TALLY_LEN).astype(np.uint64)
        n = len(strat.labels)
        blocks = rng.integers(0, 500, (n + 3, TALLY_LEN)).astype(np.uint64)
        blocks[n + 1] = 0
        for ext in ("tsv", "csv"):
            a, b, c = (str(tmp_path / ("%s.%s" % (k, ext))) for k in "abc")
            feeder.write_summary_stratified(a, tally, strat, blocks[:n], "job", 31)
            feeder.write_summary_named(b, tally, list(strat.labels), blocks[:n], "job", 31)
            assert open(a, "rb").read() == open(b, "rb").read()
            names = list(strat.labels) + ["ctx_gc_0_15", "ctx_hp_4_6", "ctx_hp_ge21"]
            feeder.write_summary_named(c, tally, names, blocks, "job", 31)
            text = open(c).read()
            assert text.startswith(open(a).read())
            sep = "," if ext == "csv" else "\t"
            rows = [l.split(sep) for l in text.splitlines()[1:]]
            order = [r[2] for r in rows]
            assert [x for i, x in enumerate(order) if i == 0 or order[i - 1] != x] == ["ALL"] + names
            first = next(r for r in rows if r[2] == "ctx_gc_0_15" and r[1] == "GT" and r[4] == "ALL")
            want = blocks[n].reshape(-1)
            assert int(first[5]) == int(first[6]) + int(first[7]) and int(first[6]) in want.tolist()
        feeder.write_summary_named(str(tmp_path / "none.tsv"), tally, [], np.zeros(0, np.uint64), "job", 31)
        feeder.write_summary(str(tmp_path / "plain.tsv"), tally, "job", 31)
        assert open(str(tmp_path / "none.tsv"), "rb").read() == open(str(tmp_path / "plain.tsv"), "rb").read()
    finally:
        strat.close()


def test_sanitizer_program(tmp_path):
    """tests/native/context_check.cpp: the lane function over placed windows, on arrays exactly as long as it may read, built with -fsanitize=address,undefined
    and run as a program of its own (nothing is loaded into Python under a sanitizer)"""
    exe = str(tmp_path / "context_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-Wno-unknown-pragmas",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "native", "context_check.cpp")])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(out.stdout)
    assert out.returncode == 0 and "context_check: ok" in out.stdout


# what the tool refuses, by name, before it loads anything: (arguments, a piece of the message)
TOOL_REFUSALS = [(["--context-strata", "gc,hp", "--strat-lists", "host"], "cannot be combined with --strat-lists host"),
                 (["--context-strata", "gc", "--batch-form", "wide"], "cannot be combined with --batch-form wide"),
                 (["--context-strata", "hp", "--output-debug", "/nonexistent/dbg"], "cannot be combined with --output-debug"),
                 (["--context-strata", "tandem"], "--context-strata takes gc, hp or gc,hp"),
                 (["--context-gc-pad", "10"], "need --context-strata"),
                 (["--context-strata", "gc", "--context-gc-edges", "50,20"], "not strictly ascending"),
                 (["--context-strata", "gc", "--context-gc-edges", "0,102"], "above 101"),
                 (["--context-strata", "hp", "--context-hp-edges", "0,4"], "a run edge of 0"),
                 (["--context-strata", "hp", "--context-hp-pad", "1025"], "a pad above 1024"),
                 (["--context-strata", "gc", "--context-gc-edges", "7"], "one GC edge makes no label"),
                 (["--context-strata", "gc", "--context-gc-edges", "1,x"], "invalid value for --context-gc-edges")]


def test_tool_refusals_need_no_device(tmp_path):
    """aardvark_amd_compare refuses --context-strata off its one route, and a bad spec, with exit code 64 and a message — before a file is read or a context made"""
    cli = os.path.join(ROOT, "aardvark_amd", "bin", "aardvark_amd_compare")
    for extra, text in TOOL_REFUSALS:
        r = subprocess.run([cli, "-r", "none.fa", "-t", "none.vcf", "-q", "none.vcf", "-o", str(tmp_path / "out")] + extra, capture_output=True, text=True)
        assert r.returncode == 64 and text in r.stderr, (extra, r.returncode, r.stderr)
