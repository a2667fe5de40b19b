"""Stratified tallies from the compact results (aardvark_amd/csrc/avk_labels.inl), without a GPU: the per-region rule and the label loop of the gfx950 kernel run
on the CPU (tests/emu/label_emu.cpp) on a device view filled from the ORACLE's results, against the oracle's own 13 x 22 blocks; the host-side shard helper; the
refusals that need no device.  All comparisons are exact.

Mutation report (each line of avk_labels.inl changed alone, the library rebuilt, this file run): which test notices
  query toggle dropped (`query ? oa : ea` -> `ea`, same for obs)  test_region_blocks_equal_the_oracles[fuzz], [fuzz-packed-source], [case-files]; test_label_sums_*
  `if (obs > 0)` of the fn_gt counter -> `if (exp > 0)`           test_region_blocks_equal_the_oracles[fuzz], [fuzz-packed-source], [case-files]; test_label_sums_*
  type-order walk of the groups (`++k` dropped: always the joint group)  test_region_blocks_equal_the_oracles (all three: regions with several call types), test_label_sums_*
  `2 * T.tot` -> `T.tot`                                          test_region_blocks_equal_the_oracles (all three), test_label_sums_*
  a label listed twice counted once (`break` after the first add)  test_label_sums_equal_sums_of_the_oracles_blocks only (the blocks are right: the loop over the list is wrong)
  status test dropped (`region_out[4 * r] != 0` -> never)          test_label_sums_equal_sums_of_the_oracles_blocks only (two labelled regions are shown as AVK_ST_CAPACITY
                                                                  with their words and groups in place; regions that fail validation own no groups and add nothing)
"""
import ctypes as C

import numpy as np
import pytest

import aardvark_amd
import escapes_lib
import label_emu_lib
import oracle_lib
import scenarios
from aardvark_amd import dist, synth
from aardvark_amd._abi import TALLY_LEN, AvkCompareConfig, AvkPackedBatch, AvkPackedEscapes, AvkRegionLabels, AvkResultBatch, region_labels

WORDS = label_emu_lib.WORDS
HOM_ALT = 5


def copies(z):
    return 2 if z == HOM_ALT else (1 if 2 <= z <= 4 else 0)


def fuzz_input():
    """the fuzzed regions, plus the invalid ones of scenarios.invalid_regions (status != 0: they must contribute nothing)"""
    contigs, batch = scenarios.fuzz_regions(341, 400, max_vars=9, max_len=12)
    bad_contigs, bad = scenarios.invalid_regions()
    assert len(bad_contigs[0]) <= len(contigs[0])
    # the invalid regions are written for their own short contig: on the long one they keep every defect but "window past the contig end"
    return contigs, synth.concat_batches([batch, bad])


def case_files_input(tmp_path):
    from test_feeder import write_case_files
    _, contig, batch = write_case_files(tmp_path, 2500, 1_200_000)
    return [contig], batch


@pytest.fixture(scope="module")
def solved(tmp_path_factory):
    """the two inputs, each with the oracle's results: computed once, shared, never changed"""
    orc = oracle_lib.load()
    out = {}
    for name, (contigs, batch) in (("fuzz", fuzz_input()), ("case-files", case_files_input(tmp_path_factory.mktemp("case")))):
        res = oracle_lib.compare_batch(orc, batch, contigs, threads=8)
        for f in ("status", "group_metrics", "var_expected", "var_observed"):
            getattr(res, f).setflags(write=False)
        out[name] = (batch, res)
    return out


def call_range(batch, r):
    return [int(batch.t_off[r]) + i for i in range(int(batch.t_cnt[r]))] + [int(batch.q_off[r]) + i for i in range(int(batch.q_cnt[r]))]


def test_inputs_cover_the_rule(solved):
    """from the oracle's results alone: several call types in one region, every copies class, a raw space that is not the longer allele, unsolved regions"""
    seen_copies, multi_type, raw_differs, unsolved = set(), 0, 0, 0
    for batch, res in solved.values():
        for r in range(batch.n_regions):
            calls = call_range(batch, r)
            seen_copies |= set(copies(int(batch.var_zyg[v])) for v in calls)
            raw_differs += sum(int(batch.var_raw_space[v]) != max(int(batch.a0_len[v]), int(batch.a1_len[v])) for v in calls)
            if int(res.status[r]) != 0:
                unsolved += 1
                assert not res.group_metrics[r].any()
            elif len(set(int(batch.var_type[v]) for v in calls)) > 1:
                multi_type += 1
    assert seen_copies == {0, 1, 2} and multi_type >= 20 and raw_differs >= 1 and unsolved >= 1


@pytest.mark.parametrize("which", ["fuzz", "fuzz-packed-source", "case-files"])
def test_region_blocks_equal_the_oracles(solved, which):
    """every solved region's 286 words from lb_region_groups equal the oracle's block; unsolved regions get nothing"""
    batch, res = solved[which.replace("-packed-source", "")]
    view, keep = label_emu_lib.device_view(batch, res, packed_source=which.endswith("packed-source"))
    got = label_emu_lib.blocks(view, batch.n_regions)
    want = np.asarray(res.group_metrics).reshape(batch.n_regions, WORDS)
    ok = np.asarray(res.status) == 0
    assert ok.sum() > 300
    bad = [r for r in np.nonzero(ok)[0] if not np.array_equal(got[r], want[r])]
    assert not bad, "region %d: fields %s" % (bad[0], np.nonzero(got[bad[0]] != want[bad[0]])[0])
    assert not got[~ok].any()


def label_lists(n, n_labels, seed, unsolved):
    """random label lists: intervals of regions per label, plus label 0 on every region, label 1 on none, region 0 with an empty list, one region under every
    label and more, repeats inside lists, and every unsolved region labelled"""
    rng = np.random.default_rng(seed)
    lists = [[0] for _ in range(n)]
    for l in range(2, n_labels):
        for _ in range(3):
            a = int(rng.integers(0, n))
            for r in range(a, min(n, a + int(rng.integers(1, max(2, n // 6))))):
                lists[r].append(l)
    lists[0] = []
    lists[n // 2] = [l for l in range(n_labels) if l != 1] + [0, n_labels - 1]  # every label but the empty one, two of them twice
    for r in range(3, n, 17):
        if lists[r]:
            lists[r].append(lists[r][-1])  # a label named twice counts twice
    for r in unsolved:
        lists[r] = lists[r] + [0, n_labels - 1]
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in lists])
    return off, np.array([l for x in lists for l in x], np.uint32), lists


def oracle_sums(res, lists, n_labels, skip=()):
    want = np.zeros((n_labels, TALLY_LEN), np.uint64)
    for r, ls in enumerate(lists):
        if int(res.status[r]) != 0 or r in skip:
            continue
        for l in ls:
            want[l, :WORDS] += np.asarray(res.group_metrics[r]).reshape(-1).astype(np.uint64)
    return want


@pytest.mark.parametrize("n_labels,block", [(1, 1), (7, 7), (7, 3), (20, 16), (33, 16)])
def test_label_sums_equal_sums_of_the_oracles_blocks(solved, n_labels, block):
    """lb_region_labels launch by launch (labels in blocks of `block`): sums of the oracle's blocks over the regions each label names; words 286 and 287 untouched;
    sums are added"""
    batch, res = solved["fuzz"]
    unsolved = [int(r) for r in np.nonzero(np.asarray(res.status) != 0)[0]]
    assert unsolved
    off, idx, lists = label_lists(batch.n_regions, n_labels, 5 + n_labels, unsolved)
    # two solved regions with labels are shown as AVK_ST_CAPACITY: words and groups in place, and they must not count
    starved = [r for r in range(batch.n_regions) if int(res.status[r]) == 0 and lists[r] and np.asarray(res.group_metrics[r]).any()][10:12]
    assert len(starved) == 2
    view, keep = label_emu_lib.device_view(batch, res, starved=starved)
    want = oracle_sums(res, lists, n_labels, skip=starved)
    assert want[0].any()
    out = np.zeros((n_labels, TALLY_LEN), np.uint64)
    out[:, WORDS:] = 99
    label_emu_lib.tally(view, n_labels, off, idx, block, out=out)
    assert np.array_equal(out[:, :WORDS], want[:, :WORDS]) and (out[:, WORDS:] == 99).all()
    if n_labels > 1:
        assert not out[1, :WORDS].any()
    label_emu_lib.tally(view, n_labels, off, idx, block, out=out)
    assert np.array_equal(out[:, :WORDS], 2 * want[:, :WORDS])


# ---- avk_packed_shard_labels ------------------------------------------------------------------------------------------------------------------------
P = C.POINTER


def shard_lib():
    lib = aardvark_amd.load_library()
    lib.avk_packed_shard_make_esc.argtypes = [P(AvkPackedBatch), P(AvkPackedEscapes), P(C.c_uint64), C.c_uint64, C.c_uint32, C.c_uint32, P(C.c_void_p)]
    lib.avk_packed_shard_regions.restype = C.c_uint64
    lib.avk_packed_shard_regions.argtypes = [C.c_void_p, P(P(C.c_uint64))]
    lib.avk_packed_shard_free.argtypes = [C.c_void_p]
    lib.avk_packed_shard_labels.argtypes = [C.c_void_p, P(AvkRegionLabels), P(C.c_uint64), P(C.c_uint32)]
    return lib


@pytest.mark.parametrize("world", [2, 3])
def test_shard_labels_follow_index_in_whole(world):
    """the gathered lists equal a Python gather by index_in_whole, on a job with escapes; the offsets-only call sizes the index array; an empty shard works"""
    lib = shard_lib()
    contigs, batch = escapes_lib.indel_mix_job(n_truth=400, contig_len=400_000)
    _, pb = escapes_lib.escaped(batch)
    assert not pb.escapes.empty()
    n = pb.n_regions
    off, idx, lists = label_lists(n, 9, 3, [])
    lab, keep = region_labels(9, off, idx)
    st, esc = pb.c_struct(), pb.c_escapes()
    ids = np.arange(n, dtype=np.uint64)
    seen = 0
    for rank in range(world):
        h = C.c_void_p()
        assert lib.avk_packed_shard_make_esc(C.byref(st), C.byref(esc), ids.ctypes.data_as(P(C.c_uint64)), 0, rank, world, C.byref(h)) == 0
        where = P(C.c_uint64)()
        m = int(lib.avk_packed_shard_regions(h, C.byref(where)))
        index = [int(where[k]) for k in range(m)]
        soff = np.full(m + 2, 77, np.uint64)
        assert lib.avk_packed_shard_labels(h, C.byref(lab), soff.ctypes.data_as(P(C.c_uint64)), None) == 0  # offsets only
        want = [lists[r] for r in index]
        assert soff[m + 1] == 77 and list(soff[:m + 1]) == list(np.concatenate([[0], np.cumsum([len(x) for x in want])]))
        sidx = np.full(int(soff[m]) + 1, 0xFFFF, np.uint32)
        assert lib.avk_packed_shard_labels(h, C.byref(lab), soff.ctypes.data_as(P(C.c_uint64)), sidx.ctypes.data_as(P(C.c_uint32))) == 0
        assert sidx[-1] == 0xFFFF and list(sidx[:-1]) == [l for x in want for l in x]
        # the Python wrapper beside the shard functions
        _, woff, widx = dist.shard_labels(lib, h, 9, off, idx)
        assert np.array_equal(woff, soff[:m + 1]) and np.array_equal(widx, sidx[:-1])
        seen += m
        lib.avk_packed_shard_free(h)
    assert seen == n
    # a rank that owns nothing: every region id hashes to rank 0 of 2
    zero_ids = np.array([i for i in range(4 * n) if dist.region_hash([i])[0] % np.uint64(2) == 0][:n], np.uint64)
    h = C.c_void_p()
    assert lib.avk_packed_shard_make_esc(C.byref(st), C.byref(esc), zero_ids.ctypes.data_as(P(C.c_uint64)), 0, 1, 2, C.byref(h)) == 0
    assert lib.avk_packed_shard_regions(h, None) == 0
    soff = np.full(2, 77, np.uint64)
    assert lib.avk_packed_shard_labels(h, C.byref(lab), soff.ctypes.data_as(P(C.c_uint64)), None) == 0 and list(soff) == [0, 77]
    lib.avk_packed_shard_free(h)


# ---- refusals that need no device ---------------------------------------------------------------------------------------------------------------------
def refusal_cases(n):
    """(name, off, idx or None, tallies given, text of the message) for a batch of n regions and 4 labels"""
    good_off = np.arange(n + 1, dtype=np.uint64)
    good_idx = (np.arange(n) % 4).astype(np.uint32)
    down = good_off.copy()
    down[n // 2] = down[n // 2 + 1] + 1
    big = good_idx.copy()
    big[n - 1] = 4
    return [("decreasing label_off", down, good_idx, True, "label_off must not decrease"), ("index out of range", good_off, big, True, "label index 4 of 4"),
            ("label_idx missing", good_off, None, True, "label_idx missing"), ("label_tallies missing", good_off, good_idx, False, "label_tallies missing")]


@pytest.mark.parametrize("entry", ["avk_compare_packed_labels", "avk_compare_packed_submit_labels"])
def test_refusals_come_before_anything_else(entry):
    """the four refusals are AVK_E_ARG (-1) before a context is even looked at (so they need no device), with their text in avk_last_error(NULL)"""
    lib = aardvark_amd.load_library()
    contigs, batch = scenarios.fuzz_regions(2, 12, max_vars=2)
    pb = aardvark_amd.PackedBatch.from_compact(aardvark_amd.CompactBatch.from_region_batch(batch))
    st, cfg = pb.c_struct(), AvkCompareConfig(50, 0, 0)
    res = aardvark_amd.ResultBatch(pb, sequences=False, group_metrics=False)
    ro = res.c_struct()
    sums = np.zeros((4, TALLY_LEN), np.uint64)
    for name, off, idx, with_sums, text in refusal_cases(pb.n_regions):
        lab = AvkRegionLabels(4, off.ctypes.data_as(P(C.c_uint64)), idx.ctypes.data_as(P(C.c_uint32)) if idx is not None else None)
        args = [None, C.byref(st), None, C.byref(lab), C.byref(cfg), C.byref(ro), sums.ctypes.data_as(P(C.c_uint64)) if with_sums else None]
        if entry.endswith("submit_labels"):
            args.append(C.byref(C.c_void_p()))
        getattr(lib, entry).argtypes = None
        assert getattr(lib, entry)(*args) == -1, name
        assert text in lib.avk_last_error(None).decode(), name
    assert not sums.any()
