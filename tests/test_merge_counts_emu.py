"""The merge summary counters by kernel (aardvark_amd/csrc/avk_mergecount.inl), without a GPU: the per-slot function the gfx950 kernel runs, compiled for the CPU
(tests/emu/mergecount_emu.cpp), on the arrays the device holds behind the classification kernel, against the host's avk_merge_counts_esc and against a statement
of MergeSummaryWriter::add_merge_benchmark in Python; the reason numbering against the reference's order on the four strategy cases of
tests/golden/merge_crosscheck.json.  All comparisons are exact.

Mutation report (each line of avk_mergecount.inl changed alone, the emulator library rebuilt, this file run): which tests notice
  pass and fail swapped (`? 0u : 1u` -> `? 1u : 0u`)                      test_counts_equal_the_hosts[2], [3], [5], [8]; test_conflict_selection_members_is_an_index;
                                                                          test_unsolved_regions_and_empty_slots; test_refusals
  `members == input` read as a bit test (`(members >> input) & 1`)         test_counts_equal_the_hosts (all four); test_conflict_selection_members_is_an_index
  a region with non-zero status counted (`if (!solved) return run;` off)   test_counts_equal_the_hosts (all four); test_unsolved_regions_and_empty_slots
  runs of one type added as 1 (`n = len` -> `n = 1u` in mc_next)           test_counts_equal_the_hosts (all four: the escaped slot of 300 calls of one type);
                                                                          test_conflict_selection_members_is_an_index; test_unsolved_regions_and_empty_slots
  the type nibble not masked (`& 15u` dropped where mc_next reads `vt`)    every test that counts (each call carries a zygosity in the high nibble)
  the type test dropped (`bad` never set)                                  test_refusals only
"""
import json
import os

import numpy as np
import pytest

import aardvark_amd
import mergecount_emu_lib as mc

XMERGE = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "merge_crosscheck.json")))
CLS_OF = {"Different": mc.DIFFERENT, "BasepairIdentical": mc.IDENTICAL, "NoConflict": mc.NO_CONFLICT, "MajorityAgree": mc.MAJORITY, "ConflictSelection": mc.CONFLICT_SELECTION}


@pytest.fixture(scope="module")
def lib():
    return aardvark_amd.load_library()


def random_job(k, seed, n=240):
    """slots with 0 to 4 calls (a third of them empty), all 12 types in turn, one escaped slot of 300 calls of one type in a solved region, every classification"""
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, 5, n * k) * (rng.random(n * k) > 0.33)
    counts[7 * k + 1] = 300
    nv = int(counts.sum())
    types = (np.arange(nv) * 5 + rng.integers(0, 2, nv)) % 12
    at = int(counts[:7 * k + 1].sum())
    types[at:at + 300] = 2
    pmb = mc.packed_batch(k, counts, types)
    assert pmb.escapes.esc_slot.tolist() == [7 * k + 1] and pmb.in_cnt[7 * k + 1] == 0
    status, cls, members = mc.random_results(rng, n, k)
    status[7] = 0
    return pmb, status, cls, members


@pytest.mark.parametrize("k", [2, 3, 5, 8])
def test_counts_equal_the_hosts(lib, k):
    pmb, status, cls, members = random_job(k, 100 + k)
    assert set(cls.tolist()) == {0, 1, 2, 3, 4} and (status != 0).any() and set((pmb.var_type_zyg & 15).tolist()) == set(range(12))
    view, keep = mc.device_view(pmb, status, cls, members)
    got, err = mc.emu_counts(view, k)
    want = mc.host_counts(lib, pmb, status, cls, members)
    assert err == 0 and got.size == want.size == mc.merge_counts_len(lib, k)
    assert np.array_equal(got, want)
    assert np.array_equal(want, mc.python_counts(pmb, status, cls, members))
    solved_calls = sum(int(c) for r in range(pmb.n_regions) if status[r] == 0 for c in keep["in_cnt"][r * k:(r + 1) * k])
    assert int(got.sum()) == solved_calls


def test_conflict_selection_members_is_an_index(lib):
    """ConflictSelection{index}: members 1 selects input 1 (as a mask it would name input 0), members 2 input 2 (as a mask: input 1)"""
    k = 3
    pmb = mc.packed_batch(k, [1, 1, 1, 2, 1, 1], [0, 0, 0, 1, 1, 1, 1])
    status, cls, members = np.zeros(2, np.int32), np.full(2, mc.CONFLICT_SELECTION, np.uint8), np.array([1, 2], np.uint64)
    view, _ = mc.device_view(pmb, status, cls, members)
    got, err = mc.emu_counts(view, k)
    assert err == 0 and np.array_equal(got, mc.host_counts(lib, pmb, status, cls, members))
    entry = lambda reason, t, i, fail: ((reason * 12 + t) * k + i) * 2 + fail
    base = 1 + 2 * 8
    want = np.zeros_like(got)
    for e, n in ((entry(base + 1, 0, 0, 1), 1), (entry(base + 1, 0, 1, 0), 1), (entry(base + 1, 0, 2, 1), 1), (entry(base + 2, 1, 0, 1), 2), (entry(base + 2, 1, 1, 1), 1),
                 (entry(base + 2, 1, 2, 0), 1)):
        want[e] = n
    assert np.array_equal(got, want)


def test_unsolved_regions_and_empty_slots(lib):
    """a batch whose regions are all unsolved adds nothing; a batch of empty slots adds nothing; one solved region among them adds its calls alone"""
    k = 2
    pmb = mc.packed_batch(k, [3, 0, 0, 0, 2, 2], [0, 0, 0, 4, 4, 5, 5])
    cls, members = np.array([mc.IDENTICAL, mc.IDENTICAL, mc.NO_CONFLICT], np.uint8), np.array([0, 0, 1], np.uint64)
    for status, total in (([7, 3, 21], 0), ([7, 0, 21], 0), ([0, 3, 21], 3), ([7, 3, 0], 4)):
        st = np.array(status, np.int32)
        view, _ = mc.device_view(pmb, st, cls, members)
        got, err = mc.emu_counts(view, k)
        assert err == 0 and int(got.sum()) == total
        assert np.array_equal(got, mc.host_counts(lib, pmb, st, cls, members))


def test_counts_are_added(lib):
    pmb, status, cls, members = random_job(3, 9, n=40)
    view, _ = mc.device_view(pmb, status, cls, members)
    once, _ = mc.emu_counts(view, 3)
    start = np.arange(once.size, dtype=np.uint64) * np.uint64(3) + np.uint64(2 ** 40)
    twice, err = mc.emu_counts(view, 3, out=start.copy())
    assert err == 0 and np.array_equal(twice, start + once)


def test_refusals(lib):
    """what the kernel's error word says, beside the host function's answer for the same arrays"""
    k = 2
    status, cls, members = np.zeros(2, np.int32), np.array([mc.IDENTICAL, mc.DIFFERENT], np.uint8), np.zeros(2, np.uint64)
    # a type nibble of 12 in a solved region: both refuse
    pmb = mc.packed_batch(k, [1, 1, 1, 1], [0, 12, 0, 0])
    view, _ = mc.device_view(pmb, status, cls, members)
    assert mc.emu_counts(view, k)[1] == mc.ERR_TYPE
    with pytest.raises(ValueError):
        mc.host_counts(lib, pmb, status, cls, members)
    # ... in an unsolved region: the host function never looks at the call; the kernel refuses the batch (include/aardvark_amd.h, avk_merge_packed_counts)
    st = np.array([3, 0], np.int32)
    view, _ = mc.device_view(pmb, st, cls, members)
    assert mc.emu_counts(view, k)[1] == mc.ERR_TYPE
    assert int(mc.host_counts(lib, pmb, st, cls, members).sum()) == 2
    # nibbles 0..11 with every zygosity in the high nibble are fine
    pmb = mc.packed_batch(k, [6, 6, 0, 0], list(range(12)), zyg=15)
    view, _ = mc.device_view(pmb, status, cls, members)
    got, err = mc.emu_counts(view, k)
    assert err == 0 and np.array_equal(got, mc.host_counts(lib, pmb, status, cls, members)) and int(got.sum()) == 12
    # a classification that is none, a ConflictSelection index that is no input: both refuse, for solved regions only
    pmb = mc.packed_batch(k, [1, 1, 1, 1], [0, 0, 0, 0])
    for bad_cls, bad_mem in ((5, 0), (mc.CONFLICT_SELECTION, 2)):
        c2, m2 = np.array([bad_cls, mc.DIFFERENT], np.uint8), np.array([bad_mem, 0], np.uint64)
        view, _ = mc.device_view(pmb, status, c2, m2)
        assert mc.emu_counts(view, k)[1] == mc.ERR_CLASS
        with pytest.raises(ValueError):
            mc.host_counts(lib, pmb, status, c2, m2)
        view, _ = mc.device_view(pmb, np.array([3, 0], np.int32), c2, m2)
        assert mc.emu_counts(view, k)[1] == 0
    # a slot whose calls are not inside the batch (the widened arrays of a batch the upload would have refused)
    view, keep = mc.device_view(pmb, status, cls, members)
    keep["in_cnt"][3] = 2
    assert mc.emu_counts(view, k)[1] == mc.ERR_RANGE
    keep["in_cnt"][3] = 1
    keep["in_off"][0] = 5
    assert mc.emu_counts(view, k)[1] == mc.ERR_RANGE


def test_reason_numbering_on_the_known_answer_cases(lib):
    """the four strategy cases of merge_crosscheck.json (regions of four and five call sets, every classification): the shared numbering (avk_merge_reason.h) through
    the library and through the emulator, against the reference's order written down in Python; and for every k the numbering is the dense order of the keys"""
    api = mc.merge_counts_len(lib, 2) and lib  # (declares the argument types)
    emu = mc.load()
    seen = set()
    assert len(XMERGE["cases"]) == 4
    for case in XMERGE["cases"]:
        for region, e in zip(XMERGE["regions"], case["expect"]):
            k = len(region["inputs"])
            cls = CLS_OF[e[0]]
            members = 0 if len(e) == 1 else (int(e[1]) if cls == mc.CONFLICT_SELECTION else sum(1 << i for i in e[1]))
            want = mc.python_reason(k, cls, members)
            assert api.avk_merge_counts_reason(k, cls, members) == want == emu.mergecount_emu_reason(k, cls, members)
            seen.add(e[0])
    assert seen == set(CLS_OF)
    for k in range(2, 11):
        keys = [(mc.DIFFERENT, 0)] + [(mc.NO_CONFLICT, m) for m in range(2 ** k)] + [(mc.MAJORITY, m) for m in range(2 ** k)] + [(mc.CONFLICT_SELECTION, i) for i in range(k)] + [(mc.IDENTICAL, 0)]
        assert [emu.mergecount_emu_reason(k, c, m) for c, m in keys] == list(range(len(keys)))
        assert emu.mergecount_emu_words(k) == len(keys) * 12 * k * 2 == mc.merge_counts_len(lib, k)


def test_lds_rule_is_a_function_of_k_and_the_lds_size():
    emu = mc.load()
    fits = lambda k, b: emu.mergecount_emu_fits_lds(k, b) == 1
    assert [k for k in range(2, 9) if fits(k, 160 * 1024)] == [2, 3, 4, 5, 6]
    assert [k for k in range(2, 9) if fits(k, 64 * 1024)] == [2, 3, 4]
    for k in range(2, 9):
        b = int(emu.mergecount_emu_words(k)) * 8
        assert fits(k, b) and not fits(k, b - 1)
