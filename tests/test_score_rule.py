"""The rule of the curve by query score (aardvark_amd/csrc/avk_score.h) without a GPU: spec validation, the header's bin() at every edge
against the restatement of tests/score_lib.py, the points' names, the attribution cases and the lost values on hand-made results, the host route
avk_score_tallies_host against the restatement on the ORACLE's per-call outputs — whole, on threads, with labels — and the three invariants (point 0 is the
tally; TP + FN of the truth side is the same at every point; TP and query fields do not grow with the threshold).  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import aardvark_amd
import oracle_lib
import scenarios
import score_lib
import size_lib
from aardvark_amd import RegionBatch, ResultBatch, ScoreSpec, _abi, score_tallies_host

u64p, f32p = C.POINTER(C.c_uint64), C.POINTER(C.c_float)
NAN, INF = float("nan"), float("inf")
INVALID = [(), tuple(range(32)), (NAN,), (1.0, NAN), (INF,), (1.0, INF), (-INF, 0.0), (3.0, 3.0), (1.0, 6.0, 6.0, 50.0), (6.0, 1.0), (0.0, -0.0)]


def test_spec_validation():
    lib, emu = aardvark_amd.load_library(), score_lib.load()
    for t in INVALID:
        assert not score_lib.valid(t)
        spec = score_lib.c_spec(t[:31], n=len(t))
        assert emu.score_emu_spec_ok(C.byref(spec)) == 0 and lib.avk_score_n_points(C.byref(spec)) == 0, t
        assert lib.avk_score_point_name(C.byref(spec), 0, C.create_string_buffer(32), 32) == -1
    for t in score_lib.SPECS:
        assert score_lib.valid(t) and emu.score_emu_spec_ok(C.byref(score_lib.c_spec(t))) == 1 and lib.avk_score_n_points(C.byref(score_lib.c_spec(t))) == len(t) + 1
    assert lib.avk_score_n_points(None) == 0 and lib.avk_score_block(None) == 0
    assert C.sizeof(_abi.AvkScoreSpec) == 128 and ScoreSpec().thresholds == tuple(float(x) for x in score_lib.DEFAULT)


@pytest.mark.parametrize("thresholds", score_lib.SPECS)
def test_bin_at_every_edge(thresholds):
    emu, spec = score_lib.load(), score_lib.c_spec(thresholds)
    K = len(thresholds)
    t32 = np.asarray(thresholds, np.float32)
    probes = [np.float32(x) for x in (NAN, INF, -INF, -0.0, 0.0)]
    for x in t32:
        probes += [x, np.nextafter(x, np.float32(-INF), dtype=np.float32), np.nextafter(x, np.float32(INF), dtype=np.float32)]
    hit = set()
    for s in probes:
        got = emu.score_emu_bin(C.byref(spec), C.c_float(float(s)))
        assert got == score_lib.bin_of(thresholds, s), float(s)
        hit.add(got)
    assert hit == set(range(K + 1))
    assert emu.score_emu_bin(C.byref(spec), C.c_float(NAN)) == 0 and emu.score_emu_bin(C.byref(spec), C.c_float(-INF)) == 0
    assert emu.score_emu_bin(C.byref(spec), C.c_float(INF)) == K
    for k, x in enumerate(t32):  # on the threshold: kept; one ulp below: not
        assert emu.score_emu_bin(C.byref(spec), C.c_float(float(x))) == k + 1
        assert emu.score_emu_bin(C.byref(spec), C.c_float(float(np.nextafter(x, np.float32(-INF), dtype=np.float32)))) == k


def test_names():
    assert ScoreSpec().names() == ["score_all", "score_ge_5", "score_ge_10", "score_ge_15", "score_ge_20", "score_ge_25", "score_ge_30", "score_ge_35", "score_ge_40",
                                   "score_ge_50", "score_ge_60"] == score_lib.names_of(score_lib.DEFAULT)
    odd = (-2.5, 0.0, 30.5, 1e6)
    assert ScoreSpec(odd).names() == ["score_all", "score_ge_-2.5", "score_ge_0", "score_ge_30.5", "score_ge_1e+06"] == score_lib.names_of(odd)
    lib, spec = aardvark_amd.load_library(), score_lib.c_spec(score_lib.DEFAULT)
    buf = C.create_string_buffer(10)
    assert lib.avk_score_point_name(C.byref(spec), 11, buf, 10) == -1 and lib.avk_score_point_name(C.byref(spec), 2, buf, 10) == -1  # "score_ge_10" needs 12 bytes
    assert lib.avk_score_point_name(C.byref(spec), 0, buf, 10) == 0 and buf.value == b"score_all"


# ---- hand-made results: the attribution cases and the lost values ---------------------------------------------------------------------------------------
def hand_case(truth, query, scores_q):
    """one region on one contig: truth = [(expected, observed, a0, a1)], query likewise (its STORED expected / observed: the toggled entries), scores of the
    query calls -> (batch, res, scores)"""
    variants = lambda calls: [(110 + 10 * i, a0, a1, 0 if len(a0) == len(a1) else 1, 2) for i, (_, _, a0, a1) in enumerate(calls)]  # (type and zygosity by ordinal)
    regions = [{"start": 100, "end": 400, "truth": variants(truth), "query": variants(query)}]
    batch = RegionBatch.from_regions(regions)
    res = ResultBatch(batch, sequences=False, group_metrics=False)
    res.status[:] = 0
    for side_off, calls in ((int(batch.t_off[0]), truth), (int(batch.q_off[0]), query)):
        for i, (ea, oa, _, _) in enumerate(calls):
            res.var_expected[side_off + i], res.var_observed[side_off + i] = ea, oa
    scores = np.full(batch.n_variants, 1000.0, np.float32)  # (truth entries carry a score that must not be read)
    scores[int(batch.q_off[0]):int(batch.q_off[0]) + len(query)] = scores_q
    return batch, res, scores


T = (10.0, 20.0, 30.0)
TP, FN, FNGT, HTP, HFN, WTP, WFN = size_lib.TRUTH_F
QTP, QFP = size_lib.QUERY_F[0], size_lib.QUERY_F[1]


def curve(batch, res, scores):
    got = score_tallies_host(batch, res, ScoreSpec(T), scores)
    calls = size_lib.calls_of(batch, res)
    want = score_lib.expected(calls, score_lib.call_index(batch, res), size_lib.alt_eds(batch), T, scores, batch.n_regions)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    return got[0, :, 0, :].astype(np.int64)  # [point][field] of the joint group


def test_a_truth_call_takes_the_minimum_over_its_supporting_query_calls():
    """two matching query calls at scores 25 and 12, one unmatched at 3 (hap_tp 0: no support): the truth calls hold until the filter passes 12"""
    batch, res, scores = hand_case(truth=[(2, 2, b"A", b"C"), (1, 1, b"A", b"ACGT")], query=[(2, 2, b"A", b"C"), (1, 1, b"A", b"ACGT"), (0, 1, b"G", b"T")], scores_q=[25.0, 12.0, 3.0])
    c = curve(batch, res, scores)
    assert list(c[:, TP]) == [2, 2, 0, 0] and list(c[:, FN]) == [0, 0, 2, 2]      # support's minimum is 12: bin 1 -> kept at the points 0, 1
    assert list(c[:, HTP]) == [3, 3, 0, 0] and list(c[:, HFN]) == [0, 0, 3, 3]    # lost: hap_fn = expected
    assert list(c[:, WTP]) == [2 * 1 + 1 * 3, 5, 0, 0] and list(c[:, WFN]) == [0, 0, 5, 5]  # lost: w_fn = expected * alt_ed (1 and 3)
    assert list(c[:, FNGT]) == [0, 0, 0, 0]                                        # a lost call adds no FN_GT
    assert list(c[:, QTP]) == [2, 2, 1, 0] and list(c[:, QFP]) == [1, 0, 0, 0]     # a filtered query call is neither TP nor FP


def test_a_truth_call_nothing_observes_is_changed_by_no_filter():
    """observed 0: bin K whatever the region's query calls score; beside it a supported call that is lost"""
    batch, res, scores = hand_case(truth=[(1, 0, b"A", b"C"), (1, 1, b"G", b"T")], query=[(1, 1, b"G", b"T")], scores_q=[NAN])
    c = curve(batch, res, scores)
    assert list(c[:, TP]) == [1, 0, 0, 0] and list(c[:, FN]) == [1, 2, 2, 2] and list(c[:, HFN]) == [1, 2, 2, 2]
    assert list(c[:, QTP]) == [1, 0, 0, 0]  # a missing score is kept at point 0 only


def test_a_region_without_a_supporting_query_call():
    """observed > 0 on the truth side but no query call with hap_tp > 0: bin K"""
    batch, res, scores = hand_case(truth=[(2, 1, b"A", b"C")], query=[(0, 1, b"A", b"G")], scores_q=[-INF])
    c = curve(batch, res, scores)
    assert list(c[:, FN]) == [1, 1, 1, 1] and list(c[:, FNGT]) == [1, 1, 1, 1] and list(c[:, HTP]) == [1, 1, 1, 1] and list(c[:, HFN]) == [1, 1, 1, 1]
    assert list(c[:, QFP]) == [1, 0, 0, 0]


def test_scores_on_and_around_a_threshold():
    below, above = np.nextafter(np.float32(20), np.float32(-INF), dtype=np.float32), np.nextafter(np.float32(20), np.float32(INF), dtype=np.float32)
    for s, kept in ((np.float32(20), 3), (below, 2), (above, 3), (np.float32(INF), 4), (np.float32(-0.0), 1)):
        batch, res, scores = hand_case(truth=[(1, 1, b"A", b"C")], query=[(1, 1, b"A", b"C")], scores_q=[s])
        c = curve(batch, res, scores)
        assert list(c[:, QTP]) == [1] * kept + [0] * (4 - kept) and list(c[:, TP]) == [1] * kept + [0] * (4 - kept), float(s)


# ---- the oracle's results on the scenarios ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def job():
    """three oracle-solved batches (indels, unsolved regions, kilobase alleles and SV types), their calls restated, seeded scores: shared, never changed"""
    parts = []
    for k, (contigs, batch) in enumerate((scenarios.indel_small(600), scenarios.invalid_regions(), scenarios.long_allele_regions())):
        res = oracle_lib.compare_batch(oracle_lib.load(), batch, contigs, threads=8)
        parts.append(dict(batch=batch, res=res, calls=size_lib.calls_of(batch, res), vidx=score_lib.call_index(batch, res), alt_ed=size_lib.alt_eds(batch)))
    assert any((np.asarray(p["res"].status) != 0).any() for p in parts)
    return parts


def scores_of(job, thresholds):
    return [score_lib.scores_for(p["batch"].n_variants, thresholds, 11 + k) for k, p in enumerate(job)]


def host_sum(job, thresholds, scores, threads=1, labels=None):
    out = None
    for k, p in enumerate(job):
        out = score_tallies_host(p["batch"], p["res"], ScoreSpec(thresholds), scores[k], labels=None if labels is None else labels[k], threads=threads, out=out)
    return out


def want_sum(job, thresholds, scores, members=None):
    return sum(score_lib.expected(p["calls"], p["vidx"], p["alt_ed"], thresholds, scores[k], p["batch"].n_regions, None if members is None else members[k]) for k, p in enumerate(job))


@pytest.mark.parametrize("thresholds", score_lib.SPECS)
@pytest.mark.parametrize("threads", [0, 5])
def test_host_route_equals_the_restatement(job, thresholds, threads):
    scores = scores_of(job, thresholds)
    got, want = host_sum(job, thresholds, scores, threads), want_sum(job, thresholds, scores)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert got[0, -1, 0].any() and not np.array_equal(got[0, 0], got[0, -1])


@pytest.mark.parametrize("thresholds", score_lib.SPECS)
def test_invariants_against_the_oracle(job, thresholds):
    """point 0 is the oracle's tally (its group_metrics summed over the solved regions) and the size block summed over its bins; the sums and monotonicity"""
    got = host_sum(job, thresholds, scores_of(job, thresholds))
    tally = np.zeros((_abi.N_GROUPS, _abi.N_FIELDS), np.uint64)
    size = None
    for p in job:
        solved = np.asarray(p["res"].status) == 0
        tally += np.asarray(p["res"].group_metrics).reshape(p["batch"].n_regions, _abi.N_GROUPS, _abi.N_FIELDS)[solved].astype(np.uint64).sum(axis=0)
        size = aardvark_amd.size_tallies_host(p["batch"], p["res"], aardvark_amd.SizeSpec(), out=size)
    assert tally[:, :14].any() and np.array_equal(size[0].sum(axis=0), tally[:, :14])
    score_lib.check_invariants(got, tally[:, :14][None])
    assert (got[0, :-1, 0, TP] > got[0, 1:, 0, TP]).any() and (got[0, :-1, 0, FN] < got[0, 1:, 0, FN]).any(), "the curve moves"


def test_host_route_with_labels_and_it_adds(job):
    rng = np.random.default_rng(2)
    members, labels = [], []
    for p in job:
        n = p["batch"].n_regions
        m = [np.ones(n, bool), np.zeros(n, bool), rng.random(n) < 0.3]
        lists = [[l for l in range(3) if m[l][r]] for r in range(n)]
        off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint64)
        members.append(m), labels.append((3, off, np.array([l for x in lists for l in x] + [0], np.uint32)))
    scores = scores_of(job, score_lib.DEFAULT)
    got = host_sum(job, score_lib.DEFAULT, scores, 3, labels)
    assert np.array_equal(got, want_sum(job, score_lib.DEFAULT, scores, members))
    assert np.array_equal(got[1], got[0]) and not got[2].any() and got[3].any()
    score_lib.check_invariants(got)
    p = job[0]
    once = score_tallies_host(p["batch"], p["res"], ScoreSpec(), scores[0])
    assert np.array_equal(score_tallies_host(p["batch"], p["res"], ScoreSpec(), scores[0], out=once.copy()), 2 * once)


def test_refusals_leave_out_untouched(job):
    lib, p = aardvark_amd.load_library(), job[1]
    out = np.zeros((1, 32, _abi.N_GROUPS, 14), np.uint64)
    cb, ro = p["batch"].c_struct(), p["res"].c_struct()
    sc = np.zeros(p["batch"].n_variants + 1, np.float32)
    for t in INVALID:
        spec = score_lib.c_spec(t[:31], n=len(t))
        assert lib.avk_score_tallies_host(C.byref(cb), C.byref(ro), C.byref(spec), sc.ctypes.data_as(f32p), None, 1, out.ctypes.data_as(u64p)) == -1, t
        assert "strictly ascending" in lib.avk_last_error(None).decode()
        assert lib.avk_score_tallies(None, None, C.byref(spec), sc.ctypes.data_as(f32p), None, out.ctypes.data_as(u64p)) == -1
    good = score_lib.c_spec(score_lib.DEFAULT)
    assert lib.avk_score_tallies_host(C.byref(cb), C.byref(ro), None, sc.ctypes.data_as(f32p), None, 1, out.ctypes.data_as(u64p)) == -1 and "spec missing" in lib.avk_last_error(None).decode()
    assert lib.avk_score_tallies_host(C.byref(cb), C.byref(ro), C.byref(good), None, None, 1, out.ctypes.data_as(u64p)) == -1 and "scores missing" in lib.avk_last_error(None).decode()
    assert lib.avk_score_tallies_host(C.byref(cb), C.byref(ro), C.byref(good), sc.ctypes.data_as(f32p), None, 1, None) == -1 and "score_tallies missing" in lib.avk_last_error(None).decode()
    assert not out.any()
    with pytest.raises(ValueError, match="scores holds"):
        score_tallies_host(p["batch"], p["res"], ScoreSpec(), sc)
