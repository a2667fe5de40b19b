"""Packed batches with escapes (avk_packed_escapes), the host side: the Python packing and its inverse, slices, and the library's shard and merge-count functions
with escapes.  No GPU involved."""
import ctypes as C

import numpy as np
import pytest

import aardvark_amd
import escapes_lib as el
from aardvark_amd import CompactBatch, PackedBatch, ResultBatch, dist, synth
from aardvark_amd._abi import AvkPackedBatch, AvkPackedEscapes, AvkResultBatch, PackedEscapes
from aardvark_amd.merge import MergeResult, MultiBatch, PackedMultiBatch, merge_counts, merge_counts_len, shard_packed_multi

JOBS = {"genome": el.genome_job, "indel_mix_v2": el.indel_mix_job}


@pytest.fixture(scope="module", params=sorted(JOBS))
def job(request):
    contigs, batch = JOBS[request.param]()
    cb, pb = el.escaped(batch)
    return contigs, batch, cb, pb


def same_compact(a, b):
    bad = []
    for f in CompactBatch.FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        if (x is None) != (y is None) or (x is not None and not (x.dtype == y.dtype and np.array_equal(x, y))):
            bad.append(f)
    return bad


def test_round_trip_and_the_borders_of_the_narrow_fields(job):
    contigs, batch, cb, pb = job
    with pytest.raises(ValueError):
        PackedBatch.from_compact(cb)  # the default keeps raising
    assert same_compact(pb.to_compact(), cb) == []
    e = pb.escapes
    # 65,535 / 255 fit the narrow fields, 65,536 / 256 are listed; a listed entry's narrow fields are 0
    assert sorted(e.esc_len.tolist()) == [65_536, 70_000] and sorted(e.esc_cnt.tolist()) == [256, 300]
    assert int(pb.len.max()) == 65_535 and int(pb.t_cnt.max()) == 255 and int(pb.a0_len.max()) == 255 and int(pb.a1_len.max()) == 255 and int(pb.var_rel_pos.max()) == 65_535
    assert int(e.esc_a0_len.max()) == 1500 and int(e.esc_a1_len.max()) == 2000 and 256 in e.esc_a0_len.tolist() and 256 in e.esc_a1_len.tolist() and 65_536 in e.esc_rel_pos.tolist()
    assert not pb.len[e.esc_region.astype(np.int64)].any() and not pb.var_rel_pos[e.esc_call.astype(np.int64)].any()
    assert not pb.a0_len[e.esc_call.astype(np.int64)].any() and not pb.a1_len[e.esc_call.astype(np.int64)].any()
    slots = np.stack([pb.t_cnt, pb.q_cnt], axis=1).reshape(-1)
    assert not slots[e.esc_slot.astype(np.int64)].any()
    for lst in (e.esc_region, e.esc_slot, e.esc_call):
        assert np.all(np.diff(lst.astype(np.int64)) > 0)
    assert pb.nbytes() < cb.nbytes() and pb.nbytes() == PackedBatch(**{f: getattr(pb, f) for f in PackedBatch.FIELDS}).nbytes() + e.nbytes()


def test_a_batch_with_nothing_to_escape_is_the_packed_batch_it_was():
    contig, batch = synth.config_indel_mix_v2(n_truth=3000, contig_len=1_200_000)
    cb = CompactBatch.from_region_batch(batch)
    plain, esc = PackedBatch.from_compact(cb), PackedBatch.from_compact(cb, escapes=True)
    assert esc.escapes.empty() and esc.c_escapes() is None and plain.escapes is None
    for f in PackedBatch.FIELDS:
        x, y = getattr(plain, f), getattr(esc, f)
        assert (x is None and y is None) or (x.dtype == y.dtype and x.tobytes() == y.tobytes()), f
    assert same_compact(esc.to_compact(), cb) == [] and same_compact(plain.to_compact(), cb) == []


@pytest.mark.parametrize("n_parts", [2, 3, 7])
def test_split_parts_joined_back_give_the_whole(job, n_parts):
    contigs, batch, cb, pb = job
    parts = pb.split(n_parts)
    assert sum(p.n_regions for p in parts) == pb.n_regions and sum(p.n_variants for p in parts) == pb.n_variants
    assert sum(p.escapes.esc_call.size for p in parts) == pb.escapes.esc_call.size and sum(p.escapes.esc_slot.size for p in parts) == pb.escapes.esc_slot.size
    r0 = 0
    for p in parts:  # every part stands for its regions of the wide batch; the lists are ranges of the whole batch's (no copy), with bases
        assert p.escapes.first_region == r0 and p.escapes.first_slot == 2 * r0
        assert p.escapes.esc_call.size == 0 or p.escapes.esc_call.base is not None
        got = el.region_contents(p.to_compact().widen(), np.arange(p.n_regions))
        assert el.same_contents(got, el.region_contents(batch, np.arange(r0, r0 + p.n_regions))) == []
        r0 += p.n_regions
    for f in ("start", "len", "t_cnt", "q_cnt", "var_rel_pos", "a0_len", "a1_len", "var_type_zyg", "allele_bytes"):
        assert np.array_equal(np.concatenate([getattr(p, f) for p in parts]), getattr(pb, f)), f


def shard_api():
    lib = aardvark_amd.load_library()
    P = C.POINTER
    lib.avk_packed_shard_make_esc.argtypes = [P(AvkPackedBatch), P(AvkPackedEscapes), P(C.c_uint64), C.c_uint64, C.c_uint32, C.c_uint32, P(C.c_void_p)]
    lib.avk_packed_shard_batch.restype = P(AvkPackedBatch)
    lib.avk_packed_shard_batch.argtypes = [C.c_void_p]
    lib.avk_packed_shard_escapes.restype = P(AvkPackedEscapes)
    lib.avk_packed_shard_escapes.argtypes = [C.c_void_p]
    lib.avk_packed_shard_regions.restype = C.c_uint64
    lib.avk_packed_shard_regions.argtypes = [C.c_void_p, P(P(C.c_uint64))]
    lib.avk_packed_shard_scatter.argtypes = [C.c_void_p, P(AvkResultBatch), P(AvkResultBatch)]
    lib.avk_packed_shard_free.argtypes = [C.c_void_p]
    return lib


def shard_as_python(lib, handle):
    b = lib.avk_packed_shard_batch(handle).contents
    n, nv, na = int(b.n_regions), int(b.n_variants), int(b.allele_bytes_len)
    take = lambda p, k, dt: np.ctypeslib.as_array(p, shape=(max(k, 1),))[:k].astype(dt).copy() if p else None
    pb = PackedBatch(escapes=PackedEscapes.from_c(lib.avk_packed_shard_escapes(handle).contents), contig_idx=take(b.contig_idx, n, np.uint16), start=take(b.start, n, np.uint32),
                     len=take(b.len, n, np.uint16), t_cnt=take(b.t_cnt, n, np.uint8), q_cnt=take(b.q_cnt, n, np.uint8), var_rel_pos=take(b.var_rel_pos, nv, np.uint16),
                     var_type_zyg=take(b.var_type_zyg, nv, np.uint8), a0_len=take(b.a0_len, nv, np.uint8), a1_len=take(b.a1_len, nv, np.uint8),
                     var_raw_space=take(b.var_raw_space, nv, np.uint32), allele_bytes=take(b.allele_bytes, na, np.uint8))
    idx = C.POINTER(C.c_uint64)()
    m = int(lib.avk_packed_shard_regions(handle, C.byref(idx)))
    return pb, np.ctypeslib.as_array(idx, shape=(max(m, 1),))[:m].copy()


@pytest.mark.parametrize("world", [2, 3])
def test_shards_with_escapes_hold_the_wide_regions_of_the_hash_rule_and_scatter_back(job, world):
    lib = shard_api()
    contigs, batch, cb, pb = job
    st, esc = pb.c_struct(), pb.c_escapes()
    ids = np.ascontiguousarray(batch.region_id + np.uint64(77), np.uint64)
    whole = ResultBatch(pb, sequences=False, group_metrics=False, packed=True)
    rng = np.random.default_rng(3)
    want_region, want_call = rng.integers(0, 2 ** 40, pb.n_regions).astype(np.uint64), rng.integers(0, 127, pb.n_variants).astype(np.uint8)
    voff = np.concatenate([batch.t_off.astype(np.int64), [batch.n_variants]])
    listed = 0
    for rank in range(world):
        h = C.c_void_p()
        assert lib.avk_packed_shard_make_esc(C.byref(st), C.byref(esc), ids.ctypes.data_as(C.POINTER(C.c_uint64)), 0, rank, world, C.byref(h)) == 0
        shard, idx = shard_as_python(lib, h)
        assert np.array_equal(idx, np.flatnonzero(dist.region_hash(ids) % np.uint64(world) == rank))
        assert shard.escapes.first_region == 0 and shard.escapes.first_call == 0 and shard.escapes.first_slot == 0  # rebased to the shard's indices
        listed += shard.escapes.esc_call.size + shard.escapes.esc_slot.size + shard.escapes.esc_region.size
        got = el.region_contents(shard.to_compact().widen(), np.arange(shard.n_regions))
        assert el.same_contents(got, el.region_contents(batch, idx)) == []
        # the shard's results, made up here, land at the regions' and the calls' places in the whole batch's arrays
        res = ResultBatch(shard, sequences=False, group_metrics=False, packed=True)
        calls = np.concatenate([np.arange(voff[r], voff[r + 1]) for r in idx]) if idx.size else np.zeros(0, np.int64)
        res.region_packed[:shard.n_regions], res.var_packed[:shard.n_variants] = want_region[idx], want_call[calls]
        res.status[:] = (want_region[idx] & np.uint64(0x7F)).astype(np.int32)
        res.var_zyg[:shard.n_variants] = want_call[calls] >> 4
        a, b = res.c_struct(), whole.c_struct()
        assert lib.avk_packed_shard_scatter(h, C.byref(a), C.byref(b)) == 0
        lib.avk_packed_shard_free(h)
    e = pb.escapes
    assert listed == e.esc_call.size + e.esc_slot.size + e.esc_region.size
    assert np.array_equal(whole.region_packed[:pb.n_regions], want_region) and np.array_equal(whole.var_packed[:pb.n_variants], want_call)
    assert np.array_equal(whole.status, (want_region & np.uint64(0x7F)).astype(np.int32)) and np.array_equal(whole.var_zyg[:pb.n_variants], want_call >> 4)


def test_escape_lists_that_are_not_ascending_or_leave_the_batch_are_refused(job):
    lib = shard_api()
    contigs, batch, cb, pb = job
    st = pb.c_struct()
    for spoil in ("order", "range"):
        e = PackedEscapes(**{f: getattr(pb.escapes, f).copy() for f in PackedEscapes.FIELDS})
        if spoil == "order":
            e.esc_call[:2] = e.esc_call[:2][::-1].copy()
        else:
            e.esc_call[-1] = pb.n_variants
        esc, h = e.c_struct(), C.c_void_p()
        assert lib.avk_packed_shard_make_esc(C.byref(st), C.byref(esc), None, 0, 0, 2, C.byref(h)) == -1  # AVK_E_ARG


@pytest.fixture(scope="module")
def long_part():
    """(the genome job's packed batch, its second half — non-zero bases — with 2,048 entries in each list)"""
    pb = el.escaped(el.genome_job()[1])[1]
    part = pb.split(2)[1]
    assert part.escapes.first_region > 0 and part.escapes.first_call > 0
    return pb, el.promote(part, *el.exact_promotion(part, (2048, 2048, 2048)))


def _shard_rc(lib, pb):
    st, esc, h = pb.c_struct(), pb.escapes.c_struct(), C.c_void_p()
    rc = lib.avk_packed_shard_make_esc(C.byref(st), C.byref(esc), None, 0, 0, 2, C.byref(h))
    if rc == 0:
        lib.avk_packed_shard_free(h)
    return rc


@pytest.mark.parametrize("which", sorted(el.LISTS))
def test_every_list_is_checked_on_the_host_duplicates_chunk_edges_and_both_ends_of_the_range(long_part, which):
    lib = shard_api()
    good = long_part[1]
    assert _shard_rc(lib, good) == 0
    for how in el.SPOILS:
        assert _shard_rc(lib, el.spoiled(good, which, how)) == -1, how  # AVK_E_ARG
    # n_esc_* > 0 with a NULL index or value array
    for name in {"region": ("esc_region", "esc_len"), "slot": ("esc_slot", "esc_cnt"), "call": ("esc_call", "esc_rel_pos", "esc_a0_len", "esc_a1_len")}[which]:
        st, esc, h = good.c_struct(), good.escapes.c_struct(), C.c_void_p()
        setattr(esc, name, None)
        assert lib.avk_packed_shard_make_esc(C.byref(st), C.byref(esc), None, 0, 0, 2, C.byref(h)) == -1, name


def test_a_listed_entry_whose_narrow_field_is_not_zero_is_refused_by_the_shards(long_part):
    """the rule of avk_packed_escapes, for all five narrow fields (six arrays): the host route refuses what the device route refuses (tests/test_gpu_packed_escapes.py
    hands the same batches to avk_compare_packed_esc)"""
    lib = shard_api()
    plain, good = long_part
    assert _shard_rc(lib, good) == 0
    for field in el.narrow_fields(good):
        assert _shard_rc(lib, el.nonzero_under_a_listed_entry(good, field)) == -1, field
    # ... and of the batch as the packer made it (short lists; it lists no query-side count)
    assert not (plain.escapes.esc_slot % np.uint64(2)).any() and _shard_rc(lib, plain) == 0
    for field in [f for f in el.narrow_fields(plain) if f != "q_cnt"]:
        assert _shard_rc(lib, el.nonzero_under_a_listed_entry(plain, field)) == -1, field


# ---- the multi form ---------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def multi_job():
    contigs, mb = el.merge_job()
    return contigs, mb, PackedMultiBatch.from_multi(mb, escapes=True)


def same_multi(a, b):
    return [f for f in MultiBatch.FIELDS if f != "region_id" and not np.array_equal(getattr(a, f)[:getattr(b, f).size] if f == "allele_bytes" else getattr(a, f), getattr(b, f))]


def test_multi_round_trip(multi_job):
    contigs, mb, pm = multi_job
    with pytest.raises(ValueError):
        PackedMultiBatch.from_multi(mb)
    assert same_multi(mb, pm.widen()) == []
    e = pm.escapes
    assert e.esc_len.tolist() == [66_000] and e.esc_cnt.tolist() == [260, 260] and int(pm.in_cnt.max()) == 255 and int(pm.a1_len.max()) == 255
    assert {256, 300, 1200} <= set(e.esc_a1_len.tolist()) and {256, 300, 1200} <= set(e.esc_a0_len.tolist()) and 65_536 in e.esc_rel_pos.tolist()
    # nothing to escape: the batch it was
    contigs2, plain_mb = synth.config_genome_merge(scale=0.0008, k=3, threads=4)
    a, b = PackedMultiBatch.from_multi(plain_mb), PackedMultiBatch.from_multi(plain_mb, escapes=True)
    assert b.escapes.empty() and b.c_escapes() is None
    for f in PackedMultiBatch.FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert (x is None and y is None) or (x.dtype == y.dtype and x.tobytes() == y.tobytes()), f


def multi_contents(mb, idx):
    k = mb.n_inputs
    calls = np.concatenate([np.arange(int(mb.in_off[m * k]), int(mb.in_off[m * k]) + int(mb.in_cnt[m * k:(m + 1) * k].sum())) for m in idx]).astype(np.int64)
    ab = mb.allele_bytes
    alleles = b"".join(ab[int(mb.a0_off[v]):int(mb.a0_off[v]) + int(mb.a0_len[v])].tobytes() + ab[int(mb.a1_off[v]):int(mb.a1_off[v]) + int(mb.a1_len[v])].tobytes() for v in calls)
    return {"start": mb.start[idx], "end": mb.end[idx], "contig_idx": mb.contig_idx[idx], "in_cnt": mb.in_cnt.reshape(-1, k)[idx], "var_pos": mb.var_pos[calls],
            "var_type": mb.var_type[calls], "var_zyg": mb.var_zyg[calls], "a0_len": mb.a0_len[calls], "a1_len": mb.a1_len[calls], "var_raw_space": mb.var_raw_space[calls],
            "alleles": np.frombuffer(alleles, np.uint8)}


def random_results(n, k, seed, unsolved=0.02):
    rng = np.random.default_rng(seed)
    cls = rng.integers(0, 5, n).astype(np.uint8)
    masks = rng.integers(1, 1 << k, n).astype(np.uint64)
    index = rng.integers(0, k, n).astype(np.uint64)
    members = np.where((cls == 2) | (cls == 3), masks, np.where(cls == 4, index, 0)).astype(np.uint64)
    status = np.where(rng.random(n) < unsolved, 3, 0).astype(np.int32)
    status[-3:] = 0  # (the injected regions with escaped counts are counted)
    return MergeResult(status, cls, members, k)


@pytest.mark.parametrize("world", [2, 3])
def test_multi_shards_with_escapes_scatter_and_counts(multi_job, world):
    contigs, mb, pm = multi_job
    lib = aardvark_amd.load_library()
    ids = mb.region_id + np.uint64(5)
    res = random_results(pm.n_regions, 3, 9)
    whole_counts = merge_counts(lib, pm, res)
    # the escape-aware counts are those of the wide batch: every call of a solved region once, under its region's reason
    solved = np.repeat(res.status == 0, mb.in_cnt.reshape(-1, 3).sum(axis=1).astype(np.int64))
    assert int(whole_counts.sum()) == int(solved.sum())
    summed = np.zeros(merge_counts_len(lib, 3), np.uint64)
    back = MergeResult(np.full(pm.n_regions, -1, np.int32), np.zeros(pm.n_regions, np.uint8), np.zeros(pm.n_regions, np.uint64), 3)
    from aardvark_amd.merge import _shard_api
    seen = 0
    for rank in range(world):
        shard, idx = shard_packed_multi(lib, pm, ids, rank, world)
        assert np.array_equal(idx, np.flatnonzero(dist.region_hash(ids) % np.uint64(world) == rank))
        assert el.same_contents(multi_contents(shard.widen(), np.arange(shard.n_regions)), multi_contents(mb, idx)) == []
        seen += shard.escapes.esc_slot.size
        part = MergeResult(res.status[idx], res.classification[idx], res.members[idx], 3)
        merge_counts(lib, shard, part, summed)
        back.status[idx], back.classification[idx], back.members[idx] = part.status, part.classification, part.members
    assert seen == pm.escapes.esc_slot.size
    assert np.array_equal(summed, whole_counts)
    assert np.array_equal(back.status, res.status) and np.array_equal(back.classification, res.classification) and np.array_equal(back.members, res.members)
    # the counts without the escapes miss the calls of the escaped inputs (the narrow counts say 0 there): the old entry point is not enough for such a batch
    P = lambda a, t: np.ascontiguousarray(a).ctypes.data_as(C.POINTER(t))
    cb, plain = pm.c_struct(), np.zeros(summed.size, np.uint64)
    assert _shard_api(lib).avk_merge_counts(C.byref(cb), P(res.status, C.c_int32), P(res.classification, C.c_uint8), P(res.members, C.c_uint64), P(plain, C.c_uint64)) == -1


def test_the_multi_form_refuses_bad_lists_and_non_zero_narrow_fields_on_the_host(multi_job):
    from aardvark_amd.merge import _shard_api
    contigs, mb, pm = multi_job
    lib = _shard_api(aardvark_amd.load_library())
    ids = mb.region_id + np.uint64(5)
    res = random_results(pm.n_regions, 3, 9)
    # 2,048 entries in each list, and the bases of a slice of a larger batch: avk_packed_escapes carries them for both forms
    good = el.rebased(el.promote(pm, *el.exact_promotion(pm, (2048, 2048, 2048))))
    assert good.escapes.first_region > 0 and good.escapes.first_slot > 0 and good.escapes.first_call > 0
    assert np.array_equal(merge_counts(lib, good, res), merge_counts(lib, pm, res))  # the promoted, rebased batch is the same batch
    shard, idx = shard_packed_multi(lib, good, ids, 0, 2)
    assert el.same_contents(multi_contents(shard.widen(), np.arange(shard.n_regions)), multi_contents(mb, idx)) == []
    bad = [(which, el.spoiled(good, which, how)) for which in sorted(el.LISTS) for how in el.SPOILS]
    bad += [(field, el.nonzero_under_a_listed_entry(b, field)) for b in (good, pm) for field in el.narrow_fields(good)]
    assert len(bad) == 15 + 10
    for what, b in bad:
        with pytest.raises(ValueError):
            shard_packed_multi(lib, b, ids, 0, 2)
        if what in ("slot", "in_cnt"):  # avk_merge_counts_esc reads the count slots only: it checks what it reads
            with pytest.raises(ValueError):
                merge_counts(lib, b, res)
    # n_esc_* > 0 with a NULL index or value array
    P = lambda a, t: np.ascontiguousarray(a).ctypes.data_as(C.POINTER(t))
    for name in PackedEscapes.FIELDS:
        st, esc, h = good.c_struct(), good.escapes.c_struct(), C.c_void_p()
        setattr(esc, name, None)
        assert lib.avk_packed_multi_shard_make_esc(C.byref(st), C.byref(esc), P(ids, C.c_uint64), 0, 0, 2, C.byref(h)) == -1 and not h.value, name
        if name in ("esc_slot", "esc_cnt"):
            counts = np.zeros(merge_counts_len(lib, 3), np.uint64)
            assert lib.avk_merge_counts_esc(C.byref(st), C.byref(esc), P(res.status, C.c_int32), P(res.classification, C.c_uint8), P(res.members, C.c_uint64), P(counts, C.c_uint64)) == -1
            assert not counts.any()


# ---- the feeder -------------------------------------------------------------------------------------------------------------------------------

def _numpy_alloc():
    from aardvark_amd.feeder import _ALLOC
    bufs = {}

    def alloc(_user, nbytes):
        a = np.empty(max(int(nbytes), 1), np.uint8)
        bufs[a.ctypes.data] = a
        return a.ctypes.data

    def view(ptr, count, dtype):
        addr = C.cast(ptr, C.c_void_p).value
        return None if addr is None else np.frombuffer((C.c_uint8 * (count * np.dtype(dtype).itemsize)).from_address(addr), dtype).copy()

    return _ALLOC(alloc), view, bufs


def _packed_of(st, esc, view):
    n, nv, na = int(st.n_regions), int(st.n_variants), int(st.allele_bytes_len)
    from aardvark_amd.feeder import _escapes_of
    return PackedBatch(escapes=_escapes_of(esc, view), contig_idx=view(st.contig_idx, n, np.uint16), start=view(st.start, n, np.uint32), len=view(st.len, n, np.uint16),
                       t_cnt=view(st.t_cnt, n, np.uint8), q_cnt=view(st.q_cnt, n, np.uint8), var_rel_pos=view(st.var_rel_pos, nv, np.uint16), var_type_zyg=view(st.var_type_zyg, nv, np.uint8),
                       a0_len=view(st.a0_len, nv, np.uint8), a1_len=view(st.a1_len, nv, np.uint8), var_raw_space=view(st.var_raw_space, nv, np.uint32),
                       allele_bytes=view(st.allele_bytes, na, np.uint8))


def test_feeder_packs_with_escapes_what_the_plain_pack_refuses(tmp_path):
    import os
    from aardvark_amd import feeder
    p = el.write_feeder_case(tmp_path)
    lib = feeder.load_library()
    g = feeder.Genome(p["fa"])
    h = C.c_void_p()
    assert lib.avf_feed_compare(os.fsencode(p["t"]), b"", os.fsencode(p["q"]), b"", os.fsencode(p["bed"]), g.handle, el.GAP, 1, C.byref(h)) == 0
    try:
        wide = feeder.feed_compare(p["t"], p["q"], p["bed"], g, min_variant_gap=el.GAP)
        batch = wide.batch  # avf_feed_batch, field for field
        assert wide.packed is None and wide.packed_esc is not None
        assert int(batch.t_cnt.max()) == 300 and int(batch.a1_len.max()) >= 300 and int(batch.a0_len.max()) >= 2000
        cb, view, keep = _numpy_alloc()
        st, esc = AvkPackedBatch(), AvkPackedEscapes()
        lib.avf_feed_pack.argtypes = [C.c_void_p, type(cb), C.c_void_p, C.POINTER(AvkPackedBatch)]
        lib.avf_feed_pack_esc.argtypes = [C.c_void_p, type(cb), C.c_void_p, C.POINTER(AvkPackedBatch), C.POINTER(AvkPackedEscapes)]
        assert lib.avf_feed_pack(h, cb, None, C.byref(st)) == 1
        assert lib.avf_feed_pack_esc(h, cb, None, C.byref(st), C.byref(esc)) == 0
        assert int(esc.n_esc_slots) == 1 and int(esc.n_esc_calls) >= 4  # the 300-call side; the insertion and the deletion on both sides
        pb = _packed_of(st, esc, view)
        assert el.same_contents(el.region_contents(pb.to_compact().widen(), np.arange(pb.n_regions)), el.region_contents(batch, np.arange(batch.n_regions))) == []
        assert same_compact(pb.to_compact(), CompactBatch.from_region_batch(batch)) == []
        assert same_compact(wide.packed_esc.to_compact(), pb.to_compact()) == []
        # the Python packer lists the same entries
        mine = PackedBatch.from_compact(CompactBatch.from_region_batch(batch), escapes=True)
        for f in PackedEscapes.FIELDS:
            assert np.array_equal(getattr(mine.escapes, f), getattr(pb.escapes, f)), f
        # slices at several cut points: pointer ranges plus bases
        lib.avf_packed_slice_esc.argtypes = [C.c_void_p, C.POINTER(AvkPackedBatch), C.POINTER(AvkPackedEscapes), C.c_uint64, C.c_uint64, C.POINTER(AvkPackedBatch),
                                             C.POINTER(AvkPackedEscapes), C.POINTER(C.c_uint64)]
        n = pb.n_regions
        dense = int(np.argmax(batch.t_cnt))
        for first, count in ((0, n), (0, dense), (dense, 1), (dense + 1, n - dense - 1), (1, n - 2), (n, 0), (2, 3)):
            part, pe, v0 = AvkPackedBatch(), AvkPackedEscapes(), C.c_uint64()
            assert lib.avf_packed_slice_esc(h, C.byref(st), C.byref(esc), first, count, C.byref(part), C.byref(pe), C.byref(v0)) == 0
            assert int(pe.first_region) == first and int(pe.first_slot) == 2 * first and int(pe.first_call) == int(v0.value) == (int(batch.t_off[first]) if first < n else batch.n_variants)
            sl = _packed_of(part, pe, view)
            assert el.same_contents(el.region_contents(sl.to_compact().widen(), np.arange(count)), el.region_contents(batch, np.arange(first, first + count))) == [], (first, count)
    finally:
        lib.avf_feed_free(h)
        g.close()


def test_feeder_packs_a_merge_feed_with_escapes(tmp_path):
    import os
    from aardvark_amd import feeder
    from aardvark_amd.merge import AvkPackedMultiBatch
    p = el.write_feeder_case(tmp_path)
    lib = feeder.load_library()
    g = feeder.Genome(p["fa"])
    try:
        feed = feeder.feed_merge(p["vcfs"], p["bed"], g, min_variant_gap=el.GAP)
        mb = feed.batch
        assert feed.packed is None and feed.packed_esc is not None and int(mb.in_cnt.max()) == 300
        assert same_multi(mb, feed.packed_esc.widen()) == []
        mine = PackedMultiBatch.from_multi(mb, escapes=True)
        for f in PackedEscapes.FIELDS:
            assert np.array_equal(getattr(mine.escapes, f), getattr(feed.packed_esc.escapes, f)), f
        # slices through the C function
        h = C.c_void_p()
        vcfs = (C.c_char_p * 3)(*[os.fsencode(v) for v in p["vcfs"]])
        samples = (C.c_char_p * 3)(b"", b"", b"")
        assert lib.avf_feed_merge(3, vcfs, samples, os.fsencode(p["bed"]), g.handle, el.GAP, 1, C.byref(h)) == 0
        try:
            cb, view, keep = _numpy_alloc()
            st, esc = AvkPackedMultiBatch(), AvkPackedEscapes()
            lib.avf_feed_pack_multi.argtypes = [C.c_void_p, type(cb), C.c_void_p, C.POINTER(AvkPackedMultiBatch)]
            lib.avf_feed_pack_multi_esc.argtypes = [C.c_void_p, type(cb), C.c_void_p, C.POINTER(AvkPackedMultiBatch), C.POINTER(AvkPackedEscapes)]
            lib.avf_packed_multi_slice_esc.argtypes = [C.c_void_p, C.POINTER(AvkPackedMultiBatch), C.POINTER(AvkPackedEscapes), C.c_uint64, C.c_uint64,
                                                       C.POINTER(AvkPackedMultiBatch), C.POINTER(AvkPackedEscapes)]
            assert lib.avf_feed_pack_multi(h, cb, None, C.byref(st)) == 1
            assert lib.avf_feed_pack_multi_esc(h, cb, None, C.byref(st), C.byref(esc)) == 0
            n = mb.n_regions
            from aardvark_amd.feeder import _escapes_of
            for first, count in ((0, n), (1, n - 2), (n // 2, n - n // 2), (0, n // 2), (n, 0)):
                part, pe = AvkPackedMultiBatch(), AvkPackedEscapes()
                assert lib.avf_packed_multi_slice_esc(h, C.byref(st), C.byref(esc), first, count, C.byref(part), C.byref(pe)) == 0
                m, nv, na = int(part.n_regions), int(part.n_variants), int(part.allele_bytes_len)
                sl = PackedMultiBatch(3, escapes=_escapes_of(pe, view), contig_idx=view(part.contig_idx, m, np.uint16), start=view(part.start, m, np.uint32), len=view(part.len, m, np.uint16),
                                      in_cnt=view(part.in_cnt, m * 3, np.uint8), var_rel_pos=view(part.var_rel_pos, nv, np.uint16), var_type_zyg=view(part.var_type_zyg, nv, np.uint8),
                                      a0_len=view(part.a0_len, nv, np.uint8), a1_len=view(part.a1_len, nv, np.uint8), var_raw_space=view(part.var_raw_space, nv, np.uint32),
                                      allele_bytes=view(part.allele_bytes, max(na, 1), np.uint8))
                assert count == 0 or el.same_contents(multi_contents(sl.widen(), np.arange(count)), multi_contents(mb, np.arange(first, first + count))) == [], (first, count)
        finally:
            lib.avf_feed_free(h)
    finally:
        g.close()
