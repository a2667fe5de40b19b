"""ctypes plumbing for libaardvark_feeder.so (include/aardvark_feeder.h): FASTA / BED / VCF -> RegionBatch with the
reference's region ids and windows (src/parsing/region_generation.rs), and the summary.tsv writer
(src/writers/summary.rs).  Host code only; the solver stays in libaardvark_amd.so."""
import ctypes as C
import os

import numpy as np

from ._abi import AvkRegionBatch, RegionBatch

METRIC_GT, METRIC_HAP, METRIC_WEIGHTED_HAP, METRIC_BASEPAIR, METRIC_RECORD_BP = 1, 2, 4, 8, 16
_lib = None


class FeederError(RuntimeError):
    pass


def library_path():
    return os.environ.get("AVF_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libaardvark_feeder.so")


def load_library():
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise FeederError("%s is missing: build it with `python __graft_entry__.py` (make -C aardvark_amd/csrc/feeder)" % path)
    lib = C.CDLL(path)
    vp = C.c_void_p
    lib.avf_last_error.restype = C.c_char_p
    lib.avf_genome_load.argtypes = [C.c_char_p, C.POINTER(vp)]
    lib.avf_genome_n_contigs.restype = C.c_uint32
    lib.avf_genome_n_contigs.argtypes = [vp]
    lib.avf_genome_name.restype = C.c_char_p
    lib.avf_genome_name.argtypes = [vp, C.c_uint32]
    lib.avf_genome_seq.restype = C.POINTER(C.c_uint8)
    lib.avf_genome_seq.argtypes = [vp, C.c_uint32]
    lib.avf_genome_len.restype = C.c_uint64
    lib.avf_genome_len.argtypes = [vp, C.c_uint32]
    lib.avf_genome_free.argtypes = [vp]
    lib.avf_feed_compare.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, vp, C.c_uint64, C.c_int, C.POINTER(vp)]
    lib.avf_feed_batch.restype = C.POINTER(AvkRegionBatch)
    lib.avf_feed_batch.argtypes = [vp]
    lib.avf_feed_var_record.restype = C.POINTER(C.c_uint64)
    lib.avf_feed_var_record.argtypes = [vp]
    lib.avf_feed_var_alt_index.restype = C.POINTER(C.c_uint32)
    lib.avf_feed_var_alt_index.argtypes = [vp]
    lib.avf_feed_loaded_variants.restype = C.c_uint64
    lib.avf_feed_loaded_variants.argtypes = [vp, C.c_int]
    lib.avf_feed_free.argtypes = [vp]
    lib.avf_write_summary.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_uint64), C.c_uint32]
    u8p = C.POINTER(C.c_uint8)
    lib.avf_write_annotated_vcf.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, vp, C.POINTER(AvkRegionBatch), C.c_int,
                                            C.POINTER(C.c_int32), u8p, u8p, u8p]
    lib.avf_strat_load.argtypes = [C.c_char_p, C.POINTER(vp)]
    lib.avf_strat_n_labels.restype = C.c_uint32
    lib.avf_strat_n_labels.argtypes = [vp]
    lib.avf_strat_label.restype = C.c_char_p
    lib.avf_strat_label.argtypes = [vp, C.c_uint32]
    lib.avf_strat_n_intervals.restype = C.c_uint64
    lib.avf_strat_n_intervals.argtypes = [vp, C.c_uint32, C.c_char_p]
    u32p = C.POINTER(C.c_uint32)
    for f in (lib.avf_strat_containments, lib.avf_strat_overlaps):
        f.restype = C.c_uint32
        f.argtypes = [vp, C.c_char_p, C.c_int64, C.c_int64, u32p, C.c_uint32]
    lib.avf_strat_region_labels.restype = C.c_uint32
    lib.avf_strat_region_labels.argtypes = [vp, vp, C.POINTER(AvkRegionBatch), C.c_uint64, u32p, C.c_uint32]
    lib.avf_strat_free.argtypes = [vp]
    lib.avf_strat_export.argtypes = [vp, vp, C.POINTER(C.c_uint64), u32p, u32p]
    lib.avf_strat_batch_labels.argtypes = [vp, vp, C.POINTER(AvkRegionBatch), C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), u32p]
    lib.avf_write_summary_stratified.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_uint64), vp, C.POINTER(C.c_uint64), C.c_uint32]
    lib.avf_write_summary_named.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(C.c_char_p), C.POINTER(C.c_uint64), C.c_uint32]
    lib.avf_region_summary_open.argtypes = [C.c_char_p, C.c_uint32, C.POINTER(vp)]
    lib.avf_region_summary_rows.argtypes = [vp, vp, C.POINTER(AvkRegionBatch), C.c_uint64, C.c_uint64, C.POINTER(C.c_int32), C.POINTER(C.c_uint32)]
    lib.avf_region_sequences_open.argtypes = [C.c_char_p, C.POINTER(vp)]
    lib.avf_region_sequences_rows.argtypes = [vp, vp, C.POINTER(AvkRegionBatch), C.c_uint64, C.c_uint64, C.POINTER(C.c_int32), C.POINTER(C.c_uint8),
                                              C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    lib.avf_table_close.argtypes = [vp]
    from .merge import AvkMultiBatch
    cpp = C.POINTER(C.c_char_p)
    lib.avf_feed_merge.argtypes = [C.c_uint32, cpp, cpp, C.c_char_p, vp, C.c_uint64, C.c_int, C.POINTER(vp)]
    lib.avf_feed_multi_batch.restype = C.POINTER(AvkMultiBatch)
    lib.avf_feed_multi_batch.argtypes = [vp]
    lib.avf_write_merge_outputs.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, vp, C.POINTER(AvkMultiBatch), cpp,
                                            C.POINTER(C.c_int32), u8p, C.POINTER(C.c_uint64)]
    lib.avf_write_merge_summary.argtypes = [C.c_char_p, C.POINTER(AvkMultiBatch), cpp, C.POINTER(C.c_int32), u8p, C.POINTER(C.c_uint64)]
    lib.avf_write_merge_summary_counts.argtypes = [C.c_char_p, C.c_uint32, cpp, C.POINTER(C.c_uint64), C.c_uint64]
    lib.avf_calls_load.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.POINTER(vp)]
    lib.avf_calls_free.argtypes = [vp]
    lib.avf_feed_from_calls.argtypes = [C.c_uint32, C.POINTER(vp), C.c_char_p, vp, C.c_uint64, C.c_int, C.POINTER(vp)]
    lib.avf_vcf_sample_name.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint64]
    _lib = lib
    return lib


def _check(lib, rc):
    if rc:
        raise FeederError((lib.avf_last_error() or b"").decode(errors="replace"))


def _arr(ptr, n, dtype):
    if n == 0:
        return np.zeros(0, dtype)
    return np.ctypeslib.as_array(ptr, shape=(n,)).astype(dtype, copy=True)


class Genome:
    """ReferenceGenome::from_fasta: contigs in file order.  case: "upper" (default: soft-masked bases are loaded as upper case, like
    the tools' --reference-case upper) or "raw" (the file's bytes); see avf_genome_load_case in include/aardvark_feeder.h."""

    def __init__(self, fasta_path, case="upper"):
        if case not in ("upper", "raw"):
            raise ValueError("case must be 'upper' or 'raw'")
        self.lib = load_library()
        h = C.c_void_p()
        self.lib.avf_genome_load_case.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]
        _check(self.lib, self.lib.avf_genome_load_case(os.fsencode(fasta_path), 1 if case == "upper" else 0, C.byref(h)))
        self.handle = h
        n = self.lib.avf_genome_n_contigs(h)
        self.names = [self.lib.avf_genome_name(h, i).decode() for i in range(n)]

    def contigs(self):
        """list of numpy uint8 arrays (copies), in file order: what avk_ref_upload takes"""
        return [_arr(self.lib.avf_genome_seq(self.handle, i), int(self.lib.avf_genome_len(self.handle, i)), np.uint8) for i in range(len(self.names))]

    def close(self):
        if self.handle:
            self.lib.avf_genome_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Feed:
    """The result of RegionIterator over a truth/query VCF pair: a RegionBatch plus provenance; `packed` = the same batch in the packed form
    (avf_feed_pack -> PackedBatch; merge feeds: avf_feed_pack_multi -> merge.PackedMultiBatch), None when the call sets do not fit that form."""

    def __init__(self, batch, var_record, var_alt_index, loaded, packed=None, packed_esc=None):
        self.batch, self.var_record, self.var_alt_index, self.loaded, self.packed = batch, var_record, var_alt_index, loaded, packed
        # the feed packed WITH escapes (avf_feed_pack_esc / avf_feed_pack_multi_esc: a PackedBatch / PackedMultiBatch whose .escapes lists what the narrow fields
        # cannot hold), taken when the plain pack refused the feed; None otherwise, or when the wide form's own limits refuse it too
        self.packed_esc = packed_esc


_ALLOC = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_size_t)


def _escapes_of(esc, view):
    from ._abi import PackedEscapes
    nr, ns, nc = int(esc.n_esc_regions), int(esc.n_esc_slots), int(esc.n_esc_calls)
    return PackedEscapes(int(esc.first_region), int(esc.first_call), int(esc.first_slot), esc_region=view(esc.esc_region, nr, np.uint64), esc_len=view(esc.esc_len, nr, np.uint32),
                         esc_slot=view(esc.esc_slot, ns, np.uint64), esc_cnt=view(esc.esc_cnt, ns, np.uint32), esc_call=view(esc.esc_call, nc, np.uint64),
                         esc_rel_pos=view(esc.esc_rel_pos, nc, np.uint32), esc_a0_len=view(esc.esc_a0_len, nc, np.uint32), esc_a1_len=view(esc.esc_a1_len, nc, np.uint32))


def _take_packed_multi(lib, h, escapes=False):
    """avf_feed_pack_multi (escapes: avf_feed_pack_multi_esc) into numpy-owned buffers -> merge.PackedMultiBatch, or None when the feed does not fit the form"""
    from ._abi import AvkPackedEscapes
    from .merge import AvkPackedMultiBatch, PackedMultiBatch
    bufs = {}

    def alloc(_user, nbytes):
        a = np.empty(max(int(nbytes), 1), np.uint8)
        bufs[a.ctypes.data] = a
        return a.ctypes.data

    cb = _ALLOC(alloc)
    out = AvkPackedMultiBatch()
    esc = AvkPackedEscapes()
    lib.avf_feed_pack_multi.argtypes = [C.c_void_p, _ALLOC, C.c_void_p, C.POINTER(AvkPackedMultiBatch)]
    lib.avf_feed_pack_multi_esc.argtypes = [C.c_void_p, _ALLOC, C.c_void_p, C.POINTER(AvkPackedMultiBatch), C.POINTER(AvkPackedEscapes)]
    rc = lib.avf_feed_pack_multi_esc(h, cb, None, C.byref(out), C.byref(esc)) if escapes else lib.avf_feed_pack_multi(h, cb, None, C.byref(out))
    if rc == 1:
        return None
    _check(lib, rc)
    n, nv, na, k = int(out.n_regions), int(out.n_variants), int(out.allele_bytes_len), int(out.n_inputs)

    def view(ptr, count, dtype):
        addr = C.cast(ptr, C.c_void_p).value
        if addr is None:
            return None
        return bufs[addr][:count * np.dtype(dtype).itemsize].view(dtype)

    return PackedMultiBatch(k, escapes=_escapes_of(esc, view) if escapes else None, contig_idx=view(out.contig_idx, n, np.uint16), start=view(out.start, n, np.uint32), len=view(out.len, n, np.uint16),
                            in_cnt=view(out.in_cnt, n * k, np.uint8), var_rel_pos=view(out.var_rel_pos, nv, np.uint16), var_type_zyg=view(out.var_type_zyg, nv, np.uint8),
                            a0_len=view(out.a0_len, nv, np.uint8), a1_len=view(out.a1_len, nv, np.uint8), var_raw_space=view(out.var_raw_space, nv, np.uint32),
                            allele_bytes=view(out.allele_bytes, max(na, 1), np.uint8))


def _take_packed(lib, h, escapes=False):
    """avf_feed_pack (escapes: avf_feed_pack_esc) into numpy-owned buffers -> PackedBatch, or None when the feed does not fit the form"""
    from ._abi import AvkPackedBatch, AvkPackedEscapes, PackedBatch
    bufs = {}

    def alloc(_user, nbytes):
        a = np.empty(max(int(nbytes), 1), np.uint8)
        bufs[a.ctypes.data] = a
        return a.ctypes.data

    cb = _ALLOC(alloc)
    out = AvkPackedBatch()
    esc = AvkPackedEscapes()
    lib.avf_feed_pack.argtypes = [C.c_void_p, _ALLOC, C.c_void_p, C.POINTER(AvkPackedBatch)]
    lib.avf_feed_pack_esc.argtypes = [C.c_void_p, _ALLOC, C.c_void_p, C.POINTER(AvkPackedBatch), C.POINTER(AvkPackedEscapes)]
    rc = lib.avf_feed_pack_esc(h, cb, None, C.byref(out), C.byref(esc)) if escapes else lib.avf_feed_pack(h, cb, None, C.byref(out))
    if rc == 1:
        return None
    _check(lib, rc)
    n, nv, na = int(out.n_regions), int(out.n_variants), int(out.allele_bytes_len)

    def view(ptr, count, dtype):
        addr = C.cast(ptr, C.c_void_p).value
        if addr is None:
            return None
        return bufs[addr][:count * np.dtype(dtype).itemsize].view(dtype)

    return PackedBatch(escapes=_escapes_of(esc, view) if escapes else None, contig_idx=view(out.contig_idx, n, np.uint16), start=view(out.start, n, np.uint32),
                       len=view(out.len, n, np.uint16), t_cnt=view(out.t_cnt, n, np.uint8), q_cnt=view(out.q_cnt, n, np.uint8), var_rel_pos=view(out.var_rel_pos, nv, np.uint16),
                       var_type_zyg=view(out.var_type_zyg, nv, np.uint8), a0_len=view(out.a0_len, nv, np.uint8), a1_len=view(out.a1_len, nv, np.uint8),
                       var_raw_space=view(out.var_raw_space, nv, np.uint32), allele_bytes=view(out.allele_bytes, na, np.uint8))


def _both_packed(lib, h, merge):
    """(Feed.packed, Feed.packed_esc): the plain pack first, the pack with escapes when it refuses"""
    take = _take_packed_multi if merge else _take_packed
    plain = take(lib, h)
    return plain, (take(lib, h, escapes=True) if plain is None else None)


def vcf_sample_name(vcf, index=0):
    """get_vcf_sample_name: the name of sample `index` of the file's #CHROM line"""
    lib = load_library()
    buf = C.create_string_buffer(4096)
    _check(lib, lib.avf_vcf_sample_name(os.fsencode(vcf), index, buf, len(buf)))
    return buf.value.decode()


class Calls:
    """One VCF's calls, every chromosome (avf_calls_load): the first half of a feed, loadable while the genome is still loading."""

    def __init__(self, vcf, sample="", enable_trimming=True):
        self.lib = load_library()
        h = C.c_void_p()
        _check(self.lib, self.lib.avf_calls_load(os.fsencode(vcf), sample.encode(), 1 if enable_trimming else 0, C.byref(h)))
        self.handle = h

    def close(self):
        if self.handle:
            self.lib.avf_calls_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def feed_from_calls(calls, regions_bed, genome, min_variant_gap=50, merge=False):
    """avf_feed_from_calls: the region walk over loaded call sets -> the Feed of feed_compare (two inputs) or feed_merge"""
    lib = load_library()
    h = C.c_void_p()
    arr = (C.c_void_p * len(calls))(*[c.handle for c in calls])
    _check(lib, lib.avf_feed_from_calls(len(calls), arr, os.fsencode(regions_bed) if regions_bed else None, genome.handle, min_variant_gap, 1 if merge else 0, C.byref(h)))
    return _take_feed(lib, h, len(calls), merge)


def _take_feed(lib, h, k, merge):
    try:
        if merge:
            from .merge import MultiBatch
            b = lib.avf_feed_multi_batch(h).contents
            n, nv = int(b.n_regions), int(b.n_variants)
            batch = MultiBatch(k, region_id=_arr(b.region_id, n, np.uint64), contig_idx=_arr(b.contig_idx, n, np.uint32), start=_arr(b.start, n, np.uint64),
                               end=_arr(b.end, n, np.uint64), in_off=_arr(b.in_off, n * k, np.uint64), in_cnt=_arr(b.in_cnt, n * k, np.uint32),
                               var_pos=_arr(b.var_pos, nv, np.uint64), var_type=_arr(b.var_type, nv, np.uint8), var_zyg=_arr(b.var_zyg, nv, np.uint8),
                               var_raw_space=_arr(b.var_raw_space, nv, np.uint32), a0_off=_arr(b.a0_off, nv, np.uint64), a0_len=_arr(b.a0_len, nv, np.uint32),
                               a1_off=_arr(b.a1_off, nv, np.uint64), a1_len=_arr(b.a1_len, nv, np.uint32),
                               allele_bytes=_arr(b.allele_bytes, int(b.allele_bytes_len), np.uint8))
        else:
            b = lib.avf_feed_batch(h).contents
            n, nv = int(b.n_regions), int(b.n_variants)
            batch = RegionBatch(_arr(b.region_id, n, np.uint64), _arr(b.contig_idx, n, np.uint32), _arr(b.start, n, np.uint64), _arr(b.end, n, np.uint64),
                                _arr(b.t_off, n, np.uint64), _arr(b.t_cnt, n, np.uint32), _arr(b.q_off, n, np.uint64), _arr(b.q_cnt, n, np.uint32),
                                _arr(b.var_pos, nv, np.uint64), _arr(b.var_type, nv, np.uint8), _arr(b.var_zyg, nv, np.uint8), _arr(b.var_raw_space, nv, np.uint32),
                                _arr(b.a0_off, nv, np.uint64), _arr(b.a0_len, nv, np.uint32), _arr(b.a1_off, nv, np.uint64), _arr(b.a1_len, nv, np.uint32),
                                _arr(b.allele_bytes, int(b.allele_bytes_len), np.uint8))
        return Feed(batch, _arr(lib.avf_feed_var_record(h), nv, np.uint64), _arr(lib.avf_feed_var_alt_index(h), nv, np.uint32),
                    tuple(int(lib.avf_feed_loaded_variants(h, i)) for i in range(k)), *_both_packed(lib, h, merge))
    finally:
        lib.avf_feed_free(h)


def vcf_scores(vcf, field, n_records, sample=""):
    """avf_vcf_scores: the score of each of the first n_records data lines of a VCF -> float32 [n_records]; field: "QUAL" (column 6) or "GQ" (FORMAT/GQ of
    `sample`; "": the first sample); ".", an absent key or a value that is no number gives NaN"""
    lib = load_library()
    out = np.zeros(int(n_records), np.float32)
    lib.avf_vcf_scores.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint64, C.POINTER(C.c_float)]
    _check(lib, lib.avf_vcf_scores(os.fsencode(vcf), sample.encode(), field.encode(), int(n_records), out.ctypes.data_as(C.POINTER(C.c_float))))
    return out


def feed_compare(truth_vcf, query_vcf, regions_bed, genome, truth_sample="", query_sample="", min_variant_gap=50, enable_trimming=True, score_field=None):
    """score_field="QUAL" or "GQ": the feed also carries .scores, a float32 per call in the batch's (and the packed form's) call order — the query VCF's field
    gathered through var_record (avf_vcf_scores, avf_feed_scores); truth entries are NaN"""
    lib = load_library()
    h = C.c_void_p()
    _check(lib, lib.avf_feed_compare(os.fsencode(truth_vcf), truth_sample.encode(), os.fsencode(query_vcf), query_sample.encode(),
                                     os.fsencode(regions_bed) if regions_bed else None, genome.handle, min_variant_gap, 1 if enable_trimming else 0, C.byref(h)))
    try:
        b = lib.avf_feed_batch(h).contents
        n, nv = int(b.n_regions), int(b.n_variants)
        batch = RegionBatch(_arr(b.region_id, n, np.uint64), _arr(b.contig_idx, n, np.uint32), _arr(b.start, n, np.uint64), _arr(b.end, n, np.uint64),
                            _arr(b.t_off, n, np.uint64), _arr(b.t_cnt, n, np.uint32), _arr(b.q_off, n, np.uint64), _arr(b.q_cnt, n, np.uint32),
                            _arr(b.var_pos, nv, np.uint64), _arr(b.var_type, nv, np.uint8), _arr(b.var_zyg, nv, np.uint8), _arr(b.var_raw_space, nv, np.uint32),
                            _arr(b.a0_off, nv, np.uint64), _arr(b.a0_len, nv, np.uint32), _arr(b.a1_off, nv, np.uint64), _arr(b.a1_len, nv, np.uint32),
                            _arr(b.allele_bytes, int(b.allele_bytes_len), np.uint8))
        feed = Feed(batch, _arr(lib.avf_feed_var_record(h), nv, np.uint64), _arr(lib.avf_feed_var_alt_index(h), nv, np.uint32),
                    (int(lib.avf_feed_loaded_variants(h, 0)), int(lib.avf_feed_loaded_variants(h, 1))), *_both_packed(lib, h, False))
        feed.scores = None
        if score_field is not None:
            n_records = int(feed.var_record.max()) + 1 if nv else 0
            per_record = vcf_scores(query_vcf, score_field, n_records, query_sample)
            feed.scores = np.zeros(nv, np.float32)
            f32p = C.POINTER(C.c_float)
            lib.avf_feed_scores.argtypes = [C.c_void_p, f32p, C.c_uint64, f32p]
            _check(lib, lib.avf_feed_scores(h, per_record.ctypes.data_as(f32p), n_records, feed.scores.ctypes.data_as(f32p)))
        return feed
    finally:
        lib.avf_feed_free(h)


def write_summary(path, tally, compare_label="compare", metrics=METRIC_GT | METRIC_BASEPAIR):
    lib = load_library()
    t = np.ascontiguousarray(tally, dtype=np.uint64)
    _check(lib, lib.avf_write_summary(os.fsencode(path), compare_label.encode(), t.ctypes.data_as(C.POINTER(C.c_uint64)), metrics))


def write_annotated_vcf(out_path, input_vcf, genome, batch, result, source, sample_name="", version="aardvark_amd", command_line=""):
    """truth.vcf.gz (source 0) or query.vcf.gz (source 1) of `compare` + its .tbi; `result` is the ResultBatch of `batch`."""
    lib = load_library()
    cb = batch.c_struct()
    u8 = lambda a: np.ascontiguousarray(a, np.uint8).ctypes.data_as(C.POINTER(C.c_uint8))
    st = np.ascontiguousarray(result.status, np.int32)
    keep = [np.ascontiguousarray(x, np.uint8) for x in (result.var_expected, result.var_observed, result.var_class)]
    _check(lib, lib.avf_write_annotated_vcf(os.fsencode(out_path), os.fsencode(input_vcf), sample_name.encode(), version.encode(), command_line.encode(),
                                            genome.handle, C.byref(cb), source, st.ctypes.data_as(C.POINTER(C.c_int32)), u8(keep[0]), u8(keep[1]), u8(keep[2])))


class Stratifications:
    """Stratifications::from_tsv_batch (src/parsing/stratifications.rs): labelled BED sets, labels in sorted order."""

    def __init__(self, tsv_path):
        self.lib = load_library()
        h = C.c_void_p()
        _check(self.lib, self.lib.avf_strat_load(os.fsencode(tsv_path), C.byref(h)))
        self.handle = h
        self.labels = [self.lib.avf_strat_label(h, i).decode() for i in range(self.lib.avf_strat_n_labels(h))]

    def _query(self, fn, chrom, first, last):
        out = (C.c_uint32 * max(len(self.labels), 1))()
        n = fn(self.handle, chrom.encode(), first, last, out, len(self.labels))
        return [int(out[i]) for i in range(n)]

    def containments(self, chrom, first, last):
        return self._query(self.lib.avf_strat_containments, chrom, first, last)

    def overlaps(self, chrom, first, last):
        return self._query(self.lib.avf_strat_overlaps, chrom, first, last)

    def n_intervals(self, label, chrom):
        return int(self.lib.avf_strat_n_intervals(self.handle, label, chrom.encode()))

    def region_labels(self, genome, batch, r):
        cb = batch.c_struct()
        out = (C.c_uint32 * max(len(self.labels), 1))()
        n = self.lib.avf_strat_region_labels(self.handle, genome.handle, C.byref(cb), r, out, len(self.labels))
        return [int(out[i]) for i in range(n)]

    def batch_labels(self, genome, batch, first=0, n=None):
        """avf_strat_batch_labels: (label_off[n + 1], label_idx) — the labels of region first + k are label_idx[label_off[k]:label_off[k + 1]]"""
        n = batch.n_regions - first if n is None else n
        cb = batch.c_struct()
        off = np.zeros(n + 1, np.uint64)
        u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
        _check(self.lib, self.lib.avf_strat_batch_labels(self.handle, genome.handle, C.byref(cb), first, n, off.ctypes.data_as(u64p), None))
        idx = np.zeros(int(off[n]) + 1, np.uint32)
        _check(self.lib, self.lib.avf_strat_batch_labels(self.handle, genome.handle, C.byref(cb), first, n, off.ctypes.data_as(u64p), idx.ctypes.data_as(u32p)))
        return off, idx[:int(off[n])]

    def export(self, genome):
        """avf_strat_export: the sets as avk_strata_upload takes them -> (n_labels, n_contigs, tree_off, start, end_max); tree (label l, contig c of `genome`) is
        entries tree_off[l * n_contigs + c] .. tree_off[l * n_contigs + c + 1] of start (sorted) and end_max (running maximum of the exclusive ends), 32-bit"""
        n_labels, n_contigs = len(self.labels), len(genome.names)
        u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
        tree_off = np.zeros(n_labels * n_contigs + 1, np.uint64)
        _check(self.lib, self.lib.avf_strat_export(self.handle, genome.handle, tree_off.ctypes.data_as(u64p), None, None))
        total = int(tree_off[-1])
        start, end_max = np.zeros(max(total, 1), np.uint32), np.zeros(max(total, 1), np.uint32)
        _check(self.lib, self.lib.avf_strat_export(self.handle, genome.handle, tree_off.ctypes.data_as(u64p), start.ctypes.data_as(u32p), end_max.ctypes.data_as(u32p)))
        return n_labels, n_contigs, tree_off, start[:total], end_max[:total]

    def close(self):
        if self.handle:
            self.lib.avf_strat_free(self.handle)
            self.handle = None


def write_summary_stratified(path, tally, strat, strat_tallies, compare_label="compare", metrics=METRIC_GT | METRIC_BASEPAIR):
    lib = load_library()
    t = np.ascontiguousarray(tally, dtype=np.uint64)
    st = np.ascontiguousarray(strat_tallies, dtype=np.uint64).reshape(-1)
    _check(lib, lib.avf_write_summary_stratified(os.fsencode(path), compare_label.encode(), t.ctypes.data_as(C.POINTER(C.c_uint64)), strat.handle,
                                                 st.ctypes.data_as(C.POINTER(C.c_uint64)), metrics))


def write_summary_named(path, tally, names, strat_tallies, compare_label="compare", metrics=METRIC_GT | METRIC_BASEPAIR):
    """avf_write_summary_named: write_summary_stratified with the labels' names as a list (the sets' labels, then e.g. ContextSpec.names())"""
    lib = load_library()
    u64p = C.POINTER(C.c_uint64)
    t = np.ascontiguousarray(tally, dtype=np.uint64)
    st = np.ascontiguousarray(strat_tallies, dtype=np.uint64).reshape(-1)
    arr = (C.c_char_p * len(names))(*[n.encode() for n in names]) if names else None
    _check(lib, lib.avf_write_summary_named(os.fsencode(path), compare_label.encode(), t.ctypes.data_as(u64p), len(names), arr, st.ctypes.data_as(u64p), metrics))


def write_summary_size(path, bin_names, names, size_blocks, compare_label="compare", metrics=METRIC_GT | METRIC_HAP | METRIC_WEIGHTED_HAP):
    """avf_write_summary_size: summary_size.tsv — the rows of write_summary_named per scope (ALL, then `names`) and size bin, the bin's name in the `filter` column;
    size_blocks is [1 + len(names), len(bin_names), N_GROUPS, 14] (Context.size_tallies' layout).  BASEPAIR and RECORD_BP bits of `metrics` are ignored"""
    lib = load_library()
    u64p = C.POINTER(C.c_uint64)
    sb = np.ascontiguousarray(size_blocks, dtype=np.uint64)
    if sb.ndim != 4 or sb.shape[0] != 1 + len(names) or sb.shape[1] != len(bin_names) or sb.shape[3] != 14:
        raise ValueError("size_blocks is [1 + labels, bins, N_GROUPS, 14]")
    arr = (C.c_char_p * len(names))(*[n.encode() for n in names]) if names else None
    bins = (C.c_char_p * len(bin_names))(*[b.encode() for b in bin_names])
    lib.avf_write_summary_size.argtypes = [C.c_char_p, C.c_char_p, C.c_uint32, C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(C.c_char_p), u64p, C.c_uint32]
    _check(lib, lib.avf_write_summary_size(os.fsencode(path), compare_label.encode(), len(bin_names), bins, len(names), arr, sb.reshape(-1).ctypes.data_as(u64p), metrics))


def write_summary_roc(path, point_names, names, score_blocks, compare_label="compare", metrics=METRIC_GT | METRIC_HAP | METRIC_WEIGHTED_HAP):
    """avf_write_summary_roc: summary_roc.tsv — the rows of write_summary_named per scope (ALL, then `names`) and point of the curve by query score, the point's
    name in the `filter` column; score_blocks is [1 + len(names), len(point_names), N_GROUPS, 14] (Context.score_tallies' layout).  BASEPAIR and RECORD_BP bits of
    `metrics` are ignored"""
    lib = load_library()
    u64p = C.POINTER(C.c_uint64)
    sb = np.ascontiguousarray(score_blocks, dtype=np.uint64)
    if sb.ndim != 4 or sb.shape[0] != 1 + len(names) or sb.shape[1] != len(point_names) or sb.shape[3] != 14:
        raise ValueError("score_blocks is [1 + labels, points, N_GROUPS, 14]")
    arr = (C.c_char_p * len(names))(*[n.encode() for n in names]) if names else None
    points = (C.c_char_p * len(point_names))(*[b.encode() for b in point_names])
    lib.avf_write_summary_roc.argtypes = [C.c_char_p, C.c_char_p, C.c_uint32, C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(C.c_char_p), u64p, C.c_uint32]
    _check(lib, lib.avf_write_summary_roc(os.fsencode(path), compare_label.encode(), len(point_names), points, len(names), arr, sb.reshape(-1).ctypes.data_as(u64p), metrics))


def _kind_blocks(names, kind_blocks):
    kb = np.ascontiguousarray(kind_blocks, dtype=np.uint64)
    if kb.ndim != 4 or kb.shape[0] != 1 + len(names) or kb.shape[1] != 9 or kb.shape[3] != 14:
        raise ValueError("kind_blocks is [1 + labels, 9, N_GROUPS, 14]")
    return kb, (C.c_char_p * len(names))(*[n.encode() for n in names]) if names else None


def write_summary_kind(path, names, kind_blocks, compare_label="compare", metrics=METRIC_GT | METRIC_HAP | METRIC_WEIGHTED_HAP):
    """avf_write_summary_kind: summary_kind.tsv — the rows of write_summary_named per scope (ALL, then `names`) and call kind (het / hom x Ti / Tv), the kind's name in
    the `filter` column; kind_blocks is [1 + len(names), 9, N_GROUPS, 14] (Context.kind_tallies' layout).  BASEPAIR and RECORD_BP bits of `metrics` are ignored"""
    lib = load_library()
    u64p = C.POINTER(C.c_uint64)
    kb, arr = _kind_blocks(names, kind_blocks)
    lib.avf_write_summary_kind.argtypes = [C.c_char_p, C.c_char_p, C.c_uint32, C.POINTER(C.c_char_p), u64p, C.c_uint32]
    _check(lib, lib.avf_write_summary_kind(os.fsencode(path), compare_label.encode(), len(names), arr, kb.reshape(-1).ctypes.data_as(u64p), metrics))


def write_kind_ratios(path, names, kind_blocks, compare_label="compare"):
    """avf_write_kind_ratios: kind_ratios.tsv — Ti/Tv and het/hom of the GT counts per scope (ALL, then `names`), variant type and set (truth_total .. query_fp);
    kind_blocks as for write_summary_kind"""
    lib = load_library()
    u64p = C.POINTER(C.c_uint64)
    kb, arr = _kind_blocks(names, kind_blocks)
    lib.avf_write_kind_ratios.argtypes = [C.c_char_p, C.c_char_p, C.c_uint32, C.POINTER(C.c_char_p), u64p]
    _check(lib, lib.avf_write_kind_ratios(os.fsencode(path), compare_label.encode(), len(names), arr, kb.reshape(-1).ctypes.data_as(u64p)))


def write_summary_ci(path, tally, names, strat_tallies, boot_blocks, level=95, compare_label="compare", metrics=METRIC_GT | METRIC_BASEPAIR):
    """avf_write_summary_ci: the rows of write_summary_named with percentile intervals of recall, precision and F1 over the bootstrap replicates `boot_blocks`
    ([1 + len(names), replicates, TALLY_LEN], Context.boot_tallies' layout); level: 90, 95 or 99"""
    lib = load_library()
    u64p = C.POINTER(C.c_uint64)
    t = np.ascontiguousarray(tally, dtype=np.uint64)
    st = np.ascontiguousarray(strat_tallies if len(names) else np.zeros(1), dtype=np.uint64).reshape(-1)
    bb = np.ascontiguousarray(boot_blocks, dtype=np.uint64)
    if bb.ndim != 3 or bb.shape[0] != 1 + len(names):
        raise ValueError("boot_blocks is [1 + labels, replicates, TALLY_LEN]")
    arr = (C.c_char_p * len(names))(*[n.encode() for n in names]) if names else None
    lib.avf_write_summary_ci.argtypes = [C.c_char_p, C.c_char_p, u64p, C.c_uint32, C.POINTER(C.c_char_p), u64p, C.c_uint32, C.c_uint32, u64p, C.c_uint32]
    _check(lib, lib.avf_write_summary_ci(os.fsencode(path), compare_label.encode(), t.ctypes.data_as(u64p), len(names), arr, st.ctypes.data_as(u64p), metrics, bb.shape[1],
                                         bb.reshape(-1).ctypes.data_as(u64p), int(level)))


def _boot_blocks(names, keys, boot_blocks):
    bb = np.ascontiguousarray(boot_blocks, dtype=np.uint64)
    if bb.ndim != 5 or bb.shape[0] != 1 + len(names) or bb.shape[2] != keys or bb.shape[4] != 14 or bb.shape[1] < 1:
        raise ValueError("boot_blocks is [1 + labels, replicates, %d, N_GROUPS, 14]" % keys)
    return bb


def write_summary_size_ci(path, bin_names, names, size_blocks, boot_blocks, level=95, compare_label="compare", metrics=METRIC_GT | METRIC_HAP | METRIC_WEIGHTED_HAP):
    """avf_write_summary_size_ci: summary_size_ci.tsv — write_summary_size's rows with write_summary_ci's ten interval columns over the replicates `boot_blocks`
    ([1 + len(names), replicates, len(bin_names), N_GROUPS, 14], Context.size_boot_tallies' layout); level: 90, 95 or 99"""
    lib = load_library()
    u64p = C.POINTER(C.c_uint64)
    sb = np.ascontiguousarray(size_blocks, dtype=np.uint64)
    if sb.ndim != 4 or sb.shape[0] != 1 + len(names) or sb.shape[1] != len(bin_names) or sb.shape[3] != 14:
        raise ValueError("size_blocks is [1 + labels, bins, N_GROUPS, 14]")
    bb = _boot_blocks(names, len(bin_names), boot_blocks)
    arr = (C.c_char_p * len(names))(*[n.encode() for n in names]) if names else None
    bins = (C.c_char_p * len(bin_names))(*[b.encode() for b in bin_names])
    lib.avf_write_summary_size_ci.argtypes = [C.c_char_p, C.c_char_p, C.c_uint32, C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(C.c_char_p), u64p, C.c_uint32, C.c_uint32, u64p, C.c_uint32]
    _check(lib, lib.avf_write_summary_size_ci(os.fsencode(path), compare_label.encode(), len(bin_names), bins, len(names), arr, sb.reshape(-1).ctypes.data_as(u64p), metrics, bb.shape[1],
                                              bb.reshape(-1).ctypes.data_as(u64p), int(level)))


def write_summary_kind_ci(path, names, kind_blocks, boot_blocks, level=95, compare_label="compare", metrics=METRIC_GT | METRIC_HAP | METRIC_WEIGHTED_HAP):
    """avf_write_summary_kind_ci: summary_kind_ci.tsv — write_summary_kind's rows with the interval columns; boot_blocks is Context.kind_boot_tallies' layout"""
    lib = load_library()
    u64p = C.POINTER(C.c_uint64)
    kb, arr = _kind_blocks(names, kind_blocks)
    bb = _boot_blocks(names, 9, boot_blocks)
    lib.avf_write_summary_kind_ci.argtypes = [C.c_char_p, C.c_char_p, C.c_uint32, C.POINTER(C.c_char_p), u64p, C.c_uint32, C.c_uint32, u64p, C.c_uint32]
    _check(lib, lib.avf_write_summary_kind_ci(os.fsencode(path), compare_label.encode(), len(names), arr, kb.reshape(-1).ctypes.data_as(u64p), metrics, bb.shape[1],
                                              bb.reshape(-1).ctypes.data_as(u64p), int(level)))


def write_kind_ratios_ci(path, names, kind_blocks, boot_blocks, level=95, compare_label="compare"):
    """avf_write_kind_ratios_ci: kind_ratios_ci.tsv — write_kind_ratios' rows followed by titv_lo titv_hi hethom_lo hethom_hi replicates"""
    lib = load_library()
    u64p = C.POINTER(C.c_uint64)
    kb, arr = _kind_blocks(names, kind_blocks)
    bb = _boot_blocks(names, 9, boot_blocks)
    lib.avf_write_kind_ratios_ci.argtypes = [C.c_char_p, C.c_char_p, C.c_uint32, C.POINTER(C.c_char_p), u64p, C.c_uint32, u64p, C.c_uint32]
    _check(lib, lib.avf_write_kind_ratios_ci(os.fsencode(path), compare_label.encode(), len(names), arr, kb.reshape(-1).ctypes.data_as(u64p), bb.shape[1],
                                             bb.reshape(-1).ctypes.data_as(u64p), int(level)))


def write_debug_tables(summary_path, sequences_path, genome, batch, result, metrics=METRIC_GT | METRIC_BASEPAIR):
    """region_summary.tsv.gz and region_sequences.tsv.gz of --output-debug for one batch and its ResultBatch (with sequences)."""
    lib = load_library()
    cb = batch.c_struct()
    st = np.ascontiguousarray(result.status, np.int32)
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    for path, is_seq in ((summary_path, False), (sequences_path, True)):
        if not path:
            continue
        h = C.c_void_p()
        if is_seq:
            _check(lib, lib.avf_region_sequences_open(os.fsencode(path), C.byref(h)))
            rc = lib.avf_region_sequences_rows(h, genome.handle, C.byref(cb), 0, batch.n_regions, P(st, C.c_int32), P(result.seq_bytes, C.c_uint8),
                                               P(np.ascontiguousarray(result.seq_len, np.uint32), C.c_uint32), P(result.seq_off, C.c_uint64), P(result.seq_stride, C.c_uint32))
        else:
            _check(lib, lib.avf_region_summary_open(os.fsencode(path), metrics, C.byref(h)))
            gm = np.ascontiguousarray(result.group_metrics, np.uint32)
            rc = lib.avf_region_summary_rows(h, genome.handle, C.byref(cb), 0, batch.n_regions, P(st, C.c_int32), P(gm, C.c_uint32))
        rc2 = lib.avf_table_close(h)
        _check(lib, rc or rc2)


# ---- merge (src/main.rs run_merge: region generation over k VCFs, VariantMerger, MergeSummaryWriter) -----------------------------------
def _strs(items):
    arr = (C.c_char_p * len(items))(*[os.fsencode(x) if x is not None else None for x in items])
    return arr


def feed_merge(vcfs, regions_bed, genome, samples=None, min_variant_gap=50, enable_trimming=True):
    """RegionIterator::new_merge_iterator + the iterator: a merge.MultiBatch plus provenance (Feed.batch is the MultiBatch)."""
    from .merge import MultiBatch
    lib = load_library()
    h = C.c_void_p()
    k = len(vcfs)
    samples = list(samples or []) + [""] * (k - len(samples or []))
    _check(lib, lib.avf_feed_merge(k, _strs(vcfs), _strs(samples), os.fsencode(regions_bed) if regions_bed else None, genome.handle, min_variant_gap,
                                   1 if enable_trimming else 0, C.byref(h)))
    try:
        b = lib.avf_feed_multi_batch(h).contents
        n, nv = int(b.n_regions), int(b.n_variants)
        mb = MultiBatch(k, region_id=_arr(b.region_id, n, np.uint64), contig_idx=_arr(b.contig_idx, n, np.uint32), start=_arr(b.start, n, np.uint64),
                        end=_arr(b.end, n, np.uint64), in_off=_arr(b.in_off, n * k, np.uint64), in_cnt=_arr(b.in_cnt, n * k, np.uint32),
                        var_pos=_arr(b.var_pos, nv, np.uint64), var_type=_arr(b.var_type, nv, np.uint8), var_zyg=_arr(b.var_zyg, nv, np.uint8),
                        var_raw_space=_arr(b.var_raw_space, nv, np.uint32), a0_off=_arr(b.a0_off, nv, np.uint64), a0_len=_arr(b.a0_len, nv, np.uint32),
                        a1_off=_arr(b.a1_off, nv, np.uint64), a1_len=_arr(b.a1_len, nv, np.uint32),
                        allele_bytes=_arr(b.allele_bytes, int(b.allele_bytes_len), np.uint8))
        return Feed(mb, _arr(lib.avf_feed_var_record(h), nv, np.uint64), _arr(lib.avf_feed_var_alt_index(h), nv, np.uint32),
                    tuple(int(lib.avf_feed_loaded_variants(h, i)) for i in range(k)), *_both_packed(lib, h, True))
    finally:
        lib.avf_feed_free(h)


def _merge_args(mb, result):
    st = np.ascontiguousarray(result.status, np.int32)
    cls = np.ascontiguousarray(result.classification, np.uint8)
    mem = np.ascontiguousarray(result.members, np.uint64)
    if st.size == 0:
        st, cls, mem = np.zeros(1, np.int32), np.zeros(1, np.uint8), np.zeros(1, np.uint64)
    return st, cls, mem


def write_merge_outputs(out_folder, primary_vcf, genome, mb, result, tags=None, sample_name="", version="aardvark_amd", command_line=""):
    """passing.vcf.gz, regions.bed.gz, failed_regions.bed.gz (+ .tbi each) of `merge`; result = merge.MergeResult of `mb`"""
    lib = load_library()
    tags = list(tags) if tags else ["vcf_%d" % i for i in range(mb.n_inputs)]
    st, cls, mem = _merge_args(mb, result)
    cb = mb.c_struct()
    _check(lib, lib.avf_write_merge_outputs(os.fsencode(out_folder), os.fsencode(primary_vcf), sample_name.encode(), version.encode(), command_line.encode(),
                                            genome.handle, C.byref(cb), _strs(tags), st.ctypes.data_as(C.POINTER(C.c_int32)),
                                            cls.ctypes.data_as(C.POINTER(C.c_uint8)), mem.ctypes.data_as(C.POINTER(C.c_uint64))))


def write_merge_summary(path, mb, result, tags=None):
    lib = load_library()
    tags = list(tags) if tags else ["vcf_%d" % i for i in range(mb.n_inputs)]
    st, cls, mem = _merge_args(mb, result)
    cb = mb.c_struct()
    _check(lib, lib.avf_write_merge_summary(os.fsencode(path), C.byref(cb), _strs(tags), st.ctypes.data_as(C.POINTER(C.c_int32)),
                                            cls.ctypes.data_as(C.POINTER(C.c_uint8)), mem.ctypes.data_as(C.POINTER(C.c_uint64))))


def write_merge_summary_counts(path, n_inputs, counts, tags=None):
    """the merge summary table from the dense block of sums of a sharded merge (aardvark_amd.merge.merge_counts, summed over the ranks)"""
    lib = load_library()
    tags = list(tags) if tags else ["vcf_%d" % i for i in range(n_inputs)]
    counts = np.ascontiguousarray(counts, np.uint64)
    _check(lib, lib.avf_write_merge_summary_counts(os.fsencode(path), n_inputs, _strs(tags), counts.ctypes.data_as(C.POINTER(C.c_uint64)), counts.size))
