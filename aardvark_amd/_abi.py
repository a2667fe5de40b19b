"""ctypes mirror of include/aardvark_amd.h plus the flat batch containers.

Plumbing only: the structures here are bit-for-bit the C-ABI structs; `RegionBatch` packs
Python-side regions into the structure-of-arrays layout the library takes and `ResultBatch`
owns the caller-allocated output arrays.
"""
import ctypes as C

import numpy as np

# ---- enums (ordinals of the reference's Rust enums; include/aardvark_amd.h) -------------
VARIANT_TYPES = [
    "Snv", "Insertion", "Deletion", "Indel", "SvInsertion", "SvDeletion", "SvDuplication",
    "SvInversion", "SvBreakend", "TrContraction", "TrExpansion", "Unknown",
]
VT = {n: i for i, n in enumerate(VARIANT_TYPES)}
ZYGOSITIES = [
    "Unknown", "HomozygousReference", "UnphasedHeterozygous", "PhasedHet01", "PhasedHet10",
    "HomozygousAlternate",
]
ZYG = {n: i for i, n in enumerate(ZYGOSITIES)}
CLASSES = ["UNK", "TP", "FN", "FP"]
CLS = {n: i for i, n in enumerate(CLASSES)}
ALLELE = {"UNK": 0, "REF": 1, "ALT": 2}

N_GROUPS = 13
N_FIELDS = 22
TALLY_LEN = N_GROUPS * N_FIELDS + 2
FIELDS = [
    "GT_TRUTH_TP", "GT_TRUTH_FN", "GT_QUERY_TP", "GT_QUERY_FP", "GT_TRUTH_FN_GT", "GT_QUERY_FP_GT",
    "HAP_TRUTH_TP", "HAP_TRUTH_FN", "HAP_QUERY_TP", "HAP_QUERY_FP",
    "WHAP_TRUTH_TP", "WHAP_TRUTH_FN", "WHAP_QUERY_TP", "WHAP_QUERY_FP",
    "BP_TRUTH_TP", "BP_TRUTH_FN", "BP_QUERY_TP", "BP_QUERY_FP",
    "RBP_TRUTH_TP", "RBP_TRUTH_FN", "RBP_QUERY_TP", "RBP_QUERY_FP",
]
F = {n: i for i, n in enumerate(FIELDS)}

ST_OK = 0
ST_NAMES = {
    0: "OK", 2: "BRANCH_FACTOR", 3: "NO_RESULTS", 4: "NO_GT_RESULT", 5: "UNKNOWN_ALLELE",
    6: "BAD_ZYGOSITY", 7: "VARIANT_METRICS", 8: "TRUTH_FP", 9: "RECORD_BP", 10: "SEQ_MISMATCH",
    11: "AUTOFAIL_OOB", 20: "INVALID_INPUT", 21: "CAPACITY",
}

MERGE_SWEEP_MAX = 8  # AVK_MERGE_SWEEP_MAX: the configs one avk_merge_packed_sweep / avk_merge_classify_sweep decides on top of one pair solve

_p = C.POINTER


class AvkRegionBatch(C.Structure):
    _fields_ = [
        ("n_regions", C.c_uint64),
        ("region_id", _p(C.c_uint64)),
        ("contig_idx", _p(C.c_uint32)),
        ("start", _p(C.c_uint64)),
        ("end", _p(C.c_uint64)),
        ("t_off", _p(C.c_uint64)),
        ("t_cnt", _p(C.c_uint32)),
        ("q_off", _p(C.c_uint64)),
        ("q_cnt", _p(C.c_uint32)),
        ("n_variants", C.c_uint64),
        ("var_pos", _p(C.c_uint64)),
        ("var_type", _p(C.c_uint8)),
        ("var_zyg", _p(C.c_uint8)),
        ("var_raw_space", _p(C.c_uint32)),
        ("a0_off", _p(C.c_uint64)),
        ("a0_len", _p(C.c_uint32)),
        ("a1_off", _p(C.c_uint64)),
        ("a1_len", _p(C.c_uint32)),
        ("allele_bytes", _p(C.c_uint8)),
        ("allele_bytes_len", C.c_uint64),
    ]


class AvkCompactBatch(C.Structure):
    _fields_ = [
        ("n_regions", C.c_uint64),
        ("contig_idx", _p(C.c_uint32)),
        ("start", _p(C.c_uint32)),
        ("len", _p(C.c_uint32)),
        ("v_off", _p(C.c_uint32)),
        ("t_cnt", _p(C.c_uint16)),
        ("q_cnt", _p(C.c_uint16)),
        ("n_variants", C.c_uint64),
        ("var_pos", _p(C.c_uint32)),
        ("var_type_zyg", _p(C.c_uint8)),
        ("a_off", _p(C.c_uint32)),
        ("a0_len", _p(C.c_uint32)),
        ("a1_len", _p(C.c_uint32)),
        ("var_raw_space", _p(C.c_uint32)),
        ("allele_bytes", _p(C.c_uint8)),
        ("allele_bytes_len", C.c_uint64),
    ]


class AvkPackedBatch(C.Structure):
    _fields_ = [
        ("n_regions", C.c_uint64),
        ("contig_idx", _p(C.c_uint16)),
        ("start", _p(C.c_uint32)),
        ("len", _p(C.c_uint16)),
        ("t_cnt", _p(C.c_uint8)),
        ("q_cnt", _p(C.c_uint8)),
        ("n_variants", C.c_uint64),
        ("var_rel_pos", _p(C.c_uint16)),
        ("var_type_zyg", _p(C.c_uint8)),
        ("a0_len", _p(C.c_uint8)),
        ("a1_len", _p(C.c_uint8)),
        ("var_raw_space", _p(C.c_uint32)),
        ("allele_bytes", _p(C.c_uint8)),
        ("allele_bytes_len", C.c_uint64),
    ]


class AvkPackedEscapes(C.Structure):
    _fields_ = [
        ("first_region", C.c_uint64),
        ("first_call", C.c_uint64),
        ("first_slot", C.c_uint64),
        ("n_esc_regions", C.c_uint64),
        ("esc_region", _p(C.c_uint64)),
        ("esc_len", _p(C.c_uint32)),
        ("n_esc_slots", C.c_uint64),
        ("esc_slot", _p(C.c_uint64)),
        ("esc_cnt", _p(C.c_uint32)),
        ("n_esc_calls", C.c_uint64),
        ("esc_call", _p(C.c_uint64)),
        ("esc_rel_pos", _p(C.c_uint32)),
        ("esc_a0_len", _p(C.c_uint32)),
        ("esc_a1_len", _p(C.c_uint32)),
    ]


class AvkRegionLabels(C.Structure):
    """avk_region_labels: the containment labels of a batch's regions (label_idx[label_off[r] .. label_off[r + 1]) are region r's)"""
    _fields_ = [
        ("n_labels", C.c_uint32),
        ("label_off", _p(C.c_uint64)),
        ("label_idx", _p(C.c_uint32)),
    ]


def region_labels(n_labels, label_off, label_idx):
    """(AvkRegionLabels, the arrays it points into) from the three parts of a labels=(n_labels, off, idx) argument"""
    off = np.ascontiguousarray(label_off, np.uint64)
    idx = np.ascontiguousarray(label_idx, np.uint32)
    if idx.size == 0:
        idx = np.zeros(1, np.uint32)
    return AvkRegionLabels(int(n_labels), off.ctypes.data_as(_p(C.c_uint64)), idx.ctypes.data_as(_p(C.c_uint32))), (off, idx)


class AvkCompareConfig(C.Structure):
    _fields_ = [
        ("max_branch_factor", C.c_uint32),
        ("enable_sequences", C.c_uint32),
        ("enable_exact_shortcut", C.c_uint32),
    ]


class AvkResultBatch(C.Structure):
    _fields_ = [
        ("status", _p(C.c_int32)),
        ("ed_h1", _p(C.c_uint32)),
        ("ed_h2", _p(C.c_uint32)),
        ("n_optima", _p(C.c_uint32)),
        ("type_present", _p(C.c_uint16)),
        ("group_metrics", _p(C.c_uint32)),
        ("var_expected", _p(C.c_uint8)),
        ("var_observed", _p(C.c_uint8)),
        ("var_class", _p(C.c_uint8)),
        ("var_zyg", _p(C.c_uint8)),
        ("seq_bytes", _p(C.c_uint8)),
        ("seq_off", _p(C.c_uint64)),
        ("seq_stride", _p(C.c_uint32)),
        ("seq_len", _p(C.c_uint32)),
        ("tally", _p(C.c_uint64)),
        ("bp_off", _p(C.c_uint32)),
        ("bp_groups", _p(C.c_uint32)),
        ("region_packed", _p(C.c_uint64)),
        ("var_packed", _p(C.c_uint8)),
        ("bp_packed", _p(C.c_uint32)),
        ("bp_spilled", _p(C.c_uint32)),
    ]


def declare_submit_strata(lib):
    """avk_compare_packed_submit_strata(avk_ctx *, const avk_packed_batch *, const avk_packed_escapes *, const avk_strata *, const avk_compare_config *,
    avk_result_batch *, uint64_t *label_tallies, avk_ticket **) -> int: the submit with the resident sets' handle in place of label lists"""
    vp = C.c_void_p
    lib.avk_compare_packed_submit_strata.restype = C.c_int
    lib.avk_compare_packed_submit_strata.argtypes = [vp, _p(AvkPackedBatch), _p(AvkPackedEscapes), vp, _p(AvkCompareConfig), _p(AvkResultBatch), _p(C.c_uint64), _p(vp)]


BOOT_MAX_REPLICATES, BOOT_MAX_BLOCKS = 4096, 16384


class AvkBootSpec(C.Structure):
    """avk_boot_spec: the bootstrap replicates of a call (aardvark_amd/csrc/avk_boot.h has the rule)"""
    _fields_ = [("replicates", C.c_uint32), ("seed", C.c_uint64)]


class BootSpec:
    """`replicates` Poisson-bootstrap replicates of the tallies (1 .. 4096; with a strata handle of L labels (1 + L) * replicates <= 16384), drawn with `seed`"""

    def __init__(self, replicates, seed=1):
        self.replicates, self.seed = int(replicates), int(seed)

    def c_struct(self):
        return AvkBootSpec(self.replicates, self.seed & 0xFFFFFFFFFFFFFFFF)


def declare_boot(lib):
    """avk_boot_block, avk_boot_tallies, avk_compare_packed_boot, avk_boot_tallies_host (include/aardvark_amd.h)"""
    vp, u64p = C.c_void_p, _p(C.c_uint64)
    lib.avk_boot_block.restype = C.c_uint32
    lib.avk_boot_block.argtypes = [vp]
    lib.avk_boot_tallies.restype = C.c_int
    lib.avk_boot_tallies.argtypes = [vp, vp, _p(AvkBootSpec), vp, u64p]
    lib.avk_compare_packed_boot.restype = C.c_int
    lib.avk_compare_packed_boot.argtypes = [vp, _p(AvkPackedBatch), _p(AvkPackedEscapes), vp, _p(AvkCompareConfig), _p(AvkResultBatch), u64p, _p(AvkBootSpec), u64p]
    lib.avk_boot_tallies_host.restype = C.c_int
    lib.avk_boot_tallies_host.argtypes = [_p(AvkRegionBatch), _p(AvkResultBatch), _p(AvkBootSpec), _p(AvkRegionLabels), C.c_uint32, u64p]


SIZE_EDGES_MAX, SIZE_FIELDS = 15, 14


class AvkSizeSpec(C.Structure):
    """avk_size_spec: the edges of the size bins (aardvark_amd/csrc/avk_sizebin.h has the rule)"""
    _fields_ = [("n_edges", C.c_uint32), ("edges", C.c_uint32 * SIZE_EDGES_MAX)]


class SizeSpec:
    """Size bins of the per-call tallies: size = |a1_len - a0_len|; 1 to 15 ascending edges, the first at least 1; bin 0 is size < edges[0], the last bin
    size >= edges[-1].  The library checks the spec; an invalid one is refused there."""

    def __init__(self, edges=(1, 6, 16, 50)):
        self.edges = tuple(int(e) for e in edges)

    @property
    def n_bins(self):
        return len(self.edges) + 1

    def c_struct(self):
        s = AvkSizeSpec()
        s.n_edges = len(self.edges)
        for k, e in enumerate(self.edges[:SIZE_EDGES_MAX]):
            s.edges[k] = e & 0xFFFFFFFF
        return s

    def names(self):
        """avk_size_bin_name for every bin: len_<lo>_<hi> (inclusive), len_<lo> for one size, len_ge<lo> for the last"""
        from .api import load_library
        lib, cs, out = load_library(), self.c_struct(), []
        for j in range(self.n_bins):
            buf = C.create_string_buffer(64)
            if lib.avk_size_bin_name(C.byref(cs), j, buf, 64):
                raise ValueError(lib.avk_last_error(None).decode())
            out.append(buf.value.decode())
        return out


def declare_size(lib):
    """avk_size_n_bins, avk_size_bin_name, avk_size_block, avk_size_tallies, avk_compare_packed_size, avk_size_tallies_host (include/aardvark_amd.h)"""
    vp, u64p = C.c_void_p, _p(C.c_uint64)
    lib.avk_size_n_bins.restype = C.c_uint32
    lib.avk_size_n_bins.argtypes = [_p(AvkSizeSpec)]
    lib.avk_size_bin_name.restype = C.c_int
    lib.avk_size_bin_name.argtypes = [_p(AvkSizeSpec), C.c_uint32, C.c_char_p, C.c_size_t]
    lib.avk_size_block.restype = C.c_uint32
    lib.avk_size_block.argtypes = [vp]
    lib.avk_size_tallies.restype = C.c_int
    lib.avk_size_tallies.argtypes = [vp, vp, _p(AvkSizeSpec), vp, u64p]
    lib.avk_compare_packed_size.restype = C.c_int
    lib.avk_compare_packed_size.argtypes = [vp, _p(AvkPackedBatch), _p(AvkPackedEscapes), vp, _p(AvkCompareConfig), _p(AvkSizeSpec), _p(AvkResultBatch), u64p]
    lib.avk_size_tallies_host.restype = C.c_int
    lib.avk_size_tallies_host.argtypes = [_p(AvkRegionBatch), _p(AvkResultBatch), _p(AvkSizeSpec), _p(AvkRegionLabels), C.c_uint32, u64p]


SCORE_THRESHOLDS_MAX, SCORE_FIELDS = 31, 14
SCORE_DEFAULT = (5, 10, 15, 20, 25, 30, 35, 40, 50, 60)


class AvkScoreSpec(C.Structure):
    """avk_score_spec: the thresholds of the curve by query score (aardvark_amd/csrc/avk_score.h has the rule)"""
    _fields_ = [("n_thresholds", C.c_uint32), ("t", C.c_float * SCORE_THRESHOLDS_MAX)]


class ScoreSpec:
    """Thresholds of the precision-recall curve by query score: 1 to 31 finite, strictly ascending float32 values; point 0 is "no filter", point k is
    score >= thresholds[k - 1].  The library checks the spec; an invalid one is refused there."""

    def __init__(self, thresholds=SCORE_DEFAULT):
        self.thresholds = tuple(float(t) for t in thresholds)

    @property
    def n_points(self):
        return len(self.thresholds) + 1

    def c_struct(self):
        s = AvkScoreSpec()
        s.n_thresholds = len(self.thresholds)
        for k, t in enumerate(self.thresholds[:SCORE_THRESHOLDS_MAX]):
            s.t[k] = t
        return s

    def names(self):
        """avk_score_point_name for every point: score_all, then score_ge_<t> (%g)"""
        from .api import load_library
        lib, cs, out = load_library(), self.c_struct(), []
        for k in range(self.n_points):
            buf = C.create_string_buffer(64)
            if lib.avk_score_point_name(C.byref(cs), k, buf, 64):
                raise ValueError(lib.avk_last_error(None).decode())
            out.append(buf.value.decode())
        return out


def declare_score(lib):
    """avk_score_n_points, avk_score_point_name, avk_score_block, avk_score_tallies, avk_compare_packed_score, avk_score_tallies_host (include/aardvark_amd.h)"""
    vp, u64p, f32p = C.c_void_p, _p(C.c_uint64), _p(C.c_float)
    lib.avk_score_n_points.restype = C.c_uint32
    lib.avk_score_n_points.argtypes = [_p(AvkScoreSpec)]
    lib.avk_score_point_name.restype = C.c_int
    lib.avk_score_point_name.argtypes = [_p(AvkScoreSpec), C.c_uint32, C.c_char_p, C.c_size_t]
    lib.avk_score_block.restype = C.c_uint32
    lib.avk_score_block.argtypes = [vp]
    lib.avk_score_tallies.restype = C.c_int
    lib.avk_score_tallies.argtypes = [vp, vp, _p(AvkScoreSpec), f32p, vp, u64p]
    lib.avk_compare_packed_score.restype = C.c_int
    lib.avk_compare_packed_score.argtypes = [vp, _p(AvkPackedBatch), _p(AvkPackedEscapes), vp, _p(AvkCompareConfig), _p(AvkScoreSpec), f32p, _p(AvkResultBatch), u64p]
    lib.avk_score_tallies_host.restype = C.c_int
    lib.avk_score_tallies_host.argtypes = [_p(AvkRegionBatch), _p(AvkResultBatch), _p(AvkScoreSpec), f32p, _p(AvkRegionLabels), C.c_uint32, u64p]


N_KINDS, KIND_FIELDS = 9, 14
# avk_kind_name for every kind (aardvark_amd/csrc/avk_callkind.h has the rule): kind = 3 * gt + sub
KIND_NAMES = ["%s_%s" % (gt, sub) for gt in ("het", "hom", "nogt") for sub in ("ts", "tv", "other")]


def declare_kind(lib):
    """avk_kind_n, avk_kind_name, avk_kind_block, avk_kind_tallies, avk_compare_packed_kind, avk_kind_tallies_host (include/aardvark_amd.h)"""
    vp, u64p = C.c_void_p, _p(C.c_uint64)
    lib.avk_kind_n.restype = C.c_uint32
    lib.avk_kind_n.argtypes = []
    lib.avk_kind_name.restype = C.c_int
    lib.avk_kind_name.argtypes = [C.c_uint32, C.c_char_p, C.c_size_t]
    lib.avk_kind_block.restype = C.c_uint32
    lib.avk_kind_block.argtypes = [vp]
    lib.avk_kind_tallies.restype = C.c_int
    lib.avk_kind_tallies.argtypes = [vp, vp, vp, u64p]
    lib.avk_compare_packed_kind.restype = C.c_int
    lib.avk_compare_packed_kind.argtypes = [vp, _p(AvkPackedBatch), _p(AvkPackedEscapes), vp, _p(AvkCompareConfig), _p(AvkResultBatch), u64p]
    lib.avk_kind_tallies_host.restype = C.c_int
    lib.avk_kind_tallies_host.argtypes = [_p(AvkRegionBatch), _p(AvkResultBatch), _p(AvkRegionLabels), C.c_uint32, u64p]


CALLBOOT_MAX_BLOCKS = 262144  # AVK_CALLBOOT_MAX_BLOCKS of aardvark_amd/csrc/avk_callboot.h: (1 + labels) * replicates * keys


def declare_callboot(lib):
    """avk_callboot_block, avk_size_boot_tallies, avk_kind_boot_tallies and their host routes (include/aardvark_amd.h)"""
    vp, u64p = C.c_void_p, _p(C.c_uint64)
    lib.avk_callboot_block.restype = C.c_uint32
    lib.avk_callboot_block.argtypes = [vp, C.c_uint32]
    lib.avk_size_boot_tallies.restype = C.c_int
    lib.avk_size_boot_tallies.argtypes = [vp, vp, _p(AvkSizeSpec), _p(AvkBootSpec), vp, u64p]
    lib.avk_kind_boot_tallies.restype = C.c_int
    lib.avk_kind_boot_tallies.argtypes = [vp, vp, _p(AvkBootSpec), vp, u64p]
    lib.avk_size_boot_tallies_host.restype = C.c_int
    lib.avk_size_boot_tallies_host.argtypes = [_p(AvkRegionBatch), _p(AvkResultBatch), _p(AvkSizeSpec), _p(AvkBootSpec), _p(AvkRegionLabels), C.c_uint32, u64p]
    lib.avk_kind_boot_tallies_host.restype = C.c_int
    lib.avk_kind_boot_tallies_host.argtypes = [_p(AvkRegionBatch), _p(AvkResultBatch), _p(AvkBootSpec), _p(AvkRegionLabels), C.c_uint32, u64p]


CONTEXT_PAD_MAX, CONTEXT_GC_EDGES_MAX, CONTEXT_HP_EDGES_MAX = 1024, 17, 16


class AvkContextSpec(C.Structure):
    """avk_context_spec: the sequence-context labels of a stratified job (GC bins, homopolymer classes)"""
    _fields_ = [("gc_pad", C.c_uint32), ("n_gc_edges", C.c_uint32), ("gc_edges", C.c_uint32 * CONTEXT_GC_EDGES_MAX),
                ("hp_pad", C.c_uint32), ("n_hp_edges", C.c_uint32), ("hp_edges", C.c_uint32 * CONTEXT_HP_EDGES_MAX)]


def declare_context_strata(lib):
    """avk_strata_upload_context, avk_strata_n_context_labels, avk_context_label_name (include/aardvark_amd.h)"""
    vp, u32p = C.c_void_p, _p(C.c_uint32)
    lib.avk_strata_upload_context.restype = C.c_int
    lib.avk_strata_upload_context.argtypes = [vp, C.c_uint32, C.c_uint32, _p(C.c_uint64), u32p, u32p, _p(AvkContextSpec), _p(vp)]
    lib.avk_strata_n_context_labels.restype = C.c_uint32
    lib.avk_strata_n_context_labels.argtypes = [vp]
    lib.avk_context_label_name.restype = C.c_int
    lib.avk_context_label_name.argtypes = [_p(AvkContextSpec), C.c_uint32, C.c_char_p, C.c_size_t]


class ContextSpec:
    """The sequence-context labels of a stratified job: gc_edges percent values (n - 1 labels, window pad gc_pad), hp_edges run lengths (n labels, window pad
    hp_pad); an empty family does not exist.  The defaults are the tool's (--context-strata gc,hp)."""
    GC_EDGES = (0, 15, 20, 25, 30, 55, 60, 65, 70, 75, 80, 85, 101)
    HP_EDGES = (4, 7, 12, 21)

    def __init__(self, gc_edges=GC_EDGES, hp_edges=HP_EDGES, gc_pad=50, hp_pad=5):
        self.gc_edges, self.hp_edges = tuple(int(x) for x in gc_edges), tuple(int(x) for x in hp_edges)
        self.gc_pad, self.hp_pad = int(gc_pad), int(hp_pad)
        if len(self.gc_edges) > CONTEXT_GC_EDGES_MAX or len(self.hp_edges) > CONTEXT_HP_EDGES_MAX:
            raise ValueError("at most %d GC edges and %d run edges" % (CONTEXT_GC_EDGES_MAX, CONTEXT_HP_EDGES_MAX))
        if min(self.gc_edges + self.hp_edges + (self.gc_pad, self.hp_pad), default=0) < 0:
            raise ValueError("edges and pads are not negative")

    @property
    def n_labels(self):
        return max(len(self.gc_edges) - 1, 0) + len(self.hp_edges)

    def c_struct(self):
        s = AvkContextSpec()
        s.gc_pad, s.n_gc_edges, s.hp_pad, s.n_hp_edges = self.gc_pad, len(self.gc_edges), self.hp_pad, len(self.hp_edges)
        for i, x in enumerate(self.gc_edges):
            s.gc_edges[i] = x
        for i, x in enumerate(self.hp_edges):
            s.hp_edges[i] = x
        return s

    def names(self, lib=None):
        """avk_context_label_name for every label, in label order (host only: no device, no context)"""
        if lib is None:
            from .api import load_library
            lib = load_library()
        s, buf, out = self.c_struct(), C.create_string_buffer(64), []
        for j in range(self.n_labels):
            if lib.avk_context_label_name(C.byref(s), j, buf, len(buf)):
                raise ValueError((lib.avk_last_error(None) or b"invalid context spec").decode())
            out.append(buf.value.decode())
        return out


def declare_debug_ref_packed(lib):
    """avk_debug_ref_packed(avk_ctx *, uint32_t *words_out, uint64_t n_words_cap, uint32_t *flags_out, uint64_t n_flag_words_cap) -> int"""
    lib.avk_debug_ref_packed.restype = C.c_int
    lib.avk_debug_ref_packed.argtypes = [C.c_void_p, _p(C.c_uint32), C.c_uint64, _p(C.c_uint32), C.c_uint64]


def ref_packed_sizes(n_bases):
    """(packed words, flag words) avk_debug_ref_packed returns for a reference of n_bases bases in all"""
    n_words = (int(n_bases) + 15) // 16
    return n_words, n_words // 32 + 8


def _ptr(arr, ctype):
    return arr.ctypes.data_as(_p(ctype))


def seq_stride(start, end, a0_len, a1_len):
    """Upper bound of any haplotype length of a region (mirrors avk_seq_stride())."""
    grow = int(np.maximum(a1_len.astype(np.int64) - a0_len.astype(np.int64), 0).sum()) if len(a0_len) else 0
    return int(end - start) + grow


class RegionBatch:
    """Flat structure-of-arrays batch of CompareRegions (reference
    src/data_types/compare_region.rs:13-26).  Build with `from_regions` (a list of dicts) or
    directly from numpy arrays via the constructor."""

    def __init__(self, region_id, contig_idx, start, end, t_off, t_cnt, q_off, q_cnt,
                 var_pos, var_type, var_zyg, var_raw_space, a0_off, a0_len, a1_off, a1_len, allele_bytes):
        g = lambda a, dt: np.ascontiguousarray(a, dtype=dt)
        self.region_id = g(region_id, np.uint64)
        self.contig_idx = g(contig_idx, np.uint32)
        self.start = g(start, np.uint64)
        self.end = g(end, np.uint64)
        self.t_off = g(t_off, np.uint64)
        self.t_cnt = g(t_cnt, np.uint32)
        self.q_off = g(q_off, np.uint64)
        self.q_cnt = g(q_cnt, np.uint32)
        self.var_pos = g(var_pos, np.uint64)
        self.var_type = g(var_type, np.uint8)
        self.var_zyg = g(var_zyg, np.uint8)
        self.var_raw_space = g(var_raw_space, np.uint32)
        self.a0_off = g(a0_off, np.uint64)
        self.a0_len = g(a0_len, np.uint32)
        self.a1_off = g(a1_off, np.uint64)
        self.a1_len = g(a1_len, np.uint32)
        self.allele_bytes = g(allele_bytes, np.uint8)
        if self.allele_bytes.size == 0:
            self.allele_bytes = np.zeros(1, np.uint8)
        self.n_regions = int(self.start.size)
        self.n_variants = int(self.var_pos.size)

    @classmethod
    def from_regions(cls, regions):
        """regions: list of dicts {start, end, truth, query[, contig, region_id]}; a variant is
        (pos, allele0, allele1, type, zygosity[, raw_allele_space]) with type/zygosity by name
        or ordinal and alleles as str/bytes."""
        rid, cidx, st, en, t_off, t_cnt, q_off, q_cnt = [], [], [], [], [], [], [], []
        vpos, vtype, vzyg, vraw, a0o, a0l, a1o, a1l = [], [], [], [], [], [], [], []
        blob = bytearray()

        def add(v):
            pos, a0, a1, ty = v[0], v[1], v[2], v[3]
            zy = v[4] if len(v) > 4 else "Unknown"
            a0 = a0.encode() if isinstance(a0, str) else bytes(a0)
            a1 = a1.encode() if isinstance(a1, str) else bytes(a1)
            vpos.append(pos)
            vtype.append(VT[ty] if isinstance(ty, str) else int(ty))
            vzyg.append(ZYG[zy] if isinstance(zy, str) else int(zy))
            vraw.append(v[5] if len(v) > 5 else max(len(a0), len(a1)))
            a0o.append(len(blob)); a0l.append(len(a0)); blob.extend(a0)
            a1o.append(len(blob)); a1l.append(len(a1)); blob.extend(a1)

        for i, r in enumerate(regions):
            rid.append(r.get("region_id", i))
            cidx.append(r.get("contig", 0))
            st.append(r["start"]); en.append(r["end"])
            t_off.append(len(vpos)); t_cnt.append(len(r["truth"]))
            for v in r["truth"]:
                add(v)
            q_off.append(len(vpos)); q_cnt.append(len(r["query"]))
            for v in r["query"]:
                add(v)
        return cls(rid, cidx, st, en, t_off, t_cnt, q_off, q_cnt, vpos, vtype, vzyg, vraw,
                   a0o, a0l, a1o, a1l, np.frombuffer(bytes(blob), dtype=np.uint8))

    def c_struct(self):
        b = AvkRegionBatch()
        b.n_regions = self.n_regions
        b.region_id = _ptr(self.region_id, C.c_uint64)
        b.contig_idx = _ptr(self.contig_idx, C.c_uint32)
        b.start = _ptr(self.start, C.c_uint64)
        b.end = _ptr(self.end, C.c_uint64)
        b.t_off = _ptr(self.t_off, C.c_uint64)
        b.t_cnt = _ptr(self.t_cnt, C.c_uint32)
        b.q_off = _ptr(self.q_off, C.c_uint64)
        b.q_cnt = _ptr(self.q_cnt, C.c_uint32)
        b.n_variants = self.n_variants
        b.var_pos = _ptr(self.var_pos, C.c_uint64)
        b.var_type = _ptr(self.var_type, C.c_uint8)
        b.var_zyg = _ptr(self.var_zyg, C.c_uint8)
        b.var_raw_space = _ptr(self.var_raw_space, C.c_uint32)
        b.a0_off = _ptr(self.a0_off, C.c_uint64)
        b.a0_len = _ptr(self.a0_len, C.c_uint32)
        b.a1_off = _ptr(self.a1_off, C.c_uint64)
        b.a1_len = _ptr(self.a1_len, C.c_uint32)
        b.allele_bytes = _ptr(self.allele_bytes, C.c_uint8)
        b.allele_bytes_len = int(self.allele_bytes.size)
        return b

    def seq_strides(self):
        out = np.zeros(self.n_regions, np.uint32)
        for r in range(self.n_regions):
            lo = int(self.t_off[r]); hi = lo + int(self.t_cnt[r])
            g = seq_stride(int(self.start[r]), int(self.end[r]), self.a0_len[lo:hi], self.a1_len[lo:hi])
            lo = int(self.q_off[r]); hi = lo + int(self.q_cnt[r])
            g2 = seq_stride(int(self.start[r]), int(self.end[r]), self.a0_len[lo:hi], self.a1_len[lo:hi])
            out[r] = max(g, g2, 1)
        return out

    def slice(self, lo, hi):
        """Regions [lo, hi) as a new batch sharing the variant arrays."""
        s = np.s_[lo:hi]
        return RegionBatch(self.region_id[s], self.contig_idx[s], self.start[s], self.end[s],
                           self.t_off[s], self.t_cnt[s], self.q_off[s], self.q_cnt[s],
                           self.var_pos, self.var_type, self.var_zyg, self.var_raw_space,
                           self.a0_off, self.a0_len, self.a1_off, self.a1_len, self.allele_bytes)


class CompactBatch:
    """The same batch in the library's compact form (avk_compact_batch): 20 bytes per region, 17 per call.  `from_region_batch` checks the constraints the
    narrow fields rest on (query calls of a region right behind its truth calls, allele1 right behind allele0, 32-bit positions and offsets)."""

    FIELDS = ("contig_idx", "start", "len", "v_off", "t_cnt", "q_cnt", "var_pos", "var_type_zyg", "a_off", "a0_len", "a1_len", "var_raw_space", "allele_bytes")
    DTYPES = (np.uint32, np.uint32, np.uint32, np.uint32, np.uint16, np.uint16, np.uint32, np.uint8, np.uint32, np.uint32, np.uint32, np.uint32, np.uint8)

    def __init__(self, **arrays):
        for name, dt in zip(self.FIELDS, self.DTYPES):
            a = arrays.get(name)
            setattr(self, name, None if a is None else np.ascontiguousarray(a, dtype=dt))
        self.n_regions = int(self.start.size)
        self.n_variants = int(self.var_pos.size)

    @classmethod
    def from_region_batch(cls, b, keep_raw_space=None):
        ok = (np.array_equal(b.q_off, b.t_off + b.t_cnt) and np.array_equal(b.a1_off, b.a0_off + b.a0_len) and
              (b.n_regions == 0 or (int(b.end.max()) < 2 ** 32 and int(b.t_cnt.max()) < 65536 and int(b.q_cnt.max()) < 65536)) and
              b.n_variants < 2 ** 32 and b.allele_bytes.size < 2 ** 32 and (b.n_variants == 0 or int(b.var_pos.max()) < 2 ** 32) and bool(np.all(b.end >= b.start)) and
              (b.n_variants == 0 or (int(b.var_type.max()) < 16 and int(b.var_zyg.max()) < 16)))
        if not ok:
            raise ValueError("the batch does not satisfy the constraints of the compact form (include/aardvark_amd.h: avk_compact_batch)")
        default_raw = np.array_equal(b.var_raw_space, np.maximum(b.a0_len, b.a1_len))
        if keep_raw_space is None:
            keep_raw_space = not default_raw
        return cls(contig_idx=b.contig_idx, start=b.start, len=b.end - b.start, v_off=b.t_off, t_cnt=b.t_cnt, q_cnt=b.q_cnt, var_pos=b.var_pos,
                   var_type_zyg=b.var_type | (b.var_zyg << 4), a_off=b.a0_off, a0_len=b.a0_len, a1_len=b.a1_len, var_raw_space=b.var_raw_space if keep_raw_space else None,
                   allele_bytes=b.allele_bytes)

    def widen(self):
        """back to the wide form (what the library's dp_widen kernel writes on the device)"""
        raw = self.var_raw_space if self.var_raw_space is not None else np.maximum(self.a0_len, self.a1_len)
        toff = self.v_off.astype(np.uint64)
        return RegionBatch(np.arange(self.n_regions), self.contig_idx, self.start, self.start.astype(np.uint64) + self.len, toff, self.t_cnt, toff + self.t_cnt, self.q_cnt, self.var_pos,
                           self.var_type_zyg & 15, self.var_type_zyg >> 4, raw, self.a_off, self.a0_len, self.a_off.astype(np.uint64) + self.a0_len, self.a1_len, self.allele_bytes)

    def nbytes(self):
        return sum(getattr(self, f).nbytes for f in self.FIELDS if getattr(self, f) is not None)

    def c_struct(self):
        b = AvkCompactBatch()
        b.n_regions, b.n_variants = self.n_regions, self.n_variants
        for name, ct in (("contig_idx", C.c_uint32), ("start", C.c_uint32), ("len", C.c_uint32), ("v_off", C.c_uint32), ("t_cnt", C.c_uint16), ("q_cnt", C.c_uint16), ("var_pos", C.c_uint32),
                         ("var_type_zyg", C.c_uint8), ("a_off", C.c_uint32), ("a0_len", C.c_uint32), ("a1_len", C.c_uint32), ("var_raw_space", C.c_uint32), ("allele_bytes", C.c_uint8)):
            a = getattr(self, name)
            if a is not None:
                setattr(b, name, _ptr(a, ct))
        b.allele_bytes_len = int(self.allele_bytes.size)
        return b


class PackedEscapes:
    """The escapes of a packed batch (avk_packed_escapes): three sorted lists of overrides for the regions, count slots and calls whose values do not fit the
    narrow fields.  The listed indices carry the bases first_region / first_slot / first_call, so a slice of a batch is a slice of the lists plus new bases."""

    FIELDS = ("esc_region", "esc_len", "esc_slot", "esc_cnt", "esc_call", "esc_rel_pos", "esc_a0_len", "esc_a1_len")
    DTYPES = (np.uint64, np.uint32, np.uint64, np.uint32, np.uint64, np.uint32, np.uint32, np.uint32)

    def __init__(self, first_region=0, first_call=0, first_slot=0, **arrays):
        self.first_region, self.first_call, self.first_slot = int(first_region), int(first_call), int(first_slot)
        for name, dt in zip(self.FIELDS, self.DTYPES):
            a = arrays.get(name)
            setattr(self, name, np.zeros(0, dt) if a is None else np.ascontiguousarray(a, dtype=dt))
        assert self.esc_region.size == self.esc_len.size and self.esc_slot.size == self.esc_cnt.size
        assert self.esc_call.size == self.esc_rel_pos.size == self.esc_a0_len.size == self.esc_a1_len.size

    @classmethod
    def build(cls, length, counts, rel, a0_len, a1_len):
        """the lists for wide per-region lengths, per-slot counts and per-call (relative position, allele lengths): whatever does not fit 16 / 8 / 16, 8, 8 bits"""
        er = np.flatnonzero(length >= 65536)
        es = np.flatnonzero(counts >= 256)
        ec = np.flatnonzero((rel >= 65536) | (a0_len >= 256) | (a1_len >= 256))
        return cls(esc_region=er, esc_len=length[er], esc_slot=es, esc_cnt=counts[es], esc_call=ec, esc_rel_pos=rel[ec], esc_a0_len=a0_len[ec], esc_a1_len=a1_len[ec])

    def empty(self):
        return self.esc_region.size == 0 and self.esc_slot.size == 0 and self.esc_call.size == 0

    def nbytes(self):
        return sum(getattr(self, f).nbytes for f in self.FIELDS)

    def apply(self, length, counts, rel, a0_len, a1_len):
        """the lists written over wide (int64) copies of the narrow arrays, in place"""
        length[(self.esc_region - np.uint64(self.first_region)).astype(np.int64)] = self.esc_len
        counts[(self.esc_slot - np.uint64(self.first_slot)).astype(np.int64)] = self.esc_cnt
        v = (self.esc_call - np.uint64(self.first_call)).astype(np.int64)
        rel[v], a0_len[v], a1_len[v] = self.esc_rel_pos, self.esc_a0_len, self.esc_a1_len

    def slice(self, r0, r1, s0, s1, v0, v1):
        """the escapes of regions [r0, r1), count slots [s0, s1) and calls [v0, v1) of the batch these belong to: ranges of the same arrays, new bases"""
        cut = lambda idx, first, lo, hi: (int(np.searchsorted(idx, np.uint64(first + lo))), int(np.searchsorted(idx, np.uint64(first + hi))))
        a, b = cut(self.esc_region, self.first_region, r0, r1)
        c, d = cut(self.esc_slot, self.first_slot, s0, s1)
        e, f = cut(self.esc_call, self.first_call, v0, v1)
        return PackedEscapes(self.first_region + r0, self.first_call + v0, self.first_slot + s0, esc_region=self.esc_region[a:b], esc_len=self.esc_len[a:b],
                             esc_slot=self.esc_slot[c:d], esc_cnt=self.esc_cnt[c:d], esc_call=self.esc_call[e:f], esc_rel_pos=self.esc_rel_pos[e:f],
                             esc_a0_len=self.esc_a0_len[e:f], esc_a1_len=self.esc_a1_len[e:f])

    def pinned(self, host_array):
        """a copy whose lists live in memory handed out by `host_array(shape, dtype)` (Context.host_array)"""
        out = PackedEscapes(self.first_region, self.first_call, self.first_slot)
        for f in self.FIELDS:
            a = getattr(self, f)
            b = host_array((max(a.size, 1),), a.dtype)[:a.size]
            b[...] = a
            setattr(out, f, b)
        return out

    def c_struct(self):
        e = AvkPackedEscapes()
        e.first_region, e.first_call, e.first_slot = self.first_region, self.first_call, self.first_slot
        e.n_esc_regions, e.n_esc_slots, e.n_esc_calls = int(self.esc_region.size), int(self.esc_slot.size), int(self.esc_call.size)
        for name, ct in (("esc_region", C.c_uint64), ("esc_len", C.c_uint32), ("esc_slot", C.c_uint64), ("esc_cnt", C.c_uint32), ("esc_call", C.c_uint64),
                         ("esc_rel_pos", C.c_uint32), ("esc_a0_len", C.c_uint32), ("esc_a1_len", C.c_uint32)):
            a = getattr(self, name)
            if a.size:
                setattr(e, name, _ptr(a, ct))
        return e

    @classmethod
    def from_c(cls, e):
        """a copy of the lists of an avk_packed_escapes (a shard's)"""
        take = lambda ptr, m, dt: np.ctypeslib.as_array(ptr, shape=(max(m, 1),))[:m].astype(dt).copy() if ptr and m else np.zeros(0, dt)
        nr, ns, nc = int(e.n_esc_regions), int(e.n_esc_slots), int(e.n_esc_calls)
        return cls(int(e.first_region), int(e.first_call), int(e.first_slot), esc_region=take(e.esc_region, nr, np.uint64), esc_len=take(e.esc_len, nr, np.uint32),
                   esc_slot=take(e.esc_slot, ns, np.uint64), esc_cnt=take(e.esc_cnt, ns, np.uint32), esc_call=take(e.esc_call, nc, np.uint64),
                   esc_rel_pos=take(e.esc_rel_pos, nc, np.uint32), esc_a0_len=take(e.esc_a0_len, nc, np.uint32), esc_a1_len=take(e.esc_a1_len, nc, np.uint32))


class PackedBatch:
    """The same batch in the library's packed form (avk_packed_batch): 10 bytes per region, 5 per call plus the allele bytes; every offset is implied by
    order.  `from_compact` checks the constraints (calls and alleles back to back in region / call order, narrow fields wide enough)."""

    FIELDS = ("contig_idx", "start", "len", "t_cnt", "q_cnt", "var_rel_pos", "var_type_zyg", "a0_len", "a1_len", "var_raw_space", "allele_bytes")
    DTYPES = (np.uint16, np.uint32, np.uint16, np.uint8, np.uint8, np.uint16, np.uint8, np.uint8, np.uint8, np.uint32, np.uint8)

    def __init__(self, escapes=None, **arrays):
        for name, dt in zip(self.FIELDS, self.DTYPES):
            a = arrays.get(name)
            setattr(self, name, None if a is None else np.ascontiguousarray(a, dtype=dt))
        self.n_regions = int(self.start.size)
        self.n_variants = int(self.var_rel_pos.size)
        self.escapes = escapes  # a PackedEscapes (possibly empty), or None: the batch as it was before escapes existed

    @classmethod
    def from_compact(cls, cb, escapes=False):
        """escapes=True: values that do not fit the narrow fields go to the batch's PackedEscapes instead of raising (what is left to raise for: calls or
        alleles that are not back to back, a call in front of its region's start, more than 65,535 contigs)"""
        if escapes:
            return cls._from_compact_escaped(cb)
        n, nv = cb.n_regions, cb.n_variants
        cnt = cb.t_cnt.astype(np.int64) + cb.q_cnt
        voff = np.concatenate([[0], np.cumsum(cnt)])
        alen = cb.a0_len.astype(np.int64) + cb.a1_len
        aoff = np.concatenate([[0], np.cumsum(alen)])
        ok = (np.array_equal(cb.v_off, voff[:-1]) and int(voff[-1]) == nv and np.array_equal(cb.a_off, aoff[:-1]) and (nv == 0 or int(aoff[-1]) == cb.allele_bytes.size) and
              (n == 0 or (int(cb.len.max()) < 65536 and int(cb.t_cnt.max()) < 256 and int(cb.q_cnt.max()) < 256)) and
              (nv == 0 or (int(cb.a0_len.max()) < 256 and int(cb.a1_len.max()) < 256)) and (cb.contig_idx is None or n == 0 or int(cb.contig_idx.max()) < 65536))
        rel = None
        if ok:
            region_of = np.repeat(np.arange(n), cnt)
            rel = cb.var_pos.astype(np.int64) - cb.start.astype(np.int64)[region_of]
            ok = nv == 0 or (int(rel.min()) >= 0 and int(rel.max()) < 65536)
        if not ok:
            raise ValueError("the batch does not satisfy the constraints of the packed form (include/aardvark_amd.h: avk_packed_batch)")
        return cls(contig_idx=cb.contig_idx, start=cb.start, len=cb.len, t_cnt=cb.t_cnt, q_cnt=cb.q_cnt, var_rel_pos=rel, var_type_zyg=cb.var_type_zyg, a0_len=cb.a0_len,
                   a1_len=cb.a1_len, var_raw_space=cb.var_raw_space, allele_bytes=cb.allele_bytes)

    @classmethod
    def _from_compact_escaped(cls, cb):
        n, nv = cb.n_regions, cb.n_variants
        cnt = cb.t_cnt.astype(np.int64) + cb.q_cnt
        voff = np.concatenate([[0], np.cumsum(cnt)])
        a0, a1 = cb.a0_len.astype(np.int64), cb.a1_len.astype(np.int64)
        aoff = np.concatenate([[0], np.cumsum(a0 + a1)])
        ok = (np.array_equal(cb.v_off, voff[:-1]) and int(voff[-1]) == nv and np.array_equal(cb.a_off, aoff[:-1]) and (nv == 0 or int(aoff[-1]) == cb.allele_bytes.size) and
              (cb.contig_idx is None or n == 0 or int(cb.contig_idx.max()) < 65536))
        rel = None
        if ok:
            rel = cb.var_pos.astype(np.int64) - cb.start.astype(np.int64)[np.repeat(np.arange(n), cnt)]
            ok = nv == 0 or int(rel.min()) >= 0
        if not ok:
            raise ValueError("the batch does not satisfy the constraints of the packed form with escapes (include/aardvark_amd.h: avk_packed_escapes)")
        length = cb.len.astype(np.int64)
        slots = np.stack([cb.t_cnt.astype(np.int64), cb.q_cnt.astype(np.int64)], axis=1).reshape(-1) if n else np.zeros(0, np.int64)
        esc = PackedEscapes.build(length, slots, rel, a0, a1)
        # a listed entry's narrow fields are written as 0
        length[esc.esc_region.astype(np.int64)] = 0
        slots[esc.esc_slot.astype(np.int64)] = 0
        v = esc.esc_call.astype(np.int64)
        rel[v], a0[v], a1[v] = 0, 0, 0
        return cls(escapes=esc, contig_idx=cb.contig_idx, start=cb.start, len=length, t_cnt=slots[0::2], q_cnt=slots[1::2], var_rel_pos=rel, var_type_zyg=cb.var_type_zyg,
                   a0_len=a0, a1_len=a1, var_raw_space=cb.var_raw_space, allele_bytes=cb.allele_bytes)

    def _wide_fields(self):
        """(len, count slots, relative positions, a0_len, a1_len) as int64 with the escapes applied"""
        length, rel, a0, a1 = self.len.astype(np.int64), self.var_rel_pos.astype(np.int64), self.a0_len.astype(np.int64), self.a1_len.astype(np.int64)
        slots = np.stack([self.t_cnt.astype(np.int64), self.q_cnt.astype(np.int64)], axis=1).reshape(-1) if self.n_regions else np.zeros(0, np.int64)
        if self.escapes is not None:
            self.escapes.apply(length, slots, rel, a0, a1)
        return length, slots, rel, a0, a1

    def to_compact(self):
        """undoes the packing: the CompactBatch this batch (with its escapes) stands for"""
        length, slots, rel, a0, a1 = self._wide_fields()
        tc, qc = slots[0::2], slots[1::2]
        cnt = tc + qc
        voff = np.concatenate([[0], np.cumsum(cnt)])[:-1]
        aoff = np.concatenate([[0], np.cumsum(a0 + a1)])[:-1]
        pos = self.start.astype(np.int64)[np.repeat(np.arange(self.n_regions), cnt)] + rel
        return CompactBatch(contig_idx=self.contig_idx, start=self.start, len=length, v_off=voff, t_cnt=tc, q_cnt=qc, var_pos=pos, var_type_zyg=self.var_type_zyg, a_off=aoff,
                            a0_len=a0, a1_len=a1, var_raw_space=self.var_raw_space, allele_bytes=self.allele_bytes)

    def nbytes(self):
        return sum(getattr(self, f).nbytes for f in self.FIELDS if getattr(self, f) is not None) + (self.escapes.nbytes() if self.escapes is not None else 0)

    def c_escapes(self):
        """the avk_packed_escapes to hand in with c_struct(), or None when the batch lists nothing (the entry points without escapes then serve)"""
        return None if self.escapes is None or self.escapes.empty() else self.escapes.c_struct()

    def split(self, n_parts):
        """the batch as `n_parts` batches of consecutive regions (cut at contig boundaries where there are enough contigs): a job handed over piece by piece"""
        n = self.n_regions
        cuts = [n * i // n_parts for i in range(n_parts + 1)]
        if self.contig_idx is not None and n:
            starts = np.flatnonzero(np.diff(self.contig_idx.astype(np.int64)) != 0) + 1
            if starts.size + 1 >= n_parts:
                for i in range(1, n_parts):
                    cuts[i] = int(starts[np.argmin(np.abs(starts - cuts[i]))])
        cuts = sorted(set(cuts))
        if self.escapes is not None:
            _, slots, _, a0, a1 = self._wide_fields()
            voff = np.concatenate([[0], np.cumsum(slots[0::2] + slots[1::2])])
            aoff = np.concatenate([[0], np.cumsum(a0 + a1)])
        else:
            voff = np.concatenate([[0], np.cumsum(self.t_cnt.astype(np.int64) + self.q_cnt)])
            aoff = np.concatenate([[0], np.cumsum(self.a0_len.astype(np.int64) + self.a1_len)])
        parts = []
        for r0, r1 in zip(cuts[:-1], cuts[1:]):
            v0, v1 = int(voff[r0]), int(voff[r1])
            a0, a1 = int(aoff[v0]), int(aoff[v1])
            cut = {"contig_idx": (r0, r1), "start": (r0, r1), "len": (r0, r1), "t_cnt": (r0, r1), "q_cnt": (r0, r1), "var_rel_pos": (v0, v1), "var_type_zyg": (v0, v1),
                   "a0_len": (v0, v1), "a1_len": (v0, v1), "var_raw_space": (v0, v1), "allele_bytes": (a0, a1)}
            esc = None if self.escapes is None else self.escapes.slice(r0, r1, 2 * r0, 2 * r1, v0, v1)
            parts.append(PackedBatch(escapes=esc, **{f: (None if getattr(self, f) is None else getattr(self, f)[cut[f][0]:cut[f][1]]) for f in self.FIELDS}))
        return parts

    def c_struct(self):
        b = AvkPackedBatch()
        b.n_regions, b.n_variants = self.n_regions, self.n_variants
        for name, ct in (("contig_idx", C.c_uint16), ("start", C.c_uint32), ("len", C.c_uint16), ("t_cnt", C.c_uint8), ("q_cnt", C.c_uint8), ("var_rel_pos", C.c_uint16),
                         ("var_type_zyg", C.c_uint8), ("a0_len", C.c_uint8), ("a1_len", C.c_uint8), ("var_raw_space", C.c_uint32), ("allele_bytes", C.c_uint8)):
            a = getattr(self, name)
            if a is not None:
                setattr(b, name, _ptr(a, ct))
        b.allele_bytes_len = int(self.allele_bytes.size)
        return b


class ResultBatch:
    """Caller-allocated outputs of one avk_compare_batch / orc_compare_batch call."""

    WIDE_REGION = (("status", np.int32), ("ed_h1", np.uint32), ("ed_h2", np.uint32), ("n_optima", np.uint32), ("type_present", np.uint16))
    WIDE_CALL = ("var_expected", "var_observed", "var_class", "var_zyg")

    def __init__(self, batch, sequences=False, group_metrics=True, bp_groups=False, packed=False):
        """packed: False = the wide arrays; True = the wide arrays and the packed form (avk_result_batch::region_packed / var_packed); "only" = the packed form
        alone — 8 bytes per region and 1 per call cross PCIe, the wide arrays are None until expand()"""
        n, v = batch.n_regions, batch.n_variants
        self.n_regions, self.n_variants = n, v
        # compact per-region BASEPAIR groups (avk_result_batch::bp_off / bp_groups); bp_groups="packed": one word per region, the groups of the regions that need
        # more than a word spilled into bp_groups (avk_result_batch::bp_packed / bp_spilled)
        self.bp_off = np.zeros(n + 1, np.uint32) if bp_groups and bp_groups != "packed" else None
        self.bp_groups = np.zeros((n + v + 1, 4), np.uint32) if bp_groups else None
        self.bp_packed = np.zeros(max(n, 1), np.uint32) if bp_groups == "packed" else None
        self.bp_spilled = np.zeros(1, np.uint32) if bp_groups == "packed" else None
        wide = packed != "only"
        self.status = np.full(n, -1, np.int32) if wide else None
        self.ed_h1 = np.zeros(n, np.uint32) if wide else None
        self.ed_h2 = np.zeros(n, np.uint32) if wide else None
        self.n_optima = np.zeros(n, np.uint32) if wide else None
        self.type_present = np.zeros(n, np.uint16) if wide else None
        self.group_metrics = np.zeros((n, N_GROUPS, N_FIELDS), np.uint32) if group_metrics else None
        for f in self.WIDE_CALL:
            setattr(self, f, np.zeros(max(v, 1), np.uint8) if wide else None)
        self.region_packed = np.full(max(n, 1), 0x7F, np.uint64) if packed else None
        self.var_packed = np.zeros(max(v, 1), np.uint8) if packed else None
        self.tally = np.zeros(TALLY_LEN, np.uint64)
        self.sequences = sequences
        if sequences:
            self.seq_stride = batch.seq_strides()
            self.seq_off = np.zeros(n, np.uint64)
            if n:
                self.seq_off[1:] = np.cumsum(self.seq_stride[:-1].astype(np.uint64) * 5)
            total = int((self.seq_stride.astype(np.uint64) * 5).sum())
            self.seq_bytes = np.zeros(max(total, 1), np.uint8)
            self.seq_len = np.zeros((n, 5), np.uint32)

    def c_struct(self):
        o = AvkResultBatch()
        if self.status is not None:
            o.status = _ptr(self.status, C.c_int32)
            o.ed_h1 = _ptr(self.ed_h1, C.c_uint32)
            o.ed_h2 = _ptr(self.ed_h2, C.c_uint32)
            o.n_optima = _ptr(self.n_optima, C.c_uint32)
            o.type_present = _ptr(self.type_present, C.c_uint16)
        if self.group_metrics is not None:
            o.group_metrics = _ptr(self.group_metrics, C.c_uint32)
        if self.var_expected is not None:
            o.var_expected = _ptr(self.var_expected, C.c_uint8)
            o.var_observed = _ptr(self.var_observed, C.c_uint8)
            o.var_class = _ptr(self.var_class, C.c_uint8)
            o.var_zyg = _ptr(self.var_zyg, C.c_uint8)
        if self.region_packed is not None:
            o.region_packed = _ptr(self.region_packed, C.c_uint64)
            o.var_packed = _ptr(self.var_packed, C.c_uint8)
        o.tally = _ptr(self.tally, C.c_uint64)
        if self.bp_off is not None:
            o.bp_off = _ptr(self.bp_off, C.c_uint32)
            o.bp_groups = _ptr(self.bp_groups, C.c_uint32)
        if getattr(self, "bp_packed", None) is not None:
            o.bp_packed = _ptr(self.bp_packed, C.c_uint32)
            o.bp_spilled = _ptr(self.bp_spilled, C.c_uint32)
            o.bp_groups = _ptr(self.bp_groups, C.c_uint32)
        if self.sequences:
            o.seq_bytes = _ptr(self.seq_bytes, C.c_uint8)
            o.seq_off = _ptr(self.seq_off, C.c_uint64)
            o.seq_stride = _ptr(self.seq_stride, C.c_uint32)
            o.seq_len = _ptr(self.seq_len, C.c_uint32)
        return o

    def expanded(self, lib, batch):
        """avk_results_expand: a ResultBatch with the wide arrays rebuilt from this one's packed form (host work, no GPU involved); group_metrics,
        bp_groups, tally and sequences are shared with this one"""
        import copy
        out = copy.copy(self)
        n, v = self.n_regions, self.n_variants
        for f, dt in self.WIDE_REGION:
            setattr(out, f, np.full(n, -1, dt) if f == "status" else np.zeros(n, dt))
        for f in self.WIDE_CALL:
            setattr(out, f, np.zeros(max(v, 1), np.uint8))
        cb, src, dst = batch.c_struct(), self.c_struct(), out.c_struct()
        lib.avk_results_expand.argtypes = [C.POINTER(AvkRegionBatch), C.POINTER(AvkResultBatch), C.POINTER(AvkResultBatch)]
        rc = lib.avk_results_expand(C.byref(cb), C.byref(src), C.byref(dst))
        if rc != 0:
            raise ValueError("avk_results_expand: %d" % rc)
        return out

    def sequence(self, r, k):
        off = int(self.seq_off[r]) + k * int(self.seq_stride[r])
        return bytes(self.seq_bytes[off:off + int(self.seq_len[r, k])])

    FIELDS_CMP = ["status", "ed_h1", "ed_h2", "n_optima", "type_present", "group_metrics",
                  "var_expected", "var_observed", "var_class", "var_zyg", "tally"]

    def diff(self, other):
        """Names of the output arrays that differ from `other` (bit-exact comparison)."""
        bad = []
        for f in self.FIELDS_CMP:
            a, b = getattr(self, f), getattr(other, f)
            if a is None or b is None:
                continue
            if not np.array_equal(a, b):
                bad.append(f)
        if self.sequences and other.sequences:
            if not np.array_equal(self.seq_len, other.seq_len):
                bad.append("seq_len")
            else:
                for r in range(self.seq_len.shape[0]):
                    for k in range(5):
                        if self.sequence(r, k) != other.sequence(r, k):
                            bad.append("seq_bytes[%d,%d]" % (r, k))
                            break
        return bad
