"""ctypes bindings of libaardvark_amd.so and the host-side mirror of the reference interface.

`Context.solve_compare_regions(batch, config)` is the batched form of the reference's
`solve_compare_region(problem, reference_genome, compare_config, stratifications)`
(src/waffle_solver.rs:122-124): same inputs (CompareRegion fields, CompareConfig fields), same
outputs (CompareBenchmark fields), same per-region error behaviour (a failed region yields a
status instead of metrics and the batch continues, src/main.rs:255-265).
"""
import ctypes as C
import os
import weakref

import numpy as np

from ._abi import (TALLY_LEN, AvkCompactBatch, AvkCompareConfig, AvkPackedBatch, AvkPackedEscapes, AvkRegionBatch, AvkRegionLabels, AvkResultBatch, CompactBatch,
                   PackedBatch, RegionBatch, ResultBatch, BootSpec, ContextSpec, SizeSpec, SIZE_FIELDS, ScoreSpec, SCORE_FIELDS, N_KINDS, KIND_FIELDS, N_GROUPS, declare_boot, declare_size, declare_score, declare_kind, declare_callboot, declare_context_strata, declare_debug_ref_packed, declare_submit_strata, ref_packed_sizes,
                   region_labels)

_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None
u8p = C.POINTER(C.c_uint8)
u64p = C.POINTER(C.c_uint64)


class AardvarkAmdError(RuntimeError):
    pass


def library_path():
    """in-tree libaardvark_amd.so; AVK_LIB selects another in-tree build (kernel tuning experiments)"""
    return os.path.join(_HERE, os.environ.get("AVK_LIB", "libaardvark_amd.so"))


def load_library():
    """Loads libaardvark_amd.so (built in-tree by __graft_entry__.build() / csrc/Makefile).
    Fails loudly when it is missing: there is no fallback implementation."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise AardvarkAmdError("%s not found: build it with `make -C aardvark_amd/csrc` (hipcc, gfx950)" % path)
    lib = C.CDLL(path)
    vp = C.c_void_p
    lib.avk_version.restype = C.c_char_p
    lib.avk_source_hash.restype = C.c_char_p
    lib.avk_merge_classify.argtypes = [C.c_uint64, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_uint8),
                                       vp, C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)]
    lib.avk_edit_distance.restype = C.c_uint64
    lib.avk_edit_distance.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64]
    lib.avk_last_error.restype = C.c_char_p
    lib.avk_last_error.argtypes = [vp]
    lib.avk_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
    lib.avk_ctx_destroy.argtypes = [vp]
    lib.avk_ctx_destroy.restype = None
    lib.avk_ctx_set_stream.argtypes = [vp, vp]
    lib.avk_ctx_set_option.argtypes = [vp, C.c_char_p, C.c_int64]
    lib.avk_ref_upload.argtypes = [vp, C.c_uint32, C.POINTER(u8p), u64p]
    lib.avk_compare_batch.argtypes = [vp, C.POINTER(AvkRegionBatch), C.POINTER(AvkCompareConfig), C.POINTER(AvkResultBatch)]
    lib.avk_batch_upload.argtypes = [vp, C.POINTER(AvkRegionBatch), C.POINTER(vp)]
    lib.avk_compare_compact.argtypes = [vp, C.POINTER(AvkCompactBatch), C.POINTER(AvkCompareConfig), C.POINTER(AvkResultBatch)]
    lib.avk_batch_upload_compact.argtypes = [vp, C.POINTER(AvkCompactBatch), C.POINTER(vp)]
    lib.avk_compare_packed.argtypes = [vp, C.POINTER(AvkPackedBatch), C.POINTER(AvkCompareConfig), C.POINTER(AvkResultBatch)]
    if hasattr(lib, "avk_compare_packed_submit"):  # (AVK_LIB may name an older in-tree build: kernel A/B runs)
        lib.avk_compare_packed_submit.argtypes = [vp, C.POINTER(AvkPackedBatch), C.POINTER(AvkCompareConfig), C.POINTER(AvkResultBatch), C.POINTER(vp)]
        lib.avk_wait.argtypes = [vp, vp]
    lib.avk_batch_upload_packed.argtypes = [vp, C.POINTER(AvkPackedBatch), C.POINTER(vp)]
    esc = C.POINTER(AvkPackedEscapes)  # packed batches with escapes (avk_packed_escapes)
    lib.avk_compare_packed_esc.argtypes = [vp, C.POINTER(AvkPackedBatch), esc, C.POINTER(AvkCompareConfig), C.POINTER(AvkResultBatch)]
    lib.avk_compare_packed_submit_esc.argtypes = [vp, C.POINTER(AvkPackedBatch), esc, C.POINTER(AvkCompareConfig), C.POINTER(AvkResultBatch), C.POINTER(vp)]
    lib.avk_batch_upload_packed_esc.argtypes = [vp, C.POINTER(AvkPackedBatch), esc, C.POINTER(vp)]
    if hasattr(lib, "avk_label_block"):  # stratified sums from the compact results (avk_labels.inl); (AVK_LIB may name an older in-tree build: A/B runs)
        lab = C.POINTER(AvkRegionLabels)
        lib.avk_label_block.restype = C.c_uint32
        lib.avk_label_block.argtypes = [vp]
        lib.avk_label_tallies_compact.argtypes = [vp, vp, lab, u64p]
        lib.avk_compare_packed_labels.argtypes = [vp, C.POINTER(AvkPackedBatch), esc, lab, C.POINTER(AvkCompareConfig), C.POINTER(AvkResultBatch), u64p]
        lib.avk_compare_packed_submit_labels.argtypes = [vp, C.POINTER(AvkPackedBatch), esc, lab, C.POINTER(AvkCompareConfig), C.POINTER(AvkResultBatch), u64p, C.POINTER(vp)]
        lib.avk_packed_shard_labels.argtypes = [vp, lab, u64p, C.POINTER(C.c_uint32)]
    if hasattr(lib, "avk_strata_upload"):  # stratification sets resident on the device, lists by kernel (avk_strata.inl)
        lib.avk_strata_upload.argtypes = [vp, C.c_uint32, C.c_uint32, u64p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(vp)]
        lib.avk_strata_free.argtypes = [vp, vp]
        lib.avk_strata_free.restype = None
        lib.avk_strata_n_labels.restype = C.c_uint32
        lib.avk_strata_n_labels.argtypes = [vp]
        lib.avk_strata_region_labels.argtypes = [vp, vp, vp, u64p, C.POINTER(C.c_uint32), C.c_uint64]
        lib.avk_label_tallies_strata.argtypes = [vp, vp, vp, u64p]
        lib.avk_compare_packed_strata.argtypes = [vp, C.POINTER(AvkPackedBatch), esc, vp, C.POINTER(AvkCompareConfig), C.POINTER(AvkResultBatch), u64p]
    if hasattr(lib, "avk_compare_packed_submit_strata"):  # the submit with resident sets (AVK_LIB may name an older in-tree build: A/B runs)
        declare_submit_strata(lib)
    if hasattr(lib, "avk_strata_upload_context"):  # sequence-context labels behind the sets' (avk_context.inl); (AVK_LIB may name an older in-tree build: A/B runs)
        declare_context_strata(lib)
    if hasattr(lib, "avk_boot_tallies"):  # bootstrap replicates of the tallies (avk_boot.inl); (AVK_LIB may name an older in-tree build: A/B runs)
        declare_boot(lib)
    if hasattr(lib, "avk_size_tallies"):  # per-call tallies by size bin (avk_sizebin.inl); (AVK_LIB may name an older in-tree build: A/B runs)
        declare_size(lib)
    if hasattr(lib, "avk_score_tallies"):  # the curve by query score (avk_score.inl); (AVK_LIB may name an older in-tree build: A/B runs)
        declare_score(lib)
    if hasattr(lib, "avk_kind_tallies"):  # per-call tallies by call kind (avk_callkind.inl); (AVK_LIB may name an older in-tree build: A/B runs)
        declare_kind(lib)
    if hasattr(lib, "avk_kind_boot_tallies"):  # bootstrap replicates of the per-call blocks (avk_callboot.inl); (AVK_LIB may name an older in-tree build: A/B runs)
        declare_callboot(lib)
    if hasattr(lib, "avk_debug_ref_packed"):  # (AVK_LIB may name an older in-tree build: A/B runs)
        declare_debug_ref_packed(lib)
    lib.avk_compare_resident.argtypes = [vp, vp, C.POINTER(AvkCompareConfig), vp]
    lib.avk_results_download.argtypes = [vp, vp, C.POINTER(AvkResultBatch)]
    lib.avk_batch_free.argtypes = [vp, vp]
    lib.avk_batch_free.restype = None
    lib.avk_synchronize.argtypes = [vp]
    lib.avk_seq_stride.restype = C.c_uint32
    lib.avk_seq_stride.argtypes = [C.POINTER(AvkRegionBatch), C.c_uint64]
    lib.avk_last_kernel_ms.argtypes = [vp, C.POINTER(C.c_float)]
    lib.avk_last_solver_ms.argtypes = [vp, C.POINTER(C.c_float)]
    lib.avk_last_tier_counts.argtypes = [vp, u64p]
    lib.avk_last_compare_was_one_shot.argtypes = [vp]
    lib.avk_last_lane_ms.argtypes = [vp, C.POINTER(C.c_float)]
    lib.avk_last_lane_solved.argtypes = [vp, u64p]
    lib.avk_last_wide_solved.argtypes = [vp, u64p]
    lib.avk_debug_phase_cycles.argtypes = [vp, u64p]
    lib.avk_algorithmic_bytes.restype = C.c_uint64
    lib.avk_algorithmic_bytes.argtypes = [C.POINTER(AvkRegionBatch)]
    lib.avk_algorithmic_bytes_ex.restype = C.c_uint64
    lib.avk_algorithmic_bytes_ex.argtypes = [C.POINTER(AvkRegionBatch), C.c_int]
    lib.avk_optimize_pairs_batch.argtypes = [vp, C.POINTER(AvkRegionBatch), C.c_uint32, C.POINTER(C.c_int32), u8p]
    lib.avk_group_metrics_from_compact.argtypes = [C.POINTER(AvkRegionBatch), C.c_uint64, C.POINTER(AvkResultBatch), C.POINTER(C.c_uint32)]
    lib.avk_host_alloc.restype = vp
    lib.avk_host_alloc.argtypes = [vp, C.c_size_t]
    lib.avk_host_free.restype = None
    lib.avk_host_free.argtypes = [vp, vp]
    _lib = lib
    return lib


class CompareConfig:
    """CompareConfig (reference src/waffle_solver.rs:94-115); defaults as the reference's."""

    def __init__(self, enable_sequences=True, enable_exact_shortcut=False, max_branch_factor=50):
        self.enable_sequences = enable_sequences
        self.enable_exact_shortcut = enable_exact_shortcut
        self.max_branch_factor = max_branch_factor

    def c_struct(self):
        return AvkCompareConfig(self.max_branch_factor, 1 if self.enable_sequences else 0, 1 if self.enable_exact_shortcut else 0)


class ResidentBatch:
    """A region batch living in HBM (avk_dev_batch)."""

    def __init__(self, ctx, batch):
        self.ctx, self.batch = ctx, batch
        self.handle = C.c_void_p()
        cb = batch.c_struct()
        if isinstance(batch, PackedBatch):  # (with its escapes when it has any)
            esc = batch.c_escapes()
            if esc is None:
                ctx._check(ctx.lib.avk_batch_upload_packed(ctx.handle, C.byref(cb), C.byref(self.handle)))
            else:
                ctx._check(ctx.lib.avk_batch_upload_packed_esc(ctx.handle, C.byref(cb), C.byref(esc), C.byref(self.handle)))
            return
        if isinstance(batch, CompactBatch):
            ctx._check(ctx.lib.avk_batch_upload_compact(ctx.handle, C.byref(cb), C.byref(self.handle)))
            return
        ctx._check(ctx.lib.avk_batch_upload(ctx.handle, C.byref(cb), C.byref(self.handle)))

    def free(self):
        if self.handle:
            self.ctx.lib.avk_batch_free(self.ctx.handle, self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Strata:
    """The interval sets of a stratified job resident in HBM (avk_strata): uploaded once per context, then handed to solve_packed(strata=..),
    label_tallies_strata and strata_region_labels in place of label lists.  context=a ContextSpec: its sequence-context labels follow the sets' labels
    (avk_strata_upload_context); n_labels is then the total, n_context_labels the number of those."""

    def __init__(self, ctx, n_labels, n_contigs, tree_off, start, end_max, context=None):
        self.ctx = ctx
        self.handle = C.c_void_p()
        tree_off = np.ascontiguousarray(tree_off, np.uint64)
        start, end_max = np.ascontiguousarray(start, np.uint32), np.ascontiguousarray(end_max, np.uint32)
        if len(tree_off) != int(n_labels) * int(n_contigs) + 1 or len(start) != len(end_max) or (len(tree_off) and int(tree_off[-1]) > len(start)):
            raise ValueError("strata arrays do not fit n_labels * n_contigs trees")
        u32p = C.POINTER(C.c_uint32)
        if context is None:
            ctx._check(ctx.lib.avk_strata_upload(ctx.handle, int(n_labels), int(n_contigs), tree_off.ctypes.data_as(u64p), start.ctypes.data_as(u32p) if len(start) else None,
                                                 end_max.ctypes.data_as(u32p) if len(end_max) else None, C.byref(self.handle)))
        else:
            spec = context.c_struct()
            ctx._check(ctx.lib.avk_strata_upload_context(ctx.handle, int(n_labels), int(n_contigs), tree_off.ctypes.data_as(u64p), start.ctypes.data_as(u32p) if len(start) else None,
                                                         end_max.ctypes.data_as(u32p) if len(end_max) else None, C.byref(spec), C.byref(self.handle)))
        self.n_labels = int(ctx.lib.avk_strata_n_labels(self.handle))
        self.n_context_labels = 0 if context is None else int(ctx.lib.avk_strata_n_context_labels(self.handle))
        self.n_intervals = int(tree_off[-1]) - int(tree_off[0])
        ctx.__dict__.setdefault("_strata", weakref.WeakSet()).add(self)  # (Context.close frees the handles it still has: a handle must not outlive its context)

    def free(self):
        if self.handle and self.ctx.handle:
            self.ctx.lib.avk_strata_free(self.ctx.handle, self.handle)
        self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class _ContextCore:
    """The native context and its pinned blocks.  Arrays handed out by Context.host_array are views of avk_host_alloc memory: each block is freed when the LAST
    array that views it is collected (a finalizer on the buffer numpy keeps as the array's base), and the native context is destroyed when it has been closed AND
    its last block is gone — so an array read after close(), or at interpreter shutdown, never touches freed memory."""

    def __init__(self, lib, handle):
        self.lib, self.handle, self.live_blocks, self.closed = lib, handle, 0, False

    def release_block(self, p):
        if self.handle:
            self.lib.avk_host_free(self.handle, p)
        self.live_blocks -= 1
        self._destroy_if_done()

    def close(self):
        self.closed = True
        self._destroy_if_done()

    def _destroy_if_done(self):
        if self.closed and self.live_blocks <= 0 and self.handle:
            self.lib.avk_ctx_destroy(self.handle)
            self.handle = C.c_void_p()


class Ticket:
    """a batch in flight (Context.submit_packed); wait() returns its ResultBatch, once"""

    def __init__(self, ctx, handle, res, keep):
        self.ctx, self.handle, self.res, self._keep = ctx, handle, res, keep

    def wait(self):
        if self.handle is None:
            raise RuntimeError("the ticket has been waited for")
        h, self.handle = self.handle, None
        self.ctx._check(self.ctx.lib.avk_wait(self.ctx.handle, h))
        self._keep = None
        return self.res


class Context:
    """One GPU context (avk_ctx): owns the uploaded reference genome and the workspaces."""

    def __init__(self, device=0):
        self.lib = load_library()
        self.handle = C.c_void_p()
        rc = self.lib.avk_ctx_create(device, C.byref(self.handle))
        if rc != 0:
            raise AardvarkAmdError("avk_ctx_create(%d) failed (%d): %s" % (device, rc, self.lib.avk_last_error(None).decode()))
        self._contigs = None
        self._core = _ContextCore(self.lib, self.handle)
        self._strata = weakref.WeakSet()  # Strata handles of this context

    def close(self):
        """No call may follow.  The native context goes at once, or — when arrays of host_array / pinned_* are still referenced — with the last of them."""
        if self.handle:
            for s in list(getattr(self, "_strata", ())):
                s.free()
            self._core.close()
            self.handle = C.c_void_p()

    def host_array(self, shape, dtype):
        """a numpy array in pinned host memory (avk_host_alloc): batch and result arrays that live there are copied by DMA without a host pass;
        freed when the last array that views the block is collected (not by close(): see _ContextCore)"""
        count = int(np.prod(shape))
        nbytes = max(16, count * np.dtype(dtype).itemsize)
        p = self.lib.avk_host_alloc(self.handle, nbytes)
        if not p:
            raise AardvarkAmdError("avk_host_alloc(%d) failed: %s" % (nbytes, self.lib.avk_last_error(self.handle).decode()))
        buf = (C.c_uint8 * nbytes).from_address(p)
        self._core.live_blocks += 1
        weakref.finalize(buf, self._core.release_block, p)  # numpy keeps `buf` as the base of every view of the block
        return np.frombuffer(buf, dtype=dtype, count=count).reshape(shape)

    def pinned_batch(self, batch):
        """a copy of `batch` whose arrays live in pinned memory"""
        def pin(a):
            out = self.host_array(a.shape, a.dtype)
            out[...] = a
            return out
        return RegionBatch(*[pin(getattr(batch, f)) for f in ("region_id", "contig_idx", "start", "end", "t_off", "t_cnt", "q_off", "q_cnt", "var_pos", "var_type", "var_zyg",
                                                              "var_raw_space", "a0_off", "a0_len", "a1_off", "a1_len", "allele_bytes")])

    def pinned_compact(self, cbatch):
        """a copy of a CompactBatch whose arrays live in pinned memory"""
        def pin(a):
            if a is None:
                return None
            out = self.host_array(a.shape, a.dtype)
            out[...] = a
            return out
        return CompactBatch(**{f: pin(getattr(cbatch, f)) for f in CompactBatch.FIELDS})

    def pinned_packed(self, pbatch):
        """a copy of a PackedBatch whose arrays live in pinned memory"""
        def pin(a):
            if a is None:
                return None
            out = self.host_array(a.shape, a.dtype)
            out[...] = a
            return out
        esc = None if pbatch.escapes is None else pbatch.escapes.pinned(self.host_array)
        return PackedBatch(escapes=esc, **{f: pin(getattr(pbatch, f)) for f in PackedBatch.FIELDS})

    def solve_packed(self, pbatch, config=None, res=None, labels=None, label_tallies=None, strata=None, boot=None, boot_tallies=None, size=None, size_tallies=None, score=None, scores=None,
                     score_tallies=None, kinds=False, kind_tallies=None):
        """avk_compare_packed: solve_compare_region for every region of a batch in the packed form -> ResultBatch (indexed like the packed arrays).
        labels=(n_labels, label_off, label_idx): avk_compare_packed_labels — the per-label sums come back as res.label_tallies, a [n_labels, TALLY_LEN] uint64
        array (label_tallies: an array of that shape the sums are added to instead).
        strata=a Strata handle (upload_strata): avk_compare_packed_strata — the same sums, the lists made on the device.
        boot=a BootSpec: avk_compare_packed_boot — the bootstrap replicates come back as res.boot_tallies, a [1 + n_labels, replicates, TALLY_LEN] uint64 array
        (scope 0: every region; scope 1 + l: label l of `strata`; boot_tallies: an array of that shape the sums are added to instead).
        size=a SizeSpec: avk_compare_packed_size — the per-call tallies by size bin come back as res.size_tallies, a [1 + n_labels, n_bins, N_GROUPS, 14] uint64
        array (scopes as above; size_tallies: an array of that shape the sums are added to instead); it returns no label sums: labels, label_tallies and boot raise ValueError.
        score=a ScoreSpec, scores=a float32 array of n_variants (indexed like the packed call arrays; query entries are read, NaN: missing): avk_compare_packed_score —
        the curve by query score comes back as res.score_tallies, a [1 + n_labels, n_points, N_GROUPS, 14] uint64 array (score_tallies: an array the sums are added
        to instead); like size it excludes labels, label_tallies, boot and size.
        kinds=True: avk_compare_packed_kind — the per-call tallies by call kind (het / hom x Ti / Tv, KIND_NAMES) come back as res.kind_tallies, a
        [1 + n_labels, 9, N_GROUPS, 14] uint64 array (kind_tallies: an array of that shape the sums are added to instead); it excludes labels, label_tallies, boot,
        size and score"""
        config = config or CompareConfig(enable_sequences=False)
        res = res if res is not None else ResultBatch(pbatch, sequences=False, group_metrics=False)
        pb, cfg, ro, esc = pbatch.c_struct(), config.c_struct(), res.c_struct(), pbatch.c_escapes()
        if kinds:
            if labels is not None or label_tallies is not None or (boot is not None and boot.replicates) or size is not None or score is not None:
                raise ValueError("kinds takes strata, not label lists, returns no label sums (label_tallies) and excludes boot, size and score")
            n_labels = 0 if strata is None else strata.n_labels
            blocks = np.zeros((1 + n_labels, N_KINDS, N_GROUPS, KIND_FIELDS), np.uint64) if kind_tallies is None else kind_tallies
            self._check(self.lib.avk_compare_packed_kind(self.handle, C.byref(pb), None if esc is None else C.byref(esc), None if strata is None else strata.handle, C.byref(cfg),
                                                         C.byref(ro), blocks.ctypes.data_as(u64p)))
            res.kind_tallies = blocks
            return res
        if score is not None:
            if labels is not None or label_tallies is not None or (boot is not None and boot.replicates) or size is not None:
                raise ValueError("score takes strata, not label lists, returns no label sums (label_tallies) and excludes boot and size")
            n_labels = 0 if strata is None else strata.n_labels
            blocks = np.zeros((1 + n_labels, score.n_points, N_GROUPS, SCORE_FIELDS), np.uint64) if score_tallies is None else score_tallies
            ss, sc = score.c_struct(), _scores_array(scores, pbatch.n_variants)
            self._check(self.lib.avk_compare_packed_score(self.handle, C.byref(pb), None if esc is None else C.byref(esc), None if strata is None else strata.handle, C.byref(cfg),
                                                          C.byref(ss), None if sc is None else sc.ctypes.data_as(C.POINTER(C.c_float)), C.byref(ro), blocks.ctypes.data_as(u64p)))
            res.score_tallies = blocks
            return res
        if size is not None:
            if labels is not None or label_tallies is not None or (boot is not None and boot.replicates):
                raise ValueError("size takes strata, not label lists, returns no label sums (label_tallies) and excludes boot")
            n_labels = 0 if strata is None else strata.n_labels
            blocks = np.zeros((1 + n_labels, size.n_bins, N_GROUPS, SIZE_FIELDS), np.uint64) if size_tallies is None else size_tallies
            ss = size.c_struct()
            self._check(self.lib.avk_compare_packed_size(self.handle, C.byref(pb), None if esc is None else C.byref(esc), None if strata is None else strata.handle, C.byref(cfg),
                                                         C.byref(ss), C.byref(ro), blocks.ctypes.data_as(u64p)))
            res.size_tallies = blocks
            return res
        if boot is not None and boot.replicates:
            if labels is not None:
                raise ValueError("boot takes strata, not label lists")
            n_labels = 0 if strata is None else strata.n_labels
            sums = np.zeros((n_labels, TALLY_LEN), np.uint64) if label_tallies is None else label_tallies
            reps = np.zeros((1 + n_labels, boot.replicates, TALLY_LEN), np.uint64) if boot_tallies is None else boot_tallies
            bs = boot.c_struct()
            self._check(self.lib.avk_compare_packed_boot(self.handle, C.byref(pb), None if esc is None else C.byref(esc), None if strata is None else strata.handle, C.byref(cfg),
                                                         C.byref(ro), sums.ctypes.data_as(u64p), C.byref(bs), reps.ctypes.data_as(u64p)))
            if strata is not None:
                res.label_tallies = sums
            res.boot_tallies = reps
            return res
        if strata is not None:
            if labels is not None:
                raise ValueError("labels and strata exclude each other")
            sums = np.zeros((strata.n_labels, TALLY_LEN), np.uint64) if label_tallies is None else label_tallies
            self._check(self.lib.avk_compare_packed_strata(self.handle, C.byref(pb), None if esc is None else C.byref(esc), strata.handle, C.byref(cfg), C.byref(ro),
                                                           sums.ctypes.data_as(u64p)))
            res.label_tallies = sums
            return res
        if labels is not None:
            lab, _keep = region_labels(*labels)
            sums = np.zeros((int(labels[0]), TALLY_LEN), np.uint64) if label_tallies is None else label_tallies
            self._check(self.lib.avk_compare_packed_labels(self.handle, C.byref(pb), None if esc is None else C.byref(esc), C.byref(lab), C.byref(cfg), C.byref(ro),
                                                           sums.ctypes.data_as(u64p)))
            res.label_tallies = sums
            return res
        if esc is None:
            self._check(self.lib.avk_compare_packed(self.handle, C.byref(pb), C.byref(cfg), C.byref(ro)))
        else:
            self._check(self.lib.avk_compare_packed_esc(self.handle, C.byref(pb), C.byref(esc), C.byref(cfg), C.byref(ro)))
        return res

    def submit_packed(self, pbatch, config=None, res=None, labels=None, label_tallies=None, strata=None):
        """avk_compare_packed_submit: the batch is queued (its copies run beside the kernels of the batch submitted before) -> a Ticket; Ticket.wait() -> ResultBatch.
        `pbatch` and `res` must live in pinned memory (pinned_packed / pinned_results) for the copies to overlap anything; at most four tickets are in flight.
        labels=(n_labels, label_off, label_idx): avk_compare_packed_submit_labels — res.label_tallies holds the per-label sums once wait() has returned (pin the
        two arrays with host_array for the submit to stay asynchronous).
        strata=a Strata handle (upload_strata): avk_compare_packed_submit_strata — the same sums, the labels read from the masks made on the device; the Ticket
        keeps the Strata object alive (Strata.free() before wait() is allowed: the library finishes the batch's mask pass first)"""
        config = config or CompareConfig(enable_sequences=False)
        res = res if res is not None else ResultBatch(pbatch, sequences=False, group_metrics=False)
        pb, cfg, ro, esc = pbatch.c_struct(), config.c_struct(), res.c_struct(), pbatch.c_escapes()
        handle = C.c_void_p()
        if strata is not None:
            if labels is not None:
                raise ValueError("labels and strata exclude each other")
            sums = np.zeros((strata.n_labels, TALLY_LEN), np.uint64) if label_tallies is None else label_tallies
            self._check(self.lib.avk_compare_packed_submit_strata(self.handle, C.byref(pb), None if esc is None else C.byref(esc), strata.handle, C.byref(cfg), C.byref(ro),
                                                                  sums.ctypes.data_as(u64p), C.byref(handle)))
            res.label_tallies = sums
            return Ticket(self, handle, res, (pbatch, pb, ro, esc, strata, sums))
        if labels is not None:
            lab, keep = region_labels(*labels)
            sums = np.zeros((int(labels[0]), TALLY_LEN), np.uint64) if label_tallies is None else label_tallies
            self._check(self.lib.avk_compare_packed_submit_labels(self.handle, C.byref(pb), None if esc is None else C.byref(esc), C.byref(lab), C.byref(cfg), C.byref(ro),
                                                                  sums.ctypes.data_as(u64p), C.byref(handle)))
            res.label_tallies = sums
            return Ticket(self, handle, res, (pbatch, pb, ro, esc, lab, keep, sums))
        if esc is None:
            self._check(self.lib.avk_compare_packed_submit(self.handle, C.byref(pb), C.byref(cfg), C.byref(ro), C.byref(handle)))
        else:
            self._check(self.lib.avk_compare_packed_submit_esc(self.handle, C.byref(pb), C.byref(esc), C.byref(cfg), C.byref(ro), C.byref(handle)))
        return Ticket(self, handle, res, (pbatch, pb, ro, esc))

    def solve_compact(self, cbatch, config=None, res=None):
        """avk_compare_compact: solve_compare_region for every region of a batch in the compact form -> ResultBatch (indexed like the compact arrays)"""
        config = config or CompareConfig(enable_sequences=False)
        res = res if res is not None else ResultBatch(cbatch, sequences=False, group_metrics=False)
        cb, cfg, ro = cbatch.c_struct(), config.c_struct(), res.c_struct()
        self._check(self.lib.avk_compare_compact(self.handle, C.byref(cb), C.byref(cfg), C.byref(ro)))
        return res

    def pinned_results(self, batch, group_metrics=False, bp_groups=False, packed=False):
        """a ResultBatch whose arrays live in pinned memory (packed: as ResultBatch)"""
        res = ResultBatch(batch, sequences=False, group_metrics=group_metrics, bp_groups=bp_groups, packed=packed)
        for f in ("status", "ed_h1", "ed_h2", "n_optima", "type_present", "var_expected", "var_observed", "var_class", "var_zyg", "region_packed", "var_packed",
                  "group_metrics", "bp_off", "bp_groups", "bp_packed", "bp_spilled"):
            a = getattr(res, f, None)
            if a is None:
                continue
            b = self.host_array(a.shape, a.dtype)
            b[...] = a
            setattr(res, f, b)
        return res

    def expand_results(self, res, batch):
        """the wide arrays of a ResultBatch that holds the packed form (avk_results_expand)"""
        return res.expanded(self.lib, batch)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise AardvarkAmdError("libaardvark_amd error %d: %s" % (rc, self.lib.avk_last_error(self.handle).decode()))

    def set_option(self, name, value):
        self._check(self.lib.avk_ctx_set_option(self.handle, name.encode(), int(value)))

    def set_stream(self, hip_stream):
        self._check(self.lib.avk_ctx_set_stream(self.handle, C.c_void_p(hip_stream)))

    def upload_reference(self, contigs):
        """contigs: list of bytes / uint8 arrays (ReferenceGenome::from_fasta + get_full_chromosome,
        reference src/main.rs:94, src/waffle_solver.rs:131)."""
        arrs = [np.frombuffer(c, dtype=np.uint8) if isinstance(c, (bytes, bytearray)) else np.ascontiguousarray(c, dtype=np.uint8)
                for c in contigs]
        ptrs = (u8p * len(arrs))(*[a.ctypes.data_as(u8p) for a in arrs])
        lens = (C.c_uint64 * len(arrs))(*[a.size for a in arrs])
        self._check(self.lib.avk_ref_upload(self.handle, len(arrs), ptrs, lens))
        self._contigs = arrs

    def solve_compare_regions(self, batch, config=None, group_metrics=True, bp_groups=False, packed=False):
        """solve_compare_region for every region of `batch` -> ResultBatch."""
        config = config or CompareConfig()
        res = ResultBatch(batch, sequences=bool(config.enable_sequences), group_metrics=group_metrics, bp_groups=bp_groups, packed=packed)
        cb, cfg, ro = batch.c_struct(), config.c_struct(), res.c_struct()
        self._check(self.lib.avk_compare_batch(self.handle, C.byref(cb), C.byref(cfg), C.byref(ro)))
        return res

    # --- resident form (benchmarks, pipelines that keep batches in HBM)
    def upload(self, batch):
        """a RegionBatch, a CompactBatch, or a PackedBatch (with its escapes) -> ResidentBatch"""
        return ResidentBatch(self, batch)

    def compare_resident(self, rb, config=None, tally_dev_ptr=None):
        config = config or CompareConfig(enable_sequences=False)
        cfg = config.c_struct()
        self._check(self.lib.avk_compare_resident(self.handle, rb.handle, C.byref(cfg), C.c_void_p(tally_dev_ptr or 0)))

    def download(self, rb, sequences=False, group_metrics=True, packed=False):
        res = ResultBatch(rb.batch, sequences=sequences, group_metrics=group_metrics, packed=packed)
        ro = res.c_struct()
        self._check(self.lib.avk_results_download(self.handle, rb.handle, C.byref(ro)))
        return res

    def label_tallies(self, rb, n_labels, label_off, label_idx, out=None):
        """avk_label_tallies: per-label sums of the resident batch's per-region metric blocks (needs emit_group_metrics during
        compare_resident); returns / adds to a [n_labels, TALLY_LEN] uint64 array"""
        out = np.zeros((n_labels, TALLY_LEN), np.uint64) if out is None else out
        off = np.ascontiguousarray(label_off, np.uint64)
        idx = np.ascontiguousarray(label_idx, np.uint32)
        if idx.size == 0:
            idx = np.zeros(1, np.uint32)
        self.lib.avk_label_tallies.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
        self._check(self.lib.avk_label_tallies(self.handle, rb.handle, n_labels, off.ctypes.data_as(C.POINTER(C.c_uint64)), idx.ctypes.data_as(C.POINTER(C.c_uint32)),
                                               out.ctypes.data_as(C.POINTER(C.c_uint64))))
        return out

    def label_block(self):
        """avk_label_block: how many labels one launch of the compact label kernel sums (more labels: more passes over the regions)"""
        return int(self.lib.avk_label_block(self.handle))

    def label_tallies_compact(self, rb, n_labels, label_off, label_idx, out=None):
        """avk_label_tallies_compact: the sums of label_tallies without per-region metric blocks — from the resident batch's compact results (needs
        emit_bp_groups during compare_resident; emit_group_metrics may be 0); returns / adds to a [n_labels, TALLY_LEN] uint64 array"""
        out = np.zeros((n_labels, TALLY_LEN), np.uint64) if out is None else out
        lab, _keep = region_labels(n_labels, label_off, label_idx)
        self._check(self.lib.avk_label_tallies_compact(self.handle, rb.handle, C.byref(lab), out.ctypes.data_as(u64p)))
        return out

    def upload_strata(self, n_labels, n_contigs, tree_off, start, end_max, context=None):
        """avk_strata_upload: the interval sets of a stratified job (Stratifications.export(genome) of the feeder) into HBM, once -> Strata.
        context=a ContextSpec: avk_strata_upload_context — GC and homopolymer labels, made by kernel from the uploaded reference, behind the sets' labels
        (n_labels == 0 with tree_off == [0]: context labels only)"""
        return Strata(self, n_labels, n_contigs, tree_off, start, end_max, context)

    def strata_region_labels(self, rb, strata):
        """avk_strata_region_labels: the containment lists of a resident batch, made on the device -> (label_off[n + 1], label_idx)"""
        off = np.zeros(rb.batch.n_regions + 1, np.uint64)
        self._check(self.lib.avk_strata_region_labels(self.handle, rb.handle, strata.handle, off.ctypes.data_as(u64p), None, 0))
        idx = np.zeros(max(int(off[-1]), 1), np.uint32)
        self._check(self.lib.avk_strata_region_labels(self.handle, rb.handle, strata.handle, off.ctypes.data_as(u64p), idx.ctypes.data_as(C.POINTER(C.c_uint32)), int(off[-1])))
        return off, idx[:int(off[-1])]

    def label_tallies_strata(self, rb, strata, out=None):
        """avk_label_tallies_strata: label_tallies_compact with the lists made on the device from the resident sets; returns / adds to [n_labels, TALLY_LEN]"""
        out = np.zeros((strata.n_labels, TALLY_LEN), np.uint64) if out is None else out
        self._check(self.lib.avk_label_tallies_strata(self.handle, rb.handle, strata.handle, out.ctypes.data_as(u64p)))
        return out

    def boot_block(self):
        """avk_boot_block: how many replicates of one scope a launch of the bootstrap kernel holds (more replicates or scopes: more launches)"""
        return int(self.lib.avk_boot_block(self.handle))

    def boot_tallies(self, rb, spec, strata=None, out=None):
        """avk_boot_tallies: the bootstrap replicates of a solved resident batch (needs emit_bp_groups during compare_resident); returns / adds to a
        [1 + n_labels, replicates, TALLY_LEN] uint64 array — scope 0: every region; scope 1 + l: label l of `strata`"""
        n_labels = 0 if strata is None else strata.n_labels
        out = np.zeros((1 + n_labels, max(spec.replicates, 0), TALLY_LEN), np.uint64) if out is None else out
        bs = spec.c_struct()
        self._check(self.lib.avk_boot_tallies(self.handle, rb.handle, C.byref(bs), None if strata is None else strata.handle, out.ctypes.data_as(u64p)))
        return out

    def size_block(self):
        """avk_size_block: how many regions a workgroup of the size-bin kernel takes at a time (one lane each)"""
        return int(self.lib.avk_size_block(self.handle))

    def size_tallies(self, rb, spec, strata=None, out=None):
        """avk_size_tallies: the per-call tallies by size bin of a solved resident batch (no option is needed); returns / adds to a
        [1 + n_labels, n_bins, N_GROUPS, 14] uint64 array — scope 0: every region; scope 1 + l: label l of `strata`"""
        n_labels = 0 if strata is None else strata.n_labels
        out = np.zeros((1 + n_labels, spec.n_bins, N_GROUPS, SIZE_FIELDS), np.uint64) if out is None else out
        ss = spec.c_struct()
        self._check(self.lib.avk_size_tallies(self.handle, rb.handle, C.byref(ss), None if strata is None else strata.handle, out.ctypes.data_as(u64p)))
        return out

    def score_block(self):
        """avk_score_block: how many regions a workgroup of the score histogram kernel takes at a time (one lane each)"""
        return int(self.lib.avk_score_block(self.handle))

    def score_tallies(self, rb, spec, scores, strata=None, out=None):
        """avk_score_tallies: the precision-recall curve by query score of a solved resident batch; scores: a float32 array of the batch's n_variants, indexed like
        its call arrays (NaN: missing); returns / adds to a [1 + n_labels, n_points, N_GROUPS, 14] uint64 array — scope 0: every region; scope 1 + l: label l of
        `strata`; point 0: no filter; point k: score >= thresholds[k - 1]"""
        n_labels = 0 if strata is None else strata.n_labels
        out = np.zeros((1 + n_labels, spec.n_points, N_GROUPS, SCORE_FIELDS), np.uint64) if out is None else out
        ss, sc = spec.c_struct(), _scores_array(scores, rb.batch.n_variants)
        self._check(self.lib.avk_score_tallies(self.handle, rb.handle, C.byref(ss), None if sc is None else sc.ctypes.data_as(C.POINTER(C.c_float)),
                                               None if strata is None else strata.handle, out.ctypes.data_as(u64p)))
        return out

    def kind_block(self):
        """avk_kind_block: how many regions a workgroup of the call-kind kernel takes at a time (one lane each)"""
        return int(self.lib.avk_kind_block(self.handle))

    def kind_tallies(self, rb, strata=None, out=None):
        """avk_kind_tallies: the per-call tallies by call kind of a solved resident batch (no option is needed); returns / adds to a
        [1 + n_labels, 9, N_GROUPS, 14] uint64 array — scope 0: every region; scope 1 + l: label l of `strata`; the kinds are KIND_NAMES"""
        n_labels = 0 if strata is None else strata.n_labels
        out = np.zeros((1 + n_labels, N_KINDS, N_GROUPS, KIND_FIELDS), np.uint64) if out is None else out
        self._check(self.lib.avk_kind_tallies(self.handle, rb.handle, None if strata is None else strata.handle, out.ctypes.data_as(u64p)))
        return out

    def callboot_block(self, n_keys):
        """avk_callboot_block: how many replicates of one scope a launch of the per-call bootstrap kernel holds for n_keys keys (9 kinds, or a SizeSpec's n_bins)"""
        return int(self.lib.avk_callboot_block(self.handle, int(n_keys)))

    def size_boot_tallies(self, rb, spec, boot, strata=None, out=None):
        """avk_size_boot_tallies: the bootstrap replicates of size_tallies' block of a solved resident batch; returns / adds to a
        [1 + n_labels, replicates, n_bins, N_GROUPS, 14] uint64 array — replicate b weighs every region as replicate b of boot_tallies does for the same seed"""
        n_labels = 0 if strata is None else strata.n_labels
        out = np.zeros((1 + n_labels, max(boot.replicates, 0), spec.n_bins, N_GROUPS, SIZE_FIELDS), np.uint64) if out is None else out
        ss, bs = spec.c_struct(), boot.c_struct()
        self._check(self.lib.avk_size_boot_tallies(self.handle, rb.handle, C.byref(ss), C.byref(bs), None if strata is None else strata.handle, out.ctypes.data_as(u64p)))
        return out

    def kind_boot_tallies(self, rb, boot, strata=None, out=None):
        """avk_kind_boot_tallies: the bootstrap replicates of kind_tallies' block of a solved resident batch; returns / adds to a
        [1 + n_labels, replicates, 9, N_GROUPS, 14] uint64 array"""
        n_labels = 0 if strata is None else strata.n_labels
        out = np.zeros((1 + n_labels, max(boot.replicates, 0), N_KINDS, N_GROUPS, KIND_FIELDS), np.uint64) if out is None else out
        bs = boot.c_struct()
        self._check(self.lib.avk_kind_boot_tallies(self.handle, rb.handle, C.byref(bs), None if strata is None else strata.handle, out.ctypes.data_as(u64p)))
        return out

    def synchronize(self):
        self._check(self.lib.avk_synchronize(self.handle))

    def last_kernel_ms(self):
        ms = C.c_float(0)
        self._check(self.lib.avk_last_kernel_ms(self.handle, C.byref(ms)))
        return float(ms.value)

    def last_solver_ms(self):
        ms = C.c_float(0)
        self._check(self.lib.avk_last_solver_ms(self.handle, C.byref(ms)))
        return float(ms.value)

    def last_compare_was_one_shot(self):
        return bool(self.lib.avk_last_compare_was_one_shot(self.handle))

    def last_lane_ms(self):
        """HIP-event time from the start of the last step to the end of its lane-per-region launches (0 when it had none)"""
        ms = C.c_float(0)
        self._check(self.lib.avk_last_lane_ms(self.handle, C.byref(ms)))
        return float(ms.value)

    def last_lane_solved(self):
        """regions the lane-per-region kernel finished in the step whose results were downloaded last"""
        out = C.c_uint64(0)
        self._check(self.lib.avk_last_lane_solved(self.handle, C.byref(out)))
        return int(out.value)

    def last_wide_solved(self):
        """regions the wave-cooperative kernel of the large searches on small windows (avk_wide.inl) finished in the step whose results were downloaded last"""
        out = C.c_uint64(0)
        self._check(self.lib.avk_last_wide_solved(self.handle, C.byref(out)))
        return int(out.value)

    def last_region_launches(self):
        """launches of the packer's region pass the last device-packed upload queued (avk_last_region_launches): 1, 2 when calls were left to the host's edit
        distance; N + 1 (N + 2) on the chunked route of the option pack_chunks = N"""
        out = C.c_uint64(0)
        self.lib.avk_last_region_launches.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        self._check(self.lib.avk_last_region_launches(self.handle, C.byref(out)))
        return int(out.value)

    def last_tier_counts(self):
        out = (C.c_uint64 * 5)()
        self._check(self.lib.avk_last_tier_counts(self.handle, out))
        return [int(x) for x in out]

    def work_order(self, rb, want_order=True):
        """avk_debug_work_order: (order[n] or None, plan) of a device-packed resident batch; plan = {"class_c", "class_c_not_wide", "class_b", "lanes",
        "fast": [(first record, regions, head regions) per lane class]}"""
        import numpy as np
        n = rb.batch.n_regions
        order = np.zeros(max(n, 1), np.uint32) if want_order else None
        counts = (C.c_uint64 * 22)()
        self.lib.avk_debug_work_order.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
        self._check(self.lib.avk_debug_work_order(self.handle, rb.handle, order.ctypes.data_as(C.POINTER(C.c_uint32)) if want_order else None, counts))
        c = [int(x) for x in counts]
        return (order[:n] if want_order else None), {"class_c": c[0], "class_c_not_wide": c[1], "class_b": c[2], "lanes": c[3],
                                                      "fast": [(c[4 + 3 * k], c[5 + 3 * k], c[6 + 3 * k]) for k in range(6)]}

    def debug_ref_packed(self):
        """avk_debug_ref_packed: (packed words uint32[], flag words uint32[]) of the current reference as the device holds them — the words that cover the reference and
        the context's whole flag bitmap (include/aardvark_amd.h has the layout)"""
        if self._contigs is None:
            n_words, n_flags = 0, 8  # no upload through this object: the library refuses
        else:
            n_words, n_flags = ref_packed_sizes(sum(a.size for a in self._contigs))
        words, flags = np.zeros(max(n_words, 1), np.uint32), np.zeros(n_flags, np.uint32)
        u32p = C.POINTER(C.c_uint32)
        self._check(self.lib.avk_debug_ref_packed(self.handle, words.ctypes.data_as(u32p), n_words, flags.ctypes.data_as(u32p), n_flags))
        return words[:n_words], flags

    def debug_phase_cycles(self):
        out = (C.c_uint64 * 16)()
        self._check(self.lib.avk_debug_phase_cycles(self.handle, out))
        return [int(x) for x in out]

    def optimize_pairs(self, batch, max_branch_factor=50):
        """merge path: optimize_sequences(truth range, query range)[0].is_exact_match() per region
        (reference src/merge_solver.rs:135-147) -> (status int32[], is_exact uint8[])"""
        status = np.full(batch.n_regions, -1, np.int32)
        exact = np.zeros(max(batch.n_regions, 1), np.uint8)
        cb = batch.c_struct()
        self._check(self.lib.avk_optimize_pairs_batch(self.handle, C.byref(cb), max_branch_factor,
                                                      status.ctypes.data_as(C.POINTER(C.c_int32)), exact.ctypes.data_as(u8p)))
        return status, exact[:batch.n_regions]

    def algorithmic_bytes(self, batch, with_groups=True):
        cb = batch.c_struct()
        return int(self.lib.avk_algorithmic_bytes_ex(C.byref(cb), 1 if with_groups else 0))


def group_metrics_from_compact(batch, res):
    """avk_group_metrics_from_compact for every solved region: the full [n][13][22] blocks rebuilt on the host from the per-call outputs and the compact per-region
    BASEPAIR groups of `res` (regions with a non-zero status stay zero)"""
    lib = load_library()
    out = np.zeros((batch.n_regions, 13, 22), np.uint32)
    cb, ro = batch.c_struct(), res.c_struct()
    status = res.status if res.status is not None else (res.region_packed & np.uint64(0x7F))
    for r in range(batch.n_regions):
        if status[r] != 0:
            continue
        rc = lib.avk_group_metrics_from_compact(C.byref(cb), r, C.byref(ro), out[r].ctypes.data_as(C.POINTER(C.c_uint32)))
        if rc != 0:
            raise AardvarkAmdError("avk_group_metrics_from_compact failed for region %d" % r)
    return out


def _scores_array(scores, n_variants):
    """a contiguous float32 array (None stays None: the library refuses it by name); n_variants: the length the batch asks for, when it is known here"""
    if scores is None:
        return None
    sc = np.ascontiguousarray(scores, dtype=np.float32)
    if n_variants is not None and sc.size != int(n_variants):
        raise ValueError("scores holds %d values, the batch %d calls" % (sc.size, int(n_variants)))
    return sc


def score_tallies_host(batch, res, spec, scores, labels=None, threads=1, out=None):
    """avk_score_tallies_host: Context.score_tallies' curve on the host from a wide RegionBatch, its ResultBatch and the scores (no GPU involved);
    labels=(n_labels, label_off, label_idx) or None -> [1 + n_labels, n_points, N_GROUPS, 14] uint64 (added to `out`)"""
    lib = load_library()
    n_labels = 0 if labels is None else int(labels[0])
    out = np.zeros((1 + n_labels, spec.n_points, N_GROUPS, SCORE_FIELDS), np.uint64) if out is None else out
    cb, ro, ss, sc = batch.c_struct(), res.c_struct(), spec.c_struct(), _scores_array(scores, batch.n_variants)
    lab = None
    if labels is not None:
        lab, _keep = region_labels(*labels)
    rc = lib.avk_score_tallies_host(C.byref(cb), C.byref(ro), C.byref(ss), None if sc is None else sc.ctypes.data_as(C.POINTER(C.c_float)), None if lab is None else C.byref(lab),
                                    int(threads), out.ctypes.data_as(C.POINTER(C.c_uint64)))
    if rc:
        raise AardvarkAmdError("avk_score_tallies_host: %d: %s" % (rc, lib.avk_last_error(None).decode()))
    return out


def size_tallies_host(batch, res, spec, labels=None, threads=1, out=None):
    """avk_size_tallies_host: Context.size_tallies' sums on the host from a wide RegionBatch and its ResultBatch (no GPU involved);
    labels=(n_labels, label_off, label_idx) or None -> [1 + n_labels, n_bins, N_GROUPS, 14] uint64 (added to `out`)"""
    lib = load_library()
    n_labels = 0 if labels is None else int(labels[0])
    out = np.zeros((1 + n_labels, spec.n_bins, N_GROUPS, SIZE_FIELDS), np.uint64) if out is None else out
    cb, ro, ss = batch.c_struct(), res.c_struct(), spec.c_struct()
    lab = None
    if labels is not None:
        lab, _keep = region_labels(*labels)
    rc = lib.avk_size_tallies_host(C.byref(cb), C.byref(ro), C.byref(ss), None if lab is None else C.byref(lab), int(threads), out.ctypes.data_as(C.POINTER(C.c_uint64)))
    if rc:
        raise AardvarkAmdError("avk_size_tallies_host: %d: %s" % (rc, lib.avk_last_error(None).decode()))
    return out


def kind_tallies_host(batch, res, labels=None, threads=1, out=None):
    """avk_kind_tallies_host: Context.kind_tallies' sums on the host from a wide RegionBatch and its ResultBatch (no GPU involved);
    labels=(n_labels, label_off, label_idx) or None -> [1 + n_labels, 9, N_GROUPS, 14] uint64 (added to `out`)"""
    lib = load_library()
    n_labels = 0 if labels is None else int(labels[0])
    out = np.zeros((1 + n_labels, N_KINDS, N_GROUPS, KIND_FIELDS), np.uint64) if out is None else out
    cb, ro = batch.c_struct(), res.c_struct()
    lab = None
    if labels is not None:
        lab, _keep = region_labels(*labels)
    rc = lib.avk_kind_tallies_host(C.byref(cb), C.byref(ro), None if lab is None else C.byref(lab), int(threads), out.ctypes.data_as(C.POINTER(C.c_uint64)))
    if rc:
        raise AardvarkAmdError("avk_kind_tallies_host: %d: %s" % (rc, lib.avk_last_error(None).decode()))
    return out


def _callboot_host(name, batch, res, spec, boot, labels, threads, out, n_keys):
    lib = load_library()
    n_labels = 0 if labels is None else int(labels[0])
    out = np.zeros((1 + n_labels, max(boot.replicates, 0), n_keys, N_GROUPS, SIZE_FIELDS), np.uint64) if out is None else out
    cb, ro, bs = batch.c_struct(), res.c_struct(), boot.c_struct()
    lab = None
    if labels is not None:
        lab, _keep = region_labels(*labels)
    args = [C.byref(cb), C.byref(ro)] + ([] if spec is None else [C.byref(spec)]) + [C.byref(bs), None if lab is None else C.byref(lab), int(threads),
                                                                                     out.ctypes.data_as(C.POINTER(C.c_uint64))]
    rc = getattr(lib, name)(*args)
    if rc:
        raise AardvarkAmdError("%s: %d: %s" % (name, rc, lib.avk_last_error(None).decode()))
    return out


def size_boot_tallies_host(batch, res, spec, boot, labels=None, threads=1, out=None):
    """avk_size_boot_tallies_host: Context.size_boot_tallies' sums on the host from a wide RegionBatch and its ResultBatch (no GPU involved);
    labels=(n_labels, label_off, label_idx) or None -> [1 + n_labels, replicates, n_bins, N_GROUPS, 14] uint64 (added to `out`)"""
    return _callboot_host("avk_size_boot_tallies_host", batch, res, spec.c_struct(), boot, labels, threads, out, spec.n_bins)


def kind_boot_tallies_host(batch, res, boot, labels=None, threads=1, out=None):
    """avk_kind_boot_tallies_host: Context.kind_boot_tallies' sums on the host -> [1 + n_labels, replicates, 9, N_GROUPS, 14] uint64 (added to `out`)"""
    return _callboot_host("avk_kind_boot_tallies_host", batch, res, None, boot, labels, threads, out, N_KINDS)
