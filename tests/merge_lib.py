"""Helpers for tests of the merge path on the GPU: the small merge job of synth.config_genome_merge, and solve_merge_region for a whole MultiBatch from the C
oracle's pairs and the restated rule (oracle/merge_oracle.py: classify).  (tests/test_gpu_merge_sweep.py and tests/test_merge_shard.py carry their own copies of
oracle_merge; new tests take this one.)"""
import functools
import os
import sys

import numpy as np

import escapes_lib as el
import oracle_lib
from aardvark_amd import synth
from aardvark_amd.merge import MergeResult

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import merge_oracle as mo  # noqa: E402


@functools.lru_cache(maxsize=None)
def small_job(k, regions=None):
    """(contigs, MultiBatch) of the small job with k call sets; regions: its first so many MultiRegions"""
    contigs, mb = synth.config_genome_merge(scale=0.0008, k=k, threads=4)
    if regions is not None:
        mb = el.reordered_multi(mb, np.arange(regions))
    return contigs, mb


def same(a, b):
    return np.array_equal(a.status, b.status) and np.array_equal(a.classification, b.classification) and np.array_equal(a.members, b.members)


def oracle_merge(oracle, mb, contigs, cfg, threads=4):
    """solve_merge_region for a MultiBatch of any number of inputs -> MergeResult"""
    import bench
    k, n = mb.n_inputs, mb.n_regions
    ppr = k * (k - 1) // 2
    st, ex = oracle_lib.optimize_pairs(oracle, bench.pair_batch_of(mb), contigs, cfg.max_branch_factor, threads=threads)
    st, ex = np.asarray(st).reshape(n, ppr), np.asarray(ex).reshape(n, ppr)
    index = {(i, j): p for p, (i, j) in enumerate((i, j) for i in range(k) for j in range(i + 1, k))}
    cnt = mb.in_cnt.astype(np.int64).reshape(n, k)
    unknown = np.zeros(n, bool)
    np.logical_or.at(unknown, np.repeat(np.arange(n), cnt.sum(axis=1)), mb.var_zyg == 0)
    status, cls, members = np.zeros(n, np.int32), np.zeros(n, np.uint8), np.zeros(n, np.uint64)
    code = {"different": 0, "identical": 1, "no_conflict": 2, "majority": 3, "conflict_select": 4}
    for m in range(n):
        if unknown[m] or st[m].any():
            status[m] = 6 if unknown[m] else int(st[m][np.flatnonzero(st[m])[0]])
            continue
        got = mo.classify(cnt[m].tolist(), lambda i, j: ex[m, index[(i, j)]], cfg.no_conflict_enabled, cfg.majority_voting_enabled, cfg.conflict_selection)
        cls[m] = code[got[0]]
        members[m] = 0 if len(got) == 1 else (got[1] if got[0] == "conflict_select" else sum(1 << i for i in got[1]))
    return MergeResult(status, cls, members, k)
