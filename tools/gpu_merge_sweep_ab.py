"""One pair solve decided under several strategies (avk_merge_packed_sweep) against one call per strategy, on the 3-caller merge job of bench.py's merge leg
(profiles/merge_sweep_ab.txt).

usage: python tools/gpu_merge_sweep_ab.py [SCALE=0.1] [leg] [N=9]
  no leg: every leg below in a fresh process each, medians of N
  leg = four      a sweep of four configs (exact, no_conflict, majority, all + select 1) with counters against four avk_merge_packed_counts, the forms alternating
        one       a sweep of ONE config with counters against avk_merge_packed_counts with the same config, alternating
        single    avk_merge_packed_counts alone (AVK_LIB names the library: run it once per build to compare two builds under the same Python)
        kernels   five sweeps of four and nothing else: the process to run under `rocprofv3 --kernel-trace --stats -- python tools/gpu_merge_sweep_ab.py SCALE kernels`
Every leg first checks that the sweep's slices and blocks equal the single calls'."""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np


def leg(scale, name, reps):
    import aardvark_amd
    from aardvark_amd import synth
    from aardvark_amd.merge import MergeConfig, PackedMultiBatch, counts_on_device, merge_counts_len, merge_multi_batch, pinned_multi_batch
    contigs, mb = synth.config_genome_merge(scale=scale, k=3, threads=8)
    ctx = aardvark_amd.Context(0)
    ctx.upload_reference(contigs)
    four = [MergeConfig(), MergeConfig(no_conflict_enabled=True), MergeConfig(majority_voting_enabled=True),
            MergeConfig(no_conflict_enabled=True, majority_voting_enabled=True, conflict_selection=1)]
    pk = pinned_multi_batch(ctx, PackedMultiBatch.from_multi(mb))
    n = merge_counts_len(ctx.lib, 3)
    print("leg %s: scale %g, %d regions, %d calls, library %s (source %s), medians of %d" % (name, scale, pk.n_regions, pk.n_variants, os.environ.get("AVK_LIB", "libaardvark_amd.so"),
                                                                                         ctx.lib.avk_source_hash().decode(), reps), flush=True)
    fmt = lambda ts: "%.2f ms (median of %s)" % (float(np.median(ts)), " ".join("%.2f" % t for t in ts))

    def single(cfg):
        c = np.zeros(n, np.uint64)
        return merge_multi_batch(ctx, pk, cfg, counts=c), c

    def timed(f):
        t = time.perf_counter()
        f()
        return (time.perf_counter() - t) * 1e3

    for _ in range(3):
        single(four[2])
    if name == "single":
        print("  avk_merge_packed_counts alone:                  " + fmt([timed(lambda: single(four[2])) for _ in range(reps)]))
        ctx.close()
        return
    from aardvark_amd.merge import merge_multi_batch_sweep
    configs = four if name in ("four", "kernels") else [four[2]]

    def sweep():
        c = np.zeros((len(configs), n), np.uint64)
        return merge_multi_batch_sweep(ctx, pk, configs, counts=c), c

    got, blocks = sweep()
    ok = counts_on_device(ctx)
    for c, cfg in enumerate(configs):
        want, block = single(cfg)
        ok = ok and np.array_equal(got[c].status, want.status) and np.array_equal(got[c].classification, want.classification) and np.array_equal(got[c].members, want.members) and \
            np.array_equal(blocks[c], block)
    print("  the sweep's slices and blocks equal the single calls', counted by kernel: %s" % ok)
    if name == "kernels":
        for _ in range(5):
            sweep()
    else:
        a, b = [], []
        for _ in range(reps):  # the two forms in turn, so that neither has the warmer process
            a.append(timed(lambda: [single(cfg) for cfg in configs]))
            b.append(timed(sweep))
        print("  %d x avk_merge_packed_counts:                    " % len(configs) + fmt(a))
        print("  avk_merge_packed_sweep of %d:                    " % len(configs) + fmt(b))
    ctx.close()
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    scale = float(sys.argv[1]) if len(sys.argv) > 1 else 0.1
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 9
    if len(sys.argv) > 2 and sys.argv[2] != "all":
        leg(scale, sys.argv[2], reps)
    else:
        for name in ("four", "one", "single"):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), str(scale), name, str(reps)], timeout=900)
            if r.returncode != 0:  # (nothing more is started on the GPU behind a leg that failed)
                sys.exit(r.returncode)
