"""The merge summary counters by kernel against the host pass, on the 3-caller merge job of bench.py's merge leg (profiles/merge_counts_ab.txt).

usage: python tools/gpu_merge_counts_ab.py [SCALE=0.1] [leg]
  no leg: every leg below in a fresh process each, medians of five
  leg = host      avk_merge_counts_esc alone, on the results of one call
        calls     avk_merge_packed_esc followed by the host function, against avk_merge_packed_counts (pinned arrays, the forms alternating)
        plain     avk_merge_packed alone (AVK_LIB names the library: run it once per build to compare two builds under the same Python)
        kernel    five calls with counters and nothing else: the process to run under `rocprofv3 --kernel-trace --stats -- python tools/gpu_merge_counts_ab.py SCALE kernel`
The tool's stages are timed by the tool itself (`aardvark_amd_merge --summary-counts device|host`, its "stages [s]" line)."""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np


def median5(f):
    ts = []
    for _ in range(5):
        t = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts)), ts


def leg(scale, name):
    import aardvark_amd
    from aardvark_amd import synth
    from aardvark_amd.merge import MergeConfig, PackedMultiBatch, merge_counts, merge_counts_len, merge_multi_batch, pinned_multi_batch
    contigs, mb = synth.config_genome_merge(scale=scale, k=3, threads=8)
    ctx = aardvark_amd.Context(0)
    ctx.upload_reference(contigs)
    cfg = MergeConfig(majority_voting_enabled=True)
    pk = pinned_multi_batch(ctx, PackedMultiBatch.from_multi(mb))
    n = merge_counts_len(ctx.lib, 3)
    print("leg %s: scale %g, %d regions, %d calls, library %s" % (name, scale, pk.n_regions, pk.n_variants, os.environ.get("AVK_LIB", "libaardvark_amd.so")), flush=True)
    fmt = lambda m, ts: "%.2f ms (median of %s)" % (m, " ".join("%.2f" % t for t in ts))
    for _ in range(3):
        res = merge_multi_batch(ctx, pk, cfg)
    if name == "plain":
        print("  avk_merge_packed alone:                         " + fmt(*median5(lambda: merge_multi_batch(ctx, pk, cfg))))
    elif name == "host":
        print("  avk_merge_counts_esc alone (host):              " + fmt(*median5(lambda: merge_counts(ctx.lib, pk, res))))
    elif name == "kernel":
        counts = np.zeros(n, np.uint64)
        for _ in range(5):
            merge_multi_batch(ctx, pk, cfg, counts=counts)
    elif name == "calls":
        want = merge_counts(ctx.lib, pk, res)
        counts = np.zeros(n, np.uint64)
        merge_multi_batch(ctx, pk, cfg, counts=counts)
        from aardvark_amd.merge import counts_on_device
        print("  counters equal the host function's: %s; made by kernel: %s" % (np.array_equal(counts, want), counts_on_device(ctx)))
        a, b = [], []
        for _ in range(5):  # the two forms in turn, so that neither has the warmer process
            t = time.perf_counter(); r = merge_multi_batch(ctx, pk, cfg); merge_counts(ctx.lib, pk, r); a.append((time.perf_counter() - t) * 1e3)
            c = np.zeros(n, np.uint64)
            t = time.perf_counter(); merge_multi_batch(ctx, pk, cfg, counts=c); b.append((time.perf_counter() - t) * 1e3)
        print("  avk_merge_packed_esc + avk_merge_counts_esc:    " + fmt(float(np.median(a)), a))
        print("  avk_merge_packed_counts:                        " + fmt(float(np.median(b)), b))
    ctx.close()


if __name__ == "__main__":
    scale = float(sys.argv[1]) if len(sys.argv) > 1 else 0.1
    if len(sys.argv) > 2:
        leg(scale, sys.argv[2])
    else:
        for name in ("host", "calls", "plain"):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), str(scale), name], timeout=900)
            if r.returncode != 0:  # (nothing more is started on the GPU behind a leg that failed)
                sys.exit(r.returncode)
