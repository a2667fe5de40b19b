"""Sequence-context labels (avk_strata_upload_context, avk_context_mask_kernel) against the calls they must leave alone and against BED labels — the figures
of profiles/context_strata_ab.txt.

    python tools/gpu_context_strata_ab.py [--scale 0.1] [--runs 5] [--calls 8] [--parent-lib libaardvark_amd_parent.so] [--out profiles/context_strata_ab.txt]
    python tools/gpu_context_strata_ab.py --leg context        (one leg, in this process: what the driver starts, and what goes behind
                                                                 `rocprofv3 --kernel-trace --stats -d <dir> -o trace --` for the kernels' own times, in a run of its own)

The driver runs every leg in a FRESH process under `timeout -k 10` (one GPU step per timeout), `--runs` times, the legs alternating, and stops at the first
abnormal exit; a leg's figure is the median over its rounds of `--calls` calls, the reported figure the median over the processes.  The job is that of
tools/gpu_strata_ab.py (profiles/strata_device_ab.txt): synth.config_genome at `scale` as one pinned packed batch.

Legs (ms per call, wall around back-to-back synchronous calls):
  plain      avk_compare_packed, no labels                                           — also under AVK_LIB=<--parent-lib>: must be unchanged
  bed16      avk_compare_packed_strata with 16 BED labels (label 0 every contig, the others 8 random intervals a contig)   — also under the parent: must be unchanged
  context    avk_compare_packed_strata with the 16 default context labels alone (12 GC bins, 4 homopolymer classes)         — recorded only
  bed_ctx    the 16 BED labels and the 16 context labels in one handle                                                      — recorded only
"Unchanged": this library's median inside ±5 % (DESIGN §6's box-to-box noise) of the parent library's; the driver prints the ratio and says which side of the
margin it is on — it does not move the margin."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LEGS = ("plain", "bed16", "context", "bed_ctx")
N_BED = 16


def bed_trees(contigs, labels):
    """the interval sets as avk_strata_upload takes them: label 0 holds every contig whole, the others 8 random intervals a contig"""
    import numpy as np
    rng = np.random.default_rng(5)
    tree_off, start, end_max = [0], [], []
    for l in range(labels):
        for c in contigs:
            size = len(c)
            if l == 0:
                s, e = np.zeros(1, np.int64), np.full(1, size, np.int64)
            else:
                s = np.sort(rng.integers(0, size, 8))
                e = np.minimum(s + rng.integers(size // 200 + 1, size // 12 + 2, 8), 2**32 - 1)
            start += s.tolist()
            end_max += np.maximum.accumulate(e).tolist()
            tree_off.append(len(start))
    return labels, len(contigs), np.array(tree_off, np.uint64), np.array(start, np.uint32), np.array(end_max, np.uint32)


def run_leg(a):
    import numpy as np
    import aardvark_amd
    from aardvark_amd import CompactBatch, PackedBatch, synth
    contigs, batch = synth.config_genome(scale=a.scale, threads=16)
    ctx = aardvark_amd.Context(0)
    ctx.upload_reference(contigs)
    pb = ctx.pinned_packed(PackedBatch.from_compact(CompactBatch.from_region_batch(batch)))
    res = ctx.pinned_results(pb, packed="only")
    out = dict(leg=a.leg, regions=int(batch.n_regions), lib=os.environ.get("AVK_LIB", ""))
    strata = None
    if a.leg == "bed16":
        strata = ctx.upload_strata(*bed_trees(contigs, N_BED))
    elif a.leg == "context":
        strata = ctx.upload_strata(0, len(contigs), np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint32), context=aardvark_amd.ContextSpec())
    elif a.leg == "bed_ctx":
        strata = ctx.upload_strata(*bed_trees(contigs, N_BED), context=aardvark_amd.ContextSpec())
    sums = np.zeros((strata.n_labels if strata else 0, aardvark_amd._abi.TALLY_LEN), np.uint64)

    def round_of(calls):
        sums[...] = 0
        t0 = time.perf_counter()
        for _ in range(calls):
            if strata is None:
                ctx.solve_packed(pb, res=res)
            else:
                ctx.solve_packed(pb, res=res, strata=strata, label_tallies=sums)
        return (time.perf_counter() - t0) * 1e3 / calls

    round_of(2)  # warm-up: device code, pools
    out["ms_per_call"] = statistics.median(round_of(a.calls) for _ in range(3))
    out["labels"] = int(sums.shape[0])
    out["checksum"] = int(sums.sum() % (1 << 40))
    print("LEG " + json.dumps(out))
    if strata is not None:
        strata.free()
    ctx.close()


def drive(a):
    results = {}
    plan = [(leg, "") for leg in LEGS]
    if a.parent_lib:
        plan += [("plain", a.parent_lib), ("bed16", a.parent_lib)]
    for run in range(a.runs):
        for leg, lib in plan:
            cmd = ["timeout", "-k", "10", str(a.leg_timeout), sys.executable, os.path.abspath(__file__), "--leg", leg, "--scale", str(a.scale), "--calls", str(a.calls)]
            env = dict(os.environ)
            if lib:
                env["AVK_LIB"] = lib
            r = subprocess.run(cmd, capture_output=True, text=True, env=env)
            if r.returncode != 0:
                print("run %d, leg %s%s: exit %d — stopping here\n%s" % (run, leg, ", " + lib if lib else "", r.returncode, r.stderr[-2000:]))
                return 1
            got = json.loads([l for l in r.stdout.splitlines() if l.startswith("LEG ")][-1][4:])
            results.setdefault((leg, lib), []).append(got)
            print("run %d: %s" % (run, json.dumps(got)), flush=True)
    if a.parent_lib and len(set(g["checksum"] for lib in ("", a.parent_lib) for g in results[("bed16", lib)])) != 1:
        print("the BED-only sums of the two libraries disagree")
        return 1
    med = lambda key: statistics.median(g["ms_per_call"] for g in results[key])
    lines = ["Sequence-context labels: tools/gpu_context_strata_ab.py --scale %g --runs %d --calls %d; medians of %d fresh processes, ms per synchronous call, %d regions"
             % (a.scale, a.runs, a.calls, a.runs, results[("plain", "")][0]["regions"])]
    for leg, what in (("plain", "unlabelled avk_compare_packed"), ("bed16", "avk_compare_packed_strata, 16 BED labels")):
        line = "  %-42s this library %.3f" % (what, med((leg, "")))
        if a.parent_lib:
            ratio = med((leg, "")) / med((leg, a.parent_lib))
            line += " | parent library %.3f | ratio %.3f: %s the +-5 %% of DESIGN section 6" % (med((leg, a.parent_lib)), ratio, "inside" if 0.95 <= ratio <= 1.05 else "OUTSIDE")
        lines.append(line)
    lines.append("  %-42s this library %.3f   (recorded only)" % ("avk_compare_packed_strata, 16 context labels", med(("context", ""))))
    lines.append("  %-42s this library %.3f   (recorded only)" % ("... 16 BED + 16 context labels, one handle", med(("bed_ctx", ""))))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=LEGS)
    ap.add_argument("--scale", type=float, default=0.1)
    ap.add_argument("--calls", type=int, default=8)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--leg-timeout", type=int, default=120)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.leg:
        run_leg(a)
        return 0
    return drive(a)


if __name__ == "__main__":
    sys.exit(main())
