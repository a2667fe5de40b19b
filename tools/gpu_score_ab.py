"""The curve by query score (avk_score_tallies: avk_score_hist_kernel, avk_score_curve_kernel) against the host route and against the plain packed call — the
figures of profiles/score_ab.txt.

    python tools/gpu_score_ab.py [--scale 1.0] [--runs 9] [--calls 3] [--parent-lib libaardvark_amd_parent.so] [--out profiles/score_ab.txt]
    python tools/gpu_score_ab.py --leg score        (one leg, in this process: what the driver starts, and what goes behind
                                                      `rocprofv3 --kernel-trace --stats -d <dir> -o trace --` for the kernels' own time, in a run of its own)

The driver runs every leg in a FRESH process under `timeout -k 10` (one GPU step per timeout), `--runs` times, the legs alternating, and stops at the first
abnormal exit; a leg's figure is the median over its rounds of `--calls` calls, the reported figure the median over the processes.  The job is the benchmark
genome (synth.config_genome at `scale`) as one packed batch, the scores synthetic (seeded, uniform over -5 .. 70 with one in twenty missing); the stage legs upload
and solve it once per process and time one stage on that resident batch — the copy of the scores into the pool included —, the call legs time whole calls; wall
clock around synchronous calls.

Legs (ms per call):
  step       avk_compare_resident + synchronize: the resident solver step                                         — for scale
  score      avk_score_tallies, default thresholds, scope 0: the stage
  score16    avk_score_tallies with a handle of 16 BED labels (label 0 every contig, the others 8 random intervals): 17 scopes, six launches, with the mask pass
  host       avk_score_tallies_host, default thresholds, 16 threads, on the same results downloaded (wide batch)
  plain      avk_compare_packed: the plain packed call
  onecall    avk_compare_packed_score: the plain call with the stage behind its download
  parent     the plain packed call on the library `--parent-lib` names (an in-tree build of the parent commit, loaded through AVK_LIB); left out without the option
The plain call must stay inside the +-5 % box-to-box band of DESIGN section 6 against the parent's: the driver says whether it did.  The stage's own time has no
target; the file records what was measured, with the library's source hash."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
LEGS = ("step", "score", "score16", "host", "plain", "onecall", "parent")


def run_leg(a):
    import numpy as np
    import aardvark_amd
    from aardvark_amd import CompactBatch, PackedBatch, ResultBatch, synth
    from gpu_context_strata_ab import bed_trees
    contigs, batch = synth.config_genome(scale=a.scale, threads=16)
    ctx = aardvark_amd.Context(0)
    ctx.upload_reference(contigs)
    out = dict(leg=a.leg, regions=int(batch.n_regions), source_hash=ctx.lib.avk_source_hash().decode())
    timed_new = a.leg in ("score", "score16", "host", "onecall")  # (the parent's library has no ScoreSpec entry points: its leg touches none)
    if timed_new:
        spec = aardvark_amd.ScoreSpec()
        rng = np.random.default_rng(1)
        scores = rng.uniform(-5.0, 70.0, batch.n_variants).astype(np.float32)  # (the compact and packed forms keep the wide batch's call order)
        scores[rng.random(batch.n_variants) < 0.05] = np.nan
        sums = np.zeros((17 if a.leg == "score16" else 1, spec.n_points, 13, 14), np.uint64)
    else:
        sums = np.zeros((1, 1, 13, 14), np.uint64)
    if a.leg == "host":
        res = ctx.solve_compare_regions(batch, group_metrics=False)

        def call():
            sums[...] = 0
            aardvark_amd.score_tallies_host(batch, res, spec, scores, threads=16, out=sums)
    elif a.leg in ("plain", "onecall", "parent"):
        pb = ctx.pinned_packed(PackedBatch.from_compact(CompactBatch.from_region_batch(batch)))
        res = ResultBatch(pb, sequences=False, group_metrics=False, packed="only")

        def call():
            sums[...] = 0
            if a.leg == "onecall":
                ctx.solve_packed(pb, res=res, score=spec, scores=scores, score_tallies=sums)
            else:
                ctx.solve_packed(pb, res=res)
    else:
        ctx.set_option("emit_group_metrics", 0)
        rb = ctx.upload(PackedBatch.from_compact(CompactBatch.from_region_batch(batch)))
        ctx.compare_resident(rb)
        ctx.synchronize()
        strata = ctx.upload_strata(*bed_trees(contigs, 16)) if a.leg == "score16" else None

        def call():
            sums[...] = 0
            if a.leg == "step":
                ctx.compare_resident(rb)
                ctx.synchronize()
            else:
                ctx.score_tallies(rb, spec, scores, strata=strata, out=sums)

    def round_of(calls):
        t0 = time.perf_counter()
        for _ in range(calls):
            call()
        return (time.perf_counter() - t0) * 1e3 / calls

    round_of(1)  # warm-up: device code, pools
    out["ms_per_call"] = statistics.median(round_of(a.calls) for _ in range(3))
    out["checksum"] = int(sums[0].sum() % (1 << 40))
    print("LEG " + json.dumps(out))
    ctx.close()


def drive(a):
    results = {}
    legs = [l for l in LEGS if l != "parent" or a.parent_lib]
    for run in range(a.runs):
        for leg in legs:
            cmd = ["timeout", "-k", "10", str(a.leg_timeout), sys.executable, os.path.abspath(__file__), "--leg", leg, "--scale", str(a.scale), "--calls", str(a.calls)]
            env = dict(os.environ, AVK_LIB=a.parent_lib) if leg == "parent" else None
            r = subprocess.run(cmd, capture_output=True, text=True, env=env)
            if r.returncode != 0:
                print("run %d, leg %s: exit %d — stopping here\n%s" % (run, leg, r.returncode, r.stderr[-2000:]))
                return 1
            got = json.loads([l for l in r.stdout.splitlines() if l.startswith("LEG ")][-1][4:])
            results.setdefault(leg, []).append(got)
            print("run %d: %s" % (run, json.dumps(got)), flush=True)
    if len(set(g["checksum"] for leg in ("score", "score16", "host", "onecall") for g in results[leg])) != 1:
        print("the device's and the host's blocks disagree")
        return 1
    med = lambda leg: statistics.median(g["ms_per_call"] for g in results[leg])
    first = results["step"][0]
    lines = ["Score curve: tools/gpu_score_ab.py --scale %g --runs %d --calls %d; medians of %d fresh processes, ms per call, %d regions, source hash %s"
             % (a.scale, a.runs, a.calls, a.runs, first["regions"], first["source_hash"])]
    for leg, what in (("step", "resident solver step (avk_compare_resident)"), ("score", "avk_score_tallies, default thresholds, scope 0"),
                      ("score16", "avk_score_tallies, default thresholds, 16 BED labels (17 scopes)"), ("host", "avk_score_tallies_host, default thresholds, 16 threads"),
                      ("plain", "plain packed call (avk_compare_packed)"), ("onecall", "avk_compare_packed_score"),
                      ("parent", "plain packed call, parent commit's library (source hash %s)" % (results["parent"][0]["source_hash"] if "parent" in results else ""))):
        if leg in results:
            lines.append("  %-74s %.3f" % (what, med(leg)))
    if "parent" in results:
        ratio = med("plain") / med("parent")
        lines.append("  plain / parent = %.4f: %s the +-5 %% band" % (ratio, "inside" if 0.95 <= ratio <= 1.05 else "OUTSIDE"))
    else:
        lines.append("  the plain call against the parent commit's build: not measured (no --parent-lib)")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=LEGS)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--leg-timeout", type=int, default=300)
    ap.add_argument("--parent-lib", default="", help="file name of an in-tree build of the parent commit's library, beside libaardvark_amd.so")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.leg:
        run_leg(a)
        return 0
    return drive(a)


if __name__ == "__main__":
    sys.exit(main())
