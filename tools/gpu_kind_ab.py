"""Per-call tallies by call kind (avk_kind_tallies, avk_kind_tally_kernel) against the host route and against the plain packed call — the figures of
profiles/kind_ab.txt.

    python tools/gpu_kind_ab.py --legs kind [--scale 1.0] [--runs 9] [--calls 3] --json kind.json      (one thing timed per invocation: the legs named)
    python tools/gpu_kind_ab.py --legs plain,parent --parent-lib libaardvark_amd_parent.so --json ab.json   (the A/B: the two legs alternate)
    python tools/gpu_kind_ab.py --report kind.json kind16.json host.json ab.json --out profiles/kind_ab.txt
    python tools/gpu_kind_ab.py --leg kind          (one leg, in this process: what the driver starts)

The driver runs every leg in a FRESH process under `timeout -k 10` (one GPU step per timeout), `--runs` times, the legs named alternating, and stops at the first
abnormal exit; a leg's figure is the median over its rounds of `--calls` calls, the reported figure the median over the processes.  The job is the benchmark
genome (synth.config_genome at `scale`) as one packed batch; the stage legs upload and solve it once per process and time one stage on that resident batch, the
call legs time whole calls; wall clock around synchronous calls.

Legs (ms per call):
  kind       avk_kind_tallies, scope 0: the stage
  kind16     avk_kind_tallies with a handle of 16 BED labels (label 0 every contig, the others 8 random intervals): 17 scopes, six launches, with the mask pass
  size       avk_size_tallies, default spec, scope 0: the neighbouring stage, for scale
  host       avk_kind_tallies_host, 16 threads, on the same results downloaded (wide batch)
  plain      avk_compare_packed: the plain packed call
  onecall    avk_compare_packed_kind: the plain call with the stage behind its download
  parent     the plain packed call on the library `--parent-lib` names (an in-tree build of the parent commit, loaded through AVK_LIB)
No stage time is compared with a bound: none was fixed for this feature, the file records what was measured, with the library's source hash.  The one bound is
the plain packed call's: the report says whether its median stayed inside +-5 % of the parent library's (this pool's box-to-box resolution), and returns 1 if not."""
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
LEGS = ("kind", "kind16", "size", "host", "plain", "onecall", "parent")
WHAT = {"kind": "avk_kind_tallies, scope 0", "kind16": "avk_kind_tallies, 16 BED labels (17 scopes)", "size": "avk_size_tallies, default spec, scope 0",
        "host": "avk_kind_tallies_host, 16 threads", "plain": "plain packed call (avk_compare_packed)", "onecall": "avk_compare_packed_kind",
        "parent": "plain packed call, parent commit's library"}


def run_leg(a):
    import numpy as np
    import aardvark_amd
    from aardvark_amd import CompactBatch, PackedBatch, ResultBatch, SizeSpec, synth
    from gpu_context_strata_ab import bed_trees
    contigs, batch = synth.config_genome(scale=a.scale, threads=16)
    ctx = aardvark_amd.Context(0)
    ctx.upload_reference(contigs)
    out = dict(leg=a.leg, regions=int(batch.n_regions), source_hash=ctx.lib.avk_source_hash().decode())
    sums = np.zeros((17 if a.leg == "kind16" else 1, 5 if a.leg == "size" else 9, 13, 14), np.uint64)
    if a.leg == "host":
        res = ctx.solve_compare_regions(batch, group_metrics=False)

        def call():
            sums[...] = 0
            aardvark_amd.kind_tallies_host(batch, res, threads=16, out=sums)
    elif a.leg in ("plain", "onecall", "parent"):
        pb = ctx.pinned_packed(PackedBatch.from_compact(CompactBatch.from_region_batch(batch)))
        res = ResultBatch(pb, sequences=False, group_metrics=False, packed="only")

        def call():
            sums[...] = 0
            if a.leg == "onecall":
                ctx.solve_packed(pb, res=res, kinds=True, kind_tallies=sums)
            else:
                ctx.solve_packed(pb, res=res)
    else:
        ctx.set_option("emit_group_metrics", 0)
        rb = ctx.upload(PackedBatch.from_compact(CompactBatch.from_region_batch(batch)))
        ctx.compare_resident(rb)
        ctx.synchronize()
        strata = ctx.upload_strata(*bed_trees(contigs, 16)) if a.leg == "kind16" else None

        def call():
            sums[...] = 0
            if a.leg == "size":
                ctx.size_tallies(rb, SizeSpec(), out=sums)
            else:
                ctx.kind_tallies(rb, strata=strata, out=sums)

    def round_of(calls):
        t0 = time.perf_counter()
        for _ in range(calls):
            call()
        return (time.perf_counter() - t0) * 1e3 / calls

    round_of(1)  # warm-up: device code, pools
    out["ms_per_call"] = statistics.median(round_of(a.calls) for _ in range(3))
    out["checksum"] = int(sums[0].sum() % (1 << 40))
    if a.leg in ("kind", "kind16", "host", "onecall"):  # Ti/Tv and het/hom of the truth calls, for the record
        t = sums[0, :, 0, 0] + sums[0, :, 0, 1]
        out["truth_ti_tv"] = [int(t[0::3].sum()), int(t[1::3].sum())]
        out["truth_het_hom"] = [int(t[0:3].sum()), int(t[3:6].sum())]
    print("LEG " + json.dumps(out))
    ctx.close()


def drive(a):
    results = {}
    legs = [l for l in a.legs.split(",") if l]
    if any(l not in LEGS for l in legs) or ("parent" in legs and not a.parent_lib):
        print("unknown leg, or the parent leg without --parent-lib")
        return 2
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
            if a.json:  # (kept after every process: a run that is cut short leaves what it measured)
                with open(a.json, "w") as f:
                    json.dump(dict(scale=a.scale, runs=a.runs, calls=a.calls, results=results), f)
    return 0


def report(a):
    results, head = {}, None
    for path in a.report:
        d = json.load(open(path))
        head = head or d
        for leg, got in d["results"].items():
            results.setdefault(leg, []).extend(got)
    sums = set(g["checksum"] for leg in ("kind", "kind16", "host", "onecall") for g in results.get(leg, []))
    if len(sums) > 1:
        print("the device's and the host's blocks disagree")
        return 1
    med = lambda leg: statistics.median(g["ms_per_call"] for g in results[leg])
    inside = True
    first = next(iter(results.values()))[0]
    lines = ["Call-kind tallies: tools/gpu_kind_ab.py --scale %g --calls %d, one invocation per line group; medians of fresh processes, ms per call, %d regions, source hash %s"
             % (head["scale"], head["calls"], first["regions"], first["source_hash"])]
    for leg in LEGS:
        if leg in results:
            what = WHAT[leg] + (" (source hash %s)" % results[leg][0]["source_hash"] if leg == "parent" else "")
            lines.append("  %-74s %.3f   (%d processes)" % (what, med(leg), len(results[leg])))
    if "plain" in results and "parent" in results:
        rel = 100.0 * (med("plain") / med("parent") - 1.0)
        inside = abs(rel) <= 5.0
        lines.append("  plain / parent: %+.1f %%: %s +-5 %%" % (rel, "inside" if inside else "OUTSIDE"))
    for leg in ("kind", "onecall", "host"):
        if leg in results and "truth_ti_tv" in results[leg][0]:
            g = results[leg][0]
            lines.append("  truth calls of the genome: ti %d, tv %d; het %d, hom_alt %d" % tuple(g["truth_ti_tv"] + g["truth_het_hom"]))
            break
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 0 if inside else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=LEGS)
    ap.add_argument("--legs", default="kind")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--leg-timeout", type=int, default=300)
    ap.add_argument("--parent-lib", default="", help="file name of an in-tree build of the parent commit's library, beside libaardvark_amd.so")
    ap.add_argument("--json", default="", help="where the driver keeps what it measured")
    ap.add_argument("--report", nargs="+", help="files the driver kept: write the figures")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.leg:
        run_leg(a)
        return 0
    if a.report:
        return report(a)
    return drive(a)


if __name__ == "__main__":
    sys.exit(main())
