"""Bootstrap replicates of the per-call blocks (avk_kind_boot_tallies, avk_size_boot_tallies: avk_callboot_tally_kernel) against their host routes and against
the plain packed call — the figures of profiles/callboot_ab.txt.

    python tools/gpu_callboot_ab.py --legs kind100,size100 [--scale 1.0] [--runs 9] [--calls 1] --json stage.json    (one thing timed per invocation: the legs named)
    python tools/gpu_callboot_ab.py --legs plain,parent --parent-lib libaardvark_amd_parent.so --json ab.json          (the A/B: the two legs alternate)
    python tools/gpu_callboot_ab.py --report stage.json host.json ab.json --out profiles/callboot_ab.txt
    python tools/gpu_callboot_ab.py --leg kind100         (one leg, in this process: what the driver starts)

The driver runs every leg in a FRESH process under `timeout -k 10` (one GPU step per timeout), `--runs` times, the legs named alternating, and stops at the first
abnormal exit; a leg's figure is the median over its rounds of `--calls` calls, the reported figure the median over the processes.  The job is the benchmark
genome (synth.config_genome at `scale`) as one packed batch; the stage legs upload and solve it once per process and time one stage on that resident batch.

Legs (ms per call) are named <family><B>[_16][_host]: family kind or size (the default spec), B = 100 or 1000 replicates (the tool has no default count; 1000 is
the usual one), _16 a handle of 16 BED labels (17 scopes), _host the host route on 16 threads on the same results; plain / parent: the plain packed call on this
library and on the library `--parent-lib` names.  A leg that was not run is reported as "not measured".  No stage time is compared with a bound; the one bound is
the plain packed call's: inside +-5 % of the parent library's, else the report returns 1."""
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
LEGS = tuple(f + B + l + h for f in ("kind", "size") for B in ("100", "1000") for l in ("", "_16") for h in ("", "_host")) + ("plain", "parent")


def what_of(leg):
    if leg in ("plain", "parent"):
        return "plain packed call (avk_compare_packed)" + (", parent commit's library" if leg == "parent" else "")
    family, B = leg[:4], int(leg[4:].split("_")[0])
    return "avk_%s_boot_tallies%s, B = %d, %s" % (family, "_host (16 threads)" if leg.endswith("_host") else "", B, "16 BED labels (17 scopes)" if "_16" in leg else "scope 0")


def run_leg(a):
    import numpy as np
    import aardvark_amd
    from aardvark_amd import BootSpec, CompactBatch, PackedBatch, ResultBatch, SizeSpec, synth
    from gpu_context_strata_ab import bed_trees
    contigs, batch = synth.config_genome(scale=a.scale, threads=16)
    ctx = aardvark_amd.Context(0)
    ctx.upload_reference(contigs)
    out = dict(leg=a.leg, regions=int(batch.n_regions), source_hash=ctx.lib.avk_source_hash().decode())
    if a.leg in ("plain", "parent"):
        pb = ctx.pinned_packed(PackedBatch.from_compact(CompactBatch.from_region_batch(batch)))
        res = ResultBatch(pb, sequences=False, group_metrics=False, packed="only")
        sums = np.zeros(1, np.uint64)

        def call():
            ctx.solve_packed(pb, res=res)
    else:
        family, B, labels, host = a.leg[:4], int(a.leg[4:].split("_")[0]), "_16" in a.leg, a.leg.endswith("_host")
        boot, spec = BootSpec(B, 1), SizeSpec()
        K = 9 if family == "kind" else spec.n_bins
        sums = np.zeros((17 if labels else 1, B, K, 13, 14), np.uint64)
        out["R"] = ctx.callboot_block(K)
        ctx.set_option("emit_group_metrics", 0)
        rb = ctx.upload(PackedBatch.from_compact(CompactBatch.from_region_batch(batch)))
        ctx.compare_resident(rb)
        ctx.synchronize()
        strata = ctx.upload_strata(*bed_trees(contigs, 16)) if labels else None
        if host:
            res = ctx.solve_compare_regions(batch, group_metrics=False)
            lists = None
            if labels:
                off, idx = ctx.strata_region_labels(rb, strata)
                lists = (16, off, idx)

            def call():
                sums[...] = 0
                if family == "kind":
                    aardvark_amd.kind_boot_tallies_host(batch, res, boot, labels=lists, threads=16, out=sums)
                else:
                    aardvark_amd.size_boot_tallies_host(batch, res, spec, boot, labels=lists, threads=16, out=sums)
        else:
            def call():
                sums[...] = 0
                if family == "kind":
                    ctx.kind_boot_tallies(rb, boot, strata=strata, out=sums)
                else:
                    ctx.size_boot_tallies(rb, spec, boot, strata=strata, out=sums)

    def round_of(calls):
        t0 = time.perf_counter()
        for _ in range(calls):
            call()
        return (time.perf_counter() - t0) * 1e3 / calls

    round_of(1)  # warm-up: device code, pools
    out["ms_per_call"] = statistics.median(round_of(a.calls) for _ in range(3))
    out["checksum"] = int(sums.sum() % (1 << 40))
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
    for leg in LEGS:  # the device's and the host's blocks of the same job agree
        if leg + "_host" in results and leg in results and set(g["checksum"] for g in results[leg]) != set(g["checksum"] for g in results[leg + "_host"]):
            print("the device's and the host's blocks disagree: " + leg)
            return 1
    med = lambda leg: statistics.median(g["ms_per_call"] for g in results[leg])
    inside = True
    first = next(iter(results.values()))[0]
    lines = ["Per-call bootstrap: tools/gpu_callboot_ab.py --scale %g --calls %d; medians of fresh processes, ms per call, %d regions, source hash %s"
             % (head["scale"], head["calls"], first["regions"], first["source_hash"])]
    for leg in LEGS:
        if leg in results:
            extra = " (source hash %s)" % results[leg][0]["source_hash"] if leg == "parent" else " (R = %d)" % results[leg][0]["R"] if "R" in results[leg][0] and not leg.endswith("_host") else ""
            lines.append("  %-74s %.3f   (%d processes)" % (what_of(leg) + extra, med(leg), len(results[leg])))
        else:
            lines.append("  %-74s not measured" % what_of(leg))
    if "plain" in results and "parent" in results:
        rel = 100.0 * (med("plain") / med("parent") - 1.0)
        inside = abs(rel) <= 5.0
        lines.append("  plain / parent: %+.1f %%: %s +-5 %%" % (rel, "inside" if inside else "OUTSIDE"))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 0 if inside else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=LEGS)
    ap.add_argument("--legs", default="kind100")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--calls", type=int, default=1)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--leg-timeout", type=int, default=600)
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
