"""Bootstrap replicates of the tallies (avk_boot_tallies, avk_boot_tally_kernel) against the host route and against the stages they run beside — the figures of
profiles/boot_ab.txt.

    python tools/gpu_boot_ab.py [--scale 1.0] [--runs 9] [--calls 3] [--out profiles/boot_ab.txt]
    python tools/gpu_boot_ab.py --leg boot1000        (one leg, in this process: what the driver starts, and what goes behind
                                                        `rocprofv3 --kernel-trace --stats -d <dir> -o trace --` for the kernel's own time, in a run of its own)

The driver runs every leg in a FRESH process under `timeout -k 10` (one GPU step per timeout), `--runs` times, the legs alternating, and stops at the first
abnormal exit; a leg's figure is the median over its rounds of `--calls` calls, the reported figure the median over the processes.  The job is the benchmark
genome (synth.config_genome at `scale`) as one packed batch, uploaded and solved once per process with emit_bp_groups; a leg times one stage on that resident
batch, wall clock around synchronous calls.

Legs (ms per call):
  step       avk_compare_resident + synchronize: the resident solver step                                  — for scale
  labels     avk_label_tallies_strata, 16 BED labels (label 0 every contig, the others 8 random intervals)  — the label kernel, for scale
  boot100    avk_boot_tallies, 100 replicates, scope 0
  boot1000   avk_boot_tallies, 1000 replicates, scope 0
  host100    avk_boot_tallies_host, 100 replicates, 16 threads, on the same results downloaded (wide batch, compact BASEPAIR groups)
  host1000   the same with 1000 replicates
Nothing is compared with a bound: no time was fixed for this feature, the file records what was measured, with the library's source hash."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
LEGS = ("step", "labels", "boot100", "boot1000", "host100", "host1000")


def run_leg(a):
    import numpy as np
    import aardvark_amd
    from aardvark_amd import BootSpec, CompactBatch, PackedBatch, _abi, synth
    from gpu_context_strata_ab import bed_trees
    contigs, batch = synth.config_genome(scale=a.scale, threads=16)
    ctx = aardvark_amd.Context(0)
    ctx.upload_reference(contigs)
    out = dict(leg=a.leg, regions=int(batch.n_regions), source_hash=ctx.lib.avk_source_hash().decode())
    if a.leg.startswith("host"):
        B = int(a.leg[4:])
        res = ctx.solve_compare_regions(batch, group_metrics=False, bp_groups=True)
        cb, ro, spec = batch.c_struct(), res.c_struct(), _abi.AvkBootSpec(B, 1)
        sums = np.zeros((1, B, _abi.TALLY_LEN), np.uint64)

        def call():
            sums[...] = 0
            ctx._check(ctx.lib.avk_boot_tallies_host(C.byref(cb), C.byref(ro), C.byref(spec), None, 16, sums.ctypes.data_as(C.POINTER(C.c_uint64))))
    else:
        ctx.set_option("emit_group_metrics", 0)
        ctx.set_option("emit_bp_groups", 1)
        rb = ctx.upload(PackedBatch.from_compact(CompactBatch.from_region_batch(batch)))
        ctx.compare_resident(rb)
        ctx.synchronize()
        strata = ctx.upload_strata(*bed_trees(contigs, 16)) if a.leg == "labels" else None
        B = int(a.leg[4:]) if a.leg.startswith("boot") else 1
        sums = np.zeros((16, _abi.TALLY_LEN) if a.leg == "labels" else (1, B, _abi.TALLY_LEN), np.uint64)

        def call():
            sums[...] = 0
            if a.leg == "step":
                ctx.compare_resident(rb)
                ctx.synchronize()
            elif a.leg == "labels":
                ctx.label_tallies_strata(rb, strata, out=sums)
            else:
                ctx.boot_tallies(rb, BootSpec(B, 1), out=sums)

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
    for run in range(a.runs):
        for leg in LEGS:
            cmd = ["timeout", "-k", "10", str(a.leg_timeout), sys.executable, os.path.abspath(__file__), "--leg", leg, "--scale", str(a.scale), "--calls", str(a.calls)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                print("run %d, leg %s: exit %d — stopping here\n%s" % (run, leg, r.returncode, r.stderr[-2000:]))
                return 1
            got = json.loads([l for l in r.stdout.splitlines() if l.startswith("LEG ")][-1][4:])
            results.setdefault(leg, []).append(got)
            print("run %d: %s" % (run, json.dumps(got)), flush=True)
    for b in ("100", "1000"):
        if len(set(g["checksum"] for leg in ("boot" + b, "host" + b) for g in results[leg])) != 1:
            print("the device's and the host's replicates disagree at B = " + b)
            return 1
    med = lambda leg: statistics.median(g["ms_per_call"] for g in results[leg])
    first = results["step"][0]
    lines = ["Bootstrap replicates: tools/gpu_boot_ab.py --scale %g --runs %d --calls %d; medians of %d fresh processes, ms per call, %d regions, source hash %s"
             % (a.scale, a.runs, a.calls, a.runs, first["regions"], first["source_hash"])]
    for leg, what in (("step", "resident solver step (avk_compare_resident)"), ("labels", "label kernel, 16 BED labels (avk_label_tallies_strata)"),
                      ("boot100", "avk_boot_tallies, B = 100, scope 0"), ("boot1000", "avk_boot_tallies, B = 1000, scope 0"),
                      ("host100", "avk_boot_tallies_host, B = 100, 16 threads"), ("host1000", "avk_boot_tallies_host, B = 1000, 16 threads")):
        lines.append("  %-58s %.3f" % (what, med(leg)))
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
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.leg:
        run_leg(a)
        return 0
    return drive(a)


if __name__ == "__main__":
    sys.exit(main())
