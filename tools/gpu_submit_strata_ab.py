"""Stratified batches IN FLIGHT (avk_compare_packed_submit_strata -> avk_wait) against the other ways to get the same per-label sums — the figures of
profiles/submit_strata_ab.txt.

    python tools/gpu_submit_strata_ab.py [--scale 0.1] [--runs 5] [--batches 8] [--parent-lib libaardvark_amd_parent.so] [--out profiles/submit_strata_ab.txt]
    python tools/gpu_submit_strata_ab.py --leg submit_strata --labels 300        (one leg, in this process: what the driver starts, and what goes behind
                                                                                   `rocprofv3 --kernel-trace --stats -d <dir> -o trace --` for part (b))

The driver runs every leg in a FRESH process under `timeout -k 10`, `--runs` times per label count (20 and 300), the legs alternating, and stops at the first
abnormal exit; a leg's figure is the median over its batches, the reported figure the median over the processes.  The job is that of tools/gpu_strata_ab.py
(profiles/strata_device_ab.txt): synth.config_genome at `scale` as one pinned packed batch, label 0 on every contig, the others 8 random intervals a contig.

Legs (ms per batch, wall around `--batches` batches that end in the last wait):
  submit_strata   two tickets in flight through avk_compare_packed_submit_strata                                                     (a)
  one_call        back-to-back avk_compare_packed_strata calls                                                                        (a)
  submit_labels   two tickets in flight through avk_compare_packed_submit_labels, host-made pinned lists; list-making timed apart      (a)
  plain           two unlabelled tickets in flight (label count ignored); with --parent-lib also under AVK_LIB=<that library>           (c)
Every leg prints a checksum of its sums; the driver refuses a run whose labelled legs disagree.  Peak pool bytes per ticket are computed from the shapes: the
mask route holds ceil(labels / 32) * 4 B a region, the list route 8 B a region + 4 B a list entry (the one-call form) or the same in its staging slot (submit_labels)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LEGS = ("submit_strata", "one_call", "submit_labels", "plain")


def make_job(scale, labels):
    import numpy as np
    from aardvark_amd import feeder, synth
    contigs, batch = synth.config_genome(scale=scale, threads=16)
    names = ["c%02d" % i for i in range(len(contigs))]
    folder = tempfile.mkdtemp(prefix="submit_strata_ab_")
    with open(os.path.join(folder, "g.fa"), "w") as f:  # (the lists never read a base: the contigs only have to exist by name)
        f.write("".join(">%s\nACGT\n" % n for n in names))
    rng = np.random.default_rng(5)
    rows = []
    for l in range(labels):
        with open(os.path.join(folder, "l%03d.bed" % l), "w") as f:
            for c, name in enumerate(names):
                size = len(contigs[c])
                if l == 0:
                    f.write("%s\t0\t%d\n" % (name, size))
                    continue
                s, w = rng.integers(0, size, 8), rng.integers(size // 200 + 1, size // 12 + 2, 8)
                f.write("".join("%s\t%d\t%d\n" % (name, int(x), int(x + y)) for x, y in sorted(zip(s, w))))
        rows.append("l%03d\tl%03d.bed\n" % (l, l))
    with open(os.path.join(folder, "strat.tsv"), "w") as f:
        f.write("".join(rows))
    return contigs, batch, feeder.Genome(os.path.join(folder, "g.fa")), feeder.Stratifications(os.path.join(folder, "strat.tsv"))


def run_leg(a):
    import numpy as np
    import aardvark_amd
    from aardvark_amd import CompactBatch, PackedBatch
    contigs, batch, genome, strat = make_job(a.scale, a.labels)
    ctx = aardvark_amd.Context(0)
    ctx.upload_reference(contigs)
    pb = ctx.pinned_packed(PackedBatch.from_compact(CompactBatch.from_region_batch(batch)))
    res = [ctx.pinned_results(pb, packed="only") for _ in range(2)]
    out = dict(leg=a.leg, labels=a.labels, regions=int(batch.n_regions), lib=os.environ.get("AVK_LIB", ""))
    strata = ctx.upload_strata(*strat.export(genome)) if a.leg in ("submit_strata", "one_call") else None
    lists = None
    if a.leg == "submit_labels":
        t0 = time.perf_counter()
        off, idx = strat.batch_labels(genome, batch)
        out["lists_ms"] = (time.perf_counter() - t0) * 1e3
        poff, pidx = ctx.host_array(off.shape, np.uint64), ctx.host_array(idx.shape, np.uint32)
        poff[...], pidx[...] = off, idx
        lists = (a.labels, poff, pidx)
        out["list_entries"] = int(len(idx))
    sums = np.zeros((a.labels, aardvark_amd._abi.TALLY_LEN), np.uint64)

    def round_of(batches):
        sums[...] = 0
        t0 = time.perf_counter()
        if a.leg == "one_call":
            for _ in range(batches):
                ctx.solve_packed(pb, res=res[0], strata=strata, label_tallies=sums)
        else:
            kw = dict(strata=strata, label_tallies=sums) if a.leg == "submit_strata" else dict(labels=lists, label_tallies=sums) if a.leg == "submit_labels" else {}
            flying = []
            for k in range(batches):
                if len(flying) == 2:
                    flying.pop(0).wait()
                flying.append(ctx.submit_packed(pb, res=res[k % 2], **kw))
            for t in flying:
                t.wait()
        return (time.perf_counter() - t0) * 1e3 / batches

    round_of(2)  # warm-up: device code, pools, staging slots
    per = [round_of(a.batches) for _ in range(3)]
    out["ms_per_batch"] = statistics.median(per)
    out["checksum"] = int(sums.sum() % (1 << 40)) if a.leg != "plain" else 0
    words = (a.labels + 31) // 32
    out["mask_bytes_per_ticket"] = int(batch.n_regions) * words * 4
    print("LEG " + json.dumps(out))
    if strata is not None:
        strata.free()
    ctx.close()


def drive(a):
    results, lines = {}, []
    plan = [(leg, labels, "") for labels in (20, 300) for leg in LEGS if leg != "plain"] + [("plain", 20, "")]
    if a.parent_lib:
        plan.append(("plain", 20, a.parent_lib))
    for run in range(a.runs):
        for leg, labels, lib in plan:
            cmd = ["timeout", "-k", "10", str(a.leg_timeout), sys.executable, os.path.abspath(__file__), "--leg", leg, "--labels", str(labels), "--scale", str(a.scale),
                   "--batches", str(a.batches)]
            env = dict(os.environ)
            if lib:
                env["AVK_LIB"] = lib
            r = subprocess.run(cmd, capture_output=True, text=True, env=env)
            if r.returncode != 0:
                print("run %d, leg %s (%d labels%s): exit %d — stopping here\n%s" % (run, leg, labels, ", " + lib if lib else "", r.returncode, r.stderr[-2000:]))
                return 1
            got = json.loads([l for l in r.stdout.splitlines() if l.startswith("LEG ")][-1][4:])
            results.setdefault((leg, labels, lib), []).append(got)
            print("run %d: %s" % (run, json.dumps(got)), flush=True)
    for labels in (20, 300):
        sums = set(g["checksum"] for (leg, l, lib), gs in results.items() if l == labels and leg != "plain" for g in gs)
        if len(sums) != 1:
            print("the labelled legs disagree at %d labels: checksums %s" % (labels, sorted(sums)))
            return 1
    med = lambda key, f: statistics.median(g[f] for g in results[key])
    lines.append("Stratified batches in flight: tools/gpu_submit_strata_ab.py --scale %g --runs %d --batches %d; medians of %d fresh processes, ms per batch" % (a.scale, a.runs, a.batches, a.runs))
    for labels in (20, 300):
        one = results[("submit_labels", labels, "")][0]
        lines.append("  %3d labels (%d regions): submit_strata, two in flight %.2f | back-to-back avk_compare_packed_strata %.2f | submit_labels, two in flight %.2f (+ host lists %.1f ms a batch, made apart)"
                     % (labels, one["regions"], med(("submit_strata", labels, ""), "ms_per_batch"), med(("one_call", labels, ""), "ms_per_batch"),
                        med(("submit_labels", labels, ""), "ms_per_batch"), med(("submit_labels", labels, ""), "lists_ms")))
        lines.append("      pool bytes per ticket: masks %.1f MB; lists %.1f MB (8 B a region + 4 B an entry, %d entries)"
                     % (one["mask_bytes_per_ticket"] / 1e6, (8 * (one["regions"] + 1) + 4 * one["list_entries"]) / 1e6, one["list_entries"]))
    lines.append("  unlabelled, two in flight: this library %.2f" % med(("plain", 20, ""), "ms_per_batch") +
                 ("; parent library %.2f" % med(("plain", 20, a.parent_lib), "ms_per_batch") if a.parent_lib else ""))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=LEGS)
    ap.add_argument("--labels", type=int, default=20)
    ap.add_argument("--scale", type=float, default=0.1)
    ap.add_argument("--batches", type=int, default=8)
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
