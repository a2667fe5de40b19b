"""Stratified packed call: region -> label lists made on the device (avk_compare_packed_strata) against lists made by the host (avf_strat_batch_labels, then
avk_compare_packed_labels), in one process and one library — the figures of profiles/strata_device_ab.txt.

    python tools/gpu_strata_ab.py --labels 20 [--scale 0.1] [--jobs 3]

The job is the synthetic genome of bench.py (synth.config_genome) at `scale` as one pinned packed batch.  The labels are BED files written to a temporary folder:
label 0 holds every contig whole, the others `8 * contigs` random intervals each of 0.5 % to 8 % of a contig — heavily overlapping labels, as the public
stratification sets are.  Prints one line per timed job: the host's two list passes (wall), the host route's call, the device route's call, and whether the sums agree."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aardvark_amd  # noqa: E402
from aardvark_amd import CompactBatch, PackedBatch, feeder, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--labels", type=int, default=20)
    ap.add_argument("--scale", type=float, default=0.1)
    ap.add_argument("--jobs", type=int, default=3)
    ap.add_argument("--route", default="both", choices=["both", "device", "host"])
    a = ap.parse_args()
    contigs, batch = synth.config_genome(scale=a.scale, threads=16)
    names = ["c%02d" % i for i in range(len(contigs))]
    folder = tempfile.mkdtemp(prefix="strata_ab_")
    with open(os.path.join(folder, "g.fa"), "w") as f:  # (the lists never read a base: the contigs only have to exist by name)
        f.write("".join(">%s\nACGT\n" % n for n in names))
    rng = np.random.default_rng(5)
    rows = []
    for l in range(a.labels):
        path = os.path.join(folder, "l%03d.bed" % l)
        with open(path, "w") as f:
            for c, name in enumerate(names):
                size = len(contigs[c])
                if l == 0:
                    f.write("%s\t0\t%d\n" % (name, size))
                    continue
                s = rng.integers(0, size, 8)
                w = rng.integers(size // 200 + 1, size // 12 + 2, 8)
                f.write("".join("%s\t%d\t%d\n" % (name, int(x), int(x + y)) for x, y in sorted(zip(s, w))))
        rows.append("l%03d\tl%03d.bed\n" % (l, l))
    with open(os.path.join(folder, "strat.tsv"), "w") as f:
        f.write("".join(rows))
    genome = feeder.Genome(os.path.join(folder, "g.fa"))
    strat = feeder.Stratifications(os.path.join(folder, "strat.tsv"))
    ctx = aardvark_amd.Context(0)
    ctx.upload_reference(contigs)
    pb = ctx.pinned_packed(PackedBatch.from_compact(CompactBatch.from_region_batch(batch)))
    res = ctx.pinned_results(pb, packed="only")
    exported = strat.export(genome)
    t0 = time.perf_counter()
    strata = ctx.upload_strata(*exported)
    print("regions %d, labels %d, intervals %d (upload %.3f ms)" % (batch.n_regions, a.labels, len(exported[3]), (time.perf_counter() - t0) * 1e3))
    ctx.solve_packed(pb, res=res)  # warm-up: device code, pools
    plain = []
    for job in range(a.jobs + 1):
        t0 = time.perf_counter()
        ctx.solve_packed(pb, res=res)
        plain.append((time.perf_counter() - t0) * 1e3)
        line = "job %d: unlabelled call %.2f ms" % (job, plain[-1])
        host_sums = dev_sums = None
        if a.route in ("both", "host"):
            t0 = time.perf_counter()
            off, idx = strat.batch_labels(genome, batch)
            t_lists = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            host_sums = ctx.solve_packed(pb, res=res, labels=(a.labels, off, idx)).label_tallies
            t_call = (time.perf_counter() - t0) * 1e3
            line += "; host route: lists %.2f ms (%d entries, %.1f MB) + call %.2f ms = %.2f ms" % (t_lists, len(idx), (off.nbytes + idx.nbytes) / 1e6, t_call, t_lists + t_call)
        if a.route in ("both", "device"):
            t0 = time.perf_counter()
            dev_sums = ctx.solve_packed(pb, res=res, strata=strata).label_tallies
            line += "; device route: call %.2f ms" % ((time.perf_counter() - t0) * 1e3)
        if host_sums is not None and dev_sums is not None:
            line += "; sums equal: %s (checksum %d)" % (bool(np.array_equal(host_sums, dev_sums)), int(dev_sums.sum() % (1 << 40)))
        print(line + (" (warm-up)" if job == 0 else ""))
    strata.free()
    ctx.close()


if __name__ == "__main__":
    main()
