"""bench.py's output contract: exactly one line on stdout, a JSON object with the agreed keys — also when a RCCL communicator is up
(RCCL writes a version banner to file descriptor 1)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KEYS = ["metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
        "roofline", "cpu_baseline", "resident_value", "resident", "wide_soa", "dwfa_byte_compares_per_s", "secondary"]


@pytest.mark.gpu
@pytest.mark.parametrize("force_dist", ["0", "1"])
def test_one_json_line_on_stdout(force_dist):
    env = dict(os.environ, AVK_BENCH_FORCE_DIST=force_dist, MASTER_ADDR="127.0.0.1", MASTER_PORT="29577")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "4", "--warmup", "2", "--scale", "0.01", "--resident-steps", "4", "--merge-scale", "0.01", "--secondary-scale", "0.01"], capture_output=True, text=True, env=env,
                       timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1, r.stdout[:500]
    out = json.loads(lines[0])
    assert [k for k in KEYS if k not in out] == []
    assert out["metric"] == "compared regions/sec (whole node)" and out["unit"] == "regions/s" and out["n_gpus"] == 1 and out["steps"] == 4 and out["warmup"] == 2
    assert out["higher_is_better"] is True and out["scaling"] == "weak" and out["vs_baseline"] is None and out["dtype"] == "u8" and out["data"] == "synthetic"
    assert out["config"]["parity"] == "bit-identical" and "workload" in out["config"]
    rf = out["roofline"]
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-12 and rf["achieved"] > 0
    cb = out["cpu_baseline"]
    assert cb["kind"] == "port" and cb["unit"] == "regions/s" and cb["cores"] >= 1 and cb["value"] > 0 and cb["sample"]
    assert 0 < cb["parallel_efficiency"] < 1.5 and cb["one_thread_value"] > 0
    assert out["resident_value"] > 0 and out["resident"]["steps"] == 4
    assert out["value"] > 0 and out["ms_per_step"] > 0
    sec = out["secondary"]
    assert {"shard_1_of_8", "chr20_snv", "dense_mix", "min_variant_gap_1000", "merge_3_callers"} <= set(sec)
    assert all(sec[k]["parity"].startswith("bit-identical") for k in ("shard_1_of_8", "dense_mix", "min_variant_gap_1000", "merge_3_callers", "chr20_snv"))
    assert all(sec[k]["cpu_baseline"]["value"] > 0 and sec[k]["cpu_baseline"]["cores"] >= 1 for k in ("shard_1_of_8", "dense_mix", "min_variant_gap_1000", "merge_3_callers", "chr20_snv"))
    assert sec["shard_1_of_8"]["strong_scaling_bound"]["boundary"] > 0
    assert out["cpu_baseline"]["all_core_extrapolation"]["value"] >= out["cpu_baseline"]["value"]


@pytest.mark.gpu
def test_two_ranks_on_one_gpu_run_the_sharded_job():
    """bench.py --gpus 2 as the driver launches it (torch.distributed.run, one process per rank), on a box with ONE GPU: both ranks on GPU 0 and the sums carried by gloo
    (AVK_BENCH_ONE_DEVICE / AVK_BENCH_BACKEND; RCCL does not take two ranks on one device).  Everything else is the N-rank path: the compare job cut by hash(region_id),
    the tally all-reduce inside the timed region, the job checksum, and the merge job (configs[4]) cut the same way with its summary counters all-reduced."""
    env = dict(os.environ, AVK_BENCH_BACKEND="gloo", AVK_BENCH_ONE_DEVICE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29579")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29579",
           os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--steps", "4", "--warmup", "2", "--scale", "0.01", "--resident-steps", "4", "--merge-scale", "0.01"]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[:500]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["scaling"] == "strong" and out["config"]["parity"] == "bit-identical" and out["value"] > 0
    m = out["secondary"]["merge_3_callers"]
    assert m["n_gpus"] == 2 and m["parity"].startswith("bit-identical") and m["value"] > 0 and len(m["regions_per_rank"]) == 2
    assert sum(m["regions_per_rank"]) > 0 and abs(m["regions_per_rank"][0] - m["regions_per_rank"][1]) < 0.1 * sum(m["regions_per_rank"])
    assert m["variants_counted"] > 0


HEADLINE = ["metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"]


def region_types(batch):
    """the call types of every region, ascending: its BASEPAIR groups are the joint one and one per type, in this order"""
    return [sorted(set(batch.var_type[batch.t_off[r]:batch.t_off[r] + batch.t_cnt[r]].tolist()) | set(batch.var_type[batch.q_off[r]:batch.q_off[r] + batch.q_cnt[r]].tolist()))
            for r in range(batch.n_regions)]


def assert_dump_is(d, batch, want):
    """the arrays bench.py --dump-outputs wrote (name -> array) are the oracle's outputs on their sample"""
    import numpy as np
    assert all(a.dtype in (np.float32, np.float64) for a in d.values()) and sum(a.nbytes for a in d.values()) <= 64 << 20
    ri, vi = d["region_index"].astype(np.int64), d["call_index"].astype(np.int64)
    assert np.array_equal(d["tally"], want.tally.astype(np.float64))
    for f in ("status", "ed_h1", "ed_h2", "n_optima", "type_present"):
        assert np.array_equal(d[f], getattr(want, f)[ri].astype(np.float32)), f
    for f in ("var_expected", "var_observed", "var_class", "var_zyg"):
        assert np.array_equal(d[f], getattr(want, f)[vi].astype(np.float32)), f
    types = region_types(batch)
    first = np.concatenate([[0], np.cumsum(d["bp_group_count"].astype(np.int64))])
    assert first[-1] == d["bp_groups"].shape[0]
    for j, r in enumerate(ri):
        assert d["bp_group_count"][j] == 1 + len(types[r])
        if want.status[r] == 0:
            g = want.group_metrics[r, [0] + [1 + t for t in types[r]], 14:18]  # AVK_F_BP_TRUTH_TP .. AVK_F_BP_QUERY_FP
            assert np.array_equal(d["bp_groups"][first[j]:first[j + 1]], g.astype(np.float32)), r


def load_dump(directory):
    import numpy as np
    return {f[:-4]: np.load(os.path.join(directory, f)) for f in sorted(os.listdir(directory)) if f.endswith(".npy")}


def test_dump_outputs_do_not_depend_on_the_spill_order(tmp_path, oracle):
    """--dump-outputs lists a region's packed BASEPAIR groups as avk_group_metrics_from_compact reads them, so the order the kernels spilled them in does not show:
    the oracle's outputs packed with two spill orders give the same files, and those are the oracle's"""
    import copy
    import numpy as np
    import bench
    import oracle_lib
    from aardvark_amd import synth
    contigs, batch = synth.config_genome(scale=0.002, threads=4)
    want = oracle_lib.compare_batch(oracle, batch, contigs, threads=4, group_metrics=True)
    types = region_types(batch)
    dumps = []
    for seed in (1, 2):
        res = copy.copy(want)
        res.bp_packed = np.zeros(batch.n_regions, np.uint32)
        res.bp_groups = np.zeros((batch.n_regions + batch.n_variants + 1, 4), np.uint32)
        at = 0
        for r in np.random.default_rng(seed).permutation(batch.n_regions):
            if want.status[r] != 0:
                continue
            g = want.group_metrics[r, [0] + [1 + t for t in types[r]], 14:18]
            if (g == g[0]).all() and (g < 128).all():
                res.bp_packed[r] = g[0, 0] | g[0, 1] << 7 | g[0, 2] << 14 | g[0, 3] << 21
            else:
                res.bp_packed[r] = 0x80000000 | at
                res.bp_groups[at:at + len(g)] = g
                at += len(g)
        assert at > 0
        res.bp_spilled = np.array([at], np.uint32)
        bench.dump_outputs(str(tmp_path / str(seed)), None, batch, res)
        dumps.append(load_dump(str(tmp_path / str(seed))))
    assert sorted(dumps[0]) == sorted(dumps[1]) and all(np.array_equal(dumps[0][k], dumps[1][k]) for k in dumps[0])
    assert_dump_is(dumps[0], batch, want)


@pytest.mark.gpu
def test_plain_run_reports_the_headline_and_dumps_its_outputs(tmp_path, oracle):
    """A plain run times --steps calls and prints the headline only; --dump-outputs writes what the last timed call returned, the same in two runs of the same
    arguments, and the oracle's"""
    import oracle_lib
    from aardvark_amd import synth
    dumps = []
    for k in range(2):
        d = str(tmp_path / ("run%d" % k))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--scale", "0.01", "--dump-outputs", d],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = r.stdout.splitlines()
        assert len(lines) == 1, r.stdout[:500]
        out = json.loads(lines[0])
        assert [k for k in HEADLINE if k not in out] == []
        assert out["metric"] == "compared regions/sec (whole node)" and out["unit"] == "regions/s" and out["higher_is_better"] is True and out["dtype"] == "u8"
        assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0 and abs(out["value"] * out["ms_per_step"] * 1e-3 - out["config"]["regions_per_gpu"]) < 1e-6 * out["value"]
        assert not {"resident", "roofline", "cpu_baseline", "secondary", "pipelined"} & set(out)
        dumps.append(load_dump(d))
    import numpy as np
    assert sorted(dumps[0]) == sorted(dumps[1]) and all(np.array_equal(dumps[0][k], dumps[1][k]) for k in dumps[0])
    contigs, batch = synth.config_genome(scale=0.01, threads=8)
    assert_dump_is(dumps[0], batch, oracle_lib.compare_batch(oracle, batch, contigs, threads=8, group_metrics=True))
