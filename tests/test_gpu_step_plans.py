"""The two step plans (csrc/avk_step_plan.h; context option step_queues: 4 the launch chains folded onto the caller's stream and three more, 8 a stream per chain) on a
real MI355X, forced by the option whatever the process's hardware queues: every output array and the tally against the oracle, bit for bit — on a general batch with
every launch class, on the degenerate batches where a folded chain could lose a wait, and with both HBM tiers disabled."""
import os

import numpy as np
import pytest

import oracle_lib
import scenarios
from aardvark_amd import CompactBatch, CompareConfig, PackedBatch, RegionBatch, synth
from test_wide_parity import het_cluster_regions

pytestmark = pytest.mark.gpu
CPUS = min(os.cpu_count() or 1, 16)
PLANS = [4, 8]
FIELDS = ("status", "ed_h1", "ed_h2", "n_optima", "var_expected", "var_observed", "var_class", "var_zyg")
LANES_ALWAYS = dict(lane_min_regions=0, lane_min_batch=0)
_jobs = {}


def pair_regions(seed, n):
    """the same SNV on each side, zygosities at random: every region is of the looked-up class"""
    rng = np.random.default_rng(seed)
    contig = synth.ACGT[rng.integers(0, 4, size=6000, dtype=np.uint8)]
    regions = []
    for _ in range(n):
        L = int(rng.integers(30, 120))
        start = int(rng.integers(0, contig.size - L))
        p = int(rng.integers(start + 3, start + L - 3))
        ref = bytes(contig[p:p + 1])
        alt_t = alt_q = bytes(synth._snv_alt(contig[p:p + 1], rng))
        regions.append({"start": start, "end": start + L, "truth": [(p, ref, alt_t, "Snv", scenarios.ZY[int(rng.integers(0, 4))])],
                        "query": [(p, ref, alt_q, "Snv", scenarios.ZY[int(rng.integers(0, 4))])]})
    return [bytes(contig)], RegionBatch.from_regions(regions)


def long_windows_among_class_c():
    """class C with records avk_wide_static_ok turns down (window + growth above 255: clusters at a variant gap of 1000) among records the wide kernel takes"""
    contig, bed, truth, query = synth.contig_calls(5, 1_000_000, 3_800 / 3_000_000, seed_ref=905, seed_query=906, str_frac=0.15, multi_frac=0.05)
    long_windows = synth.cluster_regions_v(contig, bed, truth, query, 1000)
    contigs2, small = scenarios.fuzz_regions(411004, 6000, max_vars=9, span=(40, 200))
    small.contig_idx[:] = 1
    return [contig, contigs2[0]], synth.concat_batches([long_windows, small])


BATCHES = {
    # name: (maker, context options)
    "general": (lambda: synth.config_genome(scale=0.02), LANES_ALWAYS),  # (a lane class is launched however few regions it has at this scale)
    "lanes_off": (lambda: het_cluster_regions(61, 2000, n_sites=(1, 6), indel=0.2), dict(LANES_ALWAYS, lane_kernel=0)),
    "wide_off": (lambda: het_cluster_regions(61, 2000, n_sites=(1, 6), indel=0.2), dict(LANES_ALWAYS, wide_kernel=0)),
    "pairs_only": (lambda: pair_regions(62, 3000), LANES_ALWAYS),
    "three_call_only": (lambda: het_cluster_regions(63, 2000, n_sites=(3, 3), drop=0.0), LANES_ALWAYS),
    "class_c_not_wide": (long_windows_among_class_c, dict(LANES_ALWAYS, class_c_nodes_x2=1000)),
    "no_lane_region": (lambda: het_cluster_regions(64, 300, n_sites=(6, 9), drop=0.0), LANES_ALWAYS),
}


def job(oracle, name):
    """the batch and the oracle's results, made once and shared (read-only) by both plans"""
    if name not in _jobs:
        contigs, batch = BATCHES[name][0]()
        ref = oracle_lib.compare_batch(oracle, batch, contigs, threads=CPUS, group_metrics=False)
        _jobs[name] = (contigs, batch, ref, oracle_lib.stats(oracle))
    return _jobs[name]


def context(step_queues, options):
    import aardvark_amd
    ctx = aardvark_amd.Context(0)
    ctx.set_option("step_queues", step_queues)
    ctx.set_option("emit_group_metrics", 0)
    for k, v in options.items():
        ctx.set_option(k, v)
    return ctx


def same(got, ref, what):
    for name in FIELDS:
        assert np.array_equal(getattr(got, name), getattr(ref, name)), (what, name)
    assert np.array_equal(got.tally, ref.tally), what


@pytest.mark.parametrize("step_queues", PLANS)
def test_general_batch_resident_synchronous_and_in_flight(oracle, step_queues):
    contigs, batch, ref, _ = job(oracle, "general")
    ctx = context(step_queues, BATCHES["general"][1])
    try:
        ctx.upload_reference(contigs)
        rb = ctx.upload(batch)
        plan = ctx.work_order(rb, want_order=False)[1]
        print("general", step_queues, plan)
        assert plan["class_c"] and plan["lanes"] and all(f[1] for f in plan["fast"]), plan  # class C and every lane class are present
        for _ in range(3):  # queued back to back: the launches of one step beside those of the next
            ctx.compare_resident(rb, CompareConfig(enable_sequences=False))
        same(ctx.download(rb, group_metrics=False), ref, (step_queues, "resident"))
        rb.free()
        whole = ctx.pinned_packed(PackedBatch.from_compact(CompactBatch.from_region_batch(batch)))
        one = ctx.solve_packed(whole, res=ctx.pinned_results(whole, packed="only"))  # the full result, packed
        assert one.expanded(ctx.lib, batch).diff(ref) == [], step_queues
        sets = [ctx.pinned_results(whole, packed="only") for _ in range(2)]
        tickets = [ctx.submit_packed(whole, res=sets[k]) for k in range(2)]  # two in flight
        for t in tickets:
            t.wait()
        for k in range(2):
            assert np.array_equal(sets[k].region_packed, one.region_packed) and np.array_equal(sets[k].var_packed, one.var_packed), (step_queues, k)
    finally:
        ctx.close()


@pytest.mark.parametrize("step_queues", PLANS)
@pytest.mark.parametrize("name", [n for n in BATCHES if n != "general"])
def test_degenerate_batches(oracle, name, step_queues):
    contigs, batch, ref, _ = job(oracle, name)
    ctx = context(step_queues, BATCHES[name][1])
    try:
        ctx.upload_reference(contigs)
        rb = ctx.upload(batch)
        plan = ctx.work_order(rb, want_order=False)[1]
        print(name, step_queues, plan)
        used = [k for k, f in enumerate(plan["fast"]) if f[1]]
        if name in ("lanes_off", "no_lane_region"):
            assert batch.n_regions > 1 and plan["lanes"] == 0, plan
        elif name in ("pairs_only", "three_call_only"):
            assert plan["lanes"] and len(used) == 1, plan  # one fast class and no other
        elif name == "class_c_not_wide":
            assert 0 < 2 * plan["class_c_not_wide"] <= plan["class_c"], plan  # few enough that the class keeps its wide launch, with the companion launch for these
        for _ in range(2):
            ctx.compare_resident(rb, CompareConfig(enable_sequences=False))
        same(ctx.download(rb, group_metrics=False), ref, (name, step_queues, "resident"))
        if name == "wide_off":
            assert ctx.last_wide_solved() == 0 and ctx.last_lane_solved() > 0
        elif name == "lanes_off":
            assert ctx.last_lane_solved() == 0
        elif name in ("pairs_only", "three_call_only"):
            assert ctx.last_lane_solved() > 0
        rb.free()
        got = ctx.solve_compare_regions(batch, CompareConfig(enable_sequences=False), packed=True)  # the synchronous call, packed results
        assert got.expanded(ctx.lib, batch).diff(ref) == [], (name, step_queues)
    finally:
        ctx.close()


@pytest.mark.parametrize("step_queues", PLANS)
def test_both_hbm_tiers_disabled(oracle, step_queues):
    """Lanes and hand-back chains on, ws_bytes_per_wave = 0 and big_ws_bytes = 0, a batch of three-call regions whose larger searches the lanes would hand back
    (oracle: more search nodes than lane_node_cap in some region) and none of which needs an HBM tier (the default context below solves it without one).  Every
    region has a status and every output is the oracle's: the step has no launch of an HBM tier behind which the chains' leftovers were solved."""
    contigs, batch, ref, stats = job(oracle, "three_call_only")
    print("oracle: most nodes popped in a region %d, longest queue %d" % (stats["max_pops_a"], stats["max_queue_a"]))
    assert stats["max_pops_a"] > 32  # lane_node_cap: the three-call class hands such a region back
    for off in (False, True):
        ctx = context(step_queues, dict(LANES_ALWAYS, adaptive_ws=0, **(dict(ws_bytes_per_wave=0, big_ws_bytes=0) if off else {})))
        try:
            ctx.upload_reference(contigs)
            rb = ctx.upload(batch)
            for _ in range(2):
                ctx.compare_resident(rb, CompareConfig(enable_sequences=False))
            got = ctx.download(rb, group_metrics=False)
            tiers = ctx.last_tier_counts()
            print("tiers disabled %s: regions per tier %s, lanes %d, wide %d" % (off, tiers, ctx.last_lane_solved(), ctx.last_wide_solved()))
            assert tiers[2] == 0 and tiers[3] == 0, tiers  # no region needs an HBM tier: a failure below is no capacity refusal
            assert int(got.tally[-2]) == batch.n_regions  # every region has a status
            same(got, ref, (step_queues, off))
            rb.free()
        finally:
            ctx.close()
