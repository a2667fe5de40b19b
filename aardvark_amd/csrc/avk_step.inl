/* The solver step: every launch of a resident batch, queued at once on the chains of avk_step_plan.h.  Included by avk_host.hip (host code: the context, the batch and
 * the kernels are declared there).
 *
 *   Step       what one step knows while it queues its launches: the plan and its streams, the table of chain ends, the base kernel arguments, the geometry
 *              (avk_step_geometry.h) and the hand-back segments.  run_internal makes one on its stack and calls its phases in order; nothing is allocated per step.
 *   ends       the ONLY record of what the caller's stream still has to wait for: an end is recorded (seq != 0) and, once the caller's stream waits for it or the
 *              folded plan shows that it already does, waited. */

/* tile width of a lane launch (options lane_width_one / lane_width_two: 64, 32 or 16 records per wave at a time) */
static uint32_t lane_width_log2(const avk_ctx *ctx, uint32_t maxv) {
    return avk_width_log2(maxv > 2 ? ctx->lane_width_three : (maxv > 1 ? ctx->lane_width_two : ctx->lane_width_one));
}
static uint32_t head_width_log2(const avk_ctx *ctx, uint32_t head_regions) {
    int64_t w = ctx->lane_head_width;
    if (ctx->lane_head_auto && w > 4) { /* lanes that diverge take turns: a head that cannot fill the machine's lane waves 16 wide is spread over more, narrower waves */
        const int64_t fit = head_regions < 8192u ? 4 : (head_regions < 24576u ? 8 : 16);
        if (fit < w) w = fit;
    }
    return avk_width_log2(w);
}
/* which of the two kernels a lane launch runs: four lanes per region when the launch is narrow (option lane_quad) */
static bool lane_launch_is_quad(const avk_ctx *ctx, const avk::lane::LaneArgs &la) { return ctx->lane_quad && la.lanes_log2 <= 4; }
/* LDS bytes of a one-wave workgroup of the lane kernel (0: does not fit) and the grid that fills the machine (avk_lane_geometry) */
static size_t lane_launch_geometry(const avk_ctx *ctx, const avk::lane::LaneArgs &la, uint32_t *grid) {
    const AvkLaneShape shape = {la.W, la.nm, la.ed_max, la.qcap, la.pool, la.lanes_log2, la.n_tiles, lane_launch_is_quad(ctx, la)};
    const AvkLaneCaps caps = {ctx->n_cus, ctx->lane_waves_per_cu, ctx->lane_waves_three};
    return avk_lane_geometry(shape, caps, grid);
}
/* a launch of a lane class: one lane per region, or four (lane_launch_is_quad) */
/* done: an event that fires when THIS launch ends (bound to the launch's own completion signal: an event recorded behind the launch is a packet of its own in the
 * stream, and the next launch of the chain started 55-60 us later for it) */
static void launch_lane_class(const avk_ctx *ctx, uint32_t grid, size_t lds, hipStream_t s, const AvkKernelArgs &f, const avk::lane::LaneArgs &la, hipEvent_t done = nullptr) {
    if (lane_launch_is_quad(ctx, la)) {
        if (lds * 8 > 160 * 1024) hipExtLaunchKernelGGL(avk_quad_kernel_wide_regs, dim3(grid), dim3(64), lds, s, nullptr, done, 0, f, la); /* fewer than eight workgroups per CU by LDS: registers to spare */
        else hipExtLaunchKernelGGL(avk_quad_kernel, dim3(grid), dim3(64), lds, s, nullptr, done, 0, f, la);
    }
    else hipExtLaunchKernelGGL(avk_lane_kernel, dim3(grid), dim3(64), lds, s, nullptr, done, 0, f, la);
}

/* The dynamic LDS the step's kernels may ask for, once per context: the lane and quad kernels and the LDS-tier region kernels a whole CU's 160 KB, the wide kernels a
 * workgroup's 64 KB.  The call only raises a limit that a later launch is checked against — it launches and allocates nothing, and all of these kernels are in the one
 * code object the first launch of the process loads — so the wide kernels get theirs whether or not this context's steps will use them. */
static int ensure_kernel_attrs(avk_ctx *ctx) {
    if (ctx->kernel_attrs_set) return AVK_E_OK;
    const void *cu_lds[] = {(const void *)avk_lane_kernel, (const void *)avk_quad_kernel, (const void *)avk_quad_kernel_wide_regs, (const void *)avk_region_kernel_lds,
                            (const void *)avk_region_kernel_lds_lazy};
    for (const void *k : cu_lds) AVK_HIP(ctx, hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    AVK_HIP(ctx, hipFuncSetAttribute((const void *)avk_wide_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
    AVK_HIP(ctx, hipFuncSetAttribute((const void *)avk_wide_kernel_lazy, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
    ctx->kernel_attrs_set = true;
    return AVK_E_OK;
}

/* The table of avk_pairs.inl for this max_branch_factor, on `s`: sixteen probe regions through the lane kernel, outputs redirected into the table.
 * Words of d_pair_aux: [0, 768) probe records, [768, 784) probe reference, [784, 792) its exception bitmap (zeros), [792, 812) BASEPAIR offsets 0, 2, .. 32,
 * [812] tile counter, [813] overflow count, [816, 880) overflow list, [896, 896 + 2 * AVK_TALLY_STRIDE) a partial tally nobody reads. */
static int ensure_pair_table(avk_ctx *ctx, uint32_t max_branch_factor, hipStream_t s) {
    enum { AUX_WORDS = 896 + 2 * AVK_TALLY_STRIDE };
    if (!ctx->d_pair_tab) {
        AVK_HIP(ctx, hipMalloc((void **)&ctx->d_pair_tab, sizeof(avk::pairs::PairTable)));
        AVK_HIP(ctx, hipMalloc((void **)&ctx->d_pair_aux, (size_t)AUX_WORDS * 4));
        std::vector<uint32_t> aux(AUX_WORDS, 0);
        avk::pairs::pair_probe_records(aux.data(), aux.data() + 768);
        for (uint32_t k = 0; k <= avk::pairs::N_SIG; ++k) aux[792 + k] = 2 * k;
        AVK_HIP(ctx, hipMemcpy(ctx->d_pair_aux, aux.data(), (size_t)AUX_WORDS * 4, hipMemcpyHostToDevice));
        ctx->pair_tab_mbf = -1;
    }
    if (ctx->pair_tab_mbf == (int64_t)max_branch_factor) return AVK_E_OK;
    AVK_HIP(ctx, hipMemsetAsync(ctx->d_pair_tab, 0xFF, sizeof(avk::pairs::PairTable), s));
    AVK_HIP(ctx, hipMemsetAsync(ctx->d_pair_aux + 812, 0, (size_t)(AUX_WORDS - 812) * 4, s));
    AvkKernelArgs f;
    memset(&f, 0, sizeof(f));
    f.ref_2bit = ctx->d_pair_aux + 768;
    f.ref_exc = ctx->d_pair_aux + 784;
    f.n_regions = avk::pairs::N_SIG;
    f.max_branch_factor = max_branch_factor;
    f.region_out = &ctx->d_pair_tab->region[0][0];
    f.var_out = &ctx->d_pair_tab->var[0][0];
    f.group_metrics = &ctx->d_pair_tab->gm[0][0];
    f.bp_off = ctx->d_pair_aux + 792;
    f.bp_out = &ctx->d_pair_tab->bp[0][0];
    f.tally = (uint64_t *)(ctx->d_pair_aux + 896);
    f.overflow_list = ctx->d_pair_aux + 816;
    f.overflow_count = ctx->d_pair_aux + 813;
    avk::lane::LaneArgs la;
    memset(&la, 0, sizeof(la));
    const AvkFastClass &cl = AVK_FAST_CLASS[0];
    la.recs = ctx->d_pair_aux;
    la.rec_words = AVK_FAST_WORDS_OF(1);
    la.n_tiles = 1;
    la.tile_counter = ctx->d_pair_aux + 812;
    la.W = cl.W, la.nm = 2, la.ed_max = cl.ed_max, la.qcap = cl.qcap;
    la.lanes_log2 = 6;
    la.max_nodes = 250;
    uint32_t grid = 0;
    const size_t lds = lane_launch_geometry(ctx, la, &grid);
    const int ra = ensure_kernel_attrs(ctx);
    if (ra) return ra;
    hipLaunchKernelGGL(avk_lane_kernel, dim3(1), dim3(64), lds, s, f, la);
    AVK_HIP(ctx, hipGetLastError());
    ctx->pair_tab_mbf = (int64_t)max_branch_factor;
    return AVK_E_OK;
}

struct Step {
    avk_ctx *const ctx;
    const CallSpec &spec;
    avk_dev_batch *const db;
    const avk_compare_config *const cfg;
    void *const tally_dev;
    const uint32_t mode;
    const uint64_t n;

    /* which workspace tiers are on, which get a launch of their own, the last of those; which of the side kernels run */
    bool use[4], launch[4];
    int last = -1;
    bool use_fast = false, use_wide = false, timed = false;
    uint32_t n_fast = 0;
    avk::wide::WideArgs wa;
    AvkStepGeometry geo;
    int64_t big_bytes = 0;
    uint32_t big_slots = 0;
    AvkKernelArgs a; /* the base arguments; the tier launches edit and launch them, every other launch starts from a copy */
    uint32_t *lists[4];
    const uint32_t *list = nullptr, *count = nullptr; /* what the next tier launch reads (first launch: the records themselves are in work order) */
    int nlist = 0;

    /* ---- the plan: the launches name chains (avk_step_plan.h), the plan gives each chain its stream.  Two chains on one stream follow each other in the order they
     * are queued here, and the events between them are dropped:
     *   fork      a stream waits for the caller's stream once, ahead of the first chain queued on it
     *   end/join  the end of every chain is recorded as ever; the caller's stream waits per STREAM, for the last end recorded on it, and not again for an earlier one */
    bool folded = false;
    AvkStepPlan plan;
    hipStream_t slot_stream[AVK_N_CHAINS];
    bool slot_forked[AVK_N_CHAINS] = {true, false, false, false, false, false, false, false};
    struct ChainEnd {
        int slot, seq; /* seq 0: not recorded in this step */
        bool waited;   /* the caller's stream waits for it (or, folded, for a later end of its stream: the skip counts) */
    };
    ChainEnd ends[AVK_N_ENDS];
    int end_seq = 0, slot_joined[AVK_N_CHAINS] = {0, 0, 0, 0, 0, 0, 0, 0}; /* per stream: the latest end the caller's stream already waits for */

    /* ---- the first tier's launches, from one phase to the next */
    uint32_t n_c = 0;                                   /* regions of the HBM solo launch */
    uint32_t solo = 0, solo_regions = 0, hbm_solo = 0; /* workgroups of the LDS solo launch and its regions; workgroups of the HBM solo launch */
    uint32_t shared_base = 0, shared_n = 0;             /* class C records the main HBM launch helps the solo launch with, behind those a team launch has (0: the class
                                                         * went through the wide kernel, whose leftovers are the solo launch's alone) */
    /* lane chains: 0 the two-call classes, 1 the one-call classes, 2 the three-call class, 3 the heads of the two-call classes */
    enum { N_LS = 4 };
    static constexpr int lchain[N_LS] = {AVK_CH_TWO_CALL, AVK_CH_ONE_CALL, AVK_CH_THREE_CALL, AVK_CH_HEAD_HANDBACKS};
    static constexpr int lend[N_LS] = {AVK_END_LANE0, AVK_END_LANE1, AVK_END_LANE2, AVK_END_LANE3};
    bool lused[N_LS] = {false, false, false, false};
    /* hand-backs per chain: the launches of a lane stream append to a list of the stream's own, a head launch to one of its own; a list is read by a launch
     * of avk_wide.inl that follows its writers in stream order (the chain's list: on the chain's stream, no event; a head's: on the fourth lane stream,
     * behind the head's event, while the rest of the class runs).  One launch for one list behind ALL lane streams started 60-130 us after the last lane
     * launch (three event waits) and lasted as long as its longest region — a head's hand-back, 160-340 us — at the very end of the step. */
    bool chains = false;
    struct HbSeg {
        uint32_t *list, *count, *cursor;
    };
    uint32_t hb_off = 0;
    int hb_n = 0, hb_heads = 0;
    HbSeg chain_seg[2] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};
    AvkKernelArgs chain_d; /* with chains: the launch that follows the lane chains' ends (flush_chains) */
    uint32_t chain_dblocks = 0;

    Step(avk_ctx *ctx_, const CallSpec &spec_, avk_dev_batch *db_, const avk_compare_config *cfg_, void *tally_dev_, uint32_t mode_)
        : ctx(ctx_), spec(spec_), db(db_), cfg(cfg_), tally_dev(tally_dev_), mode(mode_), n(db_->n_regions) {
        memset(ends, 0, sizeof(ends));
        memset(&chain_d, 0, sizeof(chain_d));
    }

    /* ---- chains, forks, ends ---- */
    hipStream_t S(int chain) const { return slot_stream[plan.slot[chain]]; }
    bool same_stream(int c1, int c2) const { return plan.slot[c1] == plan.slot[c2]; }
    hipError_t fork(int chain, hipEvent_t ev) { /* ev: recorded on the caller's stream */
        const int s = plan.slot[chain];
        if (s == 0 || (folded && slot_forked[s])) return hipSuccess;
        slot_forked[s] = true;
        return hipStreamWaitEvent(slot_stream[s], ev, 0);
    }
    hipError_t record_end(int id, int chain) {
        ends[id] = {plan.slot[chain], ++end_seq, false};
        return hipEventRecord(ctx->ev_end[id], S(chain));
    }
    /* What the table stands for (each was a flag of its own once):
     *   LDS solo / class C / not-wide pending   recorded, and no join has named it since: the tier launches name the first two, nothing but finish() the third
     *   the lanes' hand-back launch pending     AVK_END_DONE is recorded only by a step without hand-back chains, AVK_END_EARLY only by one with lane launches, and
     *                                           both are joined only by finish()
     * Not in the table: whether the main HBM launch shares class C with the solo launch (shared_n: that depends on the wide kernel having taken the class), and
     * whether the chains' last launch has been queued (chain_dblocks, below). */
    bool pending(int id) const { return ends[id].seq != 0 && !ends[id].waited; }
    /* the caller's stream waits for those of these ends that are pending (the plan with a stream per chain: each of them, in this order) */
    hipError_t join(const int *ids, int k) {
        int order[AVK_N_ENDS], m = 0;
        for (int i = 0; i < k; ++i)
            if (pending(ids[i])) order[m++] = ids[i];
        if (folded) std::sort(order, order + m, [&](int x, int y) { return ends[x].seq > ends[y].seq; });
        for (int i = 0; i < m; ++i) {
            ChainEnd &e = ends[order[i]];
            e.waited = true;
            if (e.slot == 0 || (folded && slot_joined[e.slot] >= e.seq)) continue;
            if (slot_joined[e.slot] < e.seq) slot_joined[e.slot] = e.seq;
            const hipError_t r = hipStreamWaitEvent(ctx->stream, ctx->ev_end[order[i]], 0);
            if (r != hipSuccess) return r;
        }
        return hipSuccess;
    }
    hipError_t join1(int id) { return join(&id, 1); }
    /* what the chains' launches of avk_wide.inl left (d_overflow7): behind the ends of the lane chains, once per step.  chain_dblocks is the launch's size while it
     * waits to be queued and 0 once it is — not a matter of the ends table, which cannot tell a step whose lane ends are all joined from one that recorded none */
    bool chains_unflushed() const { return chain_dblocks != 0; }
    hipError_t flush_chains() {
        const hipError_t r = join(lend, N_LS);
        if (r != hipSuccess) return r;
        hipLaunchKernelGGL(avk_region_kernel_lds_lazy, dim3(chain_dblocks), dim3(256), (size_t)AVK_WAVES_PER_BLOCK * (size_t)ctx->lds_bytes_per_wave, ctx->stream, chain_d);
        chain_dblocks = 0;
        return hipGetLastError();
    }

    /* ---- the phases, in the order run_internal calls them ---- */

    /* which tiers and kernels run, the geometry, the workspaces and the batch's output arrays */
    int workspaces_and_outputs() {
        if (ctx->lds2_bytes_per_wave * 4 > 160 * 1024) return fail(ctx, AVK_E_ARG, "lds2_bytes_per_wave too large");
        /* sequences: allocate the output arena on first use */
        if (cfg->enable_sequences && !db->d_seq) {
            int rc = db->dev_packed ? pool_alloc_t(ctx, db, &db->d_seq, (size_t)db->seq_total + 16) : dev_alloc(ctx, &db->d_seq, (size_t)db->seq_total + 16);
            if (rc) return rc;
        }
        /* up to four launches, one per workspace tier; each consumes the overflow list of the one
         * before it (its length is read on the device, so nothing comes back to the host in between) */
        const bool use_[4] = {ctx->lds_bytes_per_wave > 0, ctx->lds2_bytes_per_wave > 0, ctx->ws_bytes_per_wave > 0, ctx->big_ws_bytes > 0};
        /* which tiers get a launch of their own: the large LDS slices normally only serve the solo launch (their
         * overflow pass runs one workgroup per CU and measured slower than handing the overflow to the HBM tier,
         * which runs twice the waves), and the big HBM slices are claimed in place by the tier-2 launch */
        const bool launch_[4] = {use_[0], use_[1] && (ctx->lds2_overflow_pass || !use_[0]), use_[2], use_[3] && !use_[2]};
        for (int t = 0; t < 4; ++t) {
            use[t] = use_[t], launch[t] = launch_[t];
            if (launch[t]) last = t;
        }
        if (last < 0) return fail(ctx, AVK_E_ARG, "every workspace tier is disabled");
        /* The lane-per-region kernel takes the fast segments at the end of the work order (WorkPlan::fast_base); what it cannot finish it
         * appends to the list the first HBM launch reads.  Without such a launch, with sequence output (the haplotype bytes are never
         * materialised there) or with the exact-match shortcut the wave-per-region bulk launch covers those records itself. */
        /* which classes go to the lanes was decided with the work order (plan_work_order, option lane_min_regions at upload time) */
        const uint32_t n_lane_regions = db->plan.n_fast_total;
        /* the lanes read the 2-bit reference only: with use_packed_reference off (a.ref_2bit == NULL) the wave-per-region kernels take every record */
        use_fast = ctx->lane_kernel && launch[0] && !launch[1] && launch[2] && !launch[3] && db->d_fast && n_lane_regions && !cfg->enable_sequences &&
                   !cfg->enable_exact_shortcut && n && ctx->use_packed_reference && ctx->d_ref2b;
        n_fast = use_fast ? n_lane_regions : 0u;
        /* the wave-cooperative kernel of avk_wide.inl takes class C and what the three-call lane class hands back ahead of the HBM-tier launches (which get what it
         * cannot take); like the lanes it reads the 2-bit reference and writes no sequences */
        use_wide = ctx->wide_kernel && launch[0] && !launch[1] && launch[2] && !launch[3] && !cfg->enable_sequences && !cfg->enable_exact_shortcut && n &&
                   ctx->use_packed_reference && ctx->d_ref2b;
        wa.lds_words = (uint32_t)(ctx->wide_lds_bytes / 4);
        wa.skip_static = 0;
        const int ra = ensure_kernel_attrs(ctx);
        if (ra) return ra;
        if (db->dev_packed && !use_fast) { /* the wave-per-region launches take every record: write the ones the packer left for later */
            const int rf = ensure_all_records(ctx, db, ctx->stream);
            if (rf) return rf;
        }
        /* the per-wave slice: the option, or what the packer's prediction asks for (device-packed batches of large windows: upload_device_packed); large
         * slices mean fewer waves per launch (option ws_budget_bytes) and more of the shared big slices for what still overflows */
        const int64_t ws_bytes = db->ws_bytes_eff > ctx->ws_bytes_per_wave ? db->ws_bytes_eff : ctx->ws_bytes_per_wave;
        const int64_t big_waves = ws_bytes > ctx->ws_bytes_per_wave && ctx->big_waves < 64 ? 64 : ctx->big_waves;
        big_bytes = db->big_bytes_eff > ctx->big_ws_bytes && ctx->big_ws_bytes > 0 ? db->big_bytes_eff : ctx->big_ws_bytes;
        const AvkStepGeometryIn gin = {ctx->n_cus, ctx->waves_per_cu, n, n_fast, use_fast, ws_bytes, ctx->ws_budget_bytes, ctx->hbm_solo_blocks, ctx->hbm_early_blocks, big_waves, big_bytes};
        geo = avk_step_geometry(gin);
        big_slots = use[2] && use[3] ? (uint32_t)(big_waves < (int64_t)AVK_CTR_BIG_BUSY_LEN ? big_waves : (int64_t)AVK_CTR_BIG_BUSY_LEN) : 0u;
        const auto t_ws = std::chrono::steady_clock::now();
        const bool ws_grows = geo.ws_need > ctx->ws_alloc;
        if (ws_grows) {
            if (ctx->d_ws) {
                AVK_HIP(ctx, hipStreamSynchronize(ctx->stream));
                (void)hipFree(ctx->d_ws);
                ctx->d_ws = nullptr;
                ctx->ws_alloc = 0;
            }
            AVK_HIP(ctx, hipMalloc((void **)&ctx->d_ws, geo.ws_need + 256));
            ctx->ws_alloc = geo.ws_need;
        }
        if (geo.big_need > ctx->big_alloc) {
            if (ctx->d_big) {
                AVK_HIP(ctx, hipStreamSynchronize(ctx->stream));
                (void)hipFree(ctx->d_big);
                ctx->d_big = nullptr;
                ctx->big_alloc = 0;
            }
            AVK_HIP(ctx, hipMalloc((void **)&ctx->d_big, geo.big_need + 256));
            ctx->big_alloc = geo.big_need;
        }
        if (getenv("AVK_TIMING") && (ws_grows || geo.big_need > 0))
            fprintf(stderr, "avk run: workspaces (%.1f GB per-wave slices%s, %.1f GB shared slices) %.3f ms\n", (double)geo.ws_need / 1e9, ws_grows ? ", allocated now" : "",
                    (double)geo.big_need / 1e9, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_ws).count());
        if (!db->scratch_clean) { /* normally left clean by avk_tally_reduce of the previous call */
            AVK_HIP(ctx, hipMemsetAsync(db->d_partials, 0, (size_t)AVK_TALLY_STRIDE * AVK_TALLY_COPIES * sizeof(uint64_t), ctx->stream));
            AVK_HIP(ctx, hipMemsetAsync(db->d_counters, 0, AVK_N_COUNTERS * sizeof(uint32_t), ctx->stream));
        }
        db->scratch_clean = false;
        if (spec.emit_bp && mode == 0 && !db->d_bp && db->d_bp_off) {
            int rc = db->dev_packed ? pool_alloc_t(ctx, db, &db->d_bp, (size_t)db->n_bp_groups * 4 + 4) : dev_alloc(ctx, &db->d_bp, (size_t)db->n_bp_groups * 4 + 4);
            if (rc) return rc;
        }
        if (spec.emit_gm && !db->d_gm) {
            int rc = db->dev_packed ? pool_alloc_t(ctx, db, &db->d_gm, (size_t)n * AVK_N_GROUPS * AVK_N_FIELDS + 4) : dev_alloc(ctx, &db->d_gm, (size_t)n * AVK_N_GROUPS * AVK_N_FIELDS);
            if (rc) return rc;
        }
        return AVK_E_OK;
    }

    /* the arguments every launch starts from, the step's first event, its plan and streams */
    int base_args() {
        memset(&a, 0, sizeof(a));
        a.regions = db->d_regions;
        a.blob = db->d_blob;
        a.ref_bytes = ctx->d_ref;
        a.ref_2bit = ctx->use_packed_reference ? ctx->d_ref2b : nullptr;
        a.ref_exc = ctx->d_refexc;
        a.n_regions = (uint32_t)n;
        a.max_branch_factor = cfg->max_branch_factor;
        a.enable_exact_shortcut = cfg->enable_exact_shortcut ? 1u : 0u;
        a.mode = mode;
        a.tier[0].ws_bytes = (uint64_t)ctx->lds_bytes_per_wave;
        a.tier[0].ed_cap = (uint32_t)ctx->lds_ed_cap;
        a.tier[1].ws_bytes = (uint64_t)ctx->lds2_bytes_per_wave;
        a.tier[1].ed_cap = (uint32_t)ctx->lds2_ed_cap;
        a.tier[2].ws_bytes = (uint64_t)geo.ws_bytes;
        a.tier[2].ed_cap = ctx->hbm_ed_cap > 0 ? ((uint32_t)ctx->hbm_ed_cap | AVK_CAP_BOUND_ONLY) : 0u;
        a.tier[3].ws_bytes = (uint64_t)big_bytes;
        a.tier[3].ed_cap = 0;
        a.region_out = db->d_region_out;
        a.group_metrics = spec.emit_gm ? db->d_gm : nullptr;
        a.var_out = db->d_var_out;
        a.seq_bytes = cfg->enable_sequences ? db->d_seq : nullptr;
        a.seq_len = cfg->enable_sequences ? db->d_seqlen : nullptr;
        a.tally = db->d_partials;
        if (spec.emit_bp && mode == 0 && db->d_bp) {
            a.bp_off = db->d_bp_off;
            a.bp_out = db->d_bp;
        }
        if (db->dev_packed && !db->records_full) { /* (only the launches for handed-back regions ever meet an index >= lazy_from) */
            a.lazy_dp = db->d_dp_args;
            a.lazy_from = db->lazy_from;
        }
        if (cfg->max_branch_factor == 0) return fail(ctx, AVK_E_ARG, "max_branch_factor must be greater than 0 (query_optimizer.rs:177)");
        lists[0] = db->d_overflow, lists[1] = db->d_overflow2, lists[2] = db->d_overflow3, lists[3] = db->d_overflow4;

        timed = ctx->timing_events != 0;
        if (timed) AVK_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
        ctx->ev_lane_valid = false;
        folded = ctx->step_queues ? ctx->step_queues < AVK_STEP_QUEUES_WIDE : ctx->step_folded_auto;
        plan = avk_step_plan(folded ? AVK_STEP_SLOTS_FOLDED : AVK_STEP_QUEUES_WIDE, use_fast);
        if (folded) {
            AvkStepPlan trial;
            if (use_fast && avk_step_plan_parse(getenv("AVK_STEP_PLAN"), &trial)) plan = trial; /* (measurements: another assignment, a digit per chain) */
            AVK_HIP(ctx, ensure_fold_streams(ctx));
        }
        hipStream_t wide_slots[AVK_N_CHAINS] = {ctx->stream, ctx->side_stream, ctx->wide_stream, ctx->side_stream2, ctx->lane_stream, ctx->lane_stream2, ctx->lane_stream3, ctx->lane_stream4};
        for (int k = 0; k < AVK_N_CHAINS; ++k) slot_stream[k] = folded && k >= 1 && k < AVK_STEP_SLOTS_FOLDED ? ctx->fold_stream[k - 1] : wide_slots[k];
        return AVK_E_OK;
    }

    /* the arguments of tier t's own launch, and the waits it needs */
    int tier_begin(int t) {
        a.pass_tier = (uint32_t)t;
        a.work_list = list;
        a.work_base = 0;
        a.n_work_dev = count;
        a.work_counter = db->d_counters + avk_ctr_tier_cursors((uint32_t)t);
        if (t != last) {
            a.overflow_list = lists[nlist];
            a.overflow_count = db->d_counters + avk_ctr_overflow_count((uint32_t)nlist);
        } else {
            a.overflow_list = nullptr;
            a.overflow_count = nullptr;
        }
        if (t >= 2) { /* the HBM launches read the list the LDS solo launch appends to; the tier-1 launch does not */
            if (chains_unflushed()) AVK_HIP(ctx, flush_chains()); /* ahead of the waits for the long solo launches, which it does not depend on */
            AVK_HIP(ctx, join1(AVK_END_LDS_SOLO));
            /* the tier-3 launch of its own (big_slots == 0) reads the list the HBM solo launch appends to */
            if (t == 3) AVK_HIP(ctx, join1(AVK_END_CLASS_C));
        }
        a.n_work = (uint32_t)n - (t == 0 ? n_fast : 0u);
        a.high_priority = 0;
        a.esc_bytes = 0;
        a.esc_enabled = 0;
        /* pairs of a merge batch: the bulk launch is long (200,000 regions beside 10 M in the lanes) and its 40 KB workgroups do not all become resident while the
         * lane launches keep taking the LDS that comes free; a statically dealt share would wait for workgroups that start when the lanes are done
         * (12 or 22 ms per whole-genome merge, from call to call) — everything is claimed there */
        /* the same for every short list — the bulk beside the lane classes (a few thousand regions) and the overflow lists of the later tiers: same step,
         * fewer slow calls (tools/gpu_static_ab.py); a static share is for the first launch of a batch that goes through the wave-per-region kernels as a whole */
        a.static_pct = mode == 0 && t == 0 && a.n_work >= 16384u ? (uint32_t)ctx->static_pct : 0u; /* (50,000 single-call regions through the bulk: 0.40 ms with the static share, 0.43 without) */
        a.n_shards = 8;
        a.claim = (uint32_t)ctx->claim;
        return AVK_E_OK;
    }
    /* behind tier t's own launch: the next tier reads what this one handed over */
    int tier_end(int t, bool first_launch) {
        AVK_HIP(ctx, hipGetLastError());
        a.extra_counter = nullptr;
        a.extra_n = 0;
        if (first_launch && timed) AVK_HIP(ctx, hipEventRecord(ctx->evk1, ctx->stream)); /* ev0 sits right before it */
        if (t != last) {
            list = lists[nlist];
            count = db->d_counters + avk_ctr_overflow_count((uint32_t)nlist);
            nlist += 1;
        }
        return AVK_E_OK;
    }

    /* Solo launches: the regions the host predicted to outgrow the small slice are solved AT THE SAME TIME, on the
     * side stream, launched just before the bulk, so the long searches overlap with the bulk instead of forming
     * the tail of a later launch:
     *   class B (WorkPlan::n_hard): one-wave workgroups with a tier-1 LDS slice each; a solo workgroup's LDS
     *           displaces exactly one bulk workgroup;
     *   class C (WorkPlan::n_hbm):  predicted to outgrow tier 1 too: a small HBM-tier launch (its registers
     *           displace about two bulk workgroups per workgroup).
     * Both hand what they cannot hold to the list the first HBM launch of the main stream reads. */
    void solo_sizes() {
        const bool solo_ok = ctx->solo_blocks_max && geo.blocks >= 8;
        const bool hbm_solo_ok = solo_ok && launch[2] && db->plan.n_hbm;
        n_c = hbm_solo_ok ? db->plan.n_hbm : 0u;
        const uint32_t n_front = db->plan.n_hbm + db->plan.n_hard - n_c; /* predicted-hard records after them */
        if (solo_ok && use[1] && n_front &&
            (size_t)ctx->lds2_bytes_per_wave <= 2 * (size_t)AVK_WAVES_PER_BLOCK * (size_t)ctx->lds_bytes_per_wave) {
            solo = n_front < (uint32_t)ctx->solo_blocks_max ? n_front : (uint32_t)ctx->solo_blocks_max;
            if (solo > geo.blocks / 4) solo = geo.blocks / 4;
            const uint64_t cap = (uint64_t)solo * (uint64_t)ctx->solo_regions_per_wave;
            solo_regions = n_front < cap ? n_front : (uint32_t)cap; /* the others lead the bulk list */
        }
        if (n_c) hbm_solo = avk_solo_blocks(n_c, geo.hbm_solo_max);
    }

    /* a launch of the HBM-tier kernels beside the solo launch, on the chain of the records that are not the wide kernel's: its slices are the last xb workgroups' of
     * the solo launch's share (that launch gets the others) */
    int side_launch(bool team, AvkKernelArgs &x, uint32_t xb) {
        x.pass_tier = 2;
        x.high_priority = 1;
        x.n_waves = xb * AVK_WAVES_PER_BLOCK;
        x.hbm_ws = geo.share(ctx->d_ws, geo.side_wave(xb));
        avk_big_slice_args(x, ctx->d_big, db->d_counters, big_slots);
        AVK_HIP(ctx, fork(AVK_CH_NOT_WIDE, ctx->ev_fork));
        if (team) hipLaunchKernelGGL(avk_region_kernel_team, dim3(xb), dim3(256), 0, S(AVK_CH_NOT_WIDE), x);
        else hipLaunchKernelGGL(avk_region_kernel_hbm, dim3(xb), dim3(256), 0, S(AVK_CH_NOT_WIDE), x);
        AVK_HIP(ctx, hipGetLastError());
        AVK_HIP(ctx, record_end(AVK_END_NOT_WIDE, AVK_CH_NOT_WIDE));
        return AVK_E_OK;
    }

    /* class C: the wide launch with its companion and its retry, or a team launch for the head of the class; then the HBM solo launch for what is left */
    int class_c_chain() {
        if (solo || hbm_solo) AVK_HIP(ctx, hipEventRecord(ctx->ev_fork, ctx->stream)); /* after the memsets */
        if (!hbm_solo) return AVK_E_OK;
        /* how many of them are not the wide kernel's by their own record (a long window, many calls on a side): none or few in a genome, all of them in a
         * batch of large windows (--min-variant-gap 1000) — which then keeps the launches of round 3: every HBM wave on the whole list */
        const uint32_t n_nw = db->plan.n_hbm_notwide < n_c ? db->plan.n_hbm_notwide : n_c;
        const bool wide_c = use_wide && 2u * n_nw <= n_c; /* class C through avk_wide.inl first; the HBM launch behind it on this stream takes the list of what that could not take */
        if (wide_c && n_nw && !db->notwide_ready) { /* (only the class's wide launch with its companion reads the list) */
            /* the list of the class C records that are not avk_wide.inl's: once per batch, and the FIRST thing queued behind the fork — made behind the class's
             * wide launch its 20-170 workgroups waited for a place among the step's persistent waves (0.2 ms in a queued shard step, 1.2 ms in a merge call) */
            AVK_HIP(ctx, fork(AVK_CH_NOT_WIDE, ctx->ev_fork));
            AVK_HIP(ctx, hipMemsetAsync(db->d_notwide + n + 1, 0, sizeof(uint32_t), S(AVK_CH_NOT_WIDE)));
            hipLaunchKernelGGL(avk_notwide_list_kernel, dim3((n_c + 255u) / 256u), dim3(256), 0, S(AVK_CH_NOT_WIDE), db->d_regions, n_c, db->d_notwide, db->d_notwide + n + 1);
            AVK_HIP(ctx, hipGetLastError());
            db->notwide_ready = true;
        }
        const uint32_t *c_list = nullptr, *c_left = nullptr; /* what the launches of avk_wide.inl leave of class C (without them: the class's records themselves) */
        AVK_HIP(ctx, fork(AVK_CH_CLASS_C, ctx->ev_fork));
        uint32_t team_head = 0; /* records at the front of class C (most calls first) that a team launch takes */
        if (wide_c) {
            AvkKernelArgs w = a;
            w.work_list = nullptr;
            w.n_work_dev = nullptr;
            w.work_base = 0;
            w.n_work = n_c;
            w.work_counter = db->d_counters + AVK_CTR_WIDE_C_CURSOR;
            w.overflow_list = db->d_overflow5;
            w.overflow_count = db->d_counters + AVK_CTR_WIDE_C_LEFT;
            /* (512 one-wave workgroups for a genome's 6,000-15,000 records; a merge job's 42,000 lasted 7.2 ms on them, the longest launch of its step: one
             * workgroup per 32 records up to four times as many — profiles/r06_merge_step.txt) */
            uint32_t wb = (uint32_t)ctx->wide_blocks;
            if (!getenv("AVK_WIDE_BLOCKS") && n_c / 32u > wb) wb = n_c / 32u < 4u * wb ? n_c / 32u : 4u * wb;
            const uint32_t wg = n_c < wb ? n_c : wb;
            /* workgroups of the launch for the records that are not the wide kernel's (avk_side_split) */
            /* (a wave for each of these records and more: they lead the list, most calls first, and a wave that claimed four of them at a time solved four long
             * searches one after the other — 1.4 ms at the end of a rank's shard whose lanes were done after 0.8, profiles/r05_small_batches.txt) */
            uint32_t want = n_nw < hbm_solo ? n_nw : hbm_solo;
            want = want < 64u ? want : 64u;
            const uint32_t xb = avk_side_split(want, geo.hbm_solo_max, &hbm_solo);
            avk::wide::WideArgs wc = wa;
            wc.skip_static = xb ? 1u : 0u; /* (without the launch below such a record is handed over like any other) */
            hipLaunchKernelGGL(avk_wide_kernel, dim3(wg), dim3(64), (size_t)ctx->wide_lds_bytes, S(AVK_CH_CLASS_C), w, wc);
            AVK_HIP(ctx, hipGetLastError());
            if (xb) { /* the records of class C that are not for the wide kernel by what they say themselves (avk_wide_static_ok: a long window, many calls on a
               * side) start at the same time, on the HBM-tier kernel and a stream of their own: they are few and each of them is long */
                /* a wave per record, one claim each, from a list made just ahead of the launch (walking the whole class in claims of four, a wave solved the
                 * records of a claim one after the other: 2.06 -> 1.91 ms for the genome's 27, 0.96 -> 0.90 for a shard's 7) */
                /* (a wave per region here: these long windows hold a handful of calls, their searches are short chains where a team's hand-overs cost more
                 * than its parallel pieces give — shard 1.19 -> 1.31 ms, dense mix 2.29 -> 2.53 with teams, profiles/r06_team.txt) */
                AvkKernelArgs x = avk_list_reader_args(a, db->d_notwide, db->d_notwide + n + 1, db->d_counters + AVK_CTR_TEAM_CURSOR);
                const int rs = side_launch(false, x, xb);
                if (rs) return rs;
            }
            c_list = db->d_overflow5;
            c_left = db->d_counters + AVK_CTR_WIDE_C_LEFT;
            if (ctx->wide_retry_lds_bytes > ctx->wide_lds_bytes) {
                /* what it hands over at run time is nearly always a search that outgrew the 16 KB (nodes, wavefront blocks): once more with the LDS of a
                 * whole workgroup, a few waves — the wave-per-region kernel needs 2 ms for such a region, at the end of this chain */
                AvkKernelArgs w2 = w;
                w2.work_list = db->d_overflow5;
                w2.n_work_dev = db->d_counters + AVK_CTR_WIDE_C_LEFT;
                w2.work_base = 0;
                w2.n_work = 0;
                w2.work_counter = db->d_counters + AVK_CTR_WIDE_RETRY_CURSOR;
                w2.overflow_list = db->d_overflow8;
                w2.overflow_count = db->d_counters + AVK_CTR_WIDE_RETRY_LEFT;
                avk::wide::WideArgs wr = wa;
                wr.lds_words = (uint32_t)(ctx->wide_retry_lds_bytes / 4);
                hipLaunchKernelGGL(avk_wide_kernel, dim3(32), dim3(64), (size_t)ctx->wide_retry_lds_bytes, S(AVK_CH_CLASS_C), w2, wr);
                AVK_HIP(ctx, hipGetLastError());
                c_list = db->d_overflow8;
                c_left = db->d_counters + AVK_CTR_WIDE_RETRY_LEFT;
            }
        } else if (ctx->team_long_windows && ctx->team_head_regions > 0 && n_c > 1) {
            /* a batch of large windows (--min-variant-gap 1000: every region is class C and none is the wide kernel's): its step is as long as its few longest
             * searches — 0.25 s on one wave for 92 calls on 20 kbp while the other 49,000 regions need 0.05 s of the whole chip — so the head of the class, which
             * is sorted most calls first, gets a workgroup per region; the other launches start behind it in the list */
            const uint32_t want = n_c / 2u < (uint32_t)ctx->team_head_regions ? n_c / 2u : (uint32_t)ctx->team_head_regions;
            const uint32_t xb = avk_side_split(want, geo.hbm_solo_max, &hbm_solo);
            if (xb) {
                AvkKernelArgs x = avk_list_reader_args(a, nullptr, nullptr, db->d_counters + AVK_CTR_TEAM_CURSOR); /* (no list: the first xb records) */
                x.n_work = xb;
                x.team = (uint32_t)ctx->team_long_windows;
                const int rs = side_launch(true, x, xb);
                if (rs) return rs;
                team_head = xb;
            }
        }
        AvkKernelArgs s = avk_list_reader_args(a, c_list, c_left, db->d_counters + AVK_CTR_HBM_SOLO_TICKET);
        s.work_base = team_head;
        s.n_work = n_c - team_head;
        s.pass_tier = 2;
        s.high_priority = 1;
        s.n_waves = hbm_solo * AVK_WAVES_PER_BLOCK;
        s.hbm_ws = geo.share(ctx->d_ws, geo.solo_wave()); /* its own slices: the main stream's HBM launch may run beside it */
        avk_big_slice_args(s, ctx->d_big, db->d_counters, big_slots);
        /* same capacities as the last tier: what does not fit fails with CAPACITY */
        if (!big_slots && launch[3]) { /* the big tier has a launch of its own */
            s.overflow_list = lists[launch[1] ? 2 : 1];
            s.overflow_count = db->d_counters + avk_ctr_overflow_count(launch[1] ? 2 : 1);
        }
        hipLaunchKernelGGL(avk_region_kernel_hbm, dim3(hbm_solo), dim3(256), 0, S(AVK_CH_CLASS_C), s);
        AVK_HIP(ctx, hipGetLastError());
        AVK_HIP(ctx, record_end(AVK_END_CLASS_C, AVK_CH_CLASS_C));
        /* (the records of class C that are the wide launch's: the main stream's HBM launch has nothing to share) */
        shared_base = team_head;
        shared_n = wide_c ? 0u : db->plan.n_hbm - team_head;
        return AVK_E_OK;
    }

    /* class B, and the bulk's share of the list behind the solo launches */
    int lds_solo() {
        if (solo) {
            const int solo_list = launch[1] ? 1 : 0; /* the list the first HBM launch reads */
            const bool later = last > solo_list;
            AvkKernelArgs s = a;
            s.pass_tier = 1;
            s.work_base = n_c;
            s.n_work = solo_regions;
            s.work_counter = db->d_counters + AVK_CTR_LDS_SOLO_CURSOR;
            s.static_pct = 0;
            s.n_shards = 1;
            s.claim = 1;
            s.n_waves = solo;
            s.high_priority = 1;
            s.overflow_list = later ? lists[solo_list] : nullptr;
            s.overflow_count = later ? db->d_counters + avk_ctr_overflow_count((uint32_t)solo_list) : nullptr;
            AVK_HIP(ctx, fork(AVK_CH_LDS_SOLO, ctx->ev_fork));
            hipLaunchKernelGGL(avk_region_kernel_lds, dim3(solo), dim3(64), (size_t)ctx->lds2_bytes_per_wave, S(AVK_CH_LDS_SOLO), s);
            AVK_HIP(ctx, hipGetLastError());
            AVK_HIP(ctx, record_end(AVK_END_LDS_SOLO, AVK_CH_LDS_SOLO));
        }
        if (solo || hbm_solo) {
            a.work_base = n_c + solo_regions;
            a.n_work = (uint32_t)n - n_fast - n_c - solo_regions;
        }
        return AVK_E_OK;
    }

    HbSeg hb_new(uint32_t cap) {
        HbSeg g = {lists[2] + hb_off, db->d_counters + AVK_CTR_HB_COUNTS + hb_n, db->d_counters + AVK_CTR_HB_CURSORS + hb_n}; /* (hb_n < AVK_CTR_HB_SEGS: two chains, the staged heads, the pairs' list) */
        hb_off += cap;
        hb_n += 1;
        return g;
    }
    hipError_t hb_consume(hipStream_t st, const HbSeg &g) {
        AvkKernelArgs w = a;
        w.work_list = g.list;
        w.n_work_dev = g.count;
        w.work_base = 0;
        w.n_work = 0;
        w.work_counter = g.cursor;
        w.overflow_list = db->d_overflow7;
        w.overflow_count = db->d_counters + AVK_CTR_WIDE_LANES_LEFT;
        hipLaunchKernelGGL(avk_wide_kernel_lazy, dim3((uint32_t)ctx->wide_lazy_blocks), dim3(64), (size_t)ctx->wide_lds_bytes, st, w, wa);
        return hipGetLastError();
    }
    hipError_t use_lane_chain(int li) {
        if (lused[li]) return hipSuccess;
        lused[li] = true;
        return fork(lchain[li], ctx->ev_lane_fork);
    }

    /* the looked-up class (avk_pairs.inl): first on the stream of the one-call classes, BESIDE everything else.  (Alone it needs 0.18 ms;
     * beside the persistent waves of the other launches its workgroups wait for wave slots and it lasts 1.1 ms — in their shadow, which
     * measured better than 0.18 ms ahead of them: 3.95 against 4.2 ms per whole-genome step.) */
    int pair_launch(const AvkKernelArgs &f) {
        const int fc = AVK_FAST_PAIR;
        /* (AVK_PAIRS_OWN_STREAM=1: on the fourth lane stream with a hand-back list of its own, the one-call chain not waiting for it — a shard's step
         * 1.04 -> 1.00 ms, a genome's 2.33 -> 2.39: profiles/r06_handback_chains.txt) */
        const int li = chains && getenv("AVK_PAIRS_OWN_STREAM") ? 3 : 1;
        AVK_HIP(ctx, use_lane_chain(li));
        const int rt = ensure_pair_table(ctx, cfg->max_branch_factor, S(lchain[li]));
        if (rt) return rt;
        avk::pairs::PairArgs pa;
        pa.recs = db->d_fast + db->fast_word_base[fc];
        pa.n_tiles = db->fast_tiles[fc];
        pa.gen_base = db->plan.fast_base[fc];
        pa.tab = ctx->d_pair_tab;
        pa.tile_counter = db->d_counters + AVK_CTR_LANE_TILES + fc;
        uint32_t pg = (uint32_t)ctx->n_cus * (uint32_t)(ctx->pair_blocks_per_cu > 0 ? ctx->pair_blocks_per_cu : 1);
        const uint32_t claims = (pa.n_tiles + avk::pairs::PAIR_CLAIM - 1) / avk::pairs::PAIR_CLAIM;
        if (pg > (claims + 3u) / 4u) pg = (claims + 3u) / 4u;
        AvkKernelArgs fp = f;
        HbSeg pseg = chain_seg[1];
        if (chains && li == 3) pseg = hb_new(pa.n_tiles * 64u);
        if (chains) fp.overflow_list = pseg.list, fp.overflow_count = pseg.count;
        hipLaunchKernelGGL(avk_pair_kernel, dim3(pg), dim3(256), 0, S(lchain[li]), fp, pa);
        AVK_HIP(ctx, hipGetLastError());
        if (chains && li == 3) AVK_HIP(ctx, hb_consume(S(lchain[li]), pseg));
        return AVK_E_OK;
    }

    /* The three-call class gives up early on large searches (la.max_nodes): those regions are for whole wavefronts.
     * They get a list of their own and an HBM-tier launch right behind the class on its stream, so that they are
     * being solved while the other lane classes still run, not after them. */
    int three_call_launch(const AvkKernelArgs &f, const avk::lane::LaneArgs &la, uint32_t grid, size_t lds) {
        const int li = 2;
        hipStream_t es = S(lchain[li]); /* where the launch for the handed-back regions goes */
        AvkKernelArgs f3 = f;
        f3.overflow_list = lists[3];
        f3.overflow_count = db->d_counters + AVK_CTR_HB3_COUNT;
        launch_lane_class(ctx, grid, lds, es, f3, la);
        AVK_HIP(ctx, hipGetLastError());
        /* the launch for what ALL lanes hand back waits for the lane launches only, not for the launch behind this class */
        AVK_HIP(ctx, record_end(lend[li], lchain[li]));
        AvkKernelArgs e = avk_list_reader_args(a, lists[3], db->d_counters + AVK_CTR_HB3_COUNT, db->d_counters + AVK_CTR_HB3_CURSOR);
        e.pass_tier = 2;
        e.high_priority = 0;
        e.hbm_ws = geo.share(ctx->d_ws, geo.early_wave());
        avk_big_slice_args(e, ctx->d_big, db->d_counters, big_slots);
        const uint32_t eb = geo.hbm_blocks < geo.hbm_early_max ? geo.hbm_blocks : geo.hbm_early_max;
        if (use_wide) { /* large searches on small windows: avk_wide.inl first, the HBM-tier launch takes what is left */
            AvkKernelArgs w = e;
            w.work_counter = db->d_counters + AVK_CTR_WIDE_HB3_CURSOR;
            w.overflow_list = db->d_overflow6;
            w.overflow_count = db->d_counters + AVK_CTR_WIDE_HB3_LEFT;
            hipLaunchKernelGGL(avk_wide_kernel_lazy, dim3((uint32_t)ctx->wide_lazy_blocks), dim3(64), (size_t)ctx->wide_lds_bytes, es, w, wa);
            AVK_HIP(ctx, hipGetLastError());
            e.work_list = db->d_overflow6;
            e.n_work_dev = db->d_counters + AVK_CTR_WIDE_HB3_LEFT;
        }
        e.n_waves = eb * AVK_WAVES_PER_BLOCK;
        hipLaunchKernelGGL(avk_region_kernel_hbm_lazy, dim3(eb), dim3(256), 0, es, e);
        AVK_HIP(ctx, hipGetLastError());
        AVK_HIP(ctx, record_end(AVK_END_EARLY, lchain[li])); /* the caller's stream waits for this one at the end */
        return AVK_E_OK;
    }

    /* The head of a one- or two-call class — the tiles of regions with estimated edits, which the cost key puts first — in narrow tiles
     * of its own: lanes that diverge take turns, so 64 expensive regions in one wave take 64 turns; 16 per wave, four times as
     * many waves.  Same records, same stream, a launch ahead of the rest of the class. */
    int head_launch(const AvkKernelArgs &f, const avk::lane::LaneArgs &la, int fc, int li, uint32_t head_tiles, uint32_t pool_heavy) {
        const uint32_t maxv = AVK_FAST_CLASS[fc == AVK_FAST_PAIR ? 1 : fc].maxv;
        avk::lane::LaneArgs hd = la;
        hd.n_tiles = head_tiles;
        hd.tile_counter = db->d_counters + AVK_CTR_HEAD_TILES + fc;
        hd.lanes_log2 = head_width_log2(ctx, db->plan.n_fast_heavy[fc]);
        hd.pool = pool_heavy;
        uint32_t hgrid = 0;
        const size_t hlds = lane_launch_geometry(ctx, hd, &hgrid);
        const int hi = (maxv == 2 && ctx->lane_head_stream) ? 3 : li; /* a long head runs beside the rest of its class */
        AVK_HIP(ctx, use_lane_chain(hi));
        AvkKernelArgs fh = f;
        HbSeg hseg = {nullptr, nullptr, nullptr};
        static_assert(sizeof(avk_ctx::ev_hb) / sizeof(hipEvent_t) == AVK_CTR_HB_HEADS, "an event per staged head");
        const bool staged = chains && hb_heads < (int)AVK_CTR_HB_HEADS && (maxv == 2 || getenv("AVK_STAGE_ALL_HEADS")); /* (the one-call heads are short: their hand-backs wait for the chain's end) */
        if (staged) {
            hseg = hb_new(head_tiles * 64u);
            fh.overflow_list = hseg.list, fh.overflow_count = hseg.count;
        } else if (chains) {
            fh.overflow_list = chain_seg[li].list, fh.overflow_count = chain_seg[li].count;
        }
        const bool hb_follows = same_stream(lchain[hi], lchain[3]); /* the consumer follows its head in stream order: no event */
        launch_lane_class(ctx, hgrid, hlds, S(lchain[hi]), fh, hd, staged && !hb_follows ? ctx->ev_hb[hb_heads] : nullptr);
        AVK_HIP(ctx, hipGetLastError());
        if (staged) { /* its hand-backs: solved beside the rest of the class */
            if (!hb_follows) AVK_HIP(ctx, hipStreamWaitEvent(S(lchain[3]), ctx->ev_hb[hb_heads], 0));
            slot_forked[plan.slot[lchain[3]]] = true;
            lused[3] = true; /* (its first command waits for an event behind ev_lane_fork) */
            AVK_HIP(ctx, hb_consume(S(lchain[3]), hseg));
            hb_heads += 1;
        }
        return AVK_E_OK;
    }

    /* ---- the lane-per-region launches (avk_lane.inl): the classes with two calls per side (long, latency-bound tiles at low
     * occupancy) on a stream of their own, the one-call classes on the caller's stream ahead of the bulk.  What a lane cannot
     * finish goes to the DEFERRED list, solved after the bulk by an LDS launch of the wave-per-region kernel. */
    int lane_chains() {
        if (!use_fast) return AVK_E_OK;
        AvkKernelArgs f = a;
        f.overflow_list = lists[2];
        f.overflow_count = db->d_counters + avk_ctr_overflow_count(AVK_CTR_DEFERRED_LIST);
        AVK_HIP(ctx, hipEventRecord(ctx->ev_lane_fork, ctx->stream));
        chains = use_wide && ctx->wide_lane_handbacks && !ctx->lane_head_stream;
        if (chains) {
            uint32_t cap[2] = {0, 0};
            for (int fc = 0; fc < AVK_FAST_CLASSES; ++fc) {
                const uint32_t mv = fc == AVK_FAST_PAIR ? 1u : AVK_FAST_CLASS[fc].maxv;
                if (db->fast_tiles[fc] && mv <= 2) cap[mv == 2 ? 0 : 1] += db->fast_tiles[fc] * 64u;
            }
            chain_seg[0] = hb_new(cap[0]);
            chain_seg[1] = hb_new(cap[1]);
        }
        for (int fc = AVK_FAST_CLASSES - 1; fc >= 0; --fc) {
            if (!db->fast_tiles[fc]) continue;
            if (fc == AVK_FAST_PAIR && mode == 0 && ctx->lane_pairs) { /* looked up, not searched */
                const int rp = pair_launch(f);
                if (rp) return rp;
                continue;
            }
            /* (the looked-up class in merge mode or with the option off: its records are those of a one-call class) */
            const AvkFastClass &cl = fc == AVK_FAST_PAIR ? AVK_FAST_CLASS[1] : AVK_FAST_CLASS[fc];
            avk::lane::LaneArgs la;
            la.recs = db->d_fast + db->fast_word_base[fc];
            la.rec_words = AVK_FAST_WORDS_OF(cl.maxv);
            la.n_tiles = db->fast_tiles[fc];
            la.tile_counter = db->d_counters + AVK_CTR_LANE_TILES + fc;
            la.W = cl.W;
            la.nm = 1u << cl.maxv;
            la.ed_max = cl.ed_max;
            la.qcap = cl.qcap;
            la.gen_base = db->plan.fast_base[fc];
            la.lanes_log2 = lane_width_log2(ctx, cl.maxv);
            /* kept node states: where the expensive searches are — the three-call class and the heads of the others (16 records per wave: half a KB of LDS per
             * slot; in the 64-wide launches of the regions without estimated edits a slot would be 2 KB) */
            const uint32_t pool_heavy = ctx->lane_pool < 0 ? (la.nm == 2 ? 2u : (la.nm == 4 ? 4u : 6u)) /* lane_pool_default */ : (uint32_t)ctx->lane_pool;
            la.pool = ctx->lane_pool < 0 ? (cl.maxv > 2 ? pool_heavy : 0u) : (uint32_t)ctx->lane_pool;
            la.max_nodes = cl.maxv > 2 ? (uint32_t)ctx->lane_node_cap : 250u;
            la.max_ed_c = (uint32_t)ctx->lane_metrics_ed_cap;
            uint32_t grid = 0;
            const size_t lds = lane_launch_geometry(ctx, la, &grid);
            if (!lds) return fail(ctx, AVK_E_ARG, "lane kernel class %d does not fit the LDS", fc);
            const int li = cl.maxv == 2 ? 0 : (cl.maxv == 1 ? 1 : 2);
            AVK_HIP(ctx, use_lane_chain(li));
            if (cl.maxv > 2) {
                const int r3 = three_call_launch(f, la, grid, lds);
                if (r3) return r3;
                continue;
            }
            const uint32_t head_tiles = ctx->lane_head_width ? (db->plan.n_fast_heavy[fc] + 63u) / 64u : 0u;
            if (head_tiles > 0 && head_tiles < la.n_tiles && (uint32_t)ctx->lane_head_width < (1u << la.lanes_log2)) {
                const int rh = head_launch(f, la, fc, li, head_tiles, pool_heavy);
                if (rh) return rh;
                la.recs += (size_t)head_tiles * la.rec_words * 64u;
                la.n_tiles -= head_tiles;
                la.gen_base += head_tiles * 64u;
                if (grid > la.n_tiles) grid = la.n_tiles;
            }
            AvkKernelArgs fr = f;
            if (chains) fr.overflow_list = chain_seg[li].list, fr.overflow_count = chain_seg[li].count;
            launch_lane_class(ctx, grid, lds, S(lchain[li]), fr, la);
            AVK_HIP(ctx, hipGetLastError());
        }
        if (chains)
            for (int li = 0; li < 2; ++li)
                if (lused[li]) AVK_HIP(ctx, hb_consume(S(lchain[li]), chain_seg[li]));
        for (int li = 0; li < N_LS; ++li)
            if (lused[li] && !ends[lend[li]].seq) AVK_HIP(ctx, record_end(lend[li], lchain[li])); /* (the three-call class recorded its own ahead of its hand-backs) */
        if (lused[1] && timed) { /* end of the one-call classes' launches */
            AVK_HIP(ctx, hipEventRecord(ctx->ev_lane, S(lchain[1])));
            ctx->ev_lane_valid = true;
        }
        return AVK_E_OK;
    }

    /* the bulk launch on the caller's stream and, beside it, the launch for what the lanes handed back */
    int bulk_and_handbacks() {
        const uint32_t blocks = geo.blocks;
        /* the three launches are sized so that all their workgroups CAN be resident at once; with lane launches beside them they are not (a 40 KB LDS
         * allocation waits for a contiguous hole) — nothing waits for a workgroup to start, late ones find the claimed part of the list empty */
        uint32_t bulk = blocks > solo + 2 * hbm_solo + blocks / 4 ? blocks - solo - 2 * hbm_solo : blocks / 4; /* (a large class C launch: the bulk keeps a quarter of its workgroups) */
        if (bulk < 1) bulk = 1;
        if (bulk > blocks) bulk = blocks;
        if (ctx->bulk_full_grid) bulk = blocks;
        const uint32_t bulk_unfit = bulk; /* (the launch for the lanes' hand-backs below is sized by this) */
        if (ctx->bulk_fit && !ctx->bulk_full_grid) {
            const uint32_t fit = (a.n_work + AVK_WAVES_PER_BLOCK - 1) / AVK_WAVES_PER_BLOCK;
            if (bulk > fit) bulk = fit < 1 ? 1 : fit;
        }
        a.hbm_ws = nullptr;
        a.n_waves = bulk * AVK_WAVES_PER_BLOCK;
        const uint64_t slice0 = a.tier[0].ws_bytes;
        if (ctx->lds_bytes_per_wave >= 1024) { /* slices shrink to make room for the workgroup's tail */
            a.tier[0].ws_bytes = avk::bulk_slice_bytes((uint64_t)ctx->lds_bytes_per_wave);
            a.esc_bytes = (uint32_t)(AVK_WAVES_PER_BLOCK * a.tier[0].ws_bytes);
            a.esc_enabled = ctx->lds_escalation ? 1u : 0u;
        }
        hipLaunchKernelGGL(avk_region_kernel_lds, dim3(bulk), dim3(256), (size_t)AVK_WAVES_PER_BLOCK * (size_t)ctx->lds_bytes_per_wave, ctx->stream, a);
        if (use_fast) {
            /* The regions the lanes handed over: small ones, so the LDS tier with its in-workgroup escalation — on the one-call lane
             * stream, behind the lane launches, BESIDE the bulk and the HBM launch of this stream.  What overflows there (rare) goes to a
             * list of its own, read by one more HBM launch at the very end (normally empty: 10 us). */
            AVK_HIP(ctx, hipGetLastError());
            const int di = lused[1] ? 1 : (lused[0] ? 0 : 2);
            hipStream_t ds = S(lchain[di]);
            /* with chains every list has been through avk_wide.inl on its own stream; what that left is for the caller's stream at the end of the step (flush_chains) */
            if (!chains)
                for (int li = 0; li < N_LS; ++li)
                    if (li != di && lused[li] && !same_stream(lchain[li], lchain[di])) AVK_HIP(ctx, hipStreamWaitEvent(ds, ctx->ev_end[lend[li]], 0));
            AvkKernelArgs d = a;
            d.work_list = chains ? db->d_overflow7 : lists[2];
            d.n_work_dev = db->d_counters + (chains ? AVK_CTR_WIDE_LANES_LEFT : avk_ctr_overflow_count(AVK_CTR_DEFERRED_LIST));
            d.work_base = 0;
            d.n_work = 0;
            d.work_counter = db->d_counters + AVK_CTR_DEFERRED_CURSORS;
            if (!chains && use_wide && ctx->wide_lane_handbacks) { /* small windows, whatever made the lanes give up: avk_wide.inl first, the LDS launch takes what is left */
                AvkKernelArgs w = d;
                w.work_counter = db->d_counters + AVK_CTR_WIDE_LANES_CURSOR;
                w.overflow_list = db->d_overflow7;
                w.overflow_count = db->d_counters + AVK_CTR_WIDE_LANES_LEFT;
                hipLaunchKernelGGL(avk_wide_kernel_lazy, dim3((uint32_t)ctx->wide_lazy_blocks), dim3(64), (size_t)ctx->wide_lds_bytes, ds, w, wa);
                AVK_HIP(ctx, hipGetLastError());
                d.work_list = db->d_overflow7;
                d.n_work_dev = db->d_counters + AVK_CTR_WIDE_LANES_LEFT;
            }
            const uint32_t dblocks = bulk_unfit < (uint32_t)ctx->n_cus ? bulk_unfit : (uint32_t)ctx->n_cus; /* one workgroup per CU: the list is short */
            d.n_waves = dblocks * AVK_WAVES_PER_BLOCK;
            d.overflow_list = lists[1];
            d.overflow_count = db->d_counters + avk_ctr_overflow_count(1);
            if (chains) {
                chain_d = d;
                chain_dblocks = dblocks;
            } else {
                hipLaunchKernelGGL(avk_region_kernel_lds_lazy, dim3(dblocks), dim3(256), (size_t)AVK_WAVES_PER_BLOCK * (size_t)ctx->lds_bytes_per_wave, ds, d);
                AVK_HIP(ctx, hipGetLastError());
                AVK_HIP(ctx, record_end(AVK_END_DONE, lchain[di])); /* everything of the lane chains is behind this record */
            }
        }
        a.tier[0].ws_bytes = slice0;
        return AVK_E_OK;
    }

    /* tiers 1 to 3: one launch each on the caller's stream */
    void tier_launch(int t) {
        if (t == 1) { /* one workgroup per CU, four large slices */
            a.hbm_ws = nullptr;
            const uint32_t b2 = (uint32_t)ctx->n_cus < geo.blocks ? (uint32_t)ctx->n_cus : geo.blocks;
            a.n_waves = b2 * AVK_WAVES_PER_BLOCK;
            hipLaunchKernelGGL(avk_region_kernel_lds, dim3(b2), dim3(256), (size_t)AVK_WAVES_PER_BLOCK * (size_t)ctx->lds2_bytes_per_wave, ctx->stream, a);
        } else if (t == 2) {
            a.hbm_ws = geo.share(ctx->d_ws, geo.main_wave());
            avk_big_slice_args(a, ctx->d_big, db->d_counters, big_slots);
            a.n_waves = geo.hbm_blocks * AVK_WAVES_PER_BLOCK;
            if (pending(AVK_END_CLASS_C) && shared_n) { /* class C records the solo launch has not started yet: every wave of this launch helps (same ticket counter) */
                a.extra_counter = db->d_counters + AVK_CTR_HBM_SOLO_TICKET;
                a.extra_base = shared_base;
                a.extra_n = shared_n;
            }
            hipLaunchKernelGGL(avk_region_kernel_hbm, dim3(geo.hbm_blocks), dim3(256), 0, ctx->stream, a);
        } else {
            a.hbm_ws = ctx->d_big;
            a.big_slots = 0;
            a.n_waves = geo.big_blocks * AVK_WAVES_PER_BLOCK;
            hipLaunchKernelGGL(avk_region_kernel_hbm, dim3(geo.big_blocks), dim3(256), 0, ctx->stream, a);
        }
    }

    /* the launches of tier t, its own and (the first tier) everything that runs beside it */
    int tier(int t) {
        const bool first_launch = list == nullptr;
        int rc = tier_begin(t);
        if (rc) return rc;
        if (t == 0) {
            solo_sizes();
            if ((rc = class_c_chain()) || (rc = lds_solo()) || (rc = lane_chains()) || (rc = bulk_and_handbacks())) return rc;
        } else {
            tier_launch(t);
        }
        return tier_end(t, first_launch);
    }

    /* the end of the step: every chain the caller's stream has not waited for, the last HBM launch, the tally */
    int finish() {
        /* (no launch of an HBM tier's own — both tiers off — has flushed the chains: never with lanes today, use_fast asks for the tier-2 launch) */
        if (chains_unflushed()) AVK_HIP(ctx, flush_chains());
        const int at_end[5] = {AVK_END_LDS_SOLO, AVK_END_CLASS_C, AVK_END_NOT_WIDE, AVK_END_DONE, AVK_END_EARLY};
        AVK_HIP(ctx, join(at_end, 5));
        ctx->last_step_chains = chains;
        if (use_fast) { /* the lane chains (lane launches, then the handed-back regions) have joined; what even the escalation could not hold */
            AvkKernelArgs h = avk_list_reader_args(a, lists[1], db->d_counters + avk_ctr_overflow_count(1), db->d_counters + AVK_CTR_LAST_CURSOR);
            h.pass_tier = 2;
            h.high_priority = 0;
            h.hbm_ws = geo.share(ctx->d_ws, geo.main_wave());
            avk_big_slice_args(h, ctx->d_big, db->d_counters, big_slots);
            const uint32_t hb = geo.hbm_blocks < 64 ? geo.hbm_blocks : 64;
            h.n_waves = hb * AVK_WAVES_PER_BLOCK;
            hipLaunchKernelGGL(avk_region_kernel_hbm_lazy, dim3(hb), dim3(256), 0, ctx->stream, h);
            AVK_HIP(ctx, hipGetLastError());
        }
        hipLaunchKernelGGL(avk_tally_reduce, dim3((AVK_TALLY_STRIDE + 63) / 64), dim3(64), 0, ctx->stream, db->d_partials, db->d_tally,
                           (uint64_t *)tally_dev, db->d_counters, (unsigned)AVK_N_COUNTERS, ctx->accumulate_tally ? 1u : 0u);
        AVK_HIP(ctx, hipGetLastError());
        db->scratch_clean = true;
        db->last_cfg = *cfg;
        db->last_mode = mode;
        db->has_run = true;
        db->bp_valid = spec.emit_bp && mode == 0 && db->d_bp != nullptr;
        if (timed) AVK_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
        ctx->ev_valid = timed;
        return 0;
    }
};

static int run_internal(avk_ctx *ctx, const CallSpec &spec, avk_dev_batch *db, const avk_compare_config *cfg, void *tally_dev, uint32_t mode) {
    if (!ctx || !db || !cfg) return AVK_E_ARG;
    AVK_HIP(ctx, hipSetDevice(ctx->device));
    Step st(ctx, spec, db, cfg, tally_dev, mode);
    int rc = st.workspaces_and_outputs();
    if (!rc) rc = st.base_args();
    for (int t = 0; t < 4 && st.n && !rc; ++t)
        if (st.launch[t]) rc = st.tier(t);
    return rc ? rc : st.finish();
}
