/* The upload of a device-packed batch: the caller's arrays (in any of the five forms of avk_upload_forms.h) into HBM, the packing kernels of avk_devpack.inl, ONE small
 * state block back, the writers.  Included by avk_host.hip behind avk_devpack_host.inl (the pool, copy_in, the kernels and the strata launches are declared there).
 *
 *   Upload     what one upload knows while it queues its copies and launches: the source, the two streams, the packing kernels' arguments, the wide destination
 *              arrays, the buffers that go back to the pool at the end, and which steps the copies' hooks have queued already.  upload_device_packed makes one on its
 *              stack and calls its phases in order.
 *   phases     return 0, or the call's error code with everything of the upload released (bail). */

/* an exclusive prefix sum over cnt_a[i] + cnt_b[i] (cnt_b may be NULL) in three launches on `side`: sums[] takes a word per AVK_PS_BLOCK entries, *total the sum */
static void queue_prefix_sum(hipStream_t side, const uint8_t *cnt_a, const uint8_t *cnt_b, uint64_t count, uint64_t *sums, uint64_t *total, uint64_t *out) {
    if (!count) return;
    const uint32_t nb = (uint32_t)((count + AVK_PS_BLOCK - 1) / AVK_PS_BLOCK);
    hipLaunchKernelGGL(avk_ps_block_sums_kernel, dim3(nb), dim3(256), 0, side, cnt_a, cnt_b, count, sums);
    hipLaunchKernelGGL(avk_ps_scan_sums_kernel, dim3(1), dim3(1024), 0, side, sums, nb, total);
    hipLaunchKernelGGL(avk_ps_apply_kernel, dim3(nb), dim3(256), 0, side, cnt_a, cnt_b, count, (const uint64_t *)sums, out);
}

struct Upload {
    typedef std::chrono::steady_clock::time_point Time;
    avk_ctx *const ctx;
    const CallSpec &spec;
    const UploadSource &src;
    const PackedOnDevice *const pre; /* a packed batch whose arrays are in a staging slot already */
    const uint64_t n, nv, alen;
    const bool has_esc, has_contig, has_raw, timing;
    const hipStream_t s;    /* (the asynchronous boundary packs on a stream of its own, beside the solve of the batch before) */
    const hipStream_t side; /* the side stream of the upload: prefix sums, widening, dp_variant under the copies, the cleared scratch */
    const uint32_t n_blocks;
    avk_dev_batch *db;
    std::vector<void *> temps; /* released (to the pool) at the end of the upload */
    int rc = 0;
    hipError_t e = hipSuccess; /* of the packing kernels, from dp_variant to the second round of the region passes: checked once, by check_state */
    dpk::DpArgs a;
    dpk::DpEsc de;
    std::vector<CopySeg> esc_segs;
    /* the caller's arrays in HBM, wide (NULL for a batch read from its packed source); the four that dp_unpack reads after the solve stay with the batch (db->d_in_*) */
    uint64_t *d_start = nullptr, *d_end = nullptr, *d_pos = nullptr, *d_a0o = nullptr, *d_a1o = nullptr;
    uint32_t *d_contig = nullptr, *d_a0l = nullptr, *d_a1l = nullptr, *d_raw = nullptr;
    uint8_t *d_type = nullptr, *d_zyg = nullptr, *d_alleles = nullptr;
    uint64_t *d_block_sums = nullptr;
    uint64_t *pk_totals = nullptr; /* packed forms: device words {sum of the call counts, sum of the allele lengths, with escapes: the error word} */
    struct { /* the packed forms' arrays in HBM as they came (multi: tc = in_cnt, qc = NULL, voff = in_off), the offsets they leave out, the prefix sums' block sums */
        uint16_t *contig, *len, *rel;
        uint32_t *start;
        uint8_t *tc, *qc, *tz, *a0, *a1;
        uint64_t *voff, *aoff, *sums;
        uint32_t nb_r, nb_v;
    } p;
    uint32_t *m_contig = nullptr; /* the merge forms' MultiRegions, wide */
    uint64_t *m_start = nullptr, *m_end = nullptr;
    /* the route */
    bool packed_src = false;  /* a compare batch in the packed form is read from the packed arrays themselves (DpIn::pk_*): no wide arrays, no widening pass */
    bool queue_early = false; /* the side stream's steps are queued from inside copy_in (option pack_queue_early, and always on the chunked route) */
    avk::pc::ChunkPlan chunk_plan = avk::pc::plan_chunks(0, 0, 0, 0); /* k > 0: the chunked route (option pack_chunks): the region pass runs on the side stream, group by group */
    bool variant_done = false; /* dp_variant queued on the side stream of a packed upload, under its copies */
    bool region_done = false;  /* ... and the region pass too: the first round of region_passes launches none */
    hipError_t hook_err = hipSuccess; /* of the steps queued from inside copy_in */
    uint32_t tiles_total = 0;
    Time t_start, t_alloc, t_copy, t_plan;

    Upload(avk_ctx *c, const CallSpec &sp, const UploadSource &u, const PackedOnDevice *pr)
        : ctx(c), spec(sp), src(u), pre(pr), n(u.n_regions()), nv(u.n_variants()), alen(u.allele_bytes_len()), has_esc(u.has_esc()), has_contig(u.has_contig()),
          has_raw(u.has_raw()), timing(getenv("AVK_TIMING") != nullptr), s(sp.up_stream ? sp.up_stream : c->stream), side(sp.up_side ? sp.up_side : c->lane_stream4),
          n_blocks((uint32_t)((n + 255) / 256)), db(new avk_dev_batch()) {
        t_start = now();
        memset(&a, 0, sizeof(a));
        memset(&de, 0, sizeof(de));
        memset(&p, 0, sizeof(p));
        db->dev_packed = true;
        db->n_regions = n;
        db->n_variants_host = nv;
        packed_src = src.form == UploadSource::PACKED && ctx->packed_source && !has_esc; /* (a batch with escapes is widened first: dp_widen_packed_esc) */
        ctx->last_region_launches = 0, ctx->tl_region_valid = false;
    }

    static Time now() { return std::chrono::steady_clock::now(); }
    static double ms(Time x, Time y) { return std::chrono::duration<double, std::milli>(y - x).count(); }
    dpk::DpState *hs() const { return (dpk::DpState *)ctx->h_dpstate; }

    /* ---- buffers ---- */
    void *tmp(size_t bytes) {
        void *q = nullptr;
        if (!rc) rc = pool_alloc(ctx, &q, bytes);
        if (q) temps.push_back(q);
        return q;
    }
    void *kept(size_t bytes) { /* (the inputs and the packer's intermediates stay with the batch: region records of lane regions are written when a launch needs them) */
        void *q = nullptr;
        if (!rc) rc = pool_alloc(ctx, &q, bytes);
        if (q) db->pooled.push_back(q);
        return q;
    }
    void *wide(size_t bytes) { return packed_src ? nullptr : kept(bytes); }
    /* (the packed arrays stay with the batch when they are what the packer and the later record writers read; a staging slot's stay with its ticket) */
    void *packed_buf(size_t bytes) { return packed_src ? kept(bytes) : tmp(bytes); }
    int bail(int code) { /* nothing of this call may still be in flight on either stream when its buffers go back */
        (void)hipStreamSynchronize(s);
        (void)hipStreamSynchronize(side);
        for (void *q : temps) pool_release(ctx, q);
        release_pooled(ctx, db);
        delete db;
        db = nullptr;
        return code;
    }
    int bail_hip(const char *what, hipError_t x) { return bail(fail(ctx, AVK_E_HIP, "%s: %s", what, hipGetErrorString(x))); }

    /* ---- AVK_TIMING ---- */
    void mark(int k) { /* a mark of the call's device timeline on the context's stream */
        if (!timing) return;
        if (!ctx->ev_tl[k] && hipEventCreate(&ctx->ev_tl[k]) != hipSuccess) {
            ctx->ev_tl[k] = nullptr;
            (void)hipGetLastError();
            return;
        }
        (void)hipEventRecord(ctx->ev_tl[k], s);
    }
    void record_region_mark(hipStream_t stream) { /* ... and of the end of the region pass, on the stream that ran it */
        if (!timing) return;
        if (!ctx->ev_tl[5] && hipEventCreate(&ctx->ev_tl[5]) != hipSuccess) ctx->ev_tl[5] = nullptr, (void)hipGetLastError();
        if (ctx->ev_tl[5] && hipEventRecord(ctx->ev_tl[5], stream) == hipSuccess) ctx->tl_region_valid = true;
    }

    /* ---- the wide outputs of the widening kernels (DpPacked, DpCompact, DpPairs: per region; DpPacked, DpCompact, DpPackedMulti: per call) ---- */
    template <typename C> void wide_region_outputs(C &c) const {
        c.w_contig = d_contig, c.w_t_cnt = db->d_in_t_cnt, c.w_q_cnt = db->d_in_q_cnt, c.w_start = d_start, c.w_end = d_end, c.w_t_off = db->d_in_t_off, c.w_q_off = db->d_in_q_off;
    }
    template <typename C> void wide_call_outputs(C &c) const {
        c.w_a0_len = d_a0l, c.w_a1_len = d_a1l, c.w_raw = nullptr, c.w_pos = d_pos, c.w_a0_off = d_a0o, c.w_a1_off = d_a1o, c.w_type = d_type, c.w_zyg = d_zyg;
    }

    int alloc_inputs() {
        d_start = (uint64_t *)wide((n + 1) * 8), d_end = (uint64_t *)wide((n + 1) * 8);
        db->d_in_t_off = (uint64_t *)wide((n + 1) * 8), db->d_in_q_off = (uint64_t *)wide((n + 1) * 8);
        db->d_in_t_cnt = (uint32_t *)wide((n + 1) * 4), db->d_in_q_cnt = (uint32_t *)wide((n + 1) * 4);
        d_contig = has_contig ? (uint32_t *)wide((n + 1) * 4) : nullptr;
        d_pos = (uint64_t *)wide((nv + 1) * 8), d_a0o = (uint64_t *)wide((nv + 1) * 8), d_a1o = (uint64_t *)wide((nv + 1) * 8);
        d_a0l = (uint32_t *)wide((nv + 1) * 4), d_a1l = (uint32_t *)wide((nv + 1) * 4);
        d_raw = has_raw ? (pre ? pre->raw : (uint32_t *)kept((nv + 1) * 4)) : nullptr;
        d_type = (uint8_t *)wide(nv + 16), d_zyg = (uint8_t *)wide(nv + 16), d_alleles = pre ? pre->alleles : (uint8_t *)kept(alen + 16);
        /* intermediates */
        a.vinfo = (dpk::DpVarInfo *)kept((nv + 1) * sizeof(dpk::DpVarInfo));
        a.rinfo = (dpk::DpRegionInfo *)kept((n + 1) * sizeof(dpk::DpRegionInfo));
        a.st = (dpk::DpState *)kept(sizeof(dpk::DpState));
        a.pending = (uint32_t *)tmp((nv + 1) * 4);
        a.slots = (dpk::DpSlot *)tmp((nv + 1) * sizeof(dpk::DpSlot));
        a.bucket16 = (uint16_t *)tmp((n + 16) * 2);
        db->d_voff = (uint32_t *)kept((n + 1) * 4);
        a.v_off = db->d_voff;
        a.blob_off8 = (uint32_t *)kept((n + 1) * 4);
        a.seq_off = (uint64_t *)kept((n + 1) * 8);
        db->d_bp_off = (uint32_t *)kept((n + 2) * 4);
        a.bp_off = db->d_bp_off;
        if (db->d_bp_off) (void)hipMemsetAsync(db->d_bp_off, 0, 8, s); /* (an empty batch: bp_off[0] = 0) */
        a.order = (uint32_t *)kept((n + 1) * 4);
        a.big_list = (uint32_t *)kept((n + 1) * 4);
        d_block_sums = (uint64_t *)tmp(((size_t)n_blocks + 1) * AVK_DP_BS * 8);
        if (!ctx->h_dpstate && !rc) {
            hipError_t x = hipHostMalloc((void **)&ctx->h_dpstate, sizeof(dpk::DpState) + 32, hipHostMallocDefault);
            if (x != hipSuccess) rc = fail(ctx, AVK_E_HIP, "pinned state block: %s", hipGetErrorString(x));
        }
        if (!ctx->d_contig_tab && !rc) rc = fail(ctx, AVK_E_STATE, "avk_ref_upload has not been called");
        if (rc) return bail(rc);
        t_alloc = now();
        mark(0);
        return 0;
    }

    /* the escape lists of a packed batch in HBM (a staging slot's, or copied with the batch's arrays), and the two exclusive sums over their values */
    int stage_escapes() {
        if (!has_esc) return 0;
        const avk_packed_escapes *esc = src.esc;
        const uint64_t er = esc->n_esc_regions, es = esc->n_esc_slots, ec = esc->n_esc_calls;
        de.region = pre ? pre->esc_region : (uint64_t *)tmp((er + 1) * 8), de.slot = pre ? pre->esc_slot : (uint64_t *)tmp((es + 1) * 8);
        de.call = pre ? pre->esc_call : (uint64_t *)tmp((ec + 1) * 8);
        de.len = pre ? pre->esc_len : (uint32_t *)tmp((er + 1) * 4), de.cnt = pre ? pre->esc_cnt : (uint32_t *)tmp((es + 1) * 4), de.rel = pre ? pre->esc_rel : (uint32_t *)tmp((ec + 1) * 4);
        de.a0 = pre ? pre->esc_a0 : (uint32_t *)tmp((ec + 1) * 4), de.a1 = pre ? pre->esc_a1 : (uint32_t *)tmp((ec + 1) * 4);
        de.cnt_before = (uint64_t *)tmp((es + 1) * 8), de.bytes_before = (uint64_t *)tmp((ec + 1) * 8);
        de.n_regions = er, de.n_slots = es, de.n_calls = ec, de.first_region = esc->first_region, de.first_slot = esc->first_slot, de.first_call = esc->first_call;
        if (rc) return bail(rc);
        if (!pre)
            esc_segs = {{esc->esc_region, (void *)de.region, er * 8}, {esc->esc_len, (void *)de.len, er * 4}, {esc->esc_slot, (void *)de.slot, es * 8}, {esc->esc_cnt, (void *)de.cnt, es * 4},
                        {esc->esc_call, (void *)de.call, ec * 8}, {esc->esc_rel_pos, (void *)de.rel, ec * 4}, {esc->esc_a0_len, (void *)de.a0, ec * 4}, {esc->esc_a1_len, (void *)de.a1, ec * 4}};
        return 0;
    }
    /* (side stream, behind the sums over the narrow arrays and the lists' copies) the lists are checked and summed; totals[0..1] gain what the narrow sums lack, totals[2] is the error word */
    void esc_scans(uint64_t *totals, uint64_t n_slots_all, uint64_t n_calls_all, uint64_t n_regions_all, const dpk::DpEscNarrow &z_slot, const dpk::DpEscNarrow &z_call,
                   const dpk::DpEscNarrow &z_region) {
        hipLaunchKernelGGL(avk_esc_scan_kernel, dim3(1), dim3(1024), 0, side, de.slot, de.cnt, (const uint32_t *)nullptr, de.n_slots, de.first_slot, de.first_slot + n_slots_all,
                           z_slot, (uint64_t *)de.cnt_before, totals, totals + 2);
        hipLaunchKernelGGL(avk_esc_scan_kernel, dim3(1), dim3(1024), 0, side, de.call, de.a0, de.a1, de.n_calls, de.first_call, de.first_call + n_calls_all, z_call,
                           (uint64_t *)de.bytes_before, totals + 1, totals + 2);
        hipLaunchKernelGGL(avk_esc_scan_kernel, dim3(1), dim3(1024), 0, side, de.region, (const uint32_t *)nullptr, (const uint32_t *)nullptr, de.n_regions, de.first_region,
                           de.first_region + n_regions_all, z_region, (uint64_t *)nullptr, (uint64_t *)nullptr, totals + 2);
    }
    /* the caller's arrays (the wide ones: NULL for a batch read from its packed source) and the context's options, as the packing kernels take them */
    void fill_args() {
        a.in.contig_idx = d_contig, a.in.start = d_start, a.in.end = d_end, a.in.t_off = db->d_in_t_off, a.in.q_off = db->d_in_q_off, a.in.t_cnt = db->d_in_t_cnt,
        a.in.q_cnt = db->d_in_q_cnt, a.in.var_pos = d_pos, a.in.var_type = d_type, a.in.var_zyg = d_zyg, a.in.var_raw = d_raw, a.in.a0_off = d_a0o, a.in.a1_off = d_a1o,
        a.in.a0_len = d_a0l, a.in.a1_len = d_a1l, a.in.alleles = d_alleles, a.in.n_regions = n, a.in.n_variants = nv, a.in.alleles_len = alen,
        a.in.contig_base = ctx->d_contig_tab, a.in.contig_len = ctx->d_contig_tab + ctx->contig_len.size(), a.in.n_contigs = (uint32_t)ctx->contig_len.size(),
        a.in.pairs_mode = src.pairs_mode ? 1u : 0u;
        const bool lanes = ctx->lane_kernel && ctx->use_packed_reference && ctx->d_ref2b;
        a.opt.tier0_bytes = avk::bulk_slice_bytes((uint64_t)ctx->lds_bytes_per_wave), a.opt.tier0_ed_cap = (uint32_t)ctx->lds_ed_cap, a.opt.tier1_bytes = (uint64_t)ctx->lds2_bytes_per_wave,
        a.opt.tier1_ed_cap = (uint32_t)ctx->lds2_ed_cap, a.opt.solo_min_variants = src.pairs_mode && !ctx->pair_classes ? 0u : (uint32_t)ctx->solo_min_variants, a.opt.max_branch = 50,
        a.opt.class_c_nodes_x2 = (uint32_t)ctx->class_c_nodes_x2, a.opt.lane_min_regions = lanes ? (uint64_t)ctx->lane_min_regions : 0xFFFFFFFFull,
        a.opt.lane_max_calls = (uint32_t)ctx->lane_max_calls, a.opt.lane_min_batch = (uint64_t)ctx->lane_min_batch, a.opt.lane_max_est = (uint32_t)ctx->lane_max_est;
        a.opt.stripe_w = ctx->lane_stripe ? (uint32_t)ctx->lane_head_width : 0u;
        a.opt.lane_pairs = ctx->lane_pairs ? 1u : 0u;
        a.opt.head_est = (uint32_t)ctx->lane_head_est, a.opt.het_min = (uint32_t)ctx->het_search_min;
        a.opt.class_c_below = (uint64_t)ctx->class_c_below;
    }
    void name_packed_source() { /* the packer reads these as they are */
        a.in.pk_start = p.start, a.in.pk_len = p.len, a.in.pk_contig = p.contig, a.in.pk_rel = p.rel, a.in.pk_tc = p.tc, a.in.pk_qc = p.qc, a.in.pk_tz = p.tz, a.in.pk_a0 = p.a0,
        a.in.pk_a1 = p.a1, a.in.pk_voff = p.voff, a.in.pk_aoff = p.aoff;
    }

    /* ---- the packed form: the packed arrays as they are, two prefix sums for the offsets they leave out, one kernel that writes the wide arrays ----
     * All copies on the context's stream, counts and lengths first; the two prefix sums (which need nothing else) and the widening kernel (everything but the
     * allele bytes) run on a stream of their own beside the copies that follow: dp_variant, the first kernel that needs every byte, starts 0.24 ms earlier.
     * (The copies themselves stay on ONE stream: a large copy queued on a second stream now and then blocks the host for 7 to 9 ms inside hipMemcpyAsync —
     * the runtime bringing up another copy engine — which made one call in fifty 16 ms long.) */
    int copy_packed() {
        p.contig = has_contig ? (pre ? pre->contig : (uint16_t *)packed_buf((n + 1) * 2)) : nullptr, p.len = pre ? pre->len : (uint16_t *)packed_buf((n + 1) * 2);
        p.rel = pre ? pre->rel_pos : (uint16_t *)packed_buf((nv + 1) * 2);
        p.start = pre ? pre->start : (uint32_t *)packed_buf((n + 1) * 4);
        p.tc = pre ? pre->t_cnt : (uint8_t *)packed_buf(n + 16), p.qc = pre ? pre->q_cnt : (uint8_t *)packed_buf(n + 16), p.tz = pre ? pre->var_type_zyg : (uint8_t *)packed_buf(nv + 16);
        p.a0 = pre ? pre->a0_len : (uint8_t *)packed_buf(nv + 16), p.a1 = pre ? pre->a1_len : (uint8_t *)packed_buf(nv + 16);
        p.nb_r = (uint32_t)((n + AVK_PS_BLOCK - 1) / AVK_PS_BLOCK), p.nb_v = (uint32_t)((nv + AVK_PS_BLOCK - 1) / AVK_PS_BLOCK);
        p.voff = (uint64_t *)packed_buf((n + 1) * 8), p.aoff = (uint64_t *)packed_buf((nv + 1) * 8), p.sums = (uint64_t *)tmp(((size_t)p.nb_r + p.nb_v + 4) * 8);
        if (rc) return bail(rc);
        if (int c = choose_packed_route()) return c;
        if (pre) rc = copy_packed_staged();
        else if (chunk_plan.k) rc = copy_packed_chunked();
        else rc = copy_packed_in_order();
        mark(1);
        if (rc) return bail(rc);
        const hipError_t ec = queue_early ? hook_err : queue_sums(); /* (queued early: they stand behind the lengths' copy already) */
        if (ec != hipSuccess) return bail_hip("packed upload", ec);
        return widen_packed();
    }
    /* The chunked route (option pack_chunks) is for the synchronous call on pinned arrays that is read from its packed source and copies by engine: a staging slot's
     * arrays are there already, a batch with escapes is widened first, pageable arrays cross piece by piece through the bounce buffer, and avk_copy_kernel occupies
     * the compute units the region pass would run on.  Everything else keeps the old order, launch for launch. */
    bool all_pinned() const {
        const avk_packed_batch *pk = src.packed;
        return is_pinned(pk->t_cnt, n) && is_pinned(pk->q_cnt, n) && is_pinned(pk->a0_len, nv) && is_pinned(pk->a1_len, nv) && is_pinned(pk->allele_bytes, alen) &&
               is_pinned(pk->start, n * 4) && is_pinned(pk->len, n * 2) && is_pinned(pk->contig_idx, n * 2) && is_pinned(pk->var_rel_pos, nv * 2) &&
               is_pinned(pk->var_type_zyg, nv) && is_pinned(pk->var_raw_space, nv * 4);
    }
    int choose_packed_route() {
        queue_early = (ctx->pack_chunks > 0 || ctx->pack_queue_early) && packed_src && nv && !pre && !spec.up_stream && !copies_by_kernel(ctx) && all_pinned();
        if (!queue_early || ctx->pack_chunks <= 0) return 0;
        chunk_plan = avk::pc::plan_chunks(n, nv, ctx->pack_chunks, (uint64_t)ctx->pack_chunk_floor);
        for (uint32_t j = 0; j + 1 < chunk_plan.k && !rc; ++j)
            if (!ctx->ev_pack_group[j] && hipEventCreateWithFlags(&ctx->ev_pack_group[j], hipEventDisableTiming) != hipSuccess) {
                ctx->ev_pack_group[j] = nullptr;
                rc = fail(ctx, AVK_E_HIP, "packed upload: %s", hipGetErrorString(hipGetLastError()));
            }
        return rc ? bail(rc) : 0;
    }
    hipError_t queue_sums() { /* the two prefix sums, on the side stream behind the counts and lengths */
        hipError_t ec = hipStreamWaitEvent(side, ctx->ev_copy_fork, 0); /* (also orders the side stream behind everything queued on the context's stream before) */
        if (ec != hipSuccess) return ec;
        uint64_t *totals = p.sums + p.nb_r + p.nb_v;
        if (has_esc && hipMemsetAsync(totals, 0, 32, side) != hipSuccess) return hipGetLastError();
        queue_prefix_sum(side, p.tc, p.qc, src.form == UploadSource::PACKED ? n : src.n_multi() * src.n_inputs(), p.sums, totals, p.voff);
        queue_prefix_sum(side, p.a0, p.a1, nv, p.sums + p.nb_r, totals + 1, p.aoff);
        return hipGetLastError();
    }
    /* Variant::alt_ed for every call, on the side stream behind the prefix sums and the allele bytes, while the region arrays still cross the bus: the state
     * block is cleared here (dp_variant counts the calls it leaves to the host); the context's stream waits for ev_copy_join below as before */
    hipError_t queue_variant() {
        a.in.pk_a0 = p.a0, a.in.pk_a1 = p.a1, a.in.pk_aoff = p.aoff, a.in.pk_start = p.start; /* (what dp_variant reads of the packed source; the rest follows below) */
        a.in.alleles = d_alleles, a.in.n_variants = nv, a.in.alleles_len = alen, a.in.n_regions = n;
        hipError_t ev = hipMemsetAsync(a.st, 0, sizeof(dpk::DpState), side);
        if (ev == hipSuccess) ev = hipStreamWaitEvent(side, ctx->ev_copy_alleles, 0);
        if (ev == hipSuccess) {
            hipLaunchKernelGGL(avk_dp_variant_kernel, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, side, a);
            ev = hipGetLastError();
        }
        variant_done = ev == hipSuccess;
        return ev;
    }
    /* The chunked route's region pass: launch j on the side stream behind dp_variant, the prefix sums and the event of group j; each block is run by exactly one
     * launch (pc_launch_of_block), the catch-all behind the last group runs what none took.  block_sums and the region info are what the one launch writes.
     *
     * WHEN these are queued matters as much as what they wait for.  The runtime maps the context's streams onto a few hardware queues, a queue takes its packets in
     * order, and every event recorded behind a copy is a packet that holds its queue until that copy is done.  Queued after copy_in has returned, the side stream's
     * kernels sit — where the side stream shares the copy stream's queue — behind the packet of the LAST copy and start when it ends: a kernel trace of the old
     * order shows the prefix sums and dp_variant starting 18 us after the last copy, whatever their events say (profiles/pack_chunks_ab.txt).  So each step is queued
     * from copy_in itself, right behind the record of the event it waits for (CopySeg::then_call, the three hooks below): in a shared queue it then stands in front of
     * the later copies' packets, in a queue of its own nothing changes. */
    void hook_sums() { hook_err = queue_sums(); }
    void hook_variant() {
        if (hook_err == hipSuccess) hook_err = queue_variant();
    }
    void hook_chunk(uint32_t j) {
        if (hook_err != hipSuccess) return;
        const bool last = j + 1 == chunk_plan.k;
        hook_err = hipStreamWaitEvent(side, last ? ctx->ev_copy_mid : ctx->ev_pack_group[j], 0);
        for (uint32_t l = j; l <= (last ? j + 1 : j) && hook_err == hipSuccess; ++l) { /* (behind the last group: the catch-all, l = k) */
            const uint32_t grid = l < chunk_plan.k ? chunk_plan.block_cut[l + 1] : n_blocks;
            hipLaunchKernelGGL(avk_dp_region_chunk_kernel, dim3(grid ? grid : 1u), dim3(256), 0, side, a, d_block_sums, chunk_plan, l, n_blocks);
            hook_err = hipGetLastError();
            ctx->last_region_launches += 1;
        }
        if (!last || hook_err != hipSuccess) return;
        record_region_mark(side);
        hook_err = hipEventRecord(ctx->ev_copy_join, side);
        region_done = hook_err == hipSuccess;
    }
    void hook_sums_and_variant(std::vector<CopySeg> &segs) { /* behind the second length array (ev_copy_fork) and the allele bytes (ev_copy_alleles) */
        segs[3].then_call = [this] { hook_sums(); };
        segs[4].then_call = [this] { hook_variant(); };
    }
    /* counts, lengths and the allele bytes, the copies every route starts with (the allele bytes cross right behind the lengths — dp_variant needs nothing else) */
    std::vector<CopySeg> packed_head_segs() const {
        const avk_packed_batch *pk = src.packed;
        return {{pk->t_cnt, p.tc, n}, {pk->q_cnt, p.qc, n}, {pk->a0_len, p.a0, nv}, {pk->a1_len, p.a1, nv, nullptr, ctx->ev_copy_fork},
                {pk->allele_bytes, d_alleles, alen, nullptr, ctx->ev_copy_alleles}};
    }
    int copy_packed_staged() { /* the arrays are in a staging slot already (or on their way there on the copy stream) */
        hipError_t ep = hipStreamWaitEvent(s, pre->ready, 0);
        if (ep == hipSuccess) ep = hipEventRecord(ctx->ev_copy_fork, s);
        if (ep == hipSuccess) ep = hipEventRecord(ctx->ev_copy_mid, s);
        if (ep == hipSuccess) ep = hipEventRecord(ctx->ev_copy_alleles, s);
        return ep == hipSuccess ? 0 : fail(ctx, AVK_E_HIP, "packed upload: %s", hipGetErrorString(ep));
    }
    /* the chunked route: counts, lengths and allele bytes, then group by group: region range j of the per-region arrays, call chunk j of the per-call arrays, an
     * event; the last group's event is ev_copy_mid */
    int copy_packed_chunked() {
        const avk_packed_batch *pk = src.packed;
        fill_args(); /* (the launches are queued from inside copy_in: everything dp_region reads is named now) */
        name_packed_source();
        a.in.v_lo = 0, a.in.v_hi = nv;
        std::vector<CopySeg> segs = packed_head_segs();
        hook_sums_and_variant(segs);
        for (uint32_t j = 0; j < chunk_plan.k; ++j) {
            const avk::pc::Range rr = avk::pc::pc_region_range(chunk_plan, j), cr = avk::pc::pc_call_range(chunk_plan, j);
            segs.push_back({pk->start + rr.first, p.start + rr.first, rr.count * 4});
            segs.push_back({pk->len + rr.first, p.len + rr.first, rr.count * 2});
            segs.push_back({has_contig ? pk->contig_idx + rr.first : nullptr, has_contig ? p.contig + rr.first : nullptr, has_contig ? rr.count * 2 : 0});
            segs.push_back({pk->var_rel_pos + cr.first, p.rel + cr.first, cr.count * 2});
            segs.push_back({pk->var_type_zyg + cr.first, p.tz + cr.first, cr.count});
            segs.push_back({has_raw ? pk->var_raw_space + cr.first : nullptr, has_raw ? d_raw + cr.first : nullptr, has_raw ? cr.count * 4 : 0, nullptr,
                            j + 1 == chunk_plan.k ? ctx->ev_copy_mid : ctx->ev_pack_group[j]});
            segs.back().then_call = [this, j] { hook_chunk(j); };
        }
        for (CopySeg &sg : segs) sg.direct = true;
        return copy_in(ctx, segs, spec.up_stream != nullptr);
    }
    /* the old order (the escape lists, when there are any, in front of the array whose event releases the widening; none: the order of the copies is what it was) */
    int copy_packed_in_order() {
        const avk_packed_batch *pk = src.packed;
        std::vector<CopySeg> segs = packed_head_segs();
        segs.insert(segs.end(), {{pk->start, p.start, n * 4}, {pk->len, p.len, n * 2}, {pk->contig_idx, p.contig, has_contig ? n * 2 : 0}, {pk->var_rel_pos, p.rel, nv * 2}});
        segs.insert(segs.end(), esc_segs.begin(), esc_segs.end());
        segs.push_back({pk->var_type_zyg, p.tz, nv, nullptr, ctx->ev_copy_mid});
        segs.push_back({pk->var_raw_space, d_raw, has_raw ? nv * 4 : 0});
        if (queue_early) { /* the prefix sums and dp_variant queued behind their events as on the chunked route */
            hook_sums_and_variant(segs);
            for (CopySeg &sg : segs) sg.direct = true;
        }
        return copy_in(ctx, segs, spec.up_stream != nullptr);
    }
    /* behind the copies: dp_variant where no hook queued it, then the wide arrays (none for a batch read from its packed source), and the context's stream joins */
    int widen_packed() {
        /* the totals must be what the caller said: n_variants calls, allele_bytes_len bytes (two words back, with the packer's state block) */
        pk_totals = p.sums + p.nb_r + p.nb_v;
        dpk::DpPacked c;
        memset(&c, 0, sizeof(c));
        c.contig_idx = p.contig, c.len = p.len, c.rel_pos = p.rel, c.start = p.start, c.var_raw = d_raw, c.t_cnt = p.tc, c.q_cnt = p.qc, c.var_type_zyg = p.tz, c.a0_len = p.a0, c.a1_len = p.a1,
        c.v_off = p.voff, c.a_off = p.aoff, c.n_regions = n, c.n_variants = nv;
        wide_region_outputs(c), wide_call_outputs(c);
        const uint64_t m = n > nv ? n : nv;
        hipError_t ew = hipSuccess;
        if (packed_src && nv && !queue_early) ew = queue_variant();
        if (queue_early && !(variant_done && (region_done || !chunk_plan.k)) && ew == hipSuccess) ew = hipErrorUnknown; /* (dp_variant and the chunked region launches were queued from copy_in) */
        if (ew == hipSuccess && !chunk_plan.k) ew = hipStreamWaitEvent(side, ctx->ev_copy_mid, 0); /* (chunked: the side stream waits group by group, in hook_chunk) */
        if (packed_src) {
            name_packed_source();
            db->d_pk_voff = p.voff, db->d_pk_tc = p.tc, db->d_pk_qc = p.qc;
        } else if (has_esc && ew == hipSuccess) {
            esc_scans(pk_totals, 2 * n, nv, n, dpk::DpEscNarrow{p.tc, p.qc, nullptr, 1u}, dpk::DpEscNarrow{p.a0, p.a1, p.rel, 0u}, dpk::DpEscNarrow{nullptr, nullptr, p.len, 0u});
            if (m) hipLaunchKernelGGL(avk_dp_widen_packed_esc_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, side, c, de);
            ew = hipGetLastError();
        } else if (m && ew == hipSuccess) {
            hipLaunchKernelGGL(avk_dp_widen_packed_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, side, c);
            ew = hipGetLastError();
        }
        if (ew == hipSuccess && !chunk_plan.k) ew = hipEventRecord(ctx->ev_copy_join, side); /* (chunked: recorded behind the catch-all launch) */
        if (ew == hipSuccess) ew = hipStreamWaitEvent(s, ctx->ev_copy_join, 0); /* from here on the context's stream has the wide arrays (and, being behind its own copies, the allele bytes) */
        return ew == hipSuccess ? 0 : bail_hip("device packing failed", ew);
    }

    int copy_wide() {
        const avk_region_batch *b = src.wide;
        std::vector<CopySeg> segs = {
            {b->start, d_start, n * 8}, {b->end, d_end, n * 8}, {b->t_off, db->d_in_t_off, n * 8}, {b->q_off, db->d_in_q_off, n * 8},
            {b->t_cnt, db->d_in_t_cnt, n * 4}, {b->q_cnt, db->d_in_q_cnt, n * 4}, {b->contig_idx, d_contig, b->contig_idx ? n * 4 : 0},
            {b->var_pos, d_pos, nv * 8}, {b->a0_off, d_a0o, nv * 8}, {b->a1_off, d_a1o, nv * 8}, {b->a0_len, d_a0l, nv * 4}, {b->a1_len, d_a1l, nv * 4},
            {b->var_raw_space, d_raw, b->var_raw_space ? nv * 4 : 0}, {b->var_type, d_type, nv}, {b->var_zyg, d_zyg, nv}, {b->allele_bytes, d_alleles, alen}};
        rc = copy_in(ctx, segs, spec.up_stream != nullptr);
        return rc ? bail(rc) : 0;
    }

    /* ---- the merge forms: the MultiRegions as they are, one kernel that writes a region per input pair; the call arrays are shared by all pairs ---- */
    int alloc_multi() {
        const uint64_t nm = src.n_multi(), mk = src.n_inputs();
        m_contig = has_contig ? (uint32_t *)tmp((nm + 1) * 4) : nullptr;
        m_start = (uint64_t *)tmp((nm + 1) * 8), m_end = (uint64_t *)tmp((nm + 1) * 8);
        db->d_m_in_off = (uint64_t *)kept((nm * mk + 1) * 8);
        db->d_m_in_cnt = (uint32_t *)kept((nm * mk + 1) * 4);
        db->d_in_zyg = d_zyg, db->d_in_type = d_type;
        db->n_multi = nm, db->m_inputs = (uint32_t)mk;
        return rc ? bail(rc) : 0;
    }
    int expand_pairs() {
        dpk::DpPairs c;
        memset(&c, 0, sizeof(c));
        c.contig_idx = m_contig, c.start = m_start, c.end = m_end, c.in_off = db->d_m_in_off, c.in_cnt = db->d_m_in_cnt, c.n_multi = src.n_multi(), c.k = src.n_inputs(),
        c.ppr = src.pairs_per_region();
        wide_region_outputs(c);
        if (!n) return 0;
        hipLaunchKernelGGL(avk_dp_expand_pairs_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, c);
        const hipError_t ew = hipGetLastError();
        return ew == hipSuccess ? 0 : bail_hip("device packing failed", ew);
    }
    int copy_multi() {
        if (int c = alloc_multi()) return c;
        const avk_multi_batch *mb = src.multi;
        const uint64_t nm = mb->n_regions, mk = mb->n_inputs;
        std::vector<CopySeg> segs = {{mb->start, m_start, nm * 8}, {mb->end, m_end, nm * 8}, {mb->in_off, db->d_m_in_off, nm * mk * 8}, {mb->in_cnt, db->d_m_in_cnt, nm * mk * 4},
                                     {mb->contig_idx, m_contig, has_contig ? nm * 4 : 0}, {mb->var_pos, d_pos, nv * 8}, {mb->a0_off, d_a0o, nv * 8}, {mb->a1_off, d_a1o, nv * 8},
                                     {mb->a0_len, d_a0l, nv * 4}, {mb->a1_len, d_a1l, nv * 4}, {mb->var_raw_space, d_raw, has_raw ? nv * 4 : 0}, {mb->var_type, d_type, nv},
                                     {mb->var_zyg, d_zyg, nv}, {mb->allele_bytes, d_alleles, alen}};
        rc = copy_in(ctx, segs, spec.up_stream != nullptr);
        return rc ? bail(rc) : expand_pairs();
    }
    /* the packed arrays as they are; in_off and a_off by prefix sums; one kernel writes the wide MultiRegion arrays the pair expansion reads.  As for avk_packed_batch:
     * copies on the context's stream, counts first; prefix sums and widening beside them */
    int copy_packed_multi() {
        if (int c = alloc_multi()) return c;
        const avk_packed_multi_batch *pm = src.packed_multi;
        const uint64_t nm = src.n_multi(), mk = src.n_inputs(), ni = nm * mk;
        p.contig = has_contig ? (uint16_t *)tmp((nm + 1) * 2) : nullptr, p.len = (uint16_t *)tmp((nm + 1) * 2), p.rel = (uint16_t *)tmp((nv + 1) * 2);
        p.start = (uint32_t *)tmp((nm + 1) * 4);
        p.tc = (uint8_t *)tmp(ni + 16), p.tz = (uint8_t *)tmp(nv + 16), p.a0 = (uint8_t *)tmp(nv + 16), p.a1 = (uint8_t *)tmp(nv + 16);
        p.nb_r = (uint32_t)((ni + AVK_PS_BLOCK - 1) / AVK_PS_BLOCK), p.nb_v = (uint32_t)((nv + AVK_PS_BLOCK - 1) / AVK_PS_BLOCK);
        p.aoff = (uint64_t *)tmp((nv + 1) * 8), p.sums = (uint64_t *)tmp(((size_t)p.nb_r + p.nb_v + 4) * 8);
        p.voff = has_esc ? (uint64_t *)tmp((ni + 1) * 8) : db->d_m_in_off; /* (with escapes: the sums over the narrow counts; the widening writes the true offsets) */
        if (rc) return bail(rc);
        std::vector<CopySeg> segs = {{pm->in_cnt, p.tc, ni}, {pm->a0_len, p.a0, nv}, {pm->a1_len, p.a1, nv, nullptr, ctx->ev_copy_fork}, {pm->start, p.start, nm * 4}, {pm->len, p.len, nm * 2},
                                     {pm->contig_idx, p.contig, has_contig ? nm * 2 : 0}, {pm->var_rel_pos, p.rel, nv * 2}};
        segs.insert(segs.end(), esc_segs.begin(), esc_segs.end()); /* (none without escapes: the order of the copies is what it was) */
        segs.push_back({pm->var_type_zyg, p.tz, nv, nullptr, ctx->ev_copy_mid});
        segs.push_back({pm->var_raw_space, d_raw, has_raw ? nv * 4 : 0});
        segs.push_back({pm->allele_bytes, d_alleles, alen});
        rc = copy_in(ctx, segs, spec.up_stream != nullptr);
        if (rc) return bail(rc);
        const hipError_t ec = queue_sums();
        if (ec != hipSuccess) return bail_hip("packed upload", ec);
        pk_totals = p.sums + p.nb_r + p.nb_v;
        dpk::DpPackedMulti w;
        memset(&w, 0, sizeof(w));
        w.contig_idx = p.contig, w.len = p.len, w.rel_pos = p.rel, w.start = p.start, w.var_raw = d_raw, w.in_cnt = p.tc, w.var_type_zyg = p.tz, w.a0_len = p.a0, w.a1_len = p.a1,
        w.in_off = p.voff, w.a_off = p.aoff, w.n_multi = nm, w.n_variants = nv, w.k = (uint32_t)mk;
        w.w_contig = m_contig, w.w_in_cnt = db->d_m_in_cnt, w.w_start = m_start, w.w_end = m_end;
        wide_call_outputs(w);
        const uint64_t mx = nm > nv ? nm : nv;
        hipError_t ew = hipStreamWaitEvent(side, ctx->ev_copy_mid, 0);
        if (has_esc && ew == hipSuccess) {
            esc_scans(pk_totals, ni, nv, nm, dpk::DpEscNarrow{p.tc, nullptr, nullptr, 0u}, dpk::DpEscNarrow{p.a0, p.a1, p.rel, 0u}, dpk::DpEscNarrow{nullptr, nullptr, p.len, 0u});
            if (mx) hipLaunchKernelGGL(avk_dp_widen_packed_multi_esc_kernel, dim3((unsigned)((mx + 255) / 256)), dim3(256), 0, side, w, de, db->d_m_in_off);
            ew = hipGetLastError();
        } else if (mx && ew == hipSuccess) {
            hipLaunchKernelGGL(avk_dp_widen_packed_multi_kernel, dim3((unsigned)((mx + 255) / 256)), dim3(256), 0, side, w);
            ew = hipGetLastError();
        }
        if (ew == hipSuccess) ew = hipEventRecord(ctx->ev_copy_join, side);
        if (ew == hipSuccess) ew = hipStreamWaitEvent(s, ctx->ev_copy_join, 0);
        return ew == hipSuccess ? expand_pairs() : bail_hip("device packing failed", ew);
    }

    int copy_compact() { /* the compact arrays as they are, then one kernel that writes the wide ones */
        const avk_compact_batch *cb = src.compact;
        dpk::DpCompact c;
        memset(&c, 0, sizeof(c));
        uint32_t *c_contig = has_contig ? (uint32_t *)tmp((n + 1) * 4) : nullptr, *c_start = (uint32_t *)tmp((n + 1) * 4), *c_len = (uint32_t *)tmp((n + 1) * 4),
                 *c_voff = (uint32_t *)tmp((n + 1) * 4), *c_pos = (uint32_t *)tmp((nv + 1) * 4), *c_aoff = (uint32_t *)tmp((nv + 1) * 4);
        uint16_t *c_tc = (uint16_t *)tmp((n + 1) * 2), *c_qc = (uint16_t *)tmp((n + 1) * 2);
        uint8_t *c_tz = (uint8_t *)tmp(nv + 16);
        if (rc) return bail(rc);
        /* a0_len / a1_len / raw_space have the wide arrays' type: they are copied straight into them */
        std::vector<CopySeg> segs = {{cb->start, c_start, n * 4}, {cb->len, c_len, n * 4}, {cb->v_off, c_voff, n * 4}, {cb->t_cnt, c_tc, n * 2}, {cb->q_cnt, c_qc, n * 2},
                                     {cb->contig_idx, c_contig, has_contig ? n * 4 : 0}, {cb->var_pos, c_pos, nv * 4}, {cb->a_off, c_aoff, nv * 4}, {cb->var_type_zyg, c_tz, nv},
                                     {cb->a0_len, d_a0l, nv * 4}, {cb->a1_len, d_a1l, nv * 4}, {cb->var_raw_space, d_raw, has_raw ? nv * 4 : 0}, {cb->allele_bytes, d_alleles, alen}};
        rc = copy_in(ctx, segs, spec.up_stream != nullptr);
        if (rc) return bail(rc);
        c.contig_idx = c_contig, c.start = c_start, c.len = c_len, c.v_off = c_voff, c.t_cnt = c_tc, c.q_cnt = c_qc, c.var_pos = c_pos, c.a_off = c_aoff, c.a0_len = d_a0l, c.a1_len = d_a1l,
        c.var_raw = nullptr, c.var_type_zyg = c_tz, c.n_regions = n, c.n_variants = nv;
        wide_region_outputs(c), wide_call_outputs(c);
        const uint64_t m = n > nv ? n : nv;
        if (!m) return 0;
        hipLaunchKernelGGL(avk_dp_widen_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, c);
        const hipError_t ew = hipGetLastError();
        return ew == hipSuccess ? 0 : bail_hip("device packing failed", ew);
    }

    int copy_form() {
        switch (src.form) {
        case UploadSource::WIDE: return copy_wide();
        case UploadSource::COMPACT: return copy_compact();
        case UploadSource::PACKED: return copy_packed();
        case UploadSource::MULTI: return copy_multi();
        default: return copy_packed_multi();
        }
    }

    int guess_owned_range() { /* (avk_owned_range; forms with explicit offsets: ownership is counted, DpIn::owned) */
        t_copy = now();
        fill_args();
        uint64_t lo = 0, hi = 0;
        const bool counted = avk_owned_range(src, &lo, &hi);
        a.in.v_lo = lo, a.in.v_hi = hi;
        if (!counted) return 0;
        a.in.owned = (uint8_t *)tmp(hi - lo + 16);
        if (rc) return bail(rc);
        if (hipMemsetAsync(a.in.owned, 0, hi - lo, s) != hipSuccess) return bail_hip("device packing failed", hipGetLastError());
        return 0;
    }

    hipError_t region_passes() { /* everything that depends on alt_ed, up to the state block on the host */
        hipError_t x = hipSuccess;
        if (n) {
            if (!region_done) {
                hipLaunchKernelGGL(avk_dp_region_kernel, dim3(n_blocks), dim3(256), 0, s, a, d_block_sums);
                ctx->last_region_launches += 1;
                record_region_mark(s);
            }
            region_done = false; /* (a second round, behind the host's edit distances, runs the whole range in one launch) */
            if (a.in.owned && a.in.v_hi > a.in.v_lo)
                hipLaunchKernelGGL(avk_dp_count_owned_kernel, dim3((unsigned)((a.in.v_hi - a.in.v_lo + 4095) / 4096)), dim3(256), 0, s, (const uint8_t *)a.in.owned, a.in.v_hi - a.in.v_lo, a.st);
            hipLaunchKernelGGL(avk_dp_scan_blocks_kernel, dim3(AVK_DP_BS), dim3(1024), 0, s, d_block_sums, n_blocks, a.st);
            hipLaunchKernelGGL(avk_dp_scan_apply_kernel, dim3(n_blocks), dim3(256), 0, s, a, (const uint64_t *)d_block_sums);
            hipLaunchKernelGGL(avk_dp_lane_switch_kernel, dim3(1), dim3(64), 0, s, a);
            hipLaunchKernelGGL(avk_dp_hist_kernel, dim3((unsigned)((n + 1023) / 1024)), dim3(1024), 0, s, a);
            hipLaunchKernelGGL(avk_dp_bucket_bases_kernel, dim3(1), dim3(256), 0, s, a);
            hipLaunchKernelGGL(avk_dp_scatter_kernel, dim3((unsigned)((n + 1023) / 1024)), dim3(1024), 0, s, a);
            x = hipGetLastError();
        }
        StrataJob *sj = n && spec.strata && !spec.strata->counted ? spec.strata : nullptr; /* (once: the lists do not depend on alt_ed, a second round of the passes leaves them) */
        const bool sj_total = sj && !sj->mask_only;
        if (x == hipSuccess && sj) x = sj_total ? strata_count_launch(sj->st, a.in, n, sj->d_mask, sj->d_sums, s) : strata_mask_launch(sj->st, a.in, n, sj->d_mask, sj->d_sums, s);
        mark(2);
        dpk::DpState *h = hs();
        if (x == hipSuccess) x = hipMemcpyAsync(h, a.st, sizeof(dpk::DpState), hipMemcpyDeviceToHost, s);
        if (x == hipSuccess && pk_totals) x = hipMemcpyAsync(h + 1, pk_totals, has_esc ? 24 : 16, hipMemcpyDeviceToHost, s); /* (the packed forms' two sums ride along: 16 bytes behind the state block) */
        if (x == hipSuccess && sj_total) x = hipMemcpyAsync((uint8_t *)(h + 1) + 24, sj->d_sums + strata_blocks(n), 8, hipMemcpyDeviceToHost, s); /* (and the lists' size behind those) */
        if (x == hipSuccess) x = hipStreamSynchronize(s);
        if (x == hipSuccess && sj_total) memcpy(&sj->total, (const uint8_t *)(h + 1) + 24, 8);
        if (x == hipSuccess && sj) sj->counted = true;
        if (x == hipSuccess) engine_rate_check(ctx);
        return x;
    }
    /* dp_variant where no copy hook queued it, the first round of the region passes, and — the state block being on the host — the packed forms' two sums */
    int first_passes() {
        e = variant_done ? hipSuccess : hipMemsetAsync(a.st, 0, sizeof(dpk::DpState), s);
        if (e == hipSuccess && nv && !variant_done) {
            hipLaunchKernelGGL(avk_dp_variant_kernel, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, s, a);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = region_passes();
        if (e != hipSuccess || !src.is_packed()) return 0;
        /* the two sums the packed form implies must be what the caller says they are */
        uint64_t tot[3] = {0, 0, 0};
        memcpy(tot, hs() + 1, has_esc ? 24 : 16);
        if (has_esc && tot[2]) return bail(fail(ctx, AVK_E_ARG, "packed batch: an escape list is not ascending, names an entry outside the batch, or lists an entry whose narrow field is not 0"));
        if (((src.form == UploadSource::PACKED_MULTI ? src.packed_multi->n_regions : n) && tot[0] != nv) || (nv && tot[1] != alen))
            return bail(fail(ctx, AVK_E_ARG, "packed batch: the call counts sum to %llu (n_variants %llu), the allele lengths to %llu (allele_bytes_len %llu)",
                             (unsigned long long)tot[0], (unsigned long long)nv, (unsigned long long)tot[1], (unsigned long long)alen));
        return 0;
    }
    /* calls whose two alleles are both long after the common prefix and suffix are gone: their alt_ed comes from the host (avk_edit_distance, the routine the
     * host-side packer uses for every call), and the region passes run again */
    int patch_host_edit_distances() {
        if (e != hipSuccess || !hs()->n_pending) return 0;
        std::vector<uint64_t> pk_aoff; /* packed forms: allele offsets and lengths on the host, escapes honoured */
        std::vector<uint32_t> pk_w0, pk_w1;
        if (src.is_packed()) avk_packed_host_alleles(src, pk_aoff, pk_w0, pk_w1);
        const uint32_t np = hs()->n_pending;
        std::vector<uint32_t> idx(np), ed(np);
        e = hipMemcpy(idx.data(), a.pending, (size_t)np * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return 0;
        const uint8_t *host_alleles = src.host_alleles();
        avk_parallel_for(np, avk_host_threads(), [&](unsigned, uint64_t lo, uint64_t hi) {
            for (uint64_t k = lo; k < hi; ++k) {
                const AvkAllelePair al = avk_pending_allele(src, idx[k], pk_aoff.data(), pk_w0.data(), pk_w1.data());
                ed[k] = (uint32_t)avk::host_edit_distance(host_alleles + al.o0, al.l0, host_alleles + al.o1, al.l1);
            }
        });
        uint32_t *d_idx = (uint32_t *)tmp((size_t)np * 4), *d_ed = (uint32_t *)tmp((size_t)np * 4);
        if (rc) return bail(rc);
        e = hipMemcpy(d_idx, idx.data(), (size_t)np * 4, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(d_ed, ed.data(), (size_t)np * 4, hipMemcpyHostToDevice);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(avk_dp_patch_ed_kernel, dim3((np + 255) / 256), dim3(256), 0, s, a.vinfo, (const uint32_t *)d_idx, (const uint32_t *)d_ed, np);
            e = hipMemsetAsync(a.st, 0, sizeof(dpk::DpState), s);
        }
        if (e == hipSuccess) e = region_passes();
        return 0;
    }

    int check_state() {
        if (e != hipSuccess) return bail_hip("device packing failed", e);
        const dpk::DpState *h = hs();
        t_plan = now();
        if (h->err & dpk::DP_ERR_RANGE) return bail(fail(ctx, AVK_E_ARG, "variant range of a region exceeds n_variants"));
        if (h->err & dpk::DP_ERR_ALLELE) return bail(fail(ctx, AVK_E_ARG, "allele range exceeds allele_bytes_len"));
        if (h->err & dpk::DP_ERR_BLOB) return bail(fail(ctx, AVK_E_ARG, "region blob exceeds 2 GiB; split the region's alleles"));
        if (h->total_v > 0x7FFFFFFFull) return bail(fail(ctx, AVK_E_ARG, "more than 2^31 variant records; split the batch"));
        db->v_lo = a.in.v_lo, db->v_hi = a.in.v_hi;
        if (h->err & dpk::DP_NOTE_OUTSIDE) db->v_lo = 0, db->v_hi = nv;
        /* every call of the range is owned, and once: nothing to preserve.  The packed forms' offsets are the running sums of the counts — dense when the sums are right;
         * forms with explicit offsets are dense when as many calls are marked as the range has and the counts add up to the same number */
        db->var_dense = !(h->err & dpk::DP_NOTE_OUTSIDE) && h->total_v == db->v_hi - db->v_lo && (!a.in.owned || h->n_owned == db->v_hi - db->v_lo);
        if (h->total_blob_words / 2 > 0xFFFFFFFFull) return bail(fail(ctx, AVK_E_ARG, "region blob arena exceeds its limits; split the batch"));
        db->n_variants_dev = h->total_v;
        db->seq_total = h->total_seq;
        db->n_bp_groups = h->total_groups;
        return 0;
    }

    int size_slices_and_plan() {
        const dpk::DpState *h = hs();
        /* per-wave HBM slices of this batch's launches: large enough for 98 % of the regions predicted to need the tier (64 MB at most) */
        const int64_t want = 1ll << (20 + avk_slice_pick(h->need_hist, dpk::DP_NEED_BUCKETS));
        db->ws_bytes_eff = want > ctx->ws_bytes_per_wave && ctx->ws_bytes_per_wave > 0 && ctx->adaptive_ws ? want : 0;
        /* regions predicted beyond the last bucket (windows of tens of kilobases with dozens of calls): the shared slices start at the size of the library's first
         * capacity retry, so that these regions are solved in the step and not again, one sub-batch at a time, by avk_results_download */
        db->big_bytes_eff = h->need_hist[dpk::DP_NEED_BUCKETS - 1] > 0 && ctx->adaptive_ws ? (1ll << 30) : 0;
        db->plan.n_hbm = h->n_hbm, db->plan.n_hard = h->n_hard, db->plan.n_fast_total = h->n_fast_total, db->plan.n_hbm_notwide = h->n_hbm_notwide;
        tiles_total = 0;
        for (int fc = 0; fc < AVK_FAST_CLASSES; ++fc) {
            db->plan.n_fast[fc] = h->n_fast[fc], db->plan.n_fast_heavy[fc] = h->n_fast_heavy[fc], db->plan.fast_base[fc] = h->fast_base[fc];
            db->fast_word_base[fc] = h->fast_word_base[fc], db->fast_tiles[fc] = h->fast_tiles[fc];
            tiles_total += h->fast_tiles[fc];
        }
        return 0;
    }

    int alloc_batch() { /* the batch's own buffers */
        const dpk::DpState *h = hs();
        const uint64_t nvd = h->total_v;
        db->d_regions = (AvkDevRegion *)kept((n + 1) * sizeof(AvkDevRegion));
        db->d_blob = (uint32_t *)kept(((size_t)h->total_blob_words + 4) * 4);
        db->d_region_out = (uint32_t *)kept((n * 4 + 4) * 4);
        db->d_var_out = (uint32_t *)kept((nvd + 1) * 4);
        db->d_seqlen = (uint32_t *)kept((n * 5 + 1) * 4);
        db->d_tally = (uint64_t *)kept((size_t)AVK_TALLY_STRIDE * 8);
        db->d_partials = (uint64_t *)kept((size_t)AVK_TALLY_STRIDE * AVK_TALLY_COPIES * 8);
        db->d_counters = (uint32_t *)kept((size_t)AVK_N_COUNTERS * 4);
        db->d_overflow = (uint32_t *)kept((n + 1024) * 4);
        db->d_overflow2 = (uint32_t *)kept((n + 1) * 4);
        db->d_overflow3 = (uint32_t *)kept((3 * (n + 1) + 1024) * 4);
        db->d_overflow4 = (uint32_t *)kept((n + 1) * 4);
        db->d_overflow5 = (uint32_t *)kept((n + 1) * 4);
        db->d_overflow6 = (uint32_t *)kept((n + 1) * 4);
        db->d_overflow7 = (uint32_t *)kept((n + 1) * 4);
        db->d_overflow8 = (uint32_t *)kept((n + 1) * 4);
        db->d_notwide = (uint32_t *)kept((n + 2) * 4);
        if (h->n_fast_total) db->d_fast = (uint32_t *)kept(((size_t)h->fast_words + 64) * 4);
        /* the packer's arguments in device memory: the waves that solve handed-back regions write their records themselves */
        if (h->n_fast_total) db->d_dp_args = (dpk::DpArgs *)kept(sizeof(dpk::DpArgs));
        if (rc) return bail(rc);
        a.regions = db->d_regions, a.blob = db->d_blob, a.fast = db->d_fast;
        db->dp_args = a;
        return 0;
    }

    int queue_writers() {
        const dpk::DpState *h = hs();
        const bool clear_beside = n >= 262144; /* (a small batch: the two events between the streams cost more than the fills, 1.16 instead of 0.98 ms per 46,000-region call) */
        if (clear_beside) { /* the batch's partial tallies and counters are cleared beside the writers, on the side stream (in front of the solver launches the two fills took 55 us) */
            hipError_t ez = hipEventRecord(ctx->ev_copy_fork, s); /* the buffers may have been another batch's until here */
            if (ez == hipSuccess) ez = hipStreamWaitEvent(side, ctx->ev_copy_fork, 0);
            if (ez == hipSuccess && db->d_dp_args) ez = hipMemcpyAsync(db->d_dp_args, &db->dp_args, sizeof(dpk::DpArgs), hipMemcpyHostToDevice, side); /* (behind the writers it was
                                                                                                         most of a 130 us gap in front of the solver launches) */
            if (ez == hipSuccess) ez = hipMemsetAsync(db->d_partials, 0, (size_t)AVK_TALLY_STRIDE * AVK_TALLY_COPIES * sizeof(uint64_t), side);
            if (ez == hipSuccess) ez = hipMemsetAsync(db->d_counters, 0, AVK_N_COUNTERS * sizeof(uint32_t), side);
            if (ez == hipSuccess) ez = hipEventRecord(ctx->ev_copy_join, side);
            if (ez != hipSuccess) return bail_hip("device packing failed", ez);
            db->scratch_clean = true;
        }
        if (tiles_total) hipLaunchKernelGGL(avk_dp_fast_records_kernel, dim3((tiles_total + 3) / 4), dim3(256), 0, s, a, tiles_total);
        /* records and blobs: now for the regions the wave-per-region launches start with; for the lanes' regions when (and if) a launch asks for them */
        const uint32_t n_eager = (uint32_t)n - h->n_fast_total;
        if (n_eager) {
            hipLaunchKernelGGL(avk_dp_region_records_kernel, dim3((n_eager + 255) / 256), dim3(256), 0, s, a, n_eager);
            hipLaunchKernelGGL(avk_dp_region_records_wave_kernel, dim3(256), dim3(256), 0, s, a);
        }
        db->records_full = h->n_fast_total == 0;
        db->lazy_from = n_eager;
        if (db->d_dp_args && !clear_beside) {
            const hipError_t ec = hipMemcpyAsync(db->d_dp_args, &db->dp_args, sizeof(dpk::DpArgs), hipMemcpyHostToDevice, s);
            if (ec != hipSuccess) return bail_hip("device packing failed", ec);
        }
        hipError_t x = hipGetLastError();
        if (x == hipSuccess && clear_beside) x = hipStreamWaitEvent(s, ctx->ev_copy_join, 0); /* the cleared scratch, before anything that follows on this stream */
        if (x != hipSuccess) return bail_hip("device packing failed", x);
        mark(3);
        return 0;
    }

    int finish(avk_dev_batch **out) {
        for (void *q : temps) pool_release(ctx, q); /* in stream order: the writers above run before anything that is handed these buffers next */
        if (!spec.up_stream && ctx->ev_pool_fence) { /* ... which an upload on the packing stream of the asynchronous boundary is not, by itself: it waits for this point once */
            if (hipEventRecord(ctx->ev_pool_fence, s) == hipSuccess) ctx->pool_fence_pending = true;
            else (void)hipGetLastError();
        }
        const dpk::DpState *h = hs();
        if (timing)
            fprintf(stderr, "avk upload (device-packed): %llu regions, %llu calls: buffers %.3f ms, copies queued %.3f ms, packing kernels + plan %.3f ms, writers queued %.3f ms; lanes %u regions in %u tiles, class C %u, class B %u\n",
                    (unsigned long long)n, (unsigned long long)nv, ms(t_start, t_alloc), ms(t_alloc, t_copy), ms(t_copy, t_plan), ms(t_plan, now()), h->n_fast_total, tiles_total,
                    h->n_hbm, h->n_hard);
        *out = db;
        return 0;
    }
};

/* `pre`: the arrays of a PACKED source are in a staging slot already (avk_compare_packed_submit) */
static int upload_device_packed(avk_ctx *ctx, const CallSpec &spec, const UploadSource &source, const PackedOnDevice *pre, avk_dev_batch **out) {
    const char *msg = nullptr;
    if (const int code = avk_upload_check(source, &msg)) return fail(ctx, code, "%s", msg);
    Upload u(ctx, spec, source, pre);
    int rc = u.alloc_inputs();
    if (!rc) rc = u.stage_escapes();
    if (!rc) rc = u.copy_form(); /* copy_wide, copy_compact, copy_packed, copy_multi or copy_packed_multi */
    if (!rc) rc = u.guess_owned_range();
    if (!rc) rc = u.first_passes();
    if (!rc) rc = u.patch_host_edit_distances();
    if (!rc) rc = u.check_state();
    if (!rc) rc = u.size_slices_and_plan();
    if (!rc) rc = u.alloc_batch();
    if (!rc) rc = u.queue_writers();
    return rc ? rc : u.finish(out);
}
