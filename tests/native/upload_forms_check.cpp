/*
 * upload_forms_check.cpp — the forms of an upload (avk_upload_forms.h) on the CPU, a program of its own (tests/test_upload_forms.py builds it with
 * -fsanitize=address,undefined and runs it).
 *
 * The reference is the upload as it was written before the header: one function of five pointers (b, cb, mb, pk, pm — all but one NULL, `mb` beside `pm` carrying
 * the header fields) whose sizes, flags, checks and host-side reads were chains of `pk ? .. : (b ? .. : (cb ? .. : mb->..))`.  Those expressions stand here longhand
 * (struct Old); every hand-made batch below goes through both and must come out the same:
 *   - sizes and flags: empty batches, 0 to 3 inputs for the merge forms, contig / raw arrays present and absent;
 *   - avk_upload_check: every required array nulled in turn, the code and the very message; the size limits;
 *   - avk_owned_range: a first region without truth calls, without query calls, without any; a last region past n_variants; lo > hi; n = 0; shared call arrays;
 *   - avk_pending_allele: every call of every form, the packed forms with and without an escape on the call;
 *   - avk_slice_pick: 63 and 64 regions, the 98 % point on a bucket's edge, the mass in the last bucket.
 */
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../aardvark_amd/csrc/avk_upload_forms.h"

static int failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (failures < 20) {                          \
                fprintf(stderr, "FAIL %s: ", #cond);      \
                fprintf(stderr, __VA_ARGS__);             \
                fprintf(stderr, "\n");                    \
            }                                             \
            ++failures;                                   \
        }                                                 \
    } while (0)

/* ---- the upload's own expressions, as they were ---- */
struct Old {
    const avk_region_batch *b = nullptr;
    const avk_compact_batch *cb = nullptr;
    const avk_multi_batch *mb = nullptr;
    const avk_packed_batch *pk = nullptr;
    const avk_packed_multi_batch *pm = nullptr;
    const avk_packed_escapes *esc = nullptr;
    bool pairs_mode = false;

    bool has_esc() const { return (pk || pm) && esc_present(esc); }
    uint32_t mk() const { return mb ? mb->n_inputs : 0; }
    uint32_t mppr() const { return mk() * (mk() - (mk() ? 1u : 0u)) / 2; }
    uint64_t n() const { return pk ? pk->n_regions : (b ? b->n_regions : (cb ? cb->n_regions : mb->n_regions * mppr())); }
    uint64_t nv() const { return pk ? pk->n_variants : (b ? b->n_variants : (cb ? cb->n_variants : mb->n_variants)); }
    uint64_t alen() const { return pk ? pk->allele_bytes_len : (b ? b->allele_bytes_len : (cb ? cb->allele_bytes_len : mb->allele_bytes_len)); }
    bool has_contig() const {
        return pm ? pm->contig_idx != nullptr : (pk ? pk->contig_idx != nullptr : (b ? b->contig_idx != nullptr : (cb ? cb->contig_idx != nullptr : mb->contig_idx != nullptr)));
    }
    bool has_raw() const {
        return pm ? pm->var_raw_space != nullptr
                  : (pk ? pk->var_raw_space != nullptr : (b ? b->var_raw_space != nullptr : (cb ? cb->var_raw_space != nullptr : mb->var_raw_space != nullptr)));
    }
    const uint8_t *host_alleles() const { return pk ? pk->allele_bytes : (b ? b->allele_bytes : (cb ? cb->allele_bytes : mb->allele_bytes)); }

    int check(const char **msg) const {
        auto fail = [&](const char *m) {
            *msg = m;
            return (int)AVK_E_ARG;
        };
        *msg = nullptr;
        const uint64_t n = this->n(), nv = this->nv(), alen = this->alen();
        if (has_esc() && !esc_arrays_ok(esc)) return fail("escape arrays missing");
        if (pk && n && (!pk->start || !pk->len || !pk->t_cnt || !pk->q_cnt)) return fail("region arrays missing");
        if (pk && nv && (!pk->var_rel_pos || !pk->var_type_zyg || !pk->a0_len || !pk->a1_len || !pk->allele_bytes)) return fail("variant arrays missing");
        if (pm && pm->n_regions && (!pm->start || !pm->len || !pm->in_cnt)) return fail("region arrays missing");
        if (pm && nv && (!pm->var_rel_pos || !pm->var_type_zyg || !pm->a0_len || !pm->a1_len || !pm->allele_bytes)) return fail("variant arrays missing");
        if (mb && !pm && mb->n_regions && (!mb->start || !mb->end || !mb->in_off || !mb->in_cnt)) return fail("region arrays missing");
        if (mb && !pm && nv && (!mb->var_pos || !mb->var_type || !mb->var_zyg || !mb->a0_off || !mb->a0_len || !mb->a1_off || !mb->a1_len || !mb->allele_bytes))
            return fail("variant arrays missing");
        if (n > 0x7FFFFFFFull || nv > 0x7FFFFFFFull) return fail("batch too large (more than 2^31 regions or variants); split it");
        if (b && n && (!b->start || !b->end || !b->t_off || !b->t_cnt || !b->q_off || !b->q_cnt)) return fail("region arrays missing");
        if (b && nv && (!b->var_pos || !b->var_type || !b->var_zyg || !b->a0_off || !b->a0_len || !b->a1_off || !b->a1_len || !b->allele_bytes)) return fail("variant arrays missing");
        if (cb && n && (!cb->start || !cb->len || !cb->v_off || !cb->t_cnt || !cb->q_cnt)) return fail("region arrays missing");
        if (cb && nv && (!cb->var_pos || !cb->var_type_zyg || !cb->a_off || !cb->a0_len || !cb->a1_len || !cb->allele_bytes)) return fail("variant arrays missing");
        if (cb && alen > 0xFFFFFFFFull) return fail("the compact form holds at most 2^32 allele bytes");
        return 0;
    }
    bool owned_range(uint64_t *lo_out, uint64_t *hi_out) const {
        const uint64_t n = this->n(), nv = this->nv();
        uint64_t lo = 0, hi = 0;
        if (pk) {
            hi = nv;
        } else if (n && b) {
            const uint64_t a0 = b->t_cnt[0] ? b->t_off[0] : b->q_off[0], a1 = b->q_cnt[0] ? b->q_off[0] : b->t_off[0];
            lo = a0 < a1 ? a0 : a1;
            const uint64_t e0 = b->t_off[n - 1] + b->t_cnt[n - 1], e1 = b->q_off[n - 1] + b->q_cnt[n - 1];
            hi = e0 > e1 ? e0 : e1;
        } else if (n && cb) {
            lo = cb->v_off[0];
            hi = (uint64_t)cb->v_off[n - 1] + cb->t_cnt[n - 1] + cb->q_cnt[n - 1];
        } else
            hi = nv;
        if (hi > nv) hi = nv;
        if (lo > hi) lo = hi;
        *lo_out = lo, *hi_out = hi;
        return (b || cb) && !pairs_mode && hi > lo;
    }
    /* the host's allele offsets of a packed batch: the loop without escapes, packed_host_alleles with them */
    void pending(uint64_t v, uint64_t *o0, uint64_t *l0, uint64_t *o1, uint64_t *l1) const {
        const uint8_t *pk_l0 = pk ? pk->a0_len : (pm ? pm->a0_len : nullptr), *pk_l1 = pk ? pk->a1_len : (pm ? pm->a1_len : nullptr);
        const uint64_t nv = this->nv();
        std::vector<uint64_t> pk_aoff;
        std::vector<uint32_t> pk_w0, pk_w1;
        if (pk_l0 && has_esc()) {
            pk_aoff.resize(nv + 1), pk_w0.resize(nv + 1), pk_w1.resize(nv + 1);
            for (uint64_t i = 0; i < nv; ++i) pk_w0[i] = pk_l0[i], pk_w1[i] = pk_l1[i];
            for (uint64_t p = 0; p < esc->n_esc_calls; ++p) {
                const uint64_t i = esc->esc_call[p] - esc->first_call;
                if (i < nv) pk_w0[i] = esc->esc_a0_len[p], pk_w1[i] = esc->esc_a1_len[p];
            }
            uint64_t run = 0;
            for (uint64_t i = 0; i < nv; ++i) pk_aoff[i] = run, run += (uint64_t)pk_w0[i] + pk_w1[i];
        } else if (pk_l0) {
            pk_aoff.resize(nv + 1);
            uint64_t run = 0;
            for (uint64_t i = 0; i < nv; ++i) pk_aoff[i] = run, run += (uint64_t)pk_l0[i] + pk_l1[i];
        }
        *o0 = pk_l0 ? pk_aoff[v] : (b ? b->a0_off[v] : (cb ? cb->a_off[v] : mb->a0_off[v]));
        *l0 = pk_l0 ? (has_esc() ? pk_w0[v] : (uint32_t)pk_l0[v]) : (b ? b->a0_len[v] : (cb ? cb->a0_len[v] : mb->a0_len[v]));
        *o1 = pk_l0 ? *o0 + *l0 : (b ? b->a1_off[v] : (cb ? *o0 + *l0 : mb->a1_off[v]));
        *l1 = pk_l0 ? (has_esc() ? pk_w1[v] : (uint32_t)pk_l1[v]) : (b ? b->a1_len[v] : (cb ? cb->a1_len[v] : mb->a1_len[v]));
    }
    static int slice_pick(const uint64_t *need_hist, int n_buckets) {
        uint64_t n_c = 0, run = 0;
        for (int k = 0; k < n_buckets; ++k) n_c += need_hist[k];
        int pick = 0;
        for (int k = 0; k < n_buckets && n_c >= 64; ++k) {
            run += need_hist[k];
            pick = k;
            if (run * 100 >= n_c * 98) break;
        }
        if (pick > 6) pick = 6;
        return pick;
    }
};

/* ---- a small job in every form: R regions, region r with truth and query counts tc[r], qc[r]; call v with alleles of a0[v] and a1[v] bytes ---- */
struct Job {
    std::vector<uint32_t> tc, qc, a0, a1;
    uint32_t k = 3; /* the merge forms: inputs per MultiRegion; the regions' calls are dealt to the inputs as in_cnt = {tc, qc, 0, ..} */
    bool contig = true, raw = true;
    uint64_t shift = 0, extra = 0; /* the wide and the compact form: the call arrays hold `shift` calls of other batches in front and `extra` behind */
    bool escape_calls = false;     /* the packed forms: every third call is listed (its narrow lengths 0) */

    /* storage */
    std::vector<uint64_t> w_start, w_end, w_toff, w_qoff, w_pos, w_a0o, w_a1o, m_inoff, e_call;
    std::vector<uint32_t> w_contig, w_tc, w_qc, w_a0l, w_a1l, w_raw, c_start, c_len, c_voff, c_pos, c_aoff, m_incnt, p_start, e_rel, e_a0, e_a1;
    std::vector<uint16_t> c_tc, c_qc, p_contig, p_len, p_rel;
    std::vector<uint8_t> type, zyg, tz, bytes, p_tc, p_qc, p_a0, p_a1, pm_incnt;
    avk_region_batch b;
    avk_compact_batch cb;
    avk_packed_batch pk;
    avk_multi_batch mb, head;
    avk_packed_multi_batch pm;
    avk_packed_escapes esc;

    template <typename T> static const T *ptr(const std::vector<T> &v) { return v.data() ? v.data() : (const T *)""; /* an empty array is still an array */ }

    void build() {
        const uint64_t R = tc.size(), own = a0.size(), nv = shift + own + extra;
        uint64_t run = shift, arun = 0;
        w_a0l.assign(nv, 1), w_a1l.assign(nv, 1);
        for (uint64_t v = 0; v < own; ++v) w_a0l[shift + v] = a0[v], w_a1l[shift + v] = a1[v];
        for (uint64_t v = 0; v < nv; ++v) {
            w_a0o.push_back(arun), w_a1o.push_back(arun + w_a0l[v]), c_aoff.push_back((uint32_t)arun), arun += (uint64_t)w_a0l[v] + w_a1l[v];
            w_pos.push_back(1000 + 10 * v), c_pos.push_back((uint32_t)(1000 + 10 * v)), w_raw.push_back(7), type.push_back(1), zyg.push_back(2), tz.push_back(0x21), p_rel.push_back(3);
        }
        bytes.assign(arun + 1, 'A');
        for (uint64_t r = 0; r < R; ++r) {
            w_start.push_back(100 * r), w_end.push_back(100 * r + 50), w_contig.push_back(0), w_toff.push_back(run), w_qoff.push_back(run + tc[r]), w_tc.push_back(tc[r]), w_qc.push_back(qc[r]);
            c_start.push_back((uint32_t)(100 * r)), c_len.push_back(50), c_voff.push_back((uint32_t)run), c_tc.push_back((uint16_t)tc[r]), c_qc.push_back((uint16_t)qc[r]);
            p_start.push_back((uint32_t)(100 * r)), p_len.push_back(50), p_contig.push_back(0), p_tc.push_back((uint8_t)tc[r]), p_qc.push_back((uint8_t)qc[r]);
            for (uint32_t i = 0; i < k; ++i) {
                const uint32_t c = i == 0 ? tc[r] : (i == 1 ? qc[r] : 0u);
                m_inoff.push_back(run + (i == 0 ? 0 : (i == 1 ? tc[r] : tc[r] + qc[r]))), m_incnt.push_back(c), pm_incnt.push_back((uint8_t)c);
            }
            run += tc[r] + qc[r];
        }
        memset(&b, 0, sizeof(b)), memset(&cb, 0, sizeof(cb)), memset(&pk, 0, sizeof(pk)), memset(&mb, 0, sizeof(mb)), memset(&pm, 0, sizeof(pm)), memset(&esc, 0, sizeof(esc));
        b.n_regions = R, b.contig_idx = contig ? ptr(w_contig) : nullptr, b.start = ptr(w_start), b.end = ptr(w_end), b.t_off = ptr(w_toff), b.t_cnt = ptr(w_tc), b.q_off = ptr(w_qoff),
        b.q_cnt = ptr(w_qc), b.n_variants = nv, b.var_pos = ptr(w_pos), b.var_type = ptr(type), b.var_zyg = ptr(zyg), b.var_raw_space = raw ? ptr(w_raw) : nullptr, b.a0_off = ptr(w_a0o),
        b.a0_len = ptr(w_a0l), b.a1_off = ptr(w_a1o), b.a1_len = ptr(w_a1l), b.allele_bytes = ptr(bytes), b.allele_bytes_len = arun;
        cb.n_regions = R, cb.contig_idx = b.contig_idx, cb.start = ptr(c_start), cb.len = ptr(c_len), cb.v_off = ptr(c_voff), cb.t_cnt = ptr(c_tc), cb.q_cnt = ptr(c_qc), cb.n_variants = nv,
        cb.var_pos = ptr(c_pos), cb.var_type_zyg = ptr(tz), cb.a_off = ptr(c_aoff), cb.a0_len = ptr(w_a0l), cb.a1_len = ptr(w_a1l), cb.var_raw_space = b.var_raw_space,
        cb.allele_bytes = ptr(bytes), cb.allele_bytes_len = arun;
        mb.n_regions = R, mb.n_inputs = k, mb.contig_idx = b.contig_idx, mb.start = ptr(w_start), mb.end = ptr(w_end), mb.in_off = ptr(m_inoff), mb.in_cnt = ptr(m_incnt), mb.n_variants = nv,
        mb.var_pos = ptr(w_pos), mb.var_type = ptr(type), mb.var_zyg = ptr(zyg), mb.var_raw_space = b.var_raw_space, mb.a0_off = ptr(w_a0o), mb.a0_len = ptr(w_a0l), mb.a1_off = ptr(w_a1o),
        mb.a1_len = ptr(w_a1l), mb.allele_bytes = ptr(bytes), mb.allele_bytes_len = arun;
        /* the packed forms own their calls (shift = extra = 0 for them) */
        p_a0.clear(), p_a1.clear();
        for (uint64_t v = 0; v < own; ++v) {
            const bool listed = escape_calls && v % 3 == 0;
            p_a0.push_back(listed ? 0 : (uint8_t)a0[v]), p_a1.push_back(listed ? 0 : (uint8_t)a1[v]);
            if (listed) e_call.push_back(5000 + v), e_rel.push_back(3), e_a0.push_back(a0[v]), e_a1.push_back(a1[v]);
        }
        esc.first_call = 5000, esc.n_esc_calls = e_call.size(), esc.esc_call = ptr(e_call), esc.esc_rel_pos = ptr(e_rel), esc.esc_a0_len = ptr(e_a0), esc.esc_a1_len = ptr(e_a1);
        pk.n_regions = R, pk.contig_idx = contig ? ptr(p_contig) : nullptr, pk.start = ptr(p_start), pk.len = ptr(p_len), pk.t_cnt = ptr(p_tc), pk.q_cnt = ptr(p_qc), pk.n_variants = own,
        pk.var_rel_pos = ptr(p_rel), pk.var_type_zyg = ptr(tz), pk.a0_len = ptr(p_a0), pk.a1_len = ptr(p_a1), pk.var_raw_space = raw ? ptr(w_raw) : nullptr, pk.allele_bytes = ptr(bytes),
        pk.allele_bytes_len = arun;
        pm.n_regions = R, pm.n_inputs = k, pm.contig_idx = pk.contig_idx, pm.start = ptr(p_start), pm.len = ptr(p_len), pm.in_cnt = ptr(pm_incnt), pm.n_variants = own,
        pm.var_rel_pos = ptr(p_rel), pm.var_type_zyg = ptr(tz), pm.a0_len = ptr(p_a0), pm.a1_len = ptr(p_a1), pm.var_raw_space = pk.var_raw_space, pm.allele_bytes = ptr(bytes),
        pm.allele_bytes_len = arun;
        memset(&head, 0, sizeof(head)); /* as the merge path makes it beside a packed multi batch */
        head.n_regions = R, head.n_inputs = k, head.n_variants = own, head.allele_bytes = pm.allele_bytes, head.allele_bytes_len = pm.allele_bytes_len;
    }
};

enum { N_FORMS = 5 };
static const char *const FORM_NAMES[N_FORMS] = {"wide", "compact", "packed", "multi", "packed multi"};
static void both(const Job &j, int form, bool pairs_mode, Old *o, UploadSource *u) {
    const avk_packed_escapes *esc = j.escape_calls ? &j.esc : nullptr;
    *o = Old();
    o->pairs_mode = pairs_mode;
    switch (form) {
    case 0: o->b = &j.b, *u = UploadSource::of(&j.b, pairs_mode); break;
    case 1: o->cb = &j.cb, *u = UploadSource::of(&j.cb); break;
    case 2: o->pk = &j.pk, o->esc = esc, *u = UploadSource::of(&j.pk, esc); break;
    case 3: o->mb = &j.mb, o->pairs_mode = true, *u = UploadSource::of(&j.mb); break;
    default: o->mb = &j.head, o->pm = &j.pm, o->esc = esc, o->pairs_mode = true, *u = UploadSource::of(&j.pm, j.head, esc); break;
    }
}

static void compare(const Job &j, const char *what, int form, bool pairs_mode = false) {
    Old o;
    UploadSource u;
    both(j, form, pairs_mode, &o, &u);
    const char *name = FORM_NAMES[form];
    CHECK(u.n_regions() == o.n() && u.n_variants() == o.nv() && u.allele_bytes_len() == o.alen(), "%s, %s: sizes %llu %llu %llu, were %llu %llu %llu", what, name,
          (unsigned long long)u.n_regions(), (unsigned long long)u.n_variants(), (unsigned long long)u.allele_bytes_len(), (unsigned long long)o.n(), (unsigned long long)o.nv(),
          (unsigned long long)o.alen());
    CHECK(u.has_contig() == o.has_contig() && u.has_raw() == o.has_raw() && u.has_esc() == o.has_esc() && u.host_alleles() == o.host_alleles(), "%s, %s: flags", what, name);
    CHECK(u.n_inputs() == o.mk() && u.pairs_per_region() == o.mppr() && u.pairs_mode == o.pairs_mode, "%s, %s: inputs %u pairs %u", what, name, u.n_inputs(), u.pairs_per_region());
    const char *m0 = "?", *m1 = "?";
    const int c0 = o.check(&m0), c1 = avk_upload_check(u, &m1);
    CHECK(c0 == c1 && ((!m0 && !m1) || (m0 && m1 && !strcmp(m0, m1))), "%s, %s: check %d '%s', was %d '%s'", what, name, c1, m1 ? m1 : "", c0, m0 ? m0 : "");
    if (c0) return;
    uint64_t lo0 = 9, hi0 = 9, lo1 = 8, hi1 = 8;
    const bool w0 = o.owned_range(&lo0, &hi0), w1 = avk_owned_range(u, &lo1, &hi1);
    CHECK(w0 == w1 && lo0 == lo1 && hi0 == hi1, "%s, %s: owned [%llu, %llu) %d, was [%llu, %llu) %d", what, name, (unsigned long long)lo1, (unsigned long long)hi1, (int)w1,
          (unsigned long long)lo0, (unsigned long long)hi0, (int)w0);
    std::vector<uint64_t> aoff;
    std::vector<uint32_t> l0, l1;
    if (u.is_packed()) avk_packed_host_alleles(u, aoff, l0, l1);
    for (uint64_t v = 0; v < o.nv(); ++v) {
        uint64_t x[4];
        o.pending(v, &x[0], &x[1], &x[2], &x[3]);
        const AvkAllelePair al = avk_pending_allele(u, v, aoff.data(), l0.data(), l1.data());
        CHECK(al.o0 == x[0] && al.l0 == x[1] && al.o1 == x[2] && al.l1 == x[3], "%s, %s: call %llu at %llu+%llu, %llu+%llu, was %llu+%llu, %llu+%llu", what, name, (unsigned long long)v,
              (unsigned long long)al.o0, (unsigned long long)al.l0, (unsigned long long)al.o1, (unsigned long long)al.l1, (unsigned long long)x[0], (unsigned long long)x[1],
              (unsigned long long)x[2], (unsigned long long)x[3]);
        CHECK(al.o1 + al.l1 <= o.alen(), "%s, %s: call %llu ends behind the allele bytes", what, name, (unsigned long long)v);
    }
}
static void compare_all(const Job &j, const char *what) {
    for (int form = 0; form < N_FORMS; ++form) compare(j, what, form);
    compare(j, what, 0, true); /* the wide form as the pair solve hands it in: no ownership map */
}

static Job job(std::vector<uint32_t> tc, std::vector<uint32_t> qc, uint32_t k = 3) {
    Job j;
    j.tc = tc, j.qc = qc, j.k = k;
    uint64_t nv = 0;
    for (size_t r = 0; r < tc.size(); ++r) nv += tc[r] + qc[r];
    for (uint64_t v = 0; v < nv; ++v) j.a0.push_back(1 + (uint32_t)(v * 7 % 5)), j.a1.push_back(1 + (uint32_t)(v * 3 % 4));
    return j;
}

/* ---- sizes, flags, ownership and the host's alleles ---- */
static void check_jobs() {
    for (uint32_t k = 0; k <= 3; ++k)
        for (int arrays = 0; arrays < 4; ++arrays) {
            Job j = job({2, 0, 1, 3}, {1, 2, 0, 3}, k);
            j.contig = arrays & 1, j.raw = arrays & 2;
            j.build();
            compare_all(j, "four regions");
            Job e = job({}, {}, k);
            e.contig = arrays & 1, e.raw = arrays & 2;
            e.build();
            compare_all(e, "an empty batch");
            Job z = job({0, 0, 0}, {0, 0, 0}, k); /* regions, no calls */
            z.build();
            compare_all(z, "regions without calls");
        }
    { /* escapes on every third call (long alleles among them) */
        Job j = job({2, 0, 1, 3}, {1, 2, 0, 3});
        j.a0[0] = 300, j.a1[3] = 1000, j.a0[6] = 256, j.escape_calls = true;
        j.build();
        compare(j, "escaped calls", 2), compare(j, "escaped calls", 4);
    }
    /* the first region: no truth calls, no query calls, neither; shared call arrays in front (lo > 0) and behind */
    const std::vector<uint32_t> firsts[][2] = {{{0, 2, 1}, {3, 1, 1}}, {{3, 2, 1}, {0, 1, 1}}, {{0, 2, 1}, {0, 1, 1}}, {{1, 2, 1}, {2, 1, 0}}};
    for (const auto &f : firsts)
        for (uint64_t shift : {0ull, 5ull})
            for (uint64_t extra : {0ull, 4ull}) {
                Job j = job(f[0], f[1]);
                j.shift = shift, j.extra = extra;
                j.build();
                compare(j, "first region", 0), compare(j, "first region", 1), compare(j, "first region", 0, true);
            }
    { /* a last region that ends past n_variants: hi is clamped; one whose first region starts behind it too: lo is clamped to hi */
        Job j = job({1, 2, 1}, {2, 1, 1});
        j.shift = 3;
        j.build();
        j.w_tc[2] += 40, j.w_qc[2] += 50, j.c_tc[2] += 40, j.c_qc[2] += 50;
        compare(j, "last region past the calls", 0), compare(j, "last region past the calls", 1);
        j.w_toff[0] = j.w_qoff[0] = 1000, j.c_voff[0] = 1000;
        compare(j, "first region past the calls", 0), compare(j, "first region past the calls", 1);
        j.w_tc[2] = j.w_qc[2] = 0, j.c_tc[2] = j.c_qc[2] = 0, j.w_toff[2] = j.w_qoff[2] = 2, j.c_voff[2] = 2; /* lo > hi with hi inside the arrays */
        compare(j, "lo behind hi", 0), compare(j, "lo behind hi", 1);
    }
}

/* ---- avk_upload_check: every required array nulled in turn; the limits ---- */
template <typename B, typename F> static void null_each(Job &j, B &batch, std::vector<F B::*> fields, int form, const char *what) {
    for (F B::*f : fields) {
        const F saved = batch.*f;
        batch.*f = nullptr;
        compare(j, what, form);
        Old o;
        UploadSource u;
        both(j, form, false, &o, &u);
        const char *m = nullptr;
        CHECK(avk_upload_check(u, &m) == AVK_E_ARG && m && strstr(m, "arrays missing"), "%s, %s: a NULL array passed", what, FORM_NAMES[form]);
        batch.*f = saved;
    }
}
static void check_checks() {
    Job j = job({2, 0, 1}, {1, 2, 0});
    j.build();
    null_each<avk_region_batch, const uint64_t *>(j, j.b, {&avk_region_batch::start, &avk_region_batch::end, &avk_region_batch::t_off, &avk_region_batch::q_off, &avk_region_batch::var_pos,
                                                           &avk_region_batch::a0_off, &avk_region_batch::a1_off}, 0, "NULL array");
    null_each<avk_region_batch, const uint32_t *>(j, j.b, {&avk_region_batch::t_cnt, &avk_region_batch::q_cnt, &avk_region_batch::a0_len, &avk_region_batch::a1_len}, 0, "NULL array");
    null_each<avk_region_batch, const uint8_t *>(j, j.b, {&avk_region_batch::var_type, &avk_region_batch::var_zyg, &avk_region_batch::allele_bytes}, 0, "NULL array");
    null_each<avk_compact_batch, const uint32_t *>(j, j.cb, {&avk_compact_batch::start, &avk_compact_batch::len, &avk_compact_batch::v_off, &avk_compact_batch::var_pos,
                                                             &avk_compact_batch::a_off, &avk_compact_batch::a0_len, &avk_compact_batch::a1_len}, 1, "NULL array");
    null_each<avk_compact_batch, const uint16_t *>(j, j.cb, {&avk_compact_batch::t_cnt, &avk_compact_batch::q_cnt}, 1, "NULL array");
    null_each<avk_compact_batch, const uint8_t *>(j, j.cb, {&avk_compact_batch::var_type_zyg, &avk_compact_batch::allele_bytes}, 1, "NULL array");
    null_each<avk_packed_batch, const uint32_t *>(j, j.pk, {&avk_packed_batch::start}, 2, "NULL array");
    null_each<avk_packed_batch, const uint16_t *>(j, j.pk, {&avk_packed_batch::len, &avk_packed_batch::var_rel_pos}, 2, "NULL array");
    null_each<avk_packed_batch, const uint8_t *>(j, j.pk, {&avk_packed_batch::t_cnt, &avk_packed_batch::q_cnt, &avk_packed_batch::var_type_zyg, &avk_packed_batch::a0_len,
                                                           &avk_packed_batch::a1_len, &avk_packed_batch::allele_bytes}, 2, "NULL array");
    null_each<avk_multi_batch, const uint64_t *>(j, j.mb, {&avk_multi_batch::start, &avk_multi_batch::end, &avk_multi_batch::in_off, &avk_multi_batch::var_pos, &avk_multi_batch::a0_off,
                                                           &avk_multi_batch::a1_off}, 3, "NULL array");
    null_each<avk_multi_batch, const uint32_t *>(j, j.mb, {&avk_multi_batch::in_cnt, &avk_multi_batch::a0_len, &avk_multi_batch::a1_len}, 3, "NULL array");
    null_each<avk_multi_batch, const uint8_t *>(j, j.mb, {&avk_multi_batch::var_type, &avk_multi_batch::var_zyg, &avk_multi_batch::allele_bytes}, 3, "NULL array");
    null_each<avk_packed_multi_batch, const uint32_t *>(j, j.pm, {&avk_packed_multi_batch::start}, 4, "NULL array");
    null_each<avk_packed_multi_batch, const uint16_t *>(j, j.pm, {&avk_packed_multi_batch::len, &avk_packed_multi_batch::var_rel_pos}, 4, "NULL array");
    null_each<avk_packed_multi_batch, const uint8_t *>(j, j.pm, {&avk_packed_multi_batch::in_cnt, &avk_packed_multi_batch::var_type_zyg, &avk_packed_multi_batch::a0_len,
                                                                 &avk_packed_multi_batch::a1_len, &avk_packed_multi_batch::allele_bytes}, 4, "NULL array");
    { /* the optional arrays are optional */
        Job o = job({2, 0, 1}, {1, 2, 0});
        o.contig = o.raw = false;
        o.build();
        const char *m = "?";
        for (int form = 0; form < N_FORMS; ++form) {
            Old old;
            UploadSource u;
            both(o, form, false, &old, &u);
            CHECK(avk_upload_check(u, &m) == 0 && !m, "%s: refused without contig_idx and var_raw_space", FORM_NAMES[form]);
        }
    }
    { /* escape lists with an array missing: the packed forms refuse them first (in front of their own NULL arrays), the others never look */
        Job e = job({2, 0, 1}, {1, 2, 0});
        e.escape_calls = true;
        e.build();
        const uint32_t *saved = e.esc.esc_a1_len;
        e.esc.esc_a1_len = nullptr, e.pk.start = nullptr, e.pm.start = nullptr;
        for (int form : {2, 4}) {
            compare(e, "escape array NULL", form);
            Old old;
            UploadSource u;
            both(e, form, false, &old, &u);
            const char *m = nullptr;
            CHECK(avk_upload_check(u, &m) == AVK_E_ARG && m && !strcmp(m, "escape arrays missing"), "%s: '%s'", FORM_NAMES[form], m ? m : "");
        }
        e.esc.esc_a1_len = saved;
        e.esc.n_esc_slots = 2; /* a list that names entries but has no arrays */
        compare(e, "escape list without arrays", 2), compare(e, "escape list without arrays", 4);
    }
    { /* the limits: 2^31 regions or calls (the packed and the merge forms look at their arrays first, the wide and the compact form at the size), 2^32 compact bytes */
        for (int form = 0; form < N_FORMS; ++form)
            for (int what = 0; what < 4; ++what) {
                Job big = job({2, 0, 1}, {1, 2, 0}, what == 3 ? 64 : 3);
                big.build();
                const uint64_t count = what == 3 ? 1100000ull : 0x80000000ull; /* (64 inputs: 2016 pairs per MultiRegion) */
                if (what != 1) big.b.n_regions = big.cb.n_regions = big.pk.n_regions = big.mb.n_regions = big.pm.n_regions = big.head.n_regions = count;
                if (what == 1) big.b.n_variants = big.cb.n_variants = big.pk.n_variants = big.mb.n_variants = big.pm.n_variants = big.head.n_variants = count;
                if (what == 2) big.b.start = nullptr, big.cb.start = nullptr, big.pk.start = nullptr, big.mb.start = nullptr, big.pm.start = nullptr;
                Old old;
                UploadSource u;
                both(big, form, false, &old, &u);
                const char *m0 = nullptr, *m1 = nullptr;
                const int c0 = old.check(&m0), c1 = avk_upload_check(u, &m1); /* (the checks read no array) */
                CHECK(c0 == c1 && c1 == (what == 3 && form < 3 ? 0 : AVK_E_ARG) && (!m0 ? !m1 : m1 && !strcmp(m0, m1)), "limit %d, %s: %d '%s', was %d '%s'", what, FORM_NAMES[form], c1,
                      m1 ? m1 : "", c0, m0 ? m0 : "");
                if (what < 2) CHECK(m1 && strstr(m1, "batch too large"), "limit %d, %s: '%s'", what, FORM_NAMES[form], m1 ? m1 : "");
            }
        Job c = job({2, 0, 1}, {1, 2, 0});
        c.build();
        for (uint64_t bytes : {0xFFFFFFFFull, 0x100000000ull}) {
            c.cb.allele_bytes_len = bytes;
            UploadSource u = UploadSource::of(&c.cb);
            Old old;
            old.cb = &c.cb;
            const char *m0 = nullptr, *m1 = nullptr;
            const int c0 = old.check(&m0), c1 = avk_upload_check(u, &m1);
            CHECK(c0 == c1 && c1 == (bytes > 0xFFFFFFFFull ? AVK_E_ARG : 0) && (!m0 ? !m1 : m1 && !strcmp(m0, m1)), "compact bytes %llu: %d", (unsigned long long)bytes, c1);
            if (c1) CHECK(!strcmp(m1, "the compact form holds at most 2^32 allele bytes"), "'%s'", m1);
        }
    }
}

/* ---- avk_slice_pick ---- */
static void check_slices() {
    enum { B = 9 };
    const struct {
        uint64_t h[B];
        int pick;
    } cases[] = {
        {{0, 0, 0, 0, 0, 0, 0, 0, 0}, 0},
        {{0, 0, 0, 63, 0, 0, 0, 0, 0}, 0},  /* fewer than 64 regions: the option's slice */
        {{0, 0, 0, 64, 0, 0, 0, 0, 0}, 3},
        {{10, 20, 30, 3, 0, 0, 0, 0, 0}, 0}, /* 63 over several buckets */
        {{10, 20, 30, 4, 0, 0, 0, 0, 0}, 3}, /* 64: 60 of 64 are 93.75 % */
        {{98, 0, 2, 0, 0, 0, 0, 0, 0}, 0},   /* the 98 % point exactly at the end of bucket 0 */
        {{97, 0, 3, 0, 0, 0, 0, 0, 0}, 2},   /* ... and one region short of it */
        {{49, 49, 0, 0, 2, 0, 0, 0, 0}, 1},
        {{0, 0, 0, 0, 0, 0, 0, 0, 100}, 6}, /* the mass in the last bucket: 64 MB at most */
        {{0, 0, 0, 0, 0, 0, 0, 100, 0}, 6},
        {{0, 0, 0, 0, 0, 0, 100, 0, 0}, 6},
        {{50, 0, 0, 0, 0, 0, 0, 0, 50}, 6},
        {{1000000000000ull, 0, 0, 0, 0, 20000000000ull, 0, 0, 0}, 0},
    };
    for (const auto &c : cases) {
        const int got = avk_slice_pick(c.h, B), was = Old::slice_pick(c.h, B);
        CHECK(got == c.pick && got == was, "histogram starting %llu %llu %llu %llu: bucket %d, was %d, expected %d", (unsigned long long)c.h[0], (unsigned long long)c.h[1],
              (unsigned long long)c.h[2], (unsigned long long)c.h[3], got, was, c.pick);
    }
    uint64_t state = 12345;
    for (int round = 0; round < 20000; ++round) { /* ... and random ones against the loop as it was */
        uint64_t h[B];
        for (uint64_t &x : h) state = state * 6364136223846793005ull + 1442695040888963407ull, x = (state >> 40) % ((round % 3) ? 40 : 4);
        CHECK(avk_slice_pick(h, B) == Old::slice_pick(h, B), "random histogram %d", round);
    }
}

int main() {
    check_jobs();
    check_checks();
    check_slices();
    if (failures) {
        fprintf(stderr, "upload_forms_check: %d failures\n", failures);
        return 1;
    }
    printf("upload_forms_check: ok\n");
    return 0;
}
