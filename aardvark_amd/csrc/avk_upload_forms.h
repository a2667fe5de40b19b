/* The five forms a batch reaches upload_device_packed in (avk_upload.inl), behind one type: which form it is, the one pointer that belongs to it, and every size,
 * flag and host-side read the upload takes from the caller's arrays — written once per form here instead of as a chain of `pk ? .. : (b ? .. : (cb ? .. : mb->..))`
 * at every use.  Also the argument checks of the upload, the range of calls a batch owns, and the HBM slice a batch's need histogram asks for.
 *
 * Plain C++, no HIP types: tests/native/upload_forms_check.cpp compiles this header for the CPU, next to the expressions it replaced. */
#ifndef AVK_UPLOAD_FORMS_H
#define AVK_UPLOAD_FORMS_H

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/aardvark_amd.h"

/* an avk_packed_escapes that lists something, with every array it needs */
static inline bool esc_present(const avk_packed_escapes *e) { return e && (e->n_esc_regions || e->n_esc_slots || e->n_esc_calls); }
static inline bool esc_arrays_ok(const avk_packed_escapes *e) {
    if (!esc_present(e)) return true;
    return (!e->n_esc_regions || (e->esc_region && e->esc_len)) && (!e->n_esc_slots || (e->esc_slot && e->esc_cnt)) &&
           (!e->n_esc_calls || (e->esc_call && e->esc_rel_pos && e->esc_a0_len && e->esc_a1_len));
}

struct UploadSource {
    enum Form { WIDE, COMPACT, PACKED, MULTI, PACKED_MULTI };
    Form form;
    union { /* the batch, in the form's own type */
        const avk_region_batch *wide;
        const avk_compact_batch *compact;
        const avk_packed_batch *packed;
        const avk_multi_batch *multi; /* a batch of MultiRegions (the merge path): one region per input pair is made on the device (dp_expand_pairs) */
        const avk_packed_multi_batch *packed_multi;
    };
    avk_multi_batch head;          /* PACKED_MULTI: n_regions, n_inputs, n_variants, allele_bytes and allele_bytes_len of the batch (every array but allele_bytes NULL) */
    const avk_packed_escapes *esc; /* the packed forms' escape lists, or NULL */
    bool pairs_mode;
    /* read once, when the source is made */
    uint64_t regions, variants, bytes_len; /* regions: those the solver sees — for the merge forms one per MultiRegion and input pair */
    uint64_t multi_regions;
    uint32_t inputs;
    bool contig, raw;
    const uint8_t *alleles;

    static UploadSource of(const avk_region_batch *b, bool pairs_mode) {
        UploadSource s = made(WIDE, b, b, nullptr, pairs_mode);
        s.wide = b, s.regions = b->n_regions;
        return s;
    }
    static UploadSource of(const avk_compact_batch *cb) {
        UploadSource s = made(COMPACT, cb, cb, nullptr, false);
        s.compact = cb, s.regions = cb->n_regions;
        return s;
    }
    static UploadSource of(const avk_packed_batch *pk, const avk_packed_escapes *esc) {
        UploadSource s = made(PACKED, pk, pk, esc, false);
        s.packed = pk, s.regions = pk->n_regions;
        return s;
    }
    static UploadSource of(const avk_multi_batch *mb) {
        UploadSource s = made(MULTI, mb, mb, nullptr, true);
        s.multi = mb, s.pair_regions(*mb);
        return s;
    }
    static UploadSource of(const avk_packed_multi_batch *pm, const avk_multi_batch &head, const avk_packed_escapes *esc) {
        UploadSource s = made(PACKED_MULTI, &head, pm, esc, true); /* (the sizes and the allele bytes are the header's, as they always were) */
        s.packed_multi = pm, s.head = head, s.pair_regions(head);
        return s;
    }

    bool is_packed() const { return form == PACKED || form == PACKED_MULTI; }
    bool is_multi() const { return form == MULTI || form == PACKED_MULTI; }
    bool has_esc() const { return is_packed() && esc_present(esc); }
    uint32_t n_inputs() const { return inputs; }
    uint32_t pairs_per_region() const { return inputs * (inputs - (inputs ? 1u : 0u)) / 2; } /* k (k - 1) / 2; 0 for k = 0 */
    uint64_t n_multi() const { return multi_regions; }
    uint64_t n_regions() const { return regions; }
    uint64_t n_variants() const { return variants; }
    uint64_t allele_bytes_len() const { return bytes_len; }
    bool has_contig() const { return contig; }
    bool has_raw() const { return raw; }
    const uint8_t *host_alleles() const { return alleles; }
    /* the packed forms' allele lengths as the caller wrote them (a call with an escape: 0) */
    const uint8_t *packed_a0_len() const { return form == PACKED ? packed->a0_len : (form == PACKED_MULTI ? packed_multi->a0_len : nullptr); }
    const uint8_t *packed_a1_len() const { return form == PACKED ? packed->a1_len : (form == PACKED_MULTI ? packed_multi->a1_len : nullptr); }

  private:
    /* sizes: the struct that carries n_variants and the allele bytes; arrays: the one whose optional arrays are looked at */
    template <typename S, typename A> static UploadSource made(Form f, const S *sizes, const A *arrays, const avk_packed_escapes *esc, bool pairs_mode) {
        UploadSource s;
        s.form = f, s.wide = nullptr, s.head = avk_multi_batch(), s.esc = esc, s.pairs_mode = pairs_mode;
        s.regions = s.multi_regions = 0, s.inputs = 0;
        s.variants = sizes->n_variants, s.bytes_len = sizes->allele_bytes_len, s.alleles = sizes->allele_bytes;
        s.contig = arrays->contig_idx != nullptr, s.raw = arrays->var_raw_space != nullptr;
        return s;
    }
    void pair_regions(const avk_multi_batch &h) { inputs = h.n_inputs, multi_regions = h.n_regions, regions = h.n_regions * pairs_per_region(); }
};

/* The argument checks of an upload: 0, or the code with *msg the message.  Every form is checked in the order it always was: the packed and the merge forms' arrays
 * in front of the size limit, the wide and the compact form's behind it. */
static inline int avk_upload_check(const UploadSource &u, const char **msg) {
    static const char *const no_esc = "escape arrays missing", *const no_regions = "region arrays missing", *const no_variants = "variant arrays missing",
                             *const too_large = "batch too large (more than 2^31 regions or variants); split it";
    auto bad = [&](const char *m) {
        *msg = m;
        return (int)AVK_E_ARG;
    };
    if (u.has_esc() && !esc_arrays_ok(u.esc)) return bad(no_esc);
    const uint64_t n = u.n_regions(), nv = u.n_variants();
    const bool big = n > 0x7FFFFFFFull || nv > 0x7FFFFFFFull;
    switch (u.form) {
    case UploadSource::PACKED: {
        const avk_packed_batch *pk = u.packed;
        if (n && (!pk->start || !pk->len || !pk->t_cnt || !pk->q_cnt)) return bad(no_regions);
        if (nv && (!pk->var_rel_pos || !pk->var_type_zyg || !pk->a0_len || !pk->a1_len || !pk->allele_bytes)) return bad(no_variants);
        if (big) return bad(too_large);
        break;
    }
    case UploadSource::PACKED_MULTI: {
        const avk_packed_multi_batch *pm = u.packed_multi;
        if (pm->n_regions && (!pm->start || !pm->len || !pm->in_cnt)) return bad(no_regions);
        if (nv && (!pm->var_rel_pos || !pm->var_type_zyg || !pm->a0_len || !pm->a1_len || !pm->allele_bytes)) return bad(no_variants);
        if (big) return bad(too_large);
        break;
    }
    case UploadSource::MULTI: {
        const avk_multi_batch *mb = u.multi;
        if (mb->n_regions && (!mb->start || !mb->end || !mb->in_off || !mb->in_cnt)) return bad(no_regions);
        if (nv && (!mb->var_pos || !mb->var_type || !mb->var_zyg || !mb->a0_off || !mb->a0_len || !mb->a1_off || !mb->a1_len || !mb->allele_bytes)) return bad(no_variants);
        if (big) return bad(too_large);
        break;
    }
    case UploadSource::WIDE: {
        const avk_region_batch *b = u.wide;
        if (big) return bad(too_large);
        if (n && (!b->start || !b->end || !b->t_off || !b->t_cnt || !b->q_off || !b->q_cnt)) return bad(no_regions);
        if (nv && (!b->var_pos || !b->var_type || !b->var_zyg || !b->a0_off || !b->a0_len || !b->a1_off || !b->a1_len || !b->allele_bytes)) return bad(no_variants);
        break;
    }
    case UploadSource::COMPACT: {
        const avk_compact_batch *cb = u.compact;
        if (big) return bad(too_large);
        if (n && (!cb->start || !cb->len || !cb->v_off || !cb->t_cnt || !cb->q_cnt)) return bad(no_regions);
        if (nv && (!cb->var_pos || !cb->var_type_zyg || !cb->a_off || !cb->a0_len || !cb->a1_len || !cb->allele_bytes)) return bad(no_variants);
        if (u.allele_bytes_len() > 0xFFFFFFFFull) return bad("the compact form holds at most 2^32 allele bytes");
        break;
    }
    }
    *msg = nullptr;
    return 0;
}

/* The calls this batch owns, [*lo, *hi), guessed from its first and last region (batches of one job may share the call arrays: compare_main.cpp); dp_region notes
 * any region outside the guess.  true: the form has explicit offsets, so ownership is counted call by call (DpIn::owned, hi - lo bytes). */
static inline bool avk_owned_range(const UploadSource &u, uint64_t *lo_out, uint64_t *hi_out) {
    const uint64_t n = u.n_regions(), nv = u.n_variants();
    uint64_t lo = 0, hi = nv; /* the packed form owns its calls by construction; the pair form has no per-call outputs */
    if (n && u.form == UploadSource::WIDE) {
        const avk_region_batch *b = u.wide;
        const uint64_t a0 = b->t_cnt[0] ? b->t_off[0] : b->q_off[0], a1 = b->q_cnt[0] ? b->q_off[0] : b->t_off[0];
        lo = a0 < a1 ? a0 : a1;
        const uint64_t e0 = b->t_off[n - 1] + b->t_cnt[n - 1], e1 = b->q_off[n - 1] + b->q_cnt[n - 1];
        hi = e0 > e1 ? e0 : e1;
    } else if (n && u.form == UploadSource::COMPACT) {
        const avk_compact_batch *cb = u.compact;
        lo = cb->v_off[0];
        hi = (uint64_t)cb->v_off[n - 1] + cb->t_cnt[n - 1] + cb->q_cnt[n - 1];
    }
    if (hi > nv) hi = nv;
    if (lo > hi) lo = hi;
    *lo_out = lo, *hi_out = hi;
    return (u.form == UploadSource::WIDE || u.form == UploadSource::COMPACT) && !u.pairs_mode && hi > lo;
}

/* allele offsets and lengths of a packed batch's calls on the host, escapes honoured (only made for the few calls whose edit distance is left to the host) */
static inline void avk_packed_host_alleles(const UploadSource &u, std::vector<uint64_t> &aoff, std::vector<uint32_t> &w0, std::vector<uint32_t> &w1) {
    const uint8_t *l0 = u.packed_a0_len(), *l1 = u.packed_a1_len();
    const uint64_t nv = u.n_variants();
    aoff.resize(nv + 1), w0.resize(nv + 1), w1.resize(nv + 1);
    for (uint64_t v = 0; v < nv; ++v) w0[v] = l0[v], w1[v] = l1[v];
    if (u.has_esc())
        for (uint64_t p = 0; p < u.esc->n_esc_calls; ++p) {
            const uint64_t v = u.esc->esc_call[p] - u.esc->first_call;
            if (v < nv) w0[v] = u.esc->esc_a0_len[p], w1[v] = u.esc->esc_a1_len[p];
        }
    uint64_t run = 0;
    for (uint64_t v = 0; v < nv; ++v) aoff[v] = run, run += (uint64_t)w0[v] + w1[v];
    aoff[nv] = run;
}

/* Where the two alleles of call v lie in host_alleles(): {offset, length} of allele 0 and of allele 1.  The packed forms read what avk_packed_host_alleles made
 * (aoff, w0, w1); the others their own arrays, and ignore the three. */
struct AvkAllelePair {
    uint64_t o0, l0, o1, l1;
};
static inline AvkAllelePair avk_pending_allele(const UploadSource &u, uint64_t v, const uint64_t *aoff, const uint32_t *w0, const uint32_t *w1) {
    switch (u.form) {
    case UploadSource::WIDE: return {u.wide->a0_off[v], u.wide->a0_len[v], u.wide->a1_off[v], u.wide->a1_len[v]};
    case UploadSource::COMPACT: return {u.compact->a_off[v], u.compact->a0_len[v], (uint64_t)u.compact->a_off[v] + u.compact->a0_len[v], u.compact->a1_len[v]};
    case UploadSource::MULTI: return {u.multi->a0_off[v], u.multi->a0_len[v], u.multi->a1_off[v], u.multi->a1_len[v]};
    default: return {aoff[v], w0[v], aoff[v] + w0[v], w1[v]};
    }
}

/* The bucket of a batch's need histogram (DpState::need_hist; bucket k: slices of 1 MB << k) that is large enough for 98 % of the regions predicted to need the
 * HBM tier: 0 for fewer than 64 such regions, 6 (64 MB) at most. */
static inline int avk_slice_pick(const uint64_t *need_hist, int n_buckets) {
    uint64_t n_c = 0, run = 0;
    for (int k = 0; k < n_buckets; ++k) n_c += need_hist[k];
    int pick = 0;
    for (int k = 0; k < n_buckets && n_c >= 64; ++k) {
        run += need_hist[k];
        pick = k;
        if (run * 100 >= n_c * 98) break;
    }
    return pick > 6 ? 6 : pick;
}

#endif
