/*
 * context_emu.cpp — the sequence-context labels of a stratified job (aardvark_amd/csrc/avk_context.inl: GC bins, homopolymer classes) on the CPU.
 *
 * Test infrastructure like strata_emu.cpp, and a translation unit of its own: cx_region_bits is one-lane code (no cross-lane primitive), so the SAME source the
 * gfx950 kernel runs is called here region by region, on the arrays the device would hold — the wide arrays of a batch, the byte copy of the reference, and the
 * 2-bit copy with its flag bitmap laid out as avk_pack_reference lays them out — and the bits are compared with a numpy restatement of the rule
 * (tests/context_lib.py, tests/test_context_strata.py).  Built by tests/context_emu_lib.py with the flags of tests/emu/Makefile.
 */
#define AVK_EMU 1
#include <string.h>

#include <vector>

#include "../../aardvark_amd/csrc/avk_context.inl"

namespace {

/* the reference as avk_ref_upload leaves it: the contigs concatenated (64 bytes of room behind them), the packed copy and its flag bitmap in the sizes it
 * allocates, filled as avk_pack_reference fills them */
struct EmuRef {
    std::vector<uint8_t> bytes;
    std::vector<uint32_t> packed, exc;
    std::vector<uint64_t> tab; /* contig_base[n] then contig_len[n] */
    avk::cx::CxRef view;
    EmuRef(const uint8_t *const *seqs, const uint64_t *lens, uint32_t n_contigs) {
        tab.assign(2 * (size_t)n_contigs + 2, 0);
        uint64_t total = 0;
        for (uint32_t c = 0; c < n_contigs; ++c) tab[c] = total, tab[n_contigs + c] = lens[c], total += lens[c];
        bytes.assign(total + 64, 0);
        for (uint32_t c = 0; c < n_contigs; ++c)
            if (lens[c]) memcpy(bytes.data() + tab[c], seqs[c], lens[c]);
        const uint64_t n_words = (total + 15) >> 4;
        packed.assign(n_words + 80, 0);
        exc.assign((n_words >> 5) + 8, 0);
        for (uint64_t p = 0; p < total; ++p) {
            const uint8_t ch = bytes[p];
            const uint32_t code = ch == 'A' ? 0u : ch == 'C' ? 1u : ch == 'G' ? 2u : ch == 'T' ? 3u : 4u;
            if (code > 3u) exc[(p >> 4) >> 5] |= 1u << ((p >> 4) & 31);
            else packed[p >> 4] |= code << (2 * (p & 15));
        }
        view.bytes = bytes.data(), view.packed = packed.data(), view.exc = exc.data(), view.contig_base = tab.data(), view.contig_len = tab.data() + n_contigs, view.n_contigs = n_contigs;
    }
};

} // namespace

extern "C" {

/* the device view of a batch's wide arrays (names of avk::dp::DpIn), as strata_emu_view has them */
struct context_emu_view {
    uint64_t n_regions, n_variants;
    const uint32_t *contig_idx;
    const uint64_t *start, *t_off, *q_off;
    const uint32_t *t_cnt, *q_cnt;
    const uint64_t *var_pos;
    const uint32_t *a0_len;
};

int context_emu_spec_size(void) { return (int)sizeof(avk::cx::CxSpec); }

/* bits[n_regions]: cx_region_bits of every region */
int context_emu_region_bits(const context_emu_view *e, const uint8_t *const *seqs, const uint64_t *lens, uint32_t n_contigs, const avk::cx::CxSpec *spec, uint32_t *bits) {
    avk::dp::DpIn in;
    memset(&in, 0, sizeof(in));
    in.n_regions = e->n_regions, in.n_variants = e->n_variants;
    in.contig_idx = e->contig_idx, in.start = e->start, in.t_off = e->t_off, in.q_off = e->q_off, in.t_cnt = e->t_cnt, in.q_cnt = e->q_cnt, in.var_pos = e->var_pos, in.a0_len = e->a0_len;
    const EmuRef ref(seqs, lens, n_contigs);
    for (uint64_t r = 0; r < e->n_regions; ++r) bits[r] = avk::cx::cx_region_bits(in, ref.view, *spec, r);
    return 0;
}

/* the bits of explicit spans [first[k], last[k]] of contig[k]; force_bytes: every word read from the byte copy (the two routes against each other) */
int context_emu_span_bits(const uint8_t *const *seqs, const uint64_t *lens, uint32_t n_contigs, const avk::cx::CxSpec *spec, uint64_t n, const uint32_t *contig,
                          const uint64_t *first, const uint64_t *last, int force_bytes, uint32_t *bits) {
    const EmuRef ref(seqs, lens, n_contigs);
    for (uint64_t k = 0; k < n; ++k) {
        avk::sx::SxSpan sp;
        sp.first = first[k], sp.last = last[k], sp.contig = contig[k], sp.ok = true;
        bits[k] = avk::cx::cx_span_bits(ref.view, *spec, sp, force_bytes != 0);
    }
    return 0;
}

/* (a, g, longest run) of the window [lo, hi) of the concatenated reference by one route: out[3] */
int context_emu_counts(const uint8_t *const *seqs, const uint64_t *lens, uint32_t n_contigs, uint64_t lo, uint64_t hi, int force_bytes, uint64_t *out) {
    const EmuRef ref(seqs, lens, n_contigs);
    const avk::cx::CxCounts c = avk::cx::cx_scan(ref.view, lo, hi, true, force_bytes != 0);
    out[0] = c.a, out[1] = c.g, out[2] = c.run;
    return 0;
}

/* what avk_context_mask_kernel's lanes do to the word-major masks the BED labels' kernel left (mask[w * n + r]): cx_store_region — the shared word OR-ed into,
 * every later word stored; fresh: the first word stored too.  Returns the number of context hits. */
uint64_t context_emu_place(const uint32_t *bits, uint64_t n, uint32_t n_bed, uint32_t n_ctx, int fresh, uint32_t *mask) {
    uint64_t hits = 0;
    for (uint64_t r = 0; r < n; ++r) {
        avk::cx::cx_store_region(mask, r, n, bits[r], n_bed, n_ctx, fresh != 0);
        hits += (uint64_t)avk_popc64(bits[r]);
    }
    return hits;
}

} /* extern "C" */
