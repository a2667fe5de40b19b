/*
 * kind_check.cpp — the functions of aardvark_amd/csrc/avk_callkind.h behind a C interface, for tests/test_kind_rule.py (built into a small library of its own by
 * tests/kind_lib.py).  Test infrastructure: nothing but the header is compiled here.
 */
#include "../../aardvark_amd/csrc/avk_callkind.h"

extern "C" {

uint32_t kind_check_n(void) { return AVK_N_KINDS; }
uint32_t kind_check_gt(uint32_t zyg) { return avk_kind_gt_of(zyg); }
uint32_t kind_check_sub(uint32_t a0_len, uint32_t a1_len, uint32_t b0, uint32_t b1) { return avk_kind_sub_of(a0_len, a1_len, b0, b1); }
uint32_t kind_check_kind(uint32_t gt, uint32_t sub) { return avk_kind_of(gt, sub); }
uint32_t kind_check_field(uint32_t k, int query) { return avk_size_field_of(k, query); }
const char *kind_check_name(uint32_t k) { return avk_kind_name_of(k); }
/* sub of every pair of bytes at lengths 1 / 1: out[b0 * 256 + b1] */
void kind_check_pairs(uint8_t *out) {
    for (uint32_t b0 = 0; b0 < 256; ++b0)
        for (uint32_t b1 = 0; b1 < 256; ++b1) out[b0 * 256 + b1] = (uint8_t)avk_kind_sub_of(1, 1, b0, b1);
}

} /* extern "C" */
