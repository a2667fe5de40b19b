/*
 * avk_counters.h — the map of avk_dev_batch::d_counters, the block of 32-bit words the launches of one solver step coordinate
 * through: which words belong to which launch.  Plain C++ (no HIP): shared by run_internal (avk_host.hip), the kernels
 * (avk_solver.inl), the emulator's copy of the step's wiring (tests/emu/wave_emu.cpp) and the diagnostic tools.
 *
 * Every range is a first word NAME and a length NAME_LEN, and is listed in AVK_CTR_RANGE_LIST below: the checks at the end of this
 * file refuse a range that intersects another one or ends behind the block.  A launch that needs a word takes a free one, gives it a
 * name here and adds it to the list.  The block is all zero between steps (avk_tally_reduce clears it).
 */
#ifndef AVK_COUNTERS_H
#define AVK_COUNTERS_H

#include <stdint.h>
#include "avk_dev_types.h"

constexpr uint32_t AVK_N_COUNTERS = 1408; /* words of avk_dev_batch::d_counters */

/* ---- claim cursors of the tier launches: AvkKernelArgs::work_counter of the launch of tier t is the tier's block; shard s of its
 * work list claims at word AVK_CTR_SHARD_STRIDE * s of it (128 bytes apart), n_shards <= AVK_CTR_SHARDS */
constexpr uint32_t AVK_CTR_SHARD_STRIDE = 32, AVK_CTR_SHARDS = 8, AVK_CTR_TIER_STRIDE = 256;
constexpr uint32_t AVK_CTR_TIER_CURSORS = 0, AVK_CTR_TIER_CURSORS_LEN = 4 * AVK_CTR_TIER_STRIDE;
constexpr uint32_t avk_ctr_tier_cursors(uint32_t tier) { return AVK_CTR_TIER_CURSORS + AVK_CTR_TIER_STRIDE * tier; }
static_assert(AVK_CTR_SHARD_STRIDE * AVK_CTR_SHARDS <= AVK_CTR_TIER_STRIDE, "a tier's shards stay inside the tier's block");
/* Two launches of the lane path borrow the blocks of tiers that have no launch of their own then.  Aliases, not ranges: they are safe
 * because use_fast (run_internal) requires launch[1] and launch[3] to be off — with the lanes on, tiers 1 and 3 never start a launch
 * that would claim through these words. */
constexpr uint32_t AVK_CTR_DEFERRED_CURSORS = avk_ctr_tier_cursors(3); /* the deferred LDS launch for what the lanes hand back (up to 8 shards) */
constexpr uint32_t AVK_CTR_LAST_CURSOR = avk_ctr_tier_cursors(1);      /* the HBM launch at the end of the step for what that launch could not hold */

/* ---- lengths of the overflow lists: list k of run_internal's lists[] (k < 3: two between the tier launches, the lanes' deferred list) */
constexpr uint32_t AVK_CTR_OVERFLOW_LISTS = 3, AVK_CTR_OVERFLOW_STRIDE = 16;
constexpr uint32_t AVK_CTR_OVERFLOW_COUNTS = 1024, AVK_CTR_OVERFLOW_COUNTS_LEN = AVK_CTR_OVERFLOW_STRIDE * (AVK_CTR_OVERFLOW_LISTS - 1) + 1;
constexpr uint32_t avk_ctr_overflow_count(uint32_t k) { return AVK_CTR_OVERFLOW_COUNTS + AVK_CTR_OVERFLOW_STRIDE * k; }
constexpr uint32_t AVK_CTR_DEFERRED_LIST = 2; /* the list the lane launches hand over to (without hand-back chains) */

constexpr uint32_t AVK_CTR_LDS_SOLO_CURSOR = 1072, AVK_CTR_LDS_SOLO_CURSOR_LEN = 1; /* class B: the LDS solo launch */
constexpr uint32_t AVK_CTR_HBM_SOLO_TICKET = 1076, AVK_CTR_HBM_SOLO_TICKET_LEN = 1; /* class C: the HBM solo launch, shared with the main HBM launch (AvkKernelArgs::extra_counter) */

/* ---- busy flags of the shared big slices (AvkKernelArgs::big_busy, one word per slice): the length is the most slices a launch may be given */
constexpr uint32_t AVK_CTR_BIG_BUSY = 1088, AVK_CTR_BIG_BUSY_LEN = 128;

/* ---- tile cursors of the lane launches, one per class: the class's launch, and the launch of its head */
constexpr uint32_t AVK_CTR_LANE_TILES = 1220, AVK_CTR_LANE_TILES_LEN = AVK_FAST_CLASSES;
constexpr uint32_t AVK_CTR_HEAD_TILES = 1230, AVK_CTR_HEAD_TILES_LEN = AVK_FAST_CLASSES;

/* ---- the launches of avk_wide.inl: a claim cursor each, and the length of the list of what the launch could not take */
constexpr uint32_t AVK_CTR_WIDE_C_CURSOR = 1240, AVK_CTR_WIDE_C_CURSOR_LEN = 1;         /* class C */
constexpr uint32_t AVK_CTR_WIDE_C_LEFT = 1244, AVK_CTR_WIDE_C_LEFT_LEN = 1;
constexpr uint32_t AVK_CTR_WIDE_HB3_CURSOR = 1248, AVK_CTR_WIDE_HB3_CURSOR_LEN = 1;     /* the hand-backs of the three-call lane class */
constexpr uint32_t AVK_CTR_WIDE_HB3_LEFT = 1252, AVK_CTR_WIDE_HB3_LEFT_LEN = 1;
constexpr uint32_t AVK_CTR_WIDE_LANES_CURSOR = 1260, AVK_CTR_WIDE_LANES_CURSOR_LEN = 1; /* the deferred list (without hand-back chains) */
constexpr uint32_t AVK_CTR_WIDE_LANES_LEFT = 1264, AVK_CTR_WIDE_LANES_LEFT_LEN = 1;     /* ... and what every chain's launch leaves */
constexpr uint32_t AVK_CTR_WIDE_RETRY_CURSOR = 1268, AVK_CTR_WIDE_RETRY_CURSOR_LEN = 1; /* class C once more with a workgroup's LDS */
constexpr uint32_t AVK_CTR_WIDE_RETRY_LEFT = 1272, AVK_CTR_WIDE_RETRY_LEFT_LEN = 1;

/* ---- the launch beside class C's wide launch: the records that are not the wide kernel's, or the team launch of the long windows.
 * A team writes its progress (team_run, avk_solver.inl) to words it finds relative to the cursor it was handed. */
constexpr uint32_t AVK_CTR_TEAM_CURSOR = 1256, AVK_CTR_TEAM_CURSOR_LEN = 1;
constexpr uint32_t AVK_CTR_TEAM_PROGRESS_REL = 17; /* work_counter + this: [gen, stage, n, -, kind, -, -] */
constexpr uint32_t AVK_CTR_TEAM_PROGRESS = AVK_CTR_TEAM_CURSOR + AVK_CTR_TEAM_PROGRESS_REL, AVK_CTR_TEAM_PROGRESS_LEN = 7;

/* ---- hand-back chains: segment i of the deferred list has its length at AVK_CTR_HB_COUNTS + i and the cursor of the launch that reads
 * it at AVK_CTR_HB_CURSORS + i.  run_internal makes at most two chains, eight staged heads and the pairs' own list. */
constexpr uint32_t AVK_CTR_HB_HEADS = 8, AVK_CTR_HB_SEGS = 2 + AVK_CTR_HB_HEADS + 1;
constexpr uint32_t AVK_CTR_HB_COUNTS = 1296, AVK_CTR_HB_COUNTS_LEN = AVK_CTR_HB_SEGS;
constexpr uint32_t AVK_CTR_HB_CURSORS = 1328, AVK_CTR_HB_CURSORS_LEN = AVK_CTR_HB_SEGS;

/* ---- the three-call lane class: length of its hand-back list, and the cursor of the HBM-tier launch that reads it */
constexpr uint32_t AVK_CTR_HB3_COUNT = 1344, AVK_CTR_HB3_COUNT_LEN = 1;
constexpr uint32_t AVK_CTR_HB3_CURSOR = 1376, AVK_CTR_HB3_CURSOR_LEN = 1;

#define AVK_CTR_RANGE_LIST(X)                                                                                                             \
    X(AVK_CTR_TIER_CURSORS) X(AVK_CTR_OVERFLOW_COUNTS) X(AVK_CTR_LDS_SOLO_CURSOR) X(AVK_CTR_HBM_SOLO_TICKET) X(AVK_CTR_BIG_BUSY)          \
    X(AVK_CTR_LANE_TILES) X(AVK_CTR_HEAD_TILES) X(AVK_CTR_WIDE_C_CURSOR) X(AVK_CTR_WIDE_C_LEFT) X(AVK_CTR_WIDE_HB3_CURSOR)                \
    X(AVK_CTR_WIDE_HB3_LEFT) X(AVK_CTR_TEAM_CURSOR) X(AVK_CTR_WIDE_LANES_CURSOR) X(AVK_CTR_WIDE_LANES_LEFT) X(AVK_CTR_WIDE_RETRY_CURSOR)  \
    X(AVK_CTR_WIDE_RETRY_LEFT) X(AVK_CTR_TEAM_PROGRESS) X(AVK_CTR_HB_COUNTS) X(AVK_CTR_HB_CURSORS) X(AVK_CTR_HB3_COUNT) X(AVK_CTR_HB3_CURSOR)

/* ---- launch arguments that are the same wherever they occur (run_internal and the emulator's copy of it) ---- */

/* A launch of the wave-per-region kernels that reads a hand-over list: record indices from `list`, whose length the device holds at
 * *n_work_dev, claimed one at a time through one cursor; none of the bulk launch's static share, shards, escalation or second work source,
 * and nowhere to hand over to (what the launch cannot hold fails with CAPACITY unless the caller names a list).  list == NULL: the records
 * [work_base, work_base + n_work) themselves, which the caller sets.  The tier, the priority, the waves and the workspaces are the caller's. */
static inline AvkKernelArgs avk_list_reader_args(const AvkKernelArgs &base, const uint32_t *list, const uint32_t *n_work_dev, uint32_t *cursor) {
    AvkKernelArgs r = base;
    r.work_list = list;
    r.n_work_dev = n_work_dev;
    r.work_base = 0;
    r.n_work = 0;
    r.work_counter = cursor;
    r.static_pct = 0;
    r.n_shards = 1;
    r.claim = 1;
    r.esc_bytes = 0;
    r.esc_enabled = 0;
    r.extra_counter = nullptr;
    r.extra_n = 0;
    r.overflow_list = nullptr;
    r.overflow_count = nullptr;
    return r;
}

/* the shared big slices an HBM-tier launch escalates into: big_slots <= AVK_CTR_BIG_BUSY_LEN slices of tier[3] bytes at big_ws, their flags in the batch's counters */
static inline void avk_big_slice_args(AvkKernelArgs &x, uint8_t *big_ws, uint32_t *counters, uint32_t big_slots) {
    x.big_ws = big_ws;
    x.big_busy = counters + AVK_CTR_BIG_BUSY;
    x.big_slots = big_slots;
}

/* ---- the checks: no two ranges intersect, none ends behind the block ---- */
struct AvkCtrRange {
    uint32_t first, len;
};
#define AVK_CTR_ENTRY(R) {R, R##_LEN},
constexpr AvkCtrRange AVK_CTR_RANGES[] = {AVK_CTR_RANGE_LIST(AVK_CTR_ENTRY)};
#undef AVK_CTR_ENTRY
/* how many ranges of the table hold a word of [first, first + len): one for a range of the table, itself */
constexpr int avk_ctr_ranges_touching(uint32_t first, uint32_t len) {
    int n = 0;
    for (const AvkCtrRange &r : AVK_CTR_RANGES)
        if (first < r.first + r.len && r.first < first + len) n += 1;
    return n;
}
#define AVK_CTR_CHECK(R)                                                                                     \
    static_assert(R##_LEN > 0 && R + R##_LEN <= AVK_N_COUNTERS, #R " ends behind AVK_N_COUNTERS");           \
    static_assert(avk_ctr_ranges_touching(R, R##_LEN) == 1, #R " intersects another range of d_counters");
AVK_CTR_RANGE_LIST(AVK_CTR_CHECK)
#undef AVK_CTR_CHECK

#endif
