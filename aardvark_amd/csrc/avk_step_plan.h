/* The launch chains of a solver step (Step, avk_step.inl) and the stream each of them is queued on.
 *
 * A chain is a run of launches that follow each other in stream order; chains run beside each other.  The step names chains only; the plan says which of the
 * context's streams ("slots") a chain is queued on.  Two plans:
 *
 *   wide    one stream per chain (slot == chain).  For processes with eight or more hardware queues (GPU_MAX_HW_QUEUES): every chain has a queue of its own.
 *   folded  the caller's stream and three more.  For processes with fewer queues, where streams that share a queue run in turn anyway and WHICH of them share one
 *           is left to the runtime: here whole chains are queued one behind the other on a stream, in the order the step queues them, and the events that
 *           forked and joined two chains of one stream are dropped (stream order does their work).
 *
 * Plain C++, no HIP types: tests/native/step_plan_check.cpp compiles this header for the CPU. */
#ifndef AVK_STEP_PLAN_H
#define AVK_STEP_PLAN_H

enum AvkStepChain {
    AVK_CH_CALLER = 0,     /* the caller's stream: bulk, the HBM tiers, what the chains left, the tally */
    AVK_CH_LDS_SOLO,       /* class B: the LDS solo launch */
    AVK_CH_NOT_WIDE,       /* class C records that are not the wide kernel's: their list, then their HBM-tier (or team) launch */
    AVK_CH_CLASS_C,        /* class C: the wide launch, its retry with a workgroup's LDS, the HBM solo launch for what is left */
    AVK_CH_TWO_CALL,       /* lane classes with two calls per side: heads, the rest, the chain's hand-backs */
    AVK_CH_ONE_CALL,       /* the looked-up pairs and the one-call lane classes, the chain's hand-backs */
    AVK_CH_THREE_CALL,     /* the three-call lane class, its hand-backs through the wide kernel and the HBM tier */
    AVK_CH_HEAD_HANDBACKS, /* what the staged heads hand back, each list behind its head launch */
    AVK_N_CHAINS
};

/* The ends of the chains: each is an event (avk_ctx::ev_end) recorded behind the last launch of a chain — or, for the three-call class, behind its lane launch
 * (AVK_END_LANE2) and again behind the launches for what it handed back (AVK_END_EARLY).  The caller's stream waits for them; AVK_TIMING prints when each fired. */
enum AvkStepEnd {
    AVK_END_LDS_SOLO,
    AVK_END_CLASS_C,
    AVK_END_NOT_WIDE,
    AVK_END_LANE0, /* the lane chains, in the order of AvkStepChain: two-call, one-call, three-call, the heads' hand-backs */
    AVK_END_LANE1,
    AVK_END_LANE2,
    AVK_END_LANE3,
    AVK_END_EARLY,
    AVK_END_DONE, /* a step without hand-back chains: the launch for everything the lanes handed back */
    AVK_N_ENDS
};
static const char *const AVK_STEP_END_NAME[AVK_N_ENDS] = {"LDS solo",      "HBM solo",      "wide",           "lane stream 1",     "lane stream 2",
                                                          "lane stream 3", "lane stream 4", "early hand-backs", "hand-back launches"};

enum { AVK_STEP_SLOTS_FOLDED = 4, AVK_STEP_QUEUES_WIDE = 8 /* from this many hardware queues on: a stream per chain */ };

struct AvkStepPlan {
    int slot[AVK_N_CHAINS]; /* slot 0 is the caller's stream */
    int n_slots;            /* slots in use: AVK_N_CHAINS or AVK_STEP_SLOTS_FOLDED */
};

/* chain -> slot of the folded plan.  Queue order on a slot is the step's: the solo chains ahead of the lane chains (class C, then the one-call classes, ahead of the
 * bulk on the caller's stream; the LDS solo launch ahead of the two-call classes; the long launch of the records that are not the wide kernel's ahead of the heads'
 * hand-backs, which wait for their head anyway).  By the chains' durations in a four-queue trace this is the best split into four (2.46 ms on the longest stream);
 * profiles/step_four_queues.txt has the trace and the three assignments that were measured. */
static const int AVK_STEP_FOLDED_SLOTS[AVK_N_CHAINS] = {
    /* caller */ 0, /* LDS solo */ 2, /* not wide */ 3, /* class C */ 0, /* two-call */ 2, /* one-call */ 0, /* three-call */ 1, /* heads' hand-backs */ 3,
};
/* a step without lane launches has four chains: a stream each (class C beside the bulk, not ahead of it) */
static const int AVK_STEP_FOLDED_SLOTS_NO_LANES[AVK_N_CHAINS] = {0, 1, 2, 3, 2, 0, 1, 2};

/* n_queues: the hardware queues the process has (GPU_MAX_HW_QUEUES); 0 or negative: not known, the wide plan.  lanes: the step has lane launches */
static inline AvkStepPlan avk_step_plan(int n_queues, bool lanes = true) {
    AvkStepPlan p;
    const bool wide = n_queues <= 0 || n_queues >= AVK_STEP_QUEUES_WIDE;
    for (int c = 0; c < AVK_N_CHAINS; ++c) p.slot[c] = wide ? c : lanes ? AVK_STEP_FOLDED_SLOTS[c] : AVK_STEP_FOLDED_SLOTS_NO_LANES[c];
    p.n_slots = wide ? (int)AVK_N_CHAINS : (int)AVK_STEP_SLOTS_FOLDED;
    return p;
}

/* a plan from a string of AVK_N_CHAINS digits, chain by chain (AVK_STEP_PLAN, for measurements): false when the string is not a folded plan */
static inline bool avk_step_plan_parse(const char *s, AvkStepPlan *p) {
    if (!s) return false;
    for (int c = 0; c < AVK_N_CHAINS; ++c) {
        if (s[c] < '0' || s[c] >= '0' + AVK_STEP_SLOTS_FOLDED) return false;
        p->slot[c] = s[c] - '0';
    }
    if (s[AVK_N_CHAINS] != 0 || p->slot[AVK_CH_CALLER] != 0) return false;
    p->n_slots = AVK_STEP_SLOTS_FOLDED;
    return true;
}

#endif
