// The step plans of csrc/avk_step_plan.h, printed for tests/test_step_plan.py: a line per queue count and per kind of step,
//   queues <n> lanes <0|1> slots <n_slots> : <slot of chain 0> <slot of chain 1> ...
// and what avk_step_plan_parse makes of a few strings.
#include <cstdio>

#include "../../aardvark_amd/csrc/avk_step_plan.h"

int main() {
    printf("chains %d\n", (int)AVK_N_CHAINS);
    for (int q = -1; q <= 40; ++q)
        for (int lanes = 0; lanes < 2; ++lanes) {
            const AvkStepPlan p = avk_step_plan(q, lanes != 0);
            printf("queues %d lanes %d slots %d :", q, lanes, p.n_slots);
            for (int c = 0; c < AVK_N_CHAINS; ++c) printf(" %d", p.slot[c]);
            printf("\n");
        }
    const char *trials[] = {"03302012", "00000000", "01230123", "13302012", "0330201", "033020123", "04302012", "0330201x", ""};
    for (const char *t : trials) {
        AvkStepPlan p;
        printf("parse '%s' %d\n", t, avk_step_plan_parse(t, &p) ? 1 : 0);
    }
    AvkStepPlan p;
    printf("parse null %d\n", avk_step_plan_parse(nullptr, &p) ? 1 : 0);
    printf("step_plan_check: ok\n");
    return 0;
}
