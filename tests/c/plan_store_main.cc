// plan_store_main.cc -- plan_levels_store of csrc/lqr_plan.h alone, without a GPU (tests/test_levels_store_plan.py builds this with
// -Werror under AddressSanitizer and UndefinedBehaviorSanitizer).  For every line "group hw_queues spin knob" on stdin -- a lock-step
// group of 4K carvers at delta_x 1 in a process with that many hardware queues, spinning kernels allowed or not, the
// lqrhip_set_levels_store knob -- prints "streams images P wg_slots store_rows" of the group's first batch
#include <stdio.h>
#include "lqr_plan.h"

int main()
{
    int group, queues, spin, knob;
    while (scanf("%d %d %d %d", &group, &queues, &spin, &knob) == 4) {
        PlanKnobs k;
        PlanDevice d;
        PlanBatch b;
        k.levels_store = knob;
        d.wgs_plain = d.wgs_general = d.wgs_px4 = d.n_cu = 256;
        d.wgs_levels = 768; d.wgs_levels2 = 256;
        d.hw_queues = queues;
        const int nb = plan_streams(k, d, group);
        b.images = (group + nb - 1) / nb; b.shared_n = nb; b.shared = nb > 1; b.spin = spin != 0; b.wk_h = 2160;
        const StepPlan s = plan_seam_step(k, d, b, 1, false, 3840, 2160, false, 1);
        printf("%d %d %d %d %d\n", nb, b.images, s.levels_P, s.levels_wg_slots, s.levels_store);
    }
    return 0;
}
