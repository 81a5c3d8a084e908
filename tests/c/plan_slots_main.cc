// plan_slots_main.cc -- plan_levels_P of csrc/lqr_plan.h alone, without a GPU (tests/test_plan_slots.py builds this with -Werror under
// AddressSanitizer and UndefinedBehaviorSanitizer).  Prints "LV_PMAX LV_AUTO_MIN", then for every line
//   images shared_n shared wgs_levels band_levels
// on stdin (a batch of `images` carvers, one of `shared_n` sub-batches of its group, `shared` 0 / 1; the device's residency bound of
// k_band_levels; the lqrhip_set_band_levels knob) the slots per image the plan gives a 4K frame at delta_x 1.
#include <stdio.h>
#include "lqr_plan.h"

int main(void)
{
    printf("%d %d\n", LV_PMAX, LV_AUTO_MIN);
    int images, shared_n, shared, wgs, knob;
    while (scanf("%d %d %d %d %d", &images, &shared_n, &shared, &wgs, &knob) == 5) {
        PlanKnobs k;
        PlanDevice d;
        PlanBatch b;
        k.band_levels = knob;
        d.wgs_plain = d.wgs_general = d.wgs_px4 = d.n_cu = 256;
        d.wgs_levels = wgs;
        d.hw_queues = 4;
        b.images = images; b.shared_n = shared_n; b.shared = shared != 0; b.wk_h = 2160;
        printf("%d\n", plan_levels_P(k, d, b, 3839, 2160, 1));
    }
    return 0;
}
