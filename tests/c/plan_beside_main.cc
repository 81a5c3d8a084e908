// plan_beside_main.cc -- csrc/lqr_plan.h alone, without a GPU (tests/test_plan_beside.py builds this with -Werror under
// AddressSanitizer and UndefinedBehaviorSanitizer): where a seam step runs the energy update beside the carve (StepPlan::energy_beside).
// Reads the knob (lqrhip_set_carve_beside's -1 / 0 / 1) from stdin; prints the threshold CARVE_BESIDE_MIN and the knob's default, then
// one line per combination of group size 1 .. 96 (as one batch, and as sub-batches of 2 and 4 sibling streams where the size
// divides), delta_x 0 .. 4, value plane or packed pixels, frame widths 2, 3 and 100:
//   images shared_n delta value w carve energy_beside carve_with_the_knob_at_0
#include <stdio.h>
#include "lqr_plan.h"
#include "lqr_hip.h"

int main(void)
{
    PlanKnobs k, off;
    PlanDevice d;
    d.wgs_plain = d.wgs_general = d.wgs_px4 = d.wgs_levels = d.n_cu = 256;
    d.hw_queues = 4;
    printf("min %d default %d\n", CARVE_BESIDE_MIN, k.carve_beside);
    if (scanf("%d", &k.carve_beside) != 1) return 2;
    off.carve_beside = 0;
    static const int widths[] = {2, 3, 100};
    for (int n = 1; n <= 96; n++)
        for (int sn : {1, 2, 4}) {
            if (n % sn) continue;
            for (int delta = 0; delta <= 4; delta++)
                for (int value = 0; value <= 1; value++)
                    for (int w : widths) {
                        PlanBatch b;
                        b.images = n / sn; b.shared_n = sn; b.shared = sn > 1; b.wk_h = 70; b.value = value != 0;
                        const StepPlan s = plan_seam_step(k, d, b, delta, false, w, 70, false, 0);
                        const StepPlan s0 = plan_seam_step(off, d, b, delta, false, w, 70, false, 0);
                        printf("%d %d %d %d %d %d %d %d\n", n, sn, delta, value, w, s.carve, (int) s.energy_beside, s0.carve);
                    }
        }
    return 0;
}
