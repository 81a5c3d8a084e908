// plan_pair_main.cc -- plan_levels_wg_slots of csrc/lqr_plan.h and lv2_grid / lv2_block of csrc/lqr_geom.h alone, without a GPU
// (tests/test_levels_pair_plan.py builds this with -Werror under AddressSanitizer and UndefinedBehaviorSanitizer).
//   plan: for every line "group hw_queues spin knob wgs_levels2" on stdin -- a lock-step group of 4K carvers at delta_x 1 in a process with
//         that many hardware queues, spinning kernels allowed or not, the lqrhip_set_levels_wg_slots knob, the device's residency bound
//         of k_band_levels2 -- prints "streams images P wg_slots" of the group's first batch
//   map:  for every line "n P" prints lv2_grid(n, P), then "image slot" of every block
#include <stdio.h>
#include <string.h>
#include "lqr_plan.h"

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "plan")) {
        int group, queues, spin, knob, wgs2;
        while (scanf("%d %d %d %d %d", &group, &queues, &spin, &knob, &wgs2) == 5) {
            PlanKnobs k;
            PlanDevice d;
            PlanBatch b;
            k.levels_wg_slots = knob;
            d.wgs_plain = d.wgs_general = d.wgs_px4 = d.n_cu = 256;
            d.wgs_levels = 768; d.wgs_levels2 = wgs2;
            d.hw_queues = queues;
            const int nb = plan_streams(k, d, group);
            b.images = (group + nb - 1) / nb; b.shared_n = nb; b.shared = nb > 1; b.spin = spin != 0; b.wk_h = 2160;
            const StepPlan s = plan_seam_step(k, d, b, 1, false, 3840, 2160, false, 1);
            printf("%d %d %d %d\n", nb, b.images, s.levels_P, s.levels_wg_slots);
        }
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "map")) {
        int n, P;
        while (scanf("%d %d", &n, &P) == 2) {
            const unsigned grid = lv2_grid((size_t) n, P);
            printf("%u\n", grid);
            for (unsigned blk = 0; blk < grid; blk++) {
                const LvBlock m = lv2_block((int) blk, P);
                printf("%d %d\n", m.image, m.slot);
            }
        }
        return 0;
    }
    return 2;
}
