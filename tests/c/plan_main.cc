// plan_main.cc -- csrc/lqr_plan.h alone, without a GPU (tests/test_plan.py builds this with -Werror under AddressSanitizer and
// UndefinedBehaviorSanitizer).  Device inputs: 256 compute units and 256 workgroups for each residency bound, an MI355X's figures
// (profiles/shimforms/README.md).  The first word on stdin selects what is done:
//   census   the knobs, delta_x, use_rigidity, rigmask, then "D w h" (a session's first full DP) and "S w h full_rebuild" (a seam step)
//            lines of ONE 8-bit image: prints the LQRHIP_CENSUS_SLOTS counters that launching those plans adds up to
//   sweep    plans over widths, heights, delta_x, group sizes and spinning on / off: what the launch code relies on must hold
//   rules    the frozen lag per batch size and k_emap_update's samples per delta_x, as the plans give them
#include <stdio.h>
#include <string.h>
#include "lqr_plan.h"
#include "lqr_hip.h"

static PlanDevice mi355x(void)
{
    PlanDevice d;
    d.wgs_plain = d.wgs_general = d.wgs_px4 = d.wgs_levels = d.n_cu = 256;
    d.hw_queues = 8;
    return d;
}

static bool is_tile_p(int form) { return form >= LQRHIP_CENSUS_TILE_P_G3 && form <= LQRHIP_CENSUS_TILE_P_GENERAL; }

// what launching the plan counts (lqr_shim.hip: launch_dp, launch_dp_persistent, launch_dp_tiled)
static void count_dp(unsigned long long *c, const DpPlan &dp, const PlanBatch &b, int h)
{
    if (dp.form == LQRHIP_CENSUS_DP_TILE) c[dp.form] += (unsigned) ((h + DPT_ROWS - 1) / DPT_ROWS);
    else if (is_tile_p(dp.form)) c[dp.form] += (unsigned) ((b.images + dp.per - 1) / dp.per);
    else if (dp.form >= 0) {
        const int lg = dp.px == 1 ? 0 : dp.px == 2 ? 1 : dp.px == 4 ? 2 : dp.px == 8 ? 3 : 4;
        c[LQRHIP_CENSUS_SWEEP + 2 * lg + (dp.threads == DP_THREADS ? 1 : 0)]++;
        c[dp.form]++;
        if (lds_needs_attr(dp.lds)) c[LQRHIP_CENSUS_LDS_ATTR_SWEEP]++;
    }
}

static int census(void)
{
    PlanKnobs k;
    PlanBatch b;
    const PlanDevice d = mi355x();
    int spin, delta, use_rig, rigmask;
    if (scanf("%d %d %d %d %d %d %d %d %d %d %d %d", &k.vpath_mode, &k.vpath_par_max, &k.sweep_threads, &k.carve_fused, &k.update_mode,
              &k.band_levels, &k.dpp_limit, &k.dpp_px, &spin, &delta, &use_rig, &rigmask) != 12) return 2;
    b.spin = spin != 0; b.rigmask = rigmask != 0;
    unsigned long long c[LQRHIP_CENSUS_SLOTS];
    memset(c, 0, sizeof c);
    char what[8];
    int w, h, full;
    while (scanf("%7s %d %d", what, &w, &h) == 3) {
        b.wk_h = h;
        if (what[0] == 'D') { count_dp(c, plan_full_dp(k, d, b, w, delta, use_rig != 0), b, h); continue; }
        if (scanf("%d", &full) != 1) return 2;
        const StepPlan s = plan_seam_step(k, d, b, delta, use_rig != 0, w, h, full != 0, 0);
        c[s.backtrack]++; c[s.carve]++;
        if (s.band >= 0) c[s.band]++;
        count_dp(c, s.dp, b, h);
    }
    for (int i = 0; i < LQRHIP_CENSUS_SLOTS; i++) printf("%llu%c", c[i], i + 1 < LQRHIP_CENSUS_SLOTS ? ' ' : '\n');
    return 0;
}

static long g_failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_failures++ < 20) { fprintf(stderr, "%s: ", #cond); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } } } while (0)

// a DP plan for a frame w x h of the batch
static void check_dp(const DpPlan &dp, const PlanDevice &d, const PlanBatch &b, int w, int h, int delta)
{
    if (is_tile_p(dp.form)) {
        CHECK(dp.px >= 2 && dp.px <= 4 && dp.per >= 1 && dp.per <= b.images, "px %d per %d (w %d h %d delta %d images %d)", dp.px, dp.per, w, h, delta, b.images);
        if (dp.px < 2 || dp.px > 4) return;
        CHECK(dp.general == (dp.form == LQRHIP_CENSUS_TILE_P_GENERAL) && (!dp.general || dp.px == 2), "general %d px %d", (int) dp.general, dp.px);
        const int bound = dp.general ? d.wgs_general : dp.px == 3 ? std::min(d.wgs_plain, d.n_cu) : dp.px == 2 ? d.wgs_plain : d.wgs_px4;
        const long long grid = (long long) ((w + dpp_own(dp.px) - 1) / dpp_own(dp.px)) * dp.per;
        CHECK(grid <= bound, "grid %lld > %d (w %d px %d per %d)", grid, bound, w, dp.px, dp.per);
        const int rows = dp.px == 4 ? dpp_halo(4) : dpp_rb(dp.px, delta);
        CHECK((h + rows - 1) / rows < (1 << DPP_BLK_BITS), "h %d: blocks of %d rows pass the block field", h, rows);
        CHECK(b.spin && !b.shared, "a spinning grid without leave (w %d h %d)", w, h);
    } else if (dp.form == LQRHIP_CENSUS_SWEEP_FULL || dp.form == LQRHIP_CENSUS_SWEEP_UPDATE) {
        CHECK(dp.px == 1 || dp.px == 2 || dp.px == 4 || dp.px == 8 || dp.px == 16, "px %d (w %d)", dp.px, w);
        CHECK((long long) dp.px * dp.threads >= w && (dp.threads == 256 || dp.threads == DP_THREADS), "%d px x %d threads, w %d", dp.px, dp.threads, w);
        CHECK(dp.lds >= (size_t) 2 * w * sizeof(float), "lds %zu, w %d", dp.lds, w);
    } else CHECK(dp.form == LQRHIP_CENSUS_DP_TILE && delta == 1, "form %d (w %d h %d delta %d)", dp.form, w, h, delta);
}

// The widths of the sweep: every width up to 66, every 53rd, and two either side of every width at which a choice can change --
// multiples of 256 (k_dp_sweep's px per thread and thread count, the level kernel's 4096), 4200, and the widths at which n images'
// tiles of 32, 64 or 128 columns fill the 256 workgroups of a residency bound (all 16383 widths take 24 s under the sanitizers)
static bool g_width[LQRHIP_MAX_FRAME_WIDTH + 1];
static void mark(int t) { for (int w = std::max(t - 2, 2); w <= std::min(t + 2, LQRHIP_MAX_FRAME_WIDTH); w++) g_width[w] = true; }
static void choose_widths(void)
{
    for (int w = 2; w <= LQRHIP_MAX_FRAME_WIDTH; w++) g_width[w] = w <= 66 || w % 53 == 0;
    for (int t = 256; t <= LQRHIP_MAX_FRAME_WIDTH; t += 256) mark(t);
    mark(4200);
    for (int own : {32, 64, 128}) for (int n = 1; n <= 96; n++) mark(256 / n * own), mark(256 * own / n);
}

static int sweep(void)
{
    choose_widths();
    static const int heights[] = {2, 62, 999, 1000, 8160, 8161, 12285, 12286, 16320, 16384};
    static const int images[] = {1, 2, 3, 4, 8, 16, 48, 49, 64, 96}, shared_n[] = {1, 2, 4};
    const PlanKnobs k;
    const PlanDevice d = mi355x();
    long plans = 0;
    for (int spin = 0; spin <= 1; spin++)
    for (int n : images) for (int sn : shared_n) for (int delta = 0; delta <= 16; delta++) for (int h : heights) {
        PlanBatch b;
        b.images = n; b.shared_n = sn; b.shared = sn > 1; b.spin = spin != 0; b.wk_h = h;
        for (int w = 2; w <= LQRHIP_MAX_FRAME_WIDTH; w++) {
            if (!g_width[w]) continue;
            check_dp(plan_full_dp(k, d, b, w, delta, false), d, b, w, h, delta);
            const StepPlan s = plan_seam_step(k, d, b, delta, false, w, h, false, 0);
            plans += 2;
            if (w - 1 <= 1) { CHECK(s.dp.form < 0 && s.band < 0, "w %d: something to update", w); continue; }
            check_dp(s.dp, d, b, w - 1, h, delta);
            CHECK(s.band < 0 ? is_tile_p(s.dp.form) : s.dp.form == LQRHIP_CENSUS_SWEEP_UPDATE, "band %d with dp %d", s.band, s.dp.form);
            if (s.band == LQRHIP_CENSUS_BAND_LEVELS) {
                const int rows = lv_rows(delta, false);
                CHECK(s.levels_P >= 1 && s.levels_P <= LV_PMAX && (long long) s.levels_P * n * sn <= d.wgs_levels, "P %d, %d x %d images", s.levels_P, n, sn);
                CHECK((w - 1 + 63) / 64 <= LV_MAX_TILES && (h + rows - 1) / rows <= LV_MAX_LEVELS && b.spin, "levels at w %d h %d delta %d", w - 1, h, delta);
            } else CHECK(s.levels_P == 0, "P %d without the level kernel", s.levels_P);
        }
    }
    if (g_failures) { fprintf(stderr, "%ld checks failed\n", g_failures); return 1; }
    printf("sweep ok %ld plans\n", plans);
    return 0;
}

static int rules(void)
{
    const PlanKnobs k;
    const PlanDevice d = mi355x();
    for (int n = 1; n <= 8; n++) {          // the largest lag after which the frozen planes are NOT caught up
        PlanBatch b;
        b.images = n; b.wk_h = 100;
        int lag = 0;
        while (lag < 100000 && !plan_seam_step(k, d, b, 1, false, 100, 100, false, lag + 1).catchup) lag++;
        printf("lag %d %d\n", n, lag);
    }
    for (int delta = 0; delta <= LQRHIP_MAX_DELTA; delta++) printf("nt %d %d\n", delta, plan_seam_step(k, d, PlanBatch(), delta, false, 100, 100, false, 0).eu_nt);
    return 0;
}

int main(void)
{
    char mode[16];
    if (scanf("%15s", mode) != 1) return 2;
    return !strcmp(mode, "census") ? census() : !strcmp(mode, "sweep") ? sweep() : !strcmp(mode, "rules") ? rules() : 2;
}
