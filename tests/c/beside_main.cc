// beside_main.cc -- csrc/lqr_beside.h and csrc/lqr_plan.h alone, without a GPU (tests/test_backtrack_beside.py builds this with -Werror
// under AddressSanitizer and UndefinedBehaviorSanitizer): what the walk role of k_carve_v decides and hands over, and where the planner
// takes that launch.  The first argument names the check; each prints "ok ..." and returns 0, or says what failed and returns 1.
//   bound     every delta_x-connected path of every frame h <= 7, w <= 9, delta_x 1 and 2, and every prefix of its walk: a side the bound
//             decides is the side of the rule on the whole path; with no rows left it decides
//   overflow  the bound on 16384 x 16384 frames against the same sums in 128 bits (and under UBSan: no signed overflow in 64)
//   pack      entries pack and unpack: image < 1024, row-quad < 4096, origin < 16384, either role and side; tags are never 0 and alternate
//   count     h = 1 .. 300, radius 0 .. 3: a walk in chunks of BB_WALK_ROWS rows, published chunk by chunk, in batches, and with the side
//             decided late, pushes every row-quad and every energy block exactly once -- the consumer count -- and none before the rows
//             it reads are final
//   plan      reads the knob from stdin; prints one line per combination (see main) for the Python side to check against the rule
#include <stdio.h>
#include <string.h>
#include <vector>
#include "lqr_plan.h"
#include "lqr_hip.h"

static int fail(const char *what, long long a = 0, long long b = 0, long long c = 0, long long d = 0)
{
    printf("FAILED %s: %lld %lld %lld %lld\n", what, a, b, c, d);
    return 1;
}

static int check_bound(void)
{
    long long paths = 0, early = 0, prefixes = 0;
    for (int delta = 1; delta <= 2; delta++)
        for (int h = 1; h <= 7; h++)
            for (int w = 1; w <= 9; w++) {
                std::vector<int> x(h, 0);        // x[y], y = 0 the top row; the walk starts on row h - 1
                // odometer over the start column and the steps
                std::vector<int> step(h, -delta);
                for (int x0 = 0; x0 < w; x0++) {
                    std::fill(step.begin(), step.end(), -delta);
                    while (true) {
                        bool inside = true;
                        x[h - 1] = x0;
                        for (int y = h - 2; y >= 0 && inside; y--) { x[y] = x[y + 1] + step[y]; inside = x[y] >= 0 && x[y] < w; }
                        if (inside) {
                            paths++;
                            long long sum = 0;
                            for (int y = 0; y < h; y++) sum += x[y];
                            const int exact = 2 * sum < (long long) h * (w - 1) ? 1 : 0;
                            long long S = 0;
                            for (int y = h - 1; y >= 0; y--) {
                                S += x[y];
                                const int d = bb_side_bound(S, x[y], y, delta, w, h);
                                prefixes++;
                                if (d >= 0 && d != exact) return fail("bound decides the other side", delta, h, w, y);
                                if (y == 0 && d < 0) return fail("bound undecided with no rows left", delta, h, w, x0);
                                if (y > 0 && d >= 0) early++;
                            }
                        }
                        int i = 0;
                        while (i < h - 1 && step[i] == delta) step[i++] = -delta;
                        if (i >= h - 1) break;
                        step[i]++;
                    }
                }
            }
    if (early == 0) return fail("the bound never decides early");
    printf("ok bound: %lld paths, %lld prefixes, %lld decided before the end\n", paths, prefixes, early);
    return 0;
}

static int check_overflow(void)
{
    const int W = 16384, H = 16384;
    long long n = 0;
    for (int delta : {0, 1, 2, 10})
        for (int x : {0, 1, 8191, 8192, 16382, 16383})
            for (int r : {0, 1, 2, 4095, 8192, 16383}) {
                __int128 lo = 0, hi = 0;
                for (int k = 1; k <= r; k++) {
                    const long long a = (long long) x - (long long) delta * k, b = (long long) x + (long long) delta * k;
                    lo += a < 0 ? 0 : a;
                    hi += b > W - 1 ? W - 1 : b;
                }
                if ((__int128) bb_rem_min(x, r, delta) != lo) return fail("rem_min", delta, x, r);
                if ((__int128) bb_rem_max(x, r, delta, W) != hi) return fail("rem_max", delta, x, r);
                const long long rows = H - r;        // rows walked, each column 0 .. W - 1
                for (long long S : {0ll, (long long) x, rows * (W - 1) / 2, rows * (W - 1)}) {
                    const __int128 all = (__int128) H * (W - 1);
                    const int want = 2 * ((__int128) S + hi) < all ? 1 : 2 * ((__int128) S + lo) >= all ? 0 : -1;
                    if (bb_side_bound(S, x, r, delta, W, H) != want) return fail("side_bound", delta, x, r, S);
                    n++;
                }
            }
    printf("ok overflow: %lld cases\n", n);
    return 0;
}

static int check_pack(void)
{
    long long n = 0;
    const int idx[] = {0, 1, 2, 3, 7, 8, 61, 62, 63, 64, 255, 256, 1023, 1024, 2047, 2048, 4094, 4095};
    const int org[] = {0, 1, 2, 127, 128, 8191, 8192, 16382, 16383};
    const unsigned tags[] = {1u, 2u, 3u, 0x155555u, BB_EPOCHS - 1, BB_EPOCHS};
    for (int image = 0; image < BB_MAX_IMAGES; image++)
        for (int q : idx)
            for (int o : org)
                for (int side = 0; side <= 1; side++)
                    for (int energy = 0; energy <= 1; energy++)
                        for (unsigned tag : tags) {
                            const uint64_t e = bb_pack(tag, energy, image, q, side, o);
                            const BbEntry u = bb_unpack(e);
                            if (e == 0 || (unsigned) (e >> BB_TAG_SHIFT) != tag) return fail("tag", tag, image, q, o);
                            if (u.tag != tag || u.energy != energy || u.image != image || u.index != q || u.side != side || u.org != o) return fail("round trip", tag, image, q, o);
                            n++;
                        }
    if (BB_EPOCHS % 2 != 0) return fail("the tags' period is odd");
    for (unsigned l : {0u, 1u, 2u, BB_EPOCHS - 2, BB_EPOCHS - 1, BB_EPOCHS, BB_EPOCHS + 1, 0xfffffffeu}) {
        const unsigned a = bb_tag(l), b = bb_tag(l + 1);
        if (a == 0 || b == 0 || a > BB_EPOCHS || ((a ^ b) & 1) == 0) return fail("tags of consecutive launches", l, a, b);
    }
    if ((4096 + 3) / 4 > 4096 || bb_energy_entries(BB_MAX_ROWS) > 4096) return fail("an index does not fit its field");
    printf("ok pack: %lld entries\n", n);
    return 0;
}

// one walk of a frame h high: `every` = chunks per publishing pass, `decide_at` = the side is known once lo <= decide_at
static int walk_counts(int h, int radius, int every, int decide_at)
{
    const int rblk = bb_carve_entries(h), eblk = bb_energy_entries(h);
    std::vector<int> quad(rblk, 0), blk(eblk, 0);
    int next_q = rblk - 1, next_e = eblk - 1, chunk = 0;
    long long pushed = 0;
    auto publish = [&](int lo) -> int {
        if (lo > decide_at && lo > 0) return 0;
        const int e0 = bb_first_eblk(lo, radius), q0 = bb_first_quad(lo, radius);
        for (int e = next_e; e >= e0; e--) {
            // rows emap_update_block reads for block e: its rows and two halo rows, their neighbours, `radius` beyond
            const int first = e * BB_EU_ROWS - 2 - radius;
            if (std::max(first, 0) < lo) return fail("energy block pushed early", h, e, lo, radius);
            blk[e]++; pushed++;
        }
        for (int q = next_q; q >= q0; q--) {
            const int first = 4 * q - 1 - radius;
            if (std::max(first, 0) < lo) return fail("row-quad pushed early", h, q, lo, radius);
            quad[q]++; pushed++;
        }
        next_e = std::min(next_e, e0 - 1); next_q = std::min(next_q, q0 - 1);
        return 0;
    };
    for (int y_top = h - 1; y_top >= 1;) {
        const int nrows = std::min(BB_WALK_ROWS, y_top);
        const int lo = y_top - nrows + 1;
        y_top -= nrows;
        if (++chunk % every == 0 && publish(lo)) return 1;
    }
    if (publish(0)) return 1;
    for (int c : quad) if (c != 1) return fail("a row-quad not pushed exactly once", h, radius, every, decide_at);
    for (int c : blk) if (c != 1) return fail("an energy block not pushed exactly once", h, radius, every, decide_at);
    // the consumer workgroups of the launch, as the shim counts them for one image
    if (pushed != (h + 3) / 4 + (h + 61) / 62 || pushed != bb_entries(1, h)) return fail("entry count", h, pushed);
    return 0;
}
static int check_count(void)
{
    long long n = 0;
    for (int h = 1; h <= 300; h++)
        for (int radius = 0; radius <= 3; radius++)
            for (int every : {1, 2, 5, 1000})
                for (int decide_at : {h, h / 2, 13, 0}) {
                    if (walk_counts(h, radius, every, decide_at)) return 1;
                    n++;
                }
    if (bb_entries(64, 2160) != 64ll * (540 + 35)) return fail("entries of 64 x 2160 rows");
    printf("ok count: %lld walks\n", n);
    return 0;
}

// images shared_n delta value w h spin lag | backtrack carve energy_beside catchup backtrack_beside
static int print_plans(void)
{
    PlanKnobs k;
    PlanDevice d;
    d.wgs_plain = d.wgs_general = d.wgs_px4 = d.wgs_levels = d.n_cu = 256;
    d.hw_queues = 4;
    printf("min %d default %d vpath1 %d rows %d %d images %d\n", BACKTRACK_BESIDE_MIN, k.backtrack_beside, LQRHIP_CENSUS_VPATH1, BB_MIN_ROWS, BB_MAX_ROWS, BB_MAX_IMAGES);
    if (scanf("%d", &k.backtrack_beside) != 1) return 2;
    for (int n : {1, 3, 4, 5, 7, 8, 9, 16, 64, 96, 1024, 1028})
        for (int sn : {1, 2, 4}) {
            if (n % sn) continue;
            for (int delta = 0; delta <= 4; delta++)
                for (int value = 0; value <= 1; value++)
                    for (int w : {2, 3, 100})
                        for (int h : {1, 2, 36, 37, 38, 1000, 2160, 4096, 4097})
                            for (int spin = 0; spin <= 1; spin++)
                                for (int lag : {0, 200}) {
                                    PlanBatch b;
                                    b.images = n / sn; b.shared_n = sn; b.shared = sn > 1; b.wk_h = h; b.value = value != 0; b.spin = spin != 0;
                                    const StepPlan s = plan_seam_step(k, d, b, delta, false, w, h, false, lag);
                                    printf("%d %d %d %d %d %d %d %d %d %d %d %d %d\n", n, sn, delta, value, w, h, spin, lag, s.backtrack, s.carve, (int) s.energy_beside,
                                           (int) s.catchup, (int) s.backtrack_beside);
                                }
        }
    return 0;
}

int main(int argc, char **argv)
{
    const char *what = argc > 1 ? argv[1] : "";
    if (!strcmp(what, "bound")) return check_bound();
    if (!strcmp(what, "overflow")) return check_overflow();
    if (!strcmp(what, "pack")) return check_pack();
    if (!strcmp(what, "count")) return check_count();
    if (!strcmp(what, "plan")) return print_plans();
    return 2;
}
