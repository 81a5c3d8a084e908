/* sizes_range_main.c -- lqr_geom_size_range (host/lqr_sched.c) against the walk it is the closed form of, without a GPU.
 * For every geometry -- w_start 2 .. 70, every max_level, both orientations, five enlargement steps, the current width at both ends
 * of the range, at w_start and in between -- the sizes lqr_walk_needs_maps lets pass are collected by brute force over every size
 * from 1 to 3 w_start + 8.  They must be an interval, hold the current width and equal [lo, hi] of the closed form.
 * Second sweep: the one geometry where the two differ.  A carver enlarged under a large step whose step is then lowered shows a width
 * above the new hi; the walk lets that width pass because there is nothing to do.  Without it the set is [lo, hi] again.
 * Compiled with lqr_sched.c alone by tests/test_sizes_range.py (AddressSanitizer, UndefinedBehaviorSanitizer). */
#include <stdio.h>
#include "lqr_sched.h"

static const float k_steps[5] = {1.01f, 1.1f, 1.5f, 2.0f, 3.0f};

static void geom(LqrGeom *g, int ws, int ml, int transposed, int cur)
{
    g->w_start = ws; g->h_start = 7;
    g->max_level = ml;
    g->w0 = ws + ml - 1; g->h0 = 7;
    g->h = 7;
    g->transposed = transposed;
    lqr_geom_set_width(g, cur);
}

/* the set the walk lets pass, as first, last, count; `skip`: a size left out (0: none) */
static void brute(const LqrGeom *g, float enl, int skip, int *first, int *last, int *count)
{
    int w1;
    *first = 0; *last = 0; *count = 0;
    for (w1 = 1; w1 <= 3 * g->w_start + 8; w1++) {
        if (w1 == skip || lqr_walk_needs_maps(g, enl, w1, g->transposed)) continue;
        if (!*count) *first = w1;
        *last = w1;
        ++*count;
    }
}

int main(void)
{
    long checked = 0, lowered = 0;
    int ws, ml, t, e, i;
    for (ws = 2; ws <= 70; ws++)
        for (ml = 1; ml <= ws; ml++)
            for (t = 0; t < 2; t++)
                for (e = 0; e < 5; e++) {
                    LqrGeom g;
                    int lo, hi, cur[5];
                    geom(&g, ws, ml, t, ws);
                    lqr_geom_size_range(&g, k_steps[e], &lo, &hi);
                    if (lo < 1 || lo > ws || hi < ws) { printf("range [%d, %d] of w_start %d max_level %d step %g\n", lo, hi, ws, ml, k_steps[e]); return 1; }
                    if (ml == 1 && lo != hi) { printf("a flat carver of %d has the range [%d, %d]\n", ws, lo, hi); return 1; }
                    cur[0] = lo; cur[1] = hi; cur[2] = ws; cur[3] = (lo + ws) / 2; cur[4] = (ws + hi + 1) / 2;
                    for (i = 0; i < 5; i++) {
                        int first, last, count, lo2, hi2;
                        geom(&g, ws, ml, t, cur[i]);
                        lqr_geom_size_range(&g, k_steps[e], &lo2, &hi2);
                        brute(&g, k_steps[e], 0, &first, &last, &count);
                        if (lo2 != lo || hi2 != hi || first != lo || last != hi || count != hi - lo + 1 || cur[i] < first || cur[i] > last) {
                            printf("w_start %d max_level %d transposed %d step %g width %d: closed form [%d, %d], the walk passes %d sizes from %d to %d\n", ws,
                                   ml, t, k_steps[e], cur[i], lo2, hi2, count, first, last);
                            return 1;
                        }
                        checked++;
                    }
                    /* enlarged to the top of the range under step 2.0, then the step is lowered */
                    if (k_steps[e] < 2.0f) {
                        int lo2, hi2, first, last, count;
                        geom(&g, ws, ml, t, ws);
                        lqr_geom_size_range(&g, 2.0f, &lo2, &hi2);
                        if (hi2 > hi) {
                            geom(&g, ws, ml, t, hi2);
                            brute(&g, k_steps[e], hi2, &first, &last, &count);
                            if (lqr_walk_needs_maps(&g, k_steps[e], hi2, t) || first != lo || last != hi || count != hi - lo + 1) {
                                printf("lowered step: w_start %d max_level %d step %g width %d: [%d, %d] against %d sizes from %d to %d\n", ws, ml, k_steps[e],
                                       hi2, lo, hi, count, first, last);
                                return 1;
                            }
                            lowered++;
                        }
                    }
                }
    printf("sizes range ok %ld %ld\n", checked, lowered);
    return 0;
}
