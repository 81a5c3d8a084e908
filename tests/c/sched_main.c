/* Stand-alone exercise of host/lqr_sched.c (tests/test_sched.py builds it with -fsanitize=address,undefined).
 *
 *   sched_main sweep   the schedule against the walks host/lqr_carver.c held before it read them from lqr_sched.h: frame_refused,
 *                      inactive_refused and the arithmetic of group_resize_dir / group_build_maps / group_build_vsmap, kept below
 *                      verbatim over a plain struct with the device calls removed.  Exhaustive over small geometries, plus the edge
 *                      of the frame limit.  Prints "sched sweep ok <cases>".
 *   sched_main plan    reads "new W H", "cfg ENL_STEP SWITCH_FREQ UPDATE_STEP ORDER" and "resize W1 H1" lines and prints what the
 *                      schedule says a carver does: the refusal, per direction the steps, sessions, seams and progress reports, and
 *                      the geometry afterwards.  tests/test_sched.py compares that with tests/geometry_cases.py and with the oracle.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lqr_hip.h"        /* LQRHIP_MAX_FRAME_WIDTH */
#include "lqr_sched.h"

#define MAXI(a, b) ((a) > (b) ? (a) : (b))
#define MINI(a, b) ((a) < (b) ? (a) : (b))

/* ======================= the reference: what lqr_carver.c held ============ */
typedef struct {
    int w_start, h_start, w, h, w0, h0;
    int level, max_level;
    int transposed, active;
    float enl_step;
} Ref;

static int ref_frame_refused(const Ref *r, int w1, int want_transposed)
{
    const int same = (r->transposed == want_transposed);
    int ws = same ? r->w_start : r->h_start, wc = same ? r->w : r->h, delta_max;
    if (w1 == wc) return 0;                             /* nothing to carve in this direction */
    if (ws > LQRHIP_MAX_FRAME_WIDTH || wc > LQRHIP_MAX_FRAME_WIDTH) return 1;
    for (;;) {
        int new_w;
        delta_max = (int) ((r->enl_step - 1) * ws) - 1;
        if (delta_max < 1) delta_max = 1;
        new_w = MINI(w1, ws + delta_max);
        if (new_w >= w1) return 0;
        ws = new_w;                                     /* flattened: the next session starts from here */
        if (ws > LQRHIP_MAX_FRAME_WIDTH) return 1;
    }
}

static int ref_inactive_refused(const Ref *r, int w1, int want_transposed)
{
    const int same = (r->transposed == want_transposed);
    int delta, delta_max;
    if (r->active) return 0;
    if (w1 == (same ? r->w : r->h)) return 0;           /* nothing to do in this direction */
    if (!same) return 1;
    delta = w1 - r->w_start;
    if (delta < 0) return -delta + 1 > r->max_level;
    delta_max = (int) ((r->enl_step - 1) * r->w_start) - 1;
    if (delta_max < 1) delta_max = 1;
    return delta > delta_max || delta + 1 > r->max_level;
}

static void ref_set_width(Ref *r, int w1)
{
    r->w = w1;
    r->level = r->w0 - w1 + 1;
}

/* group_flatten's bookkeeping (where the carver is its own flattening and the call returns early, these are no change) */
static void ref_flatten(Ref *r)
{
    r->w0 = r->w; r->h0 = r->h;
    r->w_start = r->w; r->h_start = r->h;
    r->level = 1; r->max_level = 1;
}

static void ref_transpose(Ref *r)
{
    int d;
    if (r->level > 1 || r->max_level > 1 || r->w0 != r->w) ref_flatten(r);
    d = r->w0; r->w0 = r->h0; r->h0 = d;
    r->w = r->w0; r->h = r->h0;
    r->w_start = r->w0; r->h_start = r->h0;
    r->level = 1; r->max_level = 1;
    r->transposed = r->transposed ? 0 : 1;
}

/* group_build_maps / session_run / group_build_vsmap; returns the frame the session started from, 0 without a session */
static int ref_build_maps(Ref *r, int depth)
{
    int l, w1, frame;
    if (depth <= r->max_level) return 0;
    ref_set_width(r, r->w_start - r->max_level + 1);    /* the carved frame */
    frame = r->w;
    if (depth == 0) depth = r->w_start + 1;
    for (l = r->max_level; l < depth; l++) { r->level++; r->w--; }
    w1 = r->w0 + (depth - 1) - r->max_level + 1;
    r->level = depth; r->max_level = depth;
    r->w0 = w1;
    ref_set_width(r, r->w_start);
    return frame;
}

#define MAX_STEPS 256
typedef struct { int transpose, depth, frame, new_w, gamma, flatten; } RefStep;

/* group_resize_dir; returns the number of steps, -1 past MAX_STEPS */
static int ref_resize_dir(Ref *r, int w1, int want_transposed, RefStep *out, int *total)
{
    int delta, gamma, delta_max, n = 0;
    if (r->transposed == want_transposed) {
        delta = w1 - r->w_start; gamma = w1 - r->w;
        delta_max = (int) ((r->enl_step - 1) * r->w_start) - 1;
    } else {
        delta = w1 - r->h_start; gamma = w1 - r->h;
        delta_max = (int) ((r->enl_step - 1) * r->h_start) - 1;
    }
    if (delta_max < 1) delta_max = 1;
    if (delta < 0) { delta = -delta; delta_max = delta; }
    *total = gamma > 0 ? gamma : -gamma;

    while (gamma) {
        int delta0 = MINI(delta, delta_max), new_w;
        RefStep *s;
        if (n == MAX_STEPS) return -1;
        s = &out[n++];
        delta -= delta0;
        s->transpose = (r->transposed != want_transposed);
        if (r->transposed != want_transposed) ref_transpose(r);
        new_w = MINI(w1, r->w_start + delta_max);
        gamma = w1 - new_w;
        s->depth = delta0 + 1;
        s->frame = ref_build_maps(r, delta0 + 1);
        ref_set_width(r, new_w);
        s->new_w = new_w; s->gamma = gamma;
        s->flatten = (new_w < w1);
        if (new_w < w1) {
            ref_flatten(r);
            delta_max = (int) ((r->enl_step - 1) * r->w_start) - 1;
            if (delta_max < 1) delta_max = 1;
        }
    }
    return n;
}

/* ======================= sweep =========================================== */
static long g_cases = 0;

static void geom_of(const Ref *r, LqrGeom *g)
{
    g->w_start = r->w_start; g->h_start = r->h_start; g->w = r->w; g->h = r->h; g->w0 = r->w0; g->h0 = r->h0;
    g->level = r->level; g->max_level = r->max_level; g->transposed = r->transposed;
}

static int same_geom(const Ref *r, const LqrGeom *g)
{
    return g->w_start == r->w_start && g->h_start == r->h_start && g->w == r->w && g->h == r->h && g->w0 == r->w0 && g->h0 == r->h0 &&
           g->level == r->level && g->max_level == r->max_level && g->transposed == r->transposed;
}

#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } while (0)
#define WHERE "w_start %d h_start %d max_level %d w %d transposed %d enl_step %g w1 %d want %d"
#define WHERE_ARGS r0->w_start, r0->h_start, r0->max_level, r0->w, r0->transposed, (double) r0->enl_step, w1, want

/* one input: both predicates (active and not), every step, the total and the geometry afterwards */
static void check_one(const Ref *r0, int w1, int want)
{
    static RefStep ref[MAX_STEPS];
    Ref r = *r0, ra = *r0;
    LqrGeom g;
    LqrWalk k;
    LqrWalkStep s;
    int n, i = 0, total;
    geom_of(r0, &g);
    g_cases++;
    if (lqr_walk_frame_refused(&g, r0->enl_step, w1, want, LQRHIP_MAX_FRAME_WIDTH) != ref_frame_refused(r0, w1, want))
        FAIL("frame_refused differs: " WHERE, WHERE_ARGS);
    ra.active = 0;
    if (lqr_walk_needs_maps(&g, r0->enl_step, w1, want) != ref_inactive_refused(&ra, w1, want)) FAIL("inactive_refused differs: " WHERE, WHERE_ARGS);
    ra.active = 1;
    if (ref_inactive_refused(&ra, w1, want)) FAIL("an active carver refused: " WHERE, WHERE_ARGS);
    n = ref_resize_dir(&r, w1, want, ref, &total);
    if (n < 0) FAIL("more than %d steps: " WHERE, MAX_STEPS, WHERE_ARGS);
    lqr_walk_begin(&k, &g, r0->enl_step, w1, want);
    if (k.total != total) FAIL("total %d, reference %d: " WHERE, k.total, total, WHERE_ARGS);
    while (lqr_walk_next(&k, &s)) {
        if (i >= n) FAIL("more steps than the reference's %d: " WHERE, n, WHERE_ARGS);
        if (s.transpose != ref[i].transpose || s.depth != ref[i].depth || s.frame != ref[i].frame || s.new_w != ref[i].new_w ||
            s.gamma != ref[i].gamma || s.flatten != ref[i].flatten)
            FAIL("step %d: transpose %d depth %d frame %d new_w %d gamma %d flatten %d, reference %d %d %d %d %d %d: " WHERE, i, s.transpose,
                 s.depth, s.frame, s.new_w, s.gamma, s.flatten, ref[i].transpose, ref[i].depth, ref[i].frame, ref[i].new_w, ref[i].gamma,
                 ref[i].flatten, WHERE_ARGS);
        i++;
    }
    if (i != n) FAIL("%d steps, reference %d: " WHERE, i, n, WHERE_ARGS);
    if (!same_geom(&r, &k.g)) FAIL("the geometry after the walk differs: " WHERE, WHERE_ARGS);
}

/* a carver of w_start x h_start with max_level - 1 seams in its map, showing w columns */
static void ref_make(Ref *r, int w_start, int h_start, int max_level, int w, int transposed, float enl_step)
{
    r->w_start = w_start; r->h_start = r->h = r->h0 = h_start;
    r->max_level = max_level;
    r->w0 = w_start + max_level - 1;
    r->transposed = transposed; r->active = 1; r->enl_step = enl_step;
    ref_set_width(r, w);
}

static const float k_enl[5] = {1.01f, 1.1f, 1.3f, 1.5f, 2.0f};

static int thin(int v, int lo, int hi)      /* the ends, their neighbours and every fifth value between */
{
    return v - lo < 3 || hi - v < 3 || v % 5 == 0;
}

/* The grid is thinned where a value cannot matter.  Along the carver's direction the rows are only carried along: one h_start, and
 * every max_level and visible width up to w_start 12, thinned above.  Across it the carver is flattened and transposed first, so that
 * h_start becomes the frame and the levels only decide whether a flatten comes first: h_start thinned, three levels, three widths. */
static void sweep_small(void)
{
    int w_start, h_start, max_level, w, t, e, w1;
    Ref r;
    for (w_start = 1; w_start <= 48; w_start++)
        for (max_level = 1; max_level <= w_start; max_level++) {
            const int lo = w_start - max_level + 1, hi = w_start + max_level - 1;
            const int ends_l = (max_level <= 2 || max_level == w_start);
            if (w_start > 12 && !thin(max_level, 1, w_start)) continue;
            for (w = lo; w <= hi; w++) {
                const int ends_w = (w == lo || w == hi || w == w_start);
                if (w_start > 12 && !thin(w, lo, hi) && w != w_start) continue;
                for (t = 0; t < 2; t++)
                    for (e = 0; e < 5; e++) {
                        ref_make(&r, w_start, 7, max_level, w, t, k_enl[e]);
                        for (w1 = 1; w1 <= 120; w1++) check_one(&r, w1, t);
                        if (!ends_l || !ends_w) continue;
                        for (h_start = 1; h_start <= 48; h_start++) {
                            if (!thin(h_start, 1, 48)) continue;
                            ref_make(&r, w_start, h_start, max_level, w, t, k_enl[e]);
                            for (w1 = 1; w1 <= 120; w1++) check_one(&r, w1, !t);
                        }
                    }
            }
        }
}

static void sweep_limit(void)
{
    int ws, w1, t, want, e, hidden;
    Ref r;
    for (ws = 16380; ws <= 16390; ws++)
        for (hidden = 0; hidden < 3; hidden++)
            for (t = 0; t < 2; t++)
                for (e = 0; e < 5; e++)
                    for (want = 0; want < 2; want++)
                        for (w1 = 16380; w1 <= 16390; w1++) {
                            ref_make(&r, ws, 6, 1 + hidden, ws - hidden, t, k_enl[e]);
                            if (want == t) check_one(&r, w1, want);
                            ref_make(&r, 6, ws, 1, 6, t, k_enl[e]);             /* the long side lies across */
                            if (want != t) check_one(&r, w1, want);
                        }
    /* the stepwise enlargements of tests/geometry_cases.py */
    ref_make(&r, 11000, 6, 1, 11000, 0, 1.5f);
    check_one(&r, 16499, 0);
    if (ref_frame_refused(&r, 16499, 0)) FAIL("11000 -> 16499 refused");
    check_one(&r, 16500, 0);
    if (!ref_frame_refused(&r, 16500, 0)) FAIL("11000 -> 16500 not refused");
    ref_make(&r, 10922, 6, 1, 10922, 0, 1.5f);
    check_one(&r, 16382, 0);
    check_one(&r, 16390, 0);
    if (ref_frame_refused(&r, 16390, 0)) FAIL("10922 -> 16390 refused");
}

/* a session's numbers against both spellings lqr_carver.c had (the seam loop's, the roll-back's), and its seams against the loop */
static void sweep_sessions(void)
{
    static const int k_freq[4] = {0, 1, 2, 5};
    int max_level, w_start, depth, f, cur, ustep;
    for (w_start = 1; w_start <= 40; w_start++)
        for (max_level = 1; max_level <= w_start; max_level++)
            for (depth = max_level + 1; depth <= w_start + 1; depth++)
                for (f = 0; f < 4; f++)
                    for (cur = 0; cur < 3; cur++)
                        for (ustep = 1; ustep <= 3; ustep++) {
                            const int freq = k_freq[f], total = depth - max_level + cur + 1, wc0 = w_start - max_level + 1;
                            int l, w = wc0, finish = 0, lr_switch_interval = 0;
                            LqrSession s;
                            lqr_session_begin(&s, max_level, depth, wc0, freq, cur, total, ustep);
                            g_cases++;
                            if (freq) lr_switch_interval = (depth - max_level - 1) / freq + 1;
                            for (l = max_level; l < depth; l++) {
                                int full = 0, w_before = w;
                                const int report = ((l - max_level + cur) % ustep == 0);
                                LqrSeam q;
                                if (w_before - 1 > 1) {
                                    if (freq && ((l - max_level + lr_switch_interval / 2) % lr_switch_interval) == 0) full = 1;
                                } else {
                                    finish = 1;
                                }
                                lqr_session_seam(&s, l, &q);
                                if (q.w_before != w_before || q.full != full || q.report != report ||
                                    (report && q.fraction != (double) (l - max_level + cur) / (double) total))
                                    FAIL("seam %d of a session max_level %d depth %d w_start %d freq %d", l, max_level, depth, w_start, freq);
                                w--;
                            }
                            if (s.n_seams != depth - max_level || s.wc0 != wc0 || s.first_level != 2 * max_level - 1 || s.finish != finish ||
                                s.finish != (wc0 - (depth - max_level) <= 1) || s.lr_switch_interval != lr_switch_interval)
                                FAIL("session max_level %d depth %d w_start %d freq %d", max_level, depth, w_start, freq);
                        }
}

/* the two float products, against the expressions lqr_carver.c had and at values where float and double part ways */
static void sweep_floats(void)
{
    static const float k_us[4] = {0.02f, 0.1f, 0.005f, 0.3f};
    int n, e;
    for (n = 0; n <= 20000; n++)
        for (e = 0; e < 5; e++) {
            int delta_max = (int) ((k_enl[e] - 1) * n) - 1;
            if (delta_max < 1) delta_max = 1;
            if (lqr_sched_delta_max(k_enl[e], n) != delta_max) FAIL("delta_max of %d at %g", n, (double) k_enl[e]);
            if (e < 4 && lqr_sched_update_step(n, k_us[e]) != (int) MAXI(n * k_us[e], 1)) FAIL("update step of %d at %g", n, (double) k_us[e]);
            g_cases++;
        }
    if (lqr_sched_update_step(200, 0.02f) != 4) FAIL("200 * 0.02f rounds to 4 in float (3.9999999 in double): 4 seams between reports");
    if (lqr_sched_delta_max(1.5f, 11000) != 5499 || lqr_sched_delta_max(1.5f, 10922) != 5460 || lqr_sched_delta_max(2.0f, 1) != 1)
        FAIL("delta_max of the stepwise cases");
}

/* ======================= plan ============================================ */
static void plan_dir(LqrGeom *g, float enl_step, int switch_freq, float update_step, int w1, int want)
{
    const char t = want ? 'h' : 'w';
    LqrWalk k;
    LqrWalkStep s;
    int current = 0, ustep;
    lqr_walk_begin(&k, g, enl_step, w1, want);
    ustep = lqr_sched_update_step(k.total, update_step);
    if (k.total) printf("init %c\n", t);
    for (;;) {
        const LqrGeom before = k.g;
        if (!lqr_walk_next(&k, &s)) break;
        printf("step %d %d %d %d %d %d\n", s.transpose, s.depth, s.frame, s.new_w, s.gamma, s.flatten);
        if (s.frame) {
            const int max_level = s.transpose ? 1 : before.max_level;       /* as the session finds it: after the transposition */
            const int rows = k.g.h;                                         /* (which alone changes the rows) */
            LqrSession q;
            int l;
            lqr_session_begin(&q, max_level, s.depth, s.frame, switch_freq, current, k.total, ustep);
            printf("session %d %d %d %d %d\n", q.wc0, rows, q.n_seams, q.finish, q.first_level);
            for (l = q.max_level; l < q.depth; l++) {
                LqrSeam m;
                lqr_session_seam(&q, l, &m);
                if (m.report) printf("update %.17g\n", m.fraction);
                printf("seam %d %d\n", m.w_before, m.full);
            }
        }
        current = k.total - (s.gamma > 0 ? s.gamma : -s.gamma);
        /* the depth of the map a dump after the step holds, before a flatten drops it */
        printf("map %d\n", s.frame ? s.depth - 1 : s.transpose ? 0 : before.w0 - before.w_start);
    }
    if (k.total) printf("end %c\n", t);
    *g = k.g;
}

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "sweep")) {
        sweep_small();
        sweep_limit();
        sweep_sessions();
        sweep_floats();
        printf("sched sweep ok %ld\n", g_cases);
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "plan")) {
        char line[256];
        LqrGeom g;
        float enl_step = 2.0f, update_step = 0.02f;
        int switch_freq = 0, order = 0, a, b;
        lqr_geom_reset(&g, 1, 1);
        while (fgets(line, sizeof line, stdin)) {
            if (sscanf(line, "new %d %d", &a, &b) == 2) lqr_geom_reset(&g, a, b);
            else if (sscanf(line, "cfg %f %d %f %d", &enl_step, &switch_freq, &update_step, &order) == 4) continue;
            else if (sscanf(line, "resize %d %d", &a, &b) == 2) {
                const int refused = lqr_walk_frame_refused(&g, enl_step, a, 0, LQRHIP_MAX_FRAME_WIDTH) ||
                                    lqr_walk_frame_refused(&g, enl_step, b, 1, LQRHIP_MAX_FRAME_WIDTH);
                printf("resize %d %d refused %d\n", a, b, refused);        /* (planned all the same: what the refusal keeps off the device) */
                plan_dir(&g, enl_step, switch_freq, update_step, order ? b : a, order ? 1 : 0);
                plan_dir(&g, enl_step, switch_freq, update_step, order ? a : b, order ? 0 : 1);
                printf("geom %d %d %d %d %d %d %d %d\n", g.transposed ? g.h : g.w, g.transposed ? g.w : g.h, g.transposed ? g.h_start : g.w_start,
                       g.transposed ? g.w_start : g.h_start, g.transposed, g.w0 - g.w_start, g.w, g.h);
            } else
                FAIL("bad line: %s", line);
        }
        return 0;
    }
    fprintf(stderr, "usage: sched_main sweep | plan\n");
    return 2;
}
