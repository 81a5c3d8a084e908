/* lqr_sched.c -- see lqr_sched.h */
#include "lqr_sched.h"

#define MINI(a, b) ((a) < (b) ? (a) : (b))
#define MAXI(a, b) ((a) > (b) ? (a) : (b))

/* ======================= geometry ======================================== */
void lqr_geom_reset(LqrGeom *g, int img_w, int img_h)
{
    g->level = g->max_level = 1;
    g->w = g->w0 = g->w_start = img_w;
    g->h = g->h0 = g->h_start = img_h;
    g->transposed = 0;
}

void lqr_geom_set_width(LqrGeom *g, int w1)
{
    g->w = w1;
    g->level = g->w0 - w1 + 1;
}

void lqr_geom_flattened(LqrGeom *g)
{
    g->w0 = g->w; g->h0 = g->h;
    g->w_start = g->w; g->h_start = g->h;
    g->level = 1; g->max_level = 1;
}

void lqr_geom_transposed(LqrGeom *g)
{
    const int d = g->w0;
    g->w0 = g->h0; g->h0 = d;
    g->w = g->w0; g->h = g->h0;
    g->w_start = g->w0; g->h_start = g->h0;
    g->level = 1; g->max_level = 1;
    g->transposed = g->transposed ? 0 : 1;
}

void lqr_geom_session_done(LqrGeom *g, int depth, int n_seams)
{
    g->w0 += n_seams;                           /* every seam of the session is doubled in the base layout */
    g->level = depth; g->max_level = depth;
    lqr_geom_set_width(g, g->w_start);
}

void lqr_geom_map_loaded(LqrGeom *g, int depth)
{
    g->max_level = g->level = depth + 1;
    g->w0 = g->w_start + depth;
    lqr_geom_set_width(g, g->w_start);
}

int lqr_geom_needs_flatten(const LqrGeom *g)
{
    return g->w != g->w0 || g->w_start != g->w0 || g->h != g->h0 || g->h_start != g->h0;
}

/* nothing hidden, nothing inserted */
int lqr_geom_is_flat(const LqrGeom *g)
{
    return g->w == g->w0 && g->level == 1 && g->max_level == 1 && g->w_start == g->w0;
}

int lqr_geom_flatten_before_transpose(const LqrGeom *g)
{
    return g->level > 1 || g->max_level > 1 || g->w0 != g->w;
}

int lqr_sched_delta_max(float enl_step, int w_start)
{
    const int delta_max = (int) ((enl_step - 1) * w_start) - 1;
    return delta_max < 1 ? 1 : delta_max;
}

int lqr_sched_update_step(int total, float update_step)
{
    return (int) MAXI(total * update_step, 1);
}

/* ======================= one direction of a resize ======================= */
void lqr_walk_begin(LqrWalk *k, const LqrGeom *g, float enl_step, int w1, int want_transposed)
{
    const int same = (g->transposed == want_transposed);
    k->g = *g;
    k->enl_step = enl_step;
    k->w1 = w1; k->want_transposed = want_transposed;
    k->delta = w1 - (same ? g->w_start : g->h_start);
    k->gamma = w1 - (same ? g->w : g->h);
    k->delta_max = lqr_sched_delta_max(enl_step, same ? g->w_start : g->h_start);
    if (k->delta < 0) { k->delta = -k->delta; k->delta_max = k->delta; }
    k->total = k->gamma > 0 ? k->gamma : -k->gamma;
}

int lqr_walk_next(LqrWalk *k, LqrWalkStep *s)
{
    LqrGeom *g = &k->g;
    const int delta0 = MINI(k->delta, k->delta_max);
    if (!k->gamma) return 0;
    k->delta -= delta0;
    s->transpose = (g->transposed != k->want_transposed);
    if (s->transpose) {
        if (lqr_geom_flatten_before_transpose(g)) lqr_geom_flattened(g);
        lqr_geom_transposed(g);
    }
    s->new_w = MINI(k->w1, g->w_start + k->delta_max);
    s->gamma = k->gamma = k->w1 - s->new_w;
    s->depth = delta0 + 1;
    s->frame = 0;
    if (s->depth > g->max_level) {
        s->frame = g->w_start - g->max_level + 1;
        lqr_geom_session_done(g, s->depth, s->depth - g->max_level);
    }
    lqr_geom_set_width(g, s->new_w);
    s->flatten = (s->new_w < k->w1);
    if (s->flatten) {
        lqr_geom_flattened(g);
        k->delta_max = lqr_sched_delta_max(k->enl_step, g->w_start);
    }
    return 1;
}

int lqr_walk_frame_refused(const LqrGeom *g, float enl_step, int w1, int want_transposed, int max_frame)
{
    const int same = (g->transposed == want_transposed);
    LqrWalk k;
    LqrWalkStep s;
    if (w1 == (same ? g->w : g->h)) return 0;           /* nothing to carve in this direction */
    if ((same ? g->w_start : g->h_start) > max_frame || (same ? g->w : g->h) > max_frame) return 1;
    lqr_walk_begin(&k, g, enl_step, w1, want_transposed);
    while (lqr_walk_next(&k, &s))
        if (s.frame > max_frame) return 1;
    return 0;
}

int lqr_walk_needs_maps(const LqrGeom *g, float enl_step, int w1, int want_transposed)
{
    LqrWalk k;
    LqrWalkStep s;
    int steps = 0;
    lqr_walk_begin(&k, g, enl_step, w1, want_transposed);
    while (lqr_walk_next(&k, &s))
        if (s.transpose || s.frame || ++steps > 1) return 1;
    return 0;
}

void lqr_geom_size_range(const LqrGeom *g, float enl_step, int *lo, int *hi)
{
    *lo = g->w_start - (g->max_level - 1);
    *hi = g->w_start + MINI(g->max_level - 1, lqr_sched_delta_max(enl_step, g->w_start));
}

/* ======================= one session ===================================== */
void lqr_session_begin(LqrSession *s, int max_level, int depth, int wc0, int lr_switch_frequency, int rescale_current, int rescale_total,
                       int update_step)
{
    if (depth == 0) depth = wc0 + max_level;            /* = w_start + 1 */
    s->max_level = max_level; s->depth = depth;
    s->n_seams = depth - max_level;
    s->wc0 = wc0;
    s->first_level = 2 * max_level - 1;
    s->finish = (wc0 - s->n_seams <= 1);                /* the last seam leaves at most one column */
    s->lr_switch_frequency = lr_switch_frequency;
    /* "frequency" = number of side switches per rescale operation */
    s->lr_switch_interval = lr_switch_frequency ? (depth - max_level - 1) / lr_switch_frequency + 1 : 0;
    s->rescale_current = rescale_current; s->rescale_total = rescale_total; s->update_step = update_step;
}

void lqr_session_seam(const LqrSession *s, int l, LqrSeam *out)
{
    const int i = l - s->max_level, done = i + s->rescale_current;
    out->w_before = s->wc0 - i;
    out->report = (done % s->update_step == 0);
    out->fraction = (double) done / (double) s->rescale_total;
    out->full = out->w_before - 1 > 1 && s->lr_switch_frequency && ((i + s->lr_switch_interval / 2) % s->lr_switch_interval) == 0;
}
