/*
 * lqr_sched.h -- the host's resize schedule (liblqr's bookkeeping), stated once: what lqr_carver.c does on the device it reads here.
 *
 * Pure integer and float bookkeeping, no device call, no I/O, no allocation: (1) the carver's geometry and the transitions that a
 * pass over the planes makes, (2) the walk of one direction of a resize -- liblqr's lqr_carver_resize_width: per step a session of
 * `depth`, the width shown after it, a flatten between the steps of an enlargement --, (3) one session's seam schedule: progress
 * reports, side switches, the levels a roll-back removes.  Compiled alone by tests/test_sched.py and compared with the walks
 * lqr_carver.c held before it read them from here, with tests/geometry_cases.py and with the CPU reference.
 *
 * Float evaluation matters (build with -ffp-contract=off): delta_max and the update step are float products truncated to int, as
 * in liblqr.
 */
#ifndef LQR_SCHED_H
#define LQR_SCHED_H

/* ---- geometry, in the carver frame (transposed => frame x runs along image y) ---- */
typedef struct LqrGeom {
    int w_start, h_start, w, h, w0, h0;
    int level, max_level;
    int transposed;
} LqrGeom;

void lqr_geom_reset(LqrGeom *g, int img_w, int img_h);         /* the image as it was handed in */
void lqr_geom_set_width(LqrGeom *g, int w1);                   /* the visible width, inside the multi-size range */
void lqr_geom_flattened(LqrGeom *g);                           /* what is visible became the image */
void lqr_geom_transposed(LqrGeom *g);                          /* of a flat carver */
/* levels up to `depth` built and inflated, n_seams of them new (depth - max_level of the root: an attached carver grows with it); the
 * width back at w_start */
void lqr_geom_session_done(LqrGeom *g, int depth, int n_seams);
void lqr_geom_map_loaded(LqrGeom *g, int depth);               /* a map of `depth` seams became a flat carver's levels */

/* three conditions that are NOT one: */
int lqr_geom_needs_flatten(const LqrGeom *g);                  /* the mask calls: anything hidden, inserted or not at full size */
int lqr_geom_is_flat(const LqrGeom *g);                        /* group_flatten: the carver is its own flattening */
int lqr_geom_flatten_before_transpose(const LqrGeom *g);       /* group_transpose */

/* the most columns one session may add to a frame of w_start: (int) ((enl_step - 1) * w_start) - 1 in float, at least 1 */
int lqr_sched_delta_max(float enl_step, int w_start);
/* seams between two progress reports: (int) max(total * update_step, 1) in float */
int lqr_sched_update_step(int total, float update_step);

/* ---- one direction of a resize ---- */
typedef struct LqrWalk {
    LqrGeom g;                  /* the walk's own copy, advanced step by step */
    float enl_step;
    int w1, want_transposed;
    int delta, gamma, delta_max;
    int total;                  /* |gamma| at the start: what progress is reported against */
} LqrWalk;

typedef struct LqrWalkStep {
    int transpose;              /* a transposition comes first */
    int depth;                  /* asked of group_build_maps: a session only where it lies beyond max_level ... */
    int frame;                  /* ... which then starts from a frame this wide (else 0) */
    int new_w;                  /* the width shown after the step */
    int gamma;                  /* columns still to go after the step */
    int flatten;                /* a flatten follows: the next step enlarges what this one made */
} LqrWalkStep;

void lqr_walk_begin(LqrWalk *k, const LqrGeom *g, float enl_step, int w1, int want_transposed);
int lqr_walk_next(LqrWalk *k, LqrWalkStep *s);                 /* 0: the direction is done, *s untouched */

/* some session would start from a frame wider than max_frame (decided from the sizes alone) */
int lqr_walk_frame_refused(const LqrGeom *g, float enl_step, int w1, int want_transposed, int max_frame);
/* a carver that cannot build maps: some step would need a transposition, a depth beyond max_level, or a second step */
int lqr_walk_needs_maps(const LqrGeom *g, float enl_step, int w1, int want_transposed);

/* the sizes of the current direction that lqr_walk_needs_maps refuses nothing of, as a closed form: one step, no session, no
 * transposition, no second step -- [w_start - (max_level - 1), w_start + min(max_level - 1, delta_max)].  (The walk also lets the
 * current width pass, whatever it is, because there is nothing to do: it lies inside the interval unless the enlargement step was
 * lowered after the carver was enlarged.) */
void lqr_geom_size_range(const LqrGeom *g, float enl_step, int *lo, int *hi);

/* ---- one session (one visibility-map build) ---- */
typedef struct LqrSession {
    int max_level, depth;       /* seams l = max_level .. depth - 1 */
    int n_seams, wc0;           /* from a carved frame wc0 wide */
    int first_level;            /* seam l is stored as level l + max_level - 1 */
    int finish;                 /* the session carves down to one column */
    int lr_switch_frequency, lr_switch_interval;
    int rescale_current, rescale_total, update_step;
} LqrSession;

typedef struct LqrSeam {
    int w_before;
    int report;                 /* a progress report is due before the seam ... */
    double fraction;            /* ... of this much of the direction */
    int full;                   /* after the carve the side flips and the DP is rebuilt in full */
} LqrSeam;

/* depth 0: down to one column */
void lqr_session_begin(LqrSession *s, int max_level, int depth, int wc0, int lr_switch_frequency, int rescale_current, int rescale_total,
                       int update_step);
void lqr_session_seam(const LqrSession *s, int l, LqrSeam *out);

#endif /* LQR_SCHED_H */
