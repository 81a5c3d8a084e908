/*
 * lqr_mask_queue.h -- the host-side queue behind lqr_carver_bias_add_xy / lqr_carver_rigmask_add_xy (include/lqr_masks.h).
 *
 * Pure bookkeeping, no device call and no pixel arithmetic: entries {index into the base layout, the caller's gdouble} in call
 * order, and for each entry the number of earlier entries of the run that hit the same pixel (its occurrence number).  A flush
 * applies the entries bucket by bucket -- all first occurrences, then all second ones, ... -- one kernel launch per bucket in
 * order on one stream: inside a bucket every pixel is distinct, so the launch needs no atomics, and a pixel sees its values in
 * call order, which is what float addition (bias) and last-writer-wins (rigidity) need.  Almost every real run has one bucket.
 *
 * The queue is bounded (max_entries; LQR_MASKQ_DEFAULT_MAX by default): an append to a full queue returns LQR_MASKQ_FULL, the
 * caller flushes and appends again.  Allocation failures return LQR_MASKQ_NOMEM and leave the queue as it was.
 */
#ifndef LQR_MASK_QUEUE_H
#define LQR_MASK_QUEUE_H

#include <stddef.h>

#define LQR_MASKQ_OK 0
#define LQR_MASKQ_FULL 1
#define LQR_MASKQ_NOMEM (-1)
#define LQR_MASKQ_EARG (-2)      /* an index outside the layout: nothing is queued */
/* 4 Mi entries: 16 bytes each in the queue, 12 more in the packed form of a flush */
#define LQR_MASKQ_DEFAULT_MAX ((size_t) 1 << 22)

typedef struct LqrMaskQueue {
    int *index;             /* [n] position in the base layout */
    double *value;          /* [n] the caller's value, untouched */
    unsigned *occ;          /* [n] earlier entries of this run on the same pixel */
    size_t n, cap, max_entries;
    unsigned *count;        /* [npix] entries of this run per pixel */
    size_t npix;
    unsigned buckets;       /* 1 + the largest occurrence number (0: empty) */
} LqrMaskQueue;

void lqr_maskq_init(LqrMaskQueue *q, size_t max_entries);      /* max_entries 0: the default bound */
/* one entry for pixel `index` of a base layout of npix pixels (npix may change only while the queue is empty) */
int lqr_maskq_append(LqrMaskQueue *q, size_t npix, int index, double value);
/* the entries ordered by bucket, call order kept inside a bucket: index_out / value_out hold n entries, start[b] .. start[b + 1]
 * are bucket b's (start holds buckets + 1 values) */
void lqr_maskq_pack(const LqrMaskQueue *q, int *index_out, double *value_out, size_t *start);
/* drop the entries, keep the storage */
void lqr_maskq_reset(LqrMaskQueue *q);
void lqr_maskq_free(LqrMaskQueue *q);

#endif /* LQR_MASK_QUEUE_H */
