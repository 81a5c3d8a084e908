/* lqr_mask_queue.c -- see lqr_mask_queue.h.  Plain C, no dependency but the C library: tests/test_mask_queue.py compiles it alone. */
#include <stdlib.h>
#include <string.h>

#include "lqr_mask_queue.h"

void lqr_maskq_init(LqrMaskQueue *q, size_t max_entries)
{
    memset(q, 0, sizeof *q);
    q->max_entries = max_entries ? max_entries : LQR_MASKQ_DEFAULT_MAX;
}

static int grow(LqrMaskQueue *q)
{
    size_t cap = q->cap ? 2 * q->cap : 1024;
    int *index;
    double *value;
    unsigned *occ;
    if (cap > q->max_entries) cap = q->max_entries;
    /* one array at a time: whichever was moved stays valid for the old capacity if a later one fails */
    if (!(index = (int *) realloc(q->index, cap * sizeof *index))) return LQR_MASKQ_NOMEM;
    q->index = index;
    if (!(value = (double *) realloc(q->value, cap * sizeof *value))) return LQR_MASKQ_NOMEM;
    q->value = value;
    if (!(occ = (unsigned *) realloc(q->occ, cap * sizeof *occ))) return LQR_MASKQ_NOMEM;
    q->occ = occ;
    q->cap = cap;
    return LQR_MASKQ_OK;
}

int lqr_maskq_append(LqrMaskQueue *q, size_t npix, int index, double value)
{
    if (index < 0 || (size_t) index >= npix) return LQR_MASKQ_EARG;
    if (q->n >= q->max_entries) return LQR_MASKQ_FULL;
    if (q->npix != npix || !q->count) {
        unsigned *count;
        if (q->n) return LQR_MASKQ_FULL;            /* another layout: what is queued belongs to the old one */
        if (!(count = (unsigned *) calloc(npix, sizeof *count))) return LQR_MASKQ_NOMEM;
        free(q->count);
        q->count = count;
        q->npix = npix;
    }
    if (q->n == q->cap) {
        int rc = grow(q);
        if (rc) return rc;
    }
    q->index[q->n] = index;
    q->value[q->n] = value;
    q->occ[q->n] = q->count[index]++;
    if (q->occ[q->n] + 1 > q->buckets) q->buckets = q->occ[q->n] + 1;
    q->n++;
    return LQR_MASKQ_OK;
}

void lqr_maskq_pack(const LqrMaskQueue *q, int *index_out, double *value_out, size_t *start)
{
    size_t i, b, at;
    /* counting sort by occurrence number: stable, so call order is kept inside a bucket */
    for (b = 0; b <= q->buckets; b++) start[b] = 0;
    for (i = 0; i < q->n; i++) start[q->occ[i] + 1]++;
    for (b = 0; b < q->buckets; b++) start[b + 1] += start[b];
    for (i = 0; i < q->n; i++) {
        at = start[q->occ[i]]++;
        index_out[at] = q->index[i];
        value_out[at] = q->value[i];
    }
    for (b = q->buckets; b > 0; b--) start[b] = start[b - 1];      /* the cursors ended where the next bucket starts */
    start[0] = 0;
}

void lqr_maskq_reset(LqrMaskQueue *q)
{
    size_t i;
    /* a short run on a large image clears only what it touched */
    if (q->count) {
        if (q->n < q->npix / 8)
            for (i = 0; i < q->n; i++) q->count[q->index[i]] = 0;
        else
            memset(q->count, 0, q->npix * sizeof *q->count);
    }
    q->n = 0;
    q->buckets = 0;
}

void lqr_maskq_free(LqrMaskQueue *q)
{
    const size_t max_entries = q->max_entries;
    free(q->index); free(q->value); free(q->occ); free(q->count);
    lqr_maskq_init(q, max_entries);
}
