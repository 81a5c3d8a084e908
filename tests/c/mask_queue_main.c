/* Stand-alone exercise of host/lqr_mask_queue.c (tests/test_mask_queue.py builds it with -fsanitize=address,undefined):
 * an empty flush, a single entry, repeats that force several buckets, the bound, reset followed by reuse. */
#include <stdio.h>
#include <stdlib.h>

#include "lqr_mask_queue.h"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "line %d: %s\n", __LINE__, #c); return 1; } } while (0)

/* pack, and check that applying the buckets in order gives what applying the calls one by one gives: per pixel the sequence of values */
static int pack_matches_call_order(const LqrMaskQueue *q, size_t npix)
{
    int *index = (int *) malloc((q->n + 1) * sizeof *index);
    double *value = (double *) malloc((q->n + 1) * sizeof *value);
    size_t *start = (size_t *) malloc(((size_t) q->buckets + 1) * sizeof *start);
    /* "last value written" and "sum in order" per pixel, by calls and by buckets: order-sensitive folds */
    double *by_call = (double *) calloc(npix, sizeof(double)), *by_bucket = (double *) calloc(npix, sizeof(double));
    char *seen = (char *) calloc(npix, 1);
    size_t i, b, p;
    int ok = 1;
    lqr_maskq_pack(q, index, value, start);
    ok &= start[0] == 0 && start[q->buckets] == q->n;
    for (i = 0; i < q->n; i++) by_call[q->index[i]] = by_call[q->index[i]] * 3.0 + q->value[i];
    for (b = 0; b < q->buckets; b++) {
        ok &= start[b] <= start[b + 1];
        for (p = 0; p < npix; p++) seen[p] = 0;
        for (i = start[b]; i < start[b + 1]; i++) {
            ok &= !seen[index[i]];              /* every pixel at most once per bucket */
            seen[index[i]] = 1;
            by_bucket[index[i]] = by_bucket[index[i]] * 3.0 + value[i];
        }
    }
    for (p = 0; p < npix; p++) ok &= by_call[p] == by_bucket[p];
    free(index); free(value); free(start); free(by_call); free(by_bucket); free(seen);
    return ok;
}

int main(void)
{
    LqrMaskQueue q;
    size_t i, start1[1];
    int idx1[1];
    double val1[1];

    /* an empty flush */
    lqr_maskq_init(&q, 0);
    CHECK(q.n == 0 && q.buckets == 0 && q.max_entries == LQR_MASKQ_DEFAULT_MAX);
    lqr_maskq_pack(&q, idx1, val1, start1);
    CHECK(start1[0] == 0);
    lqr_maskq_reset(&q);
    CHECK(pack_matches_call_order(&q, 4));

    /* a single entry */
    CHECK(lqr_maskq_append(&q, 12, 5, 0.75) == LQR_MASKQ_OK);
    CHECK(q.n == 1 && q.buckets == 1 && q.index[0] == 5 && q.value[0] == 0.75 && q.occ[0] == 0);
    CHECK(pack_matches_call_order(&q, 12));
    /* an index outside the layout, another layout while entries are queued */
    CHECK(lqr_maskq_append(&q, 12, 12, 1.0) == LQR_MASKQ_EARG && lqr_maskq_append(&q, 12, -1, 1.0) == LQR_MASKQ_EARG);
    CHECK(lqr_maskq_append(&q, 20, 5, 1.0) == LQR_MASKQ_FULL && q.n == 1);
    lqr_maskq_reset(&q);
    CHECK(q.n == 0 && q.buckets == 0);
    CHECK(lqr_maskq_append(&q, 20, 19, 1.0) == LQR_MASKQ_OK && q.npix == 20);
    lqr_maskq_free(&q);

    /* repeats: 5000 entries on 700 pixels in an interleaved order, more than one growth of the arrays; some pixels 8 times, some 7 */
    lqr_maskq_init(&q, 0);
    for (i = 0; i < 5000; i++) CHECK(lqr_maskq_append(&q, 1000, (int) ((i * 37) % 700), (double) i + 0.5) == LQR_MASKQ_OK);
    CHECK(q.n == 5000 && q.buckets == 8);
    CHECK(pack_matches_call_order(&q, 1000));
    /* reset followed by reuse: the counts start over */
    lqr_maskq_reset(&q);
    for (i = 0; i < 1000; i++) CHECK(q.count[i] == 0);
    for (i = 0; i < 30; i++) CHECK(lqr_maskq_append(&q, 1000, (int) (i % 10), (double) i) == LQR_MASKQ_OK);
    CHECK(q.buckets == 3 && pack_matches_call_order(&q, 1000));
    lqr_maskq_reset(&q);                /* the short-run path of reset */
    for (i = 0; i < 1000; i++) CHECK(q.count[i] == 0);
    lqr_maskq_free(&q);
    CHECK(q.n == 0 && q.index == NULL && q.count == NULL);

    /* the bound */
    lqr_maskq_init(&q, 8);
    for (i = 0; i < 8; i++) CHECK(lqr_maskq_append(&q, 4, (int) (i % 4), 1.0) == LQR_MASKQ_OK);
    CHECK(lqr_maskq_append(&q, 4, 0, 2.0) == LQR_MASKQ_FULL && q.n == 8 && q.buckets == 2);
    CHECK(pack_matches_call_order(&q, 4));
    lqr_maskq_reset(&q);
    CHECK(lqr_maskq_append(&q, 4, 0, 2.0) == LQR_MASKQ_OK && q.n == 1 && q.buckets == 1 && q.cap <= 8);
    lqr_maskq_free(&q);
    lqr_maskq_free(&q);                 /* twice is harmless */
    printf("mask queue ok\n");
    return 0;
}
