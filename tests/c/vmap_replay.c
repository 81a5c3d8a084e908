/*
 * vmap_replay.c -- a C caller of seam-map loading (include/lqr_vmap.h).
 *
 * The sequence is the one a video pipeline makes: the key frame is carved, its seam map is dumped and copied into a map
 * object of the caller's own (lqr_vmap_new), that map is loaded into the next frame -- a carver lqr_carver_init has never
 * seen -- and the frame is resized by it and scanned, at the key frame's new width and at an enlarged one.
 *
 *   vmap_replay IN OUT
 *   IN:  int32 w, h, channels, new width, enlarged width; then the key frame and the next frame, w x h x channels bytes each
 *   OUT: int32 depth, orientation; the map (w x h int32); the next frame at the new width, then at the enlarged width
 * Exit status: 0 ok, 2 usage / I/O, 3 a library call failed, 4 a call that must fail did not.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lqr.h"
#include "lqr_vmap.h"

static int scan_to(LqrCarver *r, guchar *out, int w, int h, int ch)
{
    gint n;
    guchar *line;
    int lines = 0;
    if (lqr_carver_get_width(r) != w || lqr_carver_get_height(r) != h || !lqr_carver_scan_by_row(r)) return 0;
    lqr_carver_scan_reset(r);
    while (lqr_carver_scan_line(r, &n, &line)) {
        memcpy(out + (size_t) n * w * ch, line, (size_t) w * ch);
        lines++;
    }
    return lines == h;
}

int main(int argc, char **argv)
{
    FILE *f;
    int hd[5], w, h, ch, w1, w2, out_hd[2];
    size_t nbytes;
    guchar *key, *next, *small, *large;
    gint *copy;
    LqrCarver *a, *b;
    LqrVMap *dumped, *mine;

    if (argc != 3 || !(f = fopen(argv[1], "rb"))) return 2;
    if (fread(hd, sizeof(int), 5, f) != 5) return 2;
    w = hd[0]; h = hd[1]; ch = hd[2]; w1 = hd[3]; w2 = hd[4];
    nbytes = (size_t) w * h * ch;
    key = (guchar *) malloc(nbytes);
    next = (guchar *) malloc(nbytes);
    small = (guchar *) malloc((size_t) w1 * h * ch);
    large = (guchar *) malloc((size_t) w2 * h * ch);
    copy = (gint *) malloc((size_t) w * h * sizeof(gint));
    if (!key || !next || !small || !large || !copy) return 2;
    if (fread(key, 1, nbytes, f) != nbytes || fread(next, 1, nbytes, f) != nbytes) return 2;
    fclose(f);

    /* the key frame: carved, its map dumped and copied */
    a = lqr_carver_new(key, w, h, ch);          /* the carver owns `key` now */
    if (!a || lqr_carver_init(a, 1, 0) != LQR_OK) return 3;
    if (lqr_carver_resize(a, w1, h) != LQR_OK) return 3;
    if (!(dumped = lqr_vmap_dump(a))) return 3;
    if (lqr_vmap_get_width(dumped) != w || lqr_vmap_get_height(dumped) != h) return 3;
    memcpy(copy, lqr_vmap_get_data(dumped), (size_t) w * h * sizeof(gint));
    out_hd[0] = lqr_vmap_get_depth(dumped); out_hd[1] = lqr_vmap_get_orientation(dumped);
    mine = lqr_vmap_new(copy, w, h, out_hd[0], out_hd[1]);     /* the map owns `copy` now */
    if (!mine) return 3;
    if (lqr_vmap_load(a, mine) != LQR_ERROR) return 4;         /* an initialised carver takes no map */

    /* the next frame: no lqr_carver_init, the key frame's seams */
    b = lqr_carver_new(next, w, h, ch);
    if (!b) return 3;
    if (lqr_vmap_load(b, mine) != LQR_OK) return 3;
    if (lqr_carver_get_depth(b) != out_hd[0] || lqr_carver_get_enl_step(b) != 2.0f) return 3;
    if (lqr_carver_resize(b, w1 - 1, h) != LQR_ERROR) return 4;  /* one seam more than the map holds */
    if (lqr_carver_resize(b, w1, h) != LQR_OK || !scan_to(b, small, w1, h, ch)) return 3;
    if (lqr_carver_resize(b, w2, h) != LQR_OK || !scan_to(b, large, w2, h, ch)) return 3;
    if (lqr_vmap_internal_dump(b) != LQR_OK || !lqr_vmap_list_start(b)) return 3;

    if (!(f = fopen(argv[2], "wb"))) return 2;
    if (fwrite(out_hd, sizeof(int), 2, f) != 2 || fwrite(lqr_vmap_get_data(mine), sizeof(gint), (size_t) w * h, f) != (size_t) w * h ||
        fwrite(small, 1, (size_t) w1 * h * ch, f) != (size_t) w1 * h * ch || fwrite(large, 1, (size_t) w2 * h * ch, f) != (size_t) w2 * h * ch) return 2;
    fclose(f);
    lqr_vmap_destroy(dumped);
    lqr_vmap_destroy(mine);
    lqr_carver_destroy(a);
    lqr_carver_destroy(b);
    free(small); free(large);
    return 0;
}
