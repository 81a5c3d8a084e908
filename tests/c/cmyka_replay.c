/*
 * cmyka_replay.c -- a consumer of the image-type surface (include/lqr_imagetype.h), in C.
 *
 * The sequence is the one an image library makes that hands over "all the pixel channels" of a 32-bit float CMYK image with
 * an alpha channel: it raises the channel limit once after loading the library, keeps its own pixel buffer
 * (lqr_carver_set_preserve_input_image), makes no configuration call -- five channels are CMYKA by default -- carves with the
 * library defaults and reads the result back pixel by pixel with lqr_carver_scan_ext.
 *
 *   cmyka_replay IN OUT
 *   IN:  int32 w, h, new_w, new_h; then w x h x 5 floats (C, M, Y, K, alpha, interleaved)
 *   OUT: int32 new_w, new_h, pixels visited; then new_w x new_h x 5 floats, then the (x, y) of every visit in order
 * Exit status: 0 ok, 2 usage / I/O, 3 a library call failed, 4 the caller's buffer was changed.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lqr.h"
#include "lqr_imagetype.h"

#define CH 5

int main(int argc, char **argv)
{
    FILE *f;
    int hd[4], w, h, nw, nh, x, y, n = 0;
    size_t npx;
    float *pixels, *copy, *out;
    int *visits;
    void *px;
    LqrCarver *r;

    if (argc != 3 || !(f = fopen(argv[1], "rb"))) return 2;
    if (fread(hd, sizeof(int), 4, f) != 4) return 2;
    w = hd[0]; h = hd[1]; nw = hd[2]; nh = hd[3];
    npx = (size_t) w * h;
    pixels = (float *) malloc(npx * CH * sizeof(float));
    copy = (float *) malloc(npx * CH * sizeof(float));
    out = (float *) calloc((size_t) nw * nh * CH, sizeof(float));
    visits = (int *) malloc((size_t) nw * nh * 2 * sizeof(int));
    if (!pixels || !copy || !out || !visits) return 2;
    if (fread(pixels, sizeof(float), npx * CH, f) != npx * CH) return 2;
    fclose(f);
    memcpy(copy, pixels, npx * CH * sizeof(float));

    if (lqr_carver_new_ext(pixels, w, h, CH, LQR_COLDEPTH_32F)) return 3;       /* refused under the default limit */
    if (lqrx_set_max_channels(8) != 4 || lqrx_set_max_channels(3) != 8 || lqrx_set_max_channels(8) != 8) return 3;
    r = lqr_carver_new_ext(pixels, w, h, CH, LQR_COLDEPTH_32F);
    if (!r) return 3;
    lqr_carver_set_preserve_input_image(r);
    if (lqr_carver_get_col_depth(r) != LQR_COLDEPTH_32F || lqr_carver_get_image_type(r) != LQR_CMYKA_IMAGE) return 3;
    if (lqr_carver_init(r, 1, 0.0f) != LQR_OK) return 3;
    if (lqr_carver_resize(r, nw, nh) != LQR_OK) return 3;
    if (lqr_carver_get_width(r) != nw || lqr_carver_get_height(r) != nh || lqr_carver_get_channels(r) != CH) return 3;
    lqr_carver_scan_reset(r);
    while (lqr_carver_scan_ext(r, &x, &y, &px)) {
        if (x < 0 || x >= nw || y < 0 || y >= nh || n >= nw * nh) return 3;
        memcpy(out + ((size_t) y * nw + x) * CH, px, CH * sizeof(float));
        visits[2 * n] = x;
        visits[2 * n + 1] = y;
        n++;
    }
    lqr_carver_destroy(r);

    if (memcmp(copy, pixels, npx * CH * sizeof(float)) != 0) return 4;
    free(pixels);           /* the caller's buffer: the carver did not free it */
    free(copy);

    if (!(f = fopen(argv[2], "wb"))) return 2;
    hd[0] = nw; hd[1] = nh; hd[2] = n;
    if (fwrite(hd, sizeof(int), 3, f) != 3 || fwrite(out, sizeof(float), (size_t) nw * nh * CH, f) != (size_t) nw * nh * CH ||
        fwrite(visits, sizeof(int), (size_t) n * 2, f) != (size_t) n * 2)
        return 2;
    fclose(f);
    free(out);
    free(visits);
    return 0;
}
