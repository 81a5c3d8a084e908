/*
 * energy_replay.c -- a C caller of the energy read-outs (include/lqr_energy.h).
 *
 * The sequence is the one an editor makes that shows the user what the carver "sees" next to its mask editor: an
 * 8-bit image, the energy function chosen, then the true energy, the normalised energy and an RGBA preview of it
 * for seams of one orientation -- before any resize, and without lqr_carver_init.
 *
 *   energy_replay IN OUT
 *   IN:  int32 w, h, channels, energy function, orientation; then w x h x channels bytes
 *   OUT: int32 w, h, orientation after the calls; w x h floats (true), w x h floats (normalised), w x h x 4 bytes (RGBA)
 * Exit status: 0 ok, 2 usage / I/O, 3 a library call failed, 4 a call that must fail did not.
 */
#include <stdio.h>
#include <stdlib.h>

#include "lqr.h"
#include "lqr_coldepth.h"
#include "lqr_energy.h"

int main(int argc, char **argv)
{
    FILE *f;
    int hd[5], w, h, ch, o, out_hd[3];
    size_t npx;
    guchar *pixels, *rgba;
    gfloat *true_e, *norm_e;
    LqrCarver *r;

    if (argc != 3 || !(f = fopen(argv[1], "rb"))) return 2;
    if (fread(hd, sizeof(int), 5, f) != 5) return 2;
    w = hd[0]; h = hd[1]; ch = hd[2]; o = hd[4];
    npx = (size_t) w * h;
    pixels = (guchar *) malloc(npx * ch);
    true_e = (gfloat *) malloc(npx * sizeof(gfloat));
    norm_e = (gfloat *) malloc(npx * sizeof(gfloat));
    rgba = (guchar *) malloc(npx * 4);
    if (!pixels || !true_e || !norm_e || !rgba) return 2;
    if (fread(pixels, 1, npx * ch, f) != npx * ch) return 2;
    fclose(f);

    r = lqr_carver_new(pixels, w, h, ch);       /* the carver owns `pixels` now */
    if (!r) return 3;
    if (lqr_carver_set_energy_function_builtin(r, (LqrEnergyFuncBuiltinType) hd[3]) != LQR_OK) return 3;
    if (lqr_carver_get_energy(r, norm_e, 2) != LQR_ERROR || lqr_carver_get_true_energy(r, NULL, o) != LQR_ERROR) return 4;
    if (lqr_carver_get_energy_image(r, rgba, o, LQR_COLDEPTH_8I, LQR_CUSTOM_IMAGE) != LQR_ERROR) return 4;
    if (lqr_carver_get_true_energy(r, true_e, o) != LQR_OK) return 3;
    if (lqr_carver_get_energy(r, norm_e, o) != LQR_OK) return 3;
    if (lqr_carver_get_energy_image(r, rgba, o, LQR_COLDEPTH_8I, LQR_RGBA_IMAGE) != LQR_OK) return 3;
    out_hd[0] = lqr_carver_get_width(r); out_hd[1] = lqr_carver_get_height(r); out_hd[2] = lqr_carver_get_orientation(r);
    lqr_carver_destroy(r);
    if (out_hd[0] != w || out_hd[1] != h) return 3;

    if (!(f = fopen(argv[2], "wb"))) return 2;
    if (fwrite(out_hd, sizeof(int), 3, f) != 3 || fwrite(true_e, sizeof(gfloat), npx, f) != npx ||
        fwrite(norm_e, sizeof(gfloat), npx, f) != npx || fwrite(rgba, 4, npx, f) != npx) return 2;
    fclose(f);
    free(true_e); free(norm_e); free(rgba);
    return 0;
}
