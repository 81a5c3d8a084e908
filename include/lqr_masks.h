/*
 * lqr_masks.h -- liblqr-1's computed-mask surface: bias and rigidity masks as gdouble planes or one
 * (x, y, value) at a time, and the same planes taken straight from device memory.
 *
 * lqr.h has the two forms gimp-lqr-plugin feeds from painted 8-bit layers (lqr_carver_bias_add_rgb_area,
 * lqr_carver_rigmask_add_rgb_area).  A caller that derives its masks from a detector (faces, saliency,
 * text) uses the forms below; digiKam's content-aware resize calls lqr_carver_bias_add_xy once for every
 * pixel of its mask.  This header adds them on top of lqr.h with liblqr 0.4.1's prototypes, and leaves
 * lqr.h, lqr_coldepth.h and lqr_imagetype.h as they are.
 *
 * Semantics (liblqr 0.4.1's; tests/golden/masks/ holds what the genuine code gave, tests/mask_cases.py
 * the same rules as a numpy model).  (x, y), the offsets and the mask sizes are in IMAGE orientation: a
 * carver in orientation 1 maps them to its own frame.
 *   - Every form first flattens a carver that is not at its base size.
 *   - The area forms clip as the rgb forms do: offsets may be negative, the mask may hang over any side
 *     of the image or miss it altogether (nothing is written, LQR_OK).
 *   - lqr_carver_bias_add_area ADDS (gfloat) ((gdouble) bias_factor * v / 2) to the pixel's bias;
 *     bias_factor == 0 returns LQR_OK and does nothing at all (no flattening either).
 *   - lqr_carver_bias_add_xy ADDS (gfloat) bias / 2; bias == 0 likewise does nothing.
 *   - lqr_carver_rigmask_add_area, _add, _add_rgb ASSIGN (gfloat) v: the last writer wins.
 *     lqr_carver_rigmask_add_xy ADDS (gfloat) rigidity (liblqr 0.4.1 does; the name is meant literally).
 *   - lqr_carver_bias_add, lqr_carver_rigmask_add and the two _rgb forms are the _area forms at the
 *     carver's current width and height and offset 0.
 *   - lqr_carver_bias_clear / lqr_carver_rigmask_clear drop the plane (and what is queued for it): the
 *     carver carves as one that never had it.
 * Every operation is rounded to its C type, as an SSE2 build of liblqr rounds it:
 * the product and the halving in double, one conversion to float, one float addition.
 *
 * Return values.  The rigidity forms need a carver that lqr_carver_init has seen and return LQR_ERROR on
 * any other, attached ones included, as liblqr does.  The bias forms of this header are served before
 * lqr_carver_init too, as liblqr serves them (lqr_carver_bias_add_rgb_area of lqr.h keeps returning
 * LQR_ERROR there).  Where the engine cannot follow liblqr:
 *   - the bias forms on a carver that is attached to another return LQR_ERROR here (as
 *     lqr_carver_bias_add_rgb_area always has); liblqr accepts them and keeps a bias plane that no energy
 *     ever reads;
 *   - the _xy forms with (x, y) outside the image return LQR_ERROR and write nothing; liblqr does not
 *     check and writes outside its plane;
 *   - lqr_carver_rigmask_add and lqr_carver_rigmask_add_rgb take the mask to have the carver's current
 *     width and height, as documented above and as liblqr's two bias forms do.  liblqr takes the size from
 *     the carver's buffers as they are before it flattens, in the carver's own frame: on a carver that is
 *     not flat, or in orientation 1, it reads the mask with another row length and past its end.
 *
 * The _xy forms are queued on the host: a call costs no device work, and a run of them
 * reaches the planes, in call order, before anything reads or changes the planes -- another mask call, a
 * clear, lqr_carver_resize, lqr_carver_flatten, lqrx_carver_resize_batch, the read-outs below.  Only the
 * first call of a run may flatten the carver and allocate the plane.  LQR_NOMEM from any of them leaves
 * the carver usable.
 *
 * Orientation 1.  liblqr 0.4.1 swaps the axes of a transposed carver AFTER it has added max(0, x_off)
 * and max(0, y_off), so that there the positive part of x_off moves the mask along y and that of y_off
 * along x -- past the end of a row, into the next one or out of the plane (DESIGN.md 3.2 has the
 * vectors).  The engine applies the offsets in image orientation whatever the carver's orientation, as
 * its rgb forms of lqr.h always have; the two agree whenever max(0, x_off) == max(0, y_off).
 *
 * Extensions.  lqrx_carver_bias_add_area_device / lqrx_carver_rigmask_add_area_device are the _area
 * forms on width * height values of `depth` (LQR_COLDEPTH_32F: float, LQR_COLDEPTH_64F: double; another
 * depth is LQR_ERROR) that already lie in DEVICE memory, e.g. the output tensor of a saliency model: no
 * staging copy is made, and the call returns when the kernel has read the buffer, so the caller may
 * reuse it.  A float value is widened to double first (exactly), then treated as above.
 * lqrx_carver_get_bias / lqrx_carver_get_rigmask (test hooks) copy the plane of a FLAT carver out in
 * image orientation, lqr_carver_get_width x lqr_carver_get_height floats; all zeros when the carver has
 * none; LQR_ERROR when the carver is not flat.
 */
#ifndef __LQR_MASKS_H__
#define __LQR_MASKS_H__

#include "lqr.h"
#include "lqr_coldepth.h"

#ifdef __cplusplus
extern "C" {
#endif

LqrRetVal lqr_carver_bias_add_xy(LqrCarver *r, gdouble bias, gint x, gint y);
LqrRetVal lqr_carver_bias_add_area(LqrCarver *r, gdouble *buffer, gint bias_factor, gint width, gint height, gint x_off, gint y_off);
LqrRetVal lqr_carver_bias_add(LqrCarver *r, gdouble *buffer, gint bias_factor);
LqrRetVal lqr_carver_bias_add_rgb(LqrCarver *r, guchar *rgb, gint bias_factor, gint channels);
void lqr_carver_bias_clear(LqrCarver *r);
LqrRetVal lqr_carver_rigmask_add_xy(LqrCarver *r, gdouble rigidity, gint x, gint y);
LqrRetVal lqr_carver_rigmask_add_area(LqrCarver *r, gdouble *buffer, gint width, gint height, gint x_off, gint y_off);
LqrRetVal lqr_carver_rigmask_add(LqrCarver *r, gdouble *buffer);
LqrRetVal lqr_carver_rigmask_add_rgb(LqrCarver *r, guchar *rgb, gint channels);
void lqr_carver_rigmask_clear(LqrCarver *r);

LqrRetVal lqrx_carver_bias_add_area_device(LqrCarver *r, const void *device_buffer, LqrColDepth depth, gint bias_factor,
                                           gint width, gint height, gint x_off, gint y_off);
LqrRetVal lqrx_carver_rigmask_add_area_device(LqrCarver *r, const void *device_buffer, LqrColDepth depth,
                                              gint width, gint height, gint x_off, gint y_off);
LqrRetVal lqrx_carver_get_bias(LqrCarver *r, gfloat *out);
LqrRetVal lqrx_carver_get_rigmask(LqrCarver *r, gfloat *out);

#ifdef __cplusplus
}
#endif

#endif /* __LQR_MASKS_H__ */
