/*
 * lqr_energy.h -- liblqr-1's energy read-outs: the energy the carver "sees", as it is, normalised to [0, 1], or
 * as a picture of any colour depth and image type; and the same three written straight to device memory.
 *
 * A caller shows the result next to its mask editor, uses it as a saliency picture, or combines it with a
 * detector of its own.  This header adds the calls on top of lqr.h with liblqr 0.4.1's prototypes, and leaves
 * lqr.h, lqr_coldepth.h, lqr_imagetype.h and lqr_masks.h as they are.
 *
 * Semantics (liblqr 0.4.1's; tests/golden/energy/ holds what the genuine code gave, tests/energy_cases.py the
 * same rules as a numpy model).
 *   - `orientation` must be 0 or 1 and `buffer` non-NULL, else LQR_ERROR and nothing happens.
 *   - The carver is prepared as lqr_carver_resize prepares it for seams of that orientation: a carver that is
 *     not at the width its visibility map was built for (enlarged, or grown again after a shrink) is flattened;
 *     a carver whose orientation differs from `orientation` is flattened if need be, TRANSPOSED AND LEFT THAT
 *     WAY: afterwards lqr_carver_get_orientation returns `orientation`, lqr_carver_scan_by_row changes with it,
 *     and the rigidity table has been rescaled as by any transposition.  A carver that was only shrunk and is
 *     asked for its own orientation stays as it is.  Attached carvers follow their root.
 *   - The energy is then built in that frame with the carver's energy function and bias: `orientation` selects
 *     the energy as vertical seams (0) or horizontal seams (1) see it.
 *   - The buffer receives lqr_carver_get_width x lqr_carver_get_height values, row-major, in IMAGE orientation
 *     whatever `orientation` is.  Nothing past them is written.
 *   - The calls are served on a carver that lqr_carver_init has not seen; a later lqr_carver_init and resize
 *     give what they would have given without the read-out (from the orientation the read-out left).
 *
 * lqr_carver_get_true_energy stores the energy values as they are (gfloat).
 *
 * lqr_carver_get_energy squashes each value and normalises; every operation is a float operation, rounded on
 * its own:
 *     s = 1 / (1 + 1 / e)         for e >= 0         (e = 0 gives 0)
 *     s = -1 / (1 - 1 / e)        for e < 0
 *     e_max starts at 0 (NOT at the first value), e_min at FLT_MAX; both are taken over s;
 *     if e_max > e_min every value becomes (s - e_min) / (e_max - e_min), otherwise the values stay s.
 * Because e_max starts at 0 an all-negative plane (a negative bias under LQR_EF_NULL) normalises to
 * [0, something below 1], not to [0, 1]; a plane of one non-negative value stays that squashed value (0 for
 * LQR_EF_NULL without bias), a plane of one negative value becomes 0.
 *
 * lqr_carver_get_energy_image writes a normalised energy e as width x height pixels of `col_depth` and
 * `image_type`, which are the caller's choice and independent of the carver's own:
 *     LQR_GREY_IMAGE, LQR_GREYA_IMAGE, LQR_RGB_IMAGE, LQR_RGBA_IMAGE    every colour channel e
 *     LQR_CMY_IMAGE                                                     every colour channel 1 - e
 *     LQR_CMYK_IMAGE, LQR_CMYKA_IMAGE                                   C = M = Y = 0, K = 1 - e
 *     alpha, where the type has one                                     1
 *     LQR_CUSTOM_IMAGE                                                  LQR_ERROR; nothing is written, the carver stays as it is
 * A value v is stored as (guchar) (v * 255) and (guint16) (v * 65535), products in double and truncated
 * (0.24875 stores as 63), as (gfloat) v, or as the double v itself.
 * The picture's e is NOT the float lqr_carver_get_energy stores (the vectors settle this; the two differ in
 * the last place).  In liblqr the picture has a loop of its own in which float and double are mixed, and it is
 * pinned here as the 53-bit build evaluates it: the squash above computed in double and rounded to float ONCE,
 * e_min and e_max floats over those, then (s - e_min) / (e_max - e_min) and 1 - e in double, unrounded until
 * they are stored.  Where e_max == e_min the picture is that of e = 0 (the float form keeps s there).
 *
 * Precision.  lqr_carver_get_energy is float-only code: as for the other float-only functions,
 * "bit-exact" refers to an SSE2 build of liblqr, which rounds every operation to float.  The i386 build as
 * shipped keeps x87 intermediates and differs from it by a few units in the last place.
 *
 * Where the engine does not follow liblqr:
 *   - a carver that is attached to another returns LQR_ERROR from all five calls and nothing changes.  liblqr
 *     serves it, and may flatten or transpose the attached carver ALONE; it then no longer has the geometry of
 *     its root, whose next resize walks it with the root's sizes.  Here the planes of an attached carver follow
 *     the root's in one pass and cannot be re-laid alone; read the energy from a root carver made of that image.
 *   - a frame ONE pixel wide (an image 1 wide read with orientation 0, 1 high with orientation 1): the energy
 *     is 0, as it has always been in this engine's carving and in lqrx_carver_get_energy.  liblqr's gradient
 *     reads the neighbour outside the frame -- the pixel of the next row, nothing after the last -- and reports
 *     that difference.
 *   - a `col_depth` outside the enum returns LQR_ERROR and nothing happens.  liblqr flattens and transposes the
 *     carver, writes nothing and returns LQR_OK.
 *   - energies that are NaN or infinite (float images holding such pixels): the result is unspecified.  liblqr's
 *     MAX / MIN macros make its own result depend on the order of the pixels there.
 * LQR_NOMEM from any of the calls leaves the carver usable, in one of the states the sequence above passes through
 * (as it was; flattened; transposed), and the buffer untouched.
 *
 * Extensions.  lqrx_carver_get_energy_device is lqr_carver_get_energy (normalised != 0) or
 * lqr_carver_get_true_energy (normalised == 0), and lqrx_carver_get_energy_image_device is
 * lqr_carver_get_energy_image, into DEVICE memory, e.g. a tensor the caller feeds to a model next: the same
 * semantics and side effects, nothing is copied to the host, and the call returns once the buffer has been
 * written.  The buffer must be aligned to its element (1, 2, 4 or 8 bytes); pixels are stored with wider
 * vector stores when its address allows them.
 */
#ifndef __LQR_ENERGY_H__
#define __LQR_ENERGY_H__

#include "lqr.h"
#include "lqr_coldepth.h"

#ifdef __cplusplus
extern "C" {
#endif

LqrRetVal lqr_carver_get_energy(LqrCarver *r, gfloat *buffer, gint orientation);
LqrRetVal lqr_carver_get_true_energy(LqrCarver *r, gfloat *buffer, gint orientation);
LqrRetVal lqr_carver_get_energy_image(LqrCarver *r, void *buffer, gint orientation, LqrColDepth col_depth, LqrImageType image_type);

LqrRetVal lqrx_carver_get_energy_device(LqrCarver *r, void *device_buffer, gint orientation, gint normalised);
LqrRetVal lqrx_carver_get_energy_image_device(LqrCarver *r, void *device_buffer, gint orientation, LqrColDepth col_depth,
                                              LqrImageType image_type);

#ifdef __cplusplus
}
#endif

#endif /* __LQR_ENERGY_H__ */
