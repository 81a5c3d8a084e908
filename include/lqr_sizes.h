/*
 * lqr_sizes.h -- a carver read at many sizes in one pass (an extension: liblqr has no such call).
 *
 * A carver is liblqr's multi-size image.  After one session of lqr_carver_resize, or one lqr_vmap_load, its
 * seam map covers every size between the smallest it was carved to and the largest it was enlarged to, in
 * the direction the map lies.  lqr_carver_resize followed by a read-out serves those sizes one at a time;
 * the calls here serve any number of them from ONE pass over the carver's pixels and map, without touching
 * the carver.
 *
 * lqrx_carver_size_range tells which sizes: the closed interval [*min_size, *max_size] (either pointer may be
 * NULL) of widths when it returns 0, of heights when it returns 1 -- lqr_carver_get_orientation, the direction
 * of the carver's map.  It returns -1 on a NULL carver.  The interval holds exactly the sizes that
 * lqr_carver_resize reaches by showing or hiding seams of the map it has, in one step:
 *     min = ref - depth,  max = ref + min(depth, delta_max)
 * where ref is lqr_carver_get_ref_width (_height), depth lqr_carver_get_depth and delta_max the most one step
 * may add at the carver's enlargement step: (int) ((enl_step - 1) * ref) - 1, at least 1.  A larger size is a
 * stepwise enlargement in liblqr -- a flatten and a new session -- and not the threshold picture of this map:
 * it is refused.  A carver that has no map (a new, a flattened one) has min == max, its own size.  A smaller
 * enlargement step (lqr_carver_set_enl_step) lowers max -- below the carver's current size, if it was enlarged
 * further under the larger step: that size is then refused like any other above max.  lqr_vmap_load sets the step
 * to 2.0, so a carver with a loaded map serves the whole map.  An attached carver answers with its root's step.
 *
 * lqrx_carver_read_sizes_device writes n images into DEVICE memory, lqrx_carver_read_sizes into host memory.
 * out[k] is the image at sizes[k]: sizes[k] x height pixels when the direction is 0, width x sizes[k] when it
 * is 1, in IMAGE orientation, row-major, each pixel lqr_carver_get_channels samples of the carver's colour
 * depth (lqrx_carver_read_image_device, by contrast, writes in the carver's orientation).
 *
 * The contract:
 *   - out[k] equals, byte for byte, what lqr_carver_resize to that size followed by lqrx_carver_read_image
 *     returns.
 *   - The call is a pure read.  Afterwards the carver has the visible size, level and orientation it had; its
 *     scan-line cursor and cache are untouched; nothing is flattened or transposed.  As with the other
 *     read-outs of lqr.h the carver's state word is not consulted: a cancelled carver is read all the same.
 *   - It works on a root and on an attached carver, which is read through its root's map.
 *   - It works at every colour depth, channel count and image type: pixels are moved, never interpreted.
 *   - Sizes may come in any order and may repeat (each output is written).
 *   - A device output may start at any address that is a multiple of the SAMPLE size (1, 2, 4 or 8 bytes),
 *     as a slice of a tensor does; outputs must not overlap.  The call returns when they are written.
 *   - LQR_ERROR, and nothing is written, when r, sizes, the output array or one of its pointers is NULL,
 *     when n < 1, or when a size lies outside the range.
 *   - LQR_NOMEM when an allocation fails: the carver is as it was, nothing has leaked, no output has been
 *     written, and the same call made again gives the full result.
 */
#ifndef __LQR_SIZES_H__
#define __LQR_SIZES_H__

#include "lqr.h"

#ifdef __cplusplus
extern "C" {
#endif

gint lqrx_carver_size_range(LqrCarver *r, gint *min_size, gint *max_size);
LqrRetVal lqrx_carver_read_sizes_device(LqrCarver *r, const gint *sizes, gint n, void *const *device_out);
LqrRetVal lqrx_carver_read_sizes(LqrCarver *r, const gint *sizes, gint n, void *const *host_out);

#ifdef __cplusplus
}
#endif

#endif /* __LQR_SIZES_H__ */
