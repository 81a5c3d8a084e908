/*
 * lqr_clipforward.h -- forward-energy seams for a clip (Rubinstein, Shamir, Avidan 2008): ONE seam map from ALL frames of a clip, found
 * with forward energy.  lqr_static.h gives a clip one map, but finds it with liblqr's backward seams on a folded energy plane that is never
 * recomputed as seams leave: the carved frames do not shimmer, but the structure in them breaks.  lqr_forward.h gives forward seams, but
 * a map per frame: every frame finds seams of its own and the animation shimmers again.  This header is their combination: the forward
 * costs of every frame are folded into one set of costs, the costs are formed again where a seam has left, the map is built in device
 * memory and loaded from there into every frame, and no key carver is involved.  It adds calls on top of lqr.h and lqr_vmap.h and leaves
 * every other header as it is.  It lies in include_ext/, beside include/, whose list of headers is closed: compile with both on the
 * include path.
 *
 * The frames are n root carvers of one configuration, as lqr_static.h defines it (what lqrx_carver_resize_batch carves in lock-step: size,
 * colour depth, image type, energy function, bias or none, initialised or not -- all alike), 1 <= n <= 65535, all showing the same size.
 *
 * The rule.  There is no liblqr counterpart: tests/clipforward_cases.py holds the rule as a numpy model and the engine equals it bit for bit.
 * In the frame of the carving direction -- lines of length L (the width for orientation 0, the height for 1), x along a line, y across
 * the H lines -- and for the frames t = 0 .. n-1:
 *     I_t(x, y)   the I of lqr_forward.h: the (float) of the double frame t's energy function reads, for every colour depth and image type
 *     P_t(x, y)   the bias of frame t divided by L, a float division; 0 without a bias
 * Planes made once, which travel with their pixels when seams leave:
 *     T  = max_{t >= 1} |I_t - I_{t-1}|         float subtraction and absolute value; T = 0 for n = 1
 *     Pm = max_t P_t
 *     Q  = Pm + temporal * T                    the product rounded, then the sum; temporal: a finite float >= 0
 * For seam k = 1 .. depth, on the current frames of width wc = L - k + 1, with
 *     l_t = I_t(max(x-1,0), y)    r_t = I_t(min(x+1,wc-1), y)    u_t = I_t(x, y-1)
 * each cost is formed per frame as lqr_forward.h forms it, then the largest over the frames is taken:
 *     CU = max_t |r_t - l_t|     CL = max_t (|r_t - l_t| + |u_t - l_t|)     CR = max_t (|r_t - l_t| + |u_t - r_t|)
 *     M(x,0) = Q + CU
 *     M(x,y) = Q + min(M(x,y-1) + CU, M(x-1,y-1) + CL, M(x+1,y-1) + CR)             (parents outside the frame do not exist)
 * Every operation is a float operation rounded on its own, in the order written.  Ties: up, then left, then right.  The seam ends at the
 * smallest x with the least M(., H-1) and is walked up through the choices; its pixels get level k at the positions they had in the
 * image, and leave every frame, Q and the costs (what lay right of them moves one place left).  A maximum does not depend on the order it
 * is taken in, so the map is exact whatever the grouping of the frames.  For n = 1, and for identical frames, the map is lqr_forward.h's
 * for any temporal.  The result is ONE map as lqr_vmap_dump lays it out: width x height gints, row-major in IMAGE orientation, values
 * 0 .. depth, every level once in every line of the carving direction.  Pixel values that are not finite may give any seams, but the map
 * is always one that lqr_vmap_load accepts.  delta_x, the rigidity and the rigidity mask play no part.
 *
 * The map calls -- lqrx_clip_forward_map_device (into the caller's device memory, width x height gints, 4-byte aligned),
 * lqrx_clip_forward_map (a caller-owned LqrVMap, as lqr_vmap_dump's: lqr_vmap_destroy frees it; NULL on any failure):
 *   - The map is of the images the frames SHOW NOW, read whichever way the frames lie: no frame is transposed.
 *   - Frames that are not flat (they were resized, or hold a map) are flattened first, as lqr_vmap_load does it; otherwise every frame
 *     is left as it is.
 *
 * lqrx_clip_load_forward builds the map and loads it into all n frames and the carvers attached to them, without a trip through the
 * host: afterwards every frame is what lqrx_vmap_load_batch of that map leaves (lqr_vmap.h: depth, enl_step 2.0, orientation the map's --
 * frames that lay the other way have been transposed).  The map passes the same validation as any caller's.  Like
 * lqrx_carver_load_forward, and unlike lqr_vmap_load, it ALSO ACCEPTS INITIALISED frames: the warm start of lqr_vmap.h, item 5.
 *
 * lqrx_clip_resize_forward(frames, n, w1, h1, temporal) is lqrx_carver_resize_batch with the clip's forward seams: in the resize order
 * of frame 0, a direction whose size does not change is skipped; otherwise load_forward(|change|, that direction) and then
 * lqrx_carver_resize_batch to the new size, shrinking or enlarging.  A change of L or more in a direction is refused up front, before
 * any frame changes.
 *
 * Refused with LQR_ERROR (the map call: NULL), before any device work and with one line on stderr: NULL arguments; n < 1 or n > 65535;
 * an attached carver among the frames; frames that are not of one configuration; an orientation that is not 0 or 1; a temporal that is
 * negative, NaN or infinite; depth < 1 or depth >= L; L > 16384 (the engine's widest frame); more than 65535 lines.
 *
 * State, cancel, errors (all four calls), as in lqr_forward.h.  They enter the state word of every frame as a batch resize does
 * (lqr_control.h): a frame inside another call returns LQR_ERROR, one marked cancelled LQR_USRCANCEL.  The build is enqueued in slices
 * of 16 seams and lqr_carver_cancel on any frame, from another thread, is looked for between slices: the call returns LQR_USRCANCEL
 * with the frames' images, sizes and depths as they were.  Everything a build needs is allocated before its first launch: LQR_NOMEM
 * leaves the frames unchanged and has given every block back.  ONE EXCEPTION to "unchanged", for both: frames that were not flat are
 * flattened before the build starts and STAY FLATTENED -- they show the same image at the same size, but their depth is 0 and the seams
 * they held are gone, as after lqr_carver_flatten.  (Frames marked cancelled BEFORE the call are refused before that, and not
 * flattened.)  NO PROGRESS CALLBACKS fire during a build or its load; lqrx_clip_resize_forward's lqrx_carver_resize_batch fires them as
 * always.
 *
 * Cost.  One workgroup finds a seam for the whole clip, so one compute unit serves it whatever n is; the removal and the refresh of the
 * costs run on all of them.  A build holds one float per pixel and frame, and 23 bytes per pixel of the clip's own (27 with a bias).
 */
#ifndef __LQR_CLIPFORWARD_H__
#define __LQR_CLIPFORWARD_H__

#include "lqr.h"
#include "lqr_vmap.h"

#ifdef __cplusplus
extern "C" {
#endif

LqrRetVal lqrx_clip_forward_map_device(LqrCarver **frames, gint n, gint depth, gint orientation, gfloat temporal, gint *device_map);
LqrVMap *lqrx_clip_forward_map(LqrCarver **frames, gint n, gint depth, gint orientation, gfloat temporal);
LqrRetVal lqrx_clip_load_forward(LqrCarver **frames, gint n, gint depth, gint orientation, gfloat temporal);
LqrRetVal lqrx_clip_resize_forward(LqrCarver **frames, gint n, gint w1, gint h1, gfloat temporal);

#ifdef __cplusplus
}
#endif

#endif /* __LQR_CLIPFORWARD_H__ */
