/*
 * lqr_static.h -- static seams for video (Rubinstein, Shamir, Avidan 2008, section 3): ONE seam map made from ALL frames of a clip.
 * Carving an animation frame by frame lets every frame find seams of its own, and the result shimmers; replaying the seams of a key
 * frame (lqrx_vmap_load_batch) cuts straight through whatever moves into their path a few frames later.  The cheap standard answer
 * folds the clip into one energy plane -- for each pixel the largest spatial energy over time and the largest change between
 * neighbouring frames --, finds seams on that plane, and applies them to every frame.
 *
 * The fold is one streaming pass over the n images in device memory (csrc/k_static.hip).  The seam finder is the one the engine has:
 * an LQR_EF_NULL carver that carries the plane as its bias is exactly "carve on a given energy that travels with the pixels".  The map
 * it builds is loaded into the frames like any other (lqr_vmap.h), and lqrx_carver_resize_batch / lqrx_carver_read_sizes serve the
 * sizes.  This header adds calls on top of lqr.h and lqr_vmap.h and leaves every other header as it is.  It lies in include_ext/,
 * beside include/, whose list of headers is closed: compile with both on the include path.
 *
 * The frames are n root carvers of one configuration (what lqrx_carver_resize_batch carves in lock-step: size, colour depth, image
 * type, energy function, bias or none, initialised or not -- all alike), 1 <= n <= 65535, all showing width x height pixels.
 *
 * The rule.  There is no liblqr counterpart: tests/static_cases.py holds the rule as a numpy model and the engine equals it bit for bit.
 * In IMAGE orientation, for frame t:
 *     S_t(x, y)   what lqr_carver_get_true_energy(frame t, ., orientation) stores for the pixel: the frame's own builtin energy
 *                 function, bias / L included (L: the width for orientation 0, the height for 1), with this engine's conventions at
 *                 the borders and in frames one pixel wide (lqr_energy.h)
 *     I_t(x, y)   the (float) of the double the frame's energy function reads (the I of lqr_forward.h)
 *     S = max_t S_t
 *     T = max_{t >= 1} |I_t - I_{t-1}|        subtraction and absolute value in float; T = 0 for n = 1
 *     E = alpha * S + (1 - alpha) * T         four float operations, each rounded on its own: the two products, 1 - alpha, the sum
 * alpha lies in [0, 1]; the paper uses 0.3.  A maximum does not depend on the order it is taken in, so E is exact whatever the
 * grouping of the frames.  Values that are not finite: unspecified.
 *
 * lqrx_carvers_static_energy_device writes E, width x height floats row-major in IMAGE orientation, to the caller's device memory
 * (4-byte aligned; nothing past the plane is written), lqrx_carvers_static_energy to host memory.
 *   - E is of the images the frames SHOW NOW, read whichever way the frames lie: no frame is transposed, no working plane is
 *     allocated, and apart from the next item every frame is left exactly as it was.
 *   - Frames that are not flat (they were resized, or hold a map) are flattened first, as lqr_vmap_load does it.
 *
 * lqrx_carvers_static_map returns the seam map of the clip, a caller-owned LqrVMap as lqr_vmap_dump's (lqr_vmap_destroy frees it; NULL
 * on any failure): `depth` seams of `orientation` found on E with liblqr's own seams, pinned against the genuine liblqr call by call:
 *     lqr_carver_new on a width x height 8-bit one-channel image of zeros;  lqr_carver_set_energy_function_builtin(LQR_EF_NULL);
 *     lqrx_carver_bias_add_area_device(E, LQR_COLDEPTH_32F, bias_factor 2, width, height, 0, 0)     (factor 2: the bias plane IS E,
 *     the seam loop sees E / L);  lqr_carver_init(delta_x, rigidity);  lqr_carver_resize by `depth` seams;  lqr_vmap_dump.
 * That key carver is internal to the call and destroyed before it returns, on every path.
 *
 * lqrx_carvers_load_static builds the map and loads it into all n frames and the carvers attached to them: afterwards every frame is
 * what lqrx_vmap_load_batch of that map leaves (lqr_vmap.h: depth, enl_step 2.0, orientation the map's -- frames that lay the other
 * way have been transposed).  Like lqrx_carver_load_forward, and unlike lqr_vmap_load, it ALSO ACCEPTS INITIALISED frames.  The map
 * passes from the key carver to the frames through host memory (profiles/static/ says what that costs).
 *
 * lqrx_carvers_resize_static(frames, n, w1, h1, ...) is lqrx_carver_resize_batch with static seams: in the resize order of frame 0, a
 * direction whose size does not change is skipped; otherwise load_static(|change|, that direction) and then lqrx_carver_resize_batch
 * to the new size, shrinking or enlarging.  A change of L or more in a direction is refused up front, before any frame changes.
 *
 * Refused with LQR_ERROR (the map call: NULL), before any device work and with one line on stderr: NULL arguments; n < 1 or n > 65535;
 * an attached carver among the frames; frames that are not of one configuration; an orientation that is not 0 or 1; alpha outside
 * [0, 1] or NaN; for the map, load and resize calls depth < 1, depth >= L, L > 16384 (the engine's widest frame), delta_x < 0 or
 * delta_x > 16 (what lqr_carver_init of the key carver takes).  The energy calls have no limit on L.
 *
 * State, cancel, errors (all five calls).  They enter the state word of every frame as a batch resize does (lqr_control.h): a frame
 * inside another call returns LQR_ERROR, one marked cancelled LQR_USRCANCEL.  lqr_carver_cancel on any frame, from another thread, is
 * looked for before the flatten, before every launch of the fold (one per 16 frames) and before the key carver's resize: the call
 * returns LQR_USRCANCEL with the frames' images, sizes and depths as they were.  THE KEY CARVER'S OWN RESIZE IS NOT INTERRUPTED: a
 * cancel that arrives during it is seen when it has finished, before anything is loaded.  Everything the fold needs is allocated
 * before its first launch: LQR_NOMEM, from the fold or from the key carver, leaves the frames unchanged and has given every block back.  ONE EXCEPTION
 * to "unchanged", for both: frames that were not flat are flattened first and STAY FLATTENED -- they show the same image at the same
 * size, but their depth is 0 and the seams they held are gone, as after lqr_carver_flatten.  (Frames marked cancelled BEFORE the call
 * are refused before that, and not flattened.)  NO PROGRESS CALLBACKS fire during the fold, the key carver's resize or the load;
 * lqrx_carvers_resize_static's lqrx_carver_resize_batch fires them as always.
 *
 * Cost.  The fold reads every frame pixel once and the running planes once per 16 frames; profiles/static/ has the measured figures.
 */
#ifndef __LQR_STATIC_H__
#define __LQR_STATIC_H__

#include "lqr.h"
#include "lqr_vmap.h"

#ifdef __cplusplus
extern "C" {
#endif

LqrRetVal lqrx_carvers_static_energy_device(LqrCarver **frames, gint n, gint orientation, gfloat alpha, gfloat *device_energy);
LqrRetVal lqrx_carvers_static_energy(LqrCarver **frames, gint n, gint orientation, gfloat alpha, gfloat *energy);
LqrVMap *lqrx_carvers_static_map(LqrCarver **frames, gint n, gint depth, gint orientation, gfloat alpha, gint delta_x, gfloat rigidity);
LqrRetVal lqrx_carvers_load_static(LqrCarver **frames, gint n, gint depth, gint orientation, gfloat alpha, gint delta_x, gfloat rigidity);
LqrRetVal lqrx_carvers_resize_static(LqrCarver **frames, gint n, gint w1, gint h1, gfloat alpha, gint delta_x, gfloat rigidity);

#ifdef __cplusplus
}
#endif

#endif /* __LQR_STATIC_H__ */
