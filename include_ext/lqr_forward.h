/*
 * lqr_forward.h -- forward-energy seams (Rubinstein, Shamir, Avidan 2008), the one thing a user of a seam-carving library asks for
 * that liblqr never had.  liblqr removes the seam that CARRIES the least gradient; forward energy removes the seam whose removal
 * INSERTS the least: the new neighbours it creates are what is charged.  That is what keeps edges of structured images from breaking.
 *
 * The engine separates finding seams from applying them (lqr_vmap.h): a carver that was given a seam map serves every size the map
 * covers -- shrinking, enlarging, attached carvers, lqr_vmap_dump, lqrx_carver_read_sizes -- with no DP at all.  So the forward seam
 * finder WRITES A SEAM MAP, on the device, and the map is loaded like any other.  The incremental seam loop of lqr_carver_resize is not
 * involved and behaves as before.  This header adds calls on top of lqr.h and lqr_vmap.h and leaves every other header as it is.
 * It lies in include_ext/, beside include/, whose list of headers is closed: compile with both on the include path.
 *
 * The rule.  There is no liblqr counterpart: tests/forward_cases.py holds the rule as a numpy model and the engine equals it bit for bit.
 * In the frame of the carving direction -- lines of length L (the width for orientation 0, the height for 1), x along a line, y across
 * the H lines -- I(x, y) is the (float) of the double the carver's energy function reads (brightness, or luma for the LUMA_* builtins,
 * for every colour depth and image type), P(x, y) the bias term bias / L as a float division (0 without a bias).  delta_x, the rigidity
 * and the rigidity mask play no part.  For seam k = 1 .. depth, on the current frame of width wc = L - k + 1:
 *     l = I(max(x-1,0), y)    r = I(min(x+1,wc-1), y)    u = I(x, y-1)
 *     CU = |r - l|     CL = CU + |u - l|     CR = CU + |u - r|
 *     M(x,0) = P(x,0) + CU
 *     M(x,y) = P(x,y) + min(M(x,y-1) + CU, M(x-1,y-1) + CL, M(x+1,y-1) + CR)        (parents outside the frame do not exist)
 * Every operation is a float operation rounded on its own, in the order written.  Ties: up, then left, then right.  The seam ends at the
 * smallest x with the least M(., H-1) and is walked up through the choices; its pixels get level k at the positions they had in the
 * image, and leave I and P (what lay right of them moves one place left).  The result is a map as lqr_vmap_dump lays it out: width x
 * height gints, row-major in IMAGE orientation, values 0 .. depth, every level once in every line of the carving direction.
 * Pixel values that are not finite may give any seams, but the map is always one that lqr_vmap_load accepts.
 *
 * The map calls -- lqrx_carver_forward_map_device (into the caller's device memory, width x height gints, 4-byte aligned),
 * lqrx_carver_forward_map (a caller-owned LqrVMap, as lqr_vmap_dump's: lqr_vmap_destroy frees it; NULL on any failure),
 * lqrx_carver_forward_maps_device (n carvers that lqrx_carver_resize_batch would carve in lock-step, one launch sequence for all) --
 * take root carvers, initialised or not (a carver must be initialised to have a rigidity mask; a bias it can have either way).
 *   - The map is of the image the carver SHOWS NOW, read whichever way the carver lies: the carver is not transposed.
 *   - A carver that is not flat (it was resized, or holds a map) is flattened first, as lqr_vmap_load does it; otherwise the
 *     carver is left as it is.
 *   - Refused with LQR_ERROR, before any device work and with one line on stderr: an attached carver; depth < 1 or depth >= L;
 *     L > 16384 (the engine's widest frame); more than 65535 lines, or more than 65535 carvers in a batch (what one launch of the
 *     build takes); NULL arguments; for the batch form, carvers of different configuration.
 *
 * lqrx_carver_load_forward builds the map and loads it in place, without a trip through the host: afterwards the carver is what
 * lqrx_vmap_load_device of that map leaves (lqr_vmap.h: depth, enl_step 2.0, orientation the map's -- a carver that lay the other
 * way has been transposed --, attached carvers laid out with it).  The map passes the same validation as any caller's.  Unlike
 * lqr_vmap_load it ALSO ACCEPTS AN INITIALISED CARVER.  That state is the one lqr_vmap.h, item 5, describes (lqr_carver_init after a
 * load): the sizes the map covers are served from the map, and a later lqr_carver_resize beyond them continues with liblqr's backward
 * seams, found on the frame the forward seams leave and stacked on top of them -- a warm start.  (The tie side and the rigidity
 * table are the carver's own, as they stand: lqr_vmap.h item 5 says what that means for a comparison with a new carver.)
 *
 * lqrx_carver_resize_forward(r, w1, h1) is lqr_carver_resize with forward seams: in the carver's resize order, a direction whose size
 * does not change is skipped; otherwise load_forward(|change|, that direction) and then lqr_carver_resize to the new size, shrinking
 * or enlarging (an enlargement inserts, as with every loaded map, the average of a seam's pixel and its left neighbour).  A change of
 * L or more in a direction -- no frame has that many seams -- is refused up front with LQR_ERROR, before the carver changes in either
 * direction.
 *
 * State, cancel, errors (all five calls).  They enter the carver's state word as a resize does (lqr_control.h): a carver inside another
 * call returns LQR_ERROR, one marked cancelled LQR_USRCANCEL.  The build is enqueued in slices of 16 seams and lqr_carver_cancel,
 * from another thread, is looked for between slices: the call returns LQR_USRCANCEL with the carver's image, size and depth as they
 * were.  Everything a build needs is allocated before its first launch: LQR_NOMEM leaves the carver unchanged and has given every
 * block back.  ONE EXCEPTION to "unchanged", for both: a carver that was not flat is flattened before the build starts, and STAYS
 * FLATTENED -- it shows the same image at the same size, but its depth is 0 and the seams it held are gone, as after lqr_carver_flatten.
 * (A carver marked cancelled BEFORE the call is refused before that, and is not flattened.)  NO PROGRESS CALLBACKS fire during a build; lqrx_carver_resize_forward's
 * lqr_carver_resize fires them as always (it has nothing left to build, so: init and end).
 *
 * Cost.  One workgroup per image finds a seam: a single image builds slower than the tiled backward path carves it, a
 * batch of 64 keeps 64 compute units busy.  profiles/forward/ has the measured figures.
 */
#ifndef __LQR_FORWARD_H__
#define __LQR_FORWARD_H__

#include "lqr.h"
#include "lqr_vmap.h"

#ifdef __cplusplus
extern "C" {
#endif

LqrRetVal lqrx_carver_forward_map_device(LqrCarver *r, gint depth, gint orientation, gint *device_map);
LqrVMap *lqrx_carver_forward_map(LqrCarver *r, gint depth, gint orientation);
LqrRetVal lqrx_carver_forward_maps_device(LqrCarver **carvers, gint n, gint depth, gint orientation, gint *const *device_maps);
LqrRetVal lqrx_carver_load_forward(LqrCarver *r, gint depth, gint orientation);
LqrRetVal lqrx_carver_resize_forward(LqrCarver *r, gint w1, gint h1);

#ifdef __cplusplus
}
#endif

#endif /* __LQR_FORWARD_H__ */
