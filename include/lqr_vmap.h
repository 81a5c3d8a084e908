/*
 * lqr_vmap.h -- the other half of liblqr-1's visibility-map API: a seam map that lqr_vmap_dump handed out (or
 * that the caller made) is loaded into a carver, which then resizes by that map with no energy, no DP and no
 * seam loop.  A video pipeline carves a key frame and replays its seams on the other frames; an editor keeps
 * the map next to the image and renders another size later.
 *
 * This header adds the calls on top of lqr.h with liblqr 0.4.1's prototypes, and leaves lqr.h and the other
 * headers as they are.
 *
 * A map is width x height gints, row-major in IMAGE orientation whatever its `orientation` is, as
 * lqr_vmap_dump hands it out: 0 for a pixel no seam crosses, k (1 .. depth) for a pixel of the k-th seam.
 * `orientation` 0: vertical seams (the width changes), one pixel of every seam in every ROW; 1: horizontal
 * seams (the height changes), one pixel of every seam in every COLUMN.
 *
 * Semantics (liblqr 0.4.1's; tests/golden/vmap/ holds what the genuine code gave).
 *   - lqr_vmap_new wraps a malloc'd buffer, which the map owns from then on (lqr_vmap_destroy frees it).
 *     Nothing is checked.
 *   - lqr_vmap_load on a carver that lqr_carver_init has seen returns LQR_ERROR and changes nothing.
 *   - On a carver of the map's size that has not been initialised it returns LQR_OK.  The map is copied: the
 *     LqrVMap may be destroyed right away.  Afterwards lqr_carver_get_depth is the map's depth,
 *     lqr_carver_get_enl_step is 2.0 (the load sets it), lqr_carver_get_orientation is the map's (a carver
 *     that lay the other way has been transposed), and the size and the reference size are unchanged.
 *   - lqr_carver_resize then serves every size from (length - depth) to (length + depth) in the map's
 *     direction, in any order and back again, and each result is byte for byte what the carver that made the
 *     map gives at that size.  Enlarging inserts, before each pixel of seams 1 .. k, the average of that
 *     pixel and its left neighbour.  lqr_vmap_dump of the loaded carver gives the loaded map back.
 *   - Attached carvers follow: the load lays them out with their root and they follow its resizes.
 *   - lqr_carver_init after a load succeeds; the sizes the map covers are served as before, another
 *     lqr_vmap_load is refused (the carver is initialised now), and a resize below (length - depth) returns
 *     LQR_OK with a depth that has grown (a map of 10 seams, resized to 15 less, has depth 15; but see 5).
 *   - lqr_vmap_internal_dump appends the carver's map as it stands to the carver's own list
 *     (lqr_vmap_list_start), as every resize does under lqr_carver_set_dump_vmaps.
 *   - The map need not hold connected seams: any map in which every line holds every level once is served
 *     (tests/vmap_cases.py has the rule as a numpy model, checked against the genuine code).
 *
 * Where the engine does not follow liblqr:
 *   1. THE MAP IS VALIDATED, on the device, before anything changes: 0 < depth < line length (the width for
 *      orientation 0, the height for 1), every value in [0, depth], and every level 1 .. depth exactly once in
 *      every line of the carving direction.  Otherwise the call returns LQR_ERROR, says why in one line on
 *      stderr, and the carver is untouched -- not flattened, not transposed, enl_step as it was.  liblqr does
 *      not look at the contents at all and reads and writes out of bounds later.  Connected seams are NOT
 *      required.
 *   2. THE SIZE IS CHECKED AGAINST WHAT THE CARVER SHOWS NOW.  A carver that was resized since its last load
 *      is flattened first, as in liblqr, and the load is accepted only if that flattened size is the map's.
 *      liblqr compares with the size before the flattening: a second load onto a carver resized from 40 to 50
 *      columns takes the 40-column map for a 50-column image and returns LQR_OK with garbage.  Here that is
 *      LQR_ERROR and the carver is unchanged.
 *   3. A RESIZE THE CARVER CANNOT SERVE IS REFUSED UP FRONT.  A carver that is not initialised cannot build
 *      maps: a size beyond the loaded range, or any change in the other direction, returns LQR_ERROR before
 *      anything is touched, and the carver still serves every size in range afterwards.  liblqr carries out
 *      what it can (in a two-direction request the first direction, then a transposition), fails, and from then
 *      on refuses every resize of that carver, also sizes that had worked.
 *   4. A carver that is itself attached to another returns LQR_ERROR: its planes follow its root's.
 *   5. lqr_carver_init AFTER A LOAD, THEN A DEEPER RESIZE, IS A WARM START.  The further seams are found on the
 *      frame the loaded map leaves visible and stacked on top of its seams: the result is what the carver that
 *      made the map gives when it is carved on to that size.  liblqr returns the same values, but its
 *      lqr_carver_init lays the frame out as the first columns of the inflated layout instead of the visible
 *      pixels; it finds the further seams there, writes their levels over others, and the map it dumps
 *      afterwards holds levels twice and lacks others (tests/golden/vmap/, init_after_load_h and _v).
 *      "What the carver that made the map gives" holds for what a map carries.  Two things it does not carry: which side
 *      wins ties (it survives flattening and changes at every side switch; a new carver starts on the left), and the
 *      rigidity table, which liblqr rescales at every transposition and a new carver computes afresh.  With side-switch
 *      frequency 0 and rigidity 0 the new carver continues exactly as the old one (tests/sequence_cases.py, "reopen").
 *   6. A map dumped from a carver that was carved down to ONE column carries liblqr's finish_vsmap mark, a
 *      level above the depth in the column that is left.  The mark means what 0 means at every size the map
 *      covers; item 1 refuses it as any value above depth.  Clear it (set it to 0) before loading such a map.
 * LQR_NOMEM leaves the carver usable, in one of the states the load passes through: as it was, flattened, or
 * flattened and transposed.
 *
 * Extensions.  lqrx_vmap_load_device is lqr_vmap_load of a map that lies in DEVICE memory (width x height
 * 32-bit ints, 4-byte aligned), e.g. one a model produced: it is read where it lies, never copied to the host,
 * and may be reused once the call has returned.  lqrx_vmap_load_batch loads ONE map into n root carvers of its
 * size and of one configuration (what lqrx_carver_resize_batch carves in lock-step): the map is brought to the
 * device and validated once, and every carver reads its levels from that one plane.  Either all n carvers are
 * loaded or, on LQR_ERROR, none has changed; lqrx_carver_resize_batch then resizes them together.
 */
#ifndef __LQR_VMAP_H__
#define __LQR_VMAP_H__

#include "lqr.h"

#ifdef __cplusplus
extern "C" {
#endif

LqrVMap *lqr_vmap_new(gint *buffer, gint width, gint height, gint depth, gint orientation);
LqrRetVal lqr_vmap_load(LqrCarver *r, LqrVMap *vmap);
LqrRetVal lqr_vmap_internal_dump(LqrCarver *r);

LqrRetVal lqrx_vmap_load_device(LqrCarver *r, const gint *device_map, gint width, gint height, gint depth, gint orientation);
LqrRetVal lqrx_vmap_load_batch(LqrCarver **carvers, gint n, LqrVMap *vmap);

#ifdef __cplusplus
}
#endif

#endif /* __LQR_VMAP_H__ */
