/*
 * lqr_remove.h -- object removal: carve until the discard mask is gone (Avidan & Shamir 2007, section 4.6).
 *
 * The plug-in's auto-size button asks lqrx_guess_new_size how far to shrink: the longest count of mask pixels in a line.  That number is
 * only a LOWER BOUND on the seams an object needs -- a seam removes at most one marked pixel per line, and nothing forces it through a
 * marked pixel in every line -- so the picture delivered at the guessed size can still hold pieces of what the user painted out.
 * These two calls look at the carver itself: which marked pixels are still visible, and how deep the deepest of them lies.  They add
 * a scan on the device beside the seam loop and leave every other header and every other call as it is.  The header lies in
 * include_ext/, beside include/, whose list of headers is closed: compile with both on the include path.
 *
 * A pixel is MARKED when its bias -- the plane lqrx_carver_get_bias returns, before the division by the line length -- is below
 * -strength.  strength must be finite and >= 0; 0 means any negative bias.  The bias may come from any mask call: the rgb forms, the
 * gdouble forms, _xy (the queue is flushed first) or the device forms.  orientation is 0 for vertical seams (the width shrinks, the
 * lines are the image's rows), 1 for horizontal seams, the meaning it has in lqr_forward.h, or LQRX_ORIENTATION_AUTO.  A line has
 * length L (the width for orientation 0).  Any out pointer may be NULL.
 *
 * lqrx_carver_discard_scan is a PURE READ, like the read-outs of lqr_sizes.h: it consults no state word, does not flatten or transpose,
 * and leaves the scan-line cursor where it was.  *marked is the number of marked pixels visible at the carver's current size, *need the
 * largest such count in one line of the given orientation.  It is defined for a carver in any state -- flat, shrunk, regrown inside its
 * map, enlarged, lying transposed -- and returns what the same scan returns after lqr_carver_flatten.  With AUTO it reports the
 * orientation with the smaller need; a tie goes to 0.  A carver without a bias plane gives 0 and 0.  Refused with LQR_ERROR: a NULL or
 * attached carver (as the bias calls refuse it), an orientation outside -1, 0, 1, a bad strength.
 *
 * lqrx_carver_remove_discarded.  tests/remove_cases.py holds the rule as a numpy model over the carver API; run on the CPU oracle the
 * model gives what this call gives, bit for bit.
 *   1. Refused with LQR_ERROR, before any device work and with one line on stderr: a NULL, attached or uninitialised carver; an
 *      orientation outside -1, 0, 1; a bad strength; max_seams < 1; a line length L < 3 (with AUTO: of either orientation).  A carver
 *      marked cancelled before the call returns LQR_USRCANCEL and is not touched.
 *   2. The mask queue is flushed; a carver that is not flat is flattened, as lqrx_carver_load_forward does it.  With AUTO both orientations
 *      are scanned and one is picked as above; *orientation_used says which.
 *   3. The scan.  need == 0: LQR_OK with *seams = 0 and *left = 0; the carver is as step 2 left it.
 *   4. cap = min(max_seams, L - 2).  (At L - 1 seams the dumped map gives the last column a level too: "has no level" would no longer
 *      mean "still visible", and a line marked end to end cannot be emptied anyway.)
 *   5. While need > 0 and cur < cap: step = min(max(need, LQRX_REMOVE_MIN_STEP), cap - cur), cur += step; lqr_carver_resize to L0 - cur in
 *      that orientation, the other dimension unchanged; the scan again: need is the largest count in one line of marked pixels that have
 *      no level, deepest the largest level among marked pixels, in lqr_vmap_dump's numbering -- one pass on the device, 16 bytes to the
 *      host.  The state word is looked at before every round: a cancel returns LQR_USRCANCEL with the carver as the last completed round
 *      left it.  Progress callbacks fire as each round's lqr_carver_resize fires them.
 *   6. need == 0: fin = deepest; if fin < cur, lqr_carver_resize up to L0 - fin, which the map serves with no seam work -- so rounding a
 *      round up to LQRX_REMOVE_MIN_STEP seams costs at most 15 wasted seams; *seams = fin, *left = 0.  Otherwise the cap was reached:
 *      *seams = cur, *left = the marked pixels still visible, and the return is still LQR_OK.
 *   7. With restore set: lqr_carver_flatten, then lqr_carver_resize to the size the carver had at step 2 -- the plug-in's
 *      SCALEBACK_MODE_LQRBACK.  In both outcomes of step 6.
 *   8. LQR_NOMEM from any step leaves the carver in one of the states the sequence passes through; nothing leaks.  Attached carvers follow
 *      the root, as in any resize.
 *
 * THE ROUNDS AND THE RESULT.  A round costs a session set-up and a host round trip, and rounds of exactly `need` seams degenerate into
 * runs of one-seam sessions; hence at least LQRX_REMOVE_MIN_STEP seams a round.  With side-switch frequency 0 the round size never
 * changes the result, which also equals a single lqr_carver_resize to the final size.  With a switch frequency above 0 liblqr's switch
 * interval depends on the session's depth, and THE ROUNDS ARE PART OF THE RESULT: the model is the rule.
 */
#ifndef __LQR_REMOVE_H__
#define __LQR_REMOVE_H__

#include "lqr.h"

#ifdef __cplusplus
extern "C" {
#endif

#ifndef LQRX_REMOVE_MIN_STEP    /* (a library built with another value is a measuring aid: scripts/bench_remove.py) */
#define LQRX_REMOVE_MIN_STEP 16
#endif
#define LQRX_ORIENTATION_AUTO (-1)

LqrRetVal lqrx_carver_discard_scan(LqrCarver *r, gint orientation, gfloat strength, gint *marked, gint *need);
LqrRetVal lqrx_carver_remove_discarded(LqrCarver *r, gint orientation, gfloat strength, gint max_seams, gint restore, gint *orientation_used,
                                       gint *seams, gint *left);

#ifdef __cplusplus
}
#endif

#endif /* __LQR_REMOVE_H__ */
