/*
 * lqr_control.h -- the rest of liblqr-1's carver-control calls: lqr_carver_cancel, which stops a resize from a progress callback or
 * from another thread, and five small calls that finish the same part of liblqr's header.  A caller such as digiKam's content-aware
 * filter, which cancels from its UI thread while a worker sits in lqr_carver_resize, includes this header next to lqr.h.  lqr.h and
 * the other headers stay as they are; the plug-in needs none of this.
 *
 * The six prototypes and the three types are liblqr 0.4.1's, word for word (tests/golden/ref/abi.json).
 *
 * lqr_carver_cancel (tests/golden/control/ holds what the genuine code gave).
 *   - It may be called from ANY thread, at any time between lqr_carver_new and lqr_carver_destroy, and from inside a progress
 *     callback.  It reads and writes one atomic word of the carver and nothing else (host/lqr_state.h); it never waits and never
 *     touches the device.  It is the only call with that licence: every other call on a carver stays with one thread
 *     (INTEGRATION.md section 6).
 *   - While no call on the carver is running it changes nothing and returns LQR_OK; the next resize runs as usual.
 *   - While lqr_carver_resize, lqr_carver_flatten, an energy read-out or lqr_vmap_load runs on the carver, it marks the carver
 *     cancelled and returns LQR_OK.  The running call stops at its next check point and returns LQR_USRCANCEL: no further update
 *     event and no end event is fired.
 *   - On an attached carver it returns LQR_ERROR and touches nothing, as in liblqr: cancel the root.
 *   - A cancelled carver stays cancelled: every later lqr_carver_resize, lqr_carver_flatten, energy read-out and lqr_vmap_load
 *     returns LQR_USRCANCEL at once, as in liblqr, where only lqr_carver_destroy ends that.  The getters, the scans, lqr_vmap_dump
 *     and the masks' bookkeeping still serve.  Here lqrx_carver_cancel_clear makes the carver usable again.
 *
 * Where the engine does not follow liblqr: WHAT A CANCELLED CARVER HOLDS.  liblqr leaves the carver inside the visibility map it was
 * building: its width, its depth and its map are those of a half-built session, and its own BUGS file says the cancel signal
 * "scrambles up the internal state".  Here a cancelled session is rolled back like a failed one: nothing of it was committed, and
 * the carver holds, and serves, its state after the last COMPLETED session -- the first direction if the second was cancelled, the
 * first enlargement step if the second was, the image as it was if the first was.  After lqrx_carver_cancel_clear the same resize,
 * called again, gives bit for bit what it gives on a carver that was never cancelled.
 *
 * Check points and latency.  The word is looked at on entry to a call, before each direction that has something to carve, before each step of a direction,
 * before each flatten, transpose and inflate pass, before every seam is enqueued, and right after an update callback returns
 * (where the host has just synchronised: a cancel issued from the callback, or during it, is seen with nothing queued).  Once a
 * session's self-check has passed, the session commits and inflates to its end and the cancel is seen at the next check point.
 *   - A caller WITH an update callback is stopped within one report interval plus what was already enqueued.
 *   - A caller WITHOUT one has a whole session enqueued within milliseconds (the host runs ahead of the device); it is stopped at the
 *     session's end, before the next session.
 *
 * Batches (lqrx_carver_resize_batch).  A cancel on any member ends the call for the whole lock-step group with LQR_USRCANCEL; every
 * member is back at its state from before the session; only the member that was cancelled is marked cancelled.  No further sub-group
 * is started after a cancelled one, and a heterogeneous list stops at the first LQR_USRCANCEL.
 *
 * The five small calls.
 *   - lqr_carver_set_use_cache is accepted and has NO EFFECT: liblqr's cache is a plane of the brightness the energy reads, and the
 *     engine's read plane is that cache whatever the flag says.  Results are the same either way, in liblqr too.
 *   - lqr_carver_set_no_dump_vmaps undoes lqr_carver_set_dump_vmaps: later resizes append no maps; those already dumped stay.
 *   - lqr_carver_list_foreach calls func(carver, data) on every carver of the list in attach order and stops at the first return
 *     value that is not LQR_OK, which it returns.  lqr_carver_list_foreach_recursive is the same here: an attached carver has no
 *     attached carvers that the engine follows: they lie one level deep, so there is nothing deeper to visit.
 *   - lqr_carver_set_gradient_function is the 0.3-era spelling of lqr_carver_set_energy_function_builtin: LQR_GF_NORM, _SUMABS and
 *     _XABS select LQR_EF_GRAD_NORM, _SUMABS and _XABS; LQR_GF_NULL, and LQR_GF_NORM_BIAS and LQR_GF_YABS, which have no builtin
 *     energy left in 0.4, select LQR_EF_NULL -- exactly as the genuine code maps them.  Any other value is ignored.
 *
 * Extensions.  lqrx_carver_cancelled is 1 while the carver (or, for an attached carver, its root) is marked cancelled.
 * lqrx_carver_cancel_clear ends that state; it returns LQR_ERROR while a call on the carver is running (the cancelled call has not
 * returned yet) and on an attached carver, LQR_OK otherwise, also on a carver that was not cancelled.
 */
#ifndef __LQR_CONTROL_H__
#define __LQR_CONTROL_H__

#include "lqr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the token lqr_carver_list_foreach hands to its callback: one word, read as whichever member the caller wrote */
typedef union _LqrDataTok {
    LqrCarver *carver;
    gint integer;
    gpointer data;
} LqrDataTok;

typedef LqrRetVal (*LqrCarverFunc) (LqrCarver *carver, LqrDataTok data);

typedef enum _LqrGradFuncType {
    LQR_GF_NORM = 0,
    LQR_GF_NORM_BIAS = 1,
    LQR_GF_SUMABS = 2,
    LQR_GF_XABS = 3,
    LQR_GF_YABS = 4,
    LQR_GF_NULL = 5
} LqrGradFuncType;

LqrRetVal lqr_carver_cancel(LqrCarver *r);
void lqr_carver_set_use_cache(LqrCarver *r, gboolean use_cache);
void lqr_carver_set_no_dump_vmaps(LqrCarver *r);
LqrRetVal lqr_carver_list_foreach(LqrCarverList *list, LqrCarverFunc func, LqrDataTok data);
LqrRetVal lqr_carver_list_foreach_recursive(LqrCarverList *list, LqrCarverFunc func, LqrDataTok data);
void lqr_carver_set_gradient_function(LqrCarver *r, LqrGradFuncType gf_ind);

gint lqrx_carver_cancelled(LqrCarver *r);
LqrRetVal lqrx_carver_cancel_clear(LqrCarver *r);

#ifdef __cplusplus
}
#endif

#endif /* __LQR_CONTROL_H__ */
