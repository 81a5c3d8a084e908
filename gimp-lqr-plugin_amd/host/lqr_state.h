/*
 * lqr_state.h -- liblqr's carver state (LqrCarverState: idle, resizing, inflating, transposing, flattening, cancelled) as ONE atomic
 * word per root carver, and the only thing in the engine a second thread may touch: lqr_carver_cancel (include/lqr_control.h) is
 * lqr_state_cancel on that word and nothing else.  Plain C on the GCC __atomic builtins: no device call, no I/O, no allocation, so
 * that tests/test_state.py compiles it alone, under AddressSanitizer and under ThreadSanitizer.
 *
 * The word holds the state in its low byte and LQR_STATE_IN_CALL while a call on the carver runs:
 *     enter    idle -> busy state, in a call.  Refused on a cancelled word (the call returns LQR_USRCANCEL) and on one in a call.
 *     phase    inside a call: another busy state (transposing, flattening, inflating, back to resizing).  A cancelled word stays.
 *     leave    the call is over: the word is idle again -- unless it is cancelled, which leaving never overwrites.
 *     cancel   busy and in a call -> cancelled.  On an idle word (no call is running) it changes nothing, as in liblqr.
 *     check    is it cancelled?  One relaxed load: what the seam loop does per seam.
 *     clear    cancelled and not in a call -> idle (lqrx_carver_cancel_clear).  Refused while a call runs.
 * A cancel that found a call running is seen by every later check, until clear: nothing between the two erases it.
 */
#ifndef LQR_STATE_H
#define LQR_STATE_H

#ifdef __cplusplus
extern "C" {
#endif

/* liblqr's LqrCarverState, value for value */
enum {
    LQR_STATE_STD = 0,
    LQR_STATE_RESIZING = 1,
    LQR_STATE_INFLATING = 2,
    LQR_STATE_TRANSPOSING = 3,
    LQR_STATE_FLATTENING = 4,
    LQR_STATE_CANCELLED = 5
};
#define LQR_STATE_MASK 0xff
#define LQR_STATE_IN_CALL 0x100

typedef struct { int word; } LqrState;

/* what lqr_state_enter says */
enum { LQR_STATE_ENTERED = 1, LQR_STATE_IS_CANCELLED = 0, LQR_STATE_IS_BUSY = -1 };

void lqr_state_init(LqrState *s);
int lqr_state_enter(LqrState *s, int busy);     /* LQR_STATE_ENTERED, or the word is as it was */
int lqr_state_phase(LqrState *s, int busy);     /* 1: the word holds `busy` now; 0: it is cancelled and stays so */
void lqr_state_leave(LqrState *s);
int lqr_state_cancel(LqrState *s);              /* 1: a call was running and the word is cancelled now; 0: nothing changed */
int lqr_state_check(const LqrState *s);         /* 1: cancelled */
int lqr_state_clear(LqrState *s);               /* 1: idle now; 0: a call is running, nothing changed */
int lqr_state_get(const LqrState *s);           /* the state (low byte) */
int lqr_state_in_call(const LqrState *s);
/* whose word a carver's calls look at: an attached carver has none of its own in use, it reads its root's */
LqrState *lqr_state_word(LqrState *own, LqrState *root_or_null);

#ifdef __cplusplus
}
#endif

#endif /* LQR_STATE_H */
