/* lqr_state.c -- the carver's state word (lqr_state.h): every transition is one compare-and-swap loop on one int */
#include "lqr_state.h"

static int is_busy(int state) { return state >= LQR_STATE_RESIZING && state <= LQR_STATE_FLATTENING; }

void lqr_state_init(LqrState *s) { __atomic_store_n(&s->word, LQR_STATE_STD, __ATOMIC_RELEASE); }

int lqr_state_enter(LqrState *s, int busy)
{
    int cur = __atomic_load_n(&s->word, __ATOMIC_ACQUIRE);
    if (!is_busy(busy)) return LQR_STATE_IS_BUSY;
    for (;;) {
        if ((cur & LQR_STATE_MASK) == LQR_STATE_CANCELLED) return LQR_STATE_IS_CANCELLED;
        if (cur & LQR_STATE_IN_CALL) return LQR_STATE_IS_BUSY;
        if (__atomic_compare_exchange_n(&s->word, &cur, busy | LQR_STATE_IN_CALL, 0, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE)) return LQR_STATE_ENTERED;
    }
}

int lqr_state_phase(LqrState *s, int busy)
{
    int cur = __atomic_load_n(&s->word, __ATOMIC_ACQUIRE);
    if (!is_busy(busy)) return 0;
    for (;;) {
        if ((cur & LQR_STATE_MASK) == LQR_STATE_CANCELLED) return 0;
        if (__atomic_compare_exchange_n(&s->word, &cur, busy | (cur & LQR_STATE_IN_CALL), 0, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE)) return 1;
    }
}

void lqr_state_leave(LqrState *s)
{
    int cur = __atomic_load_n(&s->word, __ATOMIC_ACQUIRE);
    for (;;) {
        const int next = (cur & LQR_STATE_MASK) == LQR_STATE_CANCELLED ? LQR_STATE_CANCELLED : LQR_STATE_STD;
        if (__atomic_compare_exchange_n(&s->word, &cur, next, 0, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE)) return;
    }
}

int lqr_state_cancel(LqrState *s)
{
    int cur = __atomic_load_n(&s->word, __ATOMIC_ACQUIRE);
    for (;;) {
        if (!(cur & LQR_STATE_IN_CALL) || !is_busy(cur & LQR_STATE_MASK)) return 0;
        if (__atomic_compare_exchange_n(&s->word, &cur, LQR_STATE_CANCELLED | LQR_STATE_IN_CALL, 0, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE)) return 1;
    }
}

int lqr_state_check(const LqrState *s) { return (__atomic_load_n(&s->word, __ATOMIC_RELAXED) & LQR_STATE_MASK) == LQR_STATE_CANCELLED; }

int lqr_state_clear(LqrState *s)
{
    int cur = __atomic_load_n(&s->word, __ATOMIC_ACQUIRE);
    for (;;) {
        if (cur & LQR_STATE_IN_CALL) return 0;
        if (cur == LQR_STATE_STD) return 1;
        if (__atomic_compare_exchange_n(&s->word, &cur, LQR_STATE_STD, 0, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE)) return 1;
    }
}

int lqr_state_get(const LqrState *s) { return __atomic_load_n(&s->word, __ATOMIC_ACQUIRE) & LQR_STATE_MASK; }
int lqr_state_in_call(const LqrState *s) { return (__atomic_load_n(&s->word, __ATOMIC_ACQUIRE) & LQR_STATE_IN_CALL) != 0; }
LqrState *lqr_state_word(LqrState *own, LqrState *root_or_null) { return root_or_null ? root_or_null : own; }
