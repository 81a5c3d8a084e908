/* The carver's state word (gimp-lqr-plugin_amd/host/lqr_state.c) alone, for tests/test_state.py.
 *   state_main transitions     every operation on every value of the word, and whose word an attached carver reads
 *                              (built with -fsanitize=address,undefined)
 *   state_main race N          N calls on one thread while a second thread cancels at arbitrary moments
 *                              (built with -fsanitize=thread)
 */
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lqr_state.h"

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "state_main: line %d: %s\n", __LINE__, #cond); exit(1); } } while (0)

static const int busy_states[4] = {LQR_STATE_RESIZING, LQR_STATE_INFLATING, LQR_STATE_TRANSPOSING, LQR_STATE_FLATTENING};

static int transitions(void)
{
    LqrState s, root, aux[3];
    int i, j, n = 0;
    lqr_state_init(&s);
    CHECK(lqr_state_get(&s) == LQR_STATE_STD && !lqr_state_in_call(&s) && !lqr_state_check(&s));
    /* idle: a cancel changes nothing, a clear has nothing to do, leaving is harmless */
    CHECK(lqr_state_cancel(&s) == 0 && s.word == LQR_STATE_STD);
    CHECK(lqr_state_clear(&s) == 1 && s.word == LQR_STATE_STD);
    lqr_state_leave(&s);
    CHECK(s.word == LQR_STATE_STD);
    CHECK(lqr_state_enter(&s, LQR_STATE_STD) == LQR_STATE_IS_BUSY && lqr_state_enter(&s, LQR_STATE_CANCELLED) == LQR_STATE_IS_BUSY && s.word == LQR_STATE_STD);
    for (i = 0; i < 4; i++) {
        /* enter, every phase, leave */
        CHECK(lqr_state_enter(&s, busy_states[i]) == LQR_STATE_ENTERED);
        CHECK(lqr_state_get(&s) == busy_states[i] && lqr_state_in_call(&s) && !lqr_state_check(&s));
        CHECK(lqr_state_enter(&s, busy_states[i]) == LQR_STATE_IS_BUSY);           /* no call inside a call */
        CHECK(lqr_state_clear(&s) == 0);                                           /* not while a call runs */
        for (j = 0; j < 4; j++) { CHECK(lqr_state_phase(&s, busy_states[j]) == 1 && lqr_state_get(&s) == busy_states[j] && lqr_state_in_call(&s)); n++; }
        CHECK(lqr_state_phase(&s, LQR_STATE_STD) == 0 && lqr_state_phase(&s, LQR_STATE_CANCELLED) == 0 && lqr_state_get(&s) == busy_states[3]);
        lqr_state_leave(&s);
        CHECK(s.word == LQR_STATE_STD);
        /* cancel from every busy state: seen by every check until clear; phases and leaving never erase it */
        for (j = 0; j < 4; j++) {
            CHECK(lqr_state_enter(&s, busy_states[i]) == LQR_STATE_ENTERED && lqr_state_phase(&s, busy_states[j]) == 1);
            CHECK(lqr_state_cancel(&s) == 1 && lqr_state_check(&s) && lqr_state_in_call(&s));
            CHECK(lqr_state_cancel(&s) == 0 && lqr_state_check(&s));               /* a second one finds nothing busy */
            CHECK(lqr_state_phase(&s, busy_states[(j + 1) & 3]) == 0 && lqr_state_check(&s));
            CHECK(lqr_state_clear(&s) == 0 && lqr_state_check(&s));                /* the cancelled call has not returned yet */
            lqr_state_leave(&s);
            CHECK(lqr_state_check(&s) && !lqr_state_in_call(&s) && s.word == LQR_STATE_CANCELLED);
            CHECK(lqr_state_enter(&s, busy_states[i]) == LQR_STATE_IS_CANCELLED && s.word == LQR_STATE_CANCELLED);
            CHECK(lqr_state_cancel(&s) == 0 && s.word == LQR_STATE_CANCELLED);
            lqr_state_leave(&s);
            CHECK(s.word == LQR_STATE_CANCELLED);
            CHECK(lqr_state_clear(&s) == 1 && s.word == LQR_STATE_STD && !lqr_state_check(&s));
            n++;
        }
    }
    /* attached carvers: their calls look at the root's word, their own is never touched */
    lqr_state_init(&root);
    for (i = 0; i < 3; i++) { lqr_state_init(&aux[i]); CHECK(lqr_state_word(&aux[i], &root) == &root); }
    CHECK(lqr_state_word(&root, NULL) == &root);
    CHECK(lqr_state_enter(&root, LQR_STATE_RESIZING) == LQR_STATE_ENTERED && lqr_state_cancel(lqr_state_word(&root, NULL)) == 1);
    for (i = 0; i < 3; i++) CHECK(lqr_state_check(lqr_state_word(&aux[i], &root)) == 1 && aux[i].word == LQR_STATE_STD);
    lqr_state_leave(&root);
    for (i = 0; i < 3; i++) CHECK(lqr_state_check(lqr_state_word(&aux[i], &root)) == 1);
    CHECK(lqr_state_clear(&root) == 1);
    for (i = 0; i < 3; i++) CHECK(lqr_state_check(lqr_state_word(&aux[i], &root)) == 0);
    printf("state transitions ok %d\n", n);
    return 0;
}

/* ---- two threads ---- */
static LqrState g_state;
static long g_hits, g_idle, g_stop;          /* cancels that found a call running / found none (atomics) */

static void *canceller(void *arg)
{
    unsigned x = 12345;
    (void) arg;
    while (!__atomic_load_n(&g_stop, __ATOMIC_ACQUIRE)) {
        int k, spin;
        if (lqr_state_cancel(&g_state)) __atomic_add_fetch(&g_hits, 1, __ATOMIC_ACQ_REL);
        else __atomic_add_fetch(&g_idle, 1, __ATOMIC_ACQ_REL);
        x = x * 1664525u + 1013904223u;         /* an arbitrary moment: 0 .. 255 empty turns */
        spin = (int) (x >> 24);
        for (k = 0; k < spin; k++) __atomic_load_n(&g_stop, __ATOMIC_RELAXED);
    }
    return NULL;
}

static int race(long n)
{
    pthread_t t;
    long i, seen = 0, seen_in_call = 0;
    lqr_state_init(&g_state);
    CHECK(pthread_create(&t, NULL, canceller, NULL) == 0);
    for (i = 0; i < n; i++) {
        int j, in_call = 0;
        /* the word is idle here (cleared below): whatever the other thread did since changed nothing */
        CHECK(lqr_state_enter(&g_state, busy_states[i & 3]) == LQR_STATE_ENTERED);
        for (j = 0; j < 8 && !in_call; j++) {           /* the seam loop: check, go on */
            if (lqr_state_check(&g_state)) { in_call = 1; break; }
            (void) lqr_state_phase(&g_state, busy_states[(i + j) & 3]);
        }
        if (in_call) {
            CHECK(lqr_state_clear(&g_state) == 0);          /* a call is running */
            CHECK(lqr_state_phase(&g_state, LQR_STATE_INFLATING) == 0);
        }
        lqr_state_leave(&g_state);                      /* never erases a cancel */
        if (in_call) CHECK(lqr_state_check(&g_state));
        if (lqr_state_check(&g_state)) {
            /* exactly one cancel found this call running, and it is seen here at the latest */
            seen++; seen_in_call += in_call;
            CHECK(lqr_state_enter(&g_state, LQR_STATE_RESIZING) == LQR_STATE_IS_CANCELLED);
            CHECK(lqr_state_clear(&g_state) == 1);
        }
    }
    __atomic_store_n(&g_stop, 1, __ATOMIC_RELEASE);
    CHECK(pthread_join(t, NULL) == 0);
    CHECK(!lqr_state_check(&g_state) && g_state.word == LQR_STATE_STD);      /* no call has run since the last clear */
    /* (counted after the join: the other thread adds to g_hits after its cancel has returned)
     * every cancel that hit a busy state was seen, none twice, none invented */
    CHECK(g_hits == seen);
    CHECK(n < 100000 || (seen > 0 && g_idle > 0));
    printf("state race ok calls %ld cancelled %ld seen_in_call %ld idle_cancels %ld\n", n, seen, seen_in_call, g_idle);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 2 && !strcmp(argv[1], "transitions")) return transitions();
    if (argc >= 3 && !strcmp(argv[1], "race")) return race(atol(argv[2]));
    fprintf(stderr, "usage: state_main transitions | race N\n");
    return 2;
}
