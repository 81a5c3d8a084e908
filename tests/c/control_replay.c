/* control_replay.c -- digiKam's content-aware filter as a C caller of include/lqr_control.h (tests/test_control_gpu.py): progress
 * callbacks, a preservation mask through lqr_carver_bias_add_xy (one call per pixel), lqr_carver_resize on one pthread and
 * lqr_carver_cancel from another at a handshake, then the scan of what the carver holds and lqr_carver_destroy.
 *
 *   control_replay in.bin out.bin
 *   in.bin:  int32 w, h, channels, w1, h1, at (the update event at which the other thread cancels), then w*h*channels bytes
 *   out.bin: int32 resize's return value, cancel's, update events seen, end events seen, width, height, then the scanned image
 */
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lqr.h"
#include "lqr_masks.h"
#include "lqr_control.h"

static LqrCarver *g_carver;
static int g_updates, g_ends, g_at, g_cancel_ret = -1;
static int g_asked, g_done;
static pthread_mutex_t g_lock = PTHREAD_MUTEX_INITIALIZER;
static pthread_cond_t g_cond = PTHREAD_COND_INITIALIZER;

/* the UI thread: waits until the worker's progress says "now", cancels, says so */
static void *ui_thread(void *arg)
{
    (void) arg;
    pthread_mutex_lock(&g_lock);
    while (!g_asked) pthread_cond_wait(&g_cond, &g_lock);
    pthread_mutex_unlock(&g_lock);
    g_cancel_ret = (int) lqr_carver_cancel(g_carver);
    pthread_mutex_lock(&g_lock);
    g_done = 1;
    pthread_cond_broadcast(&g_cond);
    pthread_mutex_unlock(&g_lock);
    return NULL;
}

static LqrRetVal on_init(const gchar *m) { (void) m; return LQR_OK; }
static LqrRetVal on_end(const gchar *m) { (void) m; g_ends++; return LQR_OK; }
static LqrRetVal on_update(gdouble p)
{
    (void) p;
    if (++g_updates == g_at) {
        pthread_mutex_lock(&g_lock);
        g_asked = 1;
        pthread_cond_broadcast(&g_cond);
        while (!g_done) pthread_cond_wait(&g_cond, &g_lock);
        pthread_mutex_unlock(&g_lock);
    }
    return LQR_OK;
}

struct job { int w1, h1; LqrRetVal ret; };
static void *worker_thread(void *arg)
{
    struct job *j = (struct job *) arg;
    j->ret = lqr_carver_resize(g_carver, j->w1, j->h1);
    return NULL;
}

int main(int argc, char **argv)
{
    int hdr[6], w, h, ch, x, y, out[6];
    guchar *img, *res;
    LqrProgress *p;
    pthread_t ui, worker;
    struct job j;
    FILE *f;
    if (argc != 3 || !(f = fopen(argv[1], "rb"))) return 2;
    if (fread(hdr, sizeof hdr, 1, f) != 1) return 2;
    w = hdr[0]; h = hdr[1]; ch = hdr[2]; j.w1 = hdr[3]; j.h1 = hdr[4]; g_at = hdr[5];
    img = (guchar *) malloc((size_t) w * h * ch);
    if (!img || fread(img, (size_t) w * h * ch, 1, f) != 1) return 2;
    fclose(f);

    g_carver = lqr_carver_new(img, w, h, ch);           /* owns img from here on */
    if (!g_carver) return 3;
    if (lqr_carver_init(g_carver, 1, 0) != LQR_OK) return 3;
    for (y = h / 4; y < h / 2; y++)
        for (x = w / 4; x < w / 2; x++)
            if (lqr_carver_bias_add_xy(g_carver, 1000.0, x, y) != LQR_OK) return 4;
    p = lqr_progress_new();
    if (!p) return 3;
    lqr_progress_set_init(p, on_init);
    lqr_progress_set_update(p, on_update);
    lqr_progress_set_end(p, on_end);
    lqr_carver_set_progress(g_carver, p);
    lqr_carver_set_use_cache(g_carver, TRUE);

    if (pthread_create(&ui, NULL, ui_thread, NULL) || pthread_create(&worker, NULL, worker_thread, &j)) return 5;
    pthread_join(worker, NULL);
    pthread_mutex_lock(&g_lock);            /* (a resize that ended before the handshake must not leave the UI thread waiting) */
    g_asked = 1;
    pthread_cond_broadcast(&g_cond);
    pthread_mutex_unlock(&g_lock);
    pthread_join(ui, NULL);

    out[0] = (int) j.ret; out[1] = g_cancel_ret; out[2] = g_updates; out[3] = g_ends;
    out[4] = lqr_carver_get_width(g_carver); out[5] = lqr_carver_get_height(g_carver);
    res = (guchar *) calloc((size_t) out[4] * out[5], ch);
    if (!res) return 3;
    {
        gint n;
        guchar *line;
        lqr_carver_scan_reset(g_carver);
        while (lqr_carver_scan_line(g_carver, &n, &line)) {
            if (lqr_carver_scan_by_row(g_carver)) memcpy(res + (size_t) n * out[4] * ch, line, (size_t) out[4] * ch);
            else
                for (y = 0; y < out[5]; y++) memcpy(res + ((size_t) y * out[4] + n) * ch, line + (size_t) y * ch, ch);
        }
    }
    if (lqrx_carver_cancelled(g_carver) != (j.ret == LQR_USRCANCEL)) return 6;
    lqr_carver_destroy(g_carver);
    if (!(f = fopen(argv[2], "wb"))) return 2;
    fwrite(out, sizeof out, 1, f);
    fwrite(res, (size_t) out[4] * out[5] * ch, 1, f);
    fclose(f);
    free(res);
    return 0;
}
