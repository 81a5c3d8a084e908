/*
 * lqr_carver.c -- host side (plain C) of the MI355X seam-carving engine: the
 * LqrCarver C ABI of include/lqr.h, implemented on top of the device shim of
 * include/lqr_hip.h.  It is what gimp-lqr-plugin's src/render.c and
 * src/io_functions.c bind instead of liblqr-1.
 *
 * This file holds NO pixel arithmetic: it keeps what liblqr keeps in LqrCarver,
 * does on the device what the resize schedule of lqr_sched.h says comes next
 * (the geometry's transitions, the steps of a direction, per seam whether the DP
 * map is rebuilt or band-updated), fires the progress callbacks, and serves
 * scan lines from a packed read-back.  All planes live in
 * HBM; every stage is a kernel launched through lqrhip_*.  There is no CPU
 * fallback: without a gfx950 device lqr_carver_new() returns NULL and says why.
 *
 * Orchestration is written once over a "group" of carvers of identical geometry
 * and configuration advancing in lock-step (lqrx_carver_resize_batch); the
 * plug-in's single carver is a group of one.
 */
#ifdef LQRHIP_TIMING
#define _POSIX_C_SOURCE 199309L
#endif
#include <stdlib.h>
#include <string.h>
#include <stdio.h>
#include <math.h>

#include "../../include/lqr.h"
#include "../../include/lqr_coldepth.h"
#include "../../include/lqr_imagetype.h"
#include "../../include/lqr_masks.h"
#include "../../include/lqr_energy.h"
#include "../../include/lqr_vmap.h"
#include "../../include/lqr_control.h"
#include "../../include/lqr_sizes.h"
#include "../../include_ext/lqr_forward.h"
#include "../../include_ext/lqr_static.h"
#include "../../include_ext/lqr_clipforward.h"
#include "../../include_ext/lqr_remove.h"
#include "../../include/lqr_hip.h"
#include "lqr_mask_queue.h"
#include "lqr_sched.h"
#include "lqr_state.h"

#define MAXI(a, b) ((a) > (b) ? (a) : (b))
#define MINI(a, b) ((a) < (b) ? (a) : (b))

/* Host timers around the fixed part of a batched resize (-DLQRHIP_TIMING in CFLAGS; compiled out by default): wall time the calling
 * thread spends in the reload, in group_open, in group_close and in a session's tail (self-check .. commit of the inflated planes),
 * printed per part when the library is unloaded.  profiles/fixedcost/README.md */
#ifdef LQRHIP_TIMING
#include <time.h>
enum { T_RELOAD, T_OPEN, T_CLOSE, T_TAIL, T_PARTS };
static double g_t_sum[T_PARTS];
static long g_t_calls[T_PARTS];
static double t_now(void) { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6; }
__attribute__((destructor)) static void t_report(void)
{
    static const char *const name[T_PARTS] = {"reload", "group_open", "group_close", "session_tail"};
    int i;
    for (i = 0; i < T_PARTS; i++)
        if (g_t_calls[i]) fprintf(stderr, "LQRHIP_TIMING %s calls %ld total_ms %.3f mean_ms %.4f\n", name[i], g_t_calls[i], g_t_sum[i], g_t_sum[i] / g_t_calls[i]);
}
#define T_BEGIN(part) const double t_begin_##part = t_now()
#define T_END(part) do { g_t_sum[part] += t_now() - t_begin_##part; g_t_calls[part]++; } while (0)
#else
#define T_BEGIN(part) do { } while (0)
#define T_END(part) do { } while (0)
#endif

struct _LqrProgress {
    gfloat update_step;
    LqrProgressFuncInit init;
    LqrProgressFuncUpdate update;
    LqrProgressFuncEnd end;
    gchar init_width_message[LQR_PROGRESS_MAX_MESSAGE_LENGTH];
    gchar end_width_message[LQR_PROGRESS_MAX_MESSAGE_LENGTH];
    gchar init_height_message[LQR_PROGRESS_MAX_MESSAGE_LENGTH];
    gchar end_height_message[LQR_PROGRESS_MAX_MESSAGE_LENGTH];
};

struct _LqrVMap {
    gint *buffer;
    gint width, height, depth, orientation;
};
struct _LqrVMapList {
    LqrVMap *current;
    LqrVMapList *next;
};
struct _LqrCarverList {
    LqrCarver *current;
    LqrCarverList *next;
};

struct _LqrCarver {
    LqrGeom geo;                /* the geometry and its transitions: lqr_sched.h */
    int channels;
    int col_depth;              /* LqrColDepth: 0 (8I, what lqr_carver_new makes) .. 3 (64F) */
    int image_type;             /* LqrImageType, with the channel indices of its roles (-1: none): what the energy reads (lqr_imagetype.h) */
    int alpha_channel, black_channel;
    int preserve_input;         /* lqr_carver_set_preserve_input_image: the caller's buffer is never written nor freed */
    int img_w, img_h;           /* the image handed to lqr_carver_new */
    int active;
    LqrCarver *root;
    LqrCarverList *attached;

    int delta_x;
    float rigidity;
    float rigidity_map[2 * LQRHIP_MAX_DELTA + 1];      /* [dx + delta_x] */
    int has_bias, has_rigmask;
    LqrMaskQueue mq[2];         /* lqr_carver_bias_add_xy / lqr_carver_rigmask_add_xy calls not yet on the device ([0] bias, [1] rigidity mask) */
    int nrg_func, nrg_radius;
    int leftright, lr_switch_frequency;
    float enl_step;
    int resize_order;
    int dump_vmaps;
    LqrState state;             /* liblqr's carver state, the one word lqr_carver_cancel touches (lqr_state.h); a root's: attached carvers read their root's */
    LqrVMapList *flushed_vs;
    LqrProgress *progress;
    int session_update_step, session_rescale_total, session_rescale_current;

    /* device */
    LqrHipCarver *dev;
    LqrHipBatch *own_batch;     /* batch of one, created lazily (roots only) */
    int wk_valid;               /* working planes describe the carved frame */

    /* read-out cache: visible image at (w, level), carver orientation */
    guchar *ro_image;
    size_t ro_image_len;
    guchar *in_buffer;          /* the caller's pixel buffer (ownership passed at lqr_carver_new), kept as liblqr keeps it */
    size_t in_buffer_len;
    int ro_valid, ro_line, ro_x;    /* ro_x: the next pixel of line ro_line for lqr_carver_scan_ext */
    guchar *ro_buffer;          /* one line, the pointer scan_line hands out */
    int ro_buffer_len;

    /* debug snapshot */
    float *dbg_en, *dbg_m;
    int *dbg_least, dbg_w, dbg_h;
    int dbg_org, dbg_org_prev, dbg_side;        /* the snapshot's seam flags (lqrhip_read_seam_flags) */
};

/* bytes per channel of each LqrColDepth */
static const int k_depth_bytes[4] = {1, 2, 4, 8};
#define PX_BYTES(r) ((size_t) (r)->channels * k_depth_bytes[(r)->col_depth])

#define MAX_SUB 8
typedef struct {
    LqrCarver **r;
    int n;
    /* the group's carvers are split over nb device batches (one HIP stream each), all advancing seam by seam:
     * the latency-bound chain kernels of one sub-batch run under the bandwidth-bound carve of another */
    LqrHipBatch *b[MAX_SUB];
    int nb;
} Group;

static int g_debug_snapshot = 0;
void lqrx_set_debug(gint on) { g_debug_snapshot = on; }

/* the shim's code behind the last non-OK return: LQRHIP_EFAULT (a kernel gave up, a self-check failed) is what
 * group_build_maps can recover from */
static int g_last_rc = 0;
static LqrRetVal hip_ret(int rc)
{
    if (rc == 0) return LQR_OK;
    g_last_rc = rc;
    fprintf(stderr, "liblqr-hip: device error %d: %s\n", rc, lqrhip_last_error());
    return rc == LQRHIP_ENOMEM ? LQR_NOMEM : LQR_ERROR;
}
/* Recovery (round 6).  The plug-in tests lqr_carver_resize's return value only against LQR_NOMEM (src/render.c:42-46,318) and
 * then writes the carver to the user's layer (:366): a resize must not end in LQR_ERROR because a spin protocol timed out on a
 * busy device.  A session (one visibility-map build) that ends in LQRHIP_EFAULT is rolled back -- the base layout is as before,
 * the host's bookkeeping restored -- and carved again on the kernels without spin waits; only if that fails too does the caller
 * see LQR_ERROR, with the carver as it was before the session.  lqrhip_set_recovery(0) switches the redo off (tests). */
#define HIP_CATCH(expr) LQR_CATCH(hip_ret(expr))

/* ======================= progress ======================================== */
LqrProgress *lqr_progress_new(void)
{
    LqrProgress *p = (LqrProgress *) calloc(1, sizeof *p);
    if (!p) return NULL;
    p->update_step = 0.02f;
    strcpy(p->init_width_message, "Resizing width...");
    strcpy(p->init_height_message, "Resizing height...");
    strcpy(p->end_width_message, "done");
    strcpy(p->end_height_message, "done");
    return p;
}
LqrRetVal lqr_progress_set_init(LqrProgress *p, LqrProgressFuncInit f) { p->init = f; return LQR_OK; }
LqrRetVal lqr_progress_set_update(LqrProgress *p, LqrProgressFuncUpdate f) { p->update = f; return LQR_OK; }
LqrRetVal lqr_progress_set_end(LqrProgress *p, LqrProgressFuncEnd f) { p->end = f; return LQR_OK; }
LqrRetVal lqr_progress_set_update_step(LqrProgress *p, gfloat s) { p->update_step = s; return LQR_OK; }
static LqrRetVal copy_message(gchar *dst, const gchar *src)
{
    if (!src) return LQR_ERROR;
    snprintf(dst, LQR_PROGRESS_MAX_MESSAGE_LENGTH, "%s", src);
    return LQR_OK;
}
LqrRetVal lqr_progress_set_init_width_message(LqrProgress *p, const gchar *m) { return copy_message(p->init_width_message, m); }
LqrRetVal lqr_progress_set_init_height_message(LqrProgress *p, const gchar *m) { return copy_message(p->init_height_message, m); }
LqrRetVal lqr_progress_set_end_width_message(LqrProgress *p, const gchar *m) { return copy_message(p->end_width_message, m); }
LqrRetVal lqr_progress_set_end_height_message(LqrProgress *p, const gchar *m) { return copy_message(p->end_height_message, m); }

/* ======================= lists, vmaps ==================================== */
/* node n at the end of a list of T (the attached carvers, the dumped maps) */
#define LIST_APPEND(T, head, n)                      \
    do {                                             \
        T **pp__ = &(head);                          \
        while (*pp__) pp__ = &(*pp__)->next;         \
        *pp__ = (n);                                 \
    } while (0)
LqrCarverList *lqr_carver_list_start(LqrCarver *r) { return r->attached; }
LqrCarver *lqr_carver_list_current(LqrCarverList *l) { return l->current; }
LqrCarverList *lqr_carver_list_next(LqrCarverList *l) { return l->next; }
LqrVMapList *lqr_vmap_list_start(LqrCarver *r) { return r->flushed_vs; }
LqrVMap *lqr_vmap_list_current(LqrVMapList *l) { return l->current; }
LqrVMapList *lqr_vmap_list_next(LqrVMapList *l) { return l->next; }
LqrRetVal lqr_vmap_list_foreach(LqrVMapList *list, LqrVMapFunc func, gpointer data)
{
    for (; list; list = list->next) LQR_CATCH(func(list->current, data));
    return LQR_OK;
}
gint *lqr_vmap_get_data(LqrVMap *v) { return v->buffer; }
gint lqr_vmap_get_width(LqrVMap *v) { return v->width; }
gint lqr_vmap_get_height(LqrVMap *v) { return v->height; }
gint lqr_vmap_get_depth(LqrVMap *v) { return v->depth; }
gint lqr_vmap_get_orientation(LqrVMap *v) { return v->orientation; }
void lqr_vmap_destroy(LqrVMap *v) { if (v) { free(v->buffer); free(v); } }
/* lqr_vmap.h: a map object around the caller's malloc'd buffer, which it owns from here on.  Nothing is checked, as in liblqr:
 * lqr_vmap_load is where a map meets a carver */
LqrVMap *lqr_vmap_new(gint *buffer, gint width, gint height, gint depth, gint orientation)
{
    LqrVMap *v = (LqrVMap *) calloc(1, sizeof *v);
    if (!v) return NULL;
    v->buffer = buffer;
    v->width = width; v->height = height; v->depth = depth; v->orientation = orientation;
    return v;
}

/* ======================= lifecycle ======================================= */
/* the carver of lqr_carver_new / lqr_carver_new_ext, arguments checked: pixels of `depth` (LqrColDepth) uploaded as the base
 * layout, liblqr's defaults */
static const LqrImageType default_type[6] = {LQR_RGB_IMAGE, LQR_GREY_IMAGE, LQR_GREYA_IMAGE, LQR_RGB_IMAGE, LQR_RGBA_IMAGE, LQR_CMYKA_IMAGE};
static void set_type_defaults(LqrCarver *r, LqrImageType t)
{
    r->image_type = (int) t;
    r->alpha_channel = t == LQR_GREYA_IMAGE ? 1 : t == LQR_RGBA_IMAGE ? 3 : t == LQR_CMYKA_IMAGE ? 4 : -1;
    r->black_channel = (t == LQR_CMYK_IMAGE || t == LQR_CMYKA_IMAGE) ? 3 : -1;
}

/* the limit on channels per pixel: 4 unless the caller raised it (lqr_imagetype.h) */
static int g_max_channels = 4;
gint lqrx_set_max_channels(gint n)
{
    const int prev = g_max_channels;
    if (n >= 4 && n <= LQRHIP_MAX_CHANNELS) g_max_channels = n;
    return prev;
}

static LqrCarver *carver_new(void *buffer, int width, int height, int channels, int depth)
{
    LqrCarver *r = (LqrCarver *) calloc(1, sizeof *r);
    if (!r) return NULL;
    r->dev = lqrhip_carver_create_ext(buffer, width, height, channels, depth);
    if (!r->dev) {
        fprintf(stderr, "liblqr-hip: lqr_carver_new failed: %s\n", lqrhip_last_error());
        free(r);
        return NULL;
    }
    /* ownership passed to the carver (render.c:220-223).  The pixels now live in HBM; the block is kept, as liblqr keeps it,
     * and becomes the read-out buffer: handing 33 MB back to the C library and asking for 31 MB again costs an munmap, an
     * mmap and a page fault per 4 KiB -- more than the transfer itself (measured: 64 x 4K uploads 207 ms with the free, 62 without) */
    r->col_depth = depth;
    r->channels = channels;
    set_type_defaults(r, channels >= 6 ? LQR_CUSTOM_IMAGE : default_type[channels]);
    (void) lqrhip_carver_set_read(r->dev, r->image_type, r->alpha_channel, r->black_channel);
    r->in_buffer = (guchar *) buffer;
    r->in_buffer_len = (size_t) width * height * channels * k_depth_bytes[depth];
    lqr_geom_reset(&r->geo, width, height);
    r->delta_x = 1;
    r->img_w = width; r->img_h = height;
    r->nrg_func = LQR_EF_GRAD_XABS;
    r->nrg_radius = 1;
    r->enl_step = 2.0f;
    r->resize_order = LQR_RES_ORDER_HOR;
    r->progress = lqr_progress_new();
    if (!r->progress) { lqrhip_carver_destroy(r->dev); free(r); return NULL; }
    lqr_maskq_init(&r->mq[0], 0);
    lqr_maskq_init(&r->mq[1], 0);
    lqr_state_init(&r->state);
    return r;
}

LqrCarver *lqr_carver_new(guchar *buffer, gint width, gint height, gint channels)
{
    if (!buffer || width < 1 || height < 1 || channels < 1) return NULL;
    if (channels > g_max_channels) {        /* (said on stderr since the limit can be raised; lqr_carver_new_ext always said it) */
        fprintf(stderr, "liblqr-hip: lqr_carver_new: %d channels are not supported (1 .. %d channels; lqrx_set_max_channels raises the limit)\n",
                channels, g_max_channels);
        return NULL;
    }
    return carver_new(buffer, width, height, channels, LQR_COLDEPTH_8I);
}

/* liblqr's entry point for pixels of any depth (lqr_coldepth.h): 8I is lqr_carver_new; a carver of another depth has a base
 * layout of channels x {2, 4, 8} bytes per pixel */
LqrCarver *lqr_carver_new_ext(void *buffer, gint width, gint height, gint channels, LqrColDepth colour_depth)
{
    const int depth = (int) colour_depth;
    if (channels > g_max_channels || depth < LQR_COLDEPTH_8I || depth > LQR_COLDEPTH_64F) {
        fprintf(stderr, "liblqr-hip: lqr_carver_new_ext: %d channels at colour depth %d are not supported (1 .. %d channels, depths 8I 16I 32F 64F; "
                "lqrx_set_max_channels raises the channel limit)\n", channels, depth, g_max_channels);
        return NULL;
    }
    if (!buffer || width < 1 || height < 1 || channels < 1) return NULL;
    return carver_new(buffer, width, height, channels, depth);
}

void lqr_carver_set_preserve_input_image(LqrCarver *r) { r->preserve_input = 1; }
LqrColDepth lqr_carver_get_col_depth(LqrCarver *r) { return (LqrColDepth) r->col_depth; }
gint lqr_carver_get_bpp(LqrCarver *r) { return r->channels; }          /* liblqr: the deprecated name of get_channels */
LqrImageType lqr_carver_get_image_type(LqrCarver *r) { return (LqrImageType) r->image_type; }

/* the image type and its roles as they stand go to the device; a root carver whose energy reads something else now lays its
 * working planes out again at the next session (an attached carver has none) */
static void type_changed(LqrCarver *r)
{
    if (lqrhip_carver_set_read(r->dev, r->image_type, r->alpha_channel, r->black_channel) == 1 && !r->root) r->wk_valid = 0;
}
LqrRetVal lqr_carver_set_image_type(LqrCarver *r, LqrImageType image_type)
{
    static const int channels_of[7] = {3, 4, 1, 2, 3, 4, 5};        /* RGB RGBA GREY GREYA CMY CMYK CMYKA */
    if ((int) image_type < LQR_RGB_IMAGE || (int) image_type > LQR_CUSTOM_IMAGE) return LQR_ERROR;
    if (image_type != LQR_CUSTOM_IMAGE && channels_of[image_type] != r->channels) return LQR_ERROR;
    set_type_defaults(r, image_type);
    type_changed(r);
    return LQR_OK;
}
/* one role moved to channel `index` (negative: cleared); the other role loses the channel if it held it */
static LqrRetVal set_role(LqrCarver *r, int *role, int *other, int index)
{
    if (index >= r->channels) return LQR_ERROR;
    if (index < 0) index = -1;
    else if (*other == index) *other = -1;
    *role = index;
    r->image_type = LQR_CUSTOM_IMAGE;
    type_changed(r);
    return LQR_OK;
}
LqrRetVal lqr_carver_set_alpha_channel(LqrCarver *r, gint i) { return set_role(r, &r->alpha_channel, &r->black_channel, i); }
LqrRetVal lqr_carver_set_black_channel(LqrCarver *r, gint i) { return set_role(r, &r->black_channel, &r->alpha_channel, i); }

/* rigidity bias ~ |dx|^1.5 summed along the seam (help/en/index.wiki:83); the
 * table is tiny and is computed on the host so that it is bit-identical to C */
static void rigidity_table(LqrCarver *r)
{
    int x;
    for (x = -r->delta_x; x <= r->delta_x; x++)
        r->rigidity_map[x + r->delta_x] = r->rigidity * powf(fabsf((float) x), 1.5f) / r->geo.h;
}

LqrRetVal lqr_carver_init(LqrCarver *r, gint delta_x, gfloat rigidity)
{
    if (r->active || delta_x < 0 || delta_x > LQRHIP_MAX_DELTA) return LQR_ERROR;
    r->delta_x = delta_x;
    r->rigidity = rigidity;
    rigidity_table(r);
    HIP_CATCH(lqrhip_carver_activate(r->dev));
    r->active = 1;
    return LQR_OK;
}

static void carver_free_host(LqrCarver *r)
{
    LqrVMapList *v, *vn;
    for (v = r->flushed_vs; v; v = vn) { vn = v->next; lqr_vmap_destroy(v->current); free(v); }
    free(r->progress);
    free(r->ro_image); free(r->ro_buffer);
    if (!r->preserve_input) free(r->in_buffer);
    free(r->dbg_en); free(r->dbg_m); free(r->dbg_least);
    lqr_maskq_free(&r->mq[0]); lqr_maskq_free(&r->mq[1]);        /* what was still queued is dropped */
    free(r);
}

void lqr_carver_destroy(LqrCarver *r)
{
    LqrCarverList *l, *ln;
    if (!r) return;
    if (r->own_batch) lqrhip_batch_destroy(r->own_batch);
    for (l = r->attached; l; l = ln) {
        ln = l->next;
        lqr_carver_destroy(l->current);
        free(l);
    }
    lqrhip_carver_destroy(r->dev);
    carver_free_host(r);
}

LqrRetVal lqr_carver_attach(LqrCarver *r, LqrCarver *aux)
{
    LqrCarverList *n;
    if (r->geo.w0 != aux->geo.w0 || r->geo.h0 != aux->geo.h0) return LQR_ERROR;
    n = (LqrCarverList *) calloc(1, sizeof *n);
    if (!n) return LQR_NOMEM;
    n->current = aux;
    LIST_APPEND(LqrCarverList, r->attached, n);
    aux->root = r;
    HIP_CATCH(lqrhip_carver_attach(r->dev, aux->dev));
    return LQR_OK;
}

/* ======================= configuration =================================== */
LqrRetVal lqr_carver_set_energy_function_builtin(LqrCarver *r, LqrEnergyFuncBuiltinType ef)
{
    /* a value-plane carver's working planes hold the value the energy reads (brightness or luma): a change of kind rebuilds them.
     * Every carver is told, a packed 8-bit one too: a later lqr_carver_set_image_type can turn it into a value-plane carver, which
     * then finds the flag; the call returns 1 only where the planes in use change. */
    const int luma = (int) ef >= LQR_EF_LUMA_GRAD_NORM && (int) ef <= LQR_EF_LUMA_GRAD_XABS;
    if ((int) ef < LQR_EF_GRAD_NORM || (int) ef > LQR_EF_NULL) return LQR_ERROR;
    if (lqrhip_carver_set_read_luma(r->dev, luma)) r->wk_valid = 0;
    r->nrg_func = (int) ef;
    r->nrg_radius = (ef == LQR_EF_NULL) ? 0 : 1;
    return LQR_OK;
}
void lqr_carver_set_resize_order(LqrCarver *r, LqrResizeOrder o) { r->resize_order = (int) o; }
void lqr_carver_set_progress(LqrCarver *r, LqrProgress *p) { free(r->progress); r->progress = p; }
void lqr_carver_set_side_switch_frequency(LqrCarver *r, guint f) { r->lr_switch_frequency = (int) f; }
LqrRetVal lqr_carver_set_enl_step(LqrCarver *r, gfloat s)
{
    if (!(s > 1 && s <= 2)) return LQR_ERROR;
    r->enl_step = s;
    return LQR_OK;
}
gfloat lqr_carver_get_enl_step(LqrCarver *r) { return r->enl_step; }
void lqr_carver_set_dump_vmaps(LqrCarver *r) { r->dump_vmaps = 1; }

/* ======================= carver control (lqr_control.h) ================== */
/* The one call a second thread may make: it touches the root's state word and nothing else.  On an attached carver: LQR_ERROR, as in
 * liblqr (tests/golden/control/, cancel_aux_idle and cancel_aux_in_resize). */
LqrRetVal lqr_carver_cancel(LqrCarver *r)
{
    if (!r || r->root) return LQR_ERROR;
    (void) lqr_state_cancel(&r->state);
    return LQR_OK;
}
gint lqrx_carver_cancelled(LqrCarver *r) { return r ? lqr_state_check(lqr_state_word(&r->state, r->root ? &r->root->state : NULL)) : 0; }
LqrRetVal lqrx_carver_cancel_clear(LqrCarver *r)
{
    if (!r || r->root) return LQR_ERROR;
    return lqr_state_clear(&r->state) ? LQR_OK : LQR_ERROR;
}
/* (the read plane is the cache: lqr_control.h) */
void lqr_carver_set_use_cache(LqrCarver *r, gboolean use_cache) { (void) r; (void) use_cache; }
void lqr_carver_set_no_dump_vmaps(LqrCarver *r) { r->dump_vmaps = 0; }
LqrRetVal lqr_carver_list_foreach(LqrCarverList *list, LqrCarverFunc func, LqrDataTok data)
{
    for (; list; list = list->next) LQR_CATCH(func(list->current, data));
    return LQR_OK;
}
/* (attached carvers lie one level deep here: nothing further to visit) */
LqrRetVal lqr_carver_list_foreach_recursive(LqrCarverList *list, LqrCarverFunc func, LqrDataTok data) { return lqr_carver_list_foreach(list, func, data); }
void lqr_carver_set_gradient_function(LqrCarver *r, LqrGradFuncType gf_ind)
{
    static const LqrEnergyFuncBuiltinType builtin_of[6] = {LQR_EF_GRAD_NORM, LQR_EF_NULL, LQR_EF_GRAD_SUMABS, LQR_EF_GRAD_XABS, LQR_EF_NULL, LQR_EF_NULL};
    if ((int) gf_ind >= LQR_GF_NORM && (int) gf_ind <= LQR_GF_NULL) (void) lqr_carver_set_energy_function_builtin(r, builtin_of[gf_ind]);
}

/* A call that works on the device enters the busy state on every root it was given and leaves it on every way out; a carver that is
 * marked cancelled refuses the call (LQR_USRCANCEL, as liblqr's LQR_CATCH_CANC), one that is inside another call too (LQR_ERROR) */
static LqrRetVal roots_enter(LqrCarver **rs, int n, int busy)
{
    int i;
    for (i = 0; i < n; i++) {
        const int rc = lqr_state_enter(&rs[i]->state, busy);
        if (rc != LQR_STATE_ENTERED) {
            while (i--) lqr_state_leave(&rs[i]->state);
            return rc == LQR_STATE_IS_CANCELLED ? LQR_USRCANCEL : LQR_ERROR;
        }
    }
    return LQR_OK;
}
static void roots_leave(LqrCarver **rs, int n)
{
    int i;
    for (i = 0; i < n; i++) lqr_state_leave(&rs[i]->state);
}

/* ======================= getters ========================================= */
gint lqr_carver_get_width(LqrCarver *r) { return r->geo.transposed ? r->geo.h : r->geo.w; }
gint lqr_carver_get_height(LqrCarver *r) { return r->geo.transposed ? r->geo.w : r->geo.h; }
gint lqr_carver_get_channels(LqrCarver *r) { return r->channels; }
gint lqr_carver_get_ref_width(LqrCarver *r) { return r->geo.transposed ? r->geo.h_start : r->geo.w_start; }
gint lqr_carver_get_ref_height(LqrCarver *r) { return r->geo.transposed ? r->geo.w_start : r->geo.h_start; }
gint lqr_carver_get_orientation(LqrCarver *r) { return r->geo.transposed ? 1 : 0; }
gint lqr_carver_get_depth(LqrCarver *r) { return r->geo.w0 - r->geo.w_start; }
gint lqrx_carver_frame_width(LqrCarver *r) { return r->geo.w; }
gint lqrx_carver_frame_height(LqrCarver *r) { return r->geo.h; }

/* ======================= group helpers =================================== */
/* what is visible changed: the read-out cache is stale and the scan starts over */
static void ro_invalidate(LqrCarver *r)
{
    r->ro_valid = 0;
    r->ro_line = 0; r->ro_x = 0;
}
static void set_width_one(LqrCarver *r, int w1)
{
    lqr_geom_set_width(&r->geo, w1);
    ro_invalidate(r);
}
static void set_width_tree(LqrCarver *r, int w1)
{
    LqrCarverList *l;
    set_width_one(r, w1);
    for (l = r->attached; l; l = l->next) set_width_tree(l->current, w1);
}

/* delta_x = 2 .. 10 (the whole range of the plug-in's dialog, src/interface.c:47), or a rigidity mask that matters: the carver runs
 * on the tiled kernels' general instantiations, which need the whole group co-resident on ONE stream */
static int is_general(const LqrCarver *c)
{
    return (c->delta_x >= 2 && c->delta_x <= 10) || (c->delta_x == 1 && c->has_rigmask && c->rigidity != 0);
}

static LqrRetVal group_open(Group *g, LqrCarver **rs, int n)
{
    int i, k;
    g->r = rs; g->n = n; g->nb = 0;
    for (k = 0; k < MAX_SUB; k++) g->b[k] = NULL;
    if (n == 1) {
        if (!rs[0]->own_batch) {
            LqrHipCarver *d = rs[0]->dev;
            rs[0]->own_batch = lqrhip_batch_create(&d, 1);
            if (!rs[0]->own_batch) return LQR_NOMEM;
        }
        g->b[0] = rs[0]->own_batch;
        g->nb = 1;
    } else {
        LqrHipCarver **ds = (LqrHipCarver **) malloc((size_t) n * sizeof *ds);
        /* sub-batch streams are for the plain kernels: a shared batch never runs the persistent tiled kernels, and a general
         * group of 32 or more (small images: the limit of lqrx_carver_resize_batch is in tiles, not images) would fall to the
         * one-wave-per-image kernels, ~30x slower */
        int nb = is_general(rs[0]) ? 1 : lqrhip_sub_batches(n);
        if (nb < 1) nb = 1;
        if (nb > MAX_SUB) nb = MAX_SUB;
        if (nb > n) nb = n;
        if (!ds) return LQR_NOMEM;
        for (i = 0; i < n; i++) {
            if (rs[i]->own_batch) { lqrhip_batch_destroy(rs[i]->own_batch); rs[i]->own_batch = NULL; }
            ds[i] = rs[i]->dev;
        }
        for (k = 0; k < nb; k++) {
            int lo = (int) ((long long) n * k / nb), hi = (int) ((long long) n * (k + 1) / nb);
            g->b[k] = lqrhip_batch_create(ds + lo, hi - lo);
            if (!g->b[k]) {     /* give the sub-batches (and their streams) created so far back */
                int q;
                for (q = 0; q < k; q++) { lqrhip_batch_destroy(g->b[q]); g->b[q] = NULL; }
                g->nb = 0;
                free(ds);
                return LQR_NOMEM;
            }
            lqrhip_batch_set_shared(g->b[k], nb > 1 ? nb : 0);       /* how many sub-batches run side by side */
            g->nb = k + 1;
        }
        free(ds);
    }
    return LQR_OK;
}
static void group_close(Group *g)
{
    int k;
    if (g->n > 1)
        for (k = 0; k < g->nb; k++) lqrhip_batch_destroy(g->b[k]);
    g->nb = 0;
}
/* the same device call on every sub-batch */
#define HIP_ALL(g, call)                                                   \
    do {                                                                   \
        int k__;                                                           \
        for (k__ = 0; k__ < (g)->nb; k__++) {                              \
            LqrHipBatch *B = (g)->b[k__];                                  \
            HIP_CATCH(call);                                               \
        }                                                                  \
    } while (0)

#define FOR_TREE(g, i, r, body)                                   \
    for (i = 0; i < (g)->n; i++) {                                \
        LqrCarverList *l__;                                       \
        LqrCarver *r = (g)->r[i];                                 \
        body;                                                     \
        for (l__ = (g)->r[i]->attached; l__; l__ = l__->next) {   \
            r = l__->current;                                     \
            body;                                                 \
        }                                                         \
    }

/* the check points of lqr_carver_cancel: one relaxed load per root */
static int group_cancelled(const Group *g)
{
    int i;
    for (i = 0; i < g->n; i++)
        if (lqr_state_check(&g->r[i]->state)) return 1;
    return 0;
}
#define CANCEL_POINT(g) do { if (group_cancelled(g)) return LQR_USRCANCEL; } while (0)
/* ... and before a pass, which also names what the carvers are busy with (liblqr's LqrCarverState) */
static LqrRetVal group_phase(Group *g, int busy)
{
    int i;
    CANCEL_POINT(g);
    for (i = 0; i < g->n; i++) (void) lqr_state_phase(&g->r[i]->state, busy);
    return LQR_OK;
}

static void dp_params(const LqrCarver *r, LqrHipDpParams *p)
{
    memset(p, 0, sizeof *p);
    p->delta_x = r->delta_x;
    p->use_rigidity = r->rigidity != 0;
    memcpy(p->rigidity_map, r->rigidity_map, sizeof p->rigidity_map);
    p->nrg_func = r->nrg_func;
    p->nrg_radius = r->nrg_radius;
    p->w_start = r->geo.w_start;
}

/* ======================= queued _xy mask calls (lqr_masks.h) ============= */
/* One plane's queue onto the device, in call order (lqr_mask_queue.h).  LQR_NOMEM (host or device) leaves the queue as it was; any
 * other failure drops it. */
static LqrRetVal mask_queue_flush_one(LqrCarver *r, int is_rig)
{
    LqrMaskQueue *q = &r->mq[is_rig];
    int *index, rc;
    double *value;
    size_t *start;
    if (!q->n) return LQR_OK;
    index = (int *) malloc(q->n * sizeof *index);
    value = (double *) malloc(q->n * sizeof *value);
    start = (size_t *) malloc(((size_t) q->buckets + 1) * sizeof *start);
    if (!index || !value || !start) { free(index); free(value); free(start); return LQR_NOMEM; }
    lqr_maskq_pack(q, index, value, start);
    rc = lqrhip_mask_scatter(r->dev, is_rig, index, value, start, (int) q->buckets);
    free(index); free(value); free(start);
    if (rc != LQRHIP_ENOMEM) lqr_maskq_reset(q);
    return hip_ret(rc);
}
/* before anything that reads or writes the mask planes or changes the layout */
static LqrRetVal mask_queue_flush(LqrCarver *r)
{
    LQR_CATCH(mask_queue_flush_one(r, 0));
    return mask_queue_flush_one(r, 1);
}

/* ======================= flatten / transpose (E11) ======================= */
static LqrRetVal group_flatten(Group *g)
{
    LqrCarver *r0 = g->r[0];
    int i;
    if (!lqr_geom_is_flat(&r0->geo)) {
        LQR_CATCH(group_phase(g, LQR_STATE_FLATTENING));
        HIP_ALL(g, lqrhip_flatten(B, r0->geo.w0, r0->geo.h0, r0->geo.w, r0->geo.level));     /* every sub-batch staged ... */
        HIP_ALL(g, lqrhip_planes_commit(B));                                                 /* ... before any adopts its flat layout */
    } else if (r0->wk_valid)       /* a flat carver is its own flattening */
        return LQR_OK;
    FOR_TREE(g, i, r, {
        lqr_geom_flattened(&r->geo);
        r->wk_valid = 0;
        ro_invalidate(r);
    });
    return LQR_OK;
}

static LqrRetVal group_transpose(Group *g)
{
    LqrCarver *r0 = g->r[0];
    int i, x;
    if (lqr_geom_flatten_before_transpose(&r0->geo)) LQR_CATCH(group_flatten(g));
    LQR_CATCH(group_phase(g, LQR_STATE_TRANSPOSING));
    HIP_ALL(g, lqrhip_transpose(B, r0->geo.w0, r0->geo.h0));
    HIP_ALL(g, lqrhip_planes_commit(B));
    FOR_TREE(g, i, r, {
        lqr_geom_transposed(&r->geo);
        if (r->active)      /* the rigidity table is rescaled, not recomputed */
            for (x = -r->delta_x; x <= r->delta_x; x++)
                r->rigidity_map[x + r->delta_x] = r->rigidity_map[x + r->delta_x] * r->geo.w0 / r->geo.h0;
        r->wk_valid = 0;
        ro_invalidate(r);
    });
    return LQR_OK;
}

LqrRetVal lqr_carver_flatten(LqrCarver *r)
{
    Group g;
    LqrRetVal ret;
    if (r->root) return LQR_ERROR;
    LQR_CATCH(roots_enter(&r, 1, LQR_STATE_FLATTENING));
    if ((ret = mask_queue_flush(r)) == LQR_OK && (ret = group_open(&g, &r, 1)) == LQR_OK) {
        ret = group_flatten(&g);
        group_close(&g);
    }
    roots_leave(&r, 1);
    return ret;
}

/* ======================= masks (E2) ====================================== */
static LqrRetVal mask_prepare(LqrCarver *r)
{
    if (!r->active || r->root) return LQR_ERROR;
    if (lqr_geom_needs_flatten(&r->geo)) LQR_CATCH(lqr_carver_flatten(r));
    return LQR_OK;
}

LqrRetVal lqr_carver_bias_add_rgb_area(LqrCarver *r, guchar *rgb, gint bias_factor, gint channels, gint width, gint height,
                                       gint x_off, gint y_off)
{
    LQR_CATCH(mask_prepare(r));
    if (bias_factor == 0) return LQR_OK;
    LQR_CATCH(mask_queue_flush(r));
    HIP_CATCH(lqrhip_mask_add(r->dev, rgb, channels, width, height, x_off, y_off, r->geo.transposed, 0, bias_factor));
    r->has_bias = 1;
    r->wk_valid = 0;
    return LQR_OK;
}

LqrRetVal lqr_carver_rigmask_add_rgb_area(LqrCarver *r, guchar *rgb, gint channels, gint width, gint height, gint x_off,
                                          gint y_off)
{
    LQR_CATCH(mask_prepare(r));
    LQR_CATCH(mask_queue_flush(r));
    HIP_CATCH(lqrhip_mask_add(r->dev, rgb, channels, width, height, x_off, y_off, r->geo.transposed, 1, 0));
    r->has_rigmask = 1;
    r->wk_valid = 0;
    return LQR_OK;
}

/* ---- computed masks (lqr_masks.h): gdouble planes from host or device memory, single values, clears ---- */
/* liblqr takes a bias before lqr_carver_init (the plane is part of the base layout, which exists from lqr_carver_new on); a rigidity
 * mask needs the initialised carver, as there (mask_prepare) */
static LqrRetVal bias_prepare(LqrCarver *r)
{
    if (r->root) return LQR_ERROR;
    if (lqr_geom_needs_flatten(&r->geo)) LQR_CATCH(lqr_carver_flatten(r));
    return LQR_OK;
}
static LqrRetVal mask_add_f(LqrCarver *r, const void *buffer, int depth, int on_device, int is_rig, int bias_factor, int width, int height,
                            int x_off, int y_off)
{
    if (!is_rig && bias_factor == 0) return LQR_OK;     /* liblqr: before anything else */
    LQR_CATCH(is_rig ? mask_prepare(r) : bias_prepare(r));
    LQR_CATCH(mask_queue_flush(r));
    HIP_CATCH(lqrhip_mask_add_f(r->dev, buffer, depth, on_device, width, height, x_off, y_off, r->geo.transposed, is_rig, bias_factor));
    if (is_rig) r->has_rigmask = 1; else r->has_bias = 1;
    r->wk_valid = 0;
    return LQR_OK;
}
LqrRetVal lqr_carver_bias_add_area(LqrCarver *r, gdouble *buffer, gint bias_factor, gint width, gint height, gint x_off, gint y_off)
{
    return mask_add_f(r, buffer, LQR_COLDEPTH_64F, 0, 0, bias_factor, width, height, x_off, y_off);
}
LqrRetVal lqr_carver_bias_add(LqrCarver *r, gdouble *buffer, gint bias_factor)
{
    return lqr_carver_bias_add_area(r, buffer, bias_factor, lqr_carver_get_width(r), lqr_carver_get_height(r), 0, 0);
}
LqrRetVal lqr_carver_bias_add_rgb(LqrCarver *r, guchar *rgb, gint bias_factor, gint channels)
{
    if (bias_factor == 0) return LQR_OK;
    LQR_CATCH(bias_prepare(r));
    LQR_CATCH(mask_queue_flush(r));
    HIP_CATCH(lqrhip_mask_add(r->dev, rgb, channels, lqr_carver_get_width(r), lqr_carver_get_height(r), 0, 0, r->geo.transposed, 0, bias_factor));
    r->has_bias = 1;
    r->wk_valid = 0;
    return LQR_OK;
}
LqrRetVal lqr_carver_rigmask_add_area(LqrCarver *r, gdouble *buffer, gint width, gint height, gint x_off, gint y_off)
{
    return mask_add_f(r, buffer, LQR_COLDEPTH_64F, 0, 1, 0, width, height, x_off, y_off);
}
LqrRetVal lqr_carver_rigmask_add(LqrCarver *r, gdouble *buffer)
{
    return lqr_carver_rigmask_add_area(r, buffer, lqr_carver_get_width(r), lqr_carver_get_height(r), 0, 0);
}
LqrRetVal lqr_carver_rigmask_add_rgb(LqrCarver *r, guchar *rgb, gint channels)
{
    return lqr_carver_rigmask_add_rgb_area(r, rgb, channels, lqr_carver_get_width(r), lqr_carver_get_height(r), 0, 0);
}
LqrRetVal lqrx_carver_bias_add_area_device(LqrCarver *r, const void *device_buffer, LqrColDepth depth, gint bias_factor, gint width, gint height,
                                           gint x_off, gint y_off)
{
    if (depth != LQR_COLDEPTH_32F && depth != LQR_COLDEPTH_64F) return LQR_ERROR;
    return mask_add_f(r, device_buffer, (int) depth, 1, 0, bias_factor, width, height, x_off, y_off);
}
LqrRetVal lqrx_carver_rigmask_add_area_device(LqrCarver *r, const void *device_buffer, LqrColDepth depth, gint width, gint height, gint x_off,
                                              gint y_off)
{
    if (depth != LQR_COLDEPTH_32F && depth != LQR_COLDEPTH_64F) return LQR_ERROR;
    return mask_add_f(r, device_buffer, (int) depth, 1, 1, 0, width, height, x_off, y_off);
}

/* One value: queued, not launched (a caller makes one call per pixel of its mask).  Only the first call of a run touches the device:
 * it flattens the carver and makes sure the plane exists.  The value goes to the device as the caller gave it; the conversion to
 * float and the halving happen in k_mask_scatter. */
static LqrRetVal mask_add_xy(LqrCarver *r, int is_rig, double v, int x, int y)
{
    LqrMaskQueue *q = &r->mq[is_rig];
    int rc, index;
    if (!q->n) {
        LQR_CATCH(is_rig ? mask_prepare(r) : bias_prepare(r));
        if (x < 0 || y < 0 || x >= lqr_carver_get_width(r) || y >= lqr_carver_get_height(r)) return LQR_ERROR;
        HIP_CATCH(lqrhip_mask_plane_ensure(r->dev, is_rig));
        if (is_rig) r->has_rigmask = 1; else r->has_bias = 1;
        r->wk_valid = 0;
    } else if (x < 0 || y < 0 || x >= lqr_carver_get_width(r) || y >= lqr_carver_get_height(r))
        return LQR_ERROR;
    index = r->geo.transposed ? x * r->geo.w0 + y : y * r->geo.w0 + x;
    rc = lqr_maskq_append(q, (size_t) r->geo.w0 * r->geo.h0, index, v);
    if (rc == LQR_MASKQ_FULL) {         /* the bound: an early flush */
        LQR_CATCH(mask_queue_flush_one(r, is_rig));
        rc = lqr_maskq_append(q, (size_t) r->geo.w0 * r->geo.h0, index, v);
    }
    return rc == LQR_MASKQ_OK ? LQR_OK : rc == LQR_MASKQ_NOMEM ? LQR_NOMEM : LQR_ERROR;
}
LqrRetVal lqr_carver_bias_add_xy(LqrCarver *r, gdouble bias, gint x, gint y)
{
    if (bias == 0) return LQR_OK;
    return mask_add_xy(r, 0, bias, x, y);
}
LqrRetVal lqr_carver_rigmask_add_xy(LqrCarver *r, gdouble rigidity, gint x, gint y) { return mask_add_xy(r, 1, rigidity, x, y); }

/* the plane goes, with what was queued for it: same_config groups the carver with unmasked ones again */
static void mask_clear(LqrCarver *r, int is_rig)
{
    lqr_maskq_reset(&r->mq[is_rig]);
    (void) hip_ret(lqrhip_mask_clear(r->dev, is_rig));
    if (is_rig) r->has_rigmask = 0; else r->has_bias = 0;
    r->wk_valid = 0;
}
void lqr_carver_bias_clear(LqrCarver *r) { mask_clear(r, 0); }
void lqr_carver_rigmask_clear(LqrCarver *r) { mask_clear(r, 1); }

static LqrRetVal mask_read(LqrCarver *r, int is_rig, gfloat *out)
{
    LQR_CATCH(mask_queue_flush(r));
    if (lqr_geom_needs_flatten(&r->geo)) return LQR_ERROR;     /* flat carvers only */
    HIP_CATCH(lqrhip_read_mask_plane(r->dev, is_rig, r->geo.transposed, out));
    return LQR_OK;
}
LqrRetVal lqrx_carver_get_bias(LqrCarver *r, gfloat *out) { return mask_read(r, 0, out); }
LqrRetVal lqrx_carver_get_rigmask(LqrCarver *r, gfloat *out) { return mask_read(r, 1, out); }

/* ======================= per-seam loop (E10) ============================= */
static LqrRetVal take_debug_snapshot(LqrCarver *r)
{
    size_t n = (size_t) r->geo.w * r->geo.h;
    free(r->dbg_en); free(r->dbg_m); free(r->dbg_least);
    r->dbg_w = r->geo.w; r->dbg_h = r->geo.h;
    r->dbg_en = (float *) malloc(n * sizeof(float));
    r->dbg_m = (float *) malloc(n * sizeof(float));
    r->dbg_least = (int *) malloc(n * sizeof(int));
    if (!r->dbg_en || !r->dbg_m || !r->dbg_least) return LQR_NOMEM;
    HIP_CATCH(lqrhip_read_working(r->dev, r->geo.w, r->geo.h, r->dbg_en, r->dbg_m, r->dbg_least));
    HIP_CATCH(lqrhip_read_seam_flags(r->dev, &r->dbg_org, &r->dbg_org_prev, &r->dbg_side));
    return LQR_OK;
}

/* the seam loop of one session and its commit; what happens at which seam is the session's schedule (lqr_sched.h) */
static LqrRetVal group_build_vsmap(Group *g, const LqrSession *s, int *reported)
{
    LqrCarver *r0 = g->r[0];
    LqrHipDpParams p;
    int l, i;
    dp_params(r0, &p);
    HIP_ALL(g, lqrhip_seam_log_reserve(B, s->n_seams, r0->geo.h));

    for (l = s->max_level; l < s->depth; l++) {
        const int lr_pick = r0->leftright;
        LqrSeam seam;
        lqr_session_seam(s, l, &seam);
        if (seam.report && r0->progress && r0->progress->update) {
            /* report completed work, not enqueued work (a session that is being redone does not report twice) */
            HIP_ALL(g, lqrhip_batch_sync(B));
            if (l > *reported) {
                r0->progress->update(seam.fraction);
                *reported = l;
            }
            CANCEL_POINT(g);        /* a cancel from the callback, or during it: nothing is queued here */
        }
        CANCEL_POINT(g);
        if (seam.full)
            for (i = 0; i < g->n; i++) g->r[i]->leftright ^= 1;
        HIP_ALL(g, lqrhip_seam_step(B, &p, seam.w_before, r0->geo.h, l - s->max_level, lr_pick, seam.full, r0->leftright));
        for (i = 0; i < g->n; i++) { g->r[i]->geo.level++; g->r[i]->geo.w--; }
    }

    if (g_debug_snapshot)
        for (i = 0; i < g->n; i++) LQR_CATCH(take_debug_snapshot(g->r[i]));

    /* the seam loop is over: nothing of it is committed to the base layout before its kernels have all ended without a device-side
     * failure and the seam log has passed its self-check */
    /* (the last check point of lqr_carver_cancel in a session: from here on the session commits and inflates to its end) */
    T_BEGIN(T_TAIL);
    HIP_ALL(g, lqrhip_session_check(B, r0->geo.h, s->wc0, s->n_seams, r0->delta_x));
    HIP_ALL(g, lqrhip_batch_sync(B));
    HIP_ALL(g, lqrhip_vs_commit(B, r0->geo.w0, r0->geo.h0, s->wc0, s->n_seams, s->first_level, s->finish));
    /* inflate (E14): every seam of this session is doubled in the base layout */
    for (i = 0; i < g->n; i++) (void) lqr_state_phase(&g->r[i]->state, LQR_STATE_INFLATING);
    HIP_ALL(g, lqrhip_inflate(B, r0->geo.w0, r0->geo.h0, s->depth - 1, s->max_level));      /* every sub-batch staged and checked ... */
    HIP_ALL(g, lqrhip_planes_commit(B));                                                    /* ... before any adopts its inflated layout */
    T_END(T_TAIL);
    FOR_TREE(g, i, r, {
        lqr_geom_session_done(&r->geo, s->depth, s->n_seams);
        ro_invalidate(r);
    });
    return LQR_OK;
}

/* one session: (re)lay the working planes out if needed, energy, DP, the seam loop, commit, inflate */
static LqrRetVal session_run(Group *g, const LqrSession *s, int redo, int *reported)
{
    LqrCarver *r0 = g->r[0];
    LqrHipDpParams p;
    int i;
    LQR_CATCH(group_phase(g, LQR_STATE_RESIZING));
    for (i = 0; i < g->n; i++) set_width_one(g->r[i], s->wc0);    /* the carved frame */
    dp_params(r0, &p);
    if (!r0->wk_valid || redo) {
        /* a flat carver: identity, and the energy in the same pass over the planes; a multi-size image (a redone deeper session,
         * working planes lost in a failed one): the pixels of the base layout without a level, in order */
        const int from_visible = (r0->geo.max_level != 1 || r0->geo.w0 != r0->geo.w_start);
        if (from_visible) HIP_ALL(g, lqrhip_wk_init(B, 1));
        else HIP_ALL(g, lqrhip_wk_init_emap(B, &p, r0->geo.w, r0->geo.h));
        for (i = 0; i < g->n; i++) g->r[i]->wk_valid = 1;
        if (from_visible) HIP_ALL(g, lqrhip_emap_build(B, &p, r0->geo.w, r0->geo.h));
    } else
        HIP_ALL(g, lqrhip_emap_build(B, &p, r0->geo.w, r0->geo.h));
    HIP_ALL(g, lqrhip_mmap_build(B, &p, r0->geo.w, r0->geo.h, r0->leftright));
    return group_build_vsmap(g, s, reported);
}

static LqrRetVal group_build_maps(Group *g, int depth)
{
    LqrCarver *r0 = g->r[0];
    LqrSession s;
    LqrRetVal ret;
    int i, k, reported = -1, *snap;
    if (depth <= r0->geo.max_level) return LQR_OK;
    if (!r0->active || r0->root) return LQR_ERROR;
    lqr_session_begin(&s, r0->geo.max_level, depth, r0->geo.w_start - r0->geo.max_level + 1, r0->lr_switch_frequency, r0->session_rescale_current,
                      r0->session_rescale_total, r0->session_update_step);
    /* what a session changes on the host before it succeeds: the roots' width, level and side */
    snap = (int *) malloc((size_t) g->n * 3 * sizeof *snap);
    if (!snap) return LQR_NOMEM;
    for (i = 0; i < g->n; i++) { snap[3 * i] = g->r[i]->geo.w; snap[3 * i + 1] = g->r[i]->geo.level; snap[3 * i + 2] = g->r[i]->leftright; }
    g_last_rc = 0;
    ret = session_run(g, &s, 0, &reported);
    for (k = 0; k < 2 && ret != LQR_OK; k++) {
        const int fault = (ret == LQR_ERROR && g_last_rc == LQRHIP_EFAULT);
        /* a cancelled session (lqr_control.h) is a failed one that is not carved again: nothing more is enqueued, what was runs out,
         * nothing of it was committed (the last check point lies before the self-check), the bookkeeping goes back */
        const int cancelled = (ret == LQR_USRCANCEL);
        /* the carver as it was before the session: the base layout (levels of this session removed if they were committed),
         * the bookkeeping; the working planes are gone */
        /* (also after an allocation failure: the staging of the inflate pass comes after the commit of the session's levels) */
        if (fault || cancelled || g_last_rc == LQRHIP_ENOMEM)
            for (i = 0; i < g->nb; i++) (void) lqrhip_session_rollback(g->b[i], r0->geo.w0, r0->geo.h0, s.first_level, s.finish);
        for (i = 0; i < g->n; i++) {
            LqrCarver *c = g->r[i];
            c->geo.w = snap[3 * i]; c->geo.level = snap[3 * i + 1]; c->leftright = snap[3 * i + 2];
            c->wk_valid = 0;
            ro_invalidate(c);
        }
        if (!fault || !lqrhip_get_recovery() || k == 1) break;
        fprintf(stderr, "liblqr-hip: the session is carved again on the kernels without spin waits\n");
        for (i = 0; i < g->nb; i++) lqrhip_batch_set_safe(g->b[i], 1);
        g_last_rc = 0;
        ret = session_run(g, &s, 1, &reported);
        for (i = 0; i < g->nb; i++) lqrhip_batch_set_safe(g->b[i], 0);
    }
    free(snap);
    return ret;
}

/* ======================= vmaps (E12) ===================================== */
LqrVMap *lqr_vmap_dump(LqrCarver *r)
{
    LqrVMap *v;
    int w = r->geo.w_start, h = r->geo.h, depth = r->geo.w0 - r->geo.w_start, x, y;
    int *frame, *buffer;
    frame = (int *) malloc((size_t) w * h * sizeof(int));
    v = (LqrVMap *) calloc(1, sizeof *v);
    if (!frame || !v) { free(frame); free(v); return NULL; }
    if (lqrhip_read_vmap(r->dev, r->geo.w0, r->geo.h0, w, r->geo.w0 - w + 1, depth, frame) != 0) {
        fprintf(stderr, "liblqr-hip: vmap read-back failed: %s\n", lqrhip_last_error());
        free(frame); free(v);
        return NULL;
    }
    if (r->geo.transposed) {    /* hand the map back in image orientation */
        buffer = (int *) malloc((size_t) w * h * sizeof(int));
        if (!buffer) { free(frame); free(v); return NULL; }
        for (y = 0; y < h; y++)
            for (x = 0; x < w; x++) buffer[(size_t) x * h + y] = frame[(size_t) y * w + x];
        free(frame);
    } else {
        buffer = frame;
    }
    v->buffer = buffer;
    v->width = lqr_carver_get_ref_width(r);
    v->height = lqr_carver_get_ref_height(r);
    v->depth = depth;
    v->orientation = r->geo.transposed;
    return v;
}

/* lqr_vmap.h: the carver's map as it stands, appended to the carver's own list (what lqr_carver_set_dump_vmaps makes every resize do) */
LqrRetVal lqr_vmap_internal_dump(LqrCarver *r)
{
    LqrVMap *v = lqr_vmap_dump(r);
    LqrVMapList *n = (LqrVMapList *) calloc(1, sizeof *n);
    if (!v || !n) return LQR_NOMEM;
    n->current = v;
    LIST_APPEND(LqrVMapList, r->flushed_vs, n);
    return LQR_OK;
}

/* ======================= vmap load (lqr_vmap.h) ========================== */
static int same_config(const LqrCarver *a, const LqrCarver *b);
/* One map onto n root carvers of its size that lqr_carver_init has not seen.  Everything that can refuse the call is decided before a
 * carver changes: the arguments and sizes here, the map's contents on the device (lqrhip_vmap_stage).  Then: flatten if the carvers
 * were resized since their last load, transpose if the map lies the other way, and the inflate pass of the whole tree with the map as
 * every carver's levels, staged on every sub-batch before any commits.  The bookkeeping is group_build_vsmap's after its inflate. */
static LqrRetVal group_vmap_load_entered(LqrCarver **rs, int n, const gint *map, int on_device, int width, int height, int depth, int orientation);
static LqrRetVal group_vmap_load(LqrCarver **rs, int n, const gint *map, int on_device, int width, int height, int depth, int orientation)
{
    LqrRetVal ret;
    int i;
    if (n < 1 || !rs || !map || (orientation != 0 && orientation != 1)) return LQR_ERROR;
    for (i = 0; i < n; i++)
        if (!rs[i] || rs[i]->root || rs[i]->active) return LQR_ERROR;
    for (i = 1; i < n; i++)
        if (!same_config(rs[0], rs[i])) return LQR_ERROR;
    LQR_CATCH(roots_enter(rs, n, LQR_STATE_RESIZING));
    ret = group_vmap_load_entered(rs, n, map, on_device, width, height, depth, orientation);
    roots_leave(rs, n);
    return ret;
}
static LqrRetVal group_vmap_load_entered(LqrCarver **rs, int n, const gint *map, int on_device, int width, int height, int depth, int orientation)
{
    Group g;
    LqrHipVMap *staged = NULL;
    LqrRetVal ret = LQR_OK;
    int i, rc;
    for (i = 0; i < n; i++) LQR_CATCH(mask_queue_flush(rs[i]));
    if (lqr_carver_get_width(rs[0]) != width || lqr_carver_get_height(rs[0]) != height) {
        fprintf(stderr, "liblqr-hip: lqr_vmap_load refused: a %d x %d map on a carver that is %d x %d now\n", width, height,
                lqr_carver_get_width(rs[0]), lqr_carver_get_height(rs[0]));
        return LQR_ERROR;
    }
    if (depth < 1 || depth >= (orientation ? height : width) || (orientation ? height : width) > LQRHIP_MAX_FRAME_WIDTH) {
        fprintf(stderr, "liblqr-hip: lqr_vmap_load refused: depth %d on lines of %d (0 < depth < line length <= %d)\n", depth,
                orientation ? height : width, LQRHIP_MAX_FRAME_WIDTH);
        return LQR_ERROR;
    }
    LQR_CATCH(group_open(&g, rs, n));
    rc = lqrhip_vmap_stage(map, on_device, width, height, depth, orientation, &staged);
    if (rc == LQRHIP_EMAP) {        /* a bad argument, not a device error: said once, nothing has changed */
        fprintf(stderr, "liblqr-hip: lqr_vmap_load refused: %s\n", lqrhip_last_error());
        ret = LQR_ERROR;
    } else
        ret = hip_ret(rc);
    if (ret == LQR_OK) ret = group_flatten(&g);
    if (ret == LQR_OK && rs[0]->geo.transposed != orientation) ret = group_transpose(&g);
    if (ret == LQR_OK) {
        int k;
        for (k = 0; k < g.nb && ret == LQR_OK; k++) ret = hip_ret(lqrhip_vmap_load(g.b[k], staged));     /* every sub-batch staged ... */
        for (k = 0; k < g.nb && ret == LQR_OK; k++) ret = hip_ret(lqrhip_planes_commit(g.b[k]));         /* ... before any adopts */
    }
    if (ret == LQR_OK) {
        FOR_TREE(&g, i, r, {
            lqr_geom_map_loaded(&r->geo, depth);
            ro_invalidate(r);
            r->enl_step = 2.0f;
            r->wk_valid = 0;
        });
    } else if (rc != LQRHIP_EMAP) {
        int k;
        for (k = 0; k < g.nb; k++) lqrhip_batch_abort(g.b[k]);          /* nothing staged may surface later */
    }
    lqrhip_vmap_release(staged);
    group_close(&g);
    return ret;
}

LqrRetVal lqr_vmap_load(LqrCarver *r, LqrVMap *vmap)
{
    if (!r || !vmap) return LQR_ERROR;
    return group_vmap_load(&r, 1, vmap->buffer, 0, vmap->width, vmap->height, vmap->depth, vmap->orientation);
}
LqrRetVal lqrx_vmap_load_device(LqrCarver *r, const gint *device_map, gint width, gint height, gint depth, gint orientation)
{
    if (!r) return LQR_ERROR;
    return group_vmap_load(&r, 1, device_map, 1, width, height, depth, orientation);
}
LqrRetVal lqrx_vmap_load_batch(LqrCarver **carvers, gint n, LqrVMap *vmap)
{
    if (!vmap) return LQR_ERROR;
    return group_vmap_load(carvers, n, vmap->buffer, 0, vmap->width, vmap->height, vmap->depth, vmap->orientation);
}

/* ======================= forward-energy seam maps (lqr_forward.h) ========= */
/* Only the up-front checks and the composition live here: the seams are found by k_forward.hip behind lqrhip_forward_*, the map is
 * loaded by group_vmap_load_entered like any other. */
#define FWD_SLICE_SEAMS 16      /* seams enqueued between two looks at the state word (lqr_carver_cancel) */

/* what refuses a map call before any device work; *len: the line length L */
static LqrRetVal forward_check(LqrCarver *const *rs, int n, int depth, int orientation, const char *who, int *len)
{
    int i, L, H;
    const char *why = NULL;
    if (!rs || n < 1 || (orientation != 0 && orientation != 1)) why = "NULL or bad arguments";
    else if (n > LQRHIP_FORWARD_MAX_LINES) why = "more carvers than one build takes";
    for (i = 0; !why && i < n; i++) {
        if (!rs[i]) why = "NULL carver";
        else if (rs[i]->root) why = "an attached carver follows its root";
        else if (i && !same_config(rs[0], rs[i])) why = "the carvers are not of one configuration";
    }
    if (why) { fprintf(stderr, "liblqr-hip: %s refused: %s\n", who, why); return LQR_ERROR; }
    L = orientation ? lqr_carver_get_height(rs[0]) : lqr_carver_get_width(rs[0]);
    H = orientation ? lqr_carver_get_width(rs[0]) : lqr_carver_get_height(rs[0]);
    if (depth < 1 || depth >= L || L > LQRHIP_MAX_FRAME_WIDTH || H > LQRHIP_FORWARD_MAX_LINES) {
        fprintf(stderr, "liblqr-hip: %s refused: depth %d on %d lines of %d (0 < depth < line length <= %d, at most %d lines)\n", who, depth, H, L,
                LQRHIP_MAX_FRAME_WIDTH, LQRHIP_FORWARD_MAX_LINES);
        return LQR_ERROR;
    }
    *len = L;
    return LQR_OK;
}

/* the slices of a build, a check point in front of each */
static LqrRetVal forward_slices(LqrCarver *const *rs, int n, LqrHipForward *f, int depth)
{
    int first, i;
    for (first = 0; first < depth; first += FWD_SLICE_SEAMS) {
        for (i = 0; i < n; i++)
            if (lqr_state_check(&rs[i]->state)) return LQR_USRCANCEL;
        HIP_CATCH(lqrhip_forward_seams(f, first, MINI(FWD_SLICE_SEAMS, depth - first)));
    }
    for (i = 0; i < n; i++)
        if (lqr_state_check(&rs[i]->state)) return LQR_USRCANCEL;
    HIP_CATCH(lqrhip_forward_finish(f));
    return LQR_OK;
}

/* Inside the call (roots_enter): flatten what is not flat, then the build.  device_maps NULL: the build keeps the maps.  On LQR_OK *out
 * holds the finished build, which the caller releases; otherwise nothing is left */
static LqrRetVal forward_build_entered(LqrCarver **rs, int n, int depth, int orientation, int L, gint *const *device_maps, LqrHipForward **out)
{
    LqrHipCarver **ds;
    LqrHipForward *f = NULL;
    LqrRetVal ret;
    int i;
    *out = NULL;
    for (i = 0; i < n; i++) LQR_CATCH(mask_queue_flush(rs[i]));
    if (!lqr_geom_is_flat(&rs[0]->geo)) {
        Group g;
        LQR_CATCH(group_open(&g, rs, n));
        ret = group_flatten(&g);
        if (ret != LQR_OK) { int k; for (k = 0; k < g.nb; k++) lqrhip_batch_abort(g.b[k]); }
        group_close(&g);
        LQR_CATCH(ret);
    }
    for (i = 0; i < n; i++)
        if (lqr_state_check(&rs[i]->state)) return LQR_USRCANCEL;
    ds = (LqrHipCarver **) malloc((size_t) n * sizeof *ds);
    if (!ds) return LQR_NOMEM;
    for (i = 0; i < n; i++) ds[i] = rs[i]->dev;
    ret = hip_ret(lqrhip_forward_begin(ds, n, depth, orientation, rs[0]->geo.transposed,
                                       rs[0]->nrg_func >= LQR_EF_LUMA_GRAD_NORM && rs[0]->nrg_func <= LQR_EF_LUMA_GRAD_XABS, L,
                                       (void *const *) device_maps, &f));
    free(ds);
    if (ret == LQR_OK) ret = forward_slices(rs, n, f, depth);
    if (ret != LQR_OK) { lqrhip_forward_release(f); return ret; }
    *out = f;
    return LQR_OK;
}

static LqrRetVal forward_maps(LqrCarver **rs, int n, int depth, int orientation, gint *const *device_maps, const char *who)
{
    LqrHipForward *f;
    LqrRetVal ret;
    int i, L;
    LQR_CATCH(forward_check(rs, n, depth, orientation, who, &L));
    for (i = 0; device_maps && i < n; i++)
        if (!device_maps[i]) device_maps = NULL;
    if (!device_maps) { fprintf(stderr, "liblqr-hip: %s refused: NULL map\n", who); return LQR_ERROR; }
    LQR_CATCH(roots_enter(rs, n, LQR_STATE_RESIZING));
    ret = forward_build_entered(rs, n, depth, orientation, L, device_maps, &f);
    if (ret == LQR_OK) lqrhip_forward_release(f);
    roots_leave(rs, n);
    return ret;
}
LqrRetVal lqrx_carver_forward_map_device(LqrCarver *r, gint depth, gint orientation, gint *device_map)
{
    return forward_maps(&r, 1, depth, orientation, &device_map, "lqrx_carver_forward_map_device");
}
LqrRetVal lqrx_carver_forward_maps_device(LqrCarver **carvers, gint n, gint depth, gint orientation, gint *const *device_maps)
{
    return forward_maps(carvers, n, depth, orientation, device_maps, "lqrx_carver_forward_maps_device");
}

LqrVMap *lqrx_carver_forward_map(LqrCarver *r, gint depth, gint orientation)
{
    LqrHipForward *f;
    LqrVMap *v = NULL;
    gint *buffer;
    int L, width, height;
    if (forward_check(&r, 1, depth, orientation, "lqrx_carver_forward_map", &L) != LQR_OK) return NULL;
    if (roots_enter(&r, 1, LQR_STATE_RESIZING) != LQR_OK) return NULL;
    width = lqr_carver_get_width(r); height = lqr_carver_get_height(r);
    buffer = (gint *) malloc((size_t) width * height * sizeof *buffer);
    if (buffer && forward_build_entered(&r, 1, depth, orientation, L, NULL, &f) == LQR_OK) {
        if (hip_ret(lqrhip_forward_read_map(f, 0, buffer)) == LQR_OK) v = lqr_vmap_new(buffer, width, height, depth, orientation);
        lqrhip_forward_release(f);
    }
    if (!v) free(buffer);
    roots_leave(&r, 1);
    return v;
}

LqrRetVal lqrx_carver_load_forward(LqrCarver *r, gint depth, gint orientation)
{
    LqrHipForward *f;
    LqrRetVal ret;
    int L;
    LQR_CATCH(forward_check(&r, 1, depth, orientation, "lqrx_carver_load_forward", &L));
    LQR_CATCH(roots_enter(&r, 1, LQR_STATE_RESIZING));
    ret = forward_build_entered(&r, 1, depth, orientation, L, NULL, &f);
    if (ret == LQR_OK) {
        /* (the map lies in the build's device memory until the load has committed) */
        ret = group_vmap_load_entered(&r, 1, lqrhip_forward_map(f, 0), 1, lqr_carver_get_width(r), lqr_carver_get_height(r), depth, orientation);
        lqrhip_forward_release(f);
    }
    roots_leave(&r, 1);
    return ret;
}

LqrRetVal lqrx_carver_resize_forward(LqrCarver *r, gint w1, gint h1)
{
    int w, h, dir, k;
    if (!r || r->root || w1 < 1 || h1 < 1) return LQR_ERROR;
    w = lqr_carver_get_width(r); h = lqr_carver_get_height(r);
    /* both directions are decided before either changes anything: no line has |change| seams, no frame is wider than the engine's */
    /* (the second direction's lines are as many as the first leaves: max(., .) covers both orders) */
    if (abs(w1 - w) >= w || abs(h1 - h) >= h || (w1 != w && w > LQRHIP_MAX_FRAME_WIDTH) || (h1 != h && h > LQRHIP_MAX_FRAME_WIDTH) ||
        (w1 != w && MAXI(h, h1) > LQRHIP_FORWARD_MAX_LINES) || (h1 != h && MAXI(w, w1) > LQRHIP_FORWARD_MAX_LINES)) {
        fprintf(stderr, "liblqr-hip: lqrx_carver_resize_forward refused: %d x %d to %d x %d (a change below the line length, lines of at most %d, "
                "at most %d of them)\n", w, h, w1, h1, LQRHIP_MAX_FRAME_WIDTH, LQRHIP_FORWARD_MAX_LINES);
        return LQR_ERROR;
    }
    for (k = 0; k < 2; k++) {
        dir = (r->resize_order == LQR_RES_ORDER_HOR) ? k : 1 - k;       /* 0: the width */
        w = lqr_carver_get_width(r); h = lqr_carver_get_height(r);
        if ((dir ? h1 - h : w1 - w) == 0) continue;
        LQR_CATCH(lqrx_carver_load_forward(r, abs(dir ? h1 - h : w1 - w), dir));
        LQR_CATCH(lqr_carver_resize(r, dir ? w : w1, dir ? h1 : h));
    }
    return LQR_OK;
}

/* test hook (lqr_hip.h): the I plane a build would form for a flat carver, H lines of L floats in the frame of `orientation` */
int lqrhip_read_forward_intensity(const void *carver, int orientation, float *out)
{
    const LqrCarver *r = (const LqrCarver *) carver;
    if (!r || r->root || !out || !lqr_geom_is_flat(&r->geo)) return LQRHIP_EARG;
    return lqrhip_forward_intensity(r->dev, orientation, r->geo.transposed,
                                    r->nrg_func >= LQR_EF_LUMA_GRAD_NORM && r->nrg_func <= LQR_EF_LUMA_GRAD_XABS, out);
}

/* ======================= static seams for a clip (lqr_static.h) ========== */
/* The up-front checks and the composition: the fold runs in k_static.hip behind lqrhip_static_*, the seams are found by an LQR_EF_NULL
 * carver of this file's own API, and the map is loaded by group_vmap_load_entered like any other. */

/* what refuses a call before any device work.  depth 0: an energy call, which has no depth, delta_x or line length to refuse */
static LqrRetVal static_check(LqrCarver *const *rs, int n, int depth, int orientation, float alpha, int delta_x, int with_map, const char *who)
{
    int i, L;
    const char *why = NULL;
    if (!rs) why = "NULL frames";
    else if (n < 1 || n > LQRHIP_STATIC_MAX_FRAMES) why = "1 .. 65535 frames";
    else if (orientation != 0 && orientation != 1) why = "orientation is 0 or 1";
    else if (!(alpha >= 0.0f && alpha <= 1.0f)) why = "alpha lies in [0, 1]";
    else if (with_map && (delta_x < 0 || delta_x > LQRHIP_MAX_DELTA)) why = "delta_x is 0 .. 16, what lqr_carver_init takes";
    for (i = 0; !why && i < n; i++) {
        if (!rs[i]) why = "NULL frame";
        else if (rs[i]->root) why = "an attached carver follows its root";
        else if (i && !same_config(rs[0], rs[i])) why = "the frames are not of one configuration";
    }
    if (why) { fprintf(stderr, "liblqr-hip: %s refused: %s\n", who, why); return LQR_ERROR; }
    if (!with_map) return LQR_OK;
    L = orientation ? lqr_carver_get_height(rs[0]) : lqr_carver_get_width(rs[0]);
    if (depth < 1 || depth >= L || L > LQRHIP_MAX_FRAME_WIDTH) {
        fprintf(stderr, "liblqr-hip: %s refused: depth %d on lines of %d (0 < depth < line length <= %d)\n", who, depth, L, LQRHIP_MAX_FRAME_WIDTH);
        return LQR_ERROR;
    }
    return LQR_OK;
}

static int roots_cancelled(LqrCarver *const *rs, int n)
{
    int i;
    for (i = 0; i < n; i++)
        if (lqr_state_check(&rs[i]->state)) return 1;
    return 0;
}

/* Inside the call (roots_enter): flatten what is not flat, then the fold.  E goes to device_energy (device memory) if that is given
 * and to host_energy if that is; with neither the fold keeps it.  On LQR_OK *out holds the finished fold, which the caller releases */
static LqrRetVal static_fold_entered(LqrCarver **rs, int n, int orientation, float alpha, float *device_energy, float *host_energy, LqrHipStatic **out)
{
    LqrHipCarver **ds;
    LqrHipStatic *st = NULL;
    LqrRetVal ret;
    int i, groups;
    *out = NULL;
    if (roots_cancelled(rs, n)) return LQR_USRCANCEL;
    for (i = 0; i < n; i++) LQR_CATCH(mask_queue_flush(rs[i]));
    if (!lqr_geom_is_flat(&rs[0]->geo)) {
        Group g;
        LQR_CATCH(group_open(&g, rs, n));
        ret = group_flatten(&g);
        if (ret != LQR_OK) { int k; for (k = 0; k < g.nb; k++) lqrhip_batch_abort(g.b[k]); }
        group_close(&g);
        LQR_CATCH(ret);
    }
    ds = (LqrHipCarver **) malloc((size_t) n * sizeof *ds);
    if (!ds) return LQR_NOMEM;
    for (i = 0; i < n; i++) ds[i] = rs[i]->dev;
    ret = hip_ret(lqrhip_static_begin(ds, n, orientation, rs[0]->geo.transposed, rs[0]->nrg_func, alpha, device_energy, &st));
    free(ds);
    groups = ret == LQR_OK ? lqrhip_static_groups(st) : 0;
    for (i = 0; ret == LQR_OK && i < groups; i++) {
        if (roots_cancelled(rs, n)) ret = LQR_USRCANCEL;
        else ret = hip_ret(lqrhip_static_fold(st));
    }
    if (ret == LQR_OK) ret = hip_ret(lqrhip_static_finish(st, host_energy));
    if (ret != LQR_OK) { lqrhip_static_release(st); return ret; }
    *out = st;
    return LQR_OK;
}

static LqrRetVal static_energy(LqrCarver **rs, int n, int orientation, float alpha, float *device_energy, float *host_energy, const char *who)
{
    LqrHipStatic *st;
    LqrRetVal ret;
    LQR_CATCH(static_check(rs, n, 0, orientation, alpha, 0, 0, who));
    if (!device_energy && !host_energy) { fprintf(stderr, "liblqr-hip: %s refused: NULL energy\n", who); return LQR_ERROR; }
    LQR_CATCH(roots_enter(rs, n, LQR_STATE_RESIZING));
    ret = static_fold_entered(rs, n, orientation, alpha, device_energy, host_energy, &st);
    if (ret == LQR_OK) lqrhip_static_release(st);
    roots_leave(rs, n);
    return ret;
}
LqrRetVal lqrx_carvers_static_energy_device(LqrCarver **frames, gint n, gint orientation, gfloat alpha, gfloat *device_energy)
{
    return static_energy(frames, n, orientation, alpha, device_energy, NULL, "lqrx_carvers_static_energy_device");
}
LqrRetVal lqrx_carvers_static_energy(LqrCarver **frames, gint n, gint orientation, gfloat alpha, gfloat *energy)
{
    return static_energy(frames, n, orientation, alpha, NULL, energy, "lqrx_carvers_static_energy");
}

/* Inside the call: the fold, then the key carver -- an LQR_EF_NULL carver on a plane of zeros whose bias plane is E -- carved by `depth`
 * seams, its map dumped.  The key carver is destroyed on every path.  (Its resize is a call of its own and is not interrupted.) */
static LqrRetVal static_map_entered(LqrCarver **rs, int n, int depth, int orientation, float alpha, int delta_x, float rigidity, LqrVMap **out)
{
    LqrHipStatic *st;
    LqrCarver *key;
    guchar *zeros;
    LqrRetVal ret;
    const int w = lqr_carver_get_width(rs[0]), h = lqr_carver_get_height(rs[0]);
    *out = NULL;
    LQR_CATCH(static_fold_entered(rs, n, orientation, alpha, NULL, NULL, &st));
    zeros = (guchar *) calloc((size_t) w * h, 1);
    key = zeros ? lqr_carver_new(zeros, w, h, 1) : NULL;        /* (the carver owns `zeros` from here) */
    if (!key) { free(zeros); lqrhip_static_release(st); return LQR_NOMEM; }
    ret = lqr_carver_set_energy_function_builtin(key, LQR_EF_NULL);
    if (ret == LQR_OK) ret = lqrx_carver_bias_add_area_device(key, lqrhip_static_energy(st), LQR_COLDEPTH_32F, 2, w, h, 0, 0);
    lqrhip_static_release(st);          /* (the bias plane holds E now) */
    if (ret == LQR_OK) ret = lqr_carver_init(key, delta_x, rigidity);
    if (ret == LQR_OK && roots_cancelled(rs, n)) ret = LQR_USRCANCEL;
    if (ret == LQR_OK) ret = lqr_carver_resize(key, orientation ? w : w - depth, orientation ? h - depth : h);
    if (ret == LQR_OK && roots_cancelled(rs, n)) ret = LQR_USRCANCEL;
    if (ret == LQR_OK && !(*out = lqr_vmap_dump(key))) ret = LQR_NOMEM;
    lqr_carver_destroy(key);
    return ret;
}

LqrVMap *lqrx_carvers_static_map(LqrCarver **frames, gint n, gint depth, gint orientation, gfloat alpha, gint delta_x, gfloat rigidity)
{
    LqrVMap *v = NULL;
    if (static_check(frames, n, depth, orientation, alpha, delta_x, 1, "lqrx_carvers_static_map") != LQR_OK) return NULL;
    if (roots_enter(frames, n, LQR_STATE_RESIZING) != LQR_OK) return NULL;
    (void) static_map_entered(frames, n, depth, orientation, alpha, delta_x, rigidity, &v);
    roots_leave(frames, n);
    return v;
}

LqrRetVal lqrx_carvers_load_static(LqrCarver **frames, gint n, gint depth, gint orientation, gfloat alpha, gint delta_x, gfloat rigidity)
{
    LqrVMap *v;
    LqrRetVal ret;
    LQR_CATCH(static_check(frames, n, depth, orientation, alpha, delta_x, 1, "lqrx_carvers_load_static"));
    LQR_CATCH(roots_enter(frames, n, LQR_STATE_RESIZING));
    ret = static_map_entered(frames, n, depth, orientation, alpha, delta_x, rigidity, &v);
    if (ret == LQR_OK) {
        /* (the key carver's map travels through host memory: lqr_static.h) */
        ret = group_vmap_load_entered(frames, n, v->buffer, 0, v->width, v->height, v->depth, v->orientation);
        lqr_vmap_destroy(v);
    }
    roots_leave(frames, n);
    return ret;
}

LqrRetVal lqrx_carvers_resize_static(LqrCarver **frames, gint n, gint w1, gint h1, gfloat alpha, gint delta_x, gfloat rigidity)
{
    int w, h, dir, k;
    LQR_CATCH(static_check(frames, n, 0, 0, alpha, delta_x, 0, "lqrx_carvers_resize_static"));
    w = lqr_carver_get_width(frames[0]); h = lqr_carver_get_height(frames[0]);
    /* both directions are decided before either changes anything: no line has |change| seams, no carved frame is wider than the engine's */
    if (delta_x < 0 || delta_x > LQRHIP_MAX_DELTA || w1 < 1 || h1 < 1 || abs(w1 - w) >= w || abs(h1 - h) >= h || (w1 != w && w > LQRHIP_MAX_FRAME_WIDTH) ||
        (h1 != h && h > LQRHIP_MAX_FRAME_WIDTH)) {
        fprintf(stderr, "liblqr-hip: lqrx_carvers_resize_static refused: %d x %d to %d x %d, delta_x %d (a change below the line length, lines of at "
                "most %d, delta_x 0 .. %d)\n", w, h, w1, h1, delta_x, LQRHIP_MAX_FRAME_WIDTH, LQRHIP_MAX_DELTA);
        return LQR_ERROR;
    }
    /* the state word is entered here too (the calls below enter it for themselves): a resize to the size the frames have skips both
     * directions, and must still refuse a frame that is marked cancelled or inside another call */
    LQR_CATCH(roots_enter(frames, n, LQR_STATE_RESIZING));
    roots_leave(frames, n);
    for (k = 0; k < 2; k++) {
        dir = (frames[0]->resize_order == LQR_RES_ORDER_HOR) ? k : 1 - k;       /* 0: the width */
        w = lqr_carver_get_width(frames[0]); h = lqr_carver_get_height(frames[0]);
        if ((dir ? h1 - h : w1 - w) == 0) continue;
        LQR_CATCH(lqrx_carvers_load_static(frames, n, abs(dir ? h1 - h : w1 - w), dir, alpha, delta_x, rigidity));
        LQR_CATCH(lqrx_carver_resize_batch(frames, n, dir ? w : w1, dir ? h1 : h));
    }
    return LQR_OK;
}

/* ======================= forward-energy seams for a clip (lqr_clipforward.h) ========== */
/* The up-front checks and the composition: the seams are found by k_clipfwd.hip behind lqrhip_clipfwd_*, in the slices of a forward build
 * (FWD_SLICE_SEAMS), and the map goes from the build's device memory to group_vmap_load_entered like any caller's. */

/* what refuses a call before any device work.  with_map 0: the resize call, which decides depths and line lengths itself */
static LqrRetVal clipfwd_check(LqrCarver *const *rs, int n, int with_map, int depth, int orientation, float temporal, const char *who, int *len)
{
    int i, L, H;
    const char *why = NULL;
    if (!rs) why = "NULL frames";
    else if (n < 1 || n > LQRHIP_FORWARD_MAX_LINES) why = "1 .. 65535 frames";
    else if (orientation != 0 && orientation != 1) why = "orientation is 0 or 1";
    else if (!(temporal >= 0.0f && isfinite(temporal))) why = "temporal is a finite number >= 0";
    for (i = 0; !why && i < n; i++) {
        if (!rs[i]) why = "NULL frame";
        else if (rs[i]->root) why = "an attached carver follows its root";
        else if (i && !same_config(rs[0], rs[i])) why = "the frames are not of one configuration";
    }
    if (why) { fprintf(stderr, "liblqr-hip: %s refused: %s\n", who, why); return LQR_ERROR; }
    if (!with_map) return LQR_OK;
    L = orientation ? lqr_carver_get_height(rs[0]) : lqr_carver_get_width(rs[0]);
    H = orientation ? lqr_carver_get_width(rs[0]) : lqr_carver_get_height(rs[0]);
    if (depth < 1 || depth >= L || L > LQRHIP_MAX_FRAME_WIDTH || H > LQRHIP_FORWARD_MAX_LINES) {
        fprintf(stderr, "liblqr-hip: %s refused: depth %d on %d lines of %d (0 < depth < line length <= %d, at most %d lines)\n", who, depth, H, L,
                LQRHIP_MAX_FRAME_WIDTH, LQRHIP_FORWARD_MAX_LINES);
        return LQR_ERROR;
    }
    *len = L;
    return LQR_OK;
}

/* Inside the call (roots_enter): flatten what is not flat, then the build in slices, a check point in front of each.  device_map NULL:
 * the build keeps the map.  On LQR_OK *out holds the finished build, which the caller releases; otherwise nothing is left */
static LqrRetVal clipfwd_build_entered(LqrCarver **rs, int n, int depth, int orientation, float temporal, int L, gint *device_map, LqrHipClipFwd **out)
{
    LqrHipCarver **ds;
    LqrHipClipFwd *f = NULL;
    LqrRetVal ret;
    int i, first;
    *out = NULL;
    for (i = 0; i < n; i++) LQR_CATCH(mask_queue_flush(rs[i]));
    if (!lqr_geom_is_flat(&rs[0]->geo)) {
        Group g;
        LQR_CATCH(group_open(&g, rs, n));
        ret = group_flatten(&g);
        if (ret != LQR_OK) { int k; for (k = 0; k < g.nb; k++) lqrhip_batch_abort(g.b[k]); }
        group_close(&g);
        LQR_CATCH(ret);
    }
    if (roots_cancelled(rs, n)) return LQR_USRCANCEL;
    ds = (LqrHipCarver **) malloc((size_t) n * sizeof *ds);
    if (!ds) return LQR_NOMEM;
    for (i = 0; i < n; i++) ds[i] = rs[i]->dev;
    ret = hip_ret(lqrhip_clipfwd_begin(ds, n, depth, orientation, rs[0]->geo.transposed,
                                       rs[0]->nrg_func >= LQR_EF_LUMA_GRAD_NORM && rs[0]->nrg_func <= LQR_EF_LUMA_GRAD_XABS, L, temporal, device_map, &f));
    free(ds);
    for (first = 0; ret == LQR_OK && first < depth; first += FWD_SLICE_SEAMS) {
        if (roots_cancelled(rs, n)) ret = LQR_USRCANCEL;
        else ret = hip_ret(lqrhip_clipfwd_seams(f, first, MINI(FWD_SLICE_SEAMS, depth - first)));
    }
    if (ret == LQR_OK && roots_cancelled(rs, n)) ret = LQR_USRCANCEL;
    if (ret == LQR_OK) ret = hip_ret(lqrhip_clipfwd_finish(f));
    if (ret != LQR_OK) { lqrhip_clipfwd_release(f); return ret; }
    *out = f;
    return LQR_OK;
}

LqrRetVal lqrx_clip_forward_map_device(LqrCarver **frames, gint n, gint depth, gint orientation, gfloat temporal, gint *device_map)
{
    LqrHipClipFwd *f;
    LqrRetVal ret;
    int L;
    LQR_CATCH(clipfwd_check(frames, n, 1, depth, orientation, temporal, "lqrx_clip_forward_map_device", &L));
    if (!device_map) { fprintf(stderr, "liblqr-hip: lqrx_clip_forward_map_device refused: NULL map\n"); return LQR_ERROR; }
    LQR_CATCH(roots_enter(frames, n, LQR_STATE_RESIZING));
    ret = clipfwd_build_entered(frames, n, depth, orientation, temporal, L, device_map, &f);
    if (ret == LQR_OK) lqrhip_clipfwd_release(f);
    roots_leave(frames, n);
    return ret;
}

LqrVMap *lqrx_clip_forward_map(LqrCarver **frames, gint n, gint depth, gint orientation, gfloat temporal)
{
    LqrHipClipFwd *f;
    LqrVMap *v = NULL;
    gint *buffer;
    int L, width, height;
    if (clipfwd_check(frames, n, 1, depth, orientation, temporal, "lqrx_clip_forward_map", &L) != LQR_OK) return NULL;
    if (roots_enter(frames, n, LQR_STATE_RESIZING) != LQR_OK) return NULL;
    width = lqr_carver_get_width(frames[0]); height = lqr_carver_get_height(frames[0]);
    buffer = (gint *) malloc((size_t) width * height * sizeof *buffer);
    if (buffer && clipfwd_build_entered(frames, n, depth, orientation, temporal, L, NULL, &f) == LQR_OK) {
        if (hip_ret(lqrhip_clipfwd_read_map(f, buffer)) == LQR_OK) v = lqr_vmap_new(buffer, width, height, depth, orientation);
        lqrhip_clipfwd_release(f);
    }
    if (!v) free(buffer);
    roots_leave(frames, n);
    return v;
}

LqrRetVal lqrx_clip_load_forward(LqrCarver **frames, gint n, gint depth, gint orientation, gfloat temporal)
{
    LqrHipClipFwd *f;
    LqrRetVal ret;
    int L;
    LQR_CATCH(clipfwd_check(frames, n, 1, depth, orientation, temporal, "lqrx_clip_load_forward", &L));
    LQR_CATCH(roots_enter(frames, n, LQR_STATE_RESIZING));
    ret = clipfwd_build_entered(frames, n, depth, orientation, temporal, L, NULL, &f);
    if (ret == LQR_OK) {
        /* (the map lies in the build's device memory until the load has committed: no trip through the host) */
        ret = group_vmap_load_entered(frames, n, lqrhip_clipfwd_map(f), 1, lqr_carver_get_width(frames[0]), lqr_carver_get_height(frames[0]), depth, orientation);
        lqrhip_clipfwd_release(f);
    }
    roots_leave(frames, n);
    return ret;
}

LqrRetVal lqrx_clip_resize_forward(LqrCarver **frames, gint n, gint w1, gint h1, gfloat temporal)
{
    int w, h, dir, k;
    LQR_CATCH(clipfwd_check(frames, n, 0, 0, 0, temporal, "lqrx_clip_resize_forward", &k));
    w = lqr_carver_get_width(frames[0]); h = lqr_carver_get_height(frames[0]);
    /* both directions are decided before either changes anything: no line has |change| seams, no frame is wider than the engine's, and
     * the second direction's lines are as many as the first leaves (max(., .) covers both orders) */
    if (w1 < 1 || h1 < 1 || abs(w1 - w) >= w || abs(h1 - h) >= h || (w1 != w && w > LQRHIP_MAX_FRAME_WIDTH) || (h1 != h && h > LQRHIP_MAX_FRAME_WIDTH) ||
        (w1 != w && MAXI(h, h1) > LQRHIP_FORWARD_MAX_LINES) || (h1 != h && MAXI(w, w1) > LQRHIP_FORWARD_MAX_LINES)) {
        fprintf(stderr, "liblqr-hip: lqrx_clip_resize_forward refused: %d x %d to %d x %d (a change below the line length, lines of at most %d, "
                "at most %d of them)\n", w, h, w1, h1, LQRHIP_MAX_FRAME_WIDTH, LQRHIP_FORWARD_MAX_LINES);
        return LQR_ERROR;
    }
    /* the state word is entered here too (the calls below enter it for themselves): a resize to the size the frames have skips both
     * directions, and must still refuse a frame that is marked cancelled or inside another call */
    LQR_CATCH(roots_enter(frames, n, LQR_STATE_RESIZING));
    roots_leave(frames, n);
    for (k = 0; k < 2; k++) {
        dir = (frames[0]->resize_order == LQR_RES_ORDER_HOR) ? k : 1 - k;       /* 0: the width */
        w = lqr_carver_get_width(frames[0]); h = lqr_carver_get_height(frames[0]);
        if ((dir ? h1 - h : w1 - w) == 0) continue;
        LQR_CATCH(lqrx_clip_load_forward(frames, n, abs(dir ? h1 - h : w1 - w), dir, temporal));
        LQR_CATCH(lqrx_carver_resize_batch(frames, n, dir ? w : w1, dir ? h1 : h));
    }
    return LQR_OK;
}

/* ======================= resize (E10) ==================================== */
/* one direction: the walk says what comes next (lqr_sched.h), here it is done on the device */
static LqrRetVal group_resize_dir(Group *g, int w1, int want_transposed)
{
    LqrCarver *r = g->r[0];
    LqrWalk walk;
    LqrWalkStep s;
    int i;
    const gchar *init_msg = want_transposed ? r->progress->init_height_message : r->progress->init_width_message;
    const gchar *end_msg = want_transposed ? r->progress->end_height_message : r->progress->end_width_message;

    lqr_walk_begin(&walk, &r->geo, r->enl_step, w1, want_transposed);
    if (walk.total) CANCEL_POINT(g);        /* (a direction with nothing to carve is no check point: a cancel that came after the last session's check ends in LQR_OK) */
    for (i = 0; i < g->n; i++) {
        LqrCarver *c = g->r[i];
        c->session_rescale_total = walk.total;
        c->session_rescale_current = 0;
        c->session_update_step = lqr_sched_update_step(walk.total, c->progress->update_step);
    }
    if (walk.total && r->progress->init) r->progress->init(init_msg);

    while (lqr_walk_next(&walk, &s)) {
        CANCEL_POINT(g);
        if (s.transpose) LQR_CATCH(group_transpose(g));
        LQR_CATCH(group_build_maps(g, s.depth));
        for (i = 0; i < g->n; i++) {
            set_width_tree(g->r[i], s.new_w);
            g->r[i]->session_rescale_current = walk.total - (s.gamma > 0 ? s.gamma : -s.gamma);
            if (g->r[i]->dump_vmaps) LQR_CATCH(lqr_vmap_internal_dump(g->r[i]));
        }
        if (s.flatten) LQR_CATCH(group_flatten(g));
    }
    if (walk.total && r->progress->end) {
        HIP_ALL(g, lqrhip_batch_sync(B));
        r->progress->end(end_msg);
    }
    return LQR_OK;
}

/* (type and roles: a group reads alike, so it is all packed or all value-plane -- reads_value in csrc/lqr_shim.hip -- and the
 * launch arguments of the read hold for every member) */
static int same_config(const LqrCarver *a, const LqrCarver *b)
{
    LqrCarverList *la = a->attached, *lb = b->attached;
    if (a->geo.w0 != b->geo.w0 || a->geo.h0 != b->geo.h0 || a->geo.w != b->geo.w || a->geo.h != b->geo.h || a->geo.w_start != b->geo.w_start ||
        a->geo.h_start != b->geo.h_start || a->geo.level != b->geo.level || a->geo.max_level != b->geo.max_level || a->channels != b->channels ||
        a->geo.transposed != b->geo.transposed || a->active != b->active || a->delta_x != b->delta_x || a->rigidity != b->rigidity ||
        a->has_bias != b->has_bias || a->has_rigmask != b->has_rigmask || a->nrg_func != b->nrg_func ||
        a->leftright != b->leftright || a->lr_switch_frequency != b->lr_switch_frequency || a->enl_step != b->enl_step ||
        a->resize_order != b->resize_order || a->wk_valid != b->wk_valid || a->col_depth != b->col_depth ||
        a->image_type != b->image_type || a->alpha_channel != b->alpha_channel || a->black_channel != b->black_channel)
        return 0;
    for (; la && lb; la = la->next, lb = lb->next)
        if (la->current->channels != lb->current->channels || la->current->col_depth != lb->current->col_depth) return 0;
    return !la && !lb;
}

/* Two refusals, both decided from the sizes alone, before the resize touches the device, by the walk group_resize_dir follows.
 * The supported geometry: a session starts from a frame of at most LQRHIP_MAX_FRAME_WIDTH px
 * in the direction it carves.  Which kernels a wider frame would meet depends on the path it happens to take (the persistent tiled
 * kernels have no such bound, k_dp_sweep behind the band kernels and on the recovery path has), so the rule is decided here. */
static int frame_refused(const LqrCarver *r, int w1, int want_transposed)
{
    return lqr_walk_frame_refused(&r->geo, r->enl_step, w1, want_transposed, LQRHIP_MAX_FRAME_WIDTH);
}
/* A carver lqr_carver_init has not seen cannot build maps: it serves the sizes the map it was given covers (lqr_vmap_load), in that
 * map's direction, and nothing else (lqr_vmap.h 3) */
static int inactive_refused(const LqrCarver *r, int w1, int want_transposed)
{
    return !r->active && lqr_walk_needs_maps(&r->geo, r->enl_step, w1, want_transposed);
}

static LqrRetVal group_resize_entered(LqrCarver **rs, int n, int w1, int h1);
static LqrRetVal group_resize(LqrCarver **rs, int n, int w1, int h1)
{
    LqrRetVal ret;
    int i;
    if (w1 < 1 || h1 < 1) return LQR_ERROR;
    for (i = 0; i < n; i++)
        if (rs[i]->root || !rs[i]->progress) return LQR_ERROR;
    LQR_CATCH(roots_enter(rs, n, LQR_STATE_RESIZING));
    ret = group_resize_entered(rs, n, w1, h1);
    roots_leave(rs, n);
    return ret;
}
static LqrRetVal group_resize_entered(LqrCarver **rs, int n, int w1, int h1)
{
    Group g;
    LqrRetVal ret = LQR_OK;
    int i;
    for (i = 0; i < n; i++) LQR_CATCH(mask_queue_flush(rs[i]));
    for (i = 0; i < n; i++)
        if (frame_refused(rs[i], w1, 0) || frame_refused(rs[i], h1, 1)) {
            fprintf(stderr, "liblqr-hip: resize refused: a frame wider than %d px in the direction being carved is not supported\n",
                    LQRHIP_MAX_FRAME_WIDTH);
            return LQR_ERROR;
        }
    for (i = 0; i < n; i++)
        if (inactive_refused(rs[i], w1, 0) || inactive_refused(rs[i], h1, 1)) return LQR_ERROR;
    {
        T_BEGIN(T_OPEN);
        LQR_CATCH(group_open(&g, rs, n));
        T_END(T_OPEN);
    }
    if (rs[0]->resize_order == LQR_RES_ORDER_HOR) {
        if ((ret = group_resize_dir(&g, w1, 0)) == LQR_OK) ret = group_resize_dir(&g, h1, 1);
    } else {
        if ((ret = group_resize_dir(&g, h1, 1)) == LQR_OK) ret = group_resize_dir(&g, w1, 0);
    }
    if (ret == LQR_OK) {        /* every sub-batch is synchronised, whatever the others returned */
        int k;
        for (k = 0; k < g.nb; k++) { LqrRetVal rk = hip_ret(lqrhip_batch_sync(g.b[k])); if (ret == LQR_OK) ret = rk; }
    }
    if (ret != LQR_OK) { int k; for (k = 0; k < g.nb; k++) lqrhip_batch_abort(g.b[k]); }      /* nothing of this resize may surface in the next one */
    FOR_TREE(&g, i, r, ro_invalidate(r));
    {
        T_BEGIN(T_CLOSE);
        group_close(&g);
        T_END(T_CLOSE);
    }
    return ret;
}

LqrRetVal lqr_carver_resize(LqrCarver *r, gint w1, gint h1) { return group_resize(&r, 1, w1, h1); }

LqrRetVal lqrx_carver_resize_batch(LqrCarver **carvers, gint n, gint w1, gint h1)
{
    int i, same = 1;
    if (n < 1) return LQR_ERROR;
    for (i = 1; i < n; i++) same &= same_config(carvers[0], carvers[i]);
    if (same) {
        /* delta_x = 2 .. 4 and rigidity masks (with rigidity) run on the tiled kernels only while the whole group's tiles are
         * co-resident; a larger group would fall to the one-wave-per-image kernels (~30x slower).  The images are
         * independent, so such a group is carved in consecutive sub-groups that fit. */
        const LqrCarver *c = carvers[0];
        if (is_general(c)) {
            int wmax = c->geo.w_start > c->geo.h_start ? c->geo.w_start : c->geo.h_start, lim;   /* either direction may be carved, shrinking or enlarging */
            if (w1 > wmax) wmax = w1;
            if (h1 > wmax) wmax = h1;
            lim = lqrhip_general_batch_limit_delta(wmax, c->delta_x);
            if (lim >= 1 && n > lim) {
                /* every sub-group is carved whatever the others returned (the images are independent); the first error is reported */
                LqrRetVal first = LQR_OK;
                for (i = 0; i < n; i += lim) {
                    const LqrRetVal r = group_resize(carvers + i, n - i < lim ? n - i : lim, w1, h1);
                    if (r == LQR_USRCANCEL) return r;       /* ... but none is started after a cancelled one (lqr_control.h) */
                    if (first == LQR_OK) first = r;
                }
                return first;
            }
        }
        return group_resize(carvers, n, w1, h1);
    }
    for (i = 0; i < n; i++) LQR_CATCH(lqr_carver_resize(carvers[i], w1, h1));     /* heterogeneous: one by one */
    return LQR_OK;
}

/* ======================= readout (E12) =================================== */
static LqrRetVal fetch_visible(LqrCarver *r)
{
    size_t n = (size_t) r->geo.w * r->geo.h * PX_BYTES(r);
    if (r->ro_valid) return LQR_OK;
    if (!r->ro_image && r->in_buffer && !r->preserve_input && r->in_buffer_len >= n) {     /* the block the image arrived in */
        r->ro_image = r->in_buffer; r->ro_image_len = r->in_buffer_len;
        r->in_buffer = NULL;
    }
    if (!r->ro_image || r->ro_image_len < n) {       /* kept across read-outs: a fresh block costs a page fault per 4 KiB */
        free(r->ro_image);
        r->ro_image = (guchar *) malloc(n ? n : 1);
        if (!r->ro_image) { r->ro_image_len = 0; return LQR_NOMEM; }
        r->ro_image_len = n;
    }
    HIP_CATCH(lqrhip_read_visible(r->dev, r->geo.w0, r->geo.h0, r->geo.w, r->geo.level, r->ro_image));
    if ((size_t) r->ro_buffer_len < r->geo.w * PX_BYTES(r)) {
        free(r->ro_buffer);
        r->ro_buffer = (guchar *) malloc(r->geo.w * PX_BYTES(r));
        if (!r->ro_buffer) return LQR_NOMEM;
        r->ro_buffer_len = (int) (r->geo.w * PX_BYTES(r));
    }
    r->ro_valid = 1;
    return LQR_OK;
}

void lqr_carver_scan_reset(LqrCarver *r) { r->ro_line = 0; r->ro_x = 0; }
gboolean lqr_carver_scan_by_row(LqrCarver *r) { return r->geo.transposed ? FALSE : TRUE; }

/* One packed device->host transfer feeds the whole scan (io_functions.c:155-164
 * calls this once per line); a line is a carver-frame row, i.e. an image column
 * when the carver is transposed. */
gboolean lqr_carver_scan_line(LqrCarver *r, gint *n, guchar **rgb)
{
    if (r->col_depth != LQR_COLDEPTH_8I) return FALSE;        /* liblqr: the 8-bit form only */
    return lqr_carver_scan_line_ext(r, n, (void **) rgb);
}

/* liblqr's cursor: a line scan starts over at the beginning of the line a pixel scan is in */
gboolean lqr_carver_scan_line_ext(LqrCarver *r, gint *n, void **rgb)
{
    const size_t line = r->geo.w * PX_BYTES(r);
    if (r->ro_line >= r->geo.h) { r->ro_line = 0; r->ro_x = 0; return FALSE; }
    if (fetch_visible(r) != LQR_OK) return FALSE;
    memcpy(r->ro_buffer, r->ro_image + (size_t) r->ro_line * line, line);
    *n = r->ro_line;
    *rgb = r->ro_buffer;
    r->ro_line++;
    r->ro_x = 0;
    return TRUE;
}

/* one pixel at a time, carver-frame rows in order; (x, y) in image coordinates */
gboolean lqr_carver_scan_ext(LqrCarver *r, gint *x, gint *y, void **rgb)
{
    const size_t px = PX_BYTES(r);
    if (r->ro_x >= r->geo.w) r->ro_x = 0;          /* (never left outside the frame: every reset of ro_line resets it too) */
    if (r->ro_line >= r->geo.h) { r->ro_line = 0; r->ro_x = 0; return FALSE; }
    if (fetch_visible(r) != LQR_OK) return FALSE;
    *x = r->geo.transposed ? r->ro_line : r->ro_x;
    *y = r->geo.transposed ? r->ro_x : r->ro_line;
    memcpy(r->ro_buffer, r->ro_image + ((size_t) r->ro_line * r->geo.w + r->ro_x) * px, px);
    *rgb = r->ro_buffer;
    if (++r->ro_x == r->geo.w) { r->ro_x = 0; r->ro_line++; }
    return TRUE;
}

gboolean lqr_carver_scan(LqrCarver *r, gint *x, gint *y, guchar **rgb)
{
    if (r->col_depth != LQR_COLDEPTH_8I) return FALSE;
    return lqr_carver_scan_ext(r, x, y, (void **) rgb);
}

LqrRetVal lqrx_carver_read_image(LqrCarver *r, guchar *out)
{
    int x, y;
    const size_t ch = PX_BYTES(r);     /* bytes per pixel */
    if (!r->geo.transposed && !r->ro_valid) {      /* straight into the caller's buffer: no second host copy */
        HIP_CATCH(lqrhip_read_visible(r->dev, r->geo.w0, r->geo.h0, r->geo.w, r->geo.level, out));
        return LQR_OK;
    }
    LQR_CATCH(fetch_visible(r));
    if (!r->geo.transposed) {
        memcpy(out, r->ro_image, (size_t) r->geo.w * r->geo.h * ch);
    } else {
        for (y = 0; y < r->geo.h; y++)
            for (x = 0; x < r->geo.w; x++) memcpy(out + ((size_t) x * r->geo.h + y) * ch, r->ro_image + ((size_t) y * r->geo.w + x) * ch, ch);
    }
    return LQR_OK;
}

LqrRetVal lqrx_carver_read_image_device(LqrCarver *r, void *device_ptr)
{
    HIP_CATCH(lqrhip_read_visible_device(r->dev, r->geo.w0, r->geo.h0, r->geo.w, r->geo.level, device_ptr));
    return LQR_OK;
}

/* ======================= many sizes in one pass (lqr_sizes.h) ============= */
/* (an attached carver follows its root's walk: the root's enlargement step) */
static void size_range(const LqrCarver *r, int *lo, int *hi)
{
    lqr_geom_size_range(&r->geo, (r->root ? r->root : r)->enl_step, lo, hi);
}

gint lqrx_carver_size_range(LqrCarver *r, gint *min_size, gint *max_size)
{
    int lo, hi;
    if (!r) return -1;
    size_range(r, &lo, &hi);
    if (min_size) *min_size = lo;
    if (max_size) *max_size = hi;
    return r->geo.transposed ? 1 : 0;
}

/* a pure read: the geometry, the read-out cache and the state word are neither consulted nor changed */
static LqrRetVal read_sizes(LqrCarver *r, const gint *sizes, gint n, void *const *out, int on_device)
{
    int lo, hi, k, rc;
    int *levels;
    if (!r || !sizes || !out || n < 1) return LQR_ERROR;
    size_range(r, &lo, &hi);
    for (k = 0; k < n; k++)
        if (!out[k] || sizes[k] < lo || sizes[k] > hi) return LQR_ERROR;
    levels = (int *) malloc((size_t) n * sizeof *levels);
    if (!levels) return LQR_NOMEM;
    for (k = 0; k < n; k++) levels[k] = r->geo.w0 - sizes[k] + 1;
    rc = lqrhip_read_sizes(r->dev, r->geo.w0, r->geo.h0, r->geo.transposed, levels, n, out, on_device);
    free(levels);
    return hip_ret(rc);
}

LqrRetVal lqrx_carver_read_sizes_device(LqrCarver *r, const gint *sizes, gint n, void *const *device_out) { return read_sizes(r, sizes, n, device_out, 1); }
LqrRetVal lqrx_carver_read_sizes(LqrCarver *r, const gint *sizes, gint n, void *const *host_out) { return read_sizes(r, sizes, n, host_out, 0); }

/* ======================= object removal (lqr_remove.h) =================== */
/* Only the checks and the composition live here: the scan is k_discard.hip's behind lqrhip_discard_scan, the rounds are
 * group_resize_entered's, the flattening group_flatten's.  No seam logic of its own. */
enum { DS_MARKED = 0, DS_NEED = 1, DS_DEEPEST = 2 };

static int strength_refused(float strength) { return !isfinite(strength) || strength < 0; }

/* The scan of r's base layout as it stands, for every orientation o whose bit is set in `which`: res[o] = {visible marked pixels, the
 * most in one line, the deepest level of a marked pixel}.  The lines of orientation o are the base layout's rows where the carver lies
 * that way, and run across them where it does not: the carver is not transposed for it */
static LqrRetVal discard_scan_run(LqrCarver *r, int which, float strength, int res[2][3])
{
    const int t = r->geo.transposed ? 1 : 0;
    int out[8], o;
    memset(out, 0, sizeof out);
    if (r->has_bias)
        HIP_CATCH(lqrhip_discard_scan(r->dev, r->geo.w0, r->geo.h0, r->geo.w, r->geo.level, r->geo.w0 - r->geo.w_start, strength,
                                      ((which >> t) & 1 ? LQRHIP_DISCARD_LINE : 0) | ((which >> (1 - t)) & 1 ? LQRHIP_DISCARD_CROSS : 0), out));
    for (o = 0; o < 2; o++) memcpy(res[o], out + (o == t ? 0 : 4), 3 * sizeof(int));
    return LQR_OK;
}
/* AUTO: the orientation with the smaller need, a tie goes to 0 */
static int discard_pick(int orientation, int res[2][3])
{
    return orientation != LQRX_ORIENTATION_AUTO ? orientation : res[1][DS_NEED] < res[0][DS_NEED] ? 1 : 0;
}

/* a pure read, as read_sizes is: the geometry, the read-out cache and the state word are neither consulted nor changed */
LqrRetVal lqrx_carver_discard_scan(LqrCarver *r, gint orientation, gfloat strength, gint *marked, gint *need)
{
    int res[2][3], o;
    if (!r || r->root || orientation < LQRX_ORIENTATION_AUTO || orientation > 1 || strength_refused(strength)) return LQR_ERROR;
    LQR_CATCH(mask_queue_flush(r));
    LQR_CATCH(discard_scan_run(r, orientation == LQRX_ORIENTATION_AUTO ? 3 : 1 << orientation, strength, res));
    o = discard_pick(orientation, res);
    if (marked) *marked = res[o][DS_MARKED];
    if (need) *need = res[o][DS_NEED];
    return LQR_OK;
}

/* inside the call (roots_enter): the carver flattened, as lqr_carver_flatten does it */
static LqrRetVal flatten_entered(LqrCarver *r)
{
    Group g;
    LqrRetVal ret;
    LQR_CATCH(group_open(&g, &r, 1));
    ret = group_flatten(&g);
    if (ret != LQR_OK) { int k; for (k = 0; k < g.nb; k++) lqrhip_batch_abort(g.b[k]); }
    group_close(&g);
    return ret;
}

static LqrRetVal remove_entered(LqrCarver *r, int orientation, float strength, int max_seams, int restore, gint *orientation_used, gint *seams,
                                gint *left)
{
    int res[2][3], o, W0, H0, L0, cap, cur = 0, fin;
    LQR_CATCH(mask_queue_flush(r));
    if (!lqr_geom_is_flat(&r->geo)) LQR_CATCH(flatten_entered(r));
    W0 = lqr_carver_get_width(r); H0 = lqr_carver_get_height(r);
    LQR_CATCH(discard_scan_run(r, orientation == LQRX_ORIENTATION_AUTO ? 3 : 1 << orientation, strength, res));
    o = discard_pick(orientation, res);
    if (orientation_used) *orientation_used = o;
    if (seams) *seams = 0;
    if (left) *left = 0;
    if (res[o][DS_NEED] == 0) return LQR_OK;
    L0 = o ? H0 : W0;
    cap = MINI(max_seams, L0 - 2);
    while (res[o][DS_NEED] > 0 && cur < cap) {
        if (lqr_state_check(&r->state)) return LQR_USRCANCEL;
        cur += MINI(MAXI(res[o][DS_NEED], LQRX_REMOVE_MIN_STEP), cap - cur);
        LQR_CATCH(group_resize_entered(&r, 1, o ? W0 : L0 - cur, o ? L0 - cur : H0));
        LQR_CATCH(discard_scan_run(r, 1 << o, strength, res));
    }
    if (res[o][DS_NEED] == 0) {
        fin = res[o][DS_DEEPEST];
        if (fin < cur) LQR_CATCH(group_resize_entered(&r, 1, o ? W0 : L0 - fin, o ? L0 - fin : H0));      /* served from the map */
        if (seams) *seams = fin;
    } else {                    /* the cap was reached */
        if (seams) *seams = cur;
        if (left) *left = res[o][DS_MARKED];
    }
    if (restore) {              /* the plug-in's SCALEBACK_MODE_LQRBACK, render.c:320-329 */
        if (lqr_state_check(&r->state)) return LQR_USRCANCEL;
        LQR_CATCH(flatten_entered(r));
        LQR_CATCH(group_resize_entered(&r, 1, W0, H0));
    }
    return LQR_OK;
}

LqrRetVal lqrx_carver_remove_discarded(LqrCarver *r, gint orientation, gfloat strength, gint max_seams, gint restore, gint *orientation_used,
                                       gint *seams, gint *left)
{
    const char *why = NULL;
    LqrRetVal ret;
    if (!r) why = "NULL carver";
    else if (r->root) why = "an attached carver follows its root";
    else if (!r->active || !r->progress) why = "the carver is not initialised";
    else if (orientation < LQRX_ORIENTATION_AUTO || orientation > 1) why = "the orientation is 0, 1 or LQRX_ORIENTATION_AUTO";
    else if (strength_refused(strength)) why = "the strength is finite and >= 0";
    else if (max_seams < 1) why = "max_seams is at least 1";
    else if ((orientation != 1 && lqr_carver_get_width(r) < 3) || (orientation != 0 && lqr_carver_get_height(r) < 3)) why = "a line of fewer than 3 pixels";
    if (why) { fprintf(stderr, "liblqr-hip: lqrx_carver_remove_discarded refused: %s\n", why); return LQR_ERROR; }
    LQR_CATCH(roots_enter(&r, 1, LQR_STATE_RESIZING));
    ret = remove_entered(r, orientation, strength, max_seams, restore, orientation_used, seams, left);
    roots_leave(&r, 1);
    return ret;
}

/* ======================= seam-map colour ramp (I5) ======================== */
LqrRetVal lqrx_vmap_to_rgba(LqrVMap *v, const gdouble col_start[3], const gdouble col_end[3], guchar *out_rgba)
{
    if (!v || !v->buffer || !out_rgba) return LQR_ERROR;
    HIP_CATCH(lqrhip_vmap_to_rgba(v->buffer, v->width, v->height, v->depth, col_start, col_end, out_rgba));
    return LQR_OK;
}

/* ======================= reload from device memory ======================= */
LqrRetVal lqrx_carver_reload_device_batch(LqrCarver **rs, gint n, void *const *device_rgb)
{
    int i, lo, rc = 0, done = 0;
    LqrHipCarver **ds;
    T_BEGIN(T_RELOAD);
    if (n < 1) return LQR_ERROR;
    for (i = 0; i < n; i++)
        if (!rs[i] || rs[i]->root || rs[i]->attached || !device_rgb[i]) return LQR_ERROR;
    ds = (LqrHipCarver **) malloc((size_t) n * sizeof *ds);
    if (!ds) return LQR_NOMEM;
    for (i = 0; i < n; i++) ds[i] = rs[i]->dev;
    /* the device side of the whole list: one call, and one copy launch per 16 images, for every run of carvers of one size */
    for (lo = 0; lo < n && !rc; lo = i) {
        for (i = lo + 1; i < n && rs[i]->img_w == rs[lo]->img_w && rs[i]->img_h == rs[lo]->img_h; i++);
        rc = lqrhip_carver_reset_batch(ds + lo, (const void *const *) device_rgb + lo, i - lo, rs[lo]->img_w, rs[lo]->img_h);
        done = rc ? lo + lqrhip_carver_reset_batch_count() : i;
    }
    free(ds);
    /* ... and the host side of every carver the device side has reset (all of them, unless it failed) */
    for (i = 0; i < done; i++) {
        LqrCarver *r = rs[i];
        LqrVMapList *v, *vn;
        lqr_maskq_reset(&r->mq[0]); lqr_maskq_reset(&r->mq[1]);        /* masks are dropped, queued ones too */
        for (v = r->flushed_vs; v; v = vn) { vn = v->next; lqr_vmap_destroy(v->current); free(v); }
        r->flushed_vs = NULL;
        lqr_geom_reset(&r->geo, r->img_w, r->img_h);
        r->leftright = 0;
        r->has_bias = r->has_rigmask = 0;
        r->wk_valid = 0;
        ro_invalidate(r);
        if (r->active) rigidity_table(r);       /* as lqr_carver_init */
    }
    HIP_CATCH(rc);
    HIP_CATCH(lqrhip_reset_sync());
    T_END(T_RELOAD);
    return LQR_OK;
}

/* ======================= auto-size (plug-in side) ======================== */
/* guess_new_size, reference src/layers_combo.c:275-392: the geometry is resolved here, the
 * per-line counting and the max over lines run on the device */
gint lqrx_guess_new_size(const guchar *mask, gint channels, gint width, gint height, gint x_off, gint y_off,
                         gint old_width, gint old_height, gint direction)
{
    int lw = MINI(old_width, width + x_off) - MAXI(0, x_off);
    int lh = MINI(old_height, height + y_off) - MAXI(0, y_off);
    int old_size = direction ? old_height : old_width, m;
    if (direction == 0)     /* lines are mask rows z1 - y_off, z1 in [max(0,y_off), min(old_h, h+y_off)) */
        m = lqrhip_mask_line_max(mask, channels, width, height, MAXI(0, y_off) - y_off, MAXI(0, -x_off),
                                 MINI(old_height, height + y_off) - MAXI(0, y_off), lw, 0);
    else
        m = lqrhip_mask_line_max(mask, channels, width, height, MAXI(0, x_off) - x_off, MAXI(0, -y_off),
                                 MINI(old_width, width + x_off) - MAXI(0, x_off), lh, 1);
    if (m < 0) { fprintf(stderr, "liblqr-hip: guess_new_size failed: %s\n", lqrhip_last_error()); return old_size; }
    return old_size - m;
}

/* ======================= test hooks ====================================== */
/* What every energy read-out does: the carver is brought to the frame seams of `orientation` are carved in, as lqr_carver_resize
 * brings it there (flattened if it is not at the width of its visibility map, transposed -- and left so -- if it lies the other way),
 * its energy is built, and the output stage writes it in image orientation.  form 0: the values as they are, 1: normalised, 2: pixels
 * of depth / image_type; -1: the working plane as it lies, in the carver's frame and without a transposition (the test hook).  A
 * failure leaves the carver in one of the states this sequence passes through. */
static LqrRetVal energy_run_entered(LqrCarver *r, void *buffer, int on_device, int orientation, int form, int depth, int image_type);
static LqrRetVal energy_run(LqrCarver *r, void *buffer, int on_device, int orientation, int form, int depth, int image_type)
{
    LqrRetVal ret;
    if (r->root) return LQR_ERROR;          /* (lqr_energy.h: an attached carver cannot be re-laid alone) */
    LQR_CATCH(roots_enter(&r, 1, LQR_STATE_RESIZING));
    ret = energy_run_entered(r, buffer, on_device, orientation, form, depth, image_type);
    roots_leave(&r, 1);
    return ret;
}
static LqrRetVal energy_run_entered(LqrCarver *r, void *buffer, int on_device, int orientation, int form, int depth, int image_type)
{
    Group g;
    LqrHipDpParams p;
    LqrRetVal ret = LQR_OK;
    LQR_CATCH(mask_queue_flush(r));
    LQR_CATCH(group_open(&g, &r, 1));
    if (r->geo.w != r->geo.w_start - r->geo.max_level + 1) ret = group_flatten(&g);
    if (ret == LQR_OK && form >= 0 && r->geo.transposed != orientation) ret = group_transpose(&g);
    /* (a carver lqr_carver_init has not seen gets its working planes here too, and stays inactive) */
    if (ret == LQR_OK && !r->wk_valid) {
        if ((ret = hip_ret(lqrhip_wk_init(g.b[0], r->geo.max_level != 1 || r->geo.w0 != r->geo.w_start))) == LQR_OK) r->wk_valid = 1;
    }
    if (ret == LQR_OK) {
        dp_params(r, &p);
        ret = hip_ret(lqrhip_emap_build(g.b[0], &p, r->geo.w, r->geo.h));
    }
    if (ret == LQR_OK)
        ret = hip_ret(form < 0 ? lqrhip_read_working(r->dev, r->geo.w, r->geo.h, (float *) buffer, NULL, NULL)
                               : lqrhip_energy_out(g.b[0], r->geo.w, r->geo.h, r->geo.transposed, form, depth, image_type, buffer, on_device));
    group_close(&g);
    return ret;
}
LqrRetVal lqrx_carver_get_energy(LqrCarver *r, gfloat *buffer) { return energy_run(r, buffer, 0, 0, -1, 0, 0); }

/* ======================= energy read-outs (lqr_energy.h) ================= */
/* all five entry points, arguments checked */
static LqrRetVal energy_read(LqrCarver *r, void *buffer, int on_device, int orientation, int form, int depth, int image_type)
{
    if (!r || !buffer || (orientation != 0 && orientation != 1)) return LQR_ERROR;
    if (form == 2 && (depth < LQR_COLDEPTH_8I || depth > LQR_COLDEPTH_64F || image_type < LQR_RGB_IMAGE || image_type >= LQR_CUSTOM_IMAGE))
        return LQR_ERROR;
    return energy_run(r, buffer, on_device, orientation, form, depth, image_type);
}
LqrRetVal lqr_carver_get_energy(LqrCarver *r, gfloat *buffer, gint orientation) { return energy_read(r, buffer, 0, orientation, 1, 0, 0); }
LqrRetVal lqr_carver_get_true_energy(LqrCarver *r, gfloat *buffer, gint orientation) { return energy_read(r, buffer, 0, orientation, 0, 0, 0); }
LqrRetVal lqr_carver_get_energy_image(LqrCarver *r, void *buffer, gint orientation, LqrColDepth col_depth, LqrImageType image_type)
{
    return energy_read(r, buffer, 0, orientation, 2, (int) col_depth, (int) image_type);
}
LqrRetVal lqrx_carver_get_energy_device(LqrCarver *r, void *device_buffer, gint orientation, gint normalised)
{
    return energy_read(r, device_buffer, 1, orientation, normalised ? 1 : 0, 0, 0);
}
LqrRetVal lqrx_carver_get_energy_image_device(LqrCarver *r, void *device_buffer, gint orientation, LqrColDepth col_depth, LqrImageType image_type)
{
    return energy_read(r, device_buffer, 1, orientation, 2, (int) col_depth, (int) image_type);
}

LqrRetVal lqrx_carver_debug_maps(LqrCarver *r, gfloat *en, gfloat *m, gint *least_dx)
{
    if (!r->active || !r->wk_valid) return LQR_ERROR;
    HIP_CATCH(lqrhip_read_working(r->dev, r->geo.w, r->geo.h, en, m, least_dx));
    return LQR_OK;
}
int lqrhip_debug_seam_flags(const void *carver, int *org, int *org_prev, int *side)
{
    const LqrCarver *r = (const LqrCarver *) carver;
    if (!r || !r->dbg_m) return LQRHIP_EARG;
    *org = r->dbg_org; *org_prev = r->dbg_org_prev; *side = r->dbg_side;
    return 0;
}
gint lqrx_carver_debug_width(LqrCarver *r) { return r->dbg_w; }
gint lqrx_carver_debug_height(LqrCarver *r) { return r->dbg_h; }
LqrRetVal lqrx_carver_debug_snapshot(LqrCarver *r, gfloat *en, gfloat *m, gint *least_dx)
{
    size_t n = (size_t) r->dbg_w * r->dbg_h;
    if (!r->dbg_m) return LQR_ERROR;
    if (en) memcpy(en, r->dbg_en, n * sizeof(float));
    if (m) memcpy(m, r->dbg_m, n * sizeof(float));
    if (least_dx) memcpy(least_dx, r->dbg_least, n * sizeof(int));
    return LQR_OK;
}
