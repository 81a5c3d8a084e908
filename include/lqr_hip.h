/*
 * lqr_hip.h -- thin C-ABI shim between the C host side of the engine
 * (gimp-lqr-plugin_amd/host/lqr_carver.c, which implements include/lqr.h) and
 * the hand-written gfx950 kernels (gimp-lqr-plugin_amd/csrc/k_*.hip, launched by csrc/lqr_shim.hip).
 *
 * Plain pointers and sizes only; no C++ or torch types.  Each entry point names
 * the liblqr engine stage it replaces and the
 * reference call site that reaches that stage.
 *
 * Everything is batch-native: a LqrHipBatch is n carvers of identical geometry
 * and configuration that advance in lock-step, one grid.y (or grid.z) slice per
 * image.  A single carver is a batch of one.  All work of a batch is enqueued
 * on the batch's HIP stream; only lqrhip_batch_sync and the read-back calls
 * block.  Every function returns 0 on success, LQRHIP_ENOMEM on device OOM and
 * another negative value on any other HIP error; none of them aborts, and no kernel
 * traps: a device-side failure (a persistent grid that was not co-resident, a failed
 * self-check of the session) is recorded in a host-visible word and returned by the next
 * lqrhip_batch_sync / lqrhip_device_sync / lqrhip_inflate as LQRHIP_EFAULT; the host side then rolls
 * the session back (lqrhip_session_rollback) and redoes it on the kernels without spin waits.
 *
 * Threading: like the plug-in's use of liblqr (GTK main loop / PDB run), the library
 * is single-threaded by contract -- the allocation cache, the error word and the
 * profiling records are process globals without locks, and the device is selected
 * (hipSetDevice) for the thread that first calls in.  The environment holds no tuning knob: LOCAL_RANK selects
 * the device, GPU_MAX_HW_QUEUES is looked at (lqrhip_sub_batches), LQRHIP_POISON* and LQRHIP_DUMP are debugging
 * aids.
 */
#ifndef LQR_HIP_H
#define LQR_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LQRHIP_OK 0
#define LQRHIP_ENOMEM (-2)
#define LQRHIP_EHIP (-1)
#define LQRHIP_EARG (-3)
#define LQRHIP_EFAULT (-4)   /* a kernel of the session gave up or a self-check failed: roll back, redo (lqrhip_session_rollback) */
#define LQRHIP_EMAP (-5)     /* lqrhip_vmap_stage: the caller's seam map is not one.  A bad argument, not a device fault: nothing to roll back */
#define LQRHIP_MAX_DELTA 16
#define LQRHIP_MAX_CHANNELS 64      /* channels per pixel at most (lqrx_set_max_channels) */
/* The widest frame, in the direction being carved, that a session may start from: k_dp_sweep holds two rows of it in LDS (128 KB)
 * at 16 px per thread.  The host side refuses wider ones before any device call (host/lqr_carver.c, frame_refused). */
#define LQRHIP_MAX_FRAME_WIDTH 16384

typedef struct LqrHipCarver LqrHipCarver;   /* device-resident planes of one carver */
typedef struct LqrHipBatch LqrHipBatch;     /* n carvers advancing in lock-step     */

/* DP parameters that stay fixed while a visibility map is being built */
typedef struct LqrHipDpParams {
    int delta_x;                                  /* lqr_carver_init, render.c:224 */
    int use_rigidity;                             /* rigidity != 0 */
    float rigidity_map[2 * LQRHIP_MAX_DELTA + 1]; /* [dx + delta_x], host-computed (powf) */
    int nrg_func;                                 /* LqrEnergyFuncBuiltinType, render.c:234 */
    int nrg_radius;                               /* 1 for gradients, 0 for LQR_EF_NULL */
    int w_start;                                  /* bias is divided by this (E4) */
} LqrHipDpParams;

/* -- device / lifetime ----------------------------------------------------- */
/* Selects the HIP device (LOCAL_RANK, else 0) on first use.  Returns the
 * device ordinal or a negative error when no gfx950 device is usable. */
int lqrhip_init(void);
const char *lqrhip_last_error(void);

/* E1 lqr_carver_new (render.c:222,894): upload the interleaved u8 image as the
 * base layout.  The host buffer is not retained. */
LqrHipCarver *lqrhip_carver_create(const unsigned char *rgb, int w, int h, int channels);
/* lqr_carver_new_ext (lqr_coldepth.h): the same for pixels of `depth` (LqrColDepth 0 .. 3: channels x 1 / 2 / 4 / 8 bytes).
 * Every call below that moves base-layout pixels (read-out, reset) moves w x h x channels x that many bytes. */
LqrHipCarver *lqrhip_carver_create_ext(const void *rgb, int w, int h, int channels, int depth);
/* a carver that reads through the value plane (depth 16I / 32F / 64F, or see lqrhip_carver_set_read) keeps the value its energy reads (brightness, or luma with `luma`) in its working
 * planes: returns 1 if that kind changed, i.e. the working planes must be laid out again (lqrhip_wk_init) */
int lqrhip_carver_set_read_luma(LqrHipCarver *c, int luma);
/* liblqr's image type (lqr_imagetype.h: LqrImageType 0 .. 7) with its alpha and black channel indices (negative: none).  8-bit grey /
 * RGB carvers with or without alpha in the default layout keep their packed pixels; every other carver reads through the value
 * plane as the deep ones do.  Returns 1 if what the energy reads changed (the working planes must be laid out again), 0 if not,
 * LQRHIP_EARG for a type or an index out of range. */
int lqrhip_carver_set_read(LqrHipCarver *c, int image_type, int alpha, int black);
void lqrhip_carver_destroy(LqrHipCarver *c);
/* Start over on an existing carver, as lqr_carver_destroy + lqr_carver_new + lqr_carver_init would
 * (render.c:376,222,224), but from an image that is already in HBM: the base layout becomes the
 * w x h x channels interleaved u8 image at `device_rgb` (device-to-device copy on the shim's stream),
 * the visibility map is cleared, masks are dropped; working planes are kept when the geometry is the
 * same.  For batch drivers that keep their inputs device-resident (bench.py). */
int lqrhip_carver_reset(LqrHipCarver *c, const void *device_rgb, int w, int h);
/* The same for n carvers of w x h at once: per carver what lqrhip_carver_reset does on the host, then one kernel launch per 16 carvers
 * that copies their images and clears their visibility maps (an image that is not 16-byte aligned is copied as lqrhip_carver_reset
 * copies it).  Every argument is checked before any carver is touched.  On a failure the carvers before the failing one are reset
 * completely, the failing one is as lqrhip_carver_reset leaves it and those after it are untouched;
 * lqrhip_carver_reset_batch_count() says how many the last call reset completely. */
int lqrhip_carver_reset_batch(LqrHipCarver **cs, const void *const *device_rgb, int n, int w, int h);
int lqrhip_carver_reset_batch_count(void);
/* wait for the copies lqrhip_carver_reset / lqrhip_carver_reset_batch enqueued */
int lqrhip_reset_sync(void);
/* attached carver (render.c:897): shares the root's visibility map */
int lqrhip_carver_attach(LqrHipCarver *root, LqrHipCarver *aux);
/* E1 lqr_carver_init (render.c:224): allocate the working planes
 * (packed pixels, en, m, back-pointers, seam buffers) for a w x h frame. */
int lqrhip_carver_activate(LqrHipCarver *c);

/* E2 lqr_carver_bias_add_rgb_area / lqr_carver_rigmask_add_rgb_area
 * (io_functions.c:94-95,125-126).  The carver must be flat.  `transposed`
 * says whether the carver frame is the transpose of image orientation. */
int lqrhip_mask_add(LqrHipCarver *c, const unsigned char *mask, int channels, int width, int height,
                    int x_off, int y_off, int transposed, int is_rigmask, int bias_factor);

/* E2 for computed masks (lqr_masks.h): the _area forms on width x height values of `depth` (LqrColDepth 2: float, 3: double), clipped
 * as lqrhip_mask_add clips.  on_device = 0: a host buffer, staged as the rgb form's; 1: `mask` is device memory and is read where it
 * lies.  Either way the call returns after the kernel has run. */
int lqrhip_mask_add_f(LqrHipCarver *c, const void *mask, int depth, int on_device, int width, int height, int x_off, int y_off,
                      int transposed, int is_rigmask, int bias_factor);
/* make sure the bias (is_rigmask 0) or rigidity-mask plane exists (zero-filled when new) */
int lqrhip_mask_plane_ensure(LqrHipCarver *c, int is_rigmask);
/* a packed run of queued _xy calls (host/lqr_mask_queue.h): n entries in `buckets` buckets, bucket b being entries start[b] ..
 * start[b + 1]; one k_mask_scatter launch per bucket, in order */
int lqrhip_mask_scatter(LqrHipCarver *c, int is_rigmask, const int *index, const double *value, const size_t *start, int buckets);
/* lqr_carver_bias_clear / lqr_carver_rigmask_clear: free the plane (base layout and working copy) */
int lqrhip_mask_clear(LqrHipCarver *c, int is_rigmask);
/* test hook behind lqrx_carver_get_bias / _get_rigmask: the plane of a flat carver in image orientation (zeros if there is none) */
int lqrhip_read_mask_plane(LqrHipCarver *c, int is_rigmask, int transposed, float *out);
/* Test hook: k_mask_scatter launches since the library was loaded (how the _xy calls were batched) */
unsigned long long lqrhip_debug_mask_flushes(void);

/* -- batch ------------------------------------------------------------------ */
/* into how many device batches (HIP streams) the host splits a lock-step group of n carvers.  Automatic (set 0): 2 for
 * groups of 32 to 48 carvers, 4 for 49 and more, when the process has the hardware queues for them (the HIP runtime's GPU_MAX_HW_QUEUES
 * >= 8 in the environment before HIP initialises; its default of 4 makes the split 30 % slower than one stream, so it is
 * then not made), else 1.  The library sets the variable to 8 itself when it is loaded with the variable unset into a
 * process whose GPU runtime is not up yet.  lqrhip_set_sub_batches(n > 0) pins the number of streams. */
int lqrhip_sub_batches(int n);
/* Images of carved-frame width w that one lock-step batch may hold and still run delta_x = 2 / rigidity-mask carvers on the
 * tiled kernels (0: unknown); larger batches of such carvers are carved group after group (lqrx_carver_resize_batch). */
int lqrhip_general_batch_limit(int w);
/* the same for a given delta_x: 2 .. 4 may also run on k_band_levels (groups of 8 and more), 5 .. 10 on the full-width tiled kernels only */
int lqrhip_general_batch_limit_delta(int w, int delta_x);
void lqrhip_set_sub_batches(int n);
LqrHipBatch *lqrhip_batch_create(LqrHipCarver **carvers, int n);
/* tell a batch how many batches of its group run concurrently on their own streams (0 or 1: alone): kernels whose grid
 * must be co-resident are then never chosen (k_dp_tile_p spins on neighbour tiles) or sized so that ALL the siblings' grids
 * fit together (k_band_levels) */
void lqrhip_batch_set_shared(LqrHipBatch *b, int shared);
/* waits for the batch's stream; the stream (idle now) and the descriptor block are parked for the next lqrhip_batch_create, up to
 * four of each; lqrhip_pool_trim gives the parked ones back */
void lqrhip_batch_destroy(LqrHipBatch *b);
int lqrhip_batch_sync(LqrHipBatch *b);
/* after a failed call on the batch: drain its stream, discard the device-side error record of the failed call, and have
 * every live batch lay its descriptors and exchange areas out afresh */
void lqrhip_batch_abort(LqrHipBatch *b);
void *lqrhip_batch_stream(LqrHipBatch *b);      /* hipStream_t, for event timing in bench.py */

/* base layout -> working planes: what liblqr's raw[y][x] = y*w+x initialisation means for compacted planes.
 * from_visible = 0: identity map (the carver is flat).  from_visible = 1: the carved frame of a multi-size image, i.e. the
 * pixels of the base layout that carry no level yet, in order (a session redone after a fault; working planes that were lost) */
int lqrhip_wk_init(LqrHipBatch *b, int from_visible);
/* E3+E4 lqr_carver_build_emap: full energy map of the w x h carved frame */
int lqrhip_emap_build(LqrHipBatch *b, const LqrHipDpParams *p, int w, int h);
/* lqrhip_wk_init(b, 0) followed by lqrhip_emap_build(b, p, w, h), as a session starts on flat carvers: one pass over the planes
 * where the pixels are packed 8-bit ones and w x h is the frame they are laid out in, the two passes otherwise.  Same planes,
 * same energies, the same allocations in the same order */
int lqrhip_wk_init_emap(LqrHipBatch *b, const LqrHipDpParams *p, int w, int h);
/* The output stage of the energy read-outs (lqr_energy.h), enqueued behind lqrhip_emap_build on the stream of a batch of ONE carver: the
 * w x h energy plane of the carver's frame goes out in IMAGE orientation (`transposed`: the frame is the transpose of it), as
 * form 0 the values as they are (floats), form 1 squashed and normalised to [0, 1] (floats), form 2 the normalised values as pixels of
 * `depth` (LqrColDepth) and `image_type` (LqrImageType 0 .. 6; the float forms ignore both).  on_device = 1: `out` is device memory
 * and nothing is copied to the host; 0: a host buffer, filled from a staging block through the pinned ring.  Returns with `out` written. */
int lqrhip_energy_out(LqrHipBatch *b, int w, int h, int transposed, int form, int depth, int image_type, void *out, int on_device);
/* E5 lqr_carver_build_mmap: full cumulative-min DP, tie rule by `leftright` */
int lqrhip_mmap_build(LqrHipBatch *b, const LqrHipDpParams *p, int w, int h, int leftright);
/* One seam of lqr_carver_build_vsmap (reached from lqr_carver_resize,
 * render.c:318,328,529), on a frame that is w wide on entry:
 *   E7 build_vpath (argmin + backtrack) -> seam `log_index` of the session log,
 *   E8 carve (all working planes shift left of the seam, w -> w-1),
 *   E6 update_emap, then either E9 update_mmap (full_rebuild = 0) or E5
 *   build_mmap with the given (already toggled) leftright (full_rebuild = 1).
 * If w-1 == 1 only E7/E8 run (liblqr's finish_vsmap case). */
int lqrhip_seam_step(LqrHipBatch *b, const LqrHipDpParams *p, int w, int h, int log_index,
                     int leftright_pick, int full_rebuild, int leftright_next);
/* reserve the session seam log (n_seams x h ints per carver) before the first seam_step */
int lqrhip_seam_log_reserve(LqrHipBatch *b, int n_seams, int h);
/* E8 update_vsmap for a whole session at once: turn the session's seam log
 * (n_seams seams, carved frame wc0 wide at session start) into visibility
 * levels first_level, first_level+1, ... in the base layout; `finish` applies
 * liblqr's finish_vsmap (last column gets level w0).  The working planes pix / bias stay behind the carved frame by the seams the
 * session has not compacted yet: that catch-up is owed per carver (the session's log is kept for it) and is paid on the batch's
 * stream at the top of the next lqrhip_emap_build or lqrhip_seam_log_reserve, or dropped where the planes are laid out afresh
 * (lqrhip_wk_init, lqrhip_carver_reset, lqrhip_session_rollback, lqrhip_planes_commit of a flatten or a transpose). */
int lqrhip_vs_commit(LqrHipBatch *b, int w0, int h0, int wc0, int n_seams, int first_level, int finish);
/* Session self-check, enqueued behind the last seam step and in front of lqrhip_vs_commit: the seam log of the session (n_seams
 * seams of h rows, carved frame wc0 wide at its start) must hold delta_x-connected seams inside their frames; a violation is
 * reported as LQRHIP_EFAULT by the next lqrhip_batch_sync.  lqrhip_inflate carries the second check (every level of the session
 * exactly once per row) and returns LQRHIP_EFAULT itself, without adopting anything.  lqrhip_set_selfcheck(0) turns both off. */
int lqrhip_session_check(LqrHipBatch *b, int h, int wc0, int n_seams, int delta_x);
void lqrhip_set_selfcheck(int on);
/* whether the host side redoes a session that ended in LQRHIP_EFAULT (default 1); 0: roll back and return LQR_ERROR (tests) */
void lqrhip_set_recovery(int on);
int lqrhip_get_recovery(void);
/* After LQRHIP_EFAULT: drain the batch's stream, drop the error record, remove the session's levels (>= first_level, and
 * finish_vsmap's w0) from the visibility map if they were committed.  The working planes are invalid afterwards. */
int lqrhip_session_rollback(LqrHipBatch *b, int w0, int h0, int first_level, int finish);
/* kernels without spin waits only (k_dp_tile, k_band_update_tw / _mw / k_band_update, k_dp_sweep): set for the redo of a session */
void lqrhip_batch_set_safe(LqrHipBatch *b, int safe);
/* after a spin time-out the whole process stays on those kernels (a shared or partitioned device); 0 re-arms the persistent ones */
void lqrhip_set_no_spin(int on);
int lqrhip_get_no_spin(void);
/* [0] spin time-outs, [1] failed activity predictions, [2] seam-log check failures, [3] level check failures, [4] sessions
 * rolled back, [5] faults injected, [6] sessions carved on the non-spinning kernels after a fault */
int lqrhip_fault_stats(unsigned long long *out8, int reset);
/* Test hook: provoke a fault in the next session(s).  kind 1 spin time-out / 2 failed prediction (the error word is written while
 * the kernels of seam step at_step run), 3 / 4 a seam-log entry out of the frame / disconnected, 5 / 6 a committed level cleared /
 * duplicated (at_step = commits to let pass first: a later sub-batch of a group); times = sessions hit in a row; kind 0 disarms. */
void lqrhip_debug_inject(int kind, int at_step, int times);
/* Test hook: the nth device allocation from now on (0 = the next one) fails once with LQRHIP_ENOMEM; -1 disarms.  What the host side
 * owes its caller then: LQR_NOMEM (the one value src/render.c:42-46 tests for) and a carver that is still consistent. */
void lqrhip_debug_fail_alloc(int nth);
/* Test hook: device blocks of the allocation cache handed out and not yet given back.  A call that fails, and a carver or batch that
 * is destroyed, leave the count where it was before. */
unsigned long long lqrhip_debug_pool_live(void);
/* Test hook: [0] batch streams parked now, and since the last reset [1] batch streams taken from the parked ones instead of created,
 * [2] carvers lqrhip_carver_reset_batch reset through k_reset_jobs, [3] through the runtime's copy and fill (unaligned images). */
void lqrhip_debug_fixedcost(unsigned long long out4[4], int reset);
/* The three passes that replace a batch's base planes run in TWO PHASES: the call stages the new planes and runs the pass -- nothing of
 * the carvers changes -- and lqrhip_planes_commit adopts what was staged.  A group commits only after every one of its sub-batches has
 * passed phase one, so that a failed self-check (LQRHIP_EFAULT) or a failed allocation (LQRHIP_ENOMEM) in one sub-batch leaves the
 * whole group where it was.  A staged pass is discarded by the next staging call, lqrhip_session_rollback, _batch_abort, _batch_destroy.
 * E14 lqr_carver_inflate(l) on roots and their attached carvers; carries the session's second self-check */
int lqrhip_inflate(LqrHipBatch *b, int w0, int h0, int l, int max_level);
/* lqr_vmap_load (lqr_vmap.h), in two steps.  lqrhip_vmap_stage brings a width x height seam map of `depth` seams (row-major in IMAGE
 * orientation; on_device = 0: host memory, uploaded once through the pinned ring; 1: device memory, read where it lies, which must stay
 * as it is until the loads that use it have been committed) to the device and checks it in one pass: 0 < depth < line length, every
 * value in [0, depth], every level 1 .. depth exactly once in every line of the carving direction (a row for orientation 0, a column
 * for 1); an orientation-1 map is laid out in the carver's frame by the same pass.  A map that fails returns LQRHIP_EMAP and changes
 * nothing: no batch is invalidated, lqrhip_fault_stats and the non-spinning mode stay as they are.  lqrhip_vmap_load is then phase one
 * of a pass like lqrhip_inflate: the batch's carvers -- flat, and in the map's frame -- stage the layout in which every seam of the map
 * is doubled, all reading their levels from the ONE checked plane; lqrhip_planes_commit adopts it.  lqrhip_vmap_release gives the
 * staged map back (after the commits, or instead of them). */
typedef struct LqrHipVMap LqrHipVMap;
int lqrhip_vmap_stage(const int *map, int on_device, int width, int height, int depth, int orientation, LqrHipVMap **out);
int lqrhip_vmap_load(LqrHipBatch *b, const LqrHipVMap *m);
void lqrhip_vmap_release(LqrHipVMap *m);
/* E11 lqr_carver_flatten (render.c:325,636): keep pixels visible at `level` */
int lqrhip_flatten(LqrHipBatch *b, int w0, int h0, int w, int level);
/* E11 lqr_carver_transpose: base planes of a flat carver, w x h -> h x w */
int lqrhip_transpose(LqrHipBatch *b, int w, int h);
int lqrhip_planes_commit(LqrHipBatch *b);
int lqrhip_inflate_commit(LqrHipBatch *b);      /* = lqrhip_planes_commit */

/* -- read-back (blocking) --------------------------------------------------- */
/* E12 scan_line source: the pixels visible at `level`, packed w x h x channels
 * in CARVER orientation (io_functions.c:155-164 then serves rows of it). */
int lqrhip_read_visible(LqrHipCarver *c, int w0, int h0, int w, int level, unsigned char *out);
/* guess_new_size (src/layers_combo.c:275-392): max over lines of the count of mask pixels at or
 * above the threshold; returns the count (>= 0) or a negative error */
int lqrhip_mask_line_max(const unsigned char *mask, int channels, int width, int height, int a0, int b0, int n_lines, int line_len,
                         int direction);
/* same, but into a caller-provided device buffer (no host round trip) */
int lqrhip_read_visible_device(LqrHipCarver *c, int w0, int h0, int w, int level, void *device_out);
/* lqr_sizes.h: the pixels visible at each of n levels (image k is w0 - levels[k] + 1 wide in the carver's frame), every image in
 * IMAGE orientation (transposed: the carver lies transposed, its frame rows are image columns), to outs[k] in device memory
 * (on_device; any multiple of the sample size) or in host memory.  One pass over the base layout per 64 sizes (and per 512 MiB of
 * scratch planes where the images do not go straight to the caller's device memory): LQRHIP_CENSUS_COMPACT_SIZES counts them.
 * Everything is allocated before anything is launched: LQRHIP_ENOMEM has written nothing.  Returns with the outputs written. */
int lqrhip_read_sizes(LqrHipCarver *c, int w0, int h0, int transposed, const int *levels, int n, void *const *outs, int on_device);
/* lqr_remove.h: the discard scan of a root carver's base layout (w0 x h0, w columns of a row visible) as it stands: nothing is flattened
 * or transposed.  A pixel is marked when its bias is below -strength and visible when its level is 0 or at least `level`.  which:
 * LQRHIP_DISCARD_LINE scans the lines that are the base layout's rows (k_discard_line), LQRHIP_DISCARD_CROSS those that run across
 * them (k_discard_cross and k_discard_fold; on a carver that hides pixels, level > 1, k_discard_rank: a column of the image is a rank
 * among a row's visible pixels), or both.  out: 8 ints -- the line scan's {visible marked pixels, the most of them in one line, the
 * deepest level of a marked pixel less `depth` (lqr_vmap_dump's numbering; 0: none has one), 0}, then the cross scan's; the words of
 * a scan not asked for are 0, and all of them for a carver without a bias plane.  One pass over bias0 and vs per scan; 16 bytes per
 * scan come back.  Everything is allocated before anything is launched.  lqrhip_discard_launches: launches of the four kernels
 * (line, cross, rank, fold) since the last reset -- a test hook; lqrhip_launch_census has no slot left for them */
#define LQRHIP_DISCARD_LINE 1
#define LQRHIP_DISCARD_CROSS 2
int lqrhip_discard_scan(LqrHipCarver *c, int w0, int h0, int w, int level, int depth, float strength, int which, int *out);
void lqrhip_discard_launches(unsigned long long out4[4], int reset);
/* lqr_forward.h: forward-energy seam maps of n FLAT root carvers of one shape and pixel kind (the host has flattened them), `depth` seams
 * in the direction `orientation` (0: the width changes).  transposed: the carvers lie transposed (their base layout's rows are image
 * columns); luma: the value read is luma; w_start: what the bias is divided by.  device_maps: n maps in device memory, width x height
 * ints each, image orientation -- or NULL, and the build keeps maps of its own (lqrhip_forward_map, lqrhip_forward_read_map).
 *   lqrhip_forward_begin    checks, allocates EVERYTHING the build needs and enqueues the one-off pass (k_fwd_init): LQRHIP_ENOMEM has
 *                           launched nothing and given every block back
 *   lqrhip_forward_seams    enqueues seams first_seam .. first_seam + n_seams - 1 (0-based, in order, every one once): two launches per
 *                           seam whatever n is.  Returns once the slice BEFORE this one has completed, so that the host is never more
 *                           than two slices ahead of the device and can stop between them
 *   lqrhip_forward_finish   waits for the build; 0: the maps are complete
 *   lqrhip_forward_release  waits for whatever is still queued and gives the build's blocks back (at any point, also instead of finish)
 * The build runs on the shim's own stream; it reads the carvers' base layouts and changes nothing of theirs.
 * A build takes at most LQRHIP_FORWARD_MAX_LINES lines per image and as many images (the launch grids' second dimension); the host
 * refuses more up front.
 * lqrhip_forward_launches: kernel launches of forward builds so far (test hook).  The counter is atomic: this one call MAY BE POLLED
 * FROM ANOTHER THREAD while a build runs (a test's second thread times its lqr_carver_cancel by it).  lqrhip_forward_intensity: the I
 * plane the one-off pass forms for one carver, H lines of L floats in the frame of the carving direction, to host memory (test hook). */
#define LQRHIP_FORWARD_MAX_LINES 65535
typedef struct LqrHipForward LqrHipForward;
int lqrhip_forward_begin(LqrHipCarver *const *cs, int n, int depth, int orientation, int transposed, int luma, int w_start,
                         void *const *device_maps, LqrHipForward **out);
int lqrhip_forward_seams(LqrHipForward *f, int first_seam, int n_seams);
int lqrhip_forward_finish(LqrHipForward *f);
const int *lqrhip_forward_map(const LqrHipForward *f, int i);       /* image i's map, device memory (after finish) */
int lqrhip_forward_read_map(LqrHipForward *f, int i, int *out);    /* ... copied to host memory */
void lqrhip_forward_release(LqrHipForward *f);
unsigned long long lqrhip_forward_launches(int reset);
int lqrhip_forward_intensity(LqrHipCarver *c, int orientation, int transposed, int luma, float *out);
/* (host/lqr_carver.c) the same for a LqrCarver, which must be flat: what tests/test_forward_gpu.py compares with the model's I */
int lqrhip_read_forward_intensity(const void *carver, int orientation, float *out);
/* lqr_static.h: the frames of a clip -- n FLAT root carvers of one shape and pixel kind (the host has flattened them), lying `transposed`
 * or not -- folded into the energy plane E of static seams, width x height floats in IMAGE orientation, as seams of `orientation` see it
 * (nrg_func: the frames' LqrEnergyFuncBuiltinType; alpha in [0, 1]).
 *   lqrhip_static_begin    checks and allocates EVERYTHING the fold needs (the table of frame pointers, the running planes of a clip of
 *                          more than 16 frames, and E unless device_energy names the caller's device memory): LQRHIP_ENOMEM has launched
 *                          nothing and given every block back
 *   lqrhip_static_groups   the launches the fold takes: one per 16 frames
 *   lqrhip_static_fold     enqueues the next group (k_static_fold; the last one writes E); the host looks for a cancel between them
 *   lqrhip_static_finish   waits for the fold; host_energy non-NULL: E is copied there.  0: E is complete
 *   lqrhip_static_energy   E in device memory, valid until the release
 *   lqrhip_static_release  waits for whatever is still queued and gives the blocks back (at any point, also instead of finish) */
#define LQRHIP_STATIC_MAX_FRAMES 65535
typedef struct LqrHipStatic LqrHipStatic;
int lqrhip_static_begin(LqrHipCarver *const *cs, int n, int orientation, int transposed, int nrg_func, float alpha, void *device_energy,
                        LqrHipStatic **out);
int lqrhip_static_groups(const LqrHipStatic *st);
int lqrhip_static_fold(LqrHipStatic *st);
int lqrhip_static_finish(LqrHipStatic *st, float *host_energy);
const float *lqrhip_static_energy(const LqrHipStatic *st);
void lqrhip_static_release(LqrHipStatic *st);
/* lqr_clipforward.h: ONE forward-energy seam map from all n frames of a clip -- FLAT root carvers of one shape and pixel kind (the host has
 * flattened them), lying `transposed` or not -- `depth` seams in the direction `orientation`.  luma, w_start: as lqrhip_forward_begin's;
 * temporal: a finite float >= 0.  device_map: the caller's device memory, width x height ints in image orientation -- or NULL, and the
 * build keeps a map of its own (lqrhip_clipfwd_map, lqrhip_clipfwd_read_map).  The family mirrors lqrhip_forward_*:
 *   lqrhip_clipfwd_begin    checks, allocates EVERYTHING the build needs and enqueues the one-off passes (k_fwd_init for the I planes, one
 *                           k_clip_fold per 16 frames): LQRHIP_ENOMEM has launched nothing and given every block back
 *   lqrhip_clipfwd_seams    enqueues seams first_seam .. first_seam + n_seams - 1 (0-based, in order, every one once): at most three
 *                           launches per seam whatever n is.  Returns once the slice BEFORE this one has completed
 *   lqrhip_clipfwd_finish   waits for the build; 0: the map is complete
 *   lqrhip_clipfwd_release  waits for whatever is still queued and gives the build's blocks back (at any point, also instead of finish)
 * The build runs on the shim's own stream; it reads the carvers' base layouts and changes nothing of theirs.  Lines and frames: at most
 * LQRHIP_FORWARD_MAX_LINES each.  lqrhip_clipfwd_launches: kernel launches of clip builds so far (test hook; atomic, MAY BE POLLED FROM
 * ANOTHER THREAD while a build runs).  They are not counted by lqrhip_forward_launches or the launch census. */
typedef struct LqrHipClipFwd LqrHipClipFwd;
int lqrhip_clipfwd_begin(LqrHipCarver *const *cs, int n, int depth, int orientation, int transposed, int luma, int w_start, float temporal,
                         void *device_map, LqrHipClipFwd **out);
int lqrhip_clipfwd_seams(LqrHipClipFwd *f, int first_seam, int n_seams);
int lqrhip_clipfwd_finish(LqrHipClipFwd *f);
const int *lqrhip_clipfwd_map(const LqrHipClipFwd *f);             /* the map, device memory (after finish) */
int lqrhip_clipfwd_read_map(LqrHipClipFwd *f, int *out);          /* ... copied to host memory */
void lqrhip_clipfwd_release(LqrHipClipFwd *f);
unsigned long long lqrhip_clipfwd_launches(int reset);
/* bench hook: the device time the fold of the last FINISHED build took (k_clip_fold's launches, first to last), in ms */
double lqrhip_clipfwd_fold_ms(void);
int lqrhip_device_sync(void);
/* free / total device memory in bytes (hipMemGetInfo) and the bytes the shim's allocation cache holds */
int lqrhip_mem_info(unsigned long long *free_bytes, unsigned long long *total_bytes, unsigned long long *cached_bytes);
/* Measured HBM ceiling of this device: a 16-byte-per-lane streaming copy of `bytes` bytes, `iters` times;
 * returns read+write GB/s through *gbps (the denominator bench.py reports next to the nominal 8 TB/s). */
int lqrhip_copy_bandwidth(unsigned long long bytes, int iters, double *gbps);
/* the colour ramp of write_vmap_to_layer (src/io_functions.c:249-279) over a
 * w x h visibility map: value = (depth+1-vs)/(depth+1), RGB = value*start + (1-value)*end,
 * alpha = 0.5*(1+value), each channel (guchar)(255*x); vs == 0 -> 0,0,0,0.  Host buffers. */
int lqrhip_vmap_to_rgba(const int *vmap, int w, int h, int depth, const double col_start[3], const double col_end[3],
                        unsigned char *out_rgba);
/* return the cached (freed) device blocks of the shim's allocation cache to the driver */
void lqrhip_pool_trim(void);
/* E12 lqr_vmap_dump (render.c:725): vs of the pixels visible at `level`
 * minus `depth` (0 stays 0), w x h in carver orientation */
int lqrhip_read_vmap(LqrHipCarver *c, int w0, int h0, int w, int level, int depth, int *out);
/* test hooks behind lqrx_carver_get_energy / lqrx_carver_debug_maps */
int lqrhip_read_working(LqrHipCarver *c, int w, int h, float *en, float *m, int *least_dx);
/* Test hook: the flags the backtrack published for the last seam: the origin of the carved planes, the origin before that seam, and
 * the side of it the carve moved (0: the right part one to the left; 1: the left part one to the right, the origin advances) */
int lqrhip_read_seam_flags(LqrHipCarver *c, int *org, int *org_prev, int *side);
/* ... and as lqrx_set_debug(1) recorded them with the snapshot of the planes after a session's last seam (include/lqr.h).  `carver` is
 * the LqrCarver (host/lqr_carver.c implements this one); 0, or LQRHIP_EARG where there is no snapshot */
int lqrhip_debug_seam_flags(const void *carver, int *org, int *org_prev, int *side);

/* kernel-time accounting for bench.py: accumulated HIP-event time (ms) and
 * launch count of the carve kernel (the roofline kernel) since the last reset */
/* 0 off; 1 HIP-event pairs around every kernel of the seam loop; 2 around k_carve only (each pair costs ~10 us
 * of queue time, so the bench's timed region uses 2 and takes the other kernels' times from rocprofv3) */
void lqrhip_prof_enable(int on);
/* how E9 (update_mmap) runs: -1 by batch size (tiled full-width keep-rule sweep up to 8 4K images, the band
 * kernel k_band_update_tw above), 0 band kernel always, 1 tiled sweep whenever its grid fits the device,
 * 2 the per-row-barrier band kernel k_band_update_mw (the default for rows wider than 4200 px), 3 the generic
 * one-wave band kernel k_band_update + k_dp_sweep (what delta_x 0 and delta_x > 10 run on, and delta_x 2 .. 10 / rigidity
 * masks where the tiled update's grid does not fit) whatever the parameters, 5 k_band_levels
 * (4 was round 4's k_band_tiles, removed in round 6: it now behaves as 0) */
void lqrhip_set_update_mode(int mode);
/* Test hook: threads of the k_dp_sweep<UPDATE> launch behind the band kernels: 256 (default) or 1024 */
void lqrhip_set_sweep_threads(int n);
/* Test hook: the largest group that runs the carve and the energy update as one launch (k_carve_e, delta_x <= 2): 0 = never, 1 = the
 * default (4), n = groups up to n images */
void lqrhip_set_carve_fused(int max_images);
/* Test hook: the energy update as workgroups of the carve's launch (k_carve_u, delta_x <= 2, packed pixels, groups too large for
 * k_carve_e): -1 = automatic (groups that have their stream to themselves, from the size lqr_plan.h names), 0 = never (k_carve, then
 * k_emap_update), 1 = wherever a form exists.  The launch is counted under LQRHIP_CENSUS_CARVE either way;
 * lqrhip_carve_beside_launches returns how many of them were combined launches since the last reset */
void lqrhip_set_carve_beside(int mode);
unsigned long long lqrhip_carve_beside_launches(int reset);
/* Test hook: the backtrack as a role of that launch too (k_carve_v: the one-wave walk hands rows to the carve and the energy update
 * of the same launch as it finds them; delta_x 1 and 2, frames of 37 to 4096 rows, where the energy update runs beside the carve and
 * spinning kernels are allowed; never on the step that compacts the frozen planes): -1 = automatic (groups that have their stream to
 * themselves, from the size lqr_plan.h names), 0 = never (k_vpath1, then k_carve_u), 1 = wherever a form exists.  Such a launch is
 * counted under LQRHIP_CENSUS_VPATH1 and LQRHIP_CENSUS_CARVE and as a carve-beside launch; lqrhip_backtrack_beside_launches returns how
 * many there were since the last reset.  Same seams, planes, flags and moved bytes either way */
void lqrhip_set_backtrack_beside(int mode);
unsigned long long lqrhip_backtrack_beside_launches(int reset);
/* E7 form: -1 = the parallel two-kernel backtrack (k_vp_maps / k_vp_solve) for groups of up to par_max images (default 3; 0 keeps the
 * current value) of 1000 rows and more, the one-wave walk k_vpath1 otherwise; 0 = k_vpath1 always; 1 = the parallel form
 * always (delta_x 1 .. 4) */
void lqrhip_set_vpath_mode(int mode, int par_max);
/* Cap on the workgroups of the persistent tiled DP sweep (k_dp_tile_p), whose tiles spin on their neighbours and
 * must all be resident: -1 = the bound derived from the occupancy query at lqrhip_init, n >= 0 = min(n, that bound).
 * Grids above the cap run as k_dp_tile (one launch per 32 rows).  0 forces that path (tests). */
void lqrhip_set_dp_persistent_limit(int workgroups);
/* Geometry of the persistent tiled sweep: 0 = by batch size (3 = 2 px per lane, 32-column tiles with 48-column halos and 48-row blocks
 * while every tile has a compute unit to itself; 2 = 2 px per lane, 64-column tiles, 32-row blocks while twice the tiles fit the
 * residency bound; else 4 px per lane), 2 / 3 / 4 = pinned (tests) */
void lqrhip_set_dp_persistent_px(int px);
void lqrhip_prof_reset(void);
int lqrhip_prof_get(const char *kernel, double *ms_total, long long *launches, double *bytes_total);
/* time during which at least one launch of `kernel` was running (launches of sub-batch streams overlap) */
int lqrhip_prof_get_union(const char *kernel, double *ms_union);
/* Bytes the carves of this process HAD to move (read + write) since the last reset: k_vpath* knows, for the seam it found, how
 * many pixels lie on the side the carve will move, and sums pixels x bytes per pixel (en; m and back pointer unless a full DP
 * follows; the rigidity mask) over images and seams.  The roofline's numerator next to SURVEY 8(d)'s half-row figure. */
int lqrhip_moved_bytes(unsigned long long *bytes, int reset);
/* Test hook: slots (workgroups) per image of k_band_levels (-1 automatic, 0 never, n exactly n). */
void lqrhip_set_band_levels(int slots);
/* Test hook: slots per WORKGROUP of the level kernel: -1 automatic, 1 never two (k_band_levels), 2 two (k_band_levels2) wherever a form
 * exists (delta_x 1, no rigidity mask that matters, at least 2 slots per image) and its grid is resident. */
void lqrhip_set_levels_wg_slots(int slots);
/* Test hook: where the groups of a carved row start or end (k_carve_e, k_carve_u, k_carve_v; k_carve keeps 0 whatever this says): 0 on a
 * 16-byte vector, as it used to be, 1 on a 32-element boundary -- a 128-byte line of the float planes -- so that a wave's accesses cover
 * whole lines, -1 automatic (plan_carve_line: 1 for k_carve_u and k_carve_v, 0 for k_carve_e).  The same vectors are loaded and stored either way: same seams, planes, flags and
 * moved bytes. */
void lqrhip_set_carve_line(int mode);
/* Test hook: what the level kernel writes back (k_band_levels2 only: k_band_levels ignores it and writes everything): 0 every row of every processed tile-level from every lane (the lanes
 * that own nothing to the spare row), 1 of an interior tile only the rows on which an own pixel changed, and of those only from the
 * own lanes that changed a pixel on any row of the level -- unchanged own lanes and all halo lanes are switched off (what is not
 * written holds what was loaded from the same addresses), -1 automatic (plan_levels_store: 1 wherever k_band_levels2 runs). */
void lqrhip_set_levels_store(int mode);
/* launches of k_band_levels2 since the last reset (they are counted under LQRHIP_CENSUS_BAND_LEVELS as well) */
unsigned long long lqrhip_levels_pair_launches(int reset);
/* k_band_levels' events since the last reset: [0] images stopped by THREE active tiles on one slot (a slot takes two, one per
 * wave; the full-width sweep took over), [1] synchronous (mispredicted or second-tile) loads, [2] tile-levels processed,
 * [3] slot-levels idle, [4] levels in which a slot had two tiles, [5] rows of processed tile-levels written back, [6] rows not written
 * because no own pixel changed on them -- both counted only while lqrhip_set_levels_store is pinned to 0 or 1 */
int lqrhip_band_levels_stats(unsigned long long *out8, int reset);
/* Test hook: the launch census -- which FORM of each stage the shim launched since the last reset, counted on the host at the
 * launch sites (lqrhip_prof_get's names do not tell: "band_update" is four kernels, "dp_update" every sweep).  Copies the first
 * min(n, LQRHIP_CENSUS_SLOTS) counters to `out`, clears all of them if `reset`, and returns LQRHIP_CENSUS_SLOTS.  Kernel launches
 * are counted, one per launch whatever the size of the batch (k_vp_maps + k_vp_solve count as one backtrack). */
enum {
    LQRHIP_CENSUS_VP_PARALLEL = 0,      /* E7: k_vp_maps / k_vp_solve */
    LQRHIP_CENSUS_VPATH1 = 1,           /*     k_vpath1<delta_x> */
    LQRHIP_CENSUS_VPATH = 2,            /*     k_vpath */
    LQRHIP_CENSUS_CARVE_E = 3,          /* E8: k_carve_e (carve + energy update) */
    LQRHIP_CENSUS_CARVE = 4,            /*     k_carve */
    LQRHIP_CENSUS_TILE_P_G3 = 5,        /* E5 / E9: k_dp_tile_p, geometry 3 (32-column tiles, plain) */
    LQRHIP_CENSUS_TILE_P_G2 = 6,        /*     geometry 2 (64-column tiles, plain) */
    LQRHIP_CENSUS_TILE_P_G4 = 7,        /*     4 px per lane (plain) */
    LQRHIP_CENSUS_TILE_P_GENERAL = 8,   /*     the delta_x 2 .. 10 / rigidity-mask instantiations */
    LQRHIP_CENSUS_DP_TILE = 9,          /* E5: k_dp_tile, one launch per 32 rows */
    LQRHIP_CENSUS_BAND_LEVELS = 10,     /* E9: k_band_levels */
    LQRHIP_CENSUS_BAND_TW = 11,         /*     k_band_update_tw */
    LQRHIP_CENSUS_BAND_MW8 = 12,        /*     k_band_update_mw, 8 waves */
    LQRHIP_CENSUS_BAND_MW16 = 13,       /*     k_band_update_mw, 16 waves */
    LQRHIP_CENSUS_BAND_GENERIC = 14,    /*     k_band_update (one wave) */
    LQRHIP_CENSUS_SWEEP = 15,           /* k_dp_sweep<P, ., T>: slot 15 + 2 * log2(P) + (T == 1024), P = 1, 2, 4, 8, 16 px per thread */
    LQRHIP_CENSUS_SWEEP_FULL = 25,      /* ... of these, the full DPs (E5) */
    LQRHIP_CENSUS_SWEEP_UPDATE = 26,    /* ... and the launches behind a band kernel (E9) */
    LQRHIP_CENSUS_LDS_ATTR_SWEEP = 27,  /* k_dp_sweep launches with more than 64 KB of dynamic LDS (hipFuncSetAttribute first) */
    LQRHIP_CENSUS_LDS_ATTR_COMMIT = 28, /* k_vs_commit launches with more than 64 KB of dynamic LDS */
    LQRHIP_CENSUS_COMPACT_SIZES = 29,   /* lqrhip_read_sizes: k_compact_sizes, one launch per chunk of sizes */
    LQRHIP_CENSUS_TRANSPOSE_SIZES = 30, /*     k_transpose_sizes, likewise (a carver that lies transposed) */
    LQRHIP_CENSUS_STATIC_FOLD = 31,     /* lqrhip_static_fold: k_static_fold, one launch per group of 16 frames (lqr_static.h) */
    LQRHIP_CENSUS_SLOTS = 32
};
int lqrhip_launch_census(unsigned long long *out, int n, int reset);

#ifdef __cplusplus
}
#endif
#endif /* LQR_HIP_H */
