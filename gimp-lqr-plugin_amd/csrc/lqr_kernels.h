// lqr_kernels.h -- every kernel of the engine, declared for the host shim (lqr_shim.hip), which launches them, and included by
// the file that defines each (so that declaration and definition cannot drift apart).  A template family with more than one
// instantiation has its set written ONCE, as an X-macro list (K_*_FORMS) next to its declaration.  Three things derive from it: the
// explicit instantiations at the end of the family's k_*.hip, the shim's launch (it picks the entry that equals the run-time values,
// and refuses values no entry has) and, for the two spinning families, the occupancy queries behind the residency bounds
// (dpp_resident_workgroups) -- so a kernel that can be launched cannot be missing from either.
#pragma once
#include "lqr_common.h"
#include "lqr_pixel.h"

// Kernels that touch pixels take the pixel's form as a compile-time parameter (lqr_pixel.h): FORM = PixPacked or PixValue<DEPTH>, VALUE =
// the working plane holds one double per pixel (carvers that are not 8-bit grey / RGB (+ alpha)), DEEP = base-layout pixels beyond 4 x 8 bits

// k_energy.hip
template <class FORM> __global__ void k_wk_init(const DevCarver *cs, int w, int h, int stride, typename FORM::Arg a);
template <class FORM> __global__ __launch_bounds__(256) void k_wk_init_visible(const DevCarver *cs, int w0, int h, int stride, typename FORM::Arg a);
// X(NRG, VALUE): k_emap_full, and k_emap_update at each sample count.  The value forms exist for energies 0, 1, 2 and 6 only (plane_nrg in lqr_shim.hip)
#define K_EMAP_FORMS(X) X(0, false) X(1, false) X(2, false) X(3, false) X(4, false) X(5, false) X(6, false) X(0, true) X(1, true) X(2, true) X(6, true)
#define K_EMAP_UPDATE_NT_FORMS(X, ...) X(12, __VA_ARGS__) X(36, __VA_ARGS__) X(68, __VA_ARGS__)      // brightness samples per row (eu_samples in lqr_plan.h)
template <int NRG, bool VALUE> __global__ void k_emap_full(const DevCarver *cs, DpK p, int w, int h, int stride);
#define K_WK_INIT_EMAP_FORMS(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6)     // LqrEnergyFuncBuiltinType; packed pixels only
template <int NRG> __global__ __launch_bounds__(256) void k_wk_init_emap(const DevCarver *cs, DpK p, int w, int h, int stride);
__global__ void k_mask_add(float *plane, int w0, const uint8_t *mask, int channels, int mw, int x0, int y0, int x1, int y1,
                           int nx, int ny, int transposed, int is_rig, int bias_factor);
template <int NRG, int EU_NT, bool VALUE> __global__ __launch_bounds__(64) void k_emap_update(const DevCarver *cs, DpK p, int w, int h, int stride, int k, int epoch);
template <bool VALUE> __global__ __launch_bounds__(256) void k_frozen_catchup(const DevCarver *cs, int from, int to, int w_from, int h, int stride);

// k_backtrack.hip
__global__ __launch_bounds__(VPATH_THREADS) void k_vpath(const DevCarver *cs, int w, int h, int stride, int lr, int delta, int log_index, int moved_unit);
#define K_VPATH1_FORMS(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7)
#define K_VP_FORMS(X) K_VPATH1_FORMS(X) X(8) X(9) X(10)         // k_vp_maps and k_vp_solve: delta_x 1 .. LQR_FAST_MAX_DELTA
template <int DELTA> __global__ __launch_bounds__(VPATH_THREADS) void k_vpath1(const DevCarver *cs, int w, int h, int stride, int lr, int log_index, int moved_unit);
unsigned long long *lqr_moved_bytes_dev(void);        // g_moved_bytes' device address (nullptr: not to be had), for k_carve_v's walk role

template <int DELTA> __global__ __launch_bounds__(256) void k_vp_maps(const DevCarver *cs, int w, int h, int stride);
template <int DELTA> __global__ __launch_bounds__(VPATH_THREADS) void k_vp_solve(const DevCarver *cs, int w, int h, int stride, int lr, int log_index, int moved_unit);

// k_carve.hip
__global__ __launch_bounds__(256) void k_carve(const DevCarver *cs, int w, int h, int stride, int delta, int move_dp);
#define K_CARVE_E_FORMS(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6)      // LqrEnergyFuncBuiltinType
template <int NRG> __global__ __launch_bounds__(256) void k_carve_e(const DevCarver *cs, DpK p, int w, int h, int stride, int move_dp, int k, int epoch, int line);
#define K_CARVE_U_FORMS(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6)      // LqrEnergyFuncBuiltinType; 12 samples per row (delta_x <= 2), packed pixels
template <int NRG> __global__ __launch_bounds__(256) void k_carve_u(const DevCarver *cs, DpK p, int w, int h, int stride, int move_dp, int k, int epoch, int n, int line);
// X(NRG, DELTA): the walk role has k_vpath1's forms for delta_x 1 and 2 (K_CARVE_V_DELTAS), the energy role K_CARVE_U_FORMS'
#define K_CARVE_V_DELTAS(X) X(1) X(2)
#define K_CARVE_V_FORMS(X) X(0, 1) X(1, 1) X(2, 1) X(3, 1) X(4, 1) X(5, 1) X(6, 1) X(0, 2) X(1, 2) X(2, 2) X(3, 2) X(4, 2) X(5, 2) X(6, 2)
// (five waves per SIMD, the carve's occupancy: the three roles together must fit its 96 registers)
template <int NRG, int DELTA> __global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5))) void k_carve_v(const DevCarver *cs, DpK p, int w, int h, int stride, int lr, int move_dp, int k, int epoch, int n,
                                                                                  int moved_unit, unsigned tag, unsigned long long *list, unsigned long long *moved_bytes, int *dev_err, int line);

// k_band.hip
#define K_DP_SWEEP_PXT_FORMS(X) X(1) X(2) X(4) X(8) X(16)       // each as <P, false, DP_THREADS>, <P, true, DP_THREADS> and <P, true, 256>
#define K_LR_RIG_FORMS(X) X(false, false) X(false, true) X(true, false) X(true, true)       // k_dp_tile, k_band_update_tw<4, ..>, k_band_update_mw<2, 8 | 16, 8, ..>
template <int PXT, bool UPDATE, int NTH = DP_THREADS> __global__ __launch_bounds__(NTH) void k_dp_sweep(const DevCarver *cs, DpK p, int w, int h, int stride, int lr);
__global__ __launch_bounds__(64) void k_band_update(const DevCarver *cs, DpK p, int w, int h, int stride, int lr);
template <int PXL, int NW, int R, bool LR, bool RIG> __global__ __launch_bounds__(64 * NW) void k_band_update_mw(const DevCarver *cs, DpK p, int w, int h, int stride);
template <int NW, bool LR, bool RIG> __global__ __launch_bounds__(128 * NW) void k_band_update_tw(const DevCarver *cs, DpK p, int w, int h, int stride, int *dev_err);

// k_tiles.hip
template <bool LR, bool RIG> __global__ __launch_bounds__(64) void k_dp_tile(const DevCarver *cs, DpK p, int w, int h, int stride, int y0);
// X(CLASS, PX, LR, RIG, UPDATE, DELTA, RIGM, HLN).  CLASS is the residency class (dpp_resident_workgroups): PX4 the plain 4-px forms,
// PLAIN the plain 2-px forms and their 24-halo-lane geometry (px code 3), GENERAL delta_x 2 .. 10 and / or a rigidity mask (2 px only).
// delta_x 5 .. 10 exist in the rigidity form only (dp_form in lqr_shim.hip).  (The order is the one they have always been instantiated in:
// a kernel's pc-relative offset to the file's globals is part of its code, and scripts/kernel_diff.py compares code.)
#define K_DP_TILE_P_FORMS_D(X, LR, UPD, D) X(GENERAL, 2, LR, false, UPD, D, false, 16) X(GENERAL, 2, LR, true, UPD, D, false, 16) X(GENERAL, 2, LR, true, UPD, D, true, 16)
#define K_DP_TILE_P_FORMS_W(X, LR, UPD, D) X(GENERAL, 2, LR, true, UPD, D, false, 16) X(GENERAL, 2, LR, true, UPD, D, true, 16)
#define K_DP_TILE_P_FORMS_LR(X, LR, UPD) \
    X(PX4, 4, LR, false, UPD, 1, false, 16) X(PX4, 4, LR, true, UPD, 1, false, 16) X(PLAIN, 2, LR, false, UPD, 1, false, 16) X(PLAIN, 2, LR, true, UPD, 1, false, 16) \
    X(GENERAL, 2, LR, true, UPD, 1, true, 16) K_DP_TILE_P_FORMS_D(X, LR, UPD, 2) K_DP_TILE_P_FORMS_D(X, LR, UPD, 3) K_DP_TILE_P_FORMS_D(X, LR, UPD, 4) \
    K_DP_TILE_P_FORMS_W(X, LR, UPD, 5) K_DP_TILE_P_FORMS_W(X, LR, UPD, 6) K_DP_TILE_P_FORMS_W(X, LR, UPD, 7) K_DP_TILE_P_FORMS_W(X, LR, UPD, 8) K_DP_TILE_P_FORMS_W(X, LR, UPD, 9) K_DP_TILE_P_FORMS_W(X, LR, UPD, 10)
#define K_DP_TILE_P_FORMS_24(X, UPD) X(PLAIN, 2, false, false, UPD, 1, false, 24) X(PLAIN, 2, false, true, UPD, 1, false, 24) X(PLAIN, 2, true, false, UPD, 1, false, 24) X(PLAIN, 2, true, true, UPD, 1, false, 24)
#define K_DP_TILE_P_FORMS(X) K_DP_TILE_P_FORMS_LR(X, false, false) K_DP_TILE_P_FORMS_LR(X, false, true) K_DP_TILE_P_FORMS_LR(X, true, false) K_DP_TILE_P_FORMS_LR(X, true, true) \
    K_DP_TILE_P_FORMS_24(X, false) K_DP_TILE_P_FORMS_24(X, true)
template <int PX, bool LR, bool RIG, bool UPDATE, int DELTA = 1, bool RIGM = false, int HLN = 16>
__global__ __launch_bounds__(64 * DPP_W) void k_dp_tile_p(DevCarver *cs, DpK p, int w, int h, int stride, unsigned long long *exch, int epoch, int *dev_err);

// k_levels.hip
// X(LR, RIG, DELTA, RIGM): one residency class
#define K_BAND_LEVELS_FORMS_D(X, LR, D) X(LR, false, D, false) X(LR, true, D, false) X(LR, true, D, true)
#define K_BAND_LEVELS_FORMS_W(X, LR, D) X(LR, true, D, false) X(LR, true, D, true)
#define K_BAND_LEVELS_FORMS_LR(X, LR) K_BAND_LEVELS_FORMS_D(X, LR, 1) K_BAND_LEVELS_FORMS_D(X, LR, 2) K_BAND_LEVELS_FORMS_D(X, LR, 3) K_BAND_LEVELS_FORMS_D(X, LR, 4) \
    K_BAND_LEVELS_FORMS_W(X, LR, 5) K_BAND_LEVELS_FORMS_W(X, LR, 6) K_BAND_LEVELS_FORMS_W(X, LR, 7) K_BAND_LEVELS_FORMS_W(X, LR, 8) K_BAND_LEVELS_FORMS_W(X, LR, 9) K_BAND_LEVELS_FORMS_W(X, LR, 10)
#define K_BAND_LEVELS_FORMS(X) K_BAND_LEVELS_FORMS_LR(X, false) K_BAND_LEVELS_FORMS_LR(X, true)
template <bool LR, bool RIG, int DELTA, bool RIGM>
__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_band_levels(DevCarver *cs, DpK p, int w, int h, int stride, unsigned long long *exch, int epoch, int *dev_err, int P, int n_img, int store_rows);

// k_levels2.hip: two slots of an image per workgroup.  X(LR, RIG): delta_x 1, no rigidity mask; one residency class of its own
#define K_BAND_LEVELS2_FORMS(X) X(false, false) X(false, true) X(true, false) X(true, true)
template <bool LR, bool RIG>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_band_levels2(DevCarver *cs, DpK p, int w, int h, int stride, unsigned long long *exch, int epoch, int *dev_err, int P, int n_img, int store_rows);
void lqr_levels_report_rows(int on);                            // lqrhip_band_levels_stats reports entries 5 and 6 (k_levels.hip)
void lqr_levels2_debug(int v);                                  // lqrhip_band_levels_debug's switches for this family's device global
int lqr_levels2_stats(unsigned long long *out, int reset);      // adds this family's event counters to out[0 .. 8)

// k_oneoff.hip
__global__ __launch_bounds__(256) void k_vs_commit(const DevCarver *cs, int w0, int h0, int wc0, int n_seams, int first_level, int finish);
template <bool DEEP> __global__ __launch_bounds__(256) void k_inflate(const InflateDev *jobs, int w0, int w1, int l, int max_level, int *dev_err);
__global__ __launch_bounds__(256) void k_vmap_check(const int32_t *map, int len, int depth, int *dev_err);
__global__ __launch_bounds__(256) void k_vmap_check_t(const int32_t *map, int32_t *out, int width, int height, int depth, int *dev_err);
__global__ __launch_bounds__(256) void k_seam_check(const DevCarver *cs, int h, int wc0, int n_seams, int delta, int *dev_err);
__global__ __launch_bounds__(256) void k_vs_rollback(const DevCarver *cs, size_t n, int first_level, int finish_level);
__global__ void k_inject(const DevCarver *cs, int what, int h, int w0, int log_index, int first_level);
template <bool DEEP> __global__ __launch_bounds__(256) void k_compact(const uint8_t *rgb, const int32_t *vs, const float *bias, const float *rig,
                                                  uint8_t *nrgb, float *nbias, float *nrig, int32_t *nvmap, int w0, int w, int ch, int level, int depth);
template <bool DEEP> __global__ __launch_bounds__(256) void k_compact_jobs(const InflateDev *jobs, int w0, int w, int level);
__global__ void k_transpose(const InflateDev *jobs, int w, int h);
__global__ void k_transpose_px(const InflateDev *jobs, int w, int h);
__global__ __launch_bounds__(256) void k_mask_line_max(const uint8_t *mask, int channels, int width, int a0, int b0, int line_len, int direction, int *out);

// k_sizes.hip (a carver read at many sizes in one pass, include/lqr_sizes.h).  X(DEEP): base-layout pixels wider than 4 bytes;
// X(WIDE) of the transposition: the same split (jobs' pixels move through an LDS tile of dwords, or pixel by pixel)
#define K_COMPACT_SIZES_FORMS(X) X(false) X(true)
#define K_TRANSPOSE_SIZES_FORMS(X) X(false) X(true)
template <bool DEEP> __global__ __launch_bounds__(256) void k_compact_sizes(const uint8_t *rgb, const int32_t *vs, const SizeJob *jobs, int n_jobs, int w0, int bytes);
template <bool WIDE> __global__ __launch_bounds__(256) void k_transpose_sizes(const SizeJob *jobs, int h, int bytes);

// k_forward.hip (forward-energy seam maps, include_ext/lqr_forward.h).  X(DEPTH) of the one-off pass: LqrColDepth; X(PXT) of the seam kernel:
// pixels per thread.  One workgroup per image in k_fwd_seam (grid n), one per line and image in k_fwd_remove (grid H x n)
#define K_FWD_INIT_FORMS(X) X(0) X(1) X(2) X(3)
#define K_FWD_SEAM_FORMS(X) X(1) X(2) X(4) X(8) X(16)
template <int DEPTH> __global__ __launch_bounds__(256) void k_fwd_init(const FwdJob *jobs, int L, int H, int fw0, int strided, DeepRead rd, int w_start, int orientation);
template <int PXT> __global__ __launch_bounds__(FWD_THREADS) void k_fwd_seam(const FwdJob *jobs, int wc, int L, int H);
__global__ __launch_bounds__(FWD_REMOVE_THREADS) void k_fwd_remove(const FwdJob *jobs, int wc, int L, int H, int level, int orientation);

// k_clipfwd.hip (forward-energy seams for a clip, include_ext/lqr_clipforward.h).  The I planes of the n frames lie one after the other in
// `in` (frame t at clip_frame_off(t, px)); `cost` holds CU, CL, CR and Q of a pixel side by side (clip_cost_off).  X(PXT) of the seam kernel:
// pixels per thread.  Grids: the fold a workgroup per CLIPFWD_FOLD_THREADS pixels of a line x H; the seam kernel one workgroup; the removal
// and the refresh one workgroup per line
#define K_CLIP_SEAM_FORMS(X) X(1) X(2) X(4) X(8) X(16)
__global__ __launch_bounds__(CLIPFWD_FOLD_THREADS) void k_clip_fold(const FwdJob *jobs, const float *in, int first, int count, int last, int L, int H, int fw0, int strided,
                                                                   int w_start, float temporal, float *cost, float *pm);
template <int PXT> __global__ __launch_bounds__(FWD_THREADS) void k_clip_seam(const float *cost, int8_t *choice, int32_t *seam, int wc, int L, int H);
__global__ __launch_bounds__(FWD_REMOVE_THREADS) void k_clip_remove(float *cost, uint16_t *pos, const int32_t *seam, int32_t *map, int wc, int L, int H, int level, int orientation);
__global__ __launch_bounds__(CLIPFWD_REFRESH_THREADS) void k_clip_refresh(const float *in, int n, float *cost, const uint16_t *pos, const int32_t *seam, int wn, int L, int H);

// k_static.hip (static seams for a clip, include_ext/lqr_static.h).  X(NRG, DEPTH, PACKED): NRG 0 / 1 / 2 / 6 (luma is DeepRead.luma, as on the value
// plane: plane_nrg in lqr_shim.hip), DEPTH the LqrColDepth, PACKED 8-bit grey / RGB (+ alpha) through px_bright.  Grid: tiles across x tiles down
#define K_STATIC_FOLD_FORMS(X) X(0, 0, true) X(1, 0, true) X(2, 0, true) X(6, 0, true) X(0, 0, false) X(1, 0, false) X(2, 0, false) X(6, 0, false) \
    X(0, 1, false) X(1, 1, false) X(2, 1, false) X(6, 1, false) X(0, 2, false) X(1, 2, false) X(2, 2, false) X(6, 2, false) \
    X(0, 3, false) X(1, 3, false) X(2, 3, false) X(6, 3, false)
template <int NRG, int DEPTH, bool PACKED>
__global__ __launch_bounds__(STATIC_THREADS) void k_static_fold(const StaticFrame *frames, int count, int first, int W, int H, int transposed, int orientation, DeepRead rd,
                                                     float alpha, float *s_plane, float *t_plane, float *i_plane, float *e_out);

// k_discard.hip (the discard scan, include_ext/lqr_remove.h).  One form each.  Grids (lqr_geom.h): the line scan a workgroup per base-layout
// row, the ranked scan too; the cross scan discard_col_blocks(w0) x discard_row_tiles(h0); the fold discard_col_blocks(columns).  res: a scan's DISCARD_WORDS result words
__global__ __launch_bounds__(DISCARD_THREADS) void k_discard_line(const float *bias, const int32_t *vs, int w0, float thr, int level, int depth, int *res);
__global__ __launch_bounds__(DISCARD_THREADS) void k_discard_cross(const float *bias, const int32_t *vs, int w0, int h0, float thr, int level, int depth,
                                                                 int *partial, int *res);
__global__ __launch_bounds__(DISCARD_THREADS) void k_discard_rank(const float *bias, const int32_t *vs, int w0, int w, float thr, int level, int depth, int *col,
                                                                int *res);
__global__ __launch_bounds__(DISCARD_THREADS) void k_discard_fold(const int *partial, int w0, int tiles, int *res);

// k_masks.hip (computed masks, include/lqr_masks.h: T = float or double)
template <class T> __global__ __launch_bounds__(256) void k_mask_add_f(float *plane, int w0, const T *mask, int mw, int x0, int y0, int x1, int y1, int nx, int ny,
                                                                       int transposed, int is_rig, int bias_factor);
__global__ __launch_bounds__(256) void k_mask_scatter(float *plane, const int *index, const double *value, size_t n, int is_rig);
__global__ __launch_bounds__(256) void k_plane_transpose(const float *plane, float *out, int w0, int h0);

// k_energy_out.hip (energy read-outs, include/lqr_energy.h: PIC = the picture loop's arithmetic, TYPE = LqrImageType 0 .. 6, DEPTH = LqrColDepth)
template <bool PIC> __global__ __launch_bounds__(256) void k_energy_range(const DevCarver *cs, int w, int h, int stride, float *partials);
__global__ __launch_bounds__(256) void k_energy_plane(const DevCarver *cs, int w, int h, int stride, int transposed, int normalised,
                                                      const float *partials, int n_partials, float *out);
#define K_ENERGY_OUT_FORMS_T(X, T) X(T, 0) X(T, 1) X(T, 2) X(T, 3)
#define K_ENERGY_OUT_FORMS(X) K_ENERGY_OUT_FORMS_T(X, 0) K_ENERGY_OUT_FORMS_T(X, 1) K_ENERGY_OUT_FORMS_T(X, 2) K_ENERGY_OUT_FORMS_T(X, 3) K_ENERGY_OUT_FORMS_T(X, 4) K_ENERGY_OUT_FORMS_T(X, 5) K_ENERGY_OUT_FORMS_T(X, 6)
template <int TYPE, int DEPTH> __global__ __launch_bounds__(256) void k_energy_out(const DevCarver *cs, int w, int h, int stride, int transposed,
                                                                                    const float *partials, int n_partials, uint8_t *out);
