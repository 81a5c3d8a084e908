// lqr_geom.h -- the geometry of every launch: the size of each buffer, dynamic-LDS block and grid that the shim (lqr_shim.hip) makes and
// the offsets and block maps by which a kernel (k_*.hip) finds its way in it, stated once, as plain C++17.  No HIP, no globals, no
// allocation: constexpr functions of values, included by the kernel and by the shim alike and run without a GPU by
// tests/c/geom_main.cc, which writes the first and the last element a kernel can touch into a block of exactly the stated size.
// A kernel with a shared buffer or dynamic LDS adds its functions here and its extents to that test.
// Slack that a size carries beyond what the kernel indexes is named where it is added; it is part of the size.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "lqr_beside.h"         // bb_carve_entries / bb_energy_entries: row-quads and energy blocks of a frame; the work list of k_carve_v

// blocks of `own` elements that cover w: tiles of a row, workgroups of a grid with a thread per element
constexpr int tiles_of(int w, int own) { return (w + own - 1) / own; }
constexpr size_t blocks_of(size_t n, size_t per) { return (n + per - 1) / per; }

// ---- limits of dynamic LDS ------------------------------------------------------------------------------------------------------
// dynamic LDS beyond this needs hipFuncSetAttribute before the launch (k_dp_sweep past 8192 columns, k_vs_commit, k_fwd_seam)
constexpr size_t LDS_ATTR_BYTES = 64 * 1024;
constexpr bool lds_needs_attr(size_t bytes) { return bytes > LDS_ATTR_BYTES; }
// k_vmap_check_t asks earlier: its static LDS (the 32 x 33 transposition tile and a count per line, 4.3 KB) counts against the same
// 64 KB, and 8 KB are left for it
constexpr size_t VMAP_T_ATTR_BYTES = 56 * 1024;
constexpr bool vmap_t_needs_attr(size_t bytes) { return bytes > VMAP_T_ATTR_BYTES; }

// ---- the working planes (ensure_working): rows `stride` apart, one row and PLANE_SLACK elements beyond the frame ----------------
constexpr int PLANE_SLACK = 1024;
constexpr int plane_stride(int w) { return ((w + 16) + 63) & ~63; }
constexpr size_t plane_elems(int stride, int h) { return (size_t) stride * (h + 1) + PLANE_SLACK; }
// seam_x: a column per row, and SEAM_X_SLACK ints; the seam log: row k holds seam k's h columns
constexpr int SEAM_X_SLACK = 8;
constexpr size_t seam_x_elems(int h) { return (size_t) h + SEAM_X_SLACK; }
constexpr size_t seam_log_elems(int n_seams, int h) { return (size_t) n_seams * h; }

// ---- k_mask_add / k_mask_add_f (k_energy.hip, k_masks.hip): the grid is nx columns (256 a workgroup) by ny rows --------------------
// Where a width x height mask laid at (x_off, y_off) over the w0 x h0 image (transposed: over the carver's transposed frame) falls: (x0, y0) what
// of the offset is negative, (x1, y1) the first pixel it covers, nx x ny how many.  The far edge is computed in long long, so that a mask
// near INT_MAX wide cannot wrap; for arguments where plain int arithmetic does not overflow the values are those it gives.
struct MaskClip { int x0, y0, x1, y1, nx, ny; };
constexpr MaskClip mask_clip(int w0, int h0, int width, int height, int x_off, int y_off, int transposed)
{
    const int wt = transposed ? h0 : w0, ht = transposed ? w0 : h0;
    const int x0 = x_off < 0 ? x_off : 0, y0 = y_off < 0 ? y_off : 0;
    const int x1 = x_off > 0 ? x_off : 0, y1 = y_off > 0 ? y_off : 0;
    const long long xe = (long long) width + x_off, ye = (long long) height + y_off;
    const int x2 = wt < xe ? wt : (int) xe, y2 = ht < ye ? ht : (int) ye;
    return MaskClip{x0, y0, x1, y1, x2 - x1, y2 - y1};
}

// ---- k_dp_tile_p (k_tiles.hip): tiles, exchange area, epochs ---------------------------------------------------------------------
// PX pixels per lane (4, or 2 when the device has room for twice the tiles: half the instructions per wave and row):
// a tile is 64 * PX columns of which the 16 outer lanes on each side are halo
// `px` below is a geometry code: 2 / 4 = pixels per lane with 16 halo lanes per side; 3 (round 6) = 2 pixels per lane with 24 halo lanes per
// side -- 32 own columns + 48-column halos, blocks of 48 rows: the hand-over through memory (a third of a 32-row level) is paid 45
// times per 4K sweep instead of 68, for twice the tiles; used while every tile still has a compute unit to itself (single images)
constexpr int dppx_px(int px) { return px == 3 ? 2 : px; }
constexpr int dppx_hl(int px) { return px == 3 ? 24 : 16; }
constexpr int dpp_halo(int px) { return dppx_hl(px) * dppx_px(px); }              // halo columns on each side = rows per block
constexpr int dpp_own(int px) { return 64 * dppx_px(px) - 2 * dpp_halo(px); }     // columns a tile owns
constexpr int dpp_ex_tile(int px) { return px == 3 ? 2 * dpp_own(3) : 2 * 2 * dpp_halo(px); }       // granules a tile publishes: [block parity][side: 0 to the left, 1 to the right][column]; px 3: [block parity][own column]
constexpr int dpp_tiles(int w, int px) { return tiles_of(w, dpp_own(px)); }
// An image's part of the exchange area: its words -- per tile dpp_ex_tile granules, then DPP_CTR_WORDS of which the first counts
// finished tiles -- and at + near_off the same again, the near copies.  Image i starts at exch_image_off(i, near_off); n images take
// exch_words(near_off, n) words.  (k_band_levels lays its own words out by the same two functions.)
constexpr int DPP_CTR_WORDS = 8;
constexpr size_t dpp_ctr_off(int ntiles, int px) { return (size_t) ntiles * dpp_ex_tile(px); }
constexpr size_t dpp_near_off(int ntiles, int px) { return dpp_ctr_off(ntiles, px) + DPP_CTR_WORDS; }
constexpr size_t exch_image_off(size_t image, size_t near_off) { return image * 2 * near_off; }
constexpr size_t exch_words(size_t near_off, size_t n) { return 2 * near_off * n; }
// the layout an exchange area was last cleared for (exch_ensure compares it): k_dp_tile_p's is its px code
constexpr int exch_layout_dpp(int px) { return px; }
constexpr int EXCH_LAYOUT_LEVELS = 103;         // k_band_levels: that kernel's own layout and tags
// A granule's tag is 32 bits: the sign bit free, DPP_EPOCH_BITS of launch epoch, then the block index in the DPP_BLK_BITS that
// lqr_plan.h bounds a frame's height by (it asserts that the two add up to 31).  The epoch is never 0: a cleared area holds no tag
constexpr int DPP_EPOCH_BITS = 19;
constexpr int dpp_epoch(int launches) { return 1 + (launches % ((1 << DPP_EPOCH_BITS) - 2)); }

// ---- k_band_levels (k_levels.hip): exchange area, epochs, grid -------------------------------------------------------------------
constexpr int LV_PMAX = 16;             // slots per image at most
constexpr int LV_OWN = 64;              // columns a tile owns
constexpr int lv_tiles(int w) { return tiles_of(w, LV_OWN); }
// per image: the slots' words [2 parities][LV_PMAX slots][2 tiles], then the granules [2 parities][ntiles][LV_OWN]; near copies as above
constexpr int LV_FLAG_WORDS = 4 * LV_PMAX;
constexpr size_t lv_near_off(int ntiles) { return (size_t) LV_FLAG_WORDS + (size_t) 2 * ntiles * LV_OWN; }
// tags = epoch << LV_LEVEL_BITS | (level + 1), 32 bits: LV_EPOCH_BITS above the level's ten (lqr_plan.h: LV_MAX_LEVELS fits them)
constexpr int LV_LEVEL_BITS = 10, LV_EPOCH_BITS = 22;
constexpr int lv_epoch(int launches) { return 1 + (launches % ((1 << LV_EPOCH_BITS) - 2)); }
// The grid: one dimension, 8 * ceil(n / 8) * P workgroups.  Workgroup b is observed to run on XCD b mod 8, so the P slots of an image are
// the workgroups b = xcd + 8 (P g + slot), image = 8 g + xcd: all on one XCD.  Blocks whose image is >= n leave at once
struct LvBlock { int image, slot; };
constexpr unsigned lv_grid(size_t n, int P) { return (unsigned) (8 * ((n + 7) / 8) * P); }
constexpr LvBlock lv_block(int b, int P) { return LvBlock{((b >> 3) / P) * 8 + (b & 7), (b >> 3) % P}; }
// k_band_levels2 (k_levels2.hip): a workgroup is two slots of one image, s and s + ceil(P / 2) (the second is missing in the last workgroup
// of an odd P); an image's ceil(P / 2) workgroups share b mod 8 as above.  lv2_block gives the image and the FIRST slot
constexpr int lv2_pairs(int P) { return (P + 1) / 2; }
constexpr unsigned lv2_grid(size_t n, int P) { return (unsigned) (8 * ((n + 7) / 8) * lv2_pairs(P)); }
constexpr LvBlock lv2_block(int b, int P) { return LvBlock{((b >> 3) / lv2_pairs(P)) * 8 + (b & 7), (b >> 3) % lv2_pairs(P)}; }

// ---- k_carve_e / k_carve_u / k_carve_v (k_carve.hip), k_emap_update: grids ------------------------------------------------------
// k_carve_u: one dimension, the energy role's n * bb_energy_entries(h) workgroups first (image by image), then the carve role's
// n * bb_carve_entries(h) row-quads (image by image)
// (k_carve_u and k_band_levels keep their maps in their own text, over these counts: called through cu_block / lv_block their
// instruction streams come out scheduled differently.  The maps here are what the test checks and what the kernels' text must say)
struct CuBlock { bool energy; int image, index; };
constexpr int cu_energy_blocks(int n, int h) { return n * bb_energy_entries(h); }
constexpr unsigned cu_grid(unsigned n, int h) { return n * (unsigned) bb_energy_entries(h) + n * (unsigned) bb_carve_entries(h); }
constexpr CuBlock cu_block(unsigned b, int n, int h)
{
    const int eblk = bb_energy_entries(h), ne = n * eblk;
    if ((int) b < ne) {
        const int img = b / eblk, blk = b - img * eblk;
        return CuBlock{true, img, blk};
    }
    const int rblk = bb_carve_entries(h), cb = b - ne, img = cb / rblk, rb = cb - img * rblk;
    return CuBlock{false, img, rb};
}
// k_carve_v: the walks' n workgroups, then one consumer per entry of the work list; the list is two tail words and the entries
constexpr unsigned cv_grid(unsigned n, int h) { return n + (unsigned) bb_entries((int) n, h); }
constexpr size_t cv_list_words(int n, int h) { return (size_t) BB_LIST_HEAD + (size_t) bb_entries(n, h); }

// ---- the parallel backtrack (k_backtrack.hip, k_vp_maps / k_vp_solve) ------------------------------------------------------------
// vp_map: a displacement byte [chunk][x], rows `stride` apart.  vp_path: the displacement before every step, four steps to a dword,
// [chunk][step / 4][x], as bytes ((chunk * R4 + step / 4) * stride + x) * 4 + step % 4 with R4 = vp_quads(rows of a chunk).
// The sizes: one chunk more than there are, and VP_MAP_SLACK bytes (k_vp_solve's 16-byte loads of vp_map end inside `stride`, not
// inside w); vp_path is 4 * R4 times vp_map.  R4 depends on delta_x: a pair sized for one delta_x may be too small for another
constexpr int VP_MAP_SLACK = 64;
constexpr int vp_col_blocks(int w) { return (w + 255) / 256; }
constexpr int vp_quads(int rows) { return (rows + 3) / 4; }
constexpr size_t vp_map_bytes(int nchunks, int stride) { return (size_t) (nchunks + 1) * stride + VP_MAP_SLACK; }
constexpr size_t vp_path_bytes(int nchunks, int stride, int rows) { return vp_map_bytes(nchunks, stride) * 4 * vp_quads(rows); }
constexpr size_t vp_map_row(int chunk, int stride) { return (size_t) chunk * stride; }                  // bytes: + x, which the caller adds to the pointer -- k_vp_solve's column can be negative
constexpr size_t vp_path_chunk(int chunk, int R4, int stride) { return (size_t) chunk * R4 * stride; }          // dwords: + r4 * stride + x
constexpr size_t vp_path_quad(int r4, int stride) { return (size_t) r4 * stride; }
constexpr size_t vp_path_step(int chunk, int R4, int r, int stride, int x) { return (((size_t) chunk * R4 + (r >> 2)) * stride + x) * 4 + (r & 3); }     // bytes
// k_vp_solve's s_xs[nchunks + 1] (every chunk's first column, and row 0's), and one int of slack
constexpr size_t vp_solve_lds(int nchunks) { return (size_t) (nchunks + 2) * sizeof(int); }

// ---- dynamic LDS of the other kernels: bytes, and where each part starts ---------------------------------------------------------
// k_frozen_catchup: xs[to - from] ints, then rem[w_from] bytes, and FC_SLACK bytes
constexpr int FC_SLACK = 16;
constexpr int fc_w_from(int from, int to, int w_at_to) { return w_at_to + (to - from); }         // the frame before seam `from`
constexpr int fc_rem_off(int from, int to) { return to - from; }                                  // in ints
constexpr size_t fc_lds(int from, int to, int w_from) { return (size_t) (to - from) * sizeof(int) + (size_t) w_from + FC_SLACK; }
// k_vs_commit: xs[n_seams], then lvl[wc0], ints
constexpr int vsc_lvl_off(int n_seams) { return n_seams; }
constexpr size_t vsc_lds(int n_seams, int wc0) { return ((size_t) n_seams + wc0) * sizeof(int); }
// (the limit is unreachable while the host refuses frames wider than LQRHIP_MAX_FRAME_WIDTH, host/lqr_carver.c: a session carves at most
// wc0 - 1 seams, so n_seams + wc0 <= 2 * 16384 - 1 ints = 128 KB)
constexpr size_t VSC_LDS_MAX = 150 * 1024;
// k_inflate: a bit per level of the session, l - max_level + 1 of them, and one word of slack
constexpr size_t inflate_lds(int l, int max_level) { return (size_t) ((l - max_level + 1 + 31) / 32 + 1) * sizeof(unsigned); }
// k_vmap_check: a bit per level; k_vmap_check_t: VT_LINES lines of them, line c at c * words
constexpr int VT_LINES = 32;            // lines of the carver's frame (columns of the map) per workgroup of k_vmap_check_t
constexpr size_t vmap_words(int depth) { return (size_t) (depth + 31) / 32; }
constexpr size_t vmap_check_lds(int depth) { return vmap_words(depth) * sizeof(unsigned); }
constexpr size_t vmap_check_t_lds(int depth) { return VT_LINES * vmap_words(depth) * sizeof(unsigned); }
constexpr int vmap_t_blocks(int width) { return tiles_of(width, VT_LINES); }
// k_band_update_mw: s_touch[h]; k_band_update_tw: s_touch[h], then s_touchR[h]; ints.  The planner takes the fast band kernels only
// where these fit (BAND_MW_LDS_MAX leaves room for the kernel's static LDS)
constexpr size_t band_mw_lds(int h) { return (size_t) h * sizeof(int); }
constexpr size_t band_tw_lds(int h) { return (size_t) 2 * h * sizeof(int); }
constexpr int band_tw_touchR_off(int h) { return h; }
constexpr size_t BAND_MW_LDS_MAX = 60 * 1024, BAND_TW_LDS_MAX = 64 * 1024;
constexpr bool band_mw_fits(int h) { return band_mw_lds(h) <= BAND_MW_LDS_MAX; }
constexpr bool band_tw_fits(int h) { return band_tw_lds(h) <= BAND_TW_LDS_MAX; }
// k_dp_sweep: two rows of the frame padded to a multiple of 4 floats: prev, then cur
constexpr int sweep_wpad(int w) { return (w + 3) & ~3; }
constexpr size_t sweep_lds(int w) { return (size_t) 2 * sweep_wpad(w) * sizeof(float); }
// k_fwd_seam: M of two rows of L floats, row parity p at p * L
constexpr size_t fwd_lds(int L) { return (size_t) 2 * L * sizeof(float); }
constexpr int fwd_row_off(int parity, int L) { return parity * L; }         // (k_fwd_seam keeps its own text: its stream differs otherwise)

// ---- k_clipfwd.hip: forward-energy seams for a clip -----------------------------------------------------------------------------------
// The I planes of the n frames, H lines of L floats each, lie one after the other in one block: frame t starts at clip_frame_off(t, px),
// px = L * H.  The costs of a pixel lie side by side, CLIP_COST_FLOATS floats from clip_cost_off(y, x, L): CU, CL, CR, then Q (while the
// fold runs: T).  The sweep's two rows of M are k_fwd_seam's (fwd_lds, fwd_row_off).  The refresh folds CLIP_REFRESH_VALUES maxima (CU, CL,
// CR of two columns) of each of its waves through LDS: wave v's at clip_refresh_off(v)
constexpr int CLIP_COST_FLOATS = 4, CLIP_REFRESH_VALUES = 6;
constexpr size_t clip_intensity_elems(int n, size_t px) { return (size_t) n * px; }
constexpr size_t clip_frame_off(int t, size_t px) { return (size_t) t * px; }
constexpr size_t clip_cost_elems(size_t px) { return px * CLIP_COST_FLOATS; }
constexpr size_t clip_cost_off(int y, int x, int L) { return ((size_t) y * L + x) * CLIP_COST_FLOATS; }
constexpr int clip_fold_groups(int n, int group) { return tiles_of(n, group); }
constexpr int clip_refresh_off(int wave) { return wave * CLIP_REFRESH_VALUES; }
constexpr size_t clip_refresh_lds_elems(int threads) { return (size_t) (threads / 64) * CLIP_REFRESH_VALUES; }

// ---- k_discard.hip: the discard scan (include_ext/lqr_remove.h) ------------------------------------------------------------------------
// The result block: DISCARD_WORDS ints per scan -- marked pixels that are visible, the most of them in one line, the deepest level of a
// marked pixel, one word unused (a scan's result is 16 bytes) -- the line scan's at discard_result_off(0), the cross scan's at (1).
// The line scan: a workgroup per base-layout row, DISCARD_CHUNK columns at a time, four neighbouring columns per lane; the chunks of row y
// start discard_lead(y, w0) columns in front of the row, so that a lane's four lie on a 16-byte boundary of the planes.
// The cross scan: a workgroup takes DISCARD_ROWS base-layout rows of DISCARD_THREADS neighbouring columns, a column per lane, and leaves
// every column's count at discard_partial_off(tile, x, w0); k_discard_fold, a lane per column, sums the tiles' counts.  That holds while
// every pixel of the base layout is visible (level 1: a column of the layout is a column of the image).  Otherwise the ranked scan: a
// workgroup per row, DISCARD_THREADS columns at a time, adds a marked pixel to the count of the image column it is shown in -- its rank
// among the row's visible pixels -- in a block of discard_rank_elems(w) counts, w the visible width; the fold reads it as one tile.
constexpr int DISCARD_THREADS = 256, DISCARD_CHUNK = 4 * DISCARD_THREADS, DISCARD_ROWS = 32, DISCARD_WORDS = 4;
constexpr int discard_result_off(int cross) { return cross * DISCARD_WORDS; }
constexpr size_t discard_result_elems() { return 2 * DISCARD_WORDS; }
constexpr int discard_lead(size_t y, int w0) { return (int) ((y * (size_t) w0) & 3); }
constexpr int discard_col_blocks(int w0) { return tiles_of(w0, DISCARD_THREADS); }
constexpr int discard_row_tiles(int h0) { return tiles_of(h0, DISCARD_ROWS); }
constexpr size_t discard_partial_elems(int w0, int h0) { return (size_t) discard_row_tiles(h0) * w0; }
constexpr size_t discard_partial_off(int tile, int x, int w0) { return (size_t) tile * w0 + x; }
constexpr size_t discard_rank_elems(int w) { return (size_t) w; }
