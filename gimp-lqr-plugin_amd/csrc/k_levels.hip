// k_levels.hip -- E9 update_mmap for batches, one image's band on SEVERAL compute units, level by level (round 5)
// (gfx950 / CDNA4, wave64; see lqr_common.h for the file map and DESIGN.md section 4.16 for the measurements)
#include "lqr_common.h"
#include "lqr_kernels.h"
#include "lqr_levels.h"

// ---------------------------------------------------------------------------
// k_band_levels: the keep-rule sweep of k_band_tiles with the tiles assigned to workgroups PER 32-ROW LEVEL.
//
// k_band_tiles (round 4) parks 8 + 4 workgroups per image on fixed 64-column tiles for the whole launch; 62 % of the
// tile-blocks they sit on are inactive (they only forward a row), and at 64 images their 768 x 2 waves x 256 registers
// starve the sibling streams' carves.  Here an image has P "slots" (workgroups of two turn-taking waves, as there), and
// what a slot works on is decided level by level:
//   * level L = rows [32 L, 32 L + 32).  A_L = the ACTIVE tiles of the level = tiles whose own 64 columns can change in
//     it: a carve-touched pixel of the level's rows within 32 columns of them, or a pixel that changed on the last row of
//     level L - 1 inside them or inside the adjacent 32 columns of a neighbour tile (a change moves one column per row).
//     Nothing else can change (any superset of the pixels with changed inputs leaves liblqr's memory),
//     so inactive tiles are not computed, not stored, not resident -- they cost nothing.
//   * tile t is processed by slot t mod P: own 64 columns + 32-column halos recomputed from the stored inputs, 2 px per
//     lane, the 32 rows staged in registers (exactly k_band_tiles' row loop).  The tiles of a level do not depend on each
//     other, so when a slot has TWO active tiles in a level (a band wider than P tiles) its two waves take one each, side by
//     side (the second with a synchronous load: its prefetch was for the next level).  THREE on one slot: every slot sees
//     that in the same A_L and the image stops there -- flags[FLAG_OVF_ROW] = 32 L, k_dp_sweep<UPDATE> redoes the rows
//     below (a band wider than 2 P tiles; counted).
//   * a LEVEL BARRIER through memory replaces the pairwise hand-over AND the in-place rule: after its level a slot
//     publishes the last row of its tile's own columns as data-tagged granules ({m, tag}, one write-through store each)
//     and one word per tile {tag, tile, changed: own / left 32 / right 32}; the wave that takes the slot's next level polls all
//     2 P words (one load, lanes 0 .. 2 P - 1; the granules it expects to need ride along in the same poll) -- when they carry the level's tag every slot has finished the level: that is the
//     barrier, the words give A_{L+1}, and the granules of the neighbouring active tiles give the halo's row above.
//     Columns whose tile was not active in level L come from memory (nothing changed there).  Level L's results are
//     stored only after the partner wave has passed that barrier: every slot has then CONSUMED its inputs of level L, so
//     in place is safe (a slot's halo columns are its neighbours' own columns); inputs of later levels are rows nobody
//     writes before those levels' own barriers.  k_band_levels2 (LV_TRACK) writes of an interior tile only what changed: the
//     rows on which the keep rule changed an own pixel, from the lanes that changed any (the rest holds what was loaded from
//     the same addresses; store_rows 0 writes everything, lqrhip_set_levels_store).
//   * no reserve tiles, no requests, no edge watches, no inactive forwarding: the only spin is the level barrier.
//   * every word and granule is published TWICE: the write-through copy above (visible from every XCD: the protocol rests on it
//     alone) and a "near" copy at + near_off written with a plain store, which stays in the writer's L2.  An image's slots are
//     observed to sit on ONE XCD (the grid mapping below), whose L2 then hands the near copy over without the trip to memory
//     and back; the poll reads the near copy three times out of four and the write-through copy the fourth, so a placement
//     that puts the slots on different XCDs only polls slower.  A stale near line can never be taken for a fresh one: tags.
//     (+3 % at 8 and 16 images, +4 % at 48: DESIGN.md 4.16; lqrhip_band_levels_debug(4) turns the near copy off.)
// tags = epoch << 10 | (level + 1): nothing is cleared between launches.  Inputs are prefetched two levels ahead for the
// tile the slot is expected to have then (the same one, or the tile of its residue nearest to the seam); a wrong guess
// costs a synchronous load, never a result.
// Grid: 8 * ceil(images / 8) * P workgroups (see the mapping at the top of the kernel), all co-resident (bounded spins, DEVERR_TILE_TIMEOUT as in k_dp_tile_p).
// The kernel's body is k_levels_body.inc: k_band_levels2 (k_levels2.hip, two slots of an image per workgroup) includes the same text.
// ---------------------------------------------------------------------------
// [0] images stopped by three active tiles on one slot, [1] synchronous (mispredicted or second-tile) loads, [2] tile-levels
// processed, [3] slot-levels idle, [4] levels in which a slot had two tiles, [5] rows of processed tile-levels written back, [6] rows
// not written because no own pixel changed on them
__device__ unsigned long long g_lv_stats[8];
#ifdef LQR_TIMING
// per slot of image 0 and wave: cycles in [0] barrier poll (wait_level), [1] active set + tile choice, [2] waiting for the partner's poll,
// [3] stores, [4] loads (issue; synchronous ones include the wait), [5] row above, [6] the 32 rows, [7] publish, [8] LDS barrier, [9] whole kernel
__device__ unsigned long long g_lv_time[16][2][10];
extern "C" int lqrhip_band_levels_timing(unsigned long long *out) { (void) hipDeviceSynchronize(); return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_lv_time), sizeof(unsigned long long) * 320) == hipSuccess ? 0 : -1; }
#endif
__device__ int g_lv_dbg;               // experiment switches (lqrhip_band_levels_debug): 1 no speculative granule fetch, 2 sleep longer in the poll, 4 no near copy, 8 an image's slots on different XCDs


// DELTA = delta_x (1 .. 4): a change moves DELTA columns per row, so a level is HALO / DELTA rows (32, 16, 8, 8); RIGM = a rigidity
// mask scales the rigidity term per pixel (one more 4-byte plane read).  The plain instantiations (1, false) use the 3-neighbour
// row dp_row, the others dp_row_g, exactly as k_dp_tile_p's general instantiations do.
template <bool LR, bool RIG, int DELTA, bool RIGM>
__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(2, 2)))
void k_band_levels(DevCarver *cs, DpK p, int w, int h, int stride, unsigned long long *exch, int epoch, int *dev_err, int P, int n_img, int store_rows)
{
// (what the body leaves to the family, k_levels_body.inc: here a workgroup is one slot)
#define LV_NT 128
#define LV_SLOT_STATE __shared__ int s_polled; __shared__ unsigned long long s_A[2];
#define LV_POLLED s_polled
#define LV_A s_A
#define LV_WAVE const int q = __builtin_amdgcn_readfirstlane(tid >> 6);
#define LV_BLOCK const int b_xcd = (int) blockIdx.x & 7, b_k = (int) blockIdx.x >> 3; const int slot = (dbg & 8) ? (int) blockIdx.x % P : b_k % P, image = (dbg & 8) ? (int) blockIdx.x / P : (b_k / P) * 8 + b_xcd;
#define LV_INIT_FLAGS if (tid == 0) { s_fail = 0; s_polled = -1; }
#define LV_AFTER_SETUP
#define LV_LEVEL_END asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
// (no change tracking in this family: three more instructions per row are what the groups it serves -- 8 and 16 images, where the row wave
// is the critical path -- lose by, 74.8 -> 76.8 and 84.6 -> 86.7 ms per step; store_rows is ignored, every row is written, counter 6 stays 0)
#define LV_TRACK 0
#define LV_DBG g_lv_dbg
#define LV_STATS g_lv_stats
#define LV_TIME g_lv_time
#include "k_levels_body.inc"
#include "k_levels_undef.inc"
}

// (the switches and the counters are both families': k_levels2.hip keeps its own device globals)
extern "C" void lqrhip_band_levels_debug(int v) { if (lqrhip_init() < 0) return; (void) hipMemcpyToSymbol(HIP_SYMBOL(g_lv_dbg), &v, sizeof v); lqr_levels2_debug(v); }
// Entries 5 and 6 (rows written back, rows skipped) are reported only while lqrhip_set_levels_store is pinned: left to itself the hook
// differs between the families, and their event counters are compared as a whole (tests/test_levels_pair_gpu.py)
static int g_lv_report_rows = 0;
void lqr_levels_report_rows(int on) { g_lv_report_rows = on; }
extern "C" int lqrhip_band_levels_stats(unsigned long long *out, int reset)
{
    if (lqrhip_init() < 0) return -1;          // the symbol of the device the library selected (LOCAL_RANK), not device 0's
    (void) hipDeviceSynchronize();
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_lv_stats), sizeof(unsigned long long) * 8) != hipSuccess) return -1;
    if (reset) { unsigned long long z[8] = {0}; (void) hipMemcpyToSymbol(HIP_SYMBOL(g_lv_stats), z, sizeof z); }
    const int rc = lqr_levels2_stats(out, reset);
    if (!g_lv_report_rows) out[5] = out[6] = 0;
    return rc;
}

// ---- the instantiations the shim launches (lqr_kernels.h lists them)
#define INST(...) template __global__ void k_band_levels<__VA_ARGS__>(DevCarver *, DpK, int, int, int, unsigned long long *, int, int *, int, int, int);
K_BAND_LEVELS_FORMS(INST)
#undef INST
