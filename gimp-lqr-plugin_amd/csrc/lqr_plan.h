// lqr_plan.h -- which form of each stage a full DP and a seam step run: the launch shim's whole policy, as plain C++17.  No HIP, no
// globals, no I/O, no allocation: values in, a plan out, so that the same code runs in tests/c/plan_main.cc without a GPU.  The shim
// (lqr_shim.hip) fills the three input structs, asks once per launch sequence and launches what the plan says; nothing outside this
// file compares a width, a height or a group size with a threshold.  A form is named by the census slot it is counted under
// (LQRHIP_CENSUS_* in include/lqr_hip.h).  tests/geometry_cases.py restates the same choices independently, in Python.
#pragma once
#include <algorithm>
#include <stddef.h>
#include "../../include/lqr_hip.h"
#include "lqr_beside.h"         // the backtrack beside the carve: its side bound, its entries and their limits
#include "lqr_geom.h"           // each launch's sizes and grid maps, and the tiles' geometry (dpp_halo, dpp_own, LV_PMAX, tiles_of)

#define DP_THREADS 1024
// ---- geometry of the persistent tiled kernels (k_tiles.hip) that the choices depend on; the tiles themselves are lqr_geom.h's
constexpr int dpp_rb(int px, int delta) { return delta >= 5 ? dpp_halo(2) / delta : delta >= 3 ? 8 : dpp_halo(px) / delta; }      // rows per block (delta_x 5 .. 10: 6, 5, 4, 4, 3, 3)
constexpr int DPP_R = 16;                       // rows per batch
constexpr int DPP_W = 2;                        // waves taking turns
static_assert(dpp_halo(2) % (2 * DPP_R) == 0 && dpp_halo(4) % (2 * DPP_R) == 0, "a block (halo / delta_x rows, delta_x <= 2) is a whole number of batches");
constexpr int DPP_BLK_BITS = 12;                // bits of the block index in a granule's tag
static_assert(DPP_EPOCH_BITS + DPP_BLK_BITS == 31, "a granule's tag: epoch above block index, the sign bit free");
#define DPT_ROWS 32
#define DPT_OWN 192
// k_band_levels (k_levels.hip): tiles per image at most (one 64-bit mask: rows up to 4096 px)
constexpr int LV_MAX_TILES = 64;
constexpr int LV_MAX_LEVELS = 1020;       // levels per image at most (10 bits of the tags hold level + 1; 4K rows at delta_x 10: 720 levels of 3 rows)
static_assert(LV_MAX_LEVELS + 1 < (1 << LV_LEVEL_BITS), "level + 1 fits its field of the tags");
constexpr int lv_rows(int delta, bool rigm = false) { return delta == 1 ? (rigm ? 16 : 32) : delta == 2 ? 16 : delta <= 4 ? 8 : 32 / delta; }      // rows per level: halo (32 columns) / delta_x (a rigidity mask: 16, for the registers)
constexpr int LQR_FAST_MAX_DELTA = 10;    // delta_x up to which the tiled kernels have instantiations (the plug-in's UI: src/interface.c:47, MAX_DELTA_X 10)
// parallel backtrack (k_backtrack.hip, k_vp_*): a chunk is VP_REACH / delta_x rows, so that a path moves at most VP_REACH columns
// inside a chunk (the displacement fits a byte); k_vp_solve walks VP_STAGE chunks per LDS-resident stage
constexpr int VP_REACH = 56;
constexpr int VP_STAGE = 20;        // (4K: 39 chunks = 2 stages; the cone of a stage is 2 * 56 * 20 columns wide: 45 KB of LDS)
constexpr int vp_chunk_rows(int delta) { return VP_REACH / delta; }
// brightness samples a row of k_emap_update takes (EU_NT): the window a seam of this delta_x can have moved
constexpr int eu_samples(int delta_x) { return delta_x <= 2 ? 12 : delta_x <= 8 ? 36 : 68; }
// The frozen planes' lag: seams they may be behind before they are compacted.  The energy update walks the seam log back to the frozen
// frame (O(lag) per sample); compacting the frozen planes costs a pass over them.  Few images: the walk is on the critical path and
// the pass is cheap -> short lag
#ifndef FROZEN_LAG_MAX
#define FROZEN_LAG_MAX 128
#endif
constexpr int frozen_lag(int images) { return images <= 4 ? FROZEN_LAG_MAX / 4 : FROZEN_LAG_MAX; }
constexpr int LV_AUTO_MIN = 7;            // slots per image the automatic choice of k_band_levels needs (6 and fewer put second tiles on a slot in 9 % of the tile-levels)

// ---- what the choice is made from -----------------------------------------------------------------------------------------------
// The knobs behind the lqrhip_set_* hooks (include/lqr_hip.h says what each value means), with their defaults
struct PlanKnobs {
    int vpath_mode = -1;            // -1: the parallel backtrack for groups up to vpath_par_max images of at least vpath_min_rows rows; 0: never; 1: always (delta_x 1 .. 10)
    int vpath_par_max = 3, vpath_min_rows = 1000;     // (3 x 4K: 58 -> 46 us per seam; 4: equal; 8: slower -- the maps of n images are n times the work)
    int sweep_threads = 256;        // threads of the k_dp_sweep<UPDATE> launch behind the band kernels (256, or 1024 as in rounds 1 - 5)
    int carve_fused = 4;            // k_carve_e (carve + energy update in one launch) for groups up to this many images (0: the two kernels always)
    int carve_beside = -1;          // k_carve_u (the energy update beside the carve, one launch): -1 automatic (plan_carve_beside); 0 never; 1 wherever a form exists
    int backtrack_beside = -1;      // k_carve_v (the backtrack as a role of the carve's launch too): -1 automatic (plan_backtrack_beside); 0 never; 1 wherever a form exists
    int update_mode = -1;           // lqrhip_set_update_mode
    int band_levels = -1;           // k_band_levels: -1 automatic; 0 never; n: n slots per image
    int levels_wg_slots = -1;       // slots per workgroup of the level kernel: -1 automatic (plan_levels_wg_slots); 1: one (k_band_levels); 2: two (k_band_levels2) wherever a form exists
    int carve_line = -1;            // where a row's groups of the carve start / end: -1 automatic (plan_carve_line: by the carve's form); 0: on a 16-byte vector; 1: on a 128-byte line of the float planes (32 elements)
    int levels_store = -1;          // what the level kernel writes back: -1 automatic (plan_levels_store); 0: every row of a level from every lane; 1: only the changed rows, from the own lanes that changed
    int dpp_limit = -1;             // -1: the occupancy-derived bounds; >= 0: at most that many workgroups for a spinning grid
    int dpp_px = 0;                 // 2, 3 or 4 pins the persistent sweep's geometry code (0 = by batch size)
    int sub_batches = 0;            // streams of a group; 0: automatic (plan_streams)
    // batches up to this many pixels use the tiled full-width update (measured break-even with the band kernel at 4K, Mseams*px/s
    // tiled / band: 7 images 118 k / 97 k, 8: 130 / 109, 9: 119 / 121, 12: 130 / 139+, 16: 158 / 175+)
    long long tiled_update_px = 8LL * 3840 * 2160;
};
// What the device said (dpp_resident_workgroups in lqr_shim.hip): workgroups of each residency class it holds at once, compute units,
// and the HIP runtime's GPU_MAX_HW_QUEUES (0: not set)
struct PlanDevice {
    int wgs_plain = 0, wgs_general = 0, wgs_px4 = 0, wgs_levels = 0;
    int wgs_levels2 = 0;            // k_band_levels2's 256-thread workgroups
    int n_cu = 0, hw_queues = 0;
};
// What a batch is
struct PlanBatch {
    int images = 1;                 // carvers of this batch (one stream)
    bool shared = false;            // sibling batches of the same group run on their own streams ...
    int shared_n = 1;               // ... this many in all
    bool spin = true;               // spinning kernels allowed (no session redone after a fault, no spin time-out in this process)
    int wk_h = 0;                   // rows of the working planes
    bool value = false;             // the working plane is the value plane (lqr_pixel.h), not packed 8-bit pixels
    bool rigmask = false;           // a carver of the batch has a rigidity mask
    size_t group() const { return (size_t) images * (size_t) std::max(shared_n, 1); }       // images of the whole lock-step group
    bool rigm(bool use_rig) const { return use_rig && rigmask; }        // a rigidity mask that matters (without rigidity the mask multiplies nothing)
};

// ---- the plans ------------------------------------------------------------------------------------------------------------------
// One DP launch sequence.  form: LQRHIP_CENSUS_TILE_P_* (k_dp_tile_p: px is the geometry code, `per` images per launch -- a general batch
// too large for one grid is swept group after group), _DP_TILE (k_dp_tile, one launch per DPT_ROWS rows), _SWEEP_FULL / _SWEEP_UPDATE
// (k_dp_sweep<px, ., threads> with `lds` bytes; px 0: the row is wider than any form covers); -1: nothing to launch
struct DpPlan {
    int form = -1, px = 0, per = 0, threads = 0;
    bool general = false;           // k_dp_tile_p's delta_x 2 .. 10 / rigidity-mask instantiations
    size_t lds = 0;
};
// One seam step on a frame w wide on entry
struct StepPlan {
    int backtrack = 0;              // LQRHIP_CENSUS_VP_PARALLEL (vp_rows per chunk, vp_chunks chunks), _VPATH1 or _VPATH
    int vp_rows = 0, vp_chunks = 0;
    int carve = 0;                  // LQRHIP_CENSUS_CARVE_E (the energy update fused in) or _CARVE
    bool energy_beside = false;     // _CARVE only: k_carve_u, the energy update as workgroups of the carve's launch (counted under _CARVE)
    bool backtrack_beside = false;  // energy_beside only: k_carve_v, the one-wave walk as a role of that launch too (no backtrack launch; counted under _VPATH1 and _CARVE)
    int carve_line = 0;             // the carve's `line` argument, whichever form runs (plan_carve_line)
    bool catchup = false;           // the frozen planes lag too far: compact them before the energy update
    int eu_nt = 0;                  // k_emap_update's samples per row
    bool full = false;              // dp is a full DP (after a side switch), not an update
    int band = -1;                  // LQRHIP_CENSUS_BAND_* in front of dp (a _SWEEP_UPDATE then); -1: dp alone (the tiled update, a full DP)
    int levels_P = 0;               // k_band_levels: slots per image
    int levels_wg_slots = 1;        // ... and per workgroup: 2 is k_band_levels2 (counted under _BAND_LEVELS too)
    int levels_store = 0;           // ... and what it writes back: 0 every row from every lane, 1 the changed rows from the lanes that changed (plan_levels_store)
    DpPlan dp;                      // form -1: nothing is left to update (liblqr's finish_vsmap case)
};

static inline int plan_limit(const PlanKnobs &k, int bound) { return k.dpp_limit >= 0 ? std::min(k.dpp_limit, bound) : bound; }     // a residency bound under the cap

// Streams a lock-step group of n carvers is split over.  Automatic: 4 for the groups that run k_band_update_tw (49 images and more), 2
// for the groups of 32 to 48 that run k_band_levels (round 5, one box, Mseams*px/s with 2 / 4 streams: 32 images 360 / 352 k, 48
// images 432 / 404 k) WHEN the process has the hardware queues for them -- GPU_MAX_HW_QUEUES (default 4, read when HIP initialises,
// shared with every other stream of the process) must be 8 or more; with fewer, streams share queues and the split is 30 % slower
// than one stream, so it is not made.
static inline int plan_streams(const PlanKnobs &k, const PlanDevice &d, int n)
{
    const int nb = k.sub_batches ? k.sub_batches : d.hw_queues >= 8 ? (n >= 49 ? 4 : n >= 32 ? 2 : 1) : 1;
    return n >= 2 * nb ? nb : 1;
}

// Can the persistent tiled sweep (k_dp_tile_p) take `images` images of this batch at once, and in which geometry (0: not at all)?
// Its tiles spin on each other, so the whole grid has to be resident.  2 px per lane while twice the tiles still fit the residency
// bound (the row chain is then ~33 instructions per wave instead of ~58, NOTES/rounds-1-5.md 4.5; measured per 4K seam round, 2 vs 4 px
// per lane: 1 image 0.40 / 0.50 ms, 4: 0.45 / 0.55, 8: 0.58 / 0.62, 12: 0.76 / 0.77), else 4.
// `general`: delta_x != 1 and / or a rigidity mask (with rigidity): those instantiations exist for 2 px per lane only
static inline int plan_persistent_px(const PlanKnobs &k, const PlanDevice &d, const PlanBatch &b, int w, bool general, int delta, int images)
{
    if (b.shared || !b.spin) return 0;
    const size_t n = (size_t) images;
    const int limit = plan_limit(k, general ? d.wgs_general : d.wgs_plain);
    const int maxblk = (1 << DPP_BLK_BITS) - 1;         // the block index is DPP_BLK_BITS bits of the granule tag
    // px code 3 (round 6): 32-column tiles with 48-column halos, 48-row blocks -- a third fewer hand-overs through memory for twice the
    // tiles; while every tile still gets a compute unit of its own (a single 4K image: 120 tiles; measured: DESIGN.md 4.2)
    if (!general && delta == 1 && (k.dpp_px == 3 || k.dpp_px == 0) && b.wk_h <= maxblk * dpp_rb(3, 1) &&
        tiles_of(w, dpp_own(3)) * n <= (size_t) std::min(limit, k.dpp_px == 3 ? limit : d.n_cu)) return 3;
    if ((general || (k.dpp_px != 4 && k.dpp_px != 3)) && b.wk_h <= maxblk * dpp_rb(2, delta) && tiles_of(w, dpp_own(2)) * n <= (size_t) limit) return 2;
    // the plain 4-px instantiations hold fewer registers than the 2-px ones: a bound of their own
    if (!general && k.dpp_px != 2 && k.dpp_px != 3 && b.wk_h <= maxblk * dpp_halo(4) && tiles_of(w, dpp_own(4)) * n <= (size_t) plan_limit(k, d.wgs_px4)) return 4;
    return 0;
}
static inline DpPlan plan_persistent(int px, bool general, int per)
{
    DpPlan p;
    p.form = general ? LQRHIP_CENSUS_TILE_P_GENERAL : px == 3 ? LQRHIP_CENSUS_TILE_P_G3 : px == 2 ? LQRHIP_CENSUS_TILE_P_G2 : LQRHIP_CENSUS_TILE_P_G4;
    p.px = px; p.general = general; p.per = per;
    return p;
}

// k_dp_sweep, one workgroup per image.  The launch behind a band kernel (update) almost always only looks at flags[FLAG_OVF_ROW]: 256
// threads for rows up to 4096 px (a workgroup that finds room at once beside the sibling streams' kernels), 1024 for the full sweeps
// and wider rows.  px per thread: the first of 1, 2, 4, 8, 16 that covers the row
static inline DpPlan plan_sweep(const PlanKnobs &k, int w, bool update)
{
    DpPlan p;
    p.form = update ? LQRHIP_CENSUS_SWEEP_UPDATE : LQRHIP_CENSUS_SWEEP_FULL;
    p.threads = (update && k.sweep_threads == 256 && w <= 16 * 256) ? 256 : DP_THREADS;
    for (p.px = 1; p.px <= 16 && p.px * p.threads < w;) p.px *= 2;
    if (p.px > 16) p.px = 0;
    p.lds = sweep_lds(w);
    return p;
}

// A full DP (E5) of a frame w wide
static inline DpPlan plan_full_dp(const PlanKnobs &k, const PlanDevice &d, const PlanBatch &b, int w, int delta, bool use_rig)
{
    const bool general = delta != 1 || b.rigm(use_rig);
    if (delta >= 1 && delta <= LQR_FAST_MAX_DELTA) {
        // round 5: a general batch too large for one persistent grid (it runs its incremental updates on k_band_levels): the full DP
        // group after group of as many images as fit -- `per` is halved until a grid fits -- instead of one 1024-thread workgroup per
        // image (k_dp_sweep: 4 - 8 ms per sweep of 16 x 4K against 2 x 0.5)
        int per = b.images, px;
        while (!(px = plan_persistent_px(k, d, b, w, general, delta, per)) && general && per > 1) per = (per + 1) / 2;
        if (px) return plan_persistent(px, general, per);
        if (!general) { DpPlan p; p.form = LQRHIP_CENSUS_DP_TILE; return p; }
    }
    return plan_sweep(k, w, false);
}

// The automatic choice may put a group of `group` images on k_band_levels (before its geometry and the residency bound are asked).
// Round 5: the default for groups of 8 to 64 images (measured, Mseams*px/s at 4K, levels / k_band_update_tw: 8 images 148 / 127, 16:
// 256 / 180, 48: 479 / 404).  64 images on four streams with 7 slots: alternating 3-step runs on three boxes 516 / 495-516, 497 / 488,
// 520 / 504; the driver's 20-step command on two boxes of equal speed (every other figure within 1 %) 567.2 / 538.9 k.  Its 448
// workgroups stretch the sibling streams' carves (k_carve 172 -> 203 us per launch) while the whole step's share of the HBM roof rises
// (0.279 -> 0.293).  96 images run 585 / 622: plain groups above 64 keep k_band_update_tw.  Also delta_x 2 .. 4 and rigidity masks
// (k_band_levels' general instantiations): a batch of such carvers used to be carved in groups of as many as the full-width tiled
// kernels hold (16 x 4K, delta_x 2: 68 k Mseams*px/s).  delta_x 5 .. 10 on request only (update mode 5): a change moves up to ten columns
// per row, the band is the whole width after a few hundred rows and the level kernel's images stop at a collision: 16 x 4K at
// delta_x 8 spent 6.6 of 9.6 ms per seam in the sweep that takes over
static inline bool levels_auto(const PlanKnobs &k, int delta, size_t group, bool plain)
{
    return k.update_mode < 0 && delta <= 4 && group >= 8 && (group <= 64 || !plain);
}
// Slots (workgroups) per image for k_band_levels on a frame w x h (0: not usable here): as many as the group's images leave room for
// within the residency bound, at most LV_PMAX; lqrhip_set_band_levels pins it.  Automatic, never fewer than LV_AUTO_MIN and never
// more than 12:
//   * a batch whose group is spread over sibling streams (b.shared): while the group's workgroups stay below ~384 (beyond that the
//     sibling kernels are starved of registers, NOTES/rounds-1-5.md 4.15 / 4.16: 48 images with 10 slots 452 k, with 8 slots 479 k);
//   * a batch that has its stream to itself -- what a process with fewer than 8 hardware queues runs, plan_streams -- has no
//     sibling: the carve runs after the levels, not beside them.  Its bound is two workgroups per compute unit (2 * n_cu, 512 on an
//     MI355X).  That figure is read off the measurements below; the explanation that goes with it -- a workgroup is two waves, so
//     up to there every wave can have a SIMD to itself -- is a supposition about where the dispatcher puts them, not something
//     observed.  Measured on one stream (profiles/onestream/README.md; ms per step of 64 / 48 x 4K, 200 seams, two rounds,
//     slots per image 7 / 8 / 9 / 10 / 12):
//         64 images (448 .. 768 workgroups)  214.9 214.6 / 210.9 211.0 / 216.2 216.2 / 217.1 216.8 / 217.8 217.9
//         48 images (336 .. 576 workgroups)  179.4 179.6 / 175.5 175.7 / 173.0 173.2 / 173.2 173.2 / 182.2 181.9
//     512 and 480 workgroups are the best or equal to it, 576 loses 3 % both times.  So 64 images get 8 slots (they had 7: -3.7 ms,
//     1.7 %) and 48 get 10 (they had 8: -2.4 ms, 1.4 %).  Only 48 and 64 images were run: every other group size of 33 .. 63 gets
//     its slots by extrapolation over the workgroup count (33 .. 42 images: 12 slots, they had 11 .. 9; 43 .. 46: 11; 47 .. 51: 10;
//     52 .. 56: 9; 57 .. 63: 8).  Groups up to 32 get 12 slots under either bound, as before
static inline int plan_levels_P(const PlanKnobs &k, const PlanDevice &d, const PlanBatch &b, int w, int h, int delta)
{
    if (!b.spin || k.band_levels == 0 || delta < 1 || delta > LQR_FAST_MAX_DELTA || tiles_of(h, lv_rows(delta, true)) > LV_MAX_LEVELS || tiles_of(w, 64) > LV_MAX_TILES) return 0;
    const int per_batch = plan_limit(k, d.wgs_levels) / std::max(b.shared_n, 1);
    const int want = k.band_levels > 0 ? k.band_levels : std::max(LV_AUTO_MIN, std::min(12, (int) ((b.shared ? 384 : 2 * d.n_cu) / std::max<size_t>(b.group(), 1))));
    const int P = std::min({LV_PMAX, per_batch / std::max(b.images, 1), want});
    return P >= (k.band_levels > 0 ? 1 : LV_AUTO_MIN) ? P : 0;
}
// Slots per workgroup of the level kernel, given its P slots per image: 2 is k_band_levels2 (k_levels2.hip), whose workgroup holds the
// slots s and s + ceil(P / 2) of one image on four waves.  A form exists at delta_x 1 without a rigidity mask that matters, for P >= 2,
// where spinning kernels are allowed (plan_levels_P gives no P otherwise) and the grid fits the family's own residency bound; the
// knob at 2 takes it wherever it exists.  Automatic: a batch that has its stream to itself whose one-slot grid would put two workgroups
// on some compute unit (group x P > n_cu); the two-slot grid is then at most one workgroup per unit.
// Measured on one stream (profiles/levels_pair/README.md; 4K, 200 seams, parent / new): the level kernel 381.3 -> 368.7 us per launch at
// 64 images; three alternating runs of 20 steps: 179.55 179.05 179.31 -> 177.39 177.04 177.22 ms per step (+1.2 %, the parent's spread
// 0.5 ms).  Mseams*px/s in the order parent, new, new, parent: 8 images 178.0 k 178.7 k 178.4 k 179.0 k and 16: 322.0 321.7 320.5 321.2
// (96 and 192 one-slot workgroups: the rule leaves them on k_band_levels, nothing moves), 32: 429.2 454.2 456.1 427.2 (384 -> 192
// workgroups, +6.3 %), 48: 512.1 535.2 543.1 522.7 (480 -> 240, +2.4 .. 6.1 %).  Every size that takes the form gains, so the threshold
// stays the reasoned one; 22 .. 31 images (12 slots: 264 .. 372 one-slot workgroups) were not run.  Sub-batches on sibling streams keep
// the one-slot kernel: round 6 measured two slots per workgroup at -18 % under the sibling streams' carves.
static inline int plan_levels_wg_slots(const PlanKnobs &k, const PlanDevice &d, const PlanBatch &b, int delta, bool general, int P)
{
    if (k.levels_wg_slots == 1 || !b.spin || delta != 1 || general || P < 2) return 1;
    if ((size_t) lv2_grid((size_t) b.images, P) > (size_t) (plan_limit(k, d.wgs_levels2) / std::max(b.shared_n, 1))) return 1;
    if (k.levels_wg_slots == 2) return 2;
    return !b.shared && b.group() * (size_t) P > (size_t) d.n_cu ? 2 : 1;
}
// What the level kernel writes back (its store_rows argument): 1 = of an interior tile only the rows on which the keep rule changed an
// own pixel, from the own lanes that changed a pixel on any row of the level -- the rest holds what the level's loads read from the
// same addresses, and the halo lanes do not write to the spare row -- 0 = every row of every processed tile-level from every lane, as
// before.  Only k_band_levels2 has the form: keeping the change bits costs three instructions per row, which the groups the one-slot
// family serves lose by (the row wave is their critical path).  The knob at 0 pins 0; otherwise 1 wherever the two-slot family runs.
// Measured (profiles/levels_store/README.md; ms per step, parent / new): 64 images 189.2 187.6 189.5 / 182.0 185.1 185.5; Mseams*px/s
// in the order parent, new, new, parent: 32 images 449.0 k 464.2 k 466.7 k 451.1 k, 48: 533.3 533.6 529.8 516.6; with the bits kept in
// the one-slot family too 8 images 177.3 k 172.9 k 172.5 k 177.4 k and 16: 313.8 306.5 306.0 313.8, without them 181.0 180.6 and 318.3 318.0.
static inline int plan_levels_store(const PlanKnobs &k, int wg_slots)
{
    return k.levels_store != 0 && wg_slots == 2 ? 1 : 0;
}
// How many images of frame width `w` (the direction being carved) one lock-step batch may hold and still run delta_x != 1 /
// rigidity-mask carvers on the tiled kernels (k_dp_tile_p's general instantiations: one workgroup per 64 columns per image, all
// co-resident).  Beyond it such a batch would fall to the one-wave-per-image band kernel (~30x slower), so the host carves larger
// batches of such carvers group after group (host/lqr_carver.c, lqrx_carver_resize_batch).  Groups the automatic choice puts on
// k_band_levels may be as large as leaves every image LV_AUTO_MIN slots: far larger than the full-width tiled kernels take; their
// full DPs (3 per resize) then run group after group (plan_full_dp)
static inline int plan_general_batch_limit(const PlanKnobs &k, const PlanDevice &d, int w, int delta)
{
    const int tiled = plan_limit(k, d.wgs_general) / tiles_of(w, dpp_own(2));
    const int lv = plan_limit(k, d.wgs_levels) / LV_AUTO_MIN;
    return levels_auto(k, delta, (size_t) std::max(lv, 0), false) && k.band_levels != 0 && tiles_of(w, 64) <= LV_MAX_TILES ? std::max(tiled, lv) : tiled;
}

// The energy update beside the carve, as workgroups of one launch (k_carve_u, k_carve.hip), for the groups too large for k_carve_e.
// A form exists for delta_x <= 2 (12 brightness samples per row) on packed pixels while a frame is left to update (wnew > 1); the
// knob at 1 takes it wherever it exists.  Automatic: batches that have their stream to themselves (what a process with fewer than 8
// hardware queues runs, plan_streams) of at least CARVE_BESIDE_MIN images.  There the energy update ran alone behind the carve, the
// chip almost empty; beside the carve its launch and its dispatch leave the step.
// Measured on one stream (profiles/carve_beside/README.md; 4K, 200 seams, parent / new): per launch k_carve 477.7 + k_emap_update 28.4 us
// -> k_carve_u 490.7 us (the carve role is 13 us longer with the energy role beside it); 64 images, three alternating runs of 20
// steps: 196.13 196.28 196.61 -> 194.56 194.34 194.65 ms per step (+0.9 %, the parent's spread 0.25 %).  Mseams*px/s in the order
// parent, new, new, parent: 8 images 170.6 k 176.4 k 177.6 k 171.9 k, 16: 292.1 303.3 300.8 294.0, 32: 399.9 403.6 407.6 396.6,
// 48: 485.6 490.4 489.9 482.7 -- every size run gains, so the threshold is the smallest size run, 8; 5 .. 7 were not run and keep
// the two launches.  Sub-batches on sibling streams (b.shared): 64 images on four streams with 16 hardware queues, parent / rule
// extended to them, two rounds: 592.3 k / 587.6 k, 583.4 k / 585.6 k -- inside the parent's own spread (the energy update never runs
// alone there: the sibling streams' kernels fill the chip around it); left out.
constexpr int CARVE_BESIDE_MIN = 8;
static inline bool plan_carve_beside(const PlanKnobs &k, const PlanBatch &b, int delta, int wnew)
{
    if (k.carve_beside == 0 || delta > 2 || b.value || wnew <= 1) return false;
    return k.carve_beside > 0 || (!b.shared && b.group() >= (size_t) CARVE_BESIDE_MIN);
}

// The backtrack beside the carve as well (k_carve_v, k_carve.hip): the one-wave walk hands rows to the carve and energy roles of the
// same launch through a work list, so the 59 us per 4K seam in which 64 chasing waves had the chip to themselves leave the step.
// A form exists where the energy update runs beside the carve (plan_carve_beside), the backtrack is the one-wave walk at delta_x
// <= 2, the frame has at least three walk chunks of rows and at most what the walk's path buffer and the entry's fields hold, and
// spinning kernels are allowed (the consumers wait for their entries).  Not on the step that compacts the frozen planes: that pass
// reads this seam's log row between the backtrack and the carve.  The knob at 1 takes the form wherever it exists.  Automatic:
// batches that have their stream to themselves, of at least BACKTRACK_BESIDE_MIN images.
// Measured on one stream (profiles/backtrack_beside/README.md; 4K, 200 seams, parent / new): per launch k_vpath1 59.1 + k_carve_u 451.0 us
// -> k_carve_v 460.5 us (the walk role itself: 100 us inside the launch); 64 images, three alternating runs of 20 steps: 200.89 202.78
// 204.49 -> 193.85 195.43 197.60 ms per step (+3.8 % at the medians, every new run below every parent run).  Mseams*px/s in the order
// parent, new, new, parent: 8 images 177.4 k 180.1 k 178.2 k 177.4 k, 16: 302.3 328.2 323.8 304.6, 32: 406.2 437.6 437.5 407.0,
// 48: 492.5 527.3 528.0 492.7 -- every size run gains (8 by the least), so the threshold is the smallest size run, which is also where
// the energy update beside the carve starts; 5 .. 7 were not run.  Sub-batches on sibling streams are left out as they are there.
constexpr int BACKTRACK_BESIDE_MIN = 8;
static inline bool plan_backtrack_beside(const PlanKnobs &k, const PlanBatch &b, int delta, int h, bool energy_beside, int backtrack, bool catchup)
{
    if (k.backtrack_beside == 0 || !energy_beside || backtrack != LQRHIP_CENSUS_VPATH1 || delta < 1 || delta > 2 || !b.spin || catchup) return false;
    if (h < BB_MIN_ROWS || h > BB_MAX_ROWS || b.images > BB_MAX_IMAGES) return false;
    return k.backtrack_beside > 0 || (!b.shared && b.group() >= (size_t) BACKTRACK_BESIDE_MIN);
}

// Where the groups of a carved row start (the side right of the seam moves) or end (the left side moves): 1 = on a 32-element boundary,
// a 128-byte line of the float planes, 0 = on a 4-element boundary, the 16-byte vector (carve_row, k_carve.hip).  The same vectors are
// loaded and stored either way; line-aligned, a wave's 1 KB access covers 8 whole lines instead of 9 in 15 cases of 16 and two
// neighbouring chunks never request or partly write the same line.  A row costs one more group where the rounding pushes its moved
// part across a 1024-element boundary.  The knob at 0 pins 0 and at 1 pins 1 (k_carve itself has no such argument: its instructions
// are pinned); automatic: 1 for the launches that stream, k_carve_u and k_carve_v, 0 for k_carve_e -- the single images and small groups
// it serves are a chain of short dependent launches, where the one row in thirty that gets a second group is the launch's tail.
// Measured (profiles/carve_line/README.md): k_carve_v per launch at 64 x 4K, two traces each, parent 453.3 453.7, argument 0 453.5
// 454.7, argument 1 440.9 441.3 us; 64 images, three alternating runs of 20 steps, parent 172.93 174.43 175.54, new 170.95 171.91
// 172.85 ms per step.  With 1 for k_carve_e too, Mseams*px/s in the order parent, new, new, parent: fhd 15 462 15 322 15 322 15 524,
// single4k 26 544 26 495 26 529 26 531.
static inline int plan_carve_line(const PlanKnobs &k, int carve) { return k.carve_line >= 0 ? k.carve_line : carve == LQRHIP_CENSUS_CARVE ? 1 : 0; }

// One seam of a lock-step batch: the frame is w wide before it; `lag` seams separate the frozen planes from the frame after it
static inline StepPlan plan_seam_step(const PlanKnobs &k, const PlanDevice &d, const PlanBatch &b, int delta, bool use_rig, int w, int h, bool full_rebuild, int lag)
{
    StepPlan s;
    const int wnew = w - 1, mode = k.update_mode;
    const bool fast_delta = delta >= 1 && delta <= LQR_FAST_MAX_DELTA, general = delta != 1 || b.rigm(use_rig);
    // Backtrack: for single images the two-kernel parallel form (k_vp_maps / k_vp_solve, k_backtrack.hip: the chip walks every column
    // through every chunk of rows, the serial part is one step per chunk); for groups the one-wave-per-image walk, whose launches
    // keep the chip busy anyway.  Measured on one box, us per seam with every kernel event-timed, k_vpath1 / parallel: 4K 70 / 41 (single4k
    // 20.9 -> 22.7 k Mseams*px/s), 8K 108 / 64 (config 5 55.5 -> 60.8 k), FHD 32 / 30, 2 x 4K 57 / 44 (51.0 -> 53.4 k), 4 x 4K 59 / 61,
    // 8 x 4K 60 / 79: each launch is ~10 us of dependent-dispatch latency, and the maps of n images are n times the work.
    // delta_x 5 .. 10: always -- the one-wave walks there take 0.2 (k_vpath1<5>) to 1.15 ms (k_vpath, delta_x 10) per 4K seam, the parallel
    // form ~0.06 whatever delta_x is (a chunk is 56 / delta_x rows, the cone of a stage as wide as at delta_x 1)
    if (fast_delta && h >= 2 && k.vpath_mode != 0 && (k.vpath_mode == 1 || delta >= 5 || (b.group() <= (size_t) k.vpath_par_max && h >= k.vpath_min_rows))) {
        s.backtrack = LQRHIP_CENSUS_VP_PARALLEL;
        s.vp_rows = vp_chunk_rows(delta);
        s.vp_chunks = tiles_of(h - 1, s.vp_rows);
    } else s.backtrack = delta >= 1 && delta <= 7 ? LQRHIP_CENSUS_VPATH1 : LQRHIP_CENSUS_VPATH;      // (the one-wave walk is unrolled for delta_x 1 .. 7; delta_x 0 walks with k_vpath's loop)
    // Single images and small groups: the carve and the energy update in one launch (k_carve_e, k_carve.hip) -- the wave that has moved
    // a row refreshes that row's energies; one dependent launch less per seam.  delta_x <= 2 (12 brightness samples per row);
    // value-plane carvers: the two kernels
    s.carve = delta <= 2 && b.group() <= (size_t) k.carve_fused && wnew > 1 && !b.value ? LQRHIP_CENSUS_CARVE_E : LQRHIP_CENSUS_CARVE;
    s.energy_beside = s.carve == LQRHIP_CENSUS_CARVE && plan_carve_beside(k, b, delta, wnew);
    s.carve_line = plan_carve_line(k, s.carve);
    s.catchup = lag > frozen_lag(b.images);
    s.backtrack_beside = plan_backtrack_beside(k, b, delta, h, s.energy_beside, s.backtrack, s.catchup);
    s.eu_nt = eu_samples(delta);
    if (wnew <= 1) return s;
    if (full_rebuild) {
        s.full = true;
        s.dp = plan_full_dp(k, d, b, wnew, delta, use_rig);
        return s;
    }
    // How E9 (update_mmap) runs.  Small batches: the whole chip recomputing every row (tiled full-width keep-rule sweep) beats the
    // one-workgroup-per-image band walk; for large batches its 14 B/px of traffic would not.  `plain`: delta_x = 1 and no rigidity mask
    // that matters -- every fast kernel.  Other delta_x and rigidity masks run on the tiled full-width update (k_dp_tile_p's general
    // instantiations) whenever its grid fits; only beyond that do they fall to the one-wave-per-image band kernel and the
    // one-workgroup-per-image sweep (measured at 8K: 37x slower).
    // Whether the tiled update is wanted is decided from w, the frame before the seam; every launch geometry below from wnew
    const bool plain = !general && mode != 3;
    const bool tiled = (plain ? (mode < 0 ? (long long) b.images * w * h <= k.tiled_update_px : mode == 1) : (fast_delta && mode != 0 && mode != 2 && mode != 3)) &&
                       plan_persistent_px(k, d, b, w, general, delta, b.images) != 0;
    // the level kernel is asked first: a positive P wins over the tiled update
    if (fast_delta && mode != 3 && (mode == 5 || levels_auto(k, delta, b.group(), plain))) s.levels_P = plan_levels_P(k, d, b, wnew, h, delta);
    if (s.levels_P > 0) { s.band = LQRHIP_CENSUS_BAND_LEVELS; s.levels_wg_slots = plan_levels_wg_slots(k, d, b, delta, general, s.levels_P); s.levels_store = plan_levels_store(k, s.levels_wg_slots); }
    else if (tiled) {
        s.dp = plan_persistent(plan_persistent_px(k, d, b, wnew, general, delta, b.images), general, b.images);
        return s;
    } else if (plain && band_mw_fits(h)) {       // (the fast band kernels keep a row's seam positions in LDS)
        // the trapezoid-wave band kernel takes rows up to ~4200 px (wider rows: the changes outgrow its 896-column window too often, and
        // an 8-slot build spills registers); beyond that, and in update mode 2, k_band_update_mw: 8 waves, 16 for rows wider than 4200 px
        // (8K: dirty regions up to ~900 px)
        s.band = mode != 2 && wnew <= 4200 && band_tw_fits(h) ? LQRHIP_CENSUS_BAND_TW : wnew > 4200 ? LQRHIP_CENSUS_BAND_MW16 : LQRHIP_CENSUS_BAND_MW8;
    } else s.band = LQRHIP_CENSUS_BAND_GENERIC;
    s.dp = plan_sweep(k, wnew, true);
    return s;
}
