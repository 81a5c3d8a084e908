"""The launch shim's width and height thresholds, restated, and the cases that stand on both sides of each.

csrc/lqr_plan.h chooses kernels, thread counts, pixels per lane and LDS sizes from the carved frame's width and height (the launch
shim, csrc/lqr_shim.hip, launches what it plans).  This file holds (1) those choices as plain Python, each with the function or
expression of the planner it mirrors -- written independently of it: tests/test_plan.py compares the two without a GPU --, (2) THRESHOLDS: every switch as a quantity and a
limit, and (3) CASES: thin frames -- 6 to 40 rows or columns in the dimension that does not matter -- that reach every switch from
both sides.  tests/test_geometry_cases.py checks the table against the thresholds and runs the oracle on every case (no GPU);
tests/test_geometry_gpu.py runs the engine on them and compares the launch census (lqrhip_launch_census) with census().

A "session" is one visibility-map build: a frame fw wide (the direction being carved) and fh rows high loses `seams` seams.
"""
import numpy as np

import datasets as D

# ---- constants of csrc/lqr_plan.h -----------------------------------------------------------------------------------------------
DP_THREADS = 1024
LV_MAX_TILES = 64                  # one 64-bit mask of 64-column tiles
LV_MAX_LEVELS = 1020
DPP_BLK_BITS = 12
LQR_FAST_MAX_DELTA = 10
VP_REACH, VP_STAGE = 56, 20
MAX_FRAME_WIDTH = 16384            # include/lqr_hip.h LQRHIP_MAX_FRAME_WIDTH; lqr_plan.h plan_sweep: px 0
MI355X_CUS = 256                   # PlanDevice.n_cu on the device the suite runs on
TILED_UPDATE_PX = 8 * 3840 * 2160  # PlanKnobs.tiled_update_px
FROZEN_CARVE_FUSED = 4             # PlanKnobs.carve_fused
VPATH_PAR_MAX, VPATH_MIN_ROWS = 3, 1000          # PlanKnobs.vpath_par_max, vpath_min_rows


def dpp_own(px):                   # dpp_own / dpp_halo
    return {2: 64, 3: 32, 4: 128}[px]


def dpp_halo(px):
    return {2: 32, 3: 48, 4: 64}[px]


def dpp_rb(px, delta):             # dpp_rb: rows per block
    return dpp_halo(2) // delta if delta >= 5 else 8 if delta >= 3 else dpp_halo(px) // delta


def lv_rows(delta):                # lv_rows as plan_levels_P calls it (rigm = true)
    return 16 if delta <= 2 else 8 if delta <= 4 else 32 // delta


def vp_chunk_rows(delta):          # vp_chunk_rows
    return VP_REACH // delta


# census slots (include/lqr_hip.h)
VP_PARALLEL, VPATH1, VPATH, CARVE_E, CARVE = 0, 1, 2, 3, 4
TILE_P_G3, TILE_P_G2, TILE_P_G4, TILE_P_GENERAL, DP_TILE = 5, 6, 7, 8, 9
BAND_LEVELS, BAND_TW, BAND_MW8, BAND_MW16, BAND_GENERIC = 10, 11, 12, 13, 14
SWEEP, SWEEP_FULL, SWEEP_UPDATE, LDS_ATTR_SWEEP, LDS_ATTR_COMMIT, SLOTS = 15, 25, 26, 27, 28, 32
SLOT_NAMES = {0: "vp_parallel", 1: "k_vpath1", 2: "k_vpath", 3: "k_carve_e", 4: "k_carve", 5: "tile_p g3", 6: "tile_p g2", 7: "tile_p g4",
              8: "tile_p general", 9: "k_dp_tile", 10: "k_band_levels", 11: "band_tw", 12: "band_mw 8", 13: "band_mw 16", 14: "k_band_update",
              25: "sweep full", 26: "sweep update", 27: "sweep > 64 KB LDS", 28: "vs_commit > 64 KB LDS"}
for _i, _p in enumerate((1, 2, 4, 8, 16)):
    SLOT_NAMES[SWEEP + 2 * _i], SLOT_NAMES[SWEEP + 2 * _i + 1] = "k_dp_sweep<%d, 256>" % _p, "k_dp_sweep<%d, 1024>" % _p


def sweep_slot(px, threads):
    return SWEEP + 2 * (1, 2, 4, 8, 16).index(px) + (1 if threads == DP_THREADS else 0)


# ---- the planner's choices, restated (each names the function of csrc/lqr_plan.h it mirrors) ---------------------------------
def hook(case, name, default):
    return case.get("hooks", {}).get(name, default)


def rigm(case):
    """a rigidity mask that matters (PlanBatch::rigm)"""
    return bool(case["kw"].get("rigmask")) and case["kw"].get("rigidity", 0.0) != 0.0


def sweep_form(case, update, w):
    """plan_sweep: k_dp_sweep's threads and px per thread (the first of 1, 2, 4, 8, 16 that covers the row); None: past the last, refused"""
    nth = 256 if (update and hook(case, "sweep_threads", 256) == 256 and w <= 16 * 256) else DP_THREADS
    pxt = (w + nth - 1) // nth
    for p in (1, 2, 4, 8, 16):
        if pxt <= p:
            return p, nth
    return None


def sweep_lds(w):
    """plan_sweep: lds"""
    return 2 * ((w + 3) & ~3) * 4


def persistent_px(case, w, h, general, delta):
    """plan_persistent_px for ONE image on an otherwise idle MI355X: the residency bounds are at least one workgroup per compute unit
    whenever the persistent kernels run at all, and a frame of 16384 columns is 256 tiles of 64"""
    if hook(case, "no_spin", 0) or hook(case, "limit", -1) == 0 or case.get("redo"):
        return 0
    px_o, maxblk = hook(case, "px", 0), (1 << DPP_BLK_BITS) - 1
    tiles = lambda px: (w + dpp_own(px) - 1) // dpp_own(px)
    if not general and delta == 1 and px_o in (0, 3) and h <= maxblk * dpp_rb(3, 1) and (px_o == 3 or tiles(3) <= MI355X_CUS):
        return 3
    if (general or px_o not in (3, 4)) and h <= maxblk * dpp_rb(2, delta) and tiles(2) <= MI355X_CUS:
        return 2
    if not general and px_o not in (2, 3) and h <= maxblk * dpp_halo(4):
        return 4
    return 0


def levels_ok(case, w, h, delta):
    """plan_levels_P, its geometry part"""
    if hook(case, "no_spin", 0) or hook(case, "band_levels", -1) == 0 or not 1 <= delta <= LQR_FAST_MAX_DELTA:
        return False
    return (h + lv_rows(delta) - 1) // lv_rows(delta) <= LV_MAX_LEVELS and (w + 63) // 64 <= LV_MAX_TILES


def band_form(case, wnew, h):
    """plan_seam_step (band): which band kernel an update that reached the band kernels runs"""
    mode, delta = hook(case, "update_mode", -1), case["kw"].get("delta_x", 1)
    fast_ok = delta == 1 and not rigm(case) and mode != 3
    fast_band = fast_ok and h * 4 <= 60 * 1024
    if fast_band and mode != 2 and wnew <= 4200 and 2 * h * 4 <= 64 * 1024:
        return BAND_TW
    if fast_band:
        return BAND_MW16 if wnew > 4200 else BAND_MW8
    return BAND_GENERIC


def sessions(case):
    """liblqr's bookkeeping (host/lqr_sched.c lqr_walk_next, which host/lqr_carver.c group_resize_dir follows), restated independently
    of it -- tests/test_sched.py compares the two without a GPU: the sessions of the case's resize, as dicts fw, fh, seams"""
    w, h, nw, nh = case["w"], case["h"], case["nw"], case["nh"]
    enl = case["kw"].get("enl_step", 150.0) / 100.0
    out = []
    order = ("w", "h") if case["kw"].get("res_order", 0) == 0 else ("h", "w")
    for d in order:
        ws, rows, target = (w, h, nw) if d == "w" else (h, w, nh)
        if target < ws:
            out.append(dict(fw=ws, fh=rows, seams=ws - target))
            ws = target
        while target > ws:
            dmax = max(int((enl - 1) * ws) - 1, 1)
            step = min(target - ws, dmax)
            out.append(dict(fw=ws, fh=rows, seams=step))
            ws += step
        if d == "w":
            w = ws
        else:
            h = ws
    return out


def seam_steps(case, s):
    """(w_before, wnew, full_rebuild) of every seam of session s (the side-switch rule of host/lqr_sched.c lqr_session_seam, restated)"""
    sf = case["kw"].get("switch_freq", 2)
    interval = (s["seams"] - 1) // sf + 1 if sf else 0
    for i in range(s["seams"]):
        wb = s["fw"] - i
        full = wb - 1 > 1 and bool(sf) and (i + interval // 2) % interval == 0
        yield wb, wb - 1, full


def census(case):
    """what lqrhip_launch_census must read after ONE 8-bit image ran the case (kind "single"), slot by slot, exactly"""
    c = [0] * SLOTS
    delta, n = case["kw"].get("delta_x", 1), 1
    mode, vmode = hook(case, "update_mode", -1), hook(case, "vpath", -1)
    general = delta != 1 or rigm(case)

    def full_dp(w, h):
        if 1 <= delta <= LQR_FAST_MAX_DELTA:
            px = persistent_px(case, w, h, general, delta)
            if px:
                c[TILE_P_GENERAL if general else {3: TILE_P_G3, 2: TILE_P_G2, 4: TILE_P_G4}[px]] += 1
                return
            if not general:
                c[DP_TILE] += (h + 31) // 32
                return
        p, t = sweep_form(case, False, w)
        c[sweep_slot(p, t)] += 1; c[SWEEP_FULL] += 1
        c[LDS_ATTR_SWEEP] += sweep_lds(w) > 64 * 1024

    def sweep_update(w):
        p, t = sweep_form(case, True, w)
        c[sweep_slot(p, t)] += 1; c[SWEEP_UPDATE] += 1
        c[LDS_ATTR_SWEEP] += sweep_lds(w) > 64 * 1024

    for s in sessions(case):
        h = s["fh"]
        full_dp(s["fw"], h)
        for wb, wnew, full in seam_steps(case, s):
            use_vp = 1 <= delta <= LQR_FAST_MAX_DELTA and h >= 2 and vmode != 0 and (vmode == 1 or delta >= 5 or (n <= VPATH_PAR_MAX and h >= VPATH_MIN_ROWS))
            c[VP_PARALLEL if use_vp else VPATH1 if 1 <= delta <= 7 else VPATH] += 1     # plan_seam_step: backtrack
            c[CARVE_E if (delta <= 2 and n <= FROZEN_CARVE_FUSED and wnew > 1) else CARVE] += 1      # the carve
            if wnew <= 1:
                continue
            if full:
                full_dp(wnew, h)
                continue
            fast_ok = delta == 1 and not rigm(case) and mode != 3                       # plan_seam_step: plain, tiled
            if fast_ok:
                tiled = (n * wb * h <= TILED_UPDATE_PX if mode < 0 else mode == 1) and persistent_px(case, wb, h, False, 1) != 0
            else:
                tiled = 1 <= delta <= LQR_FAST_MAX_DELTA and mode not in (0, 2, 3) and persistent_px(case, wb, h, True, delta) != 0
            if mode == 5 and (delta <= LQR_FAST_MAX_DELTA) and levels_ok(case, wnew, h, delta):      # plan_levels_P (a single image: on request only)
                c[BAND_LEVELS] += 1
                sweep_update(wnew)
            elif tiled:
                px = persistent_px(case, wnew, h, general, delta)
                c[TILE_P_GENERAL if general else {3: TILE_P_G3, 2: TILE_P_G2, 4: TILE_P_G4}[px]] += 1
            else:
                c[band_form(case, wnew, h)] += 1
                sweep_update(wnew)
        c[LDS_ATTR_COMMIT] += (s["seams"] + s["fw"]) * 4 > 64 * 1024                   # lqrhip_vs_commit: lds
    return c


# ---- the thresholds -------------------------------------------------------------------------------------------------------------
# name -> (mirrors, limit(case) or None where the threshold does not apply to the case, values(case, session) -> the quantity compared
# with the limit during that session, crossable inside a session).  A value <= limit is the "lo" side, above it the "hi" side.
def _delta(case):
    return case["kw"].get("delta_x", 1)


def _mode(case):
    return hook(case, "update_mode", -1)


def _one(case):
    return case["kind"] in ("single", "planes")


def _wnews(case, s):
    return [wn for _, wn, full in seam_steps(case, s) if wn > 1 and not full]


def _band_case(case):
    """updates of the case reach a band kernel and the sweep behind it"""
    return _one(case) and (census(case)[SWEEP_UPDATE] > 0)


def _levels_case(case):
    return case["kind"] == "group" and (_mode(case) == 5 or (_mode(case) < 0 and case["n"] >= 8)) and (_delta(case) <= 4 or _mode(case) == 5)


THRESHOLDS = {
    "levels_tiles_4096": ("plan_levels_P: tiles_of(w, 64) > LV_MAX_TILES",
                          lambda c: 4096 if _levels_case(c) else None, _wnews, True),
    "sweep_threads_4096": ("plan_sweep: threads, w <= 16 * 256",
                           lambda c: 4096 if (_band_case(c) or _levels_case(c)) else None, _wnews, True),
    "band_tw_width_4200": ("plan_seam_step: band, wnew <= 4200",
                           lambda c: 4200 if _band_case(c) and _mode(c) == 0 and _delta(c) == 1 and not rigm(c) else None, _wnews, True),
    "band_mw_waves_4200": ("plan_seam_step: band, wnew > 4200 -> 16 waves",
                           lambda c: 4200 if _band_case(c) and _mode(c) == 2 and _delta(c) == 1 and not rigm(c) else None, _wnews, True),
    "sweep_px_lds_8192": ("plan_sweep: px <= 8; lds_needs_attr, lds > 64 KB",
                          lambda c: 8192 if _band_case(c) else None, _wnews, True),
    "tile_geometry3_8192": ("plan_persistent_px: 32-column tiles <= compute units",
                            lambda c: 8192 if _one(c) and sum(census(c)[TILE_P_G3:TILE_P_G4 + 1]) > 0 and hook(c, "px", 0) == 0 else None,
                            lambda c, s: [s["fw"]], False),
    "commit_lds_16384": ("lqrhip_vs_commit: (n_seams + wc0) * 4 > 64 KB",
                         lambda c: 16384 if c["kind"] != "refused" else None, lambda c, s: [s["fw"], s["fw"] + s["seams"]], True),
    "frame_limit_16384": ("plan_sweep: px 0; host/lqr_carver.c frame_refused",
                          lambda c: 16384, lambda c, s: [s["fw"]], False),
    "band_tw_lds_8192_rows": ("plan_seam_step: band, 2 * h * 4 <= 64 KB",
                              lambda c: 8192 if _band_case(c) and _mode(c) == 0 and _delta(c) == 1 and max(c["w"], c["nw"]) <= 4200 else None,
                              lambda c, s: [s["fh"]], False),
    "fast_band_15360_rows": ("plan_seam_step: band, h * 4 <= 60 KB",
                             lambda c: 15360 if _band_case(c) and _mode(c) in (0, 2) and _delta(c) == 1 else None, lambda c, s: [s["fh"]], False),
    "block_field_12285_rows": ("plan_persistent_px: wk_h <= 4095 * dpp_rb(2, delta), delta 9 and 10",
                               lambda c: 4095 * dpp_rb(2, 10) if _one(c) and _delta(c) in (9, 10) and _mode(c) < 0 else None,
                               lambda c, s: [s["fh"]], False),
    "block_field_16380_rows": ("plan_persistent_px: the same, delta 7 and 8",
                               lambda c: 4095 * dpp_rb(2, 8) if _one(c) and _delta(c) in (7, 8) and _mode(c) < 0 else None,
                               lambda c, s: [s["fh"]], False),
    "levels_8160_rows": ("plan_levels_P: LV_MAX_LEVELS * lv_rows, delta 3 and 4",
                         lambda c: LV_MAX_LEVELS * lv_rows(3) if _levels_case(c) and _delta(c) in (3, 4) else None, lambda c, s: [s["fh"]], False),
    "levels_16320_rows": ("plan_levels_P: the same, delta 1 and 2",
                          lambda c: LV_MAX_LEVELS * lv_rows(2) if _levels_case(c) and _delta(c) in (1, 2) else None, lambda c, s: [s["fh"]], False),
}
CROSSED_IN_SESSION = ("levels_tiles_4096", "sweep_threads_4096", "band_tw_width_4200", "band_mw_waves_4200", "sweep_px_lds_8192", "commit_lds_16384")


def sides(case, name):
    """which sides of threshold `name` the case stands on ("lo", "hi"), and whether one of its sessions stands on both"""
    _, limit, values, _ = THRESHOLDS[name]
    lim = limit(case)
    if lim is None:
        return set(), False
    seen, crossed = set(), False
    for s in sessions(case):
        v = values(case, s)
        here = {"lo" if x <= lim else "hi" for x in v}
        seen |= here
        crossed |= len(here) == 2
    return seen, crossed


# ---- the cases ------------------------------------------------------------------------------------------------------------------
# kind: "single" -- one 8-bit image through harness.run_case, census() exact; "planes" -- the same plus the DP planes after the
# session (debug_snapshot); "group" -- n images, `expect` names slots that must be > 0 ("+"), == 0 (0) or, as a tuple, of which one
# must be > 0, "auto+": > 0 if the engine carves the n images as one group (lqrhip_general_batch_limit_delta >= n: a device-dependent
# residency bound), else 0; "fault" / "lift" -- the recovery and the 16-bit test of tests/test_geometry_gpu.py; "refused" -- the host
# must refuse it.  kw: harness.run_case's keywords (pres / rigmask: True = datasets' masks).
# hooks: update_mode, limit (lqrhip_set_dp_persistent_limit), px, no_spin, vpath, band_levels, sweep_threads.
CASES = []


def case(name, w, h, nw, nh, kind="single", n=1, hooks=None, expect=None, data=None, **kw):
    assert not any(c["name"] == name for c in CASES), name
    if kind == "group":          # the dumped maps and the progress events are compared too
        kw = dict(kw, output_seams=True, progress=True)
    CASES.append(dict(name=name, w=w, h=h, nw=nw, nh=nh, kind=kind, n=n, hooks=hooks or {}, expect=expect or {}, data=data, kw=kw))


# -- wide frames
for _w in (4096, 4097, 4108):        # 4097: the first update is of a 4096-column frame -- the switches compare wnew
    case("group8_%d" % _w, _w, 12, _w - 8, 12, kind="group", n=8,
         expect={BAND_LEVELS: "+", sweep_slot(16, 256): "+", SWEEP_UPDATE: "+", TILE_P_G4: 0} if _w <= 4097 else
                {BAND_LEVELS: 0, SWEEP_UPDATE: 0, TILE_P_G2: "+", TILE_P_G4: 0})      # 65 tiles: the tiled update, 64-column tiles
    case("single_%d_band" % _w, _w, 12, _w - 8, 12, kind="planes", hooks=dict(update_mode=0), switch_freq=0)
case("group8_4100_crosses", 4100, 12, 4090, 12, kind="group", n=8, expect={BAND_LEVELS: "+", TILE_P_G2: "+", TILE_P_G4: 0})
case("single_4100_band_crosses", 4100, 12, 4090, 12, kind="planes", hooks=dict(update_mode=0))
for _m in (0, 2):
    case("w4203_mode%d" % _m, 4203, 30, 4190, 30, kind="planes", hooks=dict(update_mode=_m))
case("w8196_sweep_delta2", 8196, 24, 8186, 24, kind="planes", hooks=dict(limit=0), delta_x=2, rigidity=2.0)
case("w8196_delta16", 8196, 24, 8186, 24, kind="planes", delta_x=16)
case("w8196_nospin", 8196, 24, 8186, 24, kind="planes", hooks=dict(no_spin=1))
case("w8192_nospin", 8192, 24, 8182, 24, hooks=dict(no_spin=1))
# (the cases in which the band kernel really hands rows over to the sweep behind it: NOTES/geometry-tests.md, the mutation record)
case("w8196_delta16_40_seams", 8196, 40, 8156, 40, kind="planes", delta_x=16)
case("w8192_own", 8192, 24, 8182, 24)
case("w8196_own", 8196, 24, 8186, 24)
W16 = dict(w=16384, h=24, nw=16344, nh=24)
case("w16384_own", **W16)
case("w16384_px2", hooks=dict(px=2), **W16)
case("w16384_px4", hooks=dict(px=4), **W16)
case("w16384_limit0", kind="planes", hooks=dict(limit=0), **W16)
case("w16384_nospin", hooks=dict(no_spin=1), **W16)
case("w16384_sweep_delta2", kind="planes", hooks=dict(limit=0), delta_x=2, rigidity=2.0, **W16)
case("w16384_delta3_rig", delta_x=3, rigidity=2.0, **W16)
case("w16384_delta16", kind="planes", delta_x=16, **W16)
case("w16384_vp_parallel", hooks=dict(vpath=1), **W16)
case("w16384_vpath1", hooks=dict(vpath=0), **W16)
case("w16384_mode3", kind="planes", hooks=dict(update_mode=3), **W16)
case("w16384_tie0", switch_freq=0, **W16)
case("w16384_tie3", switch_freq=3, **W16)
case("w16384_bias", pres=True, **W16)
case("w16384_rigmask", rigmask=True, rigidity=1.0, **W16)
case("w16384x16_both_hor", 16384, 16, 16380, 12)
case("w16384x16_both_ver", 16384, 16, 16380, 12, res_order=1)
case("tall_image_transposed", 12, 16384, 12, 16370)
case("w8400_8100_seams", 8400, 6, 300, 6)
case("w16384_enlarge", 16384, 12, 16390, 12)
# stepwise enlargement (enl_step 1.5): 11000 columns grow by at most 5499 in one session, 10922 by 5460 -- to 16499 in one step;
# to 16390 from 10922 in two, the second from a flattened image of 16382 columns; to 16500 from 11000 the second session would
# start from 16499 columns: refused (below, "past the limit")
case("w11000_enlarge_one_step", 11000, 6, 16499, 6)
case("w10922_enlarge_two_steps", 10922, 6, 16390, 6)
case("w16384x16_fault", 16384, 16, 16364, 16, kind="fault")
case("w16384x16_lift16", 16384, 16, 16364, 16, kind="lift", switch_freq=1)
case("w1200_commit_lo", 1200, 12, 1190, 12)
for _n in (2, 9):
    case("group%d_8300_band" % _n, 8300, 16, 8290, 16, kind="group", n=_n, hooks=dict(update_mode=0),
         expect={BAND_MW16: "+", BAND_LEVELS: 0, BAND_MW8: 0, BAND_TW: 0, sweep_slot(16, 1024): "+", LDS_ATTR_SWEEP: "+",
                 TILE_P_G2: "+" if _n == 2 else 0, TILE_P_G4: "+" if _n == 9 else 0})     # full DPs: 9 x 130 tiles of 64 pass the residency bound
case("group9_8300", 8300, 16, 8290, 16, kind="group", n=9, expect={BAND_LEVELS: 0, TILE_P_G4: "+", TILE_P_G2: 0, BAND_MW16: 0, SWEEP_UPDATE: 0})
# -- tall frames
for _h in (8192, 8193):
    for _m in (-1, 0, 2):
        case("h%d_mode%d" % (_h, _m), 24, _h, 16, _h, kind="single" if _m < 0 else "planes", hooks=dict(update_mode=_m))
for _h in (15360, 15361):
    for _m in (0, 2):
        case("h%d_mode%d" % (_h, _m), 20, _h, 14, _h, kind="planes", hooks=dict(update_mode=_m))
# wider than a band kernel's window, so that rows are handed to k_dp_sweep<2 / 8 px, 256 threads>
# (noise: datasets.photo_like takes seconds to make an image this tall and more than a few columns wide)
# k_band_update hands over when the band passes 248 columns of its 256, the 8-wave k_band_update_mw at 740 of its 1024; 1200 columns
# are k_dp_sweep<8 px, 256 threads>, which no narrower frame runs.  The oracle's own update of a tall frame costs a pass over most of
# it per seam, hence 3 seams (update, full rebuild, update) at 300 columns; at 1200 columns the band reaches 740 columns only in some
# of the updates, and with 3 seams a sweep that does nothing goes unnoticed (NOTES/geometry-tests.md): 6, as in the thin frames
case("h15361_w300_mode0", 300, 15361, 297, 15361, kind="planes", hooks=dict(update_mode=0), data="noise")
case("h8193_w1200_mode0", 1200, 8193, 1194, 8193, kind="planes", hooks=dict(update_mode=0), data="noise")
for _h, _d in ((12285, 10), (12286, 10), (12285, 9), (12286, 9), (16380, 8), (16381, 8), (16380, 7), (16381, 7)):
    case("h%d_delta%d" % (_h, _d), 40 if _d >= 9 else 32, _h, (40 if _d >= 9 else 32) - 6, _h, kind="planes" if _d in (10, 8) else "single", delta_x=_d)
for _h in (8160, 8161):
    case("group8_h%d_delta3_levels" % _h, 40, _h, 34, _h, kind="group", n=8, hooks=dict(update_mode=5, band_levels=7), delta_x=3,
         expect={BAND_LEVELS: "+" if _h == 8160 else 0, TILE_P_GENERAL: "+"})
    case("group8_h%d_delta3_auto" % _h, 40, _h, 34, _h, kind="group", n=8, delta_x=3,
         expect={BAND_LEVELS: "auto+" if _h == 8160 else 0, TILE_P_GENERAL: "+"})
for _h in (16320, 16321):
    case("group8_h%d_delta2_levels" % _h, 32, _h, 26, _h, kind="group", n=8, hooks=dict(update_mode=5, band_levels=7), delta_x=2,
         expect={BAND_LEVELS: "+" if _h == 16320 else 0, TILE_P_GENERAL: "+"})
    case("group8_h%d_delta2_auto" % _h, 32, _h, 26, _h, kind="group", n=8, delta_x=2,
         expect={BAND_LEVELS: "auto+" if _h == 16320 else 0, TILE_P_GENERAL: "+"})
for _d in (1, 4, 10):
    for _v in (1, 0):
        case("h16384_delta%d_vpath%d" % (_d, _v), 24, 16384, 18, 16384, hooks=dict(vpath=_v), delta_x=_d)
# -- past the limit: refused on the host
case("w16385_refused", 16385, 8, 16380, 8, kind="refused")
case("h16385_refused", 8, 16385, 8, 16380, kind="refused")
case("w11000_enlarge_two_steps_refused", 11000, 6, 16500, 6, kind="refused")

BY_NAME = {c["name"]: c for c in CASES}


def image(c, i=0):
    """noise and photo-like inputs in turn (never flat: ties would hide a column that was never computed); one image per shape, so
    that the variants of a shape share their reference"""
    seed = 9000 + (c["w"] * 7 + c["h"]) % 977 + 31 * i
    return (D.noise if (seed % 2 or c.get("data") == "noise") else D.photo_like)(c["w"], c["h"], seed)


_REF = {}


def reference(oracle, c, i=0):
    """the oracle's result for image i of the case, computed once per (shape, target, parameters)"""
    import harness as H
    key = (c["w"], c["h"], c["nw"], c["nh"], i, repr(sorted(c["kw"].items())))
    if key not in _REF:
        _REF[key] = H.run_case(oracle, image(c, i), c["nw"], c["nh"], **run_kw(c))
    return _REF[key]


def run_kw(c):
    kw = dict(c["kw"])
    if kw.pop("pres", False):
        kw["pres"] = D.ellipse_mask(c["w"], c["h"])
    if kw.pop("rigmask", False):
        kw["rigmask"] = D.top_half_mask(c["w"], c["h"])
    return kw


def vp_geometry(c):
    """chunks and LDS stages of the parallel backtrack in the case's first session (plan_seam_step: vp_chunks; k_backtrack.hip)"""
    s, r = sessions(c)[0], vp_chunk_rows(c["kw"].get("delta_x", 1))
    nchunks = (s["fh"] - 1 + r - 1) // r
    return nchunks, (nchunks + VP_STAGE - 1) // VP_STAGE
