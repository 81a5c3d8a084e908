"""The case table of tests/geometry_cases.py against the thresholds it restates (no GPU): both sides of every switch of the launch
shim are reached, the switches a session can cross are crossed inside one session, and the oracle alone accepts every case."""
import time

import numpy as np
import pytest

import geometry_cases as G
import harness as H
import lqr_ctypes as L


@pytest.mark.parametrize("name", sorted(G.THRESHOLDS))
def test_every_threshold_has_a_case_on_each_side(name):
    lo = [c["name"] for c in G.CASES if "lo" in G.sides(c, name)[0]]
    hi = [c["name"] for c in G.CASES if "hi" in G.sides(c, name)[0]]
    assert lo and hi, (name, G.THRESHOLDS[name][0], lo[:3], hi[:3])


@pytest.mark.parametrize("name", G.CROSSED_IN_SESSION)
def test_thresholds_a_session_can_cross_are_crossed_inside_one(name):
    assert G.THRESHOLDS[name][3]
    crossing = [c["name"] for c in G.CASES if G.sides(c, name)[1]]
    assert crossing, (name, G.THRESHOLDS[name][0])


def test_restated_constants_match_the_sources():
    """the numbers this table is built on, read from the sources they mirror"""
    import os
    import re
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gimp-lqr-plugin_amd", "csrc")
    common = open(os.path.join(root, "lqr_plan.h")).read()          # the geometry constants the choices depend on live with the choices
    hdr = open(os.path.join(os.path.dirname(root), "..", "include", "lqr_hip.h")).read()
    for pat, want in ((r"constexpr int LV_MAX_TILES = (\d+);", G.LV_MAX_TILES), (r"constexpr int LV_MAX_LEVELS = (\d+);", G.LV_MAX_LEVELS),
                      (r"constexpr int DPP_BLK_BITS = (\d+);", G.DPP_BLK_BITS), (r"#define DP_THREADS (\d+)", G.DP_THREADS),
                      (r"constexpr int VP_REACH = (\d+);", G.VP_REACH), (r"constexpr int VP_STAGE = (\d+);", G.VP_STAGE)):
        assert int(re.search(pat, common).group(1)) == want, pat
    assert int(re.search(r"#define LQRHIP_MAX_FRAME_WIDTH (\d+)", hdr).group(1)) == G.MAX_FRAME_WIDTH
    assert int(re.search(r"LQRHIP_CENSUS_SLOTS = (\d+)", hdr).group(1)) == G.SLOTS
    # (the selection expressions themselves -- 16 * 256, 4200, 60 KB, 64 KB -- are held by the census assertions of
    # tests/test_geometry_gpu.py: an expression that changed makes another form run)
    assert 4095 * G.dpp_rb(2, 10) == 4095 * G.dpp_rb(2, 9) == 12285 and 4095 * G.dpp_rb(2, 8) == 4095 * G.dpp_rb(2, 7) == 16380
    assert G.LV_MAX_LEVELS * G.lv_rows(3) == 8160 and G.LV_MAX_LEVELS * G.lv_rows(2) == G.LV_MAX_LEVELS * G.lv_rows(1) == 16320


def test_the_table_names_the_forms_the_issue_lists():
    """every form of the census is what some case must run, and the hand-overs meant to be tested have rows to hand over"""
    ran = [0] * G.SLOTS
    for c in G.CASES:
        if c["kind"] in ("single", "planes"):
            ran = [a + b for a, b in zip(ran, G.census(c))]
        for k, v in c["expect"].items():
            if v == "+" and not isinstance(k, tuple):
                ran[k] += 1
    never = [G.SLOT_NAMES[i] for i in sorted(G.SLOT_NAMES) if not ran[i]]
    # k_dp_sweep with 2 or 4 px per thread over 1024 threads is a FULL sweep of a frame of 1025 .. 4096 columns that no persistent and no
    # tiled kernel takes: delta_x > 10, which tests/test_parity_gpu.py runs; 4 px over 256 threads: a band-mode frame of 513 .. 1024 columns
    assert set(never) <= {"k_dp_sweep<4, 256>", "k_dp_sweep<2, 1024>", "k_dp_sweep<4, 1024>"}, never
    for must in (G.sweep_slot(16, 1024), G.sweep_slot(16, 256), G.sweep_slot(8, 1024), G.LDS_ATTR_SWEEP, G.LDS_ATTR_COMMIT, G.BAND_MW16, G.BAND_GENERIC, G.TILE_P_G2, G.TILE_P_G4):
        assert ran[must], G.SLOT_NAMES[must]
    # one session runs both band kernels, and the 8- and the 16-wave form
    c0, c2 = G.census(G.BY_NAME["w4203_mode0"]), G.census(G.BY_NAME["w4203_mode2"])
    assert c0[G.BAND_MW16] == 2 and c0[G.BAND_TW] == 9 and c2[G.BAND_MW16] == 2 and c2[G.BAND_MW8] == 9, (c0, c2)
    # the parallel backtrack at 16384 rows: 293 chunks in 15 stages at delta_x 1, 3277 in 164 at delta_x 10
    assert G.vp_geometry(G.BY_NAME["h16384_delta1_vpath1"]) == (293, 15) and G.vp_geometry(G.BY_NAME["h16384_delta10_vpath1"]) == (3277, 164)
    # the refusal is decided from the sizes: nothing wider than the limit is among the cases that run
    for c in G.CASES:
        wide = max(s["fw"] for s in G.sessions(c))
        assert (wide > G.MAX_FRAME_WIDTH) == (c["kind"] == "refused"), c["name"]


@pytest.mark.parametrize("name", [c["name"] for c in G.CASES])
def test_the_oracle_accepts_every_case(oracle, name):
    """the reference alone takes the input and finishes in the time a thin frame needs.  Measured: 0.002 .. 0.6 s of CPU time per case,
    except the two tall frames that are wider than a band kernel's window, 0.8 s (300 x 15361) and 1.8 s (1200 x 8193); 13 s for all 82.
    The bound is on CPU time, not on the clock, so that load on a shared machine cannot fail it, and leaves a factor of 2.8
    over the slowest case for a slower processor."""
    c = G.BY_NAME[name]
    img = G.image(c)
    t0 = time.process_time()
    r = H.run_case(oracle, img, c["nw"], c["nh"], **G.run_kw(c))
    dt = time.process_time() - t0
    assert r["ret"] == L.LQR_OK and r["image"].shape[:2] == (c["nh"], c["nw"]), name
    assert r["getters"] and np.asarray(r["vmap"]["data"]).max() == r["vmap"]["depth"]
    assert dt < 5.0, "%s: %.2f s of CPU time in the oracle" % (name, dt)
