"""Parity across the launch shim's width and height thresholds (-m gpu): every case of tests/geometry_cases.py on the engine against
the oracle -- maps, pixels, getters, dumped maps, progress events, bit for bit -- and the launch census (lqrhip_launch_census) against
what the table says must have run: exactly, slot by slot, for single images; the named forms for groups, whose images are each
compared in full too, with dumped maps and a progress recorder on.  A case that took another
path fails even if its pixels are right.  Where a case pins the DP itself (kind "planes") the energies, cumulative minima and back
pointers after the session's incremental updates are compared too.

Measured on one MI355X, oracle references included (each is computed once per shape and shared by the variants of that shape):
the file alone 31.6 s for 80 tests.  Per test: group8_h16320 / h16321_delta2_levels 2.3 - 2.5, group8_h8160 / h8161_delta3_levels
1.4 - 1.5, h8193_w1200_mode0 1.4 - 1.8, h12286_delta10 1.4, h16381_delta8 1.3, group8_h1632x_delta2_auto 1.2, h15361_w300_mode0 0.85,
h16384_delta10_vpath1 0.8, h12286_delta9 0.7, h16384_delta10_vpath0 0.65, h15361_mode0 / 2 0.6, h16380_delta8 0.6,
w8196_delta16_40_seams 0.6, h16381_delta7 0.6, group8_h816x_delta3_auto 0.5; every other test 0.01 - 0.5 (the 8100-seam case 0.3, the
two stepwise enlargements of 5460 - 5499 seams 0.2 - 0.3, the fault test 0.02, the lift 0.02, the refusals 0.4).
The whole -m gpu suite at the parent commit on the same machine: 493.7 s for 1248 tests; this file adds its 32 s to that.
"""
import ctypes

import numpy as np
import pytest

import datasets as D
import geometry_cases as G
import harness as H
import lqr_ctypes as L

pytestmark = pytest.mark.gpu


@pytest.fixture()
def lib(engine):
    lb = engine.lib
    lb.lqrhip_launch_census.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int, ctypes.c_int]
    lb.lqrhip_launch_census.restype = ctypes.c_int
    lb.lqrhip_fault_stats.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
    lb.lqrhip_general_batch_limit_delta.argtypes = [ctypes.c_int, ctypes.c_int]
    lb.lqrhip_general_batch_limit_delta.restype = ctypes.c_int
    lb.lqrhip_set_vpath_mode.argtypes = [ctypes.c_int, ctypes.c_int]
    for f in ("lqrhip_set_update_mode", "lqrhip_set_dp_persistent_limit", "lqrhip_set_dp_persistent_px", "lqrhip_set_no_spin",
              "lqrhip_set_band_levels", "lqrhip_set_sweep_threads"):
        getattr(lb, f).argtypes = [ctypes.c_int]
    lb.lqrhip_debug_inject.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int]
    yield lb
    reset_hooks(lb)


def reset_hooks(lb):
    lb.lqrhip_set_update_mode(-1); lb.lqrhip_set_dp_persistent_limit(-1); lb.lqrhip_set_dp_persistent_px(0); lb.lqrhip_set_no_spin(0)
    lb.lqrhip_set_band_levels(-1); lb.lqrhip_set_sweep_threads(256); lb.lqrhip_set_vpath_mode(-1, 3); lb.lqrhip_debug_inject(0, 0, 0)


def set_hooks(lb, c):
    hk = c["hooks"]
    lb.lqrhip_set_update_mode(hk.get("update_mode", -1)); lb.lqrhip_set_dp_persistent_limit(hk.get("limit", -1))
    lb.lqrhip_set_dp_persistent_px(hk.get("px", 0)); lb.lqrhip_set_no_spin(hk.get("no_spin", 0))
    lb.lqrhip_set_band_levels(hk.get("band_levels", -1)); lb.lqrhip_set_sweep_threads(hk.get("sweep_threads", 256))
    lb.lqrhip_set_vpath_mode(hk.get("vpath", -1), 3)


def census(lb, reset=True):
    out = (ctypes.c_ulonglong * G.SLOTS)()
    assert lb.lqrhip_launch_census(out, G.SLOTS, 1 if reset else 0) == G.SLOTS
    return [int(x) for x in out]


def describe(cs):
    return ", ".join("%s: %d" % (G.SLOT_NAMES.get(i, "slot %d" % i), v) for i, v in enumerate(cs) if v)


def cases(*kinds):
    return [c["name"] for c in G.CASES if c["kind"] in kinds]


@pytest.mark.parametrize("name", cases("single", "planes"))
def test_single_images_across_the_thresholds(oracle, engine, lib, name):
    c = G.BY_NAME[name]
    img, kw = G.image(c), G.run_kw(c)
    ref = G.reference(oracle, c)
    try:
        set_hooks(lib, c)
        census(lib)
        got = H.run_case(engine, img, c["nw"], c["nh"], **kw)
        ran, want = census(lib), G.census(c)
        print("%s census: %s" % (name, describe(ran)))
        H.assert_same(ref, got, name)
        assert ran == want, "%s ran [%s], the table says [%s]" % (name, describe(ran), describe(want))
        if c["kind"] == "planes":
            oracle.lqrx_set_debug(1); engine.lqrx_set_debug(1)
            s = G.sessions(c)[0]
            assert s["fw"] == c["w"]
            ca, _ = H.init_carver(oracle, img, c["nw"], c["h"], **kw); cb, _ = H.init_carver(engine, img, c["nw"], c["h"], **kw)
            assert ca.resize(c["nw"], c["h"]) == L.LQR_OK and cb.resize(c["nw"], c["h"]) == L.LQR_OK
            (ea, ma, da), (eb, mb, db) = ca.debug_snapshot(), cb.debug_snapshot()
            assert np.array_equal(ea.view(np.int32), eb.view(np.int32)), name + ": energies"
            assert np.array_equal(ma.view(np.int32), mb.view(np.int32)), name + ": cumulative minima, first at %s" % (np.argwhere(ma.view(np.int32) != mb.view(np.int32))[:1],)
            assert np.array_equal(da[1:], db[1:]), name + ": back pointers"
            ca.destroy(); cb.destroy()
    finally:
        oracle.lqrx_set_debug(0); engine.lqrx_set_debug(0)
        reset_hooks(lib)


@pytest.mark.parametrize("name", cases("group"))
def test_groups_across_the_thresholds(oracle, engine, lib, name):
    c = G.BY_NAME[name]
    kw = G.run_kw(c)
    imgs = [G.image(c, i) for i in range(c["n"])]
    try:
        set_hooks(lib, c)
        one_group = lib.lqrhip_general_batch_limit_delta(max(c["w"], c["h"], c["nw"], c["nh"]), kw.get("delta_x", 1)) >= c["n"]
        cs = [H.init_carver(engine, im, c["nw"], c["nh"], **kw)[0] for im in imgs]
        census(lib)
        ret = L.resize_batch(engine, cs, c["nw"], c["nh"])
        ran = census(lib)
        print("%s census (one group: %s): %s" % (name, one_group, describe(ran)))
        for i, cv in enumerate(cs):
            # what harness.run_case reads out after its resize: dumped maps, getters, pixels, the seam map, the progress events
            got = dict(ret=ret, vmaps=cv.dumped_vmaps(), getters=cv.getters(), aux=[], vmap=cv.vmap_dump(), events=list(cv.events))
            got["image"], got["nlines"] = cv.read_scanlines()
            ref = G.reference(oracle, c, i)
            assert ref["ret"] == L.LQR_OK and len(ref["vmaps"]) == 1 and len(ref["events"]) >= 3, name
            # a group reports its progress through its first carver (host/lqr_carver.c group_resize_dir): image 0 fires the oracle's
            # events, a later image the same ones if it leads a sub-group and none if it follows
            assert got["events"] == ref["events"] or (i > 0 and not got["events"]), "%s: progress events of image %d: %s" % (name, i, got["events"][:4])
            H.assert_same(dict(ref, events=got["events"]), got, "%s image %d" % (name, i))
        for cv in cs:
            cv.destroy()
        for slot, want in c["expect"].items():
            if want == "auto+":
                want = "+" if one_group else 0
            count = sum(ran[s] for s in slot) if isinstance(slot, tuple) else ran[slot]
            label = "/".join(G.SLOT_NAMES[s] for s in (slot if isinstance(slot, tuple) else (slot,)))
            assert (count > 0) if want == "+" else (count == want), "%s: %s launched %d times, the table says %r; ran [%s]" % (name, label, count, want, describe(ran))
    finally:
        reset_hooks(lib)


def test_an_injected_fault_in_a_16384_column_session_is_redone_on_the_recovery_kernels(oracle, engine, lib):
    """a seam-log entry out of the frame at seam 9: the self-check after the seam loop refuses the session, it is rolled back and carved again on
    k_dp_tile, k_band_update_mw<16 waves> and k_dp_sweep<16 px, 1024 threads> with 128 KB of LDS; exact"""
    c = G.BY_NAME["w16384x16_fault"]
    st = (ctypes.c_ulonglong * 8)()
    try:
        lib.lqrhip_fault_stats(st, 1)
        census(lib)
        lib.lqrhip_debug_inject(3, 9, 1)
        got = H.run_case(engine, G.image(c), c["nw"], c["nh"])
        ran = census(lib)
        lib.lqrhip_fault_stats(st, 1)
        print("fault census: %s; stats %s" % (describe(ran), list(st)))
        H.assert_same(G.reference(oracle, c), got, "recovered")
        assert st[2] == 1 and st[4] == 1 and st[5] == 1 and st[6] >= 1, list(st)
        assert lib.lqrhip_get_no_spin() == 0
        seams = c["w"] - c["nw"]
        assert ran[G.TILE_P_G2] > 0 and ran[G.DP_TILE] > 0 and ran[G.BAND_MW16] > 0 and ran[G.sweep_slot(16, 1024)] == ran[G.BAND_MW16] == ran[G.LDS_ATTR_SWEEP], describe(ran)
        assert ran[G.VPATH1] == 2 * seams and ran[G.LDS_ATTR_COMMIT] == 1, describe(ran)
    finally:
        reset_hooks(lib)


def test_a_16_bit_lift_of_a_16384_column_image_carves_the_8_bit_seams(oracle, lib):
    """coldepth_cases' lift identity at the widest frame: the 16I image v * 257 carves the seams of v, its pixels are the 8-bit
    result lifted the same way (the value-plane kernels: k_carve + k_emap_update<N, NT, true>, k_frozen_catchup<true>)"""
    c = G.BY_NAME["w16384x16_lift16"]
    eng = L.engine_coldepth_api()
    img, kw = G.image(c), G.run_kw(c)
    ref = G.reference(oracle, c)
    census(lib)
    e16 = L.Carver.from_ext(eng, img.astype(np.uint16) * 257)
    e16.configure(switch_freq=kw["switch_freq"])
    assert e16.resize(c["nw"], c["nh"]) == L.LQR_OK
    ran = census(lib)
    print("lift census: %s" % describe(ran))
    v = e16.vmap_dump()
    assert (v["depth"], v["orientation"]) == (ref["vmap"]["depth"], ref["vmap"]["orientation"]) and np.array_equal(v["data"], ref["vmap"]["data"])
    assert np.array_equal(e16.read_image_ext(), ref["image"].astype(np.uint16) * 257)
    assert ran[G.CARVE] == c["w"] - c["nw"] and ran[G.CARVE_E] == 0 and ran[G.TILE_P_G2] > 0, describe(ran)
    e16.destroy()


def test_a_frame_wider_than_16384_is_refused_on_the_host(oracle, engine, lib, capfd):
    """16385 columns: LQR_ERROR before anything is launched, the message names the limit, the carver still serves its image, and
    the next carver of 16384 columns is exact.  The same for a 16385-row image asked to lose rows, for 11000 columns asked to grow
    to 16500 (two steps at enl_step 1.5, the second from a flattened image of 16499 columns; to 16499, one step, it is carved:
    w11000_enlarge_one_step) and for a 16384-column carver enlarged to 16390 and then asked for 16380.  All of it is decided on
    the host: nothing is launched on a frame past the limit."""
    for name in cases("refused"):
        c = G.BY_NAME[name]
        img = G.image(c)
        cv, _ = H.init_carver(engine, img, c["nw"], c["nh"], **G.run_kw(c))
        census(lib)
        capfd.readouterr()
        assert cv.resize(c["nw"], c["nh"]) == L.LQR_ERROR, name
        assert "16384" in capfd.readouterr().err, name
        assert census(lib) == [0] * G.SLOTS, name
        g = cv.getters()
        assert (g["width"], g["height"], g["depth"]) == (c["w"], c["h"], 0), (name, g)
        assert np.array_equal(cv.read_image(), img), name
        cv.destroy()
    ok = G.BY_NAME["w16384x16_both_hor"]
    H.assert_same(G.reference(oracle, ok), H.run_case(engine, G.image(ok), ok["nw"], ok["nh"]), "16384 columns after a refusal")
    # enlarged past the limit: its next session would start from 16390 columns
    e = G.BY_NAME["w16384_enlarge"]
    img = G.image(e)
    ref = G.reference(oracle, e)
    cv, _ = H.init_carver(engine, img, e["nw"], e["nh"])
    assert cv.resize(e["nw"], e["nh"]) == L.LQR_OK
    census(lib)
    capfd.readouterr()
    assert cv.resize(16380, e["nh"]) == L.LQR_ERROR
    assert "16384" in capfd.readouterr().err
    assert census(lib) == [0] * G.SLOTS
    assert np.array_equal(cv.read_image(), ref["image"]) and cv.getters() == ref["getters"]
    cv.destroy()
    H.assert_same(G.reference(oracle, ok), H.run_case(engine, G.image(ok), ok["nw"], ok["nh"]), "16384 columns after the second refusal")
