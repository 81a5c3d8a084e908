"""Every form of the two spinning kernel families at the smallest shape: k_dp_tile_p (one image) and k_band_levels (a group of 8)
for every (side, rigidity / rigidity mask, delta_x) their lists in csrc/lqr_kernels.h name, against the oracle -- seam map, pixels
and the energy / cumulative-minimum / back-pointer planes, bit for bit -- with the launch census showing that the family ran.

What a change of the launch shim's dispatch can break is routing a rarely used combination to another instantiation: the side
that wins a tie (LR), the rigidity table, a rigidity mask, the reach of delta_x.  So: 200 x 70 pixels losing 12 columns -- four
64-column tiles (seven of 32 columns for the plain forms), so halos are handed over in both directions; 70 rows are several blocks at
every delta_x -- with the side switched every third of the session (side switch frequency 4), so that each side is rebuilt with and
updated with.  The side only shows where minima are equal: the pixels are drawn from four grey levels, and a test that needs no GPU
holds every input to it -- the oracle's map with the side never switched differs from the one with it switched.
"""
import numpy as np
import pytest

import datasets as D
import geometry_cases as G
import harness as H
import lqr_ctypes as L
from test_geometry_gpu import census, describe, lib, reset_hooks, set_hooks  # noqa: F401  (lib is a fixture)

W, HEIGHT, SEAMS, GROUP = 200, 70, 12, 8
RIGS = ("rig0", "rig10", "rig10_mask")
FORMS = [(d, r) for d in range(1, 11) for r in RIGS]
LEVELS_HOOKS = dict(hooks=dict(update_mode=5, band_levels=7))       # as group8_*_levels of geometry_cases.py
# the seeds of the group's images, chosen on the CPU so that test_every_input_has_ties_the_side_decides holds for each with all 30 forms
SEEDS = (1, 2, 3, 4, 5, 6, 7, 8)


def image(i=0):
    """four grey levels, one channel: equal minima in every row"""
    return (np.random.default_rng(SEEDS[i]).integers(0, 4, (HEIGHT, W)) * 85).astype(np.uint8)


def run_kw(form, switch_freq=4):
    delta, rig = form
    kw = dict(delta_x=delta, rigidity=0.0 if rig == "rig0" else 10.0, switch_freq=switch_freq)
    if rig == "rig10_mask":
        kw["rigmask"] = D.top_half_mask(W, HEIGHT)
    return kw


def general(form):
    """launch_dp_persistent: delta_x above 1 and / or a rigidity mask that matters"""
    return form[0] != 1 or form[1] == "rig10_mask"


def read_out(cv, ret):
    """what harness.run_case reads out after its resize, and the planes the seam loop left (lqrx_set_debug)"""
    got = dict(ret=ret, getters=cv.getters(), aux=[], vmap=cv.vmap_dump(), events=list(cv.events), planes=cv.debug_snapshot())
    got["image"], got["nlines"] = cv.read_scanlines()
    return got


def assert_same(ref, got, what):
    H.assert_same(ref, got, what)
    (ea, ma, da), (eb, mb, db) = ref["planes"], got["planes"]
    assert np.array_equal(ea.view(np.int32), eb.view(np.int32)), what + ": energies"
    assert np.array_equal(ma.view(np.int32), mb.view(np.int32)), what + ": cumulative minima, first at %s" % (np.argwhere(ma.view(np.int32) != mb.view(np.int32))[:1],)
    assert np.array_equal(da[1:], db[1:]), what + ": back pointers"


_REF = {}


def reference(oracle, form, i=0, switch_freq=4):
    """the oracle's result for image i in this form, computed once and shared by the single-image and the group test"""
    key = (form, i, switch_freq)
    if key not in _REF:
        oracle.lqrx_set_debug(1)
        try:
            cv, _ = H.init_carver(oracle, image(i), W - SEAMS, HEIGHT, **run_kw(form, switch_freq))
            _REF[key] = read_out(cv, cv.resize(W - SEAMS, HEIGHT))
            cv.destroy()
        finally:
            oracle.lqrx_set_debug(0)
        assert _REF[key]["ret"] == L.LQR_OK and _REF[key]["getters"]["width"] == W - SEAMS
    return _REF[key]


@pytest.mark.parametrize("delta,rig", FORMS)
def test_every_input_has_ties_the_side_decides(oracle, delta, rig):
    """(no GPU) with the side never switched the oracle carves other seams: an input for which it did not would not test LR"""
    for i in range(GROUP):
        a, b = reference(oracle, (delta, rig), i, 0), reference(oracle, (delta, rig), i, 4)
        assert not np.array_equal(a["vmap"]["data"], b["vmap"]["data"]), "image %d: the side decides no seam" % i


@pytest.mark.gpu
@pytest.mark.parametrize("delta,rig", FORMS)
def test_dp_tile_p_forms(oracle, engine, lib, delta, rig):
    form = (delta, rig)
    ref = reference(oracle, form)
    try:
        engine.lqrx_set_debug(1)
        cv, _ = H.init_carver(engine, image(), W - SEAMS, HEIGHT, **run_kw(form))
        census(lib)
        got = read_out(cv, cv.resize(W - SEAMS, HEIGHT))
        ran = census(lib)
        cv.destroy()
        print("delta_x %d %s census: %s" % (delta, rig, describe(ran)))
        assert_same(ref, got, "delta_x %d %s" % form)
        assert ran[G.TILE_P_GENERAL if general(form) else G.TILE_P_G3] > 0, describe(ran)
        assert ran[G.DP_TILE] == 0 and ran[G.BAND_GENERIC] == 0, describe(ran)
    finally:
        engine.lqrx_set_debug(0)


@pytest.mark.gpu
@pytest.mark.parametrize("delta,rig", FORMS)
def test_band_levels_forms(oracle, engine, lib, delta, rig):
    form = (delta, rig)
    try:
        set_hooks(lib, LEVELS_HOOKS)
        engine.lqrx_set_debug(1)
        cs = [H.init_carver(engine, image(i), W - SEAMS, HEIGHT, **run_kw(form))[0] for i in range(GROUP)]
        census(lib)
        ret = L.resize_batch(engine, cs, W - SEAMS, HEIGHT)
        ran = census(lib)
        print("delta_x %d %s census: %s" % (delta, rig, describe(ran)))
        for i, cv in enumerate(cs):
            assert_same(reference(oracle, form, i), read_out(cv, ret), "delta_x %d %s image %d" % (delta, rig, i))
        for cv in cs:
            cv.destroy()
        assert ran[G.BAND_LEVELS] > 0, describe(ran)
    finally:
        engine.lqrx_set_debug(0)
        reset_hooks(lib)
