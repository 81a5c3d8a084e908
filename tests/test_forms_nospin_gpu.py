"""Every form of the kernels a process runs once spinning is off (lqrhip_set_no_spin(1): after the first spin time-out on a shared
device, and in every redone session) on inputs the tie side decides: k_dp_tile<LR, RIG>, k_band_update_tw<4, LR, RIG>,
k_band_update_mw<2, 8 | 16, 8, LR, RIG>, k_band_update (lr, delta_x and the rigidity table are run-time values), k_dp_sweep as a full
sweep and as the update behind a band kernel, the one-wave backtracks k_vpath1<1..7> and k_vpath, and k_vp_maps / k_vp_solve<1..4>
-- against the oracle: seam map, pixels, getters, progress events and the energy / cumulative-minimum / back-pointer planes, bit for
bit, with the launch census equal to what tests/geometry_cases.py census() says must have run, slot by slot.

tests/test_forms_gpu.py does the same for the two spinning families.  The pixels are drawn from four grey levels and the side is
switched every third of the session (side switch frequency 4): photo-like and noise inputs have almost no equal minima, so on them a
wrong tie select, a rigidity term dropped at dx = +-delta_x or a launch of <false, RIG> for <true, RIG> carves valid seams and
passes.  A test that needs no GPU holds every input to it: the oracle's map with the side never switched differs.

The main shape, 520 x 70 losing 12 columns: three 192-column tiles of k_dp_tile in three 32-row launches; three 224-column slots of
k_band_update_tw and five of the 8-wave k_band_update_mw, so rows are handed over between slots; wider than k_band_update's
256-column window, so the window base moves; from delta_x 2 the band outgrows 248 - 2 delta_x columns within the 70 rows, so
k_dp_sweep<UPDATE> finishes rows.  The wide shape, 4210 x 24 losing 8, is the narrowest on which the 16-wave k_band_update_mw runs.
delta_x 0, 11 and 16 have no tiled instantiation: the generic kernels always.

Measured on one MI355X, oracle references included (computed once per shape, form and seed, and shared): the file alone 5.1 s for
106 GPU tests.  Per test: the first one 0.27 (it starts the device), test_group_of_8_forms_without_spinning 0.01 - 0.14 (delta_x 16 and
10 the slowest), test_multi_wave_band_forms on the wide shape 0.06 - 0.07, every other test 0.03 or less.  The 43 tests without a GPU
take 17 s on a machine without one (the planner test 3 s, every other 0.6 s or less).  The whole -m gpu suite at the parent commit on
the same machine, run just before it: 513.8 s for 1621 passed and 38 skipped; with this file, in one run on another machine, 520.6 s
for 1727 passed and 38 skipped.
"""
import numpy as np
import pytest

import datasets as D
import geometry_cases as G
import harness as H
import lqr_ctypes as L
from test_forms_gpu import assert_same, read_out
from test_geometry_gpu import census, describe, lib, reset_hooks, set_hooks  # noqa: F401  (lib is a fixture)

# seeds chosen on the CPU so that test_every_input_has_ties_the_side_decides holds for each with every form (at delta_x 0 seeds
# 1, 2, 3, 5, 9, 10, 13, 14, 17 and 36 of the main shape decide nothing)
SHAPES = dict(main=dict(w=520, h=70, seams=12, seeds=(4, 6, 7, 8, 11, 12, 15, 16)),
              wide=dict(w=4210, h=24, seams=8, seeds=(1, 2, 3, 4, 5, 6, 7, 8)))
RIGS = ("rig0", "rig10", "rig10_mask")
DELTAS = (0,) + tuple(range(1, 11)) + (11, 16)
FORMS = [(d, r) for d in DELTAS for r in RIGS]
PLAIN = [(1, "rig0"), (1, "rig10")]                                  # the forms the fast band kernels take
WIDE_FORMS = [(1, r) for r in RIGS]
GROUP_FORMS = [(d, r) for d in range(1, 11) for r in RIGS] + [(0, "rig0"), (16, "rig0")]
TILE_P_AND_LEVELS = (G.TILE_P_G3, G.TILE_P_G2, G.TILE_P_G4, G.TILE_P_GENERAL, G.BAND_LEVELS)


def image(shape, seed):
    """four grey levels, one channel: equal minima in every row"""
    s = SHAPES[shape]
    return (np.random.default_rng(seed).integers(0, 4, (s["h"], s["w"])) * 85).astype(np.uint8)


def case(shape, form, hooks=None, switch_freq=4):
    """the run as a case of geometry_cases.py: what census() and run_kw() take"""
    s, (delta, rig) = SHAPES[shape], form
    kw = dict(delta_x=delta, rigidity=0.0 if rig == "rig0" else 10.0, switch_freq=switch_freq)
    if rig == "rig10_mask":
        kw["rigmask"] = True
    return dict(name="%s delta_x %d %s" % (shape, delta, rig), w=s["w"], h=s["h"], nw=s["w"] - s["seams"], nh=s["h"], kind="planes", n=1,
                hooks=dict(hooks or {}), kw=kw)


_REF = {}


def reference(oracle, shape, form, seed, switch_freq=4):
    """the oracle's result, planes included, computed once per (shape, form, seed) and shared by every test of this file"""
    key = (shape, form, seed, switch_freq)
    if key not in _REF:
        c = case(shape, form, switch_freq=switch_freq)
        oracle.lqrx_set_debug(1)
        try:
            cv, _ = H.init_carver(oracle, image(shape, seed), c["nw"], c["nh"], **G.run_kw(c))
            _REF[key] = read_out(cv, cv.resize(c["nw"], c["nh"]))
            cv.destroy()
        finally:
            oracle.lqrx_set_debug(0)
        assert _REF[key]["ret"] == L.LQR_OK and _REF[key]["getters"]["width"] == c["nw"]
    return _REF[key]


@pytest.mark.parametrize("shape,delta,rig", [("main", d, r) for d, r in FORMS] + [("wide", d, r) for d, r in WIDE_FORMS])
def test_every_input_has_ties_the_side_decides(oracle, shape, delta, rig):
    """(no GPU) with the side never switched the oracle carves other seams: an input for which it did not would not test LR"""
    for seed in SHAPES[shape]["seeds"]:
        a, b = reference(oracle, shape, (delta, rig), seed, 0), reference(oracle, shape, (delta, rig), seed, 4)
        assert not np.array_equal(a["vmap"]["data"], b["vmap"]["data"]), "seed %d: the side decides no seam" % seed


def backtrack_hooks(delta):
    """the backtrack the planner does not choose by itself at this delta_x and size"""
    return dict(no_spin=1, vpath=0 if delta >= 5 else 1)


def test_the_planner_agrees_with_the_restated_census():
    """(no GPU) every exact census of this file is judged against geometry_cases.census(); tests/test_plan.py holds that restatement
    to csrc/lqr_plan.h for the cases of its own table, which have no delta_x 0, 11 or 16 without spinning: the same for the cases here"""
    import test_plan as P
    cs = [case("main", f, dict(no_spin=1)) for f in FORMS] + [case("main", f, dict(no_spin=1, update_mode=2)) for f in PLAIN]
    cs += [case("wide", f, dict(no_spin=1)) for f in PLAIN] + [case("main", (1, "rig0"))]
    cs += [case("main", (d, r), backtrack_hooks(d)) for d in range(1, 11) for r in RIGS]
    for c in cs:
        got, want = [int(x) for x in P.run_plan(P.plan_input(c)).split()], G.census(c)
        for slot in range(G.SLOTS):
            if slot != G.LDS_ATTR_COMMIT:           # k_vs_commit's LDS size: not a choice
                assert got[slot] == want[slot], (c["name"], c["hooks"], G.SLOT_NAMES.get(slot, slot), got[slot], want[slot])
    # what lqr_shim.hip launches at this size when left to itself: k_vpath1<1..4>, the parallel form at delta_x 5 .. 10, and k_vpath's
    # loop over the candidates wherever k_vpath1 has no instantiation -- delta_x 0 too
    want = {0: G.VPATH, 11: G.VPATH, 16: G.VPATH}
    want.update({d: G.VPATH1 for d in range(1, 5)})
    want.update({d: G.VP_PARALLEL for d in range(5, 11)})
    for d in DELTAS:
        ran = G.census(case("main", (d, "rig0"), dict(no_spin=1)))
        assert [s for s in (G.VP_PARALLEL, G.VPATH1, G.VPATH) if ran[s]] == [want[d]], (d, describe(ran))


def run_single(oracle, engine, lib, shape, form, hooks, seeds):
    """one image per seed under the hooks, each against its reference; returns the census of the last one, which must be the table's"""
    c = case(shape, form, hooks)
    want = G.census(c)
    refs = [reference(oracle, shape, form, seed) for seed in seeds]
    try:
        set_hooks(lib, c)
        engine.lqrx_set_debug(1)
        for seed, ref in zip(seeds, refs):
            cv, _ = H.init_carver(engine, image(shape, seed), c["nw"], c["nh"], **G.run_kw(c))
            census(lib)
            got = read_out(cv, cv.resize(c["nw"], c["nh"]))
            ran = census(lib)
            cv.destroy()
            print("%s seed %d census: %s" % (c["name"], seed, describe(ran)))
            assert_same(ref, got, "%s seed %d" % (c["name"], seed))
            assert ran == want, "%s ran [%s], the table says [%s]" % (c["name"], describe(ran), describe(want))
            assert not any(ran[s] for s in TILE_P_AND_LEVELS), describe(ran)
    finally:
        engine.lqrx_set_debug(0)
        reset_hooks(lib)
    return ran


@pytest.mark.gpu
@pytest.mark.parametrize("delta,rig", FORMS)
def test_single_image_forms_without_spinning(oracle, engine, lib, delta, rig):
    """delta_x 1 without a rigidity mask: k_dp_tile + k_band_update_tw + the sweep; every other form the full k_dp_sweep +
    k_band_update + the sweep"""
    s = SHAPES["main"]
    ran = run_single(oracle, engine, lib, "main", (delta, rig), dict(no_spin=1), s["seeds"][:1])
    if (delta, rig) in PLAIN:
        assert ran[G.DP_TILE] > 0 and ran[G.BAND_TW] > 0 and ran[G.SWEEP_FULL] == 0 and ran[G.BAND_GENERIC] == 0, describe(ran)
    else:
        assert ran[G.SWEEP_FULL] > 0 and ran[G.BAND_GENERIC] > 0 and ran[G.DP_TILE] == 0 and ran[G.BAND_TW] == 0, describe(ran)
    assert ran[G.SWEEP_UPDATE] > 0 and ran[G.BAND_MW8] == 0 and ran[G.BAND_MW16] == 0, describe(ran)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,slot", [("main", G.BAND_MW8), ("wide", G.BAND_MW16)])
@pytest.mark.parametrize("delta,rig", PLAIN)
def test_multi_wave_band_forms(oracle, engine, lib, delta, rig, shape, slot):
    """k_band_update_mw: 8 waves on request (update mode 2), 16 waves on its own past 4200 columns; every seed of the shape"""
    hooks = dict(no_spin=1, update_mode=2) if shape == "main" else dict(no_spin=1)
    ran = run_single(oracle, engine, lib, shape, (delta, rig), hooks, SHAPES[shape]["seeds"])
    assert ran[slot] > 0 and ran[G.DP_TILE] > 0 and ran[G.BAND_TW] == 0 and ran[G.BAND_GENERIC] == 0, describe(ran)
    assert ran[G.BAND_MW8 + G.BAND_MW16 - slot] == 0, describe(ran)


@pytest.mark.gpu
@pytest.mark.parametrize("delta,rig", [(d, r) for d in range(1, 11) for r in RIGS])
def test_backtrack_forms(oracle, engine, lib, delta, rig):
    """the backtrack the planner does not choose at this delta_x and size: delta_x 5 .. 10 on the one-wave walks (k_vpath1<5..7>,
    k_vpath at 8 .. 10), delta_x 1 .. 4 on k_vp_maps / k_vp_solve<1..4>; one launch (pair) per seam"""
    s = SHAPES["main"]
    ran = run_single(oracle, engine, lib, "main", (delta, rig), backtrack_hooks(delta), s["seeds"][:1])
    want = {G.VP_PARALLEL: 0, G.VPATH1: 0, G.VPATH: 0}
    want[G.VP_PARALLEL if delta <= 4 else G.VPATH1 if delta <= 7 else G.VPATH] = s["seams"]
    assert {x: ran[x] for x in want} == want, describe(ran)


@pytest.mark.gpu
@pytest.mark.parametrize("delta,rig", GROUP_FORMS)
def test_group_of_8_forms_without_spinning(oracle, engine, lib, delta, rig):
    """lqrx_carver_resize_batch on the eight seeds: k_carve and the separate energy update, one band workgroup per image"""
    form, s = (delta, rig), SHAPES["main"]
    c = case("main", form, dict(no_spin=1))
    refs = [reference(oracle, "main", form, seed) for seed in s["seeds"]]
    try:
        set_hooks(lib, c)
        engine.lqrx_set_debug(1)
        cs = [H.init_carver(engine, image("main", seed), c["nw"], c["nh"], **G.run_kw(c))[0] for seed in s["seeds"]]
        census(lib)
        ret = L.resize_batch(engine, cs, c["nw"], c["nh"])
        ran = census(lib)
        print("%s group census: %s" % (c["name"], describe(ran)))
        for seed, ref, cv in zip(s["seeds"], refs, cs):
            assert_same(ref, read_out(cv, ret), "%s seed %d" % (c["name"], seed))
        for cv in cs:
            cv.destroy()
        assert ran[G.BAND_TW if form in PLAIN else G.BAND_GENERIC] > 0 and ran[G.SWEEP_UPDATE] > 0, describe(ran)
        assert ran[G.BAND_GENERIC if form in PLAIN else G.BAND_TW] == 0 and ran[G.CARVE] > 0 and ran[G.CARVE_E] == 0, describe(ran)
        assert not any(ran[x] for x in TILE_P_AND_LEVELS), describe(ran)
    finally:
        engine.lqrx_set_debug(0)
        reset_hooks(lib)


@pytest.mark.gpu
def test_the_spinning_kernels_are_back_afterwards(oracle, engine, lib):
    """the last test of the file: no hook of it outlives its test -- a plain image runs k_dp_tile_p again"""
    assert lib.lqrhip_get_no_spin() == 0
    c = case("main", (1, "rig0"))
    seed = SHAPES["main"]["seeds"][0]
    census(lib)
    got = H.run_case(engine, image("main", seed), c["nw"], c["nh"], **G.run_kw(c))
    ran = census(lib)
    H.assert_same(reference(oracle, "main", (1, "rig0"), seed), got, "defaults")
    assert ran == G.census(c) and ran[G.TILE_P_G3] > 0 and ran[G.DP_TILE] == 0, describe(ran)
