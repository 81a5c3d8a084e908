"""k_carve_v: the backtrack as a role of the carve's launch (csrc/k_carve.hip; lqrhip_set_backtrack_beside), against the launches it
replaces (k_vpath1, then k_carve_u) and against the oracle.

Every case carves the same inputs as a lock-step group with the knob at 1 and at 0 (the energy update beside the carve with both), as
sessions of 1, 2, .. seams, and compares what the seam loop left after the last seam of each -- the state after every seam -- bit for
bit: the seams (the visibility map), the energies, cumulative minima and back pointers read through the origin (lqrx_set_debug's
planes), the flags the backtrack published (origin, origin before the seam, side) and lqrhip_moved_bytes.  The longest session is then
compared with the oracle through the harness, planes included, and lqrhip_backtrack_beside_launches must say that the form ran: once
per seam step except the one that compacts the frozen planes, never with the knob at 0.

What can go wrong is decided by WHEN the walk knows the side -- the carve's entries of an image are held back until then -- and by how
the rows divide into the walk's 12-row chunks, the carve's row-quads and the energy role's 62-row blocks.  A column of strongly
negative bias pins the first seam of a session (tests/test_carve_beside_gpu.py); the seams after it are free.  Per group:
  * a seam along the left edge and one along the right edge: the side is decided at the argmin;
  * seams through the middle of the frame, columns (w - 1) // 2 and w // 2: the sign of 2 sum(x) - h (w - 1) is decided in the last
    rows only, and on an odd width -- where the two are one column and the sum ties -- with the last row;
  * seams that cross the middle diagonally, one column per row (two at delta_x 2): decided midway;
  * noise without a pin.
Heights 37 (three chunks of steps exactly, no multiple of 4), 62, 63 (the energy block's rows and one more), 125 and 260; widths 300
to 1101 (wide enough for the diagonal), even and odd; groups of 5 and 9; delta_x 1 and 2.  A session with a side switch carves both
halves' picks (leftmost, then rightmost of equal minima) and has a step whose carve moves the energies alone in front of a full DP; a
session of 133 seams on nine images crosses the frozen planes' catch-up.  lqrhip_band_levels_debug is left alone, no fault is
injected."""
import ctypes

import numpy as np
import pytest

import datasets as D
import geometry_cases as G
import harness as H
import lqr_ctypes as L
from test_carve_beside_gpu import PIN, column_mask, oracle_ref, same_state
from test_forms_gpu import assert_same, read_out
from test_geometry_gpu import census, describe

pytestmark = pytest.mark.gpu


@pytest.fixture()
def lib(engine):
    lb = engine.lib
    lb.lqrhip_launch_census.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int, ctypes.c_int]
    lb.lqrhip_launch_census.restype = ctypes.c_int
    lb.lqrhip_set_carve_beside.restype, lb.lqrhip_set_carve_beside.argtypes = None, [ctypes.c_int]
    lb.lqrhip_set_backtrack_beside.restype, lb.lqrhip_set_backtrack_beside.argtypes = None, [ctypes.c_int]
    lb.lqrhip_backtrack_beside_launches.restype, lb.lqrhip_backtrack_beside_launches.argtypes = ctypes.c_ulonglong, [ctypes.c_int]
    lb.lqrhip_carve_beside_launches.restype, lb.lqrhip_carve_beside_launches.argtypes = ctypes.c_ulonglong, [ctypes.c_int]
    lb.lqrhip_set_sub_batches.restype, lb.lqrhip_set_sub_batches.argtypes = None, [ctypes.c_int]
    lb.lqrhip_moved_bytes.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
    lb.lqrhip_debug_seam_flags.restype = ctypes.c_int
    lb.lqrhip_debug_seam_flags.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_int)] * 3
    lb.lqrhip_set_sub_batches(1)
    yield lb
    lb.lqrhip_set_backtrack_beside(-1); lb.lqrhip_set_carve_beside(-1); lb.lqrhip_set_sub_batches(0)
    engine.lqrx_set_debug(0)


def carve_group(api, lib, imgs, masks, nw, kw):
    """the images as one lock-step group down to nw columns: what the seam loop left, per image, flags and moved bytes included"""
    z = ctypes.c_ulonglong(0)
    assert lib.lqrhip_moved_bytes(ctypes.byref(z), 1) == 0
    cs = [H.init_carver(api, im, nw, im.shape[0], disc=mk, **kw)[0] for im, mk in zip(imgs, masks)]
    ret = L.resize_batch(api, cs, nw, imgs[0].shape[0])
    outs = [read_out(c, ret) for c in cs]
    for c, o in zip(cs, outs):
        f = [ctypes.c_int(-1) for _ in range(3)]
        assert lib.lqrhip_debug_seam_flags(c.p, *[ctypes.byref(x) for x in f]) == 0
        o["flags"] = tuple(x.value for x in f)          # (origin, origin before the last seam, its side)
    assert lib.lqrhip_moved_bytes(ctypes.byref(z), 1) == 0
    for c in cs:
        c.destroy()
    return outs, z.value


def pins(w, h, n, delta):
    """(column on row 0, columns per row) of the seam pinned in each of the n images; None: no pin"""
    mid_l, mid_r = (w - 1) // 2, w // 2
    diag = delta                                         # crosses the middle half way down
    p = [(2, 0), (w - 3, 0), (mid_l, 0), (mid_l - diag * (h // 2), diag), None]
    if n > 5:
        p += [(mid_r, 0), (mid_r + diag * (h // 2), -diag), (w // 4, 0), (mid_l - 500 if w > 1050 else 3 * w // 4, 0)]
    return p[:n]


def group(w, h, n, delta, seed):
    pp = pins(w, h, n, delta)
    imgs = [D.noise(w, h, seed + i) for i in range(n)]
    # (an image without a pin gets an empty mask: carvers with and without a bias plane do not form one lock-step group)
    masks = [np.zeros((h, w), np.uint8) if q is None else column_mask(w, h, q[0], q[1]) for q in pp]
    return imgs, masks, pp


def check(oracle, engine, lib, imgs, masks, seams, what, prefixes=None, pinned=None, **kw):
    w, h = imgs[0].shape[1], imgs[0].shape[0]
    lib.lqrhip_set_carve_beside(1)                       # (groups of 5: the automatic choice starts at 8)
    engine.lqrx_set_debug(1)
    last = None
    for k in prefixes or range(1, seams + 1):
        outs, moved = {}, {}
        for knob in (1, 0):
            lib.lqrhip_set_backtrack_beside(knob)
            lib.lqrhip_backtrack_beside_launches(1); lib.lqrhip_carve_beside_launches(1); census(lib)
            outs[knob], moved[knob] = carve_group(engine, lib, imgs, masks, w - k, kw)
            ran, walked, beside = census(lib), lib.lqrhip_backtrack_beside_launches(1), lib.lqrhip_carve_beside_launches(1)
            print("%s, %d seams, knob %d: %d launches with the walk inside, %d moved bytes; %s" % (what, k, knob, walked, moved[knob], describe(ran)))
            # the form runs on every step but the one that compacts the frozen planes (lag > 128: once, at seam 129)
            assert walked == ((k - (1 if k > 128 else 0)) if knob else 0), (what, k, knob, walked, describe(ran))
            assert beside == k, (what, k, knob, beside)                      # an energy-beside launch with either knob
            assert ran[G.VPATH1] == k and ran[G.CARVE] == k and ran[G.CARVE_E] == 0 and ran[G.VP_PARALLEL] == 0, describe(ran)
        assert moved[1] == moved[0], "%s after %d seams: moved bytes %d with the walk inside, %d without" % (what, k, moved[1], moved[0])
        for i, (a, b) in enumerate(zip(outs[0], outs[1])):
            same_state(a, b, "%s, image %d after %d seams" % (what, i, k))
            assert a["flags"] == b["flags"], "%s, image %d after %d seams: (origin, origin before, side) %s without, %s with the walk inside" % (what, i, k, a["flags"], b["flags"])
            if pinned is not None and pinned[i] is not None and k == 1:          # the one seam of the session lies where the bias pins it
                rows, at = np.nonzero(np.asarray(b["vmap"]["data"]).reshape(h, w))
                assert np.array_equal(rows, np.arange(h)) and np.array_equal(at, pinned[i][0] + pinned[i][1] * rows), (what, i, at)
                assert b["flags"][2] == (1 if 2 * int(at.sum()) < h * (w - 1) else 0), (what, i, b["flags"])
        last = outs[1]
    for i, (im, mk, got) in enumerate(zip(imgs, masks, last)):
        assert_same(oracle_ref(oracle, im, mk, got["getters"]["width"], kw), got, "%s, image %d against the oracle" % (what, i))


# (height, width, images): every height with an even and an odd width, a group of 5 and one of 9 between them
SHAPES = [(37, 300, 5), (37, 1101, 9), (62, 301, 9), (62, 640, 5), (63, 1100, 5), (63, 333, 9), (125, 301, 5), (125, 1100, 9), (260, 600, 9), (260, 701, 5)]


@pytest.mark.parametrize("delta", [1, 2])
@pytest.mark.parametrize("h,w,n", SHAPES)
def test_when_the_side_is_decided(oracle, engine, lib, h, w, n, delta):
    imgs, masks, pp = group(w, h, n, delta, 2000 + 7 * h + w)
    check(oracle, engine, lib, imgs, masks, 3, "%d x %d x %d, delta_x %d" % (n, w, h, delta), pinned=pp, delta_x=delta, disc_coeff=PIN)


@pytest.mark.parametrize("delta", [1, 2])
def test_across_a_side_switch(oracle, engine, lib, delta):
    """side switch frequency 2: the pick changes from the leftmost to the rightmost of equal minima half way through the session, and
    that seam's launch moves the energies only (a full DP follows it)"""
    imgs, masks, pp = group(400, 63, 5, delta, 3000)
    check(oracle, engine, lib, imgs, masks, 6, "side switch, delta_x %d" % delta, pinned=pp, delta_x=delta, disc_coeff=PIN, switch_freq=2)


def test_across_a_frozen_catchup(oracle, engine, lib):
    """133 seams on nine images: past the 128 the frozen planes of a group above 4 images may lag.  The step that compacts them keeps
    the separate launches (the pass reads that seam's log row between backtrack and carve); the steps around it run the form"""
    imgs = [D.photo_like(300, 40, 3100 + i) for i in range(9)]
    check(oracle, engine, lib, imgs, [None] * 9, 133, "frozen catch-up", prefixes=[128, 129, 133])
