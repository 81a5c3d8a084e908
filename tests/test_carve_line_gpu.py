"""Line-aligned groups in the carve (carve_row, csrc/k_carve.hip; lqrhip_set_carve_line), against the vector-aligned groups it had
and against the oracle.

Every case carves the same inputs as a lock-step group with the hook at 0 (a row's groups start / end on a 16-byte vector) and at 1 (on
a 32-element boundary, a 128-byte line of the float planes), as sessions of k seams, and compares what the seam loop left after the last
seam of each -- the seams (the visibility map), the energies, cumulative minima and back pointers (lqrx_set_debug's planes), the pixels,
the flags the backtrack published (origin, origin before the seam, side) and lqrhip_moved_bytes -- bit for bit.  The longest session is
then compared with the oracle through the harness, planes included.

Both roundings load and store the same vectors; what differs is which lanes of which group take them, so what can go wrong is decided
by where the job's first (side 0, the part right of the seam moves) or last (side 1, the part left of it moves and the origin advances)
position lies against the 32-element boundaries and the 1024-element groups counted from them:
  * frames narrower than one line (20, 31 and 33 columns): the rounded group reaches below the row's first / beyond its last vector;
  * a seam in column 0 and one in column w - 1: nothing moves on the side the rule picks;
  * moved parts of exactly 1024 - 32, 1024 and 1024 + 1 elements on either side (2200 columns; at 1100 columns, where the shorter side is
    at most 549 elements, the seams at 0, 31, 32 and 33 elements from either end of the row instead): with the rounding the part is one
    group or two depending on where it starts against the line;
  * sessions of 72 seams that all fall left of the middle (a band of strongly negative bias holds them there: -PIN / 2 per pixel), so
    that the origin advances past two 32-element boundaries, and sessions that all fall right of it: sessions of 1, 2, .. 72 seams.
Each as 1 image (k_carve_e), 5 images (k_carve, which has no such argument and keeps the vector's alignment: the comparison holds
trivially there; with lqrhip_set_carve_beside(1) k_carve_u) and 8 images (k_carve_v: the frames have at least 37 rows), at delta_x 1 and 2; a rigidity mask for the loops of its plane; a side switch for the steps that move the energies alone."""
import ctypes

import numpy as np
import pytest

import datasets as D
import geometry_cases as G
import harness as H
from test_backtrack_beside_gpu import carve_group
from test_carve_beside_gpu import PIN, column_mask, oracle_ref, same_state
from test_forms_gpu import assert_same
from test_geometry_gpu import census, describe

pytestmark = pytest.mark.gpu

# form -> (images, lqrhip_set_carve_beside)
FORMS = {"e": (1, -1), "plain": (5, -1), "u": (5, 1), "v": (8, -1)}


@pytest.fixture()
def lib(engine):
    lb = engine.lib
    lb.lqrhip_launch_census.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int, ctypes.c_int]
    lb.lqrhip_launch_census.restype = ctypes.c_int
    for f in ("lqrhip_set_carve_line", "lqrhip_set_carve_beside", "lqrhip_set_backtrack_beside", "lqrhip_set_sub_batches"):
        getattr(lb, f).restype, getattr(lb, f).argtypes = None, [ctypes.c_int]
    lb.lqrhip_backtrack_beside_launches.restype, lb.lqrhip_backtrack_beside_launches.argtypes = ctypes.c_ulonglong, [ctypes.c_int]
    lb.lqrhip_carve_beside_launches.restype, lb.lqrhip_carve_beside_launches.argtypes = ctypes.c_ulonglong, [ctypes.c_int]
    lb.lqrhip_moved_bytes.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
    lb.lqrhip_debug_seam_flags.restype = ctypes.c_int
    lb.lqrhip_debug_seam_flags.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_int)] * 3
    lb.lqrhip_set_sub_batches(1)
    yield lb
    lb.lqrhip_set_carve_line(-1); lb.lqrhip_set_carve_beside(-1); lb.lqrhip_set_backtrack_beside(-1); lb.lqrhip_set_sub_batches(0)
    engine.lqrx_set_debug(0)


def band(w, h, x0, x1):
    m = np.zeros((h, w), np.uint8)
    m[:, x0:x1] = 255
    return m


def check(oracle, engine, lib, form, imgs, masks, prefixes, what, sides=None, **kw):
    """both hooks after sessions of `prefixes` seams; sides: the side every seam of every session must have moved (None: any)"""
    w, h = imgs[0].shape[1], imgs[0].shape[0]
    n, beside = FORMS[form]
    assert len(imgs) == n
    lib.lqrhip_set_carve_beside(beside)
    engine.lqrx_set_debug(1)
    last = None
    for k in prefixes:
        outs, moved = {}, {}
        for hook in (0, 1):
            lib.lqrhip_set_carve_line(hook)
            lib.lqrhip_backtrack_beside_launches(1); lib.lqrhip_carve_beside_launches(1); census(lib)
            outs[hook], moved[hook] = carve_group(engine, lib, imgs, masks, w - k, kw)
            ran, walked, besides = census(lib), lib.lqrhip_backtrack_beside_launches(1), lib.lqrhip_carve_beside_launches(1)
            print("%s, form %s, %d seams, hook %d: %d moved bytes, %d launches with the walk inside, %d with the energy beside; %s" % (what, form, k, hook, moved[hook], walked, besides, describe(ran)))
            # the form under test ran (the frames stay wider than one column; no session here reaches the frozen planes' catch-up of groups above 4)
            if form == "e": assert ran[G.CARVE_E] == k and ran[G.CARVE] == 0, describe(ran)
            if form == "plain": assert ran[G.CARVE] == k and besides == 0, (describe(ran), besides)
            if form == "u": assert ran[G.CARVE] == k and besides == k and walked == 0, (describe(ran), besides, walked)
            if form == "v": assert ran[G.CARVE] == k and walked == k, (describe(ran), walked)
        assert moved[0] == moved[1], "%s after %d seams: moved bytes %d vector-aligned, %d line-aligned" % (what, k, moved[0], moved[1])
        for i, (a, b) in enumerate(zip(outs[0], outs[1])):
            same_state(a, b, "%s, image %d after %d seams" % (what, i, k))
            assert a["flags"] == b["flags"], "%s, image %d after %d seams: (origin, origin before, side) %s vector-aligned, %s line-aligned" % (what, i, k, a["flags"], b["flags"])
            if sides is not None:        # every seam so far moved that side: the origin has advanced by one per seam, or not at all
                assert b["flags"][0] == (k if sides[i] else 0) and b["flags"][2] == sides[i], (what, i, k, b["flags"])
        last = outs[1]
    for i, (im, mk, got) in enumerate(zip(imgs, masks, last)):
        assert_same(oracle_ref(oracle, im, mk, got["getters"]["width"], kw), got, "%s, image %d against the oracle" % (what, i))


def pinned_group(w, h, n, cols, seed):
    """n noise images, image i with its first seam pinned at column cols[i % len(cols)]"""
    cc = [cols[i % len(cols)] for i in range(n)]
    return [D.noise(w, h, seed + i) for i in range(n)], [column_mask(w, h, c) for c in cc], cc


@pytest.mark.parametrize("delta", [1, 2])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("w", [20, 31, 33])
def test_frames_narrower_than_a_line(oracle, engine, lib, w, form, delta):
    """the first seam in column 0, in column w - 1 and in between; then free seams on either side, the origin advancing"""
    h = 40
    imgs, masks, cc = pinned_group(w, h, FORMS[form][0], [0, w - 1, 3, w - 5, w // 2, 1, w - 2, 4], 7000 + w)
    check(oracle, engine, lib, form, imgs, masks, range(1, 9), "%d x %d pinned at %s" % (w, h, cc), delta_x=delta, disc_coeff=PIN, switch_freq=0)


@pytest.mark.parametrize("delta", [1, 2])
@pytest.mark.parametrize("form", list(FORMS))
def test_seams_at_the_ends_and_around_the_first_line(oracle, engine, lib, form, delta):
    w, h = 1100, 40
    cols = [0, w - 1, 31, w - 1 - 31, 32, w - 1 - 32, 33, w - 1 - 33]
    imgs, masks, cc = pinned_group(w, h, FORMS[form][0], cols if form != "e" else [0], 7100)
    check(oracle, engine, lib, form, imgs, masks, [1, 2, 3], "%d x %d pinned at %s" % (w, h, cc), delta_x=delta, disc_coeff=PIN, switch_freq=0)
    if form == "e":          # (one image per group: the last column too)
        imgs, masks, cc = pinned_group(w, h, 1, [w - 1], 7101)
        check(oracle, engine, lib, form, imgs, masks, [1, 2, 3], "%d x %d pinned at %s" % (w, h, cc), delta_x=delta, disc_coeff=PIN, switch_freq=0)


# side 1 moves the v elements left of the seam, side 0 the w - 1 - v right of it
MOVED = (1024 - 32, 1024, 1024 + 1)


@pytest.mark.parametrize("delta", [1, 2])
@pytest.mark.parametrize("form", list(FORMS))
def test_moved_parts_around_one_group(oracle, engine, lib, form, delta):
    w, h = 2200, 40
    cols = [m for m in MOVED] + [w - 1 - m for m in MOVED]
    n = FORMS[form][0]
    for first in ([0] if n >= 5 else range(len(cols))):      # (five and eight images hold all six; single images go one by one)
        imgs, masks, cc = pinned_group(w, h, n, cols[first:] + cols[:first], 7200 + first)
        check(oracle, engine, lib, form, imgs, masks, [1, 2] if n >= 5 else [1], "%d x %d pinned at %s" % (w, h, cc), delta_x=delta, disc_coeff=PIN, switch_freq=0)


@pytest.mark.parametrize("delta", [1, 2])
@pytest.mark.parametrize("form", list(FORMS))
def test_the_origin_advances_past_two_lines(oracle, engine, lib, form, delta):
    """72 seams inside a band of 100 columns of strongly negative bias: left of the middle in the even images (side 1: the origin ends at
    72, past physical 32 and 64), right of it in the odd ones (side 0)"""
    w, h, n = 1100, 40, FORMS[form][0]
    imgs = [D.noise(w, h, 7300 + i) for i in range(n)]
    sides = [1 - i % 2 for i in range(n)]
    masks = [band(w, h, 20, 120) if s else band(w, h, w - 120, w - 20) for s in sides]
    check(oracle, engine, lib, form, imgs, masks, range(1, 73), "%d x %d, a band on either side" % (w, h), sides=sides, delta_x=delta, disc_coeff=PIN, switch_freq=0)
    if form == "e":          # (one image per group: the right side too)
        check(oracle, engine, lib, form, [D.noise(w, h, 7350)], [band(w, h, w - 120, w - 20)], [1, 33, 72], "%d x %d, a band on the right" % (w, h), sides=[0], delta_x=delta, disc_coeff=PIN, switch_freq=0)


@pytest.mark.parametrize("form", ["plain", "v"])
def test_the_rigidity_plane(oracle, engine, lib, form):
    w, h, n = 1100, 40, FORMS[form][0]
    imgs, masks, cc = pinned_group(w, h, n, [0, w - 1, 33, w - 34, 500, 600, 31, w - 32], 7400)
    check(oracle, engine, lib, form, imgs, masks, [1, 2, 3, 4], "rigidity mask, pinned at %s" % (cc,), rigidity=6.0, rigmask=D.top_half_mask(w, h), disc_coeff=PIN, switch_freq=0)


@pytest.mark.parametrize("form", list(FORMS))
def test_across_a_side_switch(oracle, engine, lib, form):
    """side switch frequency 2: half way through the session a full DP follows a carve that moves the energies alone (move_dp 0)"""
    w, h, n = 300, 40, FORMS[form][0]
    imgs = [D.photo_like(w, h, 7500 + i) for i in range(n)]
    check(oracle, engine, lib, form, imgs, [None] * n, range(1, 7), "side switch", switch_freq=2)
