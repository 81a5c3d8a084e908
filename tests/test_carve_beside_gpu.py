"""k_carve_u: the energy update as workgroups of the carve's launch (csrc/k_carve.hip; lqrhip_set_carve_beside), against the two
launches it replaces and against the oracle.

Every case carves the same inputs as a lock-step group with the knob at 0 (k_carve, then k_emap_update) and at 1 (k_carve_u), as
sessions of 1, 2, .. seams, and compares what the seam loop left after the last seam of each -- energies, cumulative minima, back
pointers (lqrx_set_debug's planes) and the seams themselves (the visibility map) -- bit for bit: the state after every seam.  The
longest session is then compared with the oracle through the harness, planes included, and lqrhip_carve_beside_launches must say
that the combined launch ran once per seam step that had a frame left to update (and never with the knob at 0).

The carve role leaves the energy interval of every row to the energy role and stores the elements around it one by one, so what can
go wrong is decided by where the seam lies against the 16-byte vectors, the 256-element chunks and the 1024-element groups of the
row, on either side.  A column of strongly negative bias pins the first seam of a session there whatever the image holds (the bias
is -500 per pixel, a gradient energy at most a few units); the seams after it are free.  Columns 0 .. 5, 254 .. 258, 1022 .. 1027
of a 1100-column frame move the left side (the origin advances), their mirror images the right side; 70 rows cross the energy role's
62-row block.  The other cases: frames 2 .. 9 wide and 1, 2, 3, 63 high; seams that drift by delta_x every row; each energy function;
grey, RGB and RGBA; no bias at all; a side switch (the carve moves the energy plane alone, a full DP follows); a session longer than
the frozen planes' lag (128 seams for groups above 4: the catch-up runs in front of the combined launch); groups of 5, 9 and 33
images and one split over two sub-batch streams; a session redone on the non-spinning kernels after an injected fault."""
import ctypes

import numpy as np
import pytest

import datasets as D
import geometry_cases as G
import harness as H
import lqr_ctypes as L
from test_forms_gpu import assert_same, read_out
from test_geometry_gpu import census, describe

pytestmark = pytest.mark.gpu

W, HEIGHT = 1100, 70
LEFT = (0, 1, 2, 3, 4, 5, 254, 255, 256, 257, 258, 1022, 1023, 1024, 1025, 1026, 1027)
COLUMNS = LEFT + tuple(W - 1 - c for c in LEFT)
PIN = 100000            # bias factor of the pinning column: -PIN / 2 per pixel, divided by the frame's width when it enters the energy


@pytest.fixture()
def lib(engine):
    lb = engine.lib
    lb.lqrhip_launch_census.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int, ctypes.c_int]
    lb.lqrhip_launch_census.restype = ctypes.c_int
    lb.lqrhip_set_carve_beside.restype, lb.lqrhip_set_carve_beside.argtypes = None, [ctypes.c_int]
    lb.lqrhip_carve_beside_launches.restype, lb.lqrhip_carve_beside_launches.argtypes = ctypes.c_ulonglong, [ctypes.c_int]
    lb.lqrhip_set_sub_batches.restype, lb.lqrhip_set_sub_batches.argtypes = None, [ctypes.c_int]
    lb.lqrhip_debug_inject.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int]
    lb.lqrhip_set_no_spin.argtypes = [ctypes.c_int]
    lb.lqrhip_fault_stats.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
    yield lb
    lb.lqrhip_set_carve_beside(-1); lb.lqrhip_set_sub_batches(0); lb.lqrhip_debug_inject(0, 0, 0); lb.lqrhip_set_no_spin(0)
    engine.lqrx_set_debug(0)


def column_mask(w, h, col, step=0):
    """255 on column col + step * y of row y: the seam a negative bias pins"""
    m = np.zeros((h, w), np.uint8)
    m[np.arange(h), col + step * np.arange(h)] = 255
    return m


def carve_group(api, imgs, masks, nw, kw):
    """the images as one lock-step group down to nw columns: what the seam loop left, per image"""
    cs = [H.init_carver(api, im, nw, im.shape[0], disc=mk, **kw)[0] for im, mk in zip(imgs, masks)]
    ret = L.resize_batch(api, cs, nw, imgs[0].shape[0])
    outs = [read_out(c, ret) for c in cs]
    for c in cs:
        c.destroy()
    return outs


def oracle_ref(oracle, im, mk, nw, kw):
    oracle.lqrx_set_debug(1)
    try:
        c, _ = H.init_carver(oracle, im, nw, im.shape[0], disc=mk, **kw)
        out = read_out(c, c.resize(nw, im.shape[0]))
        c.destroy()
    finally:
        oracle.lqrx_set_debug(0)
    return out


def same_state(a, b, what):
    assert a["ret"] == b["ret"], what
    (ea, ma, da), (eb, mb, db) = a["planes"], b["planes"]
    assert ea.shape == eb.shape, what
    bad = np.argwhere(ea.view(np.int32) != eb.view(np.int32))
    assert not len(bad), "%s: %d energies differ, first at (row, column) %s" % (what, len(bad), bad[0])
    assert np.array_equal(ma.view(np.int32), mb.view(np.int32)), what + ": cumulative minima"
    assert np.array_equal(da[1:], db[1:]), what + ": back pointers"
    assert np.array_equal(a["vmap"]["data"], b["vmap"]["data"]), what + ": seams"
    assert np.array_equal(a["image"], b["image"]), what + ": pixels"


def beside_steps(w, seams, sub_batches=1):
    """combined launches of one session: one per sub-batch and seam step that leaves a frame wider than one column"""
    return sub_batches * sum(1 for i in range(seams) if w - i - 1 > 1)


def check(oracle, engine, lib, imgs, masks, seams, what, prefixes=None, sub_batches=1, pinned=None, pinned_step=None, **kw):
    w = imgs[0].shape[1]
    pinned_step = pinned_step or [0] * len(imgs)
    masks = masks or [None] * len(imgs)
    lib.lqrhip_set_sub_batches(sub_batches)         # (pinned: a process with 8 hardware queues and more splits 32 images by itself)
    engine.lqrx_set_debug(1)
    last = None
    for k in prefixes or range(1, seams + 1):
        outs = {}
        for knob in (0, 1):
            lib.lqrhip_set_carve_beside(knob)
            lib.lqrhip_carve_beside_launches(1); census(lib)
            outs[knob] = carve_group(engine, imgs, masks, w - k, kw)
            ran, beside = census(lib), lib.lqrhip_carve_beside_launches(1)
            print("%s, %d seams, knob %d: %d combined launches; %s" % (what, k, knob, beside, describe(ran)))
            assert beside == (beside_steps(w, k, sub_batches) if knob else 0), (what, k, knob, beside, describe(ran))
            assert ran[G.CARVE] == k * sub_batches and ran[G.CARVE_E] == 0, describe(ran)      # counted as carves, with either knob
        for i, (a, b) in enumerate(zip(outs[0], outs[1])):
            same_state(a, b, "%s, image %d after %d seams" % (what, i, k))
            if pinned is not None and k == 1:        # the one seam of the session lies where the bias pins it
                rows, at = np.nonzero(np.asarray(b["vmap"]["data"]).reshape(imgs[i].shape[0], w))
                assert np.array_equal(rows, np.arange(imgs[i].shape[0])) and np.array_equal(at, pinned[i] + pinned_step[i] * rows), (what, i, at)
        last = outs[1]
    # (a frame carved down to one column has no DP left to update: the engine launches none, liblqr's finish_vsmap case, and the
    # planes it leaves are not the oracle's -- with either knob.  The result is compared there, the planes only between the knobs)
    against = assert_same if w - k > 1 else H.assert_same
    for i, (im, mk, got) in enumerate(zip(imgs, masks, last)):
        against(oracle_ref(oracle, im, mk, got["getters"]["width"], kw), got, "%s, image %d against the oracle" % (what, i))


@pytest.mark.parametrize("first", range(0, len(COLUMNS), 5))
def test_seam_position_against_the_vector_layout(oracle, engine, lib, first):
    """five images per group, each with its first seam pinned at another column of the list"""
    cols = [COLUMNS[(first + i) % len(COLUMNS)] for i in range(5)]
    imgs = [D.noise(W, HEIGHT, 500 + c) for c in cols]
    check(oracle, engine, lib, imgs, [column_mask(W, HEIGHT, c) for c in cols], 2, "columns %s" % (cols,), pinned=cols, disc_coeff=PIN)


@pytest.mark.parametrize("h", [1, 2, 3, 63])
def test_degenerate_frames(oracle, engine, lib, h):
    for w in range(2, 10):
        imgs = [D.noise(w, h, 600 + 10 * w + i) for i in range(5)]
        check(oracle, engine, lib, imgs, None, min(3, w - 1), "%d x %d" % (w, h), prefixes=[min(3, w - 1)])


@pytest.mark.parametrize("delta,step", [(1, 1), (2, 2), (1, 0)])
def test_seam_shape(oracle, engine, lib, delta, step):
    """a seam that drifts by delta_x columns every row, to the right in three images and to the left in two; a straight one"""
    starts = [3, 255, 600, W - 4, W - 257]
    steps = [step, step, step, -step, -step]
    imgs = [D.noise(W, HEIGHT, 700 + i) for i in range(5)]
    masks = [column_mask(W, HEIGHT, c, s) for c, s in zip(starts, steps)]
    check(oracle, engine, lib, imgs, masks, 3, "delta_x %d drifting by %d" % (delta, step), pinned=starts, pinned_step=steps, delta_x=delta, disc_coeff=PIN)


@pytest.mark.parametrize("nrg", range(7))
def test_each_energy_function(oracle, engine, lib, nrg):
    imgs = [D.photo_like(300, 70, 800 + i) for i in range(5)]
    check(oracle, engine, lib, imgs, None, 4, "energy function %d, no bias" % nrg, prefixes=[1, 4], nrg_func=nrg)


@pytest.mark.parametrize("channels", [1, 3, 4])
def test_pixel_layouts_and_a_bias_mask(oracle, engine, lib, channels):
    imgs = [D.photo_like(300, 70, 900 + i, channels=channels) for i in range(5)]
    masks = [D.band_mask(300, 70, 40 + 30 * i, 90 + 30 * i) for i in range(5)]
    check(oracle, engine, lib, imgs, masks, 4, "%d channels, a bias band" % channels, prefixes=[1, 4])


def test_across_a_side_switch(oracle, engine, lib):
    """side switch frequency 2: the side changes half way through the session -- that seam's carve moves the energies only"""
    imgs = [D.photo_like(300, 70, 1000 + i) for i in range(5)]
    check(oracle, engine, lib, imgs, None, 6, "side switch", switch_freq=2)


def test_across_a_frozen_catchup(oracle, engine, lib):
    """133 seams: past the 128 the frozen planes of a group above 4 images may lag, so a catch-up runs in front of a combined launch"""
    imgs = [D.photo_like(260, 40, 1100 + i) for i in range(5)]
    check(oracle, engine, lib, imgs, None, 133, "frozen catch-up", prefixes=[127, 128, 129, 133])


@pytest.mark.parametrize("n,sub", [(9, 1), (33, 1), (10, 2)])
def test_group_sizes_and_sub_batches(oracle, engine, lib, n, sub):
    imgs = [D.photo_like(260, 70, 1200 + i) if i % 2 else D.noise(260, 70, 1200 + i) for i in range(n)]
    check(oracle, engine, lib, imgs, None, 3, "%d images on %d streams" % (n, sub), prefixes=[3], sub_batches=sub)


def test_a_session_redone_after_a_fault_is_exact(oracle, engine, lib):
    """an error word written during seam step 2 (kind 1, as a spin time-out leaves it): the session is rolled back and carved again on
    the non-spinning kernels, with the combined launch"""
    imgs = [D.photo_like(260, 70, 1300 + i) for i in range(5)]
    st = (ctypes.c_ulonglong * 8)()
    lib.lqrhip_set_carve_beside(1); lib.lqrhip_set_sub_batches(1)
    lib.lqrhip_fault_stats(st, 1); lib.lqrhip_carve_beside_launches(1)
    lib.lqrhip_debug_inject(1, 2, 1)
    engine.lqrx_set_debug(1)
    outs = carve_group(engine, imgs, [None] * 5, 260 - 6, {})
    lib.lqrhip_fault_stats(st, 0)
    lib.lqrhip_set_no_spin(0)
    injected, rolled_back, redone = int(st[5]), int(st[4]), int(st[6])
    assert injected == 1 and rolled_back >= 1 and redone >= 1, list(st)
    assert lib.lqrhip_carve_beside_launches(1) >= 6 + 3
    for i, (im, got) in enumerate(zip(imgs, outs)):
        assert got["ret"] == L.LQR_OK
        assert_same(oracle_ref(oracle, im, None, 254, {}), got, "redone session, image %d" % i)
