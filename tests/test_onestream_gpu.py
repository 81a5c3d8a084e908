"""(-m gpu) A lock-step group that has its stream to itself, and the plane passes around its seam loop, against the oracle bit for bit:

  * slots per image of k_band_levels (lqr_plan.h, plan_levels_P): groups of 40 and 64 images on ONE stream with the automatic slot
    choice and with the choice pinned to 7 carve the oracle's seams; 320 x 96 is the smallest frame with three 32-row levels and five
    64-column tiles, so that a slot holds a second tile;
  * the start of a session on flat carvers is one pass (lqrhip_wk_init_emap: k_wk_init_emap lays the working planes out and builds
    the energy map): the energy plane after the first seam of a session, for every energy function, with and without a bias mask,
    for RGBA rows that take the 16-byte path (width a multiple of 4) and for those that do not (odd widths, 1 to 3 channels);
  * 1, 3 and 17 carvers through shrink, enlarge (k_inflate) and two more sessions on the same planes (the second pays the catch-up
    the first one owes, k_frozen_catchup), 131 x 67 (not a multiple of 4 or 64: one partial tile) and 260 x 70 (past 256 columns:
    a second chunk of the rank loops), with the energy read out after every step; a 16-bit lift through the same steps, a 64-bit
    float lift through two shrinking sessions and an enlargement.

The fused start adds no allocation and moves none (the same calls in the same order as lqrhip_wk_init + lqrhip_emap_build):
tests/test_oneoff_alloc_gpu.py's sweeps cover it as they are.
"""
import ctypes

import numpy as np
import pytest

import datasets as D
import energy_cases as EC
import geometry_cases as G
import harness as H
import lqr_ctypes as L

pytestmark = pytest.mark.gpu


@pytest.fixture()
def lib(engine):
    lb = engine.lib
    lb.lqrhip_launch_census.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int, ctypes.c_int]
    lb.lqrhip_launch_census.restype = ctypes.c_int
    lb.lqrhip_set_sub_batches.restype, lb.lqrhip_set_sub_batches.argtypes = None, [ctypes.c_int]
    lb.lqrhip_set_band_levels.argtypes = [ctypes.c_int]
    lb.lqrhip_debug_pool_live.restype, lb.lqrhip_debug_pool_live.argtypes = ctypes.c_ulonglong, []
    lb.lqrhip_pool_trim.restype, lb.lqrhip_pool_trim.argtypes = None, []
    yield lb
    lb.lqrhip_set_sub_batches(0); lb.lqrhip_set_band_levels(-1)


def census(lb):
    out = (ctypes.c_ulonglong * G.SLOTS)()
    assert lb.lqrhip_launch_census(out, G.SLOTS, 1) == G.SLOTS
    return [int(x) for x in out]


# ---- slots ------------------------------------------------------------------------------------------------------------------------
SLOT_W, SLOT_H, SLOT_SEAMS = 320, 96, 40
_slot_refs = {}


def slot_case(oracle, n):
    """image i of the slot groups and the oracle's resize of it: computed once (the group of 40 is the first 40 of the 64)"""
    for i in range(n):
        if i not in _slot_refs:
            im = D.photo_like(SLOT_W, SLOT_H, 700 + i) if i % 2 else D.noise(SLOT_W, SLOT_H, 700 + i)
            _slot_refs[i] = (im, H.run_case(oracle, im, SLOT_W - SLOT_SEAMS, SLOT_H))
    return [_slot_refs[i] for i in range(n)]


@pytest.mark.parametrize("n", [40, 64])
def test_a_group_alone_on_its_stream_carves_the_oracles_seams_with_the_automatic_slots_and_with_seven(oracle, engine, lib, n):
    refs = slot_case(oracle, n)
    lib.lqrhip_set_sub_batches(1)
    got = {}
    for slots in (-1, 7):
        lib.lqrhip_set_band_levels(slots)
        cs = [L.Carver(engine, im).configure() for im, _ in refs]
        census(lib)
        assert L.resize_batch(engine, cs, SLOT_W - SLOT_SEAMS, SLOT_H) == L.LQR_OK
        counts = census(lib)
        assert counts[G.BAND_LEVELS] > 0 and counts[G.BAND_TW] == 0 and counts[G.BAND_GENERIC] == 0, (slots, counts)
        got[slots] = [(c.vmap_dump()["data"], c.read_image()) for c in cs]
        for c in cs:
            c.destroy()
    for i, (_, ref) in enumerate(refs):
        for slots in (-1, 7):
            vmap, image = got[slots][i]
            assert np.array_equal(vmap, ref["vmap"]["data"]), "slots %d, image %d: seam map" % (slots, i)
            assert np.array_equal(image.reshape(ref["image"].shape), ref["image"]), "slots %d, image %d: pixels" % (slots, i)
        assert np.array_equal(got[-1][i][0], got[7][i][0]) and np.array_equal(got[-1][i][1], got[7][i][1]), i


# ---- the fused start of a session ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,ch", [(132, 37, 4), (131, 67, 4), (260, 9, 4), (3, 5, 4), (4, 1, 4), (67, 21, 3), (66, 20, 2), (65, 19, 1)],
                         ids=lambda v: str(v))
@pytest.mark.parametrize("nrg", range(7))
def test_the_energy_plane_of_a_session_started_in_one_pass_is_the_oracles(oracle, engine, nrg, w, h, ch):
    """one seam of a fresh carver: the energy plane afterwards is the map built at the start of the session but for the columns next to
    the seam; cumulative minima and back pointers follow from it"""
    img = D.photo_like(w, h, 800 + w + nrg, channels=ch)
    nw = w - 1
    try:
        oracle.lqrx_set_debug(1); engine.lqrx_set_debug(1)
        planes = []
        for api in (oracle, engine):
            c = L.Carver(api, img).configure(nrg_func=nrg)
            if w >= 60 and nrg % 2:
                assert c.bias_add(D.ellipse_mask(w, h), 700) == L.LQR_OK
            assert c.resize(nw, h) == L.LQR_OK
            planes.append(c.debug_snapshot())
            planes.append((c.vmap_dump()["data"], c.read_image()))
            c.destroy()
    finally:
        oracle.lqrx_set_debug(0); engine.lqrx_set_debug(0)
    (pa, oa, pb, ob) = planes
    assert np.array_equal(pa[0].view(np.int32), pb[0].view(np.int32)), "energies"
    assert np.array_equal(pa[1].view(np.int32), pb[1].view(np.int32)), "cumulative minima"
    assert np.array_equal(oa[0], ob[0]) and np.array_equal(oa[1], ob[1])


def test_the_energy_read_out_of_a_carver_resized_from_a_fused_start_is_the_oracles(oracle, engine):
    """lqr_carver_get_true_energy / lqr_carver_get_energy (lqr_energy.h) after a session that started in one pass"""
    img = D.photo_like(132, 40, 43)
    o = L.Carver(oracle, img).configure()
    assert o.resize(110, 40) == L.LQR_OK
    want = o.energy()
    o.destroy()
    c = L.Carver(L.bind_energy(engine), img).configure()
    assert c.resize(110, 40) == L.LQR_OK
    true = c.get_energy(0, true=True)
    assert np.array_equal(true.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(c.get_energy(0).view(np.uint32), EC.normalised(true).view(np.uint32))
    c.destroy()


# ---- the plane passes of a session ----------------------------------------------------------------------------------------------------
def session_steps(w, h):
    """shrink; enlarge past the original width (flatten, a session that ends in k_inflate); two sessions deeper than the enlarged
    image's map on the same planes, the second of which pays the catch-up the first owes; the other direction (transpose)"""
    return [(w - 24, h), (w + 30, h), (w - 10, h), (w - 20, h), (w - 20, h - 5)]


def observe(c, energy=True):
    o = dict(vmap=c.vmap_dump()["data"], image=c.read_image(), getters=c.getters())
    if energy:
        o["energy"] = c.energy()
    return o


def same(a, b, what):
    assert a["getters"] == b["getters"], (what, a["getters"], b["getters"])
    assert np.array_equal(a["vmap"], b["vmap"]), what + ": seam maps differ"
    assert np.array_equal(a["image"], b["image"]), what + ": images differ"
    assert np.array_equal(a["energy"].view(np.uint32), b["energy"].view(np.uint32)), what + ": energies differ"


_session_refs = {}


def session_case(oracle, w, h, i):
    """image i of a size and what the oracle shows after every step: computed once, shared by the groups of every length"""
    if (w, h, i) not in _session_refs:
        im = D.photo_like(w, h, 900 + i) if i % 3 else D.noise(w, h, 900 + i)
        c = L.Carver(oracle, im).configure()
        out = []
        for w1, h1 in session_steps(w, h):
            assert c.resize(w1, h1) == L.LQR_OK
            out.append(observe(c))
        c.destroy()
        _session_refs[(w, h, i)] = (im, out)
    return _session_refs[(w, h, i)]


@pytest.mark.parametrize("n", [1, 3, 17])
@pytest.mark.parametrize("w,h", [(131, 67), (260, 70)], ids=["131x67", "260x70"])
def test_shrink_enlarge_and_two_more_sessions_of_a_group(oracle, engine, lib, w, h, n):
    cases = [session_case(oracle, w, h, i) for i in range(n)]
    lib.lqrhip_pool_trim()
    live0 = int(lib.lqrhip_debug_pool_live())
    cs = [L.Carver(engine, im).configure() for im, _ in cases]
    for k, (w1, h1) in enumerate(session_steps(w, h)):
        assert L.resize_batch(engine, cs, w1, h1) == L.LQR_OK
        for i, c in enumerate(cs):
            same(cases[i][1][k], observe(c), "%d carvers, image %d, step %d" % (n, i, k))
    for c in cs:
        c.destroy()
    lib.lqrhip_pool_trim()
    assert int(lib.lqrhip_debug_pool_live()) == live0


def test_a_16_bit_lift_goes_through_the_same_sessions_as_the_8_bit_image(oracle, engine):
    """16I v * 257 reads the brightness the 8-bit image reads, and with colour values that are multiples of 4 (alpha 255) the pixels
    that inflate creates are lifts too for two generations of averaging -- floor((257 a + 257 b) / 2) = 257 (a + b) / 2 while a + b is
    even -- which is as far as these steps reveal them.  So the deep carver goes through every step of session_steps (the two-pass
    start on the value plane, k_inflate<true> at the end of every session, the enlargement that reveals its pixels, the flatten, the
    sessions after it of which the second pays the catch-up with k_frozen_catchup<true>, the transpose) and shows the oracle's seam
    maps and the lifted pixels after each"""
    w, h = 131, 67
    eng = L.bind_coldepth(engine)
    img = D.photo_like(w, h, 931)
    img[:, :, :3] &= 0xfc
    o = L.Carver(oracle, img).configure()
    c = L.Carver.from_ext(eng, img.astype(np.uint16) * 257).configure()
    for w1, h1 in session_steps(w, h):
        assert o.resize(w1, h1) == L.LQR_OK and c.resize(w1, h1) == L.LQR_OK
        assert np.array_equal(o.vmap_dump()["data"], c.vmap_dump()["data"]), (w1, h1)
        assert np.array_equal(c.read_image_ext(), o.read_image().astype(np.uint16) * 257), (w1, h1)
    o.destroy(); c.destroy()


def test_a_64_bit_float_lift_carves_the_8_bit_seams_and_is_enlarged_on_them(oracle, engine):
    """64F v / 255.0: two shrinking sessions (each ends in k_inflate<true>; the second pays the first one's catch-up) carve the
    oracle's seams and leave the lifted pixels; the enlargement that follows stays inside the map of those sessions and shows the
    oracle's seam map.  (A pixel that inflate creates is (a + b) * 0.5 in double, no lift of the 8-bit floor((a + b) / 2): the
    enlarged pixels are not compared, and a session on them would not carve the 8-bit seams.)"""
    w, h = 131, 67
    eng = L.bind_coldepth(engine)
    img = D.photo_like(w, h, 932)
    o = L.Carver(oracle, img).configure()
    c = L.Carver.from_ext(eng, img.astype(np.float64) / 255.0).configure()
    for w1, h1 in [(w - 24, h), (w - 40, h), (w + 30, h)]:
        assert o.resize(w1, h1) == L.LQR_OK and c.resize(w1, h1) == L.LQR_OK
        assert c.getters()["width"] == w1
        assert np.array_equal(o.vmap_dump()["data"], c.vmap_dump()["data"]), (w1, h1)
        if w1 < w:
            assert np.array_equal(c.read_image_ext().view(np.uint8), (o.read_image().astype(np.float64) / 255.0).view(np.uint8)), (w1, h1)
    o.destroy(); c.destroy()
