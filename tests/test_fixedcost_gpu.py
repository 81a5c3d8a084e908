"""(-m gpu) The fixed part of a batched resize, against the oracle bit for bit:

  * lqrx_carver_reload_device_batch resets a whole list with one k_reset_jobs launch per 16 carvers (lqrhip_carver_reset_batch): lists
    that cross the 16-job launch and the two-stream split, images with a tail past the last 16 bytes, an image smaller than one
    workgroup's reach, and sources that are not 16-byte aligned (the hipMemcpyAsync / hipMemsetAsync path);
  * the catch-up of the frozen planes at the end of a session is owed, not run (lqrhip_vs_commit): paid at the next lqrhip_emap_build
    -- the next session, an energy read-out -- dropped by a transpose, a reload, a roll-back; also for a group whose members owe
    different ranges;
  * sub-batch streams and descriptor blocks are parked between lqrx_carver_resize_batch calls and given back by lqrhip_pool_trim;
  * a group on two sub-batch streams through inflate, flatten and transpose with all of the above in place, and a failed level check
    in the second sub-batch still rolls the whole group back.
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
    lb.lqrhip_debug_inject.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int]
    lb.lqrhip_fault_stats.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
    lb.lqrhip_set_no_spin.argtypes = [ctypes.c_int]
    lb.lqrhip_debug_pool_live.restype, lb.lqrhip_debug_pool_live.argtypes = ctypes.c_ulonglong, []
    lb.lqrhip_launch_census.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int, ctypes.c_int]
    lb.lqrhip_launch_census.restype = ctypes.c_int
    lb.lqrhip_pool_trim.restype, lb.lqrhip_pool_trim.argtypes = None, []
    lb.lqrhip_set_sub_batches.restype, lb.lqrhip_set_sub_batches.argtypes = None, [ctypes.c_int]
    lb.lqrhip_debug_fixedcost.restype, lb.lqrhip_debug_fixedcost.argtypes = None, [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
    yield lb
    lb.lqrhip_debug_inject(0, 0, 0); lb.lqrhip_set_no_spin(0); lb.lqrhip_set_sub_batches(0)


def stats(lb, reset=False):
    st = (ctypes.c_ulonglong * 8)()
    assert lb.lqrhip_fault_stats(st, 1 if reset else 0) == 0
    return dict(zip(["timeouts", "predictions", "seamlog", "levels", "rolled_back", "injected", "redone", "_"], [int(x) for x in st]))


def fixedcost(lb):
    """lqrhip_debug_fixedcost, counters reset: streams parked now; since the last call streams reused, carvers reset by k_reset_jobs, by copy and fill"""
    out = (ctypes.c_ulonglong * 4)()
    lb.lqrhip_debug_fixedcost(out, 1)
    return dict(zip(["parked", "reused", "by_kernel", "by_copy"], [int(x) for x in out]))


def census(lb):
    out = (ctypes.c_ulonglong * G.SLOTS)()
    assert lb.lqrhip_launch_census(out, G.SLOTS, 1) == G.SLOTS
    return [int(x) for x in out]


def observe(c):
    return dict(vmap=c.vmap_dump()["data"], image=c.read_image(), getters=c.getters())


def same(a, b, what):
    assert a["getters"] == b["getters"], (what, a["getters"], b["getters"])
    assert np.array_equal(a["vmap"], b["vmap"]), what + ": seam maps differ"
    assert np.array_equal(a["image"], b["image"]), what + ": images differ"
    if "energy" in a:
        assert np.array_equal(a["energy"].view(np.uint32), b["energy"].view(np.uint32)), what + ": energies differ"


# ---- reload -------------------------------------------------------------------------------------------------------------------
def device_images(imgs, offset):
    """the images in one device buffer, each `offset` bytes past a 16-byte boundary: (the tensor that owns them, their addresses)"""
    import torch
    nbytes = imgs[0].size
    pitch = (nbytes + 15) // 16 * 16 + 16
    buf = torch.zeros(pitch * len(imgs) + 16, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    ptrs = []
    for i, im in enumerate(imgs):
        lo = i * pitch + offset
        buf[lo:lo + nbytes] = torch.from_numpy(np.ascontiguousarray(im).reshape(-1)).cuda()
        ptrs.append(buf.data_ptr() + lo)
    torch.cuda.synchronize()
    return buf, ptrs


RELOAD_SHAPES = [
    pytest.param(70, 33, 4, 60, 30, id="70x33-rgba-9240B-a-tail-of-8-bytes"),
    pytest.param(64, 16, 3, 56, 14, id="64x16-rgb-3072B-no-tail"),
    pytest.param(33, 7, 1, 29, 6, id="33x7-grey-231B-less-than-one-workgroup"),
]
_reload_refs = {}


def reload_ref(oracle, w, h, ch, nw, nh, i):
    """the oracle's resize of reload image i of a shape: computed once, shared by the lists of every length"""
    key = (w, h, ch, i)
    if key not in _reload_refs:
        im = D.noise(w, h, 2000 + i, channels=ch)
        _reload_refs[key] = (im, H.run_case(oracle, im, nw, nh))
    return _reload_refs[key]


@pytest.mark.parametrize("n,offset", [(1, 0), (3, 0), (17, 0), (34, 0), (17, 4)],
                         ids=["1", "3", "17-crosses-the-16-job-launch", "34-two-streams", "17-sources-4-bytes-off-alignment"])
@pytest.mark.parametrize("w,h,ch,nw,nh", RELOAD_SHAPES)
def test_reload_of_a_list_copies_every_image_clears_every_map_and_the_resize_is_exact(oracle, engine, lib, w, h, ch, nw, nh, n, offset):
    if n == 34:
        lib.lqrhip_set_sub_batches(2)
    first = [D.photo_like(w, h, 1900 + i, channels=ch) for i in range(n)]
    cs = [L.Carver(engine, im).configure() for im in first]
    if n == 3:          # masks and a resize before the reload: the reload drops both
        assert cs[0].bias_add(D.ellipse_mask(w, h), 500) == L.LQR_OK
        assert cs[0].rigmask_add(D.top_half_mask(w, h)) == L.LQR_OK
        assert cs[0].resize(w - 4, h - 1) == L.LQR_OK
        assert L.resize_batch(engine, cs[1:], w - 3, h) == L.LQR_OK
    else:               # every visibility map holds levels, up to its last bytes, before the reload clears it
        assert L.resize_batch(engine, cs, w - 3, h - 1) == L.LQR_OK
        assert all(c.vmap_dump()["data"].any() for c in cs)
    refs = [reload_ref(oracle, w, h, ch, nw, nh, i) for i in range(n)]
    buf, ptrs = device_images([r[0] for r in refs], offset)
    fixedcost(lib)
    assert L.reload_device_batch(engine, cs, ptrs) == L.LQR_OK
    f = fixedcost(lib)
    assert (f["by_kernel"], f["by_copy"]) == ((n, 0) if offset == 0 else (0, n)), f       # which way every image went
    for i, c in enumerate(cs):
        g = c.getters()
        assert (g["width"], g["height"], g["orientation"], g["depth"]) == (w, h, 0, 0), i
        assert np.array_equal(c.read_image().reshape(refs[i][0].shape), refs[i][0]), "image %d after the reload" % i
        assert not c.vmap_dump()["data"].any(), "visibility map %d after the reload" % i
    if n == 3:
        assert not cs[0].get_bias().any() and not cs[0].get_rigmask().any()
    assert L.resize_batch(engine, cs, nw, nh) == L.LQR_OK
    for i, c in enumerate(cs):
        ref = refs[i][1]
        assert np.array_equal(c.vmap_dump()["data"], ref["vmap"]["data"]), "seam map %d" % i
        assert np.array_equal(c.read_image().reshape(ref["image"].shape), ref["image"]), "image %d" % i
        c.destroy()
    del buf


# ---- the catch-up a session owes ------------------------------------------------------------------------------------------------
def steps_on(api, img, steps, energy=True):
    """one carver through `steps` ((w, h) each), observed after every step"""
    c = L.Carver(api, img).configure()
    out = []
    for w1, h1 in steps:
        assert c.resize(w1, h1) == L.LQR_OK
        o = observe(c)
        if energy:
            o["energy"] = c.energy()
        out.append(o)
    c.destroy()
    return out


def test_two_sessions_on_one_carver_across_the_lag_of_32(oracle, engine):
    """200 -> 160: the frozen planes are compacted in mid-session (a lag of 32 for up to four images) and the session ends owing seams
    33 .. 40; the energy read-out pays, and 160 -> 150 starts from paid planes"""
    img = D.photo_like(200, 40, 41)
    for i, (a, b) in enumerate(zip(steps_on(oracle, img, [(160, 40), (150, 40)]), steps_on(engine, img, [(160, 40), (150, 40)]))):
        same(a, b, "step %d" % i)


def test_two_sessions_without_a_read_out_in_between(oracle, engine):
    """... and with nothing between the sessions: the second session's lqrhip_emap_build pays"""
    img = D.photo_like(200, 40, 42)
    a, b = steps_on(oracle, img, [(160, 40), (150, 40)], energy=False), steps_on(engine, img, [(160, 40), (150, 40)], energy=False)
    same(a[1], b[1], "second session")


def test_two_sessions_of_a_group_of_five_across_the_lag_of_128(oracle, engine):
    w, h = 300, 24
    imgs = [D.photo_like(w, h, 50 + i) if i % 2 else D.noise(w, h, 50 + i) for i in range(5)]
    cs = [L.Carver(engine, im).configure() for im in imgs]
    refs = [steps_on(oracle, im, [(160, h), (150, h)]) for im in imgs]
    for k, w1 in enumerate((160, 150)):
        assert L.resize_batch(engine, cs, w1, h) == L.LQR_OK
        for i, c in enumerate(cs):
            o = observe(c)
            o["energy"] = c.energy()
            same(refs[i][k], o, "image %d, step %d" % (i, k))
    for c in cs:
        c.destroy()


def test_members_that_owe_different_ranges_are_paid_one_by_one(oracle, engine):
    """one carver carved alone (lag 32: it owes seams 33 .. 40) joins five carved together (lag 128: they owe 0 .. 40)"""
    w, h = 200, 24
    imgs = [D.photo_like(w, h, 70 + i) for i in range(6)]
    cs = [L.Carver(engine, im).configure() for im in imgs]
    assert cs[0].resize(160, h) == L.LQR_OK
    assert L.resize_batch(engine, cs[1:], 160, h) == L.LQR_OK
    assert L.resize_batch(engine, cs, 150, h) == L.LQR_OK
    for im, c in zip(imgs, cs):
        same(steps_on(oracle, im, [(160, h), (150, h)], energy=False)[1], observe(c), "mixed group")
        c.destroy()


def test_an_energy_read_out_after_a_resize_pays_the_debt(oracle, engine):
    """lqr_carver_get_energy on the carved frame, no second resize: the true energy is the oracle's, the normalised one its model"""
    img = D.photo_like(200, 40, 43)
    o = L.Carver(oracle, img).configure()
    assert o.resize(160, 40) == L.LQR_OK
    want = o.energy()
    o.destroy()
    c = L.Carver(L.bind_energy(engine), img).configure()
    assert c.resize(160, 40) == L.LQR_OK
    true = c.get_energy(0, true=True)
    assert np.array_equal(true.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(c.get_energy(0).view(np.uint32), EC.normalised(true).view(np.uint32))
    c.destroy()


def test_a_resize_in_the_other_direction_drops_the_debt(oracle, engine):
    img = D.photo_like(200, 40, 44)
    for i, (a, b) in enumerate(zip(steps_on(oracle, img, [(160, 40), (160, 31)]), steps_on(engine, img, [(160, 40), (160, 31)]))):
        same(a, b, "step %d" % i)


def test_a_fault_in_the_second_of_two_sessions_is_redone_exactly(oracle, engine, lib):
    img = D.photo_like(200, 40, 45)
    ref = steps_on(oracle, img, [(160, 40), (150, 40)])
    c = L.Carver(engine, img).configure()
    assert c.resize(160, 40) == L.LQR_OK
    stats(lib, reset=True)
    lib.lqrhip_debug_inject(1, 3, 1)                # a spin time-out in seam step 3 of the next session
    assert c.resize(150, 40) == L.LQR_OK
    s = stats(lib)
    lib.lqrhip_set_no_spin(0)
    assert s["injected"] == 1 and s["rolled_back"] >= 1 and s["redone"] >= 1, s
    o = observe(c)
    o["energy"] = c.energy()
    same(ref[1], o, "the redone second session")
    c.destroy()


# ---- parked streams ---------------------------------------------------------------------------------------------------------------
def test_streams_and_descriptor_blocks_are_parked_between_calls_and_given_back(oracle, engine, lib):
    w, h = 80, 24
    imgs = [D.photo_like(w, h, 90 + i) if i % 3 else D.noise(w, h, 90 + i) for i in range(34)]
    refs = [H.run_case(oracle, im, 70, 21) for im in imgs]
    lib.lqrhip_pool_trim()
    live0 = int(lib.lqrhip_debug_pool_live())
    lib.lqrhip_set_sub_batches(2)               # two streams for the 34 also where the process has too few hardware queues for the automatic split
    counts = []
    assert fixedcost(lib)["parked"] == 0
    for k, n in enumerate((5, 34, 5)):
        cs = [L.Carver(engine, im).configure() for im in imgs[:n]]
        census(lib)
        assert L.resize_batch(engine, cs, 70, 21) == L.LQR_OK
        counts.append(census(lib))
        f = fixedcost(lib)              # both sub-batches' streams are parked afterwards; from the second call on both were taken from there
        assert (f["parked"], f["reused"]) == (2, 2 if k else 0), (n, f)
        for i, c in enumerate(cs):
            assert np.array_equal(c.vmap_dump()["data"], refs[i]["vmap"]["data"]), (n, i)
            assert np.array_equal(c.read_image(), refs[i]["image"]), (n, i)
            c.destroy()
    assert counts[2] == counts[0]
    lib.lqrhip_pool_trim()
    assert int(lib.lqrhip_debug_pool_live()) == live0 and fixedcost(lib)["parked"] == 0


# ---- staged plane passes ----------------------------------------------------------------------------------------------------------
_staged = {}


def staged_case(oracle):
    if not _staged:
        w, h = 80, 24
        _staged["imgs"] = [D.photo_like(w, h, 130 + i) if i % 2 else D.noise(w, h, 130 + i) for i in range(34)]
        # 80 -> 130 is two enlargement sessions with a flatten in between (inflate, flatten); 130 x 24 -> 70 x 20 transposes
        _staged["refs"] = [steps_on(oracle, im, [(130, h), (70, 20)], energy=False) for im in _staged["imgs"]]
    return _staged["imgs"], _staged["refs"]


@pytest.mark.parametrize("inject", [False, True], ids=["plain", "level-cleared-in-the-second-sub-batch"])
def test_a_group_of_34_enlarged_in_two_steps_and_shrunk_in_both_directions(oracle, engine, lib, inject):
    imgs, refs = staged_case(oracle)
    cs = [L.Carver(engine, im).configure() for im in imgs]
    stats(lib, reset=True)
    lib.lqrhip_set_sub_batches(2)               # two sub-batches of 17, whatever the process's hardware queues
    if inject:
        lib.lqrhip_debug_inject(5, 1, 1)            # one committed level cleared, behind the second commit from now on
    for k, (w1, h1) in enumerate([(130, 24), (70, 20)]):
        assert L.resize_batch(engine, cs, w1, h1) == L.LQR_OK
        for i, c in enumerate(cs):
            same(refs[i][k], observe(c), "image %d, step %d" % (i, k))
    s = stats(lib)
    assert (s["injected"], s["levels"] >= 1, s["rolled_back"] >= 1) == ((1, True, True) if inject else (0, False, False)), s
    for c in cs:
        c.destroy()
