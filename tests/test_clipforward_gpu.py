"""Forward-energy seams for a clip (include_ext/lqr_clipforward.h) on the MI355X, against the numpy model of tests/clipforward_cases.py, bit
for bit: the map in every form (host, device, loaded and dumped again), for one frame the single-image build's own map, the images a
loaded map gives at every size (tests/vmap_cases.py's model applied to the model's map), lqrx_clip_resize_forward against the model's
composition, refusals, allocation failures, cancels, the launches a seam takes, and the seam loop's launch census around a build."""
import ctypes
import threading

import numpy as np
import pytest

import clipforward_cases as CC
import coldepth_cases as CD
import forward_cases as FC
import lqr_ctypes as L
import static_cases as SC
import vmap_cases as VC

pytestmark = pytest.mark.gpu
bits = CD.bits
CASES = dict(CC.cases())
K = CC.kernel_constants()
SLOTS = 32


@pytest.fixture(scope="module")
def eng():
    return L.bind_clipforward(L.bind_masks(L.bind_control(L.bind_imagetype(L.engine_api()))))


@pytest.fixture
def lib(eng):
    lb = eng.lib
    lb.lqrhip_debug_fail_alloc.argtypes = [ctypes.c_int]
    lb.lqrhip_debug_pool_live.restype, lb.lqrhip_debug_pool_live.argtypes = ctypes.c_ulonglong, []
    lb.lqrhip_launch_census.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int, ctypes.c_int]
    lb.lqrhip_launch_census.restype = ctypes.c_int
    yield lb
    lb.lqrhip_debug_fail_alloc(-1)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def shown(c):
    return c.scan_line_ext()[0]


def state(cs):
    return [(c.getters(), shown(c)) for c in cs]


def unchanged(cs, before):
    return all(g == b[0] and same(img, b[1]) for (g, img), b in zip(state(cs), before))


def flattened(cs, before):
    """what the header says of frames that were not flat when a build began: the same images at the same size, lying as they lay, but
    flat -- depth 0 -- whatever became of the build"""
    return all(same(shown(c), b[1]) and c.getters()["depth"] == 0 and
               all(c.getters()[k] == b[0][k] for k in ("width", "height", "orientation", "channels")) for c, b in zip(cs, before))


def build_frame(eng, spec, img, mask=None):
    """one frame of a spec, brought to the state the spec asks for (tests/test_forward_gpu.py's build)"""
    c = L.Carver.from_ext(eng, img, spec["depth"], init=spec["init"])
    if spec["type"] is not None:
        assert c.set_image_type(spec["type"]) == 1
    c.configure(nrg_func=spec["nrg"], res_order=spec.get("order", 0), switch_freq=2, enl_step=2.0)
    w, h = spec["w"], spec["h"]
    if spec["pre"] == "transposed":         # a flat carver that lies transposed
        assert c.resize(w, h - 2) == 1 and c.flatten() == 1 and c.getters()["orientation"] == 1
    elif spec["pre"] == "notflat":          # resized, in the direction of the map: it holds liblqr's levels and is not at full width
        assert c.resize(*((w, h - 3) if spec["o"] else (w - 3, h))) == 1
    if mask is not None:
        assert c.bias_add_f(mask, spec["bias"]) == 1
    return c


def build(eng, spec, imgs=None):
    imgs = CC.make_frames(spec) if imgs is None else imgs
    masks = CC.make_biases(spec)
    return [build_frame(eng, spec, img, None if masks is None else masks[t]) for t, img in enumerate(imgs)]


def model_of(cs, spec, d=None, o=None, temporal=None):
    """the model's map for what the frames show now"""
    st = FC.type_state(spec)
    Is = [FC.intensity(shown(c), spec["depth"], st, FC.is_luma(spec)) for c in cs]
    biases = [c.get_bias() for c in cs] if spec["bias"] else None
    return CC.clip_forward_map(Is, biases, spec["d"] if d is None else d, spec["o"] if o is None else o,
                               spec["temporal"] if temporal is None else temporal)


def same_map(m, want):
    return m is not None and m["depth"] == want["depth"] and m["orientation"] == want["orientation"] and \
        m["data"].dtype == np.int32 and np.array_equal(m["data"], want["data"])


def device_map(cs, d, o, temporal):
    import torch
    h, w = shown(cs[0]).shape[:2]
    t = torch.full((h, w), -7, dtype=torch.int32, device="cuda")
    ret = L.clip_forward_map_device(cs, t, d, o, temporal)
    return ret, t.cpu().numpy()


def destroy(cs):
    for c in cs:
        c.destroy()


# ---- 1. the map equals the model exactly ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_map_equals_the_model(eng, name):
    spec = CASES[name]
    cs = build(eng, spec)
    before = state(cs)
    want = model_of(cs, spec)
    got = L.clip_forward_map(cs, spec["d"], spec["o"], spec["temporal"])
    assert same_map(got, want), (name, np.argwhere(got["data"] != want["data"])[:8] if got else None)
    assert VC.valid_map(got, before[0][1].shape[1], before[0][1].shape[0])
    # the frames show what they showed, at the size they had, and lie as they lay; frames that were not flat have been flattened
    assert flattened(cs, before) if spec["pre"] == "notflat" else unchanged(cs, before)
    if name == "flat":
        assert np.array_equal(got["data"], np.tile(np.arange(1, spec["w"] + 1) % spec["w"], (spec["h"], 1)))       # always column 0
    if name == "bias_last":
        assert np.array_equal(got["data"][:, ::-1], np.tile(np.arange(1, spec["w"] + 1) % spec["w"], (spec["h"], 1)))   # always the last
    if name == "bias_last_v":
        assert np.array_equal(got["data"][::-1][:spec["d"]], np.tile(np.arange(1, spec["d"] + 1)[:, None], (1, spec["w"])))
    destroy(cs)


@pytest.mark.parametrize("name", ["L1025", "H65_v", "rgba_32f", "cmyk_8i", "bias_neg_v", "pre_transposed", "init_rgb", "luma_rgb"])
def test_for_one_frame_the_map_is_the_single_image_builds(eng, name):
    """engine against engine: lqrx_carver_forward_map_device of the same carver, for any temporal"""
    import torch
    spec = dict(CASES[name], n=1)
    cs = build(eng, spec)
    h, w = shown(cs[0]).shape[:2]
    t = torch.full((h, w), -7, dtype=torch.int32, device="cuda")
    assert cs[0].forward_map_device(t, spec["d"], spec["o"]) == 1
    ret, got = device_map(cs, spec["d"], spec["o"], 3.5)
    assert ret == 1 and np.array_equal(got, t.cpu().numpy())
    destroy(cs)


# ---- 2. consistency between forms, the load -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["L1025", "H65_v", "n%d" % (CC.GROUP + 1), "bias_one", "rgba_32f", "pre_transposed_v", "pre_notflat", "init_rgb"])
def test_host_form_equals_device_form_and_every_frames_dump_after_a_load(eng, name):
    spec = CASES[name]
    cs = build(eng, spec)
    imgs = [shown(c) for c in cs]
    h, w = imgs[0].shape[:2]
    want = model_of(cs, spec)
    ret, data = device_map(cs, spec["d"], spec["o"], spec["temporal"])
    assert ret == 1 and np.array_equal(data, want["data"]) and same_map(L.clip_forward_map(cs, spec["d"], spec["o"], spec["temporal"]), want)
    assert L.clip_load_forward(cs, spec["d"], spec["o"], spec["temporal"]) == 1
    for c, img in zip(cs, imgs):
        g = c.getters()
        assert (g["width"], g["height"], g["depth"], g["orientation"], g["enl_step"]) == (w, h, spec["d"], spec["o"], 2.0)
        assert same_map(c.vmap_dump(), want) and same(shown(c), img)
    destroy(cs)


@pytest.mark.parametrize("o", [0, 1])
@pytest.mark.parametrize("init", [False, True])
def test_a_loaded_map_serves_every_size_of_its_range_and_the_attached_carver_follows(eng, o, init):
    spec = dict(CASES["rgb_8i_float"], o=o, d=9, init=init, w=52, h=33, n=3)
    imgs = CC.make_frames(spec)
    aux_img = CD.base_image(np.random.default_rng(77), spec["w"], spec["h"], 3)
    cs = [L.Carver.from_ext(eng, img, 0, init=init) for img in imgs]
    auxs = [c.attach_ext(aux_img, 0) for c in cs]
    for c in cs:
        c.configure(nrg_func=2, res_order=0, switch_freq=2, enl_step=1.5)
    want = model_of(cs, spec)
    assert L.clip_load_forward(cs, spec["d"], o, spec["temporal"]) == 1
    L0 = spec["h"] if o else spec["w"]
    # every size of the range in one pass (lqrx_carver_read_sizes), as the numpy replay of the map gives it
    sizes = list(range(L0 - spec["d"], L0 + spec["d"] + 1))
    for c, img in zip(cs, imgs):
        assert same_map(c.vmap_dump(), want)
        assert c.size_range() == (o, sizes[0], sizes[-1])
        for s, out in zip(sizes, c.read_sizes(sizes)):
            assert same(out, VC.model(img, want, s)), (o, init, s)
    for k in (-4, -9, 9, 0, 5):
        size = (spec["w"], L0 + k) if o else (L0 + k, spec["h"])
        assert L.resize_batch(eng, cs, *size) == 1
        for c, aux, img in zip(cs, auxs, imgs):
            assert same(shown(c), VC.model(img, want, L0 + k)), (o, init, k)
            assert same(aux.scan_line_ext()[0], VC.model(aux_img, want, L0 + k)), (o, init, k)
    destroy(cs)


# ---- 3. resize_forward --------------------------------------------------------------------------------------------------------------
def composition(imgs, spec, w1, h1, order, temporal):
    """the model's lqrx_clip_resize_forward: per direction of the order, the model's map of what the frames show, applied to each"""
    st = FC.type_state(spec)
    for o in ((0, 1) if order == 0 else (1, 0)):
        h, w = imgs[0].shape[:2]
        change = (h1 - h) if o else (w1 - w)
        if change:
            m = CC.clip_forward_map([FC.intensity(img, spec["depth"], st, FC.is_luma(spec)) for img in imgs], None, abs(change), o, temporal)
            imgs = [VC.model(img, m, h1 if o else w1) for img in imgs]
    return imgs


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("to", [(-7, -5), (6, -4), (-3, 8), (5, 0), (0, -6), (0, 0)])
def test_resize_forward_equals_the_models_composition(eng, order, to):
    spec = dict(CASES["rgb_8i_float"], w=44, h=30, init=bool(order), n=3, order=order)
    imgs = CC.make_frames(spec)
    cs = [L.Carver.from_ext(eng, img, 0, init=spec["init"]) for img in imgs]
    for c in cs:
        c.configure(nrg_func=2, res_order=order, switch_freq=2, enl_step=1.5)
    w1, h1 = spec["w"] + to[0], spec["h"] + to[1]
    assert L.clip_resize_forward(cs, w1, h1, 0.7) == 1
    for c, want in zip(cs, composition(imgs, spec, w1, h1, order, 0.7)):
        assert same(shown(c), want), (order, to)
        assert (c.getters()["width"], c.getters()["height"]) == (w1, h1)
    destroy(cs)


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_images_sizes_and_depths_as_they_were(eng, capfd):
    import torch
    spec = dict(CASES["rgb_8i_float"], w=40, h=24, init=True, n=2)
    imgs = CC.make_frames(spec)
    cs = build(eng, spec, imgs)
    aux = cs[0].attach_ext(CD.base_image(np.random.default_rng(5), 40, 24, 3), 0)
    aux1 = cs[1].attach_ext(CD.base_image(np.random.default_rng(6), 40, 24, 3), 0)
    other = L.Carver.from_ext(eng, imgs[0], 0, init=True)
    other.configure(nrg_func=0, res_order=0, switch_freq=2, enl_step=2.0)        # another energy: not of the frames' configuration
    assert L.resize_batch(eng, cs, 36, 24) == 1                                   # (refusals must not flatten them either)
    before, aux_before = state(cs), aux.scan_line_ext()[0]
    eng.lqrhip_clipfwd_launches(1)
    capfd.readouterr()
    t = torch.zeros((24, 40), dtype=torch.int32, device="cuda")
    inf, nan = float("inf"), float("nan")
    calls = [
        lambda: L.clip_load_forward(cs, 0, 0, 1.0), lambda: L.clip_load_forward(cs, 36, 0, 1.0), lambda: L.clip_load_forward(cs, 24, 1, 1.0),
        lambda: L.clip_load_forward(cs, 3, 2, 1.0), lambda: L.clip_load_forward(cs, 3, -1, 1.0),
        lambda: L.clip_load_forward(cs, 3, 0, -0.5), lambda: L.clip_load_forward(cs, 3, 0, nan), lambda: L.clip_load_forward(cs, 3, 0, inf),
        lambda: L.clip_forward_map(cs, 36, 0, 1.0) is not None, lambda: L.clip_forward_map(cs, 3, 0, nan) is not None,
        lambda: L.clip_forward_map_device(cs, t, -1, 0, 1.0), lambda: eng.lqrx_clip_forward_map_device(L._b._frames(cs), 2, 3, 0, 1.0, None),
        lambda: L.clip_load_forward([cs[0], aux1], 3, 0, 1.0), lambda: L.clip_forward_map([aux], 3, 0, 1.0) is not None,
        lambda: L.clip_load_forward([cs[0], other], 3, 0, 1.0), lambda: L.clip_resize_forward([cs[0], other], 30, 24, 1.0),
        lambda: eng.lqrx_clip_load_forward(L._b._frames(cs), 0, 3, 0, 1.0), lambda: eng.lqrx_clip_load_forward(L._b._frames(cs), 65536, 3, 0, 1.0),
        lambda: eng.lqrx_clip_load_forward(None, 2, 3, 0, 1.0), lambda: eng.lqrx_clip_load_forward((ctypes.c_void_p * 2)(cs[0].p, None), 2, 3, 0, 1.0),
        lambda: L.clip_resize_forward(cs, 72, 24, 1.0), lambda: L.clip_resize_forward(cs, 36, 48, 1.0), lambda: L.clip_resize_forward(cs, 30, 0, 1.0),
        lambda: L.clip_resize_forward(cs, 0, 24, 1.0), lambda: L.clip_resize_forward(cs, 30, 48, 1.0), lambda: L.clip_resize_forward(cs, 30, 20, -1.0),
        lambda: L.clip_resize_forward([aux], 30, 24, 1.0),
    ]
    for i, call in enumerate(calls):
        assert call() == 0, i
        err = capfd.readouterr().err.strip().splitlines()
        assert len(err) == 1 and "refused" in err[0], (i, err)
        assert unchanged(cs, before) and same(aux.scan_line_ext()[0], aux_before), i
    assert eng.lqrhip_clipfwd_launches(0) == 0       # no device work
    assert L.clip_resize_forward(cs, 30, 20, 1.0) == 1 and all((c.getters()["width"], c.getters()["height"]) == (30, 20) for c in cs)
    destroy(cs)
    other.destroy()


def test_more_lines_than_a_build_takes_and_longer_lines_are_refused_up_front(eng, capfd):
    rng = np.random.default_rng(78)
    tall = [L.Carver.from_ext(eng, rng.integers(0, 4, (65536, 3, 1)).astype(np.uint8) * 85, 0, init=False) for _ in range(2)]
    wide = [L.Carver.from_ext(eng, rng.integers(0, 4, (2, 16385, 1)).astype(np.uint8) * 85, 0, init=False) for _ in range(2)]
    before = state(tall) + state(wide)
    eng.lqrhip_clipfwd_launches(1)
    capfd.readouterr()
    for i, call in enumerate([lambda: L.clip_forward_map(tall, 1, 0, 1.0) is not None, lambda: L.clip_load_forward(tall, 1, 0, 1.0),
                              lambda: L.clip_resize_forward(tall, 2, 65536, 1.0), lambda: L.clip_load_forward(wide, 1, 0, 1.0),
                              lambda: L.clip_resize_forward(wide, 16384, 2, 1.0)]):
        assert call() == 0, i
        err = capfd.readouterr().err.strip().splitlines()
        assert len(err) == 1 and "refused" in err[0], (i, err)
    assert unchanged(tall + wide, before) and eng.lqrhip_clipfwd_launches(0) == 0
    destroy(tall + wide)


# ---- 5. allocation failures ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["host", "device", "load"])
def test_every_allocation_of_a_build_fails_in_turn(eng, lib, form):
    """the nth device allocation of the call fails, once, for every n until the call gets through: each time LQR_NOMEM (NULL from the
    host form), the frames unchanged, the pool's live count where it was, and the same call then succeeds exactly.  (For the load form
    the count is taken around the frames' lives: their first load also makes their own batch, which they keep)"""
    spec = dict(CASES["bias_one"], init=True, n=3)
    live0 = lib.lqrhip_debug_pool_live()
    cs = build(eng, spec)
    imgs = [shown(c) for c in cs]
    w = imgs[0].shape[1]
    want = model_of(cs, spec)
    before, live = state(cs), lib.lqrhip_debug_pool_live()

    def call():
        if form == "host":
            return L.clip_forward_map(cs, spec["d"], spec["o"], spec["temporal"])
        if form == "device":
            return device_map(cs, spec["d"], spec["o"], spec["temporal"])
        return L.clip_load_forward(cs, spec["d"], spec["o"], spec["temporal"])
    failures = 0
    for n in range(64):
        lib.lqrhip_debug_fail_alloc(n)
        got = call()
        lib.lqrhip_debug_fail_alloc(-1)
        ok = same_map(got, want) if form == "host" else (got[0] == 1 and np.array_equal(got[1], want["data"])) if form == "device" else got == 1
        if ok:
            break
        failures += 1
        assert got is None if form == "host" else got[0] == L.LQR_NOMEM if form == "device" else got == L.LQR_NOMEM, (n, got)
        assert unchanged(cs, before), n
        if form != "load":
            assert lib.lqrhip_debug_pool_live() == live, n
    else:
        pytest.fail("the call never got through")
    # I of the frames, the costs, Pm, positions, choices, the seam, (the build's own map,) and the job table
    assert failures >= (8 if form != "device" else 7), failures
    if form == "load":
        assert L.resize_batch(eng, cs, w - spec["d"], spec["h"]) == 1
        assert all(same(shown(c), VC.model(img, want, w - spec["d"])) for c, img in zip(cs, imgs))
    else:
        assert unchanged(cs, before) and lib.lqrhip_debug_pool_live() == live
    destroy(cs)
    assert lib.lqrhip_debug_pool_live() == live0


# ---- 6. cancel ----------------------------------------------------------------------------------------------------------------------
def test_frames_cancelled_beforehand_refuse_every_call_unchanged(eng):
    import torch
    spec = dict(CASES["rgb_8i_float"], w=40, h=24, init=True, n=2)
    cs = [L.Carver.from_ext(eng, img, 0, init=True) for img in CC.make_frames(spec)]
    for c in cs:
        c.configure(nrg_func=2, res_order=0, switch_freq=2, enl_step=2.0, progress=True)
    cs[1].cancel_at_update(1, event="end")          # (a cancel that arrives when the resize has ended marks the carver and harms nothing)
    assert cs[0].resize(37, 24) == 1 and cs[1].resize(37, 24) == 1 and cs[0].cancelled() == 0 and cs[1].cancelled() == 1
    before = state(cs)
    eng.lqrhip_clipfwd_launches(1)
    t = torch.zeros((24, 37), dtype=torch.int32, device="cuda")
    assert L.clip_forward_map(cs, 4, 0, 1.0) is None and L.clip_forward_map_device(cs, t, 4, 0, 1.0) == L.LQR_USRCANCEL
    assert L.clip_load_forward(cs, 4, 0, 1.0) == L.LQR_USRCANCEL and L.clip_resize_forward(cs, 30, 20, 1.0) == L.LQR_USRCANCEL
    assert L.clip_resize_forward(cs, 37, 24, 1.0) == L.LQR_USRCANCEL           # (to the size they have)
    assert unchanged(cs, before) and eng.lqrhip_clipfwd_launches(0) == 0 and cs[1].cancelled() == 1
    assert cs[1].cancel_clear() == 1 and L.clip_load_forward(cs, 4, 0, 1.0) == 1 and all(c.getters()["depth"] == 4 for c in cs)
    destroy(cs)


@pytest.mark.parametrize("pre", [None, "notflat"])
def test_a_cancel_from_a_second_thread_during_a_build_is_honoured_between_slices(eng, pre):
    """depth 400: 25 slices.  The second thread waits until two slices have been enqueued, then cancels the LAST frame; the call returns
    LQR_USRCANCEL with the frames unchanged, well before the last slice.  Frames that were not flat are the header's one exception"""
    d = 400
    spec = dict(CASES["rgb_8i_float"], w=440, h=48, init=True, pre=pre, n=2)
    cs = build(eng, spec)
    before = state(cs)
    assert (before[0][0]["depth"] > 0) == (pre is not None)
    eng.lqrhip_clipfwd_launches(1)
    running, box = threading.Event(), {}
    once = 1 + 1                                    # the I planes, one group of the fold
    two_slices = once + 3 * 2 * K["FWD_SLICE_SEAMS"]

    def other_thread():
        running.set()
        while eng.lqrhip_clipfwd_launches(0) < two_slices and "ret" not in box:
            pass
        box["cancel"] = cs[-1].cancel()

    t = threading.Thread(target=other_thread)
    t.start()
    assert running.wait(60)
    try:
        box["ret"] = L.clip_load_forward(cs, d, 0, 1.0)
    finally:
        box.setdefault("ret", None)
        t.join(60)
    launches = eng.lqrhip_clipfwd_launches(0)
    assert box["ret"] == L.LQR_USRCANCEL and box["cancel"] == L.LQR_OK and cs[-1].cancelled() == 1, (box, launches)
    assert two_slices <= launches < once + 3 * d - 1
    assert flattened(cs, before) if pre else unchanged(cs, before)
    # ... and after the mark is cleared the same call builds the whole map
    assert cs[-1].cancel_clear() == 1 and L.clip_load_forward(cs, d, 0, 1.0) == 1 and all(c.getters()["depth"] == d for c in cs)
    st = FC.type_state(spec)
    want = CC.clip_forward_map([FC.intensity(b[1], 0, st, False) for b in before], None, d, 0, 1.0)
    assert all(same_map(c.vmap_dump(), want) for c in cs)
    destroy(cs)


# ---- 7. launches ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, CC.GROUP + 1])
def test_a_seam_takes_at_most_three_launches_whatever_the_number_of_frames(eng, n):
    spec = dict(CASES["n2"], n=n, d=21)
    cs = build(eng, spec)
    eng.lqrhip_clipfwd_launches(1)
    eng.lqrhip_forward_launches(1)
    assert same_map(L.clip_forward_map(cs, spec["d"], spec["o"], spec["temporal"]), model_of(cs, spec))
    launches = eng.lqrhip_clipfwd_launches(1)
    once = 1 + -(-n // K["CLIPFWD_GROUP"])          # the I planes of all frames in one launch, the fold one per group
    assert once < launches <= once + 3 * spec["d"] and eng.lqrhip_forward_launches(0) == 0
    destroy(cs)


def census(lb):
    out = (ctypes.c_ulonglong * SLOTS)()
    assert lb.lqrhip_launch_census(out, SLOTS, 1) == SLOTS
    return [int(x) for x in out]


def test_an_ordinary_resize_launches_and_gives_the_same_before_and_after_a_build(eng, lib):
    spec = dict(CASES["rgb_8i_float"], w=300, h=40, init=True, n=3)
    imgs = CC.make_frames(spec)

    def ordinary():
        c = L.Carver.from_ext(eng, imgs[0], 0, init=True)
        c.configure(nrg_func=2, res_order=0, switch_freq=2, enl_step=2.0)
        census(lib)
        assert c.resize(270, 34) == 1
        out = (census(lib), shown(c), c.vmap_dump()["data"])
        c.destroy()
        return out
    a = ordinary()
    cs = build(eng, spec, imgs)
    census(lib)
    assert L.clip_forward_map(cs, 25, 0, 1.0) is not None and L.clip_load_forward(cs, 25, 1, 1.0) == 1
    assert census(lib) == [0] * SLOTS                # a build and its load run none of the seam loop's kernels
    destroy(cs)
    b = ordinary()
    assert a[0] == b[0] and sum(a[0]) > 0 and same(a[1], b[1]) and np.array_equal(a[2], b[2])


# ---- 8. what it is for ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth,orientation,alone", [(20, 0, 80), (8, 1, 8)])
def test_the_clips_seams_leave_the_crossing_block_alone_where_frame_0s_own_do_not(eng, depth, orientation, alone):
    frames, union = SC.crossing_block()
    cs = [L.Carver.from_ext(eng, f, 0, init=False) for f in frames]
    for c in cs:
        c.configure(nrg_func=2, res_order=0, switch_freq=2, enl_step=2.0)
    m = L.clip_forward_map(cs, depth, orientation, 1.0)
    assert m is not None and CC.block_hits(m, union) == 0
    assert CC.block_hits(cs[0].forward_map(depth, orientation), union) == alone
    destroy(cs)
