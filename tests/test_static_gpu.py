"""Static seams for a clip (include_ext/lqr_static.h) on the MI355X, against the numpy model of tests/static_cases.py, bit for bit: the
folded energy plane in both forms for clips on and past the group boundary of k_static_fold, tiles on and past the tile boundary,
single lines, frames lying either way, every pixel kind; the map against the CPU oracle as the seam finder on the model's plane; the
loaded frames and the resize against twins that were given the same map through lqrx_vmap_load_batch; side effects, refusals, cancels
and allocation failures."""
import ctypes

import numpy as np
import pytest

import coldepth_cases as CD
import imgtype_cases as IT
import lqr_ctypes as L
import static_cases as SC

pytestmark = pytest.mark.gpu
bits = CD.bits
F = np.float32
SLOTS = 32
STATIC_FOLD = 31                # LQRHIP_CENSUS_STATIC_FOLD
W, H = 130, 67                  # three tiles by two, odd edges


@pytest.fixture(scope="module")
def eng():
    return L.bind_control(L.engine_static_api())


@pytest.fixture
def lib(eng):
    lb = eng.lib
    lb.lqrhip_debug_fail_alloc.argtypes = [ctypes.c_int]
    lb.lqrhip_debug_pool_live.restype, lb.lqrhip_debug_pool_live.argtypes = ctypes.c_ulonglong, []
    lb.lqrhip_launch_census.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int, ctypes.c_int]
    lb.lqrhip_launch_census.restype = ctypes.c_int
    yield lb
    lb.lqrhip_debug_fail_alloc(-1)


def census(lb):
    out = (ctypes.c_ulonglong * SLOTS)()
    assert lb.lqrhip_launch_census(out, SLOTS, 1) == SLOTS
    return [int(x) for x in out]


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def shown(c):
    return c.scan_line_ext()[0]


def state(c):
    return c.getters(), shown(c)


def unchanged(c, before):
    g, img = state(c)
    return g == before[0] and same(img, before[1])


def flattened(c, before):
    g = c.getters()
    return same(shown(c), before[1]) and g["depth"] == 0 and all(g[k] == before[0][k] for k in ("width", "height", "orientation", "channels"))


def spec_of(**kw):
    s = dict(n=3, w=W, h=H, ch=3, depth=0, nrg=0, type=None, max_ch=None, bias=False, pre=None, init=False, o=0, seed=1)
    s.update(kw)
    return s


def type_state(spec):
    st = IT.TypeState(spec["ch"])
    if spec["type"] is not None:
        assert st.apply(spec["type"]) == 1
    return st


def images(spec):
    """the clip: structured content that changes from frame to frame (another phase and noise per frame)"""
    out = []
    for t in range(spec["n"]):
        rng = np.random.default_rng([spec["seed"], t, spec["w"], spec["h"], spec["ch"]])
        out.append(CD.to_depth(rng, CD.base_image(rng, spec["w"], spec["h"], spec["ch"]), spec["depth"]))
    return out


def bias_of(spec, t, w, h):
    """float32 values, both signs: with bias_factor 2 the bias plane holds them exactly"""
    return np.random.default_rng([spec["seed"], 77, t]).uniform(-0.5, 2.0, (h, w)).astype(F)


def frame(eng, spec, img, t):
    prev = eng.lqrx_set_max_channels(spec["max_ch"]) if spec["max_ch"] else None
    try:
        c = L.Carver.from_ext(eng, img, spec["depth"], init=spec["init"])
    finally:
        if prev is not None:
            eng.lqrx_set_max_channels(prev)
    if spec["type"] is not None:
        assert c.set_image_type(spec["type"]) == 1
    c.configure(nrg_func=spec["nrg"], res_order=0, switch_freq=2, enl_step=2.0)
    w, h = spec["w"], spec["h"]
    if spec["pre"] == "transposed":         # resized in the other direction, flattened: a flat frame that lies transposed
        if not spec["init"]:
            assert c.init(1, 0.0) == 1
        assert c.resize(w, h - 2) == 1 and c.flatten() == 1 and c.getters()["orientation"] == 1
    elif spec["pre"] == "notflat":          # ... not flattened: the call flattens it, and it stays transposed
        if not spec["init"]:
            assert c.init(1, 0.0) == 1
        assert c.resize(w, h - 2) == 1 and c.getters()["orientation"] == 1 and c.getters()["depth"] == 2
    elif spec["pre"] == "notflat_same":     # resized in the direction of orientation 0
        if not spec["init"]:
            assert c.init(1, 0.0) == 1
        assert c.resize(w - 3, h) == 1 and c.getters()["depth"] == 3
    if spec["bias"]:
        g = c.getters()
        assert c.bias_add_f(bias_of(spec, t, g["width"], g["height"]).astype(np.float64), 2) == 1
    return c


def clip(eng, spec, imgs=None):
    imgs = images(spec) if imgs is None else imgs
    return [frame(eng, spec, img, t) for t, img in enumerate(imgs)]


def model_inputs(cs, spec):
    """what the frames show now, and their bias planes: the model's inputs"""
    return [shown(c) for c in cs], ([c.get_bias() for c in cs] if spec["bias"] else None)


def model(cs, spec, o, alpha):
    imgs, biases = model_inputs(cs, spec)
    return SC.static_energy(imgs, spec["depth"], type_state(spec), spec["nrg"], o, alpha, biases)


def destroy(cs):
    for c in cs:
        c.destroy()


def device_energy(cs, o, alpha):
    import torch
    g = cs[0].getters()
    t = torch.full((g["height"] * g["width"] + 16,), -7.0, dtype=torch.float32, device="cuda")
    ret = L.static_energy_device(cs, t, o, alpha)
    out = t.cpu().numpy()
    return ret, out[:-16].reshape(g["height"], g["width"]), out[-16:]


# ---- 1. the energy plane equals the model exactly -----------------------------------------------------------------------------------
ENERGY_CASES = {
    # the group boundary of the fold and past it
    "n1": spec_of(n=1), "n2": spec_of(n=2), "n16": spec_of(n=16), "n17": spec_of(n=17), "n33": spec_of(n=33), "n17_o1": spec_of(n=17, o=1),
    # the tile boundary, single lines
    "64x64": spec_of(w=64, h=64), "64x64_o1": spec_of(w=64, h=64, o=1), "65x1": spec_of(w=65, h=1), "65x1_o1": spec_of(w=65, h=1, o=1),
    "1x65": spec_of(w=1, h=65), "1x65_o1": spec_of(w=1, h=65, o=1),
    # frames lying the other way, flat and not
    "transposed_o0": spec_of(pre="transposed", o=0, bias=True), "transposed_o1": spec_of(pre="transposed", o=1, n=17),
    "notflat_o0": spec_of(pre="notflat", o=0), "notflat_o1": spec_of(pre="notflat", o=1, bias=True), "notflat_same_o0": spec_of(pre="notflat_same", o=0),
    "notflat_same_o1": spec_of(pre="notflat_same", o=1),
    # pixel kinds
    "grey": spec_of(ch=1, nrg=1), "rgba": spec_of(ch=4, nrg=2), "rgba_o1": spec_of(ch=4, nrg=2, o=1), "greya_luma": spec_of(ch=2, nrg=4),
    "16i": spec_of(ch=3, depth=1, nrg=1), "32f": spec_of(ch=4, depth=2, nrg=0, o=1), "64f": spec_of(ch=1, depth=3, nrg=2),
    "cmyk": spec_of(ch=4, type=IT.CMYK, nrg=0), "custom6": spec_of(ch=6, max_ch=6, nrg=1, o=1), "custom6_16i": spec_of(ch=6, max_ch=6, depth=1, nrg=0),
    # energies
    "luma_norm": spec_of(nrg=3), "luma_xabs_o1": spec_of(nrg=5, o=1), "null": spec_of(nrg=6), "null_bias": spec_of(nrg=6, bias=True, o=1),
    "xabs_o1": spec_of(nrg=2, o=1), "sumabs": spec_of(nrg=1),
    # bias, initialised frames
    "bias": spec_of(bias=True, n=17), "bias_o1_init": spec_of(bias=True, o=1, init=True),
}


@pytest.mark.parametrize("name", list(ENERGY_CASES))
def test_energy_equals_the_model_in_both_forms_and_leaves_the_frames_alone(eng, lib, name):
    spec = ENERGY_CASES[name]
    o = spec["o"]
    cs = clip(eng, spec)
    before = [state(c) for c in cs]
    live = lib.lqrhip_debug_pool_live()
    want = model(cs, spec, o, SC.PAPER_ALPHA)
    census(lib)
    ret, got, guard = L.static_energy(cs, o, SC.PAPER_ALPHA, guard=64)
    ran = census(lib)
    assert ret == 1 and same(got, want), (name, np.argwhere(bits(got) != bits(want))[:8])
    assert (guard == 0xa5).all()
    # one launch per 16 frames and nothing of the seam loop (a frame that was not flat is flattened first: that is no launch of the census)
    notflat = (spec["pre"] or "").startswith("notflat")
    assert ran[STATIC_FOLD] == -(-spec["n"] // SC.GROUP) and (notflat or sum(ran) == ran[STATIC_FOLD])
    ret, dev, dguard = device_energy(cs, o, SC.PAPER_ALPHA)
    assert ret == 1 and same(dev, got) and (dguard == -7.0).all()
    # the frames: untouched, lying as they lay; one that was not flat has been flattened and shows the same image
    for c, b in zip(cs, before):
        assert flattened(c, b) if notflat else unchanged(c, b)
    assert notflat or lib.lqrhip_debug_pool_live() == live          # (a flatten gives working planes back)
    # S alone is the largest of the engine's own true energies, T alone never negative, and both ends of alpha are the model's
    ret, s_only, _ = L.static_energy(cs, o, 1.0)
    assert ret == 1 and same(s_only, model(cs, spec, o, 1.0))
    ret, t_only, _ = L.static_energy(cs, o, 0.0)
    assert ret == 1 and same(t_only, model(cs, spec, o, 0.0)) and (t_only >= 0).all() and (spec["n"] > 1 or not t_only.any())
    imgs, biases = model_inputs(cs, spec)
    each = []
    for t, img in enumerate(imgs):
        twin = frame(eng, dict(spec, pre=None, bias=False, w=img.shape[1], h=img.shape[0]), img, t)
        if biases is not None:
            assert twin.bias_add_f(biases[t].astype(np.float64), 2) == 1
        each.append(twin.get_energy(o, true=True).copy())
        twin.destroy()
    assert same(s_only, np.max(each, axis=0))
    destroy(cs)


# ---- 2. the map is the oracle's on the model's plane --------------------------------------------------------------------------------
@pytest.mark.parametrize("o", (0, 1))
@pytest.mark.parametrize("delta,rigidity", [(1, 0.0), (2, 3.0)])
def test_map_equals_the_oracles_on_the_models_energy(eng, oracle, lib, o, delta, rigidity):
    spec = spec_of(n=5, nrg=3, bias=True, o=o)
    cs = clip(eng, spec)
    before = [state(c) for c in cs]
    live = lib.lqrhip_debug_pool_live()
    E = model(cs, spec, o, SC.PAPER_ALPHA)
    want = SC.key_map(oracle, L.OracleCarver, E, 40, o, delta, rigidity)
    got = L.static_map(cs, 40, o, SC.PAPER_ALPHA, delta, rigidity)
    assert got is not None and got["depth"] == 40 and got["orientation"] == o and got["data"].dtype == np.int32
    assert np.array_equal(got["data"], want["data"]), np.argwhere(got["data"] != want["data"])[:8]
    assert all(unchanged(c, b) for c, b in zip(cs, before)) and lib.lqrhip_debug_pool_live() == live
    destroy(cs)


# ---- 3. load and resize against twins given the same map -----------------------------------------------------------------------------
def observe(c):
    d, lo, hi = c.size_range()
    return c.getters(), (d, lo, hi), c.read_sizes(list(range(lo, hi + 1)))


def same_observation(a, b):
    return a[0] == b[0] and a[1] == b[1] and len(a[2]) == len(b[2]) and all(same(x, y) for x, y in zip(a[2], b[2]))


@pytest.mark.parametrize("o,init,pre", [(0, False, None), (1, False, None), (0, True, None), (1, False, "transposed"), (0, False, "notflat")])
def test_loaded_frames_equal_twins_loaded_through_vmap_load_batch(eng, o, init, pre):
    spec = spec_of(n=3, w=70, h=45, ch=4, nrg=2, init=init, pre=pre, o=o)
    cs = clip(eng, spec)
    imgs = [shown(c) for c in cs]
    m = L.static_map(cs, 12, o, SC.PAPER_ALPHA, 1, 0.0)
    assert m is not None
    assert L.load_static(cs, 12, o, SC.PAPER_ALPHA, 1, 0.0) == 1
    twins = clip(eng, dict(spec, pre=None, init=False, w=imgs[0].shape[1], h=imgs[0].shape[0]), imgs)
    assert L.vmap_load_batch(twins, m) == 1
    for c, t in zip(cs, twins):
        a, b = observe(c), observe(t)
        assert a[0]["depth"] == 12 and a[0]["orientation"] == o and a[1][0] == o
        assert same_observation(a, b)
        assert np.array_equal(c.vmap_dump()["data"], m["data"])
    destroy(cs + twins)


@pytest.mark.parametrize("w1,h1", [(58, 45), (70, 38), (61, 40), (79, 45), (70, 50)])
def test_resize_static_equals_the_twins_resized(eng, w1, h1):
    """shrinking and enlarging, one direction and both: per direction the map of |change| seams, then the batch resize"""
    spec = spec_of(n=3, w=70, h=45, ch=3, nrg=0, init=True)
    cs, twins = clip(eng, spec), clip(eng, dict(spec, init=False))
    assert L.resize_static(cs, w1, h1, SC.PAPER_ALPHA, 1, 0.0) == 1
    for o, change in ((0, abs(w1 - 70)), (1, abs(h1 - 45))):
        if not change:
            continue
        m = L.static_map(twins, change, o, SC.PAPER_ALPHA, 1, 0.0)
        assert m is not None and L.vmap_load_batch(twins, m) == 1
        g = twins[0].getters()
        assert L.resize_batch(eng, twins, *((g["width"], h1) if o else (w1, g["height"]))) == 1
    for c, t in zip(cs, twins):
        g = c.getters()
        assert (g["width"], g["height"]) == (w1, h1) and same(shown(c), shown(t))
    destroy(cs + twins)


# ---- 4. the seam loop beside it -----------------------------------------------------------------------------------------------------
def test_an_ordinary_resize_launches_and_gives_the_same_before_and_after_static_calls(eng, lib):
    img = images(spec_of(n=1, w=300, h=40))[0]

    def ordinary():
        c = L.Carver.from_ext(eng, img, 0, init=True)
        c.configure(nrg_func=2, res_order=0, switch_freq=2, enl_step=2.0)
        census(lib)
        assert c.resize(270, 34) == 1
        out = (census(lib), shown(c), c.vmap_dump()["data"])
        c.destroy()
        return out
    a = ordinary()
    cs = clip(eng, spec_of(n=18, w=300, h=40))
    assert L.static_energy(cs, 0, 0.3)[0] == 1 and L.load_static(cs, 25, 1, 0.3, 1, 0.0) == 1
    destroy(cs)
    b = ordinary()
    assert a[0] == b[0] and same(a[1], b[1]) and np.array_equal(a[2], b[2])


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------
def test_every_refusal_returns_error_and_leaves_the_frames_unchanged(eng, lib, capfd):
    spec = spec_of(n=2, w=40, h=24)
    cs = clip(eng, spec)
    odd = frame(eng, dict(spec, nrg=1), images(spec)[0], 0)                     # another energy function: not of one configuration
    aux = odd.attach_ext(images(spec)[1], 0)
    before = [state(c) for c in cs + [odd]]
    live = lib.lqrhip_debug_pool_live()
    census(lib)
    capfd.readouterr()
    E = L.LQR_ERROR

    def energy(frames, o=0, alpha=0.3):
        return L.static_energy(frames, o, alpha)[0]
    refused = [
        energy(cs, o=2), energy(cs, o=-1), energy(cs, alpha=-0.01), energy(cs, alpha=1.01), energy(cs, alpha=float("nan")),
        energy([cs[0], odd]), energy([cs[0], aux]), energy([aux]),
        L.load_static(cs, 0, 0, 0.3), L.load_static(cs, 40, 0, 0.3), L.load_static(cs, 24, 1, 0.3), L.load_static(cs, 3, 0, 0.3, delta_x=-1),
        L.load_static(cs, 3, 2, 0.3), L.load_static(cs, 3, 0, 1.5), L.load_static([cs[0], odd], 3, 0, 0.3),
        L.resize_static(cs, 0, 24, 0.3), L.resize_static(cs, 80, 24, 0.3), L.resize_static(cs, 40, 48, 0.3), L.resize_static(cs, 30, 20, 0.3, delta_x=-1),
        L.resize_static(cs, 30, 20, 2.0), L.load_static(cs, 3, 0, 0.3, delta_x=17), L.resize_static(cs, 30, 20, 0.3, delta_x=17),
    ]
    assert refused == [E] * len(refused), refused
    a = eng
    arr = (ctypes.c_void_p * 2)(cs[0].p, cs[1].p)
    assert a.lqrx_carvers_static_energy(arr, 0, 0, 0.3, None) == E and a.lqrx_carvers_static_energy(arr, 65536, 0, 0.3, None) == E
    assert a.lqrx_carvers_static_energy(arr, 2, 0, 0.3, None) == E and a.lqrx_carvers_static_energy_device(arr, 2, 0, 0.3, None) == E
    assert L.static_map(cs, 40, 0, 0.3) is None and L.static_map(cs, 3, 0, -1.0) is None and L.static_map([cs[0], aux], 3, 0, 0.3) is None
    lines = capfd.readouterr().err.strip().splitlines()
    assert len(lines) == len(refused) + 7 and all("refused" in ln for ln in lines), lines
    assert census(lib) == [0] * SLOTS and lib.lqrhip_debug_pool_live() == live          # before any device work
    assert all(unchanged(c, b) for c, b in zip(cs + [odd], before))
    destroy(cs + [odd])


@pytest.mark.parametrize("w,h,o", [(16385, 2, 0), (2, 16385, 1)])
def test_a_line_longer_than_the_widest_frame_is_refused_by_the_map_calls_and_served_by_the_energy_calls(eng, lib, capfd, w, h, o):
    """L = 16385 > LQRHIP_MAX_FRAME_WIDTH: the map, load and resize calls refuse it like every other refusal -- LQR_ERROR (NULL), one line
    on stderr, no launch, no block taken, the frames unchanged --; the energy calls have no limit on L and equal the model"""
    spec = spec_of(n=2, w=w, h=h, ch=1, nrg=1, o=o)
    cs = clip(eng, spec)
    before = [state(c) for c in cs]
    live = lib.lqrhip_debug_pool_live()
    census(lib)
    capfd.readouterr()
    assert L.static_map(cs, 3, o, 0.3) is None
    assert L.load_static(cs, 3, o, 0.3) == L.LQR_ERROR
    assert L.resize_static(cs, *((w, h - 3) if o else (w - 3, h)), 0.3) == L.LQR_ERROR
    assert L.resize_static(cs, *((w, h + 3) if o else (w + 3, h)), 0.3) == L.LQR_ERROR
    lines = capfd.readouterr().err.strip().splitlines()
    assert len(lines) == 4 and all("refused" in ln and "16384" in ln for ln in lines), lines
    assert census(lib) == [0] * SLOTS and lib.lqrhip_debug_pool_live() == live
    assert all(unchanged(c, b) for c, b in zip(cs, before))
    for oo in (0, 1):
        ret, got, guard = L.static_energy(cs, oo, SC.PAPER_ALPHA, guard=64)
        assert ret == 1 and same(got, model(cs, spec, oo, SC.PAPER_ALPHA)) and (guard == 0xa5).all(), oo
    ret, dev, dguard = device_energy(cs, o, SC.PAPER_ALPHA)
    assert ret == 1 and same(dev, model(cs, spec, o, SC.PAPER_ALPHA)) and (dguard == -7.0).all()
    assert all(unchanged(c, b) for c, b in zip(cs, before)) and lib.lqrhip_debug_pool_live() == live
    destroy(cs)


# ---- 6. cancel ----------------------------------------------------------------------------------------------------------------------
def test_a_frame_marked_cancelled_gives_usrcancel_and_nothing_changes(eng, lib):
    spec = spec_of(n=3, w=40, h=24, init=True)
    cs = clip(eng, spec)
    cs[1].set_progress_recorder()
    cs[1].cancel_at_update(1, event="end")          # the mark is set as its resize ends: every frame is 37 x 24 then, one is cancelled
    assert all(c.resize(37, 24) == 1 for c in cs) and [c.cancelled() for c in cs] == [0, 1, 0]
    before = [state(c) for c in cs]
    census(lib)
    U = L.LQR_USRCANCEL
    assert L.static_energy(cs, 0, 0.3)[0] == U and device_energy(cs, 0, 0.3)[0] == U and L.static_map(cs, 4, 0, 0.3) is None
    assert L.load_static(cs, 4, 0, 0.3) == U and L.resize_static(cs, 33, 24, 0.3) == U
    assert L.resize_static(cs, 37, 24, 0.3) == U            # ... also where neither direction has anything to do
    assert census(lib) == [0] * SLOTS and all(unchanged(c, b) for c, b in zip(cs, before))
    assert cs[1].cancel_clear() == 1 and L.load_static(cs, 4, 0, 0.3) == 1 and all(c.getters()["depth"] == 4 for c in cs)
    after = [state(c) for c in cs]
    assert L.resize_static(cs, 37, 24, 0.3) == 1 and all(unchanged(c, b) for c, b in zip(cs, after))       # nothing to do, nothing done
    destroy(cs)


def test_a_cancel_from_a_second_thread_around_the_key_carvers_resize_is_honoured_before_anything_is_loaded(eng, lib):
    """400 seams on 440 x 48: the key carver's resize is most of the call.  The second thread waits for the fold's launch and cancels
    frame 0: the mark is seen at the check point before the key carver's resize or, if that has begun, at the one after it (the resize
    itself is not interrupted).  LQR_USRCANCEL, the frames as they were, nothing loaded; once the mark is cleared the call goes through"""
    import threading
    spec = spec_of(n=2, w=440, h=48, init=True)
    cs = clip(eng, spec)
    before = [state(c) for c in cs]
    census(lib)
    running, box = threading.Event(), {}

    def folds():
        out = (ctypes.c_ulonglong * SLOTS)()
        lib.lqrhip_launch_census(out, SLOTS, 0)
        return int(out[STATIC_FOLD])

    def other_thread():
        running.set()
        while folds() < 1 and "ret" not in box:
            pass
        box["cancel"] = cs[0].cancel()

    t = threading.Thread(target=other_thread)
    t.start()
    assert running.wait(60)
    try:
        box["ret"] = L.load_static(cs, 400, 0, 0.3)
    finally:
        box.setdefault("ret", None)
        t.join(60)
    assert box["ret"] == L.LQR_USRCANCEL and box["cancel"] == L.LQR_OK and [c.cancelled() for c in cs] == [1, 0], box
    assert all(unchanged(c, b) for c, b in zip(cs, before))
    assert cs[0].cancel_clear() == 1 and L.load_static(cs, 400, 0, 0.3) == 1 and all(c.getters()["depth"] == 400 for c in cs)
    destroy(cs)


# ---- 7. allocation failures ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["host", "device", "map", "load"])
def test_every_allocation_of_a_call_fails_in_turn(eng, oracle, lib, form):
    """the nth device allocation of the call fails, once, for every n until the call gets through: each time LQR_NOMEM (NULL from the
    map form), the frames unchanged, the pool's live count where it was, and the same call then succeeds exactly.  17 frames: the fold
    has running planes.  (For the load form the count is taken around the frames' lives: the load makes batches the frames keep)"""
    spec = spec_of(n=17, w=48, h=20, bias=True, init=True)
    live0 = lib.lqrhip_debug_pool_live()
    cs = clip(eng, spec)
    E = model(cs, spec, 0, 0.3)
    want = SC.key_map(oracle, L.OracleCarver, E, 6, 0)
    before, live = [state(c) for c in cs], lib.lqrhip_debug_pool_live()

    def call():
        if form == "host":
            return L.static_energy(cs, 0, 0.3)[:2]
        if form == "device":
            return device_energy(cs, 0, 0.3)[:2]
        if form == "map":
            return L.static_map(cs, 6, 0, 0.3)
        return L.load_static(cs, 6, 0, 0.3)
    failures = 0
    for n in range(256):
        lib.lqrhip_debug_fail_alloc(n)
        got = call()
        lib.lqrhip_debug_fail_alloc(-1)
        if form in ("host", "device"):
            ok, nomem = got[0] == 1 and same(got[1], E), got[0] == L.LQR_NOMEM
        elif form == "map":
            ok, nomem = got is not None and np.array_equal(got["data"], want["data"]), got is None
        else:
            ok, nomem = got == 1, got == L.LQR_NOMEM
        if ok:
            break
        failures += 1
        assert nomem, (n, got)
        assert all(unchanged(c, b) for c, b in zip(cs, before)), n
        if form != "load":
            assert lib.lqrhip_debug_pool_live() == live, n
    else:
        pytest.fail("the call never got through")
    # the table of frames, S, T, I_prev, (E)
    assert failures >= (5 if form != "device" else 4), failures
    if form == "load":
        assert all(np.array_equal(c.vmap_dump()["data"], want["data"]) for c in cs)
    else:
        assert all(unchanged(c, b) for c, b in zip(cs, before)) and lib.lqrhip_debug_pool_live() == live
    destroy(cs)
    assert lib.lqrhip_debug_pool_live() == live0
