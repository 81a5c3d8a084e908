"""Forward-energy seam maps (include_ext/lqr_forward.h) on the MI355X, against the numpy model of tests/forward_cases.py, bit for bit:
the map in every form (host, device, batch, loaded and dumped again), the I plane the builder forms, the images a loaded map gives
(tests/vmap_cases.py's model applied to the model's map), lqrx_carver_resize_forward against the model's composition, refusals,
allocation failures, cancels, and the seam loop's launch census around a build."""
import ctypes
import threading

import numpy as np
import pytest

import coldepth_cases as CD
import forward_cases as FC
import lqr_ctypes as L
import vmap_cases as VC

pytestmark = pytest.mark.gpu
bits = CD.bits
CASES = dict(FC.cases())
K = FC.kernel_constants()
SLOTS = 32


@pytest.fixture(scope="module")
def eng():
    return L.bind_forward(L.bind_masks(L.bind_control(L.bind_imagetype(L.engine_api()))))


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


def state(c):
    return c.getters(), shown(c)


def unchanged(c, before):
    g, img = state(c)
    return g == before[0] and same(img, before[1])


def flattened(c, before):
    """what lqr_forward.h says of a carver that was not flat when a build began: the same image at the same size, lying as it lay,
    but flat -- depth 0 -- whatever became of the build"""
    g = c.getters()
    return same(shown(c), before[1]) and g["depth"] == 0 and all(g[k] == before[0][k] for k in ("width", "height", "orientation", "channels"))


def build(eng, spec, img=None):
    """the carver of a spec, brought to the state the spec asks for; what it shows now is what the map is of"""
    img = FC.make_image(spec) if img is None else img
    c = L.Carver.from_ext(eng, img, spec["depth"], init=spec["init"])
    if spec["type"] is not None:
        assert c.set_image_type(spec["type"]) == 1
    c.configure(nrg_func=spec["nrg"], res_order=0, switch_freq=2, enl_step=2.0)
    w, h = spec["w"], spec["h"]
    if spec["pre"] == "transposed":         # a flat carver that lies transposed
        assert c.resize(w, h - 2) == 1 and c.flatten() == 1 and c.getters()["orientation"] == 1
    elif spec["pre"] == "notflat":          # resized, in the direction of the map: it holds liblqr's levels and is not at full width
        assert c.resize(*((w, h - 3) if spec["o"] else (w - 3, h))) == 1
    if spec["bias"]:
        assert c.bias_add_f(FC.make_bias(spec), spec["bias"]) == 1
    return c


def model_of(c, spec, d=None, o=None):
    """(the model's map, the model's I in image orientation) for what carver c shows now"""
    img = shown(c)
    I = FC.intensity(img, spec["depth"], FC.type_state(spec), FC.is_luma(spec))
    bias = c.get_bias() if spec["bias"] else None
    return FC.forward_map(I, bias, spec["d"] if d is None else d, spec["o"] if o is None else o), I


def same_map(m, want):
    return m is not None and m["depth"] == want["depth"] and m["orientation"] == want["orientation"] and \
        m["data"].dtype == np.int32 and np.array_equal(m["data"], want["data"])


def device_map(c, d, o, h, w):
    import torch
    t = torch.full((h, w), -7, dtype=torch.int32, device="cuda")
    ret = c.forward_map_device(t, d, o)
    return ret, t.cpu().numpy()


# ---- 1. the map equals the model exactly ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_map_and_intensity_equal_the_model(eng, name):
    spec = CASES[name]
    c = build(eng, spec)
    before = state(c)
    want, I = model_of(c, spec)
    got = c.forward_map(spec["d"], spec["o"])
    assert same_map(got, want), (name, FC.boundaries(spec, K), np.argwhere(got["data"] != want["data"])[:8] if got else None)
    assert VC.valid_map(got, before[1].shape[1], before[1].shape[0])
    # the carver shows what it showed, at the size it had, and lies as it lay; one that was not flat has been flattened
    g = c.getters()
    assert same(shown(c), before[1]) and (g["width"], g["height"], g["orientation"]) == tuple(before[0][k] for k in ("width", "height", "orientation"))
    assert g["depth"] == (0 if spec["pre"] == "notflat" else before[0]["depth"])
    # the I plane the builder forms (the carver is flat now)
    assert same(c.forward_intensity(spec["o"]), np.ascontiguousarray(I.T if spec["o"] else I)), name
    c.destroy()


# ---- 2. consistency between forms -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["L65_v", "L1025", "H65_v", "rgba_32f", "cmyk_8i", "bias_neg_v", "pre_transposed", "pre_notflat_v", "init_rgb"])
def test_host_form_equals_device_form_and_the_dump_after_a_load(eng, name):
    spec = CASES[name]
    c = build(eng, spec)
    img = shown(c)
    h, w = img.shape[:2]
    want, _ = model_of(c, spec)
    ret, data = device_map(c, spec["d"], spec["o"], h, w)
    assert ret == 1 and np.array_equal(data, want["data"]) and same_map(c.forward_map(spec["d"], spec["o"]), want)
    assert c.load_forward(spec["d"], spec["o"]) == 1
    g = c.getters()
    assert (g["width"], g["height"], g["depth"], g["orientation"], g["enl_step"]) == (w, h, spec["d"], spec["o"], 2.0)
    assert same_map(c.vmap_dump(), want) and same(shown(c), img)
    c.destroy()


# ---- 3. loaded maps applied -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("o", [0, 1])
@pytest.mark.parametrize("init", [False, True])
def test_a_loaded_forward_map_serves_every_size_and_the_attached_carver_follows(eng, o, init):
    spec = dict(CASES["rgb_8i_float"], o=o, d=9, init=init, w=52, h=33)
    img = FC.make_image(spec)
    aux_img = CD.base_image(np.random.default_rng(77), spec["w"], spec["h"], 3)
    c = L.Carver.from_ext(eng, img, 0, init=init)
    aux = c.attach_ext(aux_img, 0)
    c.configure(nrg_func=2, res_order=0, switch_freq=2, enl_step=1.5)
    want, _ = model_of(c, spec)
    assert c.load_forward(spec["d"], o) == 1 and same_map(c.vmap_dump(), want)
    L0 = spec["h"] if o else spec["w"]
    for k in (-4, -9, 9, 0, 5, -9):
        size = (spec["w"], L0 + k) if o else (L0 + k, spec["h"])
        assert c.resize(*size) == 1
        assert same(shown(c), VC.model(img, want, L0 + k)), (o, init, k)
        assert same(aux.scan_line_ext()[0], VC.model(aux_img, want, L0 + k)), (o, init, k)
    c.destroy()


def test_an_initialised_carver_continues_beyond_a_forward_map_with_a_warm_start(eng):
    """lqr_vmap.h item 5, reached through load_forward: a resize below the map's range carves on with liblqr's seams on the frame the
    forward seams leave.  The reference is a second carver given the forward map's image at the end of its range"""
    spec = dict(CASES["rgb_8i_float"], o=0, d=6, init=True, w=48, h=20)
    img = FC.make_image(spec)
    c = build(eng, spec, img)
    want, _ = model_of(c, spec)
    assert c.load_forward(6, 0) == 1 and c.resize(38, 20) == 1 and c.getters()["depth"] == 10
    ref = L.Carver.from_ext(eng, VC.model(img, want, 42), 0, init=True)
    ref.configure(nrg_func=2, res_order=0, switch_freq=2, enl_step=2.0)
    assert ref.resize(38, 20) == 1
    assert same(shown(c), shown(ref))
    m = c.vmap_dump()["data"]
    assert np.array_equal(np.where(m <= 6, m, 0), want["data"]) and VC.valid_map(dict(data=m, depth=10, orientation=0), 48, 20)
    c.destroy()
    ref.destroy()


# ---- 4. resize_forward ------------------------------------------------------------------------------------------------------------
def composition(img, spec, w1, h1, order):
    """the model's lqrx_carver_resize_forward: per direction of the order, the model's map of what is shown, applied"""
    h, w = img.shape[:2]
    st = FC.type_state(spec)
    for o in ((0, 1) if order == 0 else (1, 0)):
        h, w = img.shape[:2]
        change = (h1 - h) if o else (w1 - w)
        if change:
            m = FC.forward_map(FC.intensity(img, spec["depth"], st, FC.is_luma(spec)), None, abs(change), o)
            img = VC.model(img, m, h1 if o else w1)
    return img


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("to", [(-7, -5), (6, -4), (-3, 8), (5, 0), (0, -6), (0, 0)])
def test_resize_forward_equals_the_models_composition(eng, order, to):
    spec = dict(CASES["rgb_8i_float"], w=44, h=30, init=bool(order))
    img = FC.make_image(spec)
    c = L.Carver.from_ext(eng, img, 0, init=spec["init"])
    c.configure(nrg_func=2, res_order=order, switch_freq=2, enl_step=1.5)
    w1, h1 = spec["w"] + to[0], spec["h"] + to[1]
    assert c.resize_forward(w1, h1) == 1
    assert same(shown(c), composition(img, spec, w1, h1, order)), (order, to)
    g = c.getters()
    assert (g["width"], g["height"]) == (w1, h1)
    c.destroy()


def test_every_refusal_leaves_image_size_and_depth_as_they_were(eng, capfd):
    spec = dict(CASES["rgb_8i_float"], w=40, h=24, init=True)
    img = FC.make_image(spec)
    c = build(eng, spec, img)
    aux = c.attach_ext(CD.base_image(np.random.default_rng(5), 40, 24, 3), 0)
    other = L.Carver.from_ext(eng, img, 0, init=True)
    other.configure(nrg_func=0, res_order=0, switch_freq=2, enl_step=2.0)        # another energy: not of c's configuration
    assert c.resize(36, 24) == 1                                                  # (refusals must not flatten it either)
    before, aux_before = state(c), aux.scan_line_ext()[0]
    eng.lqrhip_forward_launches(1)
    capfd.readouterr()
    import torch
    t = torch.zeros((24, 40), dtype=torch.int32, device="cuda")
    calls = [
        lambda: c.load_forward(0, 0), lambda: c.load_forward(36, 0), lambda: c.load_forward(24, 1), lambda: c.load_forward(3, 2),
        lambda: c.forward_map(36, 0) is not None, lambda: c.forward_map_device(t, -1, 0), lambda: aux.load_forward(3, 0),
        lambda: aux.forward_map(3, 0) is not None, lambda: L.forward_maps_device([c, other], [t, t], 3, 0),
        lambda: eng.lqrx_carver_forward_map_device(c.p, 3, 0, None),
        lambda: c.resize_forward(72, 24), lambda: c.resize_forward(36, 48), lambda: c.resize_forward(30, 0), lambda: c.resize_forward(0, 24),
        lambda: c.resize_forward(30, 48), lambda: aux.resize_forward(30, 24),
    ]
    for i, call in enumerate(calls):
        assert call() == 0, i
        err = capfd.readouterr().err.strip().splitlines()
        assert len(err) <= 1 and (i >= 12 or (len(err) == 1 and "refused" in err[0])), (i, err)
        assert unchanged(c, before) and same(aux.scan_line_ext()[0], aux_before), i
    assert eng.lqrhip_forward_launches(0) == 0       # no device work
    assert c.resize_forward(30, 20) == 1 and (c.getters()["width"], c.getters()["height"]) == (30, 20)
    c.destroy()
    other.destroy()


def test_more_lines_than_a_build_takes_are_refused_up_front_and_the_most_it_takes_are_built(eng, capfd):
    """LQRHIP_FORWARD_MAX_LINES = 65535 lines (the launch grids' second dimension): one more is refused before any device work, and
    65535 lines build a valid map"""
    rng = np.random.default_rng(77)
    tall = L.Carver.from_ext(eng, rng.integers(0, 4, (65536, 3, 1)).astype(np.uint8) * 85, 0, init=False)
    before = state(tall)
    eng.lqrhip_forward_launches(1)
    capfd.readouterr()
    for i, call in enumerate([lambda: tall.forward_map(1, 0) is not None, lambda: tall.load_forward(1, 0), lambda: tall.resize_forward(2, 65536),
                              lambda: tall.resize_forward(3, 65000)]):
        assert call() == 0, i
        err = capfd.readouterr().err.strip().splitlines()
        assert len(err) == 1 and "refused" in err[0], (i, err)
        assert unchanged(tall, before), i
    assert eng.lqrhip_forward_launches(0) == 0
    tall.destroy()
    most = L.Carver.from_ext(eng, rng.integers(0, 4, (65535, 3, 1)).astype(np.uint8) * 85, 0, init=False)
    got = most.forward_map(2, 0)
    assert got is not None and got["depth"] == 2 and got["orientation"] == 0 and FC.valid_levels(got["data"], 2)
    most.destroy()


# ---- 5. batches -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,o", [(3, 0), (17, 1), (17, 0)])
def test_batch_maps_equal_the_single_carver_maps_with_as_many_launches(eng, n, o):
    import torch
    spec = dict(CASES["rgb_8i_float"], w=61, h=19, o=o, d=11)
    imgs = [FC.make_image(dict(spec, seed=4000 + i, content="grey4" if i % 3 == 0 else "float")) for i in range(n)]
    cs = [build(eng, spec, img) for img in imgs]
    ts = [torch.full((spec["h"], spec["w"]), -7, dtype=torch.int32, device="cuda") for _ in range(n)]
    eng.lqrhip_forward_launches(1)
    assert L.forward_maps_device(cs, ts, spec["d"], o) == 1
    batch_launches = eng.lqrhip_forward_launches(1)
    for i, c in enumerate(cs):
        want, _ = model_of(c, spec)
        assert np.array_equal(ts[i].cpu().numpy(), want["data"]), i
    single = build(eng, spec, imgs[0])
    assert same_map(single.forward_map(spec["d"], o), model_of(single, spec)[0])
    # the one-off pass and two launches per seam, whatever n is
    assert eng.lqrhip_forward_launches(1) == batch_launches == 1 + 2 * spec["d"]
    for c in cs + [single]:
        c.destroy()


# ---- 6. allocation failures -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["host", "device", "load"])
def test_every_allocation_of_a_build_fails_in_turn(eng, lib, form):
    """the nth device allocation of the call fails, once, for every n until the call gets through: each time LQR_NOMEM (NULL from the
    host form), the carver unchanged, the pool's live count where it was, and the same call then succeeds exactly.  (For the load form
    the count is taken around the carver's life: its first load also makes the carver's own batch, which it keeps)"""
    spec = dict(CASES["bias_pos"], init=True)
    live0 = lib.lqrhip_debug_pool_live()
    c = build(eng, spec)
    img = shown(c)
    h, w = img.shape[:2]
    want, _ = model_of(c, spec)
    before, live = state(c), lib.lqrhip_debug_pool_live()

    def call():
        if form == "host":
            return c.forward_map(spec["d"], spec["o"])
        if form == "device":
            return device_map(c, spec["d"], spec["o"], h, w)
        return c.load_forward(spec["d"], spec["o"])
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
        assert unchanged(c, before), n
        if form != "load":
            assert lib.lqrhip_debug_pool_live() == live, n
    else:
        pytest.fail("the call never got through")
    # per image: I, P, positions, choices, the seam, (the build's own map,) and the job table
    assert failures >= (7 if form != "device" else 6), failures
    if form == "load":
        assert same_map(c.vmap_dump(), want) and c.resize(w - spec["d"], h) == 1 and same(shown(c), VC.model(img, want, w - spec["d"]))
    else:
        assert unchanged(c, before) and lib.lqrhip_debug_pool_live() == live
    c.destroy()
    assert lib.lqrhip_debug_pool_live() == live0


def test_an_allocation_failure_leaves_a_carver_that_was_not_flat_flattened(eng, lib):
    """the header's one exception to "unchanged": a carver that was not flat is flattened before the build allocates, and stays so.
    Every allocation of the call fails in turn (the flatten's own, if it has any, come first): each time LQR_NOMEM, the same image at
    the same size, the depth it had or -- from the first failure inside the build on -- 0 for good; then the call succeeds exactly"""
    spec = dict(CASES["pre_notflat"])
    live0 = lib.lqrhip_debug_pool_live()
    c = build(eng, spec)
    before = state(c)
    assert before[0]["depth"] > 0
    want, _ = model_of(c, spec)
    h, w = before[1].shape[:2]
    flat_failures = 0
    for n in range(64):
        lib.lqrhip_debug_fail_alloc(n)
        ret, got = device_map(c, spec["d"], spec["o"], h, w)
        lib.lqrhip_debug_fail_alloc(-1)
        if ret == 1:
            assert np.array_equal(got, want["data"]) and flattened(c, before)
            break
        assert ret == L.LQR_NOMEM, (n, ret)
        if flat_failures or c.getters()["depth"] == 0:
            assert flattened(c, before), n
            flat_failures += 1
        else:
            assert unchanged(c, before), n
    else:
        pytest.fail("the call never got through")
    # at least one failure fell inside the build, after the flatten.  (How many do is the pool's business: the injected failure hits
    # fresh blocks only, and the blocks the flatten gave back serve some of the build's planes)
    assert flat_failures >= 1, flat_failures
    c.destroy()
    assert lib.lqrhip_debug_pool_live() == live0


# ---- 7. cancel --------------------------------------------------------------------------------------------------------------------
def test_a_carver_cancelled_beforehand_refuses_every_call_unchanged(eng):
    import torch
    spec = dict(CASES["rgb_8i_float"], w=40, h=24, init=True)
    c = L.Carver.from_ext(eng, FC.make_image(spec), 0, init=True)
    c.configure(nrg_func=2, res_order=0, switch_freq=2, enl_step=2.0, progress=True)
    c.cancel_at_update(1, event="end")
    assert c.resize(37, 24) == 1 and c.cancelled() == 1
    before = state(c)
    eng.lqrhip_forward_launches(1)
    t = torch.zeros((24, 37), dtype=torch.int32, device="cuda")
    assert c.forward_map(4, 0) is None and c.forward_map_device(t, 4, 0) == L.LQR_USRCANCEL and c.load_forward(4, 0) == L.LQR_USRCANCEL
    assert c.resize_forward(30, 20) == L.LQR_USRCANCEL and L.forward_maps_device([c], [t], 4, 0) == L.LQR_USRCANCEL
    assert unchanged(c, before) and eng.lqrhip_forward_launches(0) == 0 and c.cancelled() == 1
    assert c.cancel_clear() == 1 and c.load_forward(4, 0) == 1 and c.getters()["depth"] == 4
    c.destroy()


@pytest.mark.parametrize("pre", [None, "notflat"])
def test_a_cancel_from_a_second_thread_during_a_build_is_honoured_between_slices(eng, pre):
    """depth 400: 25 slices.  The second thread waits until two slices have been enqueued, then cancels; the call returns
    LQR_USRCANCEL with the carver unchanged, well before the last slice.  A carver that was not flat (it shows 437 columns of 440) is
    the header's one exception: it shows the same image at the same size, flattened"""
    d = 400
    spec = dict(CASES["rgb_8i_float"], w=440, h=48, init=True, pre=pre)
    c = build(eng, spec)
    before = state(c)
    assert (before[0]["depth"] > 0) == (pre is not None)
    eng.lqrhip_forward_launches(1)
    running, box = threading.Event(), {}

    def other_thread():
        running.set()
        while eng.lqrhip_forward_launches(0) < 1 + 2 * 2 * K["FWD_SLICE_SEAMS"] and "ret" not in box:
            pass
        box["cancel"] = c.cancel()

    t = threading.Thread(target=other_thread)
    t.start()
    assert running.wait(60)
    try:
        box["ret"] = c.load_forward(d, 0)
    finally:
        box.setdefault("ret", None)
        t.join(60)
    launches = eng.lqrhip_forward_launches(0)
    assert box["ret"] == L.LQR_USRCANCEL and box["cancel"] == L.LQR_OK and c.cancelled() == 1, (box, launches)
    assert 1 + 2 * 2 * K["FWD_SLICE_SEAMS"] <= launches < 1 + 2 * d
    assert flattened(c, before) if pre else unchanged(c, before)
    # ... and after the mark is cleared the same call builds the whole map
    assert c.cancel_clear() == 1 and c.load_forward(d, 0) == 1 and c.getters()["depth"] == d
    assert same_map(c.vmap_dump(), FC.forward_map(FC.intensity(before[1], 0, FC.type_state(spec), False), None, d, 0))
    c.destroy()


# ---- 8. the seam loop beside it ---------------------------------------------------------------------------------------------------
def census(lb):
    out = (ctypes.c_ulonglong * SLOTS)()
    assert lb.lqrhip_launch_census(out, SLOTS, 1) == SLOTS
    return [int(x) for x in out]


def test_an_ordinary_resize_launches_and_gives_the_same_before_and_after_a_forward_build(eng, lib):
    spec = dict(CASES["rgb_8i_float"], w=300, h=40, init=True)
    img = FC.make_image(spec)

    def ordinary():
        c = L.Carver.from_ext(eng, img, 0, init=True)
        c.configure(nrg_func=2, res_order=0, switch_freq=2, enl_step=2.0)
        census(lib)
        assert c.resize(270, 34) == 1
        out = (census(lib), shown(c), c.vmap_dump()["data"])
        c.destroy()
        return out
    a = ordinary()
    f = build(eng, spec, img)
    census(lib)
    assert f.forward_map(25, 0) is not None and f.load_forward(25, 1) == 1
    assert census(lib) == [0] * SLOTS                # a forward build and its load run none of the seam loop's kernels
    f.destroy()
    b = ordinary()
    assert a[0] == b[0] and sum(a[0]) > 0 and same(a[1], b[1]) and np.array_equal(a[2], b[2])
