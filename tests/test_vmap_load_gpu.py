"""Seam-map loading (include/lqr_vmap.h) on the MI355X.

* every vector the genuine liblqr 0.4.1 recorded under tests/golden/vmap/ is reproduced through vmap_cases.run: return values, getters,
  the image at every recorded size, the map dumped again, the carver's list;
* init after a load and a deeper resize: the golden vector's return values and getters, and the pixels of a true warm start;
* round trips on the engine: a carver A makes a map, a fresh carver B of the same image loads it and equals A at length - d,
  length - d / 2, length, length + 1 and length + d, on shapes chosen for what can go wrong (SHAPES says what each crosses);
* random per-line permutation maps (no connected seams) against the numpy model, which tests/test_vmap_abi.py pins to the genuine code;
* a map in device memory, one map shared by a batch of 8 and of 34 carvers, every refusal of the header, resizes outside the loaded
  range, and an allocation failure at every allocation point of one load.
"""
import ctypes
import json
import os

import numpy as np
import pytest

import coldepth_cases as CD
import lqr_ctypes as L
import vmap_cases as VC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "vmap")
MANIFEST = json.load(open(os.path.join(GOLD, "MANIFEST.json")))
bits = CD.bits


@pytest.fixture(scope="module")
def eng():
    return L.bind_vmap(L.bind_imagetype(L.engine_api()))


@pytest.fixture
def lib(eng):
    lb = eng.lib
    lb.lqrhip_fault_stats.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
    lb.lqrhip_get_no_spin.restype = ctypes.c_int
    lb.lqrhip_debug_fail_alloc.argtypes = [ctypes.c_int]
    lb.lqrhip_debug_pool_live.restype, lb.lqrhip_debug_pool_live.argtypes = ctypes.c_ulonglong, []
    yield lb
    lb.lqrhip_debug_fail_alloc(-1)


def fault_stats(lb):
    st = (ctypes.c_ulonglong * 8)()
    assert lb.lqrhip_fault_stats(st, 0) == 0
    return [int(x) for x in st], lb.lqrhip_get_no_spin()


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ---- the genuine vectors ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [v["name"] for v in MANIFEST["vectors"]])
def test_genuine_vector_is_reproduced(eng, name):
    entry = next(v for v in MANIFEST["vectors"] if v["name"] == name)
    z = np.load(os.path.join(GOLD, entry["file"]))
    spec = json.loads(str(z["spec"]))
    meta = json.loads(str(z["record"]))["map_meta"]
    got = VC.run(eng, L.Carver, spec, vmap=dict(data=z["map"], depth=meta[0], orientation=meta[1]))
    VC.assert_same_record(got, z, name)


@pytest.mark.parametrize("name", ["init_after_load_h", "init_after_load_v"])
def test_init_after_a_load_and_a_deeper_resize_is_a_warm_start(eng, name):
    """Against the golden vector: every return value and every getter (the depth grows from the map's 10 to 15, from 7 to 12; the load
    onto the now initialised carver is refused).  NOT its images: the genuine code finds the further seams on the wrong pixels and
    dumps a map that holds levels twice (tests/test_vmap_abi.py; include/lqr_vmap.h item 5).  The reference for the pixels is the
    engine's own carver that made the map, carved on to the same size: the loaded carver continues exactly where that one stood"""
    entry = next(v for v in MANIFEST["findings"] if v["name"] == name)
    z = np.load(os.path.join(GOLD, entry["file"]))
    spec = json.loads(str(z["spec"]))
    rec = json.loads(str(z["record"]))
    d, o = rec["map_meta"]
    got = VC.run(eng, L.Carver, spec, vmap=dict(data=z["map"], depth=d, orientation=o))
    mine = json.loads(str(got["record"]))
    assert mine["rets"] == rec["rets"] == [1, 1, 1, 1, 1, 0] and mine["getters"] == rec["getters"] and mine["redump_meta"] == rec["redump_meta"]
    assert mine["getters"][2]["depth"] > d
    deeper = dict(data=got["dump@3"], depth=mine["redump_meta"]["3"][0], orientation=o)
    assert VC.valid_map(deeper, spec["w"], spec["h"]) and not VC.valid_map(dict(deeper, data=z["dump@3"]), spec["w"], spec["h"])
    # the carver that makes this map, carved on: the generator of the vector, on the engine
    a = L.Carver.from_ext(eng, z["img"], 0, delta_x=spec["delta"], rigidity=spec["rigidity"])
    a.configure(nrg_func=spec["map"]["nrg"], res_order=0, switch_freq=2, enl_step=2.0)
    assert a.resize(*spec["map"]["to"]) == 1 and np.array_equal(a.vmap_dump()["data"], z["map"])
    for i in (2, 4):
        assert a.resize(spec["ops"][i][1], spec["ops"][i][2]) == 1
        assert same(a.scan_line_ext()[0], got["image@%d" % i]), i
    assert np.array_equal(a.vmap_dump()["data"], got["dump@3"])
    a.destroy()


# ---- round trips on the engine --------------------------------------------------------------------------------------------------
SHAPES = [
    pytest.param(40, 24, 10, 0, id="40x24-d10"),
    pytest.param(300, 37, 33, 0, id="300x37-d33-two-chunks-of-256-columns-the-rank-carry-of-the-inflate"),
    pytest.param(530, 9, 200, 0, id="530x9-d200-three-chunks-seven-words-of-level-bits"),
    pytest.param(2, 3, 1, 0, id="2x3-d1-the-smallest"),
    pytest.param(64, 1, 20, 0, id="64x1-one-line-one-wave"),
    pytest.param(45, 70, 33, 1, id="45x70-d33-vertical-no-multiple-of-the-32-tile"),
    pytest.param(37, 300, 33, 1, id="37x300-d33-vertical-ten-tiles-down-two-workgroups"),
]


def _image(w, h, ch=3, seed=5):
    return CD.base_image(np.random.default_rng([seed, w, h, ch]), w, h, ch)


def _size(w, h, o, k):
    return (w + k, h) if o == 0 else (w, h + k)


def _generator(eng, img, w, h, d, o, depth=0):
    a = L.Carver.from_ext(eng, img, depth)
    a.configure(enl_step=2.0)
    assert a.resize(*_size(w, h, o, -d)) == 1
    return a, a.vmap_dump()


@pytest.mark.parametrize("w,h,d,o", SHAPES)
def test_round_trip_a_fresh_carver_with_the_loaded_map_equals_the_carver_that_made_it(eng, w, h, d, o):
    img = _image(w, h)
    a, m = _generator(eng, img, w, h, d, o)
    if (h if o else w) - d == 1:
        # carved down to ONE column, liblqr's finish_vsmap marks the column that is left with a level above the depth (here depth + 1),
        # and lqr_vmap_dump hands that mark out.  It hides and doubles nothing at any size the map covers, exactly as 0; the validation
        # (include/lqr_vmap.h item 1) takes no value above depth, so a caller clears the mark before loading such a map
        assert set(np.unique(m["data"])) == {1, d + 1}
        m["data"][m["data"] == d + 1] = 0
    assert (m["depth"], m["orientation"], m["data"].shape) == (d, o, (h, w)) and VC.valid_map(m, w, h)
    b = L.Carver.from_ext(eng, img, 0, init=False)
    assert b.vmap_load(m) == 1
    g = b.getters()
    assert (g["depth"], g["enl_step"], g["orientation"], g["width"], g["height"], g["ref_width"], g["ref_height"]) == (d, 2.0, o, w, h, w, h)
    assert np.array_equal(b.vmap_dump()["data"], m["data"])
    for k in (-d, -(d // 2), 0, 1, d, -d):
        size = _size(w, h, o, k)
        assert a.resize(*size) == 1 and b.resize(*size) == 1, k
        want, got = a.scan_line_ext()[0], b.scan_line_ext()[0]
        assert want.shape[:2] == (size[1], size[0]) and same(got, want), k
        assert same(got, VC.model(img, m, size[o])), k             # (seam-connected maps are the model's too)
    a.destroy(); b.destroy()


# ---- maps no carver made, against the model -------------------------------------------------------------------------------------
KINDS = {"8i-rgb": (3, 0, None), "8i-rgba": (4, 0, None), "16i-grey": (1, 1, None), "32f-rgba": (4, 2, None), "8i-five-channels": (5, 0, 8)}


def _kind_image(kind, w, h):
    ch, depth, max_ch = KINDS[kind]
    rng = np.random.default_rng([6, w, h, ch, depth])
    return CD.to_depth(rng, CD.base_image(rng, w, h, ch), depth), depth, max_ch


def _fresh(eng, img, depth, max_ch=None):
    prev = eng.lqrx_set_max_channels(max_ch) if max_ch else None
    try:
        return L.Carver.from_ext(eng, img, depth, init=False)
    finally:
        if prev is not None:
            eng.lqrx_set_max_channels(prev)


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("w,h,d,o", [(70, 45, 23, 0), (70, 45, 19, 1), (300, 37, 41, 0)])
def test_permutation_map_gives_the_models_image_at_every_size(eng, kind, w, h, d, o):
    img, depth, max_ch = _kind_image(kind, w, h)
    m = VC.perm_map(1000 + d, w, h, d, o)
    c = _fresh(eng, img, depth, max_ch)
    assert c.vmap_load(m) == 1
    assert np.array_equal(c.vmap_dump()["data"], m["data"])
    for k in (-d, d, -(d // 2), 1, 0):
        size = _size(w, h, o, k)
        assert c.resize(*size) == 1, k
        assert same(c.scan_line_ext()[0], VC.model(img, m, size[o])), (kind, k)
    c.destroy()


# ---- device map, batch ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("o", [0, 1])
def test_map_in_device_memory_equals_the_host_load(eng, o):
    import torch
    w, h, d = 70, 45, 15
    img = _image(w, h)
    m = VC.perm_map(2000, w, h, d, o)
    a, b = _fresh(eng, img, 0), _fresh(eng, img, 0)
    t = torch.from_numpy(m["data"]).to("cuda")
    assert a.vmap_load(m) == 1 and b.vmap_load_device(t, d, o) == 1
    assert a.getters() == b.getters() and np.array_equal(b.vmap_dump()["data"], m["data"])
    assert torch.equal(t.cpu(), torch.from_numpy(m["data"]))            # the caller's map is read, not written
    for k in (-d, d, 3):
        size = _size(w, h, o, k)
        assert a.resize(*size) == 1 and b.resize(*size) == 1
        assert same(a.read_image_ext(), b.read_image_ext()), k
    a.destroy(); b.destroy()


@pytest.mark.parametrize("n", [8, 34])
@pytest.mark.parametrize("o", [0, 1])
def test_one_map_loaded_into_a_batch_equals_each_carver_loaded_alone(eng, n, o):
    """(34: the group size of tests/test_faults_gpu.py, two sub-batch streams where the process has the queues)"""
    w, h, d = 70, 45, 21
    imgs = [_image(w, h, seed=100 + i) for i in range(n)]
    m = VC.perm_map(3000 + o, w, h, d, o)
    cs = [_fresh(eng, im, 0) for im in imgs]
    assert L.vmap_load_batch(cs, m) == 1
    alone = _fresh(eng, imgs[n - 1], 0)
    assert alone.vmap_load(m) == 1 and alone.getters() == cs[n - 1].getters()
    for k in (-d, d):
        size = _size(w, h, o, k)
        assert L.resize_batch(eng, cs, *size) == 1 and alone.resize(*size) == 1
        assert same(cs[n - 1].read_image_ext(), alone.read_image_ext()), k
        for im, c in zip(imgs, cs):
            assert same(c.scan_line_ext()[0], VC.model(im, m, size[o])), k
    for c in cs + [alone]:
        c.destroy()


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def _bad_maps(w, h, d):
    good = VC.perm_map(4000, w, h, d, 0)
    out = {}

    def variant(name, fn=None, **meta):
        m = dict(good, data=good["data"].copy())
        if fn:
            fn(m["data"])
        m.update(meta)
        out[name] = m

    def twice(a):
        y = h // 2
        a[y, np.flatnonzero(a[y] == 0)[0]] = 3
    variant("a level twice in one line", twice)

    def missing(a):
        a[h - 1][a[h - 1] == d] = 0
    variant("a level missing", missing)

    def negative(a):
        a[0, np.flatnonzero(a[0] == 0)[-1]] = -1
    variant("a value of -1", negative)

    def too_large(a):
        y = 1
        a[y][a[y] == 1] = d + 1
    variant("a value of depth + 1", too_large)
    variant("depth 0", lambda a: a.fill(0), depth=0)
    variant("depth = width", depth=w)
    variant("a map one column short", data=np.ascontiguousarray(good["data"][:, :-1]))
    vertical = VC.perm_map(4001, w, h, d, 1)
    variant("the orientation-1 map of a non-square image passed with orientation 0", data=vertical["data"])
    return good, out


REFUSED = ["a level twice in one line", "a level missing", "a value of -1", "a value of depth + 1", "depth 0", "depth = width",
           "a map one column short", "the orientation-1 map of a non-square image passed with orientation 0", "an initialised carver",
           "an attached carver", "a carver resized to a size other than the map's"]


@pytest.mark.parametrize("what", REFUSED)
def test_refused_load_returns_error_and_leaves_the_carver_exactly_as_it_was(eng, lib, what):
    w, h, d = 70, 45, 12
    img = _image(w, h)
    good, bad = _bad_maps(w, h, d)
    root = None
    if what == "an initialised carver":
        c, m = L.Carver.from_ext(eng, img, 0, init=True), good
    elif what == "an attached carver":
        root = _fresh(eng, img, 0)
        c, m = root.attach_ext(_image(w, h, seed=9), 0), good
    elif what == "a carver resized to a size other than the map's":
        c, m = _fresh(eng, img, 0), good
        assert c.vmap_load(good) == 1 and c.resize(w + 5, h) == 1
    else:
        c, m = _fresh(eng, img, 0), bad[what]
        assert not VC.valid_map(m, w, h)
    if what != "a carver resized to a size other than the map's":
        c.configure(enl_step=1.5)
    before = (c.getters(), c.scan_line_ext()[0] if what != "an attached carver" else None, lib.lqrhip_debug_pool_live(), fault_stats(lib))
    assert c.vmap_load(m) == 0, what
    assert c.getters() == before[0] and lib.lqrhip_debug_pool_live() == before[2] and fault_stats(lib) == before[3], what
    if before[1] is not None:
        assert same(c.scan_line_ext()[0], before[1]), what
    # a valid load and a resize still work
    if what in ("an initialised carver", "an attached carver"):
        target = root or c
        if root is None:
            assert c.resize(w - 4, h) == 1
        else:
            assert root.vmap_load(good) == 1 and root.resize(w - d, h) == 1
            assert same(c.scan_line_ext()[0], VC.model(_image(w, h, seed=9), good, w - d))
        target.destroy()
        return
    if what == "a carver resized to a size other than the map's":
        assert c.resize(w, h) == 1
    assert c.vmap_load(good) == 1 and c.resize(w - d, h) == 1
    assert same(c.scan_line_ext()[0], VC.model(img, good, w - d)), what
    c.destroy()


@pytest.mark.parametrize("o", [0, 1])
def test_a_resize_outside_the_loaded_range_is_refused_and_the_carver_still_serves_every_size_in_range(eng, lib, o):
    w, h, d = 70, 45, 9
    img = _image(w, h)
    m = VC.perm_map(5000, w, h, d, o)
    c = _fresh(eng, img, 0)
    assert c.vmap_load(m) == 1 and c.resize(*_size(w, h, o, -3)) == 1
    before = (c.getters(), c.scan_line_ext()[0], lib.lqrhip_debug_pool_live(), fault_stats(lib))
    other = (w, h - 2) if o == 0 else (w - 2, h)
    both = (w - 2, h - 2)
    for size in (_size(w, h, o, d + 1), _size(w, h, o, -d - 1), other, both):
        assert c.resize(*size) == 0, size
        assert c.getters() == before[0] and same(c.scan_line_ext()[0], before[1]), size
    assert lib.lqrhip_debug_pool_live() == before[2] and fault_stats(lib) == before[3]
    for k in (-d, d, 0, -1):
        size = _size(w, h, o, k)
        assert c.resize(*size) == 1 and same(c.scan_line_ext()[0], VC.model(img, m, size[o])), k
    c.destroy()


# ---- allocation failures --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("o", [0, 1])
def test_an_allocation_failure_anywhere_in_a_load_leaves_a_usable_carver(eng, lib, o):
    """the nth device allocation of the load fails, once, for every n until the load gets through.  The carver had been loaded and
    resized before (so the load flattens; for o = 1 the first map was horizontal, so it transposes too): each time LQR_NOMEM, the
    carver in one of the three states the sequence passes through, the same load repeated succeeds, the pool count returns"""
    w, h, d = 70, 45, 14
    img = _image(w, h)
    first = VC.perm_map(6000, w, h, 8, 0)
    m = VC.perm_map(6001, w, h, d, o)
    flat = img
    failures, states = 0, set()
    for n in range(0, 200):
        live = lib.lqrhip_debug_pool_live()
        c = _fresh(eng, img, 0)
        assert c.vmap_load(first) == 1 and c.resize(w - 3, h) == 1 and c.resize(w, h) == 1
        lib.lqrhip_debug_fail_alloc(n)
        ret = c.vmap_load(m)
        lib.lqrhip_debug_fail_alloc(-1)
        if ret == 1:
            assert c.resize(*_size(w, h, o, -d)) == 1 and same(c.scan_line_ext()[0], VC.model(img, m, _size(w, h, o, -d)[o]))
            c.destroy()
            assert lib.lqrhip_debug_pool_live() == live, n
            break
        assert ret == L.LQR_NOMEM, (n, ret)
        failures += 1
        g = c.getters()
        assert (g["width"], g["height"]) == (w, h) and same(c.scan_line_ext()[0], flat), n
        state = "as it was" if g["depth"] == 8 else "flattened" if g["orientation"] == 0 else "transposed"
        assert g["depth"] in (0, 8) and (g["orientation"] == 0 or o == 1), (n, g)
        states.add(state)
        assert c.vmap_load(m) == 1, n
        assert c.resize(*_size(w, h, o, d)) == 1 and same(c.scan_line_ext()[0], VC.model(img, m, _size(w, h, o, d)[o])), n
        c.destroy()
        assert lib.lqrhip_debug_pool_live() == live, n
    else:
        pytest.fail("the load never got through")
    print("allocation sweep o=%d: %d failure points, states %s" % (o, failures, sorted(states)))
    assert failures >= 3 and states >= {"as it was", "flattened"} and (o == 0 or "transposed" in states), (failures, states)
