"""Computed masks (include/lqr_masks.h) on the MI355X.

* every vector the genuine liblqr 0.4.1 recorded under tests/golden/masks/ is reproduced through mask_cases.run: every call's return
  value, both planes (snapshots and final), the energy plane at 0 ULP, the carved image and the visibility map; there is no skip list;
* the two finding vectors (liblqr's offsets on a transposed carver) give the planes include/lqr_masks.h documents, i.e. the numpy
  model's, which tests/test_masks_abi.py pins to the genuine planes everywhere else;
* the device forms on torch tensors against the host forms; a binary float mask against the same mask painted black and white;
* how the _xy calls are batched (lqrhip_debug_mask_flushes); a group of two carvers masked through different forms as one batch.
"""
import json
import os

import numpy as np
import pytest

import coldepth_cases as CD
import lqr_ctypes as L
import mask_cases as MC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "masks")
MANIFEST = json.load(open(os.path.join(GOLD, "MANIFEST.json")))
bits = CD.bits


@pytest.fixture(scope="module")
def eng():
    return L.bind_masks(L.engine_api())


def load(entry):
    z = np.load(os.path.join(GOLD, entry["file"]))
    return json.loads(str(z["spec"])), z


@pytest.mark.parametrize("name", [v["name"] for v in MANIFEST["vectors"]])
def test_genuine_vector_is_reproduced(eng, name):
    spec, z = load(next(v for v in MANIFEST["vectors"] if v["name"] == name))
    got = MC.run(eng, L.Carver, spec)
    MC.assert_same_record(got, z, name)


@pytest.mark.parametrize("name", [v["name"] for v in MANIFEST["findings"]])
def test_finding_vector_gives_the_documented_planes(eng, name):
    spec, z = load(next(v for v in MANIFEST["findings"] if v["name"] == name))
    got = MC.run(eng, L.Carver, spec)
    rec, want = json.loads(str(got["record"])), json.loads(str(z["record"]))
    assert rec["rets"] == want["rets"] and rec["step_rets"] == want["step_rets"] and rec["after_ops"] == want["after_ops"]
    _, extra = MC.make_input(spec)
    m = MC.Model(spec, extra["masks"])
    for op in spec["ops"]:
        m.apply(op)
    assert m.valid
    for which in ("bias", "rig"):
        assert np.array_equal(bits(got[which]), bits(m.plane(which))), which
        assert not np.array_equal(bits(got[which]), bits(z[which])), which          # (and so not liblqr's misplaced ones)


# ---- the device forms ---------------------------------------------------------------------------------------------------------
def _carver(eng, seed=11, w=300, h=40, transposed=False, **kw):
    rng = np.random.default_rng(seed)
    c = L.Carver.from_ext(eng, CD.base_image(rng, w, h, 3), 0, rigidity=kw.pop("rigidity", 1.5), **kw)
    c.configure(nrg_func=2)
    if transposed:
        assert c.resize(w, h - 4) == 1 and c.getters()["orientation"] == 1
    return c


def _state(c, w1, h1):
    out = dict(bias=c.get_bias(), rig=c.get_rigmask(), energy=c.energy())
    assert c.resize(w1, h1) == 1
    out.update(image=c.read_image_ext(), vmap=c.vmap_dump()["data"])
    return out


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(bits(a[k]), bits(b[k])), k


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_device_tensor_gives_what_the_host_form_gives(eng, dtype, transposed):
    import torch
    rng = np.random.default_rng(5)
    bias = rng.uniform(-1, 2, (30, 257)).astype(dtype)           # 257 columns: two blocks per row, overhanging the image below
    rig = rng.uniform(0, 2, (36, 300)).astype(dtype)
    h = 36 if transposed else 40
    res = []
    for device in (False, True):
        c = _carver(eng, transposed=transposed)
        if device:
            tb, tr = torch.from_numpy(bias).cuda(), torch.from_numpy(rig).cuda()
            assert c.bias_add_device(tb, 37, 50, 20) == 1 and c.rigmask_add_device(tr, -3, 2) == 1
            assert c.bias_add_device(tb, 0, 0, 0) == 1                          # bias_factor 0: nothing
            assert c.bias_add_device(tb, 5, 400, 0) == 1                        # wholly outside: nothing
            assert np.array_equal(tb.cpu().numpy(), bias) and np.array_equal(tr.cpu().numpy(), rig)       # the caller's buffers are only read
        else:                                                                   # the host form fed the widened values
            assert c.bias_add_f(bias.astype(np.float64), 37, 50, 20) == 1 and c.rigmask_add_f(rig.astype(np.float64), -3, 2) == 1
        res.append(_state(c, 290, h))
        c.destroy()
    assert res[0]["bias"].any() and res[0]["rig"].any()
    _same(res[0], res[1])


def test_device_form_refuses_other_depths(eng):
    import torch
    c = _carver(eng)
    t = torch.zeros((4, 4), dtype=torch.float32, device="cuda")
    f = eng.lqrx_carver_bias_add_area_device
    assert f(c.p, t.data_ptr(), L.LQR_COLDEPTH_8I, 3, 4, 4, 0, 0) == 0 and f(c.p, t.data_ptr(), L.LQR_COLDEPTH_16I, 3, 4, 4, 0, 0) == 0
    assert eng.lqrx_carver_rigmask_add_area_device(c.p, t.data_ptr(), 7, 4, 4, 0, 0) == 0
    assert not c.get_bias().any() and not c.get_rigmask().any()
    c.destroy()


def test_binary_float_mask_equals_the_same_mask_painted_black_and_white(eng):
    rng = np.random.default_rng(6)
    m = (rng.random((40, 300)) < 0.4)
    res = []
    for form in ("float", "rgb"):
        c = _carver(eng)
        if form == "float":
            assert c.bias_add_f(m.astype(np.float64), 1000, 0, 0) == 1 and c.rigmask_add_f(m.astype(np.float64), 0, 0) == 1
        else:
            painted = (m * 255).astype(np.uint8)[:, :, None]
            assert c.bias_add(painted, 1000) == 1 and c.rigmask_add(painted) == 1
        res.append(_state(c, 280, 40))
        c.destroy()
    assert set(np.unique(res[0]["bias"])) == {0.0, 500.0} and set(np.unique(res[0]["rig"])) == {0.0, 1.0}
    _same(res[0], res[1])


# ---- batching of the _xy calls ------------------------------------------------------------------------------------------------
def test_full_frame_of_xy_calls_is_one_scatter_launch_and_three_repeats_are_three(eng):
    rng = np.random.default_rng(8)
    c = L.Carver.from_ext(eng, CD.base_image(rng, 64, 64, 1), 0)
    c.configure(nrg_func=2)
    n0 = eng.lqrhip_debug_mask_flushes()
    vals = rng.uniform(-2, 2, 64 * 64)
    assert set(c.bias_add_xy([(i % 64, i // 64, vals[i]) for i in range(64 * 64)])) == {1}
    assert eng.lqrhip_debug_mask_flushes() == n0                       # nothing has reached the device yet
    assert c.resize(60, 64) == 1
    assert eng.lqrhip_debug_mask_flushes() == n0 + 1
    c.destroy()
    # every pixel three times, interleaved: three buckets, applied in call order
    spec = dict(MC.cases())["xy_repeat3"]
    img, _ = MC.make_input(spec)
    c = L.Carver.from_ext(eng, img, 0)
    entries = MC.make_run(spec, "a", 300, 40)
    n0 = eng.lqrhip_debug_mask_flushes()
    assert set(c.bias_add_xy(entries)) == {1}
    got = c.get_bias()                                                  # a read-out flushes
    assert eng.lqrhip_debug_mask_flushes() == n0 + 3
    want = np.zeros((40, 300), np.float32)
    for x, y, v in entries:
        want[y, x] = want[y, x] + np.float32(v) / np.float32(2)
    assert np.array_equal(bits(got), bits(want))
    assert c.get_bias() is not None and eng.lqrhip_debug_mask_flushes() == n0 + 3          # nothing left to flush
    c.destroy()


def test_xy_calls_outside_the_image_are_refused_and_zero_bias_is_nothing(eng):
    c = _carver(eng, w=40, h=30)
    assert c.bias_add_xy([(40, 0, 1.0), (0, 30, 1.0), (-1, 0, 1.0), (0, -1, 1.0)]) == [0, 0, 0, 0]
    assert c.rigmask_add_xy([(40, 0, 1.0), (0, 30, 1.0), (-1, 0, 1.0)]) == [0, 0, 0]
    assert c.bias_add_xy([(3, 3, 0.0)]) == [1]
    assert c.bias_add_xy([(39, 29, 3.0)]) == [1] and c.rigmask_add_xy([(0, 0, 0.5)]) == [1]
    b, r = c.get_bias(), c.get_rigmask()
    assert b[29, 39] == 1.5 and np.count_nonzero(b) == 1 and r[0, 0] == 0.5 and np.count_nonzero(r) == 1
    c.destroy()


def test_queued_calls_are_dropped_by_destroy_and_by_a_reload(eng):
    import torch
    rng = np.random.default_rng(9)
    img = CD.base_image(rng, 64, 32, 3)
    c = L.Carver.from_ext(eng, img, 0)
    c.configure(nrg_func=2)
    plain = c.energy()
    assert set(c.bias_add_xy([(x, 5, 100.0) for x in range(64)])) == {1}
    t = torch.from_numpy(img).cuda()
    assert L.reload_device_batch(eng, [c], [t.data_ptr()]) == 1
    assert not c.get_bias().any() and np.array_equal(c.energy(), plain)
    assert set(c.bias_add_xy([(x, 6, 100.0) for x in range(64)])) == {1}
    c.destroy()                                                          # with entries still queued


# ---- a group masked through different forms -----------------------------------------------------------------------------------
def test_float_form_and_rgb_form_carve_as_one_batch_and_match(eng):
    rng = np.random.default_rng(10)
    m = (rng.random((40, 300)) < 0.3)
    painted = (m * 255).astype(np.uint8)[:, :, None]

    def make(form):
        c = _carver(eng, seed=12)
        if form == "float":
            assert c.bias_add_f(m.astype(np.float64), 600, 0, 0) == 1 and c.rigmask_add_f(m.astype(np.float64), 0, 0) == 1
        elif form == "xy":
            ys, xs = np.nonzero(m)
            assert set(c.bias_add_xy([(x, y, 600.0) for x, y in zip(xs, ys)])) == {1}
            assert set(c.rigmask_add_xy([(x, y, 1.0) for x, y in zip(xs, ys)])) == {1}
        else:
            assert c.bias_add(painted, 600) == 1 and c.rigmask_add(painted) == 1
        return c

    alone = make("rgb")
    assert alone.resize(270, 40) == 1
    want = (alone.read_image_ext(), alone.vmap_dump()["data"])
    alone.destroy()
    group = [make("float"), make("rgb"), make("xy")]
    assert L.resize_batch(eng, group, 270, 40) == 1
    for c in group:
        assert np.array_equal(c.read_image_ext(), want[0]) and np.array_equal(c.vmap_dump()["data"], want[1])
        c.destroy()
    # a cleared carver groups with one that never had masks, and carves like it
    a, b = _carver(eng, seed=13), _carver(eng, seed=13)
    assert a.bias_add_f(m.astype(np.float64), 600, 0, 0) == 1 and a.rigmask_add_f(m.astype(np.float64), 0, 0) == 1
    a.bias_clear(); a.rigmask_clear()
    assert L.resize_batch(eng, [a, b], 270, 40) == 1
    assert np.array_equal(a.read_image_ext(), b.read_image_ext()) and np.array_equal(a.vmap_dump()["data"], b.vmap_dump()["data"])
    a.destroy(); b.destroy()
