"""The energy read-outs (include/lqr_energy.h) on the MI355X.

* every vector the genuine liblqr 0.4.1 recorded under tests/golden/energy/ is reproduced through energy_cases.run: every call's
  return value, the orientation after it, the float planes at 0 ULP, the pictures byte for byte, the guard bytes, and the carved image
  and visibility map of the resizes that follow; there is no skip list.  The two finding vectors (read-outs on an attached carver,
  which the engine refuses) give LQR_ERROR and change nothing;
* shapes beyond what a golden file holds, chosen from the kernels' constants (SHAPES says which boundary each crosses): the true
  energy against the old hook lqrx_carver_get_energy, and the normalised plane and two pictures against the numpy model, which
  tests/test_energy_abi.py pins to the genuine code;
* the device forms on torch tensors against the host forms, also at an address one element past an allocation's start;
* all-negative and constant planes over many workgroups (the seeds of the reduction);
* an allocation failure at every allocation point of one read-out; tests/c/energy_replay.c linked to the engine.
"""
import ctypes
import gc
import json
import os
import subprocess

import numpy as np
import pytest

import coldepth_cases as CD
import energy_cases as EC
import imgtype_cases as IT
import lqr_ctypes as L

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "energy")
MANIFEST = json.load(open(os.path.join(GOLD, "MANIFEST.json")))
bits = CD.bits


@pytest.fixture(scope="module")
def eng():
    return L.bind_energy(L.bind_masks(L.bind_imagetype(L.engine_api())))


def load(entry):
    z = np.load(os.path.join(GOLD, entry["file"]))
    return json.loads(str(z["spec"])), z


@pytest.mark.parametrize("name", [v["name"] for v in MANIFEST["vectors"]])
def test_genuine_vector_is_reproduced(eng, name):
    spec, z = load(next(v for v in MANIFEST["vectors"] if v["name"] == name))
    got = EC.run(eng, L.Carver, spec)
    EC.assert_same_record(got, z, name)


@pytest.mark.parametrize("name", [v["name"] for v in MANIFEST["findings"] if v["name"].startswith("size_")])
def test_frame_one_pixel_wide_has_energy_zero_and_the_read_outs_are_the_models(eng, name):
    """liblqr reads outside a one-pixel-wide frame and reports the brightness; the engine's energy there is 0 (include/lqr_energy.h)"""
    spec, z = load(next(v for v in MANIFEST["findings"] if v["name"] == name))
    got = EC.run(eng, L.Carver, spec)
    rec, want = json.loads(str(got["record"])), json.loads(str(z["record"]))
    assert rec == want                                  # return values, orientations, guard bytes
    for i, op in enumerate(spec["ops"]):
        true = got["true@%d" % i]
        assert true.shape == z["true@%d" % i].shape and not true.any() and z["true@%d" % i].all()
        model = EC.normalised(true) if op[0] == "norm" else EC.picture(true, op[2], op[3])
        assert got["out@%d" % i].dtype == model.dtype and np.array_equal(bits(got["out@%d" % i]), bits(model)), i


@pytest.mark.parametrize("name", [v["name"] for v in MANIFEST["findings"] if v["name"].startswith("attached_")])
def test_read_out_on_an_attached_carver_is_refused_and_changes_nothing(eng, name):
    spec, z = load(next(v for v in MANIFEST["findings"] if v["name"] == name))
    got = EC.run(eng, L.Carver, spec)
    rec, want = json.loads(str(got["record"])), json.loads(str(z["record"]))
    assert rec["rets"] == [0] * len(spec["ops"]) and all(rec["intact"])          # (liblqr: LQR_OK; include/lqr_energy.h says why not here)
    assert rec["orientation"] == want["orientation"] and rec["after_ops"] == want["after_ops"]
    assert not [k for k in got if k.startswith("out@")]


# ---- shapes from the kernels' constants ---------------------------------------------------------------------------------------
# k_energy_range: 256 threads, EO_CHUNK = 1024 pixels of a row per unit, at most EO_MAX_PARTIALS = 512 workgroups;
# k_energy_plane / k_energy_out: tiles of EO_TILE = 64 x 64, a wave per tile row, 256 threads fold the partials
SHAPES = [
    pytest.param(65, 3, id="65x3-past-a-wave-of-64-lanes-and-one-tile-across"),
    pytest.param(3, 65, id="3x65-past-one-tile-down"),
    pytest.param(257, 2, id="257x2-past-the-256-threads-of-a-workgroup"),
    pytest.param(129, 67, id="129x67-three-by-two-tiles-odd-edges"),
    pytest.param(300, 260, id="300x260-260-partials-more-than-a-wave-and-than-256-fold-threads"),
    pytest.param(1025, 3, id="1025x3-two-chunks-per-row"),
    pytest.param(31, 530, id="31x530-more-units-than-512-workgroups"),
]


def _image(w, h, seed=3):
    return CD.base_image(np.random.default_rng([seed, w, h]), w, h, 3)


def _carver(eng, img, nrg=0, bias=None, init=True):
    c = L.Carver.from_ext(eng, img, 0, init=init)
    c.configure(nrg_func=nrg)
    if bias is not None:
        assert c.bias_add_f(bias, 30) == 1
    return c


@pytest.mark.parametrize("w,h", SHAPES)
def test_shapes_across_the_kernels_boundaries_equal_the_old_hook_and_the_model(eng, w, h):
    img = _image(w, h)
    bias = np.random.default_rng([4, w, h]).uniform(-1.0, 1.0, (h, w))
    for o in (0, 1, 0):
        a = _carver(eng, img, bias=bias)
        true = a.get_energy(o, true=True)
        assert a.getters()["orientation"] == o and true.shape == (h, w)
        # the old hook on a carver brought to the same frame (by a picture read-out) gives the plane in the CARVER's frame
        b = _carver(eng, img, bias=bias)
        if o:
            b.get_energy_image(1, L.LQR_COLDEPTH_8I, L.LQR_GREY_IMAGE)
        old = b.energy()
        assert np.array_equal(bits(true), bits(np.ascontiguousarray(old.T) if o else old)), o
        b.destroy()
        assert np.array_equal(bits(a.get_energy(o)), bits(EC.normalised(true))), o
        for depth, image_type in ((L.LQR_COLDEPTH_8I, L.LQR_RGBA_IMAGE), (L.LQR_COLDEPTH_16I, L.LQR_CMYKA_IMAGE)):
            assert np.array_equal(a.get_energy_image(o, depth, image_type), EC.picture(true, depth, image_type)), (o, depth, image_type)
        assert np.array_equal(bits(a.get_energy(o, true=True)), bits(true))            # nothing above changed the energy
        a.destroy()


@pytest.mark.parametrize("kind", ["all-negative", "constant-negative", "constant-zero", "constant-positive"])
def test_the_seeds_of_the_reduction_over_many_workgroups(eng, kind):
    """300 x 260: 260 workgroups leave partials.  e_max is seeded with 0, e_min with FLT_MAX, in every stage of the fold"""
    w, h = 300, 260
    img = _image(w, h)
    bias = {"all-negative": np.random.default_rng(5).uniform(-2.0, -0.1, (h, w)), "constant-negative": np.full((h, w), -1.0),
            "constant-zero": None, "constant-positive": np.full((h, w), 1.5)}[kind]
    for o in (0, 1):
        c = _carver(eng, img, nrg=L.LQR_EF_NULL, bias=bias)
        true = c.get_energy(o, true=True)
        norm = c.get_energy(o)
        assert np.array_equal(bits(norm), bits(EC.normalised(true)))
        if kind == "all-negative":
            assert (true < 0).all() and norm.min() == 0 and 0.5 < norm.max() < 1
        elif kind == "constant-positive":
            assert len(np.unique(norm)) == 1 and 0 < norm[0, 0] < 1         # e_max == e_min: the squashed value stays
        else:
            assert not norm.any()
        pic = c.get_energy_image(o, L.LQR_COLDEPTH_8I, L.LQR_CMYK_IMAGE)
        assert np.array_equal(pic, EC.picture(true, L.LQR_COLDEPTH_8I, L.LQR_CMYK_IMAGE))
        if kind.startswith("constant"):
            assert (pic[:, :, 3] == 255).all() and not pic[:, :, :3].any()      # the picture of a constant plane is that of 0
        c.destroy()


# ---- the device forms ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("o", [0, 1])
def test_device_forms_equal_the_host_forms_also_one_element_off_an_allocation(eng, o):
    import torch
    w, h = 131, 67                                   # odd: no row of the result is vector-aligned but the first
    img = _image(w, h)
    a = _carver(eng, img)
    want_true, want_norm = a.get_energy(o, true=True), a.get_energy(o)
    formats = [(L.LQR_COLDEPTH_8I, L.LQR_RGBA_IMAGE, torch.uint8), (L.LQR_COLDEPTH_8I, L.LQR_RGB_IMAGE, torch.uint8),
               (L.LQR_COLDEPTH_16I, L.LQR_RGBA_IMAGE, torch.int16), (L.LQR_COLDEPTH_16I, L.LQR_CMYKA_IMAGE, torch.int16),
               (L.LQR_COLDEPTH_32F, L.LQR_RGBA_IMAGE, torch.float32), (L.LQR_COLDEPTH_32F, L.LQR_CMY_IMAGE, torch.float32),
               (L.LQR_COLDEPTH_64F, L.LQR_GREYA_IMAGE, torch.float64), (L.LQR_COLDEPTH_64F, L.LQR_CMYKA_IMAGE, torch.float64)]
    want_pic = [a.get_energy_image(o, d, t) for d, t, _ in formats]
    a.destroy()
    for off in (0, 1):
        c = _carver(eng, img)
        for true, want in ((True, want_true), (False, want_norm)):
            block = torch.full((w * h + off + 16,), -7.0, dtype=torch.float32, device="cuda")
            t = block[off:off + w * h]
            assert c.get_energy_device(t, o, true=true) == 1 and c.getters()["orientation"] == o
            got = block.cpu().numpy()
            assert np.array_equal(bits(got[off:off + w * h].reshape(h, w)), bits(want)), (off, true)
            assert (got[:off] == -7).all() and (got[off + w * h:] == -7).all()       # nothing before or behind it
        for (d, ty, dt), want in zip(formats, want_pic):
            n = w * h * L.IMAGE_TYPE_CHANNELS[ty]
            block = torch.zeros((n + off + 16,), dtype=dt, device="cuda")
            t = block[off:off + n]
            assert c.get_energy_image_device(t, o, d, ty) == 1
            got = block.cpu().numpy()
            assert np.array_equal(bits(got[off:off + n].view(want.dtype).reshape(want.shape)), bits(want)), (off, d, ty)
            assert not got[:off].any() and not got[off + n:].any()
        assert eng.lqrx_carver_get_energy_image_device(c.p, t.data_ptr(), o, 0, L.LQR_CUSTOM_IMAGE) == 0
        assert eng.lqrx_carver_get_energy_device(c.p, None, o, 1) == 0 and eng.lqrx_carver_get_energy_device(c.p, t.data_ptr(), 2, 1) == 0
        c.destroy()


# ---- allocation failures ------------------------------------------------------------------------------------------------------
def test_an_allocation_failure_at_every_point_of_a_read_out_leaves_a_usable_carver(eng):
    lib = eng.lib
    lib.lqrhip_debug_fail_alloc.argtypes = [ctypes.c_int]
    lib.lqrhip_debug_pool_live.restype, lib.lqrhip_debug_pool_live.argtypes = ctypes.c_ulonglong, []
    w, h = 70, 66
    img = _image(w, h)
    ref = _carver(eng, img)
    want = ref.get_energy(1)
    assert ref.resize(w - 5, h) == 1
    want_image = ref.read_image_ext()
    ref.destroy()
    gc.collect()            # (a carver that an earlier, failed test left to the collector would go while the blocks are counted)
    failures = 0
    try:
        for n in range(64):
            live = lib.lqrhip_debug_pool_live()     # device blocks handed out and not given back: the iteration leaves none behind
            c = _carver(eng, img)
            lib.lqrhip_debug_fail_alloc(n)
            ret, buf = c.energy_call(1, 1, nbytes=4 * w * h, guard=16)
            lib.lqrhip_debug_fail_alloc(-1)
            if ret == L.LQR_OK:
                assert np.array_equal(bits(buf[:4 * w * h].view(np.float32).reshape(h, w)), bits(want))
                c.destroy()
                assert lib.lqrhip_debug_pool_live() == live, n
                break
            assert ret == L.LQR_NOMEM, (n, ret)
            failures += 1
            assert (buf == 0xa5).all(), n                                   # nothing was written
            g = c.getters()
            assert (g["width"], g["height"]) == (w, h) and g["orientation"] in (0, 1), (n, g)      # as it was, or transposed
            assert np.array_equal(c.read_image_ext(), img), n              # ... and still serves its image
            assert np.array_equal(bits(c.get_energy(1)), bits(want)), n    # asked again: the exact result
            assert c.resize(w - 5, h) == 1 and np.array_equal(c.read_image_ext(), want_image), n
            c.destroy()
            assert lib.lqrhip_debug_pool_live() == live, n
        else:
            raise AssertionError("the read-out never got through")
    finally:
        lib.lqrhip_debug_fail_alloc(-1)
    print("allocation sweep energy-read-out: %d failure points" % failures)
    assert failures >= 4, failures          # the transposed planes, the working planes, the partials, the staging block


# ---- the C caller -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("o", [0, 1])
def test_energy_replay_c_reproduces_the_vector(eng, tmp_path, o):
    d = os.path.join(ROOT, "gimp-lqr-plugin_amd")
    exe = str(tmp_path / "energy_replay")
    subprocess.run(["gcc", "-std=c99", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "energy_replay.c"), "-o", exe, "-L" + d, "-l:liblqr-hip.so", "-Wl,-rpath," + d, "-lm"],
                   check=True)
    spec, z = load(next(v for v in MANIFEST["vectors"] if v["name"] == "late_alone"))
    img = z["img"]
    h, w, ch = img.shape
    (tmp_path / "in.bin").write_bytes(np.array([w, h, ch, spec["nrg"], o], np.int32).tobytes() + np.ascontiguousarray(img).tobytes())
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    raw = (tmp_path / "out.bin").read_bytes()
    assert tuple(np.frombuffer(raw[:12], np.int32)) == (w, h, o)
    n = w * h
    true = np.frombuffer(raw[12:12 + 4 * n], np.float32).reshape(h, w)
    norm = np.frombuffer(raw[12 + 4 * n:12 + 8 * n], np.float32).reshape(h, w)
    rgba = np.frombuffer(raw[12 + 8 * n:], np.uint8).reshape(h, w, 4)
    key = {0: "true@0", 1: "out@1"}[o]                      # late_alone: ["norm", 0], ["true", 1], ["image", 1, 8I, RGBA]
    assert np.array_equal(bits(true), bits(z[key]))
    assert np.array_equal(bits(norm), bits(EC.normalised(true)))
    assert np.array_equal(rgba, EC.picture(true, 0, IT.RGBA))
    if o == 0:
        assert np.array_equal(bits(norm), bits(z["out@0"]))
    else:
        assert np.array_equal(rgba, z["out@2"])
