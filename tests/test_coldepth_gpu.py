"""Carvers of 16-bit, float and double pixels (lqr_carver_new_ext, include/lqr_coldepth.h) on the MI355X.

* every vector the genuine liblqr 0.4.1 recorded under tests/golden/coldepth/ is reproduced bit for bit: pixels (float bit
  patterns included), the order and coordinates of lqr_carver_scan_ext, line scans, vmaps, dumped vmaps, getters, progress
  events, the 8-bit scans' FALSE on deep carvers, and a preserved input buffer left as it was;
* lift identities against the 8-bit engine and the 8-bit oracle, on seeded cases per energy: a 16I image v * 257 and a 64F
  image v / 255.0 carve the seams of the 8-bit image v (257 / 65535 = 1 / 255 exactly, and both correctly rounded divisions give
  the same double); shrunk, their pixels are the 8-bit result lifted the same way.  Enlargement (one direction, one step): the
  vmaps only (new pixels follow the depth's own averaging).  32F is not lifted: (float) (v / 255) is not v / 255;
* batches of deep carvers, a mixed 8I / 32F list, recovery from an injected fault on a 32F carver, and tests/c/float_replay.c
  linked to the engine.
"""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import coldepth_cases as CD
import lqr_ctypes as L

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "coldepth")
MANIFEST = json.load(open(os.path.join(GOLD, "MANIFEST.json")))
VECTORS = {v["name"]: v for v in MANIFEST["vectors"]}


@pytest.fixture(scope="module")
def eng():
    return L.bind_coldepth(L.engine_api())


def load(name):
    z = np.load(os.path.join(GOLD, VECTORS[name]["file"]))
    spec = json.loads(str(z["spec"]))
    extra = {k[3:]: z[k] for k in z.files if k.startswith("in_")}
    return spec, z["img"], extra, z


bits, assert_same_record = CD.bits, CD.assert_same_record


@pytest.mark.parametrize("name", sorted(VECTORS))
def test_genuine_vector_is_reproduced(eng, name):
    spec, img, extra, z = load(name)
    got = CD.run(eng, L.Carver, spec, img, extra)
    assert_same_record(got, z, name)
    if spec.get("preserve"):
        assert json.loads(str(got["record"]))["input_unchanged"] is True


# ---- lift identities ------------------------------------------------------------------------------------------------------
lift_case = CD.lift_case


def carve(c, nw, nh, kw):
    c.configure(**kw)
    assert c.resize(nw, nh) == L.LQR_OK
    return c


@pytest.mark.parametrize("nrg", range(7))
def test_lift_identities(eng, nrg):
    orc = L.oracle_api()
    for seed in range(60):
        img, nw, nh, kw, enlarge = lift_case(seed, nrg)
        what = "nrg %d seed %d %s" % (nrg, seed, img.shape)
        o = carve(L.Carver(orc, img), nw, nh, kw)
        e8 = carve(L.Carver(eng, img), nw, nh, kw)
        e16 = carve(L.Carver.from_ext(eng, img.astype(np.uint16) * 257), nw, nh, kw)
        e64 = carve(L.Carver.from_ext(eng, img.astype(np.float64) / 255.0), nw, nh, kw)
        vo = o.vmap_dump()
        for c, tag in ((e8, "8I"), (e16, "16I"), (e64, "64F")):
            v = c.vmap_dump()
            assert (v["depth"], v["orientation"]) == (vo["depth"], vo["orientation"]) and np.array_equal(v["data"], vo["data"]), "%s: %s vmap" % (what, tag)
        i8 = o.read_image()
        assert np.array_equal(e8.read_image(), i8), what
        if not enlarge:
            assert np.array_equal(e16.read_image_ext(), i8.astype(np.uint16) * 257), what + ": 16I pixels"
            assert np.array_equal(bits(e64.read_image_ext()), bits(i8.astype(np.float64) / 255.0)), what + ": 64F pixels"
        for c in (o, e8, e16, e64):
            c.destroy()


# ---- preserve, batches, recovery, C ---------------------------------------------------------------------------------------
def test_preserved_buffer_is_untouched_and_still_the_callers(eng):
    rng = np.random.default_rng(5)
    img = CD.to_depth(rng, CD.base_image(rng, 64, 40, 4), 2, edge=True)
    c = L.Carver.from_ext(eng, img, preserve=True)
    before = c.buffer.tobytes()
    c.configure(nrg_func=0)
    assert c.resize(50, 33) == L.LQR_OK
    c.scan_ext(); c.scan_line_ext(); c.read_image_ext()
    assert c.resize(70, 33) == L.LQR_OK
    c.scan_ext()
    c.destroy()
    assert c.buffer.tobytes() == before


def batch_images(n, depth, seed):
    rng = np.random.default_rng(seed)
    return [CD.to_depth(rng, CD.base_image(rng, 56, 36, 4), depth, edge=(i % 3 == 0)) for i in range(n)]


def single(eng, arr, nw, nh):
    c = L.Carver.from_ext(eng, arr)
    c.configure(nrg_func=2)
    assert c.resize(nw, nh) == L.LQR_OK
    out = (c.read_image_ext(), c.vmap_dump()["data"])
    c.destroy()
    return out


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_batch_of_16_deep_carvers_equals_one_by_one(eng, depth):
    imgs = batch_images(16, depth, 40 + depth)
    cs = [L.Carver.from_ext(eng, a).configure(nrg_func=2) for a in imgs]
    assert L.resize_batch(eng, cs, 45, 30) == L.LQR_OK
    for i, (c, a) in enumerate(zip(cs, imgs)):
        want = single(eng, a, 45, 30)
        assert np.array_equal(bits(c.read_image_ext()), bits(want[0])), i
        assert np.array_equal(c.vmap_dump()["data"], want[1]), i
        c.destroy()


def test_mixed_8i_and_32f_list(eng):
    imgs = batch_images(3, 2, 7) + batch_images(3, 0, 8)
    order = [imgs[0], imgs[3], imgs[1], imgs[4], imgs[2], imgs[5]]
    cs = [L.Carver.from_ext(eng, a).configure(nrg_func=2) for a in order]
    assert L.resize_batch(eng, cs, 47, 29) == L.LQR_OK
    for i, (c, a) in enumerate(zip(cs, order)):
        want = single(eng, a, 47, 29)
        assert np.array_equal(bits(c.read_image_ext()), bits(want[0])), i
        assert np.array_equal(c.vmap_dump()["data"], want[1]), i
        c.destroy()


def test_injected_fault_on_a_32f_carver_is_rolled_back_and_exact(eng):
    lb = eng.lib
    lb.lqrhip_debug_inject.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int]
    lb.lqrhip_fault_stats.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
    st = (ctypes.c_ulonglong * 8)()
    lb.lqrhip_fault_stats(st, 1)
    spec, img, extra, z = load("all_32f_e2")
    try:
        lb.lqrhip_debug_inject(3, 3, 1)           # a seam-log entry out of the frame at seam step 3
        got = CD.run(eng, L.Carver, spec, img, extra)
    finally:
        lb.lqrhip_debug_inject(0, 0, 0)
    lb.lqrhip_fault_stats(st, 0)
    assert st[5] == 1 and st[4] >= 1 and st[6] >= 1, list(st)      # injected, rolled back, redone
    assert_same_record(got, z, "all_32f_e2 after an injected fault")


def test_float_replay_c_reproduces_its_vector(tmp_path):
    d = os.path.join(ROOT, "gimp-lqr-plugin_amd")
    exe = str(tmp_path / "float_replay")
    subprocess.run(["gcc", "-std=c99", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "float_replay.c"), "-o", exe, "-L" + d, "-l:liblqr-hip.so", "-Wl,-rpath," + d, "-lm"],
                   check=True)
    spec, img, extra, z = load("float_replay_32f")
    nw, nh = spec["steps"][0]
    h, w, _ = img.shape
    (tmp_path / "in.bin").write_bytes(np.array([w, h, nw, nh], np.int32).tobytes() + np.ascontiguousarray(img, np.float32).tobytes())
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    raw = (tmp_path / "out.bin").read_bytes()
    gw, gh, n = np.frombuffer(raw[:12], np.int32)
    assert (gw, gh, n) == (nw, nh, nw * nh)
    pix = np.frombuffer(raw[12:12 + 16 * nw * nh], np.float32).reshape(nh, nw, 4)
    order = np.frombuffer(raw[12 + 16 * nw * nh:], np.int32).reshape(-1, 2)
    assert np.array_equal(bits(pix), bits(z["image0"]))
    assert np.array_equal(order, z["order0"])


SMALL, WIDE = (44, 30, 38, 31, 26), (300, 70, 262, 225, 64)


@pytest.mark.parametrize("first,second,size", [pytest.param(0, 3, SMALL, id="0-3"), pytest.param(4, 1, SMALL, id="4-1"), pytest.param(2, 5, SMALL, id="2-5"),
                                               pytest.param(0, 3, WIDE, id="0-3-wide"), pytest.param(4, 1, WIDE, id="4-1-wide"), pytest.param(2, 5, WIDE, id="2-5-wide")])
def test_energy_function_changed_between_resizes(eng, first, second, size):
    """brightness and luma are different read values: a deep carver whose energy function changes kind between two resizes
    lays its value plane out again (lift identity against the 8-bit oracle, which reads pixels afresh every time).  wide: the
    carver that is laid out again has a base layout of 338 columns and is not flat (k_wk_init_visible<PixValue<D>> over two chunks), and
    the session that follows is longer than the frozen lag; 16I as well as 64F"""
    orc = L.oracle_api()
    w, h, w1, w2, h2 = size
    rng = np.random.default_rng(first * 10 + second)
    img = CD.base_image(rng, w, h, 4)
    o, e = L.Carver(orc, img), L.Carver.from_ext(eng, img.astype(np.float64) / 255.0)
    cs = [o, e] + ([L.Carver.from_ext(eng, img.astype(np.uint16) * 257)] if size is WIDE else [])
    for c in cs:
        c.configure(nrg_func=first)
        assert c.resize(w1, h) == L.LQR_OK
        assert c.api.lqr_carver_set_energy_function_builtin(c.p, second) == L.LQR_OK
        assert c.resize(w2, h2) == L.LQR_OK
    assert np.array_equal(e.vmap_dump()["data"], o.vmap_dump()["data"])
    assert np.array_equal(bits(e.read_image_ext()), bits(o.read_image().astype(np.float64) / 255.0))
    for c in cs[2:]:
        assert np.array_equal(c.vmap_dump()["data"], o.vmap_dump()["data"])
        assert np.array_equal(c.read_image_ext(), o.read_image().astype(np.uint16) * 257)
    for c in cs:
        c.destroy()


@pytest.mark.parametrize("name", ["interactive_16i", "interactive_32f", "interactive_64f", "edge_16i", "d16i_c3_e5", "enl_vert_32f"])
def test_a_scan_given_up_part_way_restarts_after_a_resize(eng, name):
    """a lqr_carver_scan_ext loop stopped near the end of the first line, then a resize to a narrower frame: the next loop, without a
    scan_reset, visits the whole new image from its first pixel, as liblqr's cursor does (checked on the genuine code: the record
    equals the plain run's)"""
    spec, img, extra, z = load(name)
    got = CD.run(eng, L.Carver, spec, img, extra, partial=True)
    assert_same_record(got, z, name + ", scans given up before each resize")


def test_64f_reload_device_read_out_and_transposed_read_image(eng):
    """the byte counts of a deep carver's other transfers: lqrx_carver_read_image on a transposed carver with a cached read-out,
    lqrx_carver_reload_device_batch (device-to-device copy of w x h x ch x 8 bytes) and lqrx_carver_read_image_device"""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(9)
    w, h = 72, 48
    first = CD.to_depth(rng, CD.base_image(rng, w, h, 4), 3, edge=True)
    second = CD.to_depth(rng, CD.base_image(rng, w, h, 4), 3, edge=True)
    c = L.Carver.from_ext(eng, first).configure(nrg_func=0)
    assert c.resize(60, 40) == L.LQR_OK
    assert c.getters()["orientation"] == 1                        # the last direction carved was the height: transposed
    im, _ = c.scan_ext()                                          # caches the read-out
    assert np.array_equal(bits(c.read_image_ext()), bits(im))
    dev = torch.from_numpy(second).cuda()
    assert L.reload_device_batch(eng, [c], [dev.data_ptr()]) == L.LQR_OK
    g = c.getters()
    assert (g["width"], g["height"], g["orientation"], g["depth"]) == (w, h, 0, 0)
    assert c.resize(61, h) == L.LQR_OK
    fresh = L.Carver.from_ext(eng, second).configure(nrg_func=0)
    assert fresh.resize(61, h) == L.LQR_OK
    want = fresh.scan_ext()[0]
    assert np.array_equal(bits(c.read_image_ext()), bits(want))
    assert np.array_equal(c.vmap_dump()["data"], fresh.vmap_dump()["data"])
    out = torch.zeros((h, 61, 4), dtype=torch.float64, device="cuda")
    assert eng.lqrx_carver_read_image_device(c.p, out.data_ptr()) == L.LQR_OK
    torch.cuda.synchronize()
    assert np.array_equal(bits(out.cpu().numpy()), bits(want))
    c.destroy(); fresh.destroy()
