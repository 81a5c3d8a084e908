"""Carvers of CMY, CMYK, CMYKA and custom-channel pixels (include/lqr_imagetype.h) on the MI355X.

* every vector the genuine liblqr 0.4.1 recorded under tests/golden/imgtype/ is reproduced bit for bit: pixels, the order of
  lqr_carver_scan_ext, line scans, vmaps, dumped vmaps, getters (the image type among them), progress events and what every
  setter returned;
* the value-plane identity, seeded: a typed carver and a one-channel 64F carver whose pixels are the values the typed one's
  energy reads (imgtype_cases.model_value, which tests/test_imgtype_abi.py pins to the genuine read functions bit for bit)
  carve the same visibility maps under all seven energies; on shrinks the typed carver's pixels are the input's pixels, selected
  as the 64F carver selects the pixels of an attached index image;
* one cross-check of the packed 8-bit path against the value-plane path (CMY against RGB on the inverted image);
* groups and mixed lists through lqrx_carver_resize_batch, recovery from an injected fault on a carver of 5-byte pixels that is
  not flat, 64 channels, and tests/c/cmyka_replay.c linked to the engine.
"""
import contextlib
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import coldepth_cases as CD
import imgtype_cases as IT
import lqr_ctypes as L

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "imgtype")
MANIFEST = json.load(open(os.path.join(GOLD, "MANIFEST.json")))
VECTORS = {v["name"]: v for v in MANIFEST["vectors"] + MANIFEST["mid"]}
bits = CD.bits


@pytest.fixture(scope="module")
def eng():
    return L.bind_imagetype(L.engine_api())


@contextlib.contextmanager
def channel_limit(eng, n):
    prev = eng.lqrx_set_max_channels(n)
    try:
        yield
    finally:
        eng.lqrx_set_max_channels(prev)


def load(name):
    z = np.load(os.path.join(GOLD, VECTORS[name]["file"]))
    spec = json.loads(str(z["spec"]))
    extra = {k[3:]: z[k] for k in z.files if k.startswith("in_") and not k.startswith("in_read_")}
    return spec, z["img"], extra, z


def assert_same_record(got, z, what):
    class View:         # the vector without the read planes (inputs of the CPU suite)
        files = [k for k in z.files if not k.startswith("in_read_")]

        def __getitem__(self, k):
            return z[k]
    IT.assert_same_record(got, View(), what)


@pytest.mark.parametrize("name", [v["name"] for v in MANIFEST["vectors"] + MANIFEST["mid"]])
def test_genuine_vector_is_reproduced(eng, name):
    spec, img, extra, z = load(name)
    got = IT.run(eng, L.Carver, spec, img, extra)
    assert_same_record(got, z, name)
    if spec.get("preserve"):
        assert json.loads(str(got["record"]))["input_unchanged"] is True


def test_five_channels_are_refused_under_the_default_limit_and_cmyka_above_it(eng):
    img = np.zeros((8, 8, 5), np.float32)
    with pytest.raises(MemoryError):
        L.Carver.from_ext(eng, img)
    with channel_limit(eng, 5):
        c = L.Carver.from_ext(eng, img)
        assert c.getters_ext()["image_type"] == L.LQR_CMYKA_IMAGE
        c.destroy()
        with pytest.raises(MemoryError):
            L.Carver.from_ext(eng, np.zeros((8, 8, 6), np.uint8))


# ---- the value-plane identity -------------------------------------------------------------------------------------------------
def typed(eng, img, depth, ops, **kw):
    with channel_limit(eng, 64):
        c = L.Carver.from_ext(eng, img, depth, **kw)
    for op in ops:
        assert IT._apply(c, op) == L.LQR_OK
    return c


def identity_check(eng, img, depth, ops, st, nw, nh, kw, enlarge, what):
    """the typed carver against the 64F carver of its values, which drags an index image along"""
    h, w = img.shape[:2]
    luma = kw["nrg_func"] in (3, 4, 5)
    t = typed(eng, img, depth, ops).configure(**kw)
    v = L.Carver.from_ext(eng, IT.model_value(img, depth, st, luma)[:, :, None], 3)
    idx = v.attach_ext(np.arange(h * w, dtype=np.float32).reshape(h, w, 1), 2)
    v.configure(**kw)
    assert t.resize(nw, nh) == L.LQR_OK and v.resize(nw, nh) == L.LQR_OK
    a, b = t.vmap_dump(), v.vmap_dump()
    assert (a["depth"], a["orientation"]) == (b["depth"], b["orientation"]) and np.array_equal(a["data"], b["data"]), what + ": vmap"
    if not enlarge:
        sel = idx.scan_ext()[0][:, :, 0].astype(np.int64)
        want = img.reshape(h * w, -1)[sel]
        got = t.read_image_ext()
        assert got.dtype == img.dtype and np.array_equal(bits(got), bits(want)), what + ": pixels"
    t.destroy(); v.destroy()


@pytest.mark.parametrize("nrg", range(7))
def test_value_plane_identity(eng, nrg):
    for seed in range(9):
        img, depth, ops, st, nw, nh, kw, enlarge = IT.identity_case(seed, nrg)
        identity_check(eng, img, depth, ops, st, nw, nh, kw, enlarge, "nrg %d seed %d %s depth %d %s" % (nrg, seed, img.shape, depth, st.key()))


@pytest.mark.parametrize("nrg", range(7))
def test_value_plane_identity_mid(eng, nrg):
    """257 .. 600 columns, 63 .. 200 rows, 33 .. 150 seams: 14 cases over the seven energies"""
    for seed in range(2):
        img, depth, ops, st, nw, nh, kw, enlarge = IT.identity_case(seed + 2 * nrg, nrg, mid=True)
        identity_check(eng, img, depth, ops, st, nw, nh, kw, enlarge, "mid nrg %d seed %d %s depth %d %s" % (nrg, seed, img.shape, depth, st.key()))


@pytest.mark.parametrize("depth", [0, 3])
def test_sixty_four_channels_shrink_and_enlarge(eng, depth):
    rng = np.random.default_rng(640 + depth)
    img = CD.to_depth(rng, CD.base_image(rng, 40, 28, 64), depth)
    for ops in ([], [{"alpha": 63}, {"black": 17}]):
        st = IT.TypeState(64)
        for op in ops:
            st.apply(op)
        for nw, nh, enlarge in ((31, 24, False), (52, 28, True)):
            identity_check(eng, img, depth, ops, st, nw, nh, dict(nrg_func=0 if ops else 4), enlarge, "64 channels depth %d %s" % (depth, st.key()))


def test_8i_cmy_carves_the_seams_of_8i_rgb_on_the_inverted_image(eng):
    """The packed 8-bit path against the value-plane path.  An 8I CMY carver reads ((1 - c/255) + (1 - m/255) + (1 - y/255)) / 3
    through the value plane; the 8I RGB carver of 255 - image reads (((255 - c)/255 + (255 - m)/255) + (255 - y)/255) / 3 from its
    packed pixels.  1 - v/255 and (255 - v)/255 are the same real number, rounded once each way: the two values differ by an ulp of
    a double (2^-53 relative) at the most, GRAD_XABS takes |difference of two of them| (halved inside the image) and rounds it to
    float (2^-24): the energies, and with them every seam, are equal unless a gradient lies within 2^-50 of the midpoint of two
    floats (about one gradient in 2^26).  The input is seeded; on it the genuine liblqr carves equal maps and complementary pixels too"""
    rng = np.random.default_rng(4242)
    img = CD.base_image(rng, 60, 40, 3)
    a = typed(eng, img, 0, [IT.CMY]).configure(nrg_func=L.LQR_EF_GRAD_XABS)
    b = L.Carver(eng, 255 - img).configure(nrg_func=L.LQR_EF_GRAD_XABS)
    for nw, nh in ((48, 40), (44, 33)):
        assert a.resize(nw, nh) == L.LQR_OK and b.resize(nw, nh) == L.LQR_OK
        assert np.array_equal(a.vmap_dump()["data"], b.vmap_dump()["data"])
        assert np.array_equal(a.read_image_ext(), 255 - b.read_image())
    a.destroy(); b.destroy()


# ---- groups and lists ---------------------------------------------------------------------------------------------------------
def snap(c):
    return c.read_image_ext(), c.vmap_dump()["data"]


def same(a, b, what):
    assert a[0].dtype == b[0].dtype and np.array_equal(bits(a[0]), bits(b[0])), what + ": pixels"
    assert np.array_equal(a[1], b[1]), what + ": vmap"


def batch_against_singles(eng, inputs, steps, nrg=1):
    """inputs: [(img, depth, ops)]: carved as one lqrx_carver_resize_batch list and one by one"""
    group = [typed(eng, img, depth, ops).configure(nrg_func=nrg) for img, depth, ops in inputs]
    single = [typed(eng, img, depth, ops).configure(nrg_func=nrg) for img, depth, ops in inputs]
    for step, (nw, nh) in enumerate(steps):
        assert L.resize_batch(eng, group, nw, nh) == L.LQR_OK
        for i, (g, s) in enumerate(zip(group, single)):
            assert s.resize(nw, nh) == L.LQR_OK
            same(snap(g), snap(s), "carver %d after step %d" % (i, step))
    for g, s in zip(group, single):
        g.destroy(); s.destroy()


@pytest.mark.parametrize("n,depth,ch,ops", [(5, 0, 5, []), (8, 2, 7, [{"alpha": 5}, {"black": 2}]), (5, 1, 4, [IT.CMYK]), (8, 0, 6, [])])
def test_same_shape_typed_carvers_as_a_group(eng, n, depth, ch, ops):
    """shrink (read-out of odd pixels by k_compact<true>), then enlarge (k_inflate<true> with n jobs), past 256 columns"""
    rng = np.random.default_rng(500 + n + depth)
    inputs = [(CD.to_depth(rng, CD.base_image(rng, 280, 20, ch), depth, edge=(i % 2 == 0)), depth, ops) for i in range(n)]
    batch_against_singles(eng, inputs, [(246, 20), (300, 20)])


def test_list_mixing_types_of_four_channel_carvers(eng):
    """one shape, one depth, one channel count: CMYK (value plane), RGBA (packed pixels), CUSTOM with alpha -- the host splits what
    does not read alike"""
    rng = np.random.default_rng(600)
    kinds = [[IT.CMYK], [], [{"alpha": 1}], [], [IT.CMYK], [{"alpha": 1}]]
    for depth in (0, 2):
        inputs = [(CD.to_depth(rng, CD.base_image(rng, 56, 36, 4), depth), depth, ops) for ops in kinds]
        batch_against_singles(eng, inputs, [(45, 30), (60, 30)], nrg=3)


def test_list_mixing_channel_counts(eng):
    rng = np.random.default_rng(601)
    inputs = [(CD.to_depth(rng, CD.base_image(rng, 56, 36, ch), 2), 2, []) for ch in (5, 3, 6, 5, 9, 4, 6)]
    batch_against_singles(eng, inputs, [(47, 29), (58, 29)], nrg=0)


# ---- recovery, C --------------------------------------------------------------------------------------------------------------
def test_injected_fault_on_an_8i_cmyka_carver_that_is_not_flat_is_rolled_back_and_exact(eng):
    """lqrhip_debug_inject(3, 40, 1): a seam-log entry out of the frame at seam step 40.  The vector's first session has 38 seams, so
    the fault falls into the second (42 seams, after the type change that laid the planes out again), on a carver of 5-byte pixels
    with a base layout of 378 columns that is not flat: the levels are rolled back, the value plane is laid out again from the
    visible pixels (k_wk_init_visible<PixValue<0>> over two chunks) and the session carved again.  The type is not session state"""
    lb = eng.lib
    lb.lqrhip_debug_inject.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int]
    lb.lqrhip_fault_stats.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
    st = (ctypes.c_ulonglong * 8)()
    spec, img, extra, z = load("all2_cmyka_8i")
    assert [spec["w"] - s[0] for s in spec["steps"][:2]] == [38, 80] and spec["depth"] == 0 and spec["ch"] == 5
    lb.lqrhip_fault_stats(st, 1)
    try:
        lb.lqrhip_debug_inject(3, 40, 1)
        got = IT.run(eng, L.Carver, spec, img, extra)
    finally:
        lb.lqrhip_debug_inject(0, 0, 0)
    lb.lqrhip_fault_stats(st, 0)
    assert st[5] == 1 and st[4] >= 1 and st[6] >= 1, list(st)      # injected, rolled back, redone
    assert_same_record(got, z, "all2_cmyka_8i after an injected fault")


def test_cmyka_replay_c_reproduces_its_vector(tmp_path):
    d = os.path.join(ROOT, "gimp-lqr-plugin_amd")
    exe = str(tmp_path / "cmyka_replay")
    subprocess.run(["gcc", "-std=c99", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "cmyka_replay.c"), "-o", exe, "-L" + d, "-l:liblqr-hip.so", "-Wl,-rpath," + d, "-lm"],
                   check=True)
    spec, img, extra, z = load("cmyka_replay_32f")
    nw, nh = spec["steps"][0]
    h, w, ch = img.shape
    assert ch == 5
    (tmp_path / "in.bin").write_bytes(np.array([w, h, nw, nh], np.int32).tobytes() + np.ascontiguousarray(img, np.float32).tobytes())
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    raw = (tmp_path / "out.bin").read_bytes()
    gw, gh, n = np.frombuffer(raw[:12], np.int32)
    assert (gw, gh, n) == (nw, nh, nw * nh)
    pix = np.frombuffer(raw[12:12 + 20 * nw * nh], np.float32).reshape(nh, nw, 5)
    order = np.frombuffer(raw[12 + 20 * nw * nh:], np.int32).reshape(-1, 2)
    assert np.array_equal(bits(pix), bits(z["image0"]))
    assert np.array_equal(order, z["order0"])
