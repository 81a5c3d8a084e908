"""Deep-colour carvers (16I, 32F, 64F) past the sizes where their kernels change structure: base layouts of more than 256 and 512
columns (second and third chunk of the rank loops of k_wk_init_visible<PixValue<D>>, k_frozen_catchup<true>, k_inflate<true>, k_compact<true>,
k_compact_jobs<true>), more than 62 and 124 rows (blocks of k_emap_update<N, NT, true>), sessions longer than the frozen lag (32 seams up to
four carvers, 128 beyond: catch-up in mid-session, log walks from an epoch > 0), delta_x 3 .. 10 (the 36- and 68-sample
instantiations).  tests/test_coldepth_abi.py asserts from the specs that the vectors cross each of these.  Every comparison is
bit for bit.

* every vector the genuine liblqr 0.4.1 recorded under tests/golden/coldepth_mid/ is reproduced;
* the energy plane after the full build (lqrx_carver_get_energy) and the energy, cumulative-minimum and back-pointer planes after
  40 and 70 incremental seams (lqrx_set_debug / debug_snapshot) equal the planes read out of the genuine engine's memory.  (The
  engine has no hook that shows m and the back pointers before the first seam: the full build is compared on its energies.);
* families of same-shape vectors carved as one lqrx_carver_resize_batch, a mixed 8I / 16I / 32F / 64F list, batch -> enlarge ->
  flatten against single carvers;
* identities between depths at 257 .. 600 x 63 .. 200 with 33 .. 150 seams, seeded, every energy: the 8-bit lifts against the
  oracle; 16I v against 64F v / 65535.0 (deep_norm<1> is a correctly rounded division: the same doubles are read); 32F f against
  64F (double) f.  Enlargements (one direction, one step): the vmaps only, each depth averages new pixels in its own precision;
* recovery from an injected seam-log fault in a session of a carver that is not flat, wider than 256 columns;
* 3840 x 2160 RGBA, 200 seams: the 8-bit engine, 16I v * 257 and 64F v / 255.0 give one vmap and the lifted pixels.
"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import coldepth_cases as CD
import lqr_ctypes as L

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "coldepth_mid")
MANIFEST = json.load(open(os.path.join(GOLD, "MANIFEST.json")))
VECTORS = {v["name"]: v for v in MANIFEST["vectors"]}
PLANES = {v["name"]: v for v in MANIFEST["planes"]}
bits, assert_same_record = CD.bits, CD.assert_same_record


@pytest.fixture(scope="module")
def eng():
    return L.bind_coldepth(L.engine_api())


def load(name):
    z = np.load(os.path.join(GOLD, VECTORS[name]["file"]))
    spec = json.loads(str(z["spec"]))
    extra = {k[3:]: z[k] for k in z.files if k.startswith("in_")}
    return spec, z["img"], extra, z


# ---- 1. the vectors ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(VECTORS))
def test_genuine_mid_vector_is_reproduced(eng, name):
    spec, img, extra, z = load(name)
    got = CD.run(eng, L.Carver, spec, img, extra)
    assert_same_record(got, z, name)
    if spec.get("preserve"):
        assert json.loads(str(got["record"]))["input_unchanged"] is True


# ---- 2. planes --------------------------------------------------------------------------------------------------------------------
def same_plane(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    diff = np.argwhere(got.view(np.int32) != want.view(np.int32))
    assert diff.size == 0, "%s: %d values differ, the first at row %d column %d" % (what, len(diff), diff[0][0], diff[0][1])


@pytest.mark.parametrize("name", list(PLANES))
def test_deep_planes_equal_the_genuine_engines_memory(eng, name):
    import hashlib
    z = np.load(os.path.join(GOLD, PLANES[name]["file"]))
    spec = json.loads(str(z["spec"]))
    img, _ = CD.make_input(dict(spec, steps=[]))
    assert hashlib.sha1(np.ascontiguousarray(img).tobytes()).hexdigest() == str(z["input_sha1"]), "the input is not the recorded one"

    def carver():
        c = L.Carver.from_ext(eng, img, spec["depth"], delta_x=spec.get("delta", 1), rigidity=spec.get("rigidity", 0.0))
        return c.configure(nrg_func=spec["nrg"], switch_freq=0)
    eng.lqrx_set_debug(1)
    try:
        c = carver()
        same_plane(c.energy(), z["build_en"], name + ": energies after the full build")
        c.destroy()
        for k in CD.PLANE_SEAMS:
            c = carver()
            assert c.resize(spec["w"] - k, spec["h"]) == L.LQR_OK
            en, m, dx = c.debug_snapshot()
            c.destroy()
            what = "%s after %d seams: " % (name, k)
            same_plane(en, z["en%d" % k], what + "energies")
            same_plane(m, z["m%d" % k], what + "cumulative minima (m)")
            want = z["dx%d" % k].astype(np.int32)
            ok = want[1:] != -999                   # (the genuine plane keeps pointers to pixels that are out of reach by now: none recorded)
            assert PLANES[name]["stale"][str(k)] == int((~ok).sum())
            assert np.array_equal(dx[1:][ok], want[1:][ok]), what + "back pointers"
    finally:
        eng.lqrx_set_debug(0)


# ---- 3. a scan given up part-way ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["inter_16i", "enl_multistep_32f", "all3_64f"])
def test_a_scan_given_up_part_way_restarts_after_a_resize_wide(eng, name):
    spec, img, extra, z = load(name)
    got = CD.run(eng, L.Carver, spec, img, extra, partial=True)
    assert_same_record(got, z, name + ", scans given up before each resize")


# ---- 4. groups ----------------------------------------------------------------------------------------------------------------------
def against_vector(c, z, what):
    v = c.vmap_dump()
    rec = json.loads(str(z["record"]))
    assert [v["depth"], v["orientation"]] == rec["vmap_meta"][0], what
    assert np.array_equal(v["data"], z["vmap0"]), what + ": vmap"
    got = c.read_image_ext()
    assert got.dtype == z["image0"].dtype and np.array_equal(bits(got), bits(z["image0"])), what + ": pixels"


@pytest.mark.parametrize("depth,n", [(1, 5), (1, 8), (2, 5), (3, 5)])
def test_family_carved_as_one_group_equals_each_vector(eng, depth, n):
    """140 seams in a group of 5 (8): past the lag of 128 such a group has; 8: k_band_levels feeding k_carve + k_emap_update<N, NT, true>"""
    names = CD.family_names(depth)[:n]
    loaded = [load(x) for x in names]
    spec = loaded[0][0]
    cs = [L.Carver.from_ext(eng, img, depth).configure(nrg_func=spec["nrg"]) for _, img, _, _ in loaded]
    assert L.resize_batch(eng, cs, *spec["steps"][0]) == L.LQR_OK
    for name, c, (_, _, _, z) in zip(names, cs, loaded):
        against_vector(c, z, "%s in a group of %d" % (name, n))
        c.destroy()


def test_mixed_list_of_all_four_depths_at_one_geometry(eng):
    orc = L.oracle_api()
    spec = dict(CD.FAMILY_SHAPE)
    nw, nh = spec["steps"][0]
    rng = np.random.default_rng(77)
    eight = [CD.base_image(rng, spec["w"], spec["h"], spec["ch"]) for _ in range(2)]
    deep = [load(CD.family_names(d)[i]) for i in range(2) for d in (1, 2, 3)]
    order = [("8i", eight[0]), deep[0], deep[1], deep[2], ("8i", eight[1]), deep[3], deep[4], deep[5]]
    cs = [L.Carver.from_ext(eng, x[1]).configure(nrg_func=spec["nrg"]) for x in order]
    assert L.resize_batch(eng, cs, nw, nh) == L.LQR_OK
    for i, (c, x) in enumerate(zip(cs, order)):
        if x[0] == "8i":
            o = L.Carver(orc, x[1]).configure(nrg_func=spec["nrg"])
            assert o.resize(nw, nh) == L.LQR_OK
            assert np.array_equal(c.vmap_dump()["data"], o.vmap_dump()["data"]), i
            assert np.array_equal(c.read_image_ext(), o.read_image()), i
            o.destroy()
        else:
            against_vector(c, x[3], "carver %d of the mixed list" % i)
        c.destroy()


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_batch_then_enlarge_then_flatten_equals_single_carvers(eng, depth):
    """a group of 5 wide deep carvers through shrink (read-out: k_compact_jobs<true>), enlarge (k_inflate<true> with five jobs) and flatten"""
    rng = np.random.default_rng(300 + depth)
    imgs = [CD.to_depth(rng, CD.base_image(rng, 300, 24, 3), depth, edge=(i % 2 == 0)) for i in range(5)]

    def snap(c):
        return c.read_image_ext(), c.vmap_dump()["data"]

    def same(a, b, what):
        assert np.array_equal(bits(a[0]), bits(b[0])), what + ": pixels"
        assert np.array_equal(a[1], b[1]), what + ": vmap"
    group = [L.Carver.from_ext(eng, a).configure(nrg_func=1) for a in imgs]
    single = [L.Carver.from_ext(eng, a).configure(nrg_func=1) for a in imgs]
    for step, (nw, nh) in enumerate([(262, 24), (340, 24)]):
        assert L.resize_batch(eng, group, nw, nh) == L.LQR_OK
        for i, (g, s) in enumerate(zip(group, single)):
            assert s.resize(nw, nh) == L.LQR_OK
            same(snap(g), snap(s), "carver %d after step %d" % (i, step))
    for i, (g, s) in enumerate(zip(group, single)):
        assert g.flatten() == L.LQR_OK and s.flatten() == L.LQR_OK
        assert np.array_equal(bits(g.read_image_ext()), bits(s.read_image_ext())), i
    assert L.resize_batch(eng, group, 300, 24) == L.LQR_OK
    for i, (g, s) in enumerate(zip(group, single)):
        assert s.resize(300, 24) == L.LQR_OK
        same(snap(g), snap(s), "carver %d after the flatten" % i)
        g.destroy(); s.destroy()


# ---- 5. identities between depths ---------------------------------------------------------------------------------------------------
MID_SEEDS = 6


def carve(c, nw, nh, kw):
    c.configure(**kw)
    assert c.resize(nw, nh) == L.LQR_OK
    return c


def same_vmap(a, b, what):
    va, vb = a.vmap_dump(), b.vmap_dump()
    assert (va["depth"], va["orientation"]) == (vb["depth"], vb["orientation"]) and np.array_equal(va["data"], vb["data"]), what + ": vmap"


@pytest.mark.parametrize("nrg", range(7))
def test_lift_identities_mid(eng, nrg):
    orc = L.oracle_api()
    for seed in range(MID_SEEDS):
        img, nw, nh, kw, enlarge = CD.lift_case(seed, nrg, mid=True)
        what = "nrg %d seed %d %s -> %dx%d" % (nrg, seed, img.shape, nw, nh)
        o = carve(L.Carver(orc, img), nw, nh, kw)
        e16 = carve(L.Carver.from_ext(eng, img.astype(np.uint16) * 257), nw, nh, kw)
        e64 = carve(L.Carver.from_ext(eng, img.astype(np.float64) / 255.0), nw, nh, kw)
        same_vmap(e16, o, what + " 16I")
        same_vmap(e64, o, what + " 64F")
        if not enlarge:
            i8 = o.read_image()
            assert np.array_equal(e16.read_image_ext(), i8.astype(np.uint16) * 257), what + ": 16I pixels"
            assert np.array_equal(bits(e64.read_image_ext()), bits(i8.astype(np.float64) / 255.0)), what + ": 64F pixels"
        for c in (o, e16, e64):
            c.destroy()


@pytest.mark.parametrize("nrg", range(7))
def test_16i_and_32f_against_64f_mid(eng, nrg):
    for seed in range(MID_SEEDS):
        base, nw, nh, kw, enlarge = CD.lift_case(seed, nrg, mid=True)
        rng = np.random.default_rng(900000 + 100 * nrg + seed)
        what = "nrg %d seed %d %s -> %dx%d" % (nrg, seed, base.shape, nw, nh)
        u = CD.to_depth(rng, base, 1, edge=True)
        f = CD.to_depth(rng, base, 2, edge=True)
        for tag, lo, hi in (("16I", u, u.astype(np.float64) / 65535.0), ("32F", f, f.astype(np.float64))):
            a = carve(L.Carver.from_ext(eng, lo), nw, nh, kw)
            b = carve(L.Carver.from_ext(eng, hi), nw, nh, kw)
            same_vmap(a, b, "%s %s against 64F" % (what, tag))
            if not enlarge:
                pa = a.read_image_ext()
                lifted = pa.astype(np.float64) / 65535.0 if tag == "16I" else pa.astype(np.float64)
                assert np.array_equal(bits(lifted), bits(b.read_image_ext())), "%s: %s pixels against 64F" % (what, tag)
            a.destroy(); b.destroy()


# ---- 6. fault recovery --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["all2_32f", "all3_64f"])
def test_injected_fault_in_a_wide_session_that_is_not_flat_is_rolled_back_and_exact(eng, name):
    """lqrhip_debug_inject(3, 40, 1): a seam-log entry out of the frame at seam step 40 of the first session that has one.  The
    vector's first session has 38 seams, so the fault falls into the second (42 seams), after its catch-up in mid-session, on a
    carver with a base layout of more than 256 (512) columns that is not flat: the levels are rolled back and the value plane laid
    out again from the visible pixels (k_wk_init_visible<PixValue<D>> over more than one chunk) for the session carved again"""
    lb = eng.lib
    lb.lqrhip_debug_inject.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int]
    lb.lqrhip_fault_stats.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
    st = (ctypes.c_ulonglong * 8)()
    spec, img, extra, z = load(name)
    w = spec["w"]
    assert [w - s[0] for s in spec["steps"][:2]] == [38, 80]
    lb.lqrhip_fault_stats(st, 1)
    try:
        lb.lqrhip_debug_inject(3, 40, 1)
        got = CD.run(eng, L.Carver, spec, img, extra)
    finally:
        lb.lqrhip_debug_inject(0, 0, 0)
    lb.lqrhip_fault_stats(st, 0)
    assert st[5] == 1 and st[4] >= 1 and st[6] >= 1, list(st)      # injected, rolled back, redone
    assert_same_record(got, z, name + " after an injected fault")


# ---- 8. full size -------------------------------------------------------------------------------------------------------------------
def fullsize_lift_check():
    """3840 x 2160 RGBA -> 3640: parallel backtrack, k_carve and k_emap_update<N, 12, true> on 35 blocks of rows; 265 MB of 64F pixels.
    One deep carver at a time"""
    import datasets as D
    eng = L.bind_coldepth(L.engine_api())
    img = D.noise(3840, 2160, 3)
    c = L.Carver(eng, img).configure()
    assert c.resize(3640, 2160) == L.LQR_OK
    vm, out = c.vmap_dump()["data"], c.read_image()
    c.destroy()
    assert out.shape == (2160, 3640, 4) and ((vm > 0).sum(axis=1) == 200).all()
    for tag, lift in (("16I", lambda a: a.astype(np.uint16) * 257), ("64F", lambda a: a.astype(np.float64) / 255.0)):
        deep = lift(img)
        c = L.Carver.from_ext(eng, deep).configure()
        del deep
        assert c.resize(3640, 2160) == L.LQR_OK
        assert np.array_equal(c.vmap_dump()["data"], vm), tag + ": vmap"
        got = c.read_image_ext()
        c.destroy()
        assert np.array_equal(bits(got), bits(lift(out))), tag + ": pixels"
        del got
    print("fullsize lift ok")


def test_fullsize_4k_rgba_lifts_carve_the_8_bit_seams():
    """(the 8-bit engine at this size is pinned to the oracle and to the genuine vectors by tests/test_ref_golden.py and test_round3_gpu.py)"""
    r = subprocess.run([sys.executable, "-c", "import test_coldepth_mid_gpu as T; T.fullsize_lift_check()"], cwd=os.path.join(ROOT, "tests"),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "fullsize lift ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
