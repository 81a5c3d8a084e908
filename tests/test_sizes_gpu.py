"""A carver read at many sizes in one pass (include/lqr_sizes.h) on the MI355X.  Every output buffer, on the device and on the host,
is followed (and, where it starts off an aligned address, preceded) by guard bytes that are checked after every call.

1. the genuine liblqr's vectors under tests/golden/vmap/: after each successful load all sizes of the recorded resizes that follow
   are asked for in one call, without resizing, and compared with the recorded images byte for byte;
2. seeded permutation maps against the numpy model (tests/sizes_cases.py) at the boundaries of the kernels;
3. carved carvers (two sessions, then an enlargement; delta_x 1 and 2; an attached carver) against the CPU oracle resized to each
   size and against a twin engine carver driven through lqr_carver_resize + lqrx_carver_read_image, and the carver afterwards;
4. every refusal of the header; 5. a failure of every device allocation of one call.

About vector depth_len_minus_2 (12 columns, depth 10, recorded at widths 2, 7, 22 and 15): the issue this file answers expected width 22
to lie outside the range, beyond delta_max = 5 at the enlargement step 1.5 the vectors configure.  It does not: lqr_vmap_load sets the
step to 2.0, as liblqr does (the vectors' getters record it; tests/test_vmap_abi.py), so delta_max is 11, the range is [2, 22] and
lqr_carver_resize serves 22 -- every recorded image of every vector is inside the range and is compared.  The refusal the issue asks
for is tested where its premise holds: with the step set back to 1.5 after the load the range ends at 17 and 22 returns LQR_ERROR."""
import ctypes
import json
import os

import numpy as np
import pytest

import coldepth_cases as CD
import datasets as D
import lqr_ctypes as L
import sizes_cases as SC
import vmap_cases as VC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "vmap")
MANIFEST = json.load(open(os.path.join(GOLD, "MANIFEST.json")))
GUARD, PAT = 64, 0xA5
COMPACT, TRANSPOSE, SLOTS = 29, 30, 32         # include/lqr_hip.h LQRHIP_CENSUS_COMPACT_SIZES, _TRANSPOSE_SIZES, _SLOTS
bits = CD.bits


@pytest.fixture(scope="module")
def eng():
    return L.bind_sizes(L.bind_vmap(L.bind_imagetype(L.engine_api())))


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


class Outputs:
    """guarded output buffers for one call: `offset` samples of guard in front of each image (so that it starts one sample off an
    aligned address) and GUARD bytes behind it, all filled with PAT"""

    def __init__(self, c, sizes, device, offset=0):
        import torch
        self.dt = c._px()[0]
        self.shapes = [c._sizes_shape(max(s, 1)) for s in sizes]          # (a refused size of 0 or less still gets a buffer)
        self.front = offset * self.dt.itemsize
        self.nbytes = [int(np.prod(sh)) * self.dt.itemsize for sh in self.shapes]
        self.device = device
        if device:
            self.bufs = [torch.full((self.front + n + GUARD,), PAT, dtype=torch.uint8, device="cuda") for n in self.nbytes]
            base = [b.data_ptr() for b in self.bufs]
            torch.cuda.synchronize()
        else:
            self.bufs = [np.full(self.front + n + GUARD, PAT, np.uint8) for n in self.nbytes]
            base = [b.ctypes.data for b in self.bufs]
        assert all(p % 16 == 0 for p in base)
        self.ptrs = [p + self.front for p in base]

    def host(self, k):
        return self.bufs[k].cpu().numpy() if self.device else self.bufs[k]

    def guards_intact(self):
        return all((self.host(k)[:self.front] == PAT).all() and (self.host(k)[self.front + n:] == PAT).all() for k, n in enumerate(self.nbytes))

    def untouched(self):
        return all((self.host(k) == PAT).all() for k in range(len(self.bufs)))

    def image(self, k):
        return self.host(k)[self.front:self.front + self.nbytes[k]].copy().view(self.dt).reshape(self.shapes[k])


def call(eng, c, sizes, device=True, offset=0, outs=None):
    """one call into fresh guarded buffers: (LqrRetVal, Outputs)"""
    o = outs or Outputs(c, sizes, device, offset)
    arr = (ctypes.c_int * max(len(sizes), 1))(*sizes)
    ptrs = (ctypes.c_void_p * max(len(sizes), 1))(*o.ptrs)
    fn = eng.lqrx_carver_read_sizes_device if o.device else eng.lqrx_carver_read_sizes
    return fn(c.p, arr, len(sizes), ptrs), o


def read(eng, c, sizes, device=True, offset=0):
    ret, o = call(eng, c, sizes, device, offset)
    assert ret == L.LQR_OK and o.guards_intact(), (ret, sizes)
    return [o.image(k) for k in range(len(sizes))]


def fresh(eng, img, depth, max_ch=None):
    prev = eng.lqrx_set_max_channels(max_ch) if max_ch else None
    try:
        return L.Carver.from_ext(eng, img, depth, init=False)
    finally:
        if prev is not None:
            eng.lqrx_set_max_channels(prev)


# ---- 1. the genuine vectors ---------------------------------------------------------------------------------------------------
def _vector(name):
    entry = next(v for v in MANIFEST["vectors"] if v["name"] == name)
    z = np.load(os.path.join(GOLD, entry["file"]))
    return z, json.loads(str(z["spec"])), json.loads(str(z["record"]))


def _carver_of(eng, spec, z):
    img, extra = VC.make_input(spec)
    assert np.array_equal(img, z["img"])
    prev = VC._raise_channels(eng, spec)
    try:
        c = L.Carver.from_ext(eng, img, spec["depth"], init=False)
        aux = c.attach_ext(extra["aux"], 0) if "aux" in extra else None
    finally:
        VC._restore_channels(eng, prev)
    c.configure(nrg_func=spec.get("nrg", 2), res_order=0, switch_freq=2, enl_step=1.5)
    return c, aux


@pytest.mark.parametrize("name", [v["name"] for v in MANIFEST["vectors"]])
def test_genuine_vector_every_recorded_size_after_a_load_in_one_call(eng, name):
    z, spec, rec = _vector(name)
    d, o = rec["map_meta"]
    vmap = dict(data=z["map"], depth=d, orientation=o)
    c, aux = _carver_of(eng, spec, z)
    compared = 0
    for i, op in enumerate(spec["ops"]):
        if op[0] == "load":
            ret = c.vmap_load(vmap)
            if ret == 1:
                # the recorded resizes that follow, up to the next load or init
                follow = []
                for j in range(i + 1, len(spec["ops"])):
                    if spec["ops"][j][0] in ("load", "init"):
                        break
                    if spec["ops"][j][0] == "resize" and rec["rets"][j] == 1:
                        follow.append(j)
                sizes = [spec["ops"][j][2] if o else spec["ops"][j][1] for j in follow]
                length = spec["h"] if o else spec["w"]
                assert c.size_range() == (o, length - d, length + d) and all(length - d <= s <= length + d for s in sizes), name
                before = c.getters()
                for device in (True, False):
                    got = read(eng, c, sizes, device)
                    for j, g in zip(follow, got):
                        assert same(g, z["image@%d" % j]), (name, j, device)
                        compared += 1
                    if aux is not None:
                        assert aux.size_range() == c.size_range()
                        for j, g in zip(follow, read(eng, aux, sizes, device)):
                            assert same(g, z["aux_image@%d" % j]), (name, j, device)
                assert c.getters() == before
        elif op[0] == "resize":
            ret = c.resize(op[1], op[2])
        elif op[0] == "init":
            ret = c.init(spec.get("delta", 1), spec.get("rigidity", 0.0))
        else:
            ret = c.vmap_internal_dump()
        assert ret == rec["rets"][i], (name, i)
    assert compared >= 2
    c.destroy()


def test_genuine_vector_beyond_delta_max_is_refused(eng):
    """depth_len_minus_2 with the enlargement step set back to 1.5 after the load (see the module's docstring): delta_max is
    (int) (0.5 * 12) - 1 = 5, the range [2, 17]; width 22 is a stepwise enlargement and is refused, the other recorded sizes are served"""
    z, spec, rec = _vector("depth_len_minus_2")
    c, _ = _carver_of(eng, spec, z)
    assert c.vmap_load(dict(data=z["map"], depth=rec["map_meta"][0], orientation=0)) == 1
    assert c.size_range() == (0, 2, 22)
    assert eng.lqr_carver_set_enl_step(c.p, 1.5) == 1 and c.size_range() == (0, 2, 17)
    recorded = {op[1]: "image@%d" % i for i, op in enumerate(spec["ops"]) if op[0] == "resize"}
    assert sorted(recorded) == [2, 7, 15, 22]
    for device in (True, False):
        for sizes in ([22], [2, 7, 22, 15]):
            ret, o = call(eng, c, sizes, device)
            assert ret == L.LQR_ERROR and o.untouched(), (sizes, device)
        for s, g in zip([2, 7, 15, 17], read(eng, c, [2, 7, 15, 17], device)):
            assert same(g, z[recorded[s]] if s in recorded else VC.model(z["img"], dict(data=z["map"], depth=10, orientation=0), s)), s
    c.destroy()


# ---- 2. the numpy model ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SC.cases(), ids=lambda c: c["name"])
def test_permutation_map_every_size_equals_the_model(eng, lib, case):
    img, m, sizes = SC.image_of(case), SC.map_of(case), SC.sizes_of(case)
    ch, depth, max_ch = SC.PIXELS[case["px"]]
    c = fresh(eng, img, depth, max_ch)
    assert c.vmap_load(m) == 1
    assert c.size_range() == (case["o"], case["line"] - case["d"], case["line"] + case["d"])
    want = {s: SC.fast_model(img, m, s) for s in set(sizes)}
    for offset in case["offsets"]:
        census(lib)
        got = read(eng, c, sizes, True, offset)
        ran = census(lib)
        chunks = (len(sizes) + SC.MAX_JOBS - 1) // SC.MAX_JOBS
        assert ran[COMPACT] == chunks and ran[TRANSPOSE] == (chunks if case["o"] else 0) and sum(ran) == ran[COMPACT] + ran[TRANSPOSE]
        for s, g in zip(sizes, got):
            assert same(g, want[s]), (case["name"], offset, s)
    # the host form, once
    for s, g in zip(sizes, read(eng, c, sizes, False)):
        assert same(g, want[s]), (case["name"], "host", s)
    c.destroy()


def test_binding_methods(eng):
    import torch
    case = dict(line=60, lines=20, d=9, o=1, px=4)
    img, m = SC.image_of(case), SC.map_of(case)
    c = fresh(eng, img, 0)
    assert c.vmap_load(m) == 1 and c.size_range() == (1, 51, 69)
    sizes = [69, 51, 60, 51]
    tensors = [torch.zeros(c._sizes_shape(s), dtype=torch.uint8, device="cuda") for s in sizes]
    assert c.read_sizes_device(sizes, tensors) == L.LQR_OK
    for s, t, a in zip(sizes, tensors, c.read_sizes(sizes)):
        want = SC.fast_model(img, m, s)
        assert a.shape == (s, 20, 4) and same(a, want) and same(t.cpu().numpy(), want), s
    with pytest.raises(ValueError):
        c.read_sizes([70])
    c.destroy()


# ---- 3. carved carvers ----------------------------------------------------------------------------------------------------------
def _along(w, h, o, size):
    return (size, h) if o == 0 else (w, size)


@pytest.mark.parametrize("delta", [1, 2])
@pytest.mark.parametrize("o", [0, 1])
def test_carved_carver_equals_the_oracle_and_the_old_pair_of_calls_and_is_left_as_it_was(eng, oracle, o, delta):
    w, h = (60, 40) if o == 0 else (40, 60)
    img, img2 = D.photo_like(w, h, 21 + delta), D.noise(w, h, 5)
    length = h if o else w
    trio = []
    for api in (eng, eng, oracle):
        c = L.Carver(api, img, delta_x=delta)
        c.attach(img2)
        c.configure(enl_step=1.5)
        trio.append(c)
    a, twin, orc = trio
    # shrink, deeper, an enlargement beyond what the maps hold (a third session)
    for target, depth in ((length - 6, 6), (length - 13, 13), (length + 17, 17)):
        for c in trio:
            assert c.resize(*_along(w, h, o, target)) == L.LQR_OK
        lo, hi = length - depth, length + depth
        assert a.size_range() == (o, lo, hi) and a.aux[0].size_range() == (o, lo, hi)
        sizes = list(range(lo, hi + 1))
        before = (a.getters(), a.aux[0].getters(), a.read_image(), a.aux[0].read_image())
        assert before[0]["width" if o == 0 else "height"] == target
        got = read(eng, a, sizes, True)
        got_aux = read(eng, a.aux[0], sizes, False)
        assert a.getters() == before[0] and a.aux[0].getters() == before[1]
        assert same(a.read_image(), before[2]) and same(a.aux[0].read_image(), before[3])
        for s, g, ga in zip(sizes, got, got_aux):
            for other in (twin, orc):
                assert other.resize(*_along(w, h, o, s)) == L.LQR_OK
                assert same(g, other.read_image()) and same(ga, other.aux[0].read_image()), (target, s, other is orc)
        for other in (twin, orc):
            assert other.resize(*_along(w, h, o, target)) == L.LQR_OK
        assert twin.getters() == a.getters() == orc.getters()
    # a further resize, into a fourth session, is what it is without the calls
    for c in trio:
        assert c.resize(*_along(w, h, o, length - 20)) == L.LQR_OK
    assert same(a.read_image(), orc.read_image()) and same(a.read_image(), twin.read_image()) and same(a.aux[0].read_image(), orc.aux[0].read_image())
    assert np.array_equal(a.vmap_dump()["data"], orc.vmap_dump()["data"])
    for c in trio:
        c.destroy()


def test_a_scan_in_progress_goes_on_where_it_was(eng):
    img = D.photo_like(50, 30, 3)
    c = L.Carver(eng, img)
    c.configure()
    assert c.resize(44, 30) == L.LQR_OK
    whole = c.read_image()
    n, line = ctypes.c_int(0), ctypes.c_void_p()
    L.bind_coldepth(eng)
    seen = []
    for _ in range(7):
        assert eng.lqr_carver_scan_line_ext(c.p, ctypes.byref(n), ctypes.byref(line))
        seen.append((n.value, ctypes.string_at(line.value, 44 * 4)))
    read(eng, c, [44, 50, 47], True)
    read(eng, c, [45], False)
    while eng.lqr_carver_scan_line_ext(c.p, ctypes.byref(n), ctypes.byref(line)):
        seen.append((n.value, ctypes.string_at(line.value, 44 * 4)))
    assert [k for k, _ in seen] == list(range(30))
    assert b"".join(b for _, b in seen) == whole.tobytes()
    c.destroy()


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("o", [0, 1])
def test_refusals_return_error_and_write_nothing(eng, lib, o):
    case = dict(line=70, lines=45, d=9, o=o, px=4)
    img, m = SC.image_of(case), SC.map_of(case)
    c = fresh(eng, img, 0)
    assert c.size_range() == (0, img.shape[1], img.shape[1])                         # a flat carver: its own size
    assert [same(g, img) for g in read(eng, c, [img.shape[1]] * 2, True)] == [True, True]
    assert c.vmap_load(m) == 1
    lo, hi = 61, 79
    assert c.size_range() == (o, lo, hi)
    live = lib.lqrhip_debug_pool_live()
    census(lib)
    for device in (True, False):
        for sizes in ([lo - 1], [hi + 1], [lo, hi, hi + 1], [lo - 1, lo], [0], [-5, lo]):
            ret, outs = call(eng, c, sizes, device)
            assert ret == L.LQR_ERROR and outs.untouched(), (sizes, device)
        # n = 0, n < 0; NULL carver, sizes, output array; one NULL output pointer
        outs = Outputs(c, [lo, hi], device)
        arr, ptrs = (ctypes.c_int * 2)(lo, hi), (ctypes.c_void_p * 2)(*outs.ptrs)
        fn = eng.lqrx_carver_read_sizes_device if device else eng.lqrx_carver_read_sizes
        assert fn(c.p, arr, 0, ptrs) == L.LQR_ERROR and fn(c.p, arr, -1, ptrs) == L.LQR_ERROR
        assert fn(None, arr, 2, ptrs) == L.LQR_ERROR and fn(c.p, None, 2, ptrs) == L.LQR_ERROR and fn(c.p, arr, 2, None) == L.LQR_ERROR
        holed = (ctypes.c_void_p * 2)(outs.ptrs[0], None)
        assert fn(c.p, arr, 2, holed) == L.LQR_ERROR
        assert outs.untouched()
    assert census(lib) == [0] * SLOTS and lib.lqrhip_debug_pool_live() == live
    # a smaller enlargement step lowers the upper end: (int) (0.1f * 70) - 1 = 6 (the float product is 7.0000005)
    assert eng.lqr_carver_set_enl_step(c.p, 1.1) == 1
    assert c.size_range() == (o, lo, 76)
    ret, outs = call(eng, c, [77], True)
    assert ret == L.LQR_ERROR and outs.untouched()
    assert same(read(eng, c, [76], True)[0], SC.fast_model(img, m, 76))
    lo_only, hi_only = ctypes.c_int(0), ctypes.c_int(0)
    assert eng.lqrx_carver_size_range(c.p, ctypes.byref(lo_only), None) == o and eng.lqrx_carver_size_range(c.p, None, ctypes.byref(hi_only)) == o
    assert (lo_only.value, hi_only.value) == (lo, 76)
    c.destroy()


# ---- 5. allocation failures -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [True, False])
def test_every_allocation_of_a_call_fails_in_turn(eng, lib, device):
    """direction 1, 65 sizes: two chunks.  The nth device allocation of the call fails, once, for every n until the call gets through:
    LQR_NOMEM, nothing written, the pool's count where it was, the carver as it was; the same call again is exact"""
    case = dict(line=70, lines=45, d=33, o=1, px=4)
    img, m = SC.image_of(case), SC.map_of(case)
    c = fresh(eng, img, 0)
    assert c.vmap_load(m) == 1
    sizes = [int(s) for s in np.random.default_rng(9).permutation(np.arange(37, 104))[:65]]
    want = [SC.fast_model(img, m, s) for s in sizes]
    before = (c.getters(), c.read_image_ext())
    live = lib.lqrhip_debug_pool_live()
    failures = 0
    for n in range(20):
        outs = Outputs(c, sizes, device)
        census(lib)
        lib.lqrhip_debug_fail_alloc(n)
        ret, _ = call(eng, c, sizes, outs=outs)
        lib.lqrhip_debug_fail_alloc(-1)
        if ret == L.LQR_OK:
            assert outs.guards_intact() and all(same(outs.image(k), want[k]) for k in range(65))
            ran = census(lib)
            assert ran[COMPACT] == 2 and ran[TRANSPOSE] == 2
            break
        failures += 1
        assert ret == L.LQR_NOMEM and outs.untouched() and lib.lqrhip_debug_pool_live() == live, n
        assert c.getters() == before[0] and same(c.read_image_ext(), before[1])
        ret, outs = call(eng, c, sizes, device)
        assert ret == L.LQR_OK and outs.guards_intact() and all(same(outs.image(k), want[k]) for k in range(65)), n
        assert lib.lqrhip_debug_pool_live() == live
    else:
        pytest.fail("the call never got through")
    print("allocation sweep (device outputs: %s): %d failure points" % (device, failures))
    assert failures >= 2 and lib.lqrhip_debug_pool_live() == live
    c.destroy()
