"""An allocation failure at every allocation point of the one-off calls that no other sweep reaches (-m gpu): the 8-bit and the
computed mask calls, a queued run of _xy values flushed by a plane read-out, the plane read-out of a transposed carver, the image and
visibility-map read-outs, the auto-size guess and the seam-map colour ramp.

For each call lqrhip_debug_fail_alloc(n) is armed for n = 0, 1, ... until the call gets through, on a fresh 64 x 48 RGB carver each
time (where the call has a path of its own for a transposed carver, on one whose frame is 48 x 64 as well).  Each time:
  * the failed call returns what EXPECT says for that n, and lqrhip_debug_pool_live() -- device blocks handed out and not given back --
    is what it was before the call, plus what EXPECT says: the one exception is the mask plane that lqrhip_mask_plane_ensure created
    before a later allocation of the same call failed; the carver keeps it (it is zero, or holds what was added so far);
  * the same call repeated succeeds and gives, bit for bit, what a carver that never saw a failure gives;
  * after the carver is destroyed the live count is what it was before it was made.
EXPECT was recorded from a run of the engine as it was before device blocks had owners (lqr_own.h), with only the counting hook
added: the returns, the live-block differences and the number of failure points are that engine's, call by call
(profiles/ownership/README.md).  A call without a failure point fails the test: the sweep would
have checked nothing for it."""
import ctypes
import gc

import numpy as np
import pytest

import lqr_ctypes as L

pytestmark = pytest.mark.gpu

W, H = 64, 48
NOMEM = L.LQR_NOMEM


@pytest.fixture(scope="module")
def eng():
    api = L.bind_energy(L.bind_masks(L.engine_api()))
    api.lib.lqrhip_debug_fail_alloc.argtypes = [ctypes.c_int]
    api.lib.lqrhip_debug_pool_live.restype, api.lib.lqrhip_debug_pool_live.argtypes = ctypes.c_ulonglong, []
    yield api
    api.lib.lqrhip_debug_fail_alloc(-1)


def _image():
    return np.random.default_rng(64048).integers(0, 256, (H, W, 3), dtype=np.uint8)


def _fresh(eng, transposed):
    c = L.Carver(eng, _image()).configure()
    if transposed:                  # a read-out as vertical seams see it leaves the carver transposed: its frame is 48 x 64
        c.get_energy(1, true=True)
        assert c.getters()["orientation"] == 1
    return c


RNG = np.random.default_rng(7)
MASK8 = RNG.integers(0, 256, (H - 7, W - 5, 3), dtype=np.uint8)                # laid over the image at (3, 2): clipped on no side
MASKF = RNG.uniform(-3.0, 3.0, (H - 6, W - 9))
XY = [(int(x), int(y), float(v)) for x, y, v in zip(RNG.integers(0, W, 40), RNG.integers(0, H, 40), RNG.uniform(-9, 9, 40))]
GUESS = np.zeros((H, W, 3), np.uint8)
GUESS[5:30, 10:33] = 255                                                        # 23 columns, 25 rows of mask


def _bias_rgb_area(eng, c):
    return c.bias_add(MASK8, 700, 3, 2), None                   # (what it did is read once nothing is armed any more: get_bias)


def _bias_area_double(eng, c):
    return c.bias_add_f(MASKF, 450, 4, 1), None


def _bias_area_float(eng, c):
    """float values reach the engine from device memory only (lqrx_carver_bias_add_area_device)"""
    import torch
    return c.bias_add_device(torch.tensor(MASKF, dtype=torch.float32, device="cuda"), 450, 4, 1), None


def _queue_xy(eng, c):
    assert c.bias_add_xy(XY) == [L.LQR_OK] * len(XY)            # the first call makes the plane; the values wait on the host


def _flush_by_get_bias(eng, c):
    out = np.zeros((H, W), np.float32)
    ret = eng.lqrx_carver_get_bias(c.p, out.ctypes.data)
    return ret, out


def _add_rigmask(eng, c):
    assert c.rigmask_add_f(MASKF, 4, 1) == L.LQR_OK


def _get_rigmask(eng, c):
    out = np.zeros((H, W), np.float32)
    ret = eng.lqrx_carver_get_rigmask(c.p, out.ctypes.data)
    return ret, out


def _read_image(eng, c):
    out = np.zeros((H, W, 3), np.uint8)
    ret = eng.lqrx_carver_read_image(c.p, out.ctypes.data)
    return ret, out


def _vmap_dump(eng, c):
    v = eng.lqr_vmap_dump(c.p)
    if not v:
        return None, None
    d = c._vmap_to_dict(v)
    eng.lqr_vmap_destroy(v)
    return L.LQR_OK, d["data"]


def _guess(direction):
    def call(eng, c):
        got = eng.lqrx_guess_new_size(GUESS.ctypes.data, 3, W, H, 0, 0, W, H, direction)
        # (the call has no return value of its own for a failure: it answers the old size, which no mask with a set pixel gives)
        return (L.LQR_OK if got != (H if direction else W) else "old size"), np.array([got], np.int32)
    return call


def _vmap_to_rgba(eng, c):
    v = c.dumped                                                # (_carve_and_dump: the dump allocates too)
    out = np.zeros((eng.lqr_vmap_get_height(v), eng.lqr_vmap_get_width(v), 4), np.uint8)
    cs, ce = (ctypes.c_double * 3)(1.0, 1.0, 0.0), (ctypes.c_double * 3)(0.2, 0.0, 0.0)
    return eng.lqrx_vmap_to_rgba(v, cs, ce, out.ctypes.data), out


def _carve_width(eng, c):
    assert c.resize(W - 6, H) == L.LQR_OK                       # six levels in the visibility map


def _carve_and_dump(eng, c):
    _carve_width(eng, c)
    c.dumped = eng.lqr_vmap_dump(c.p)
    assert c.dumped


def _carve_height(eng, c):
    assert c.resize(W, H - 6) == L.LQR_OK and c.getters()["orientation"] == 1      # ... of a carver that is transposed for it


# name: (transposed, what is done before the allocation is armed, the call, [(return, live blocks more than before) per failure point])
# "plane kept": the call made the carver's bias plane (lqrhip_mask_plane_ensure) before its staging block failed
EXPECT = {
    "bias_add_rgb_area": (False, None, _bias_rgb_area, [(NOMEM, 0), (NOMEM, 1)]),                   # the plane; the mask's staging block: plane kept
    "bias_add_rgb_area-transposed": (True, None, _bias_rgb_area, [(NOMEM, 0), (NOMEM, 1)]),
    "bias_add_area-double": (False, None, _bias_area_double, [(NOMEM, 0), (NOMEM, 1)]),             # likewise
    "bias_add_area-double-transposed": (True, None, _bias_area_double, [(NOMEM, 0), (NOMEM, 1)]),
    "bias_add_area-float-device": (False, None, _bias_area_float, [(NOMEM, 0)]),                    # the plane; device memory is not staged
    "bias_add_xy-flushed-by-get_bias": (False, _queue_xy, _flush_by_get_bias, [(NOMEM, 0), (NOMEM, 0)]),        # indices, values
    "bias_add_xy-flushed-by-get_bias-transposed": (True, _queue_xy, _flush_by_get_bias, [(NOMEM, 0), (NOMEM, 0), (NOMEM, 0)]),   # and the transposed copy
    "get_rigmask-transposed": (True, _add_rigmask, _get_rigmask, [(NOMEM, 0)]),
    "read_image": (False, None, _read_image, [(NOMEM, 0)]),
    "read_image-transposed": (True, None, _read_image, [(NOMEM, 0)]),
    "vmap_dump": (False, _carve_width, _vmap_dump, [(None, 0)]),                                    # (NULL)
    "vmap_dump-transposed": (False, _carve_height, _vmap_dump, [(None, 0)]),
    "guess_new_size-width": (False, None, _guess(0), [("old size", 0), ("old size", 0)]),           # the mask, the result word
    "guess_new_size-height": (False, None, _guess(1), [("old size", 0), ("old size", 0)]),
    "vmap_to_rgba": (False, _carve_and_dump, _vmap_to_rgba, [(NOMEM, 0), (NOMEM, 0)]),                         # the map, the picture
}


@pytest.mark.parametrize("name", list(EXPECT))
def test_an_allocation_failure_at_every_point_of_a_one_off_call(eng, name):
    transposed, before, call, expect = EXPECT[name]
    lib = eng.lib
    live = lambda: int(lib.lqrhip_debug_pool_live())

    def made():
        c = _fresh(eng, transposed)
        if before:
            before(eng, c)
        return c

    def result(c, got):
        return c.get_bias() if got is None else got

    def destroyed(c):
        if getattr(c, "dumped", None):
            eng.lqr_vmap_destroy(c.dumped)
        c.destroy()
    gc.collect()                    # (a carver that an earlier, failed test left to the collector would go while this one counts)
    base = live()
    c = made()
    ret, want = call(eng, c)
    assert ret == L.LQR_OK
    want = result(c, want)
    destroyed(c)
    assert live() == base
    seen = []
    try:
        for n in range(16):
            c = made()
            before_call = live()
            lib.lqrhip_debug_fail_alloc(n)
            ret, got = call(eng, c)
            lib.lqrhip_debug_fail_alloc(-1)
            if ret != L.LQR_OK:
                seen.append((ret, live() - before_call))
                ret, got = call(eng, c)                         # asked again
            assert ret == L.LQR_OK, (name, n)
            got = result(c, got)
            assert got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8)), (name, n)
            destroyed(c)
            assert live() == base, (name, n)                    # nothing of the carver is left
            if len(seen) <= n:
                break
        else:
            raise AssertionError("the call never got through")
    finally:
        lib.lqrhip_debug_fail_alloc(-1)
    print("one-off sweep %s: %d failure points %s" % (name, len(seen), seen))
    assert seen, "no allocation of this call was reached: the sweep checked nothing"
    assert seen == expect
