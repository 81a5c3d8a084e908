"""Object removal (include_ext/lqr_remove.h) on the MI355X against the numpy model of tests/remove_cases.py run on the CPU oracle, bit for
bit: the removal's return value, orientation, seams, marked pixels left, getters, image, dumped map, attached image and progress events for
every case; the scan on carvers in every state against the oracle twin flattened, and the carver unchanged by it; lifted 16I / 64F twins;
a cancel in the second round; refusals; injected allocation failures; the launch counts.

The shapes at the kernels' edges (csrc/lqr_geom.h): the line scan takes DISCARD_CHUNK = 1024 columns of a row at a time on DISCARD_THREADS =
256 lanes, four columns a lane, its chunks starting 0 .. 3 columns in front of the row -- rows of 255 / 256 / 257 and 1023 / 1025 columns
on 5 .. 9 lines (an odd width times the line number gives every lead), and 3-pixel lines; the cross scan takes tiles of DISCARD_ROWS = 32
lines and blocks of 256 columns -- 31 / 32 / 33 / 65 lines, 300 x 40 and 40 x 300."""
import ctypes

import numpy as np
import pytest

import lqr_ctypes as L
import remove_cases as RC

pytestmark = pytest.mark.gpu
CASES = dict(RC.cases())
AUTO = RC.ORIENTATION_AUTO


@pytest.fixture(scope="module")
def eng():
    return L.engine_remove_api()


@pytest.fixture
def lib(eng):
    lb = eng.lib
    lb.lqrhip_debug_fail_alloc.argtypes = [ctypes.c_int]
    lb.lqrhip_debug_pool_live.restype, lb.lqrhip_debug_pool_live.argtypes = ctypes.c_ulonglong, []
    lb.lqrhip_launch_census.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int, ctypes.c_int]
    lb.lqrhip_launch_census.restype = ctypes.c_int
    yield lb
    lb.lqrhip_debug_fail_alloc(-1)


def launches(eng, reset=True):
    out = (ctypes.c_ulonglong * 4)()
    eng.lqrhip_discard_launches(out, 1 if reset else 0)
    return list(out)


def census(lib):
    out = (ctypes.c_ulonglong * 32)()
    lib.lqrhip_launch_census(out, 32, 1)
    return list(out)


def same_state(a, b, what=""):
    """two results of RC.observe: getters, image, attached images, the dumped map"""
    assert a["getters"] == b["getters"], (what, a["getters"], b["getters"])
    assert a["image"].shape == b["image"].shape and np.array_equal(a["image"], b["image"]), what + ": images differ"
    assert len(a["aux"]) == len(b["aux"]) and all(np.array_equal(x, y) for x, y in zip(a["aux"], b["aux"])), what + ": attached images differ"
    va, vb = a["vmap"], b["vmap"]
    assert (va["depth"], va["orientation"]) == (vb["depth"], vb["orientation"]) and np.array_equal(va["data"], vb["data"]), what + ": maps differ"


def same_result(got, want, what=""):
    for k in ("ret", "orientation_used", "seams", "left"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    same_state(got, want, what)
    assert got["events"] == want["events"], what + ": progress events differ"


def call(c, spec):
    return c.remove_discarded(spec["o"], spec["strength"], spec["max_seams"], spec["restore"])


# ---- 1. the removal equals the model exactly ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_removal_equals_the_model(eng, name):
    spec = CASES[name]
    c = RC.build(eng, spec)
    launches(eng)
    got = RC.observe(c, call(c, spec))
    n_line, n_cross, n_rank, n_fold = launches(eng)
    same_result(got, RC.model(name), name)
    if spec["factor"]:
        # a scan in front of the rounds -- both kinds with AUTO, the cross scan where the carver lies the other way -- and a line scan
        # after every round (the carver lies in the removal's orientation then)
        lying = 1 if spec["pre"] == "transposed" else 0
        first_cross = spec["o"] == AUTO or spec["o"] != lying
        first_line = spec["o"] == AUTO or spec["o"] == lying
        # (the carver is flat then: never the ranked scan)
        assert (n_line, n_cross, n_rank, n_fold) == (len(RC.model(name)["rounds"]) + first_line, int(first_cross), 0, int(first_cross)), name
    else:
        assert (n_line, n_cross, n_rank, n_fold) == (0, 0, 0, 0)           # no bias plane: nothing to launch
    if spec["restore"] and got["left"] == 0:
        assert c.flatten() == L.LQR_OK and not RC.marked_of(c.get_bias(), spec["strength"]).any()
    c.destroy()


@pytest.mark.parametrize("depth", [L.LQR_COLDEPTH_16I, L.LQR_COLDEPTH_64F])
@pytest.mark.parametrize("name", ["blobs_w", "diag_h_sw2", "rgba_w", "attached_h", "grey_h", "fullrow_w"])
def test_lifted_twins_give_the_same_seams_and_the_lifted_pixels(eng, name, depth):
    # (cases that create no pixel by averaging: no restore)
    spec, want = CASES[name], RC.model(name)
    assert not spec["restore"]
    c = RC.build(eng, spec, depth=depth)
    got = RC.observe(c, call(c, spec))
    for k in ("ret", "orientation_used", "seams", "left", "getters", "events"):
        assert got[k] == want[k], (name, k)
    assert np.array_equal(got["vmap"]["data"], want["vmap"]["data"])
    lifted = RC.lift(want["image"], depth)
    assert got["image"].dtype == lifted.dtype and np.array_equal(got["image"].reshape(lifted.shape), lifted)
    for a, b in zip(got["aux"], want["aux"]):
        assert np.array_equal(a.reshape(b.shape), RC.lift(b, depth))
    c.destroy()


# ---- 2. the scan, on carvers in every state ----------------------------------------------------------------------------------------
def to_state(c, spec, state):
    w, h = spec["w"], spec["h"]
    steps = dict(flat=[], shrunk=[(w - 10, h)], regrown=[(w - 10, h), (w - 4, h)], enlarged=[(w + 6, h)], transposed=[(w, h - 3)],
                 transposed_regrown=[(w, h - 4), (w, h - 2)])[state]
    for size in steps:
        assert c.resize(*size) == L.LQR_OK
    return c


@pytest.mark.parametrize("state", ["flat", "shrunk", "regrown", "enlarged", "transposed", "transposed_regrown"])
@pytest.mark.parametrize("name", ["blobs_w", "cross_300x40", "line_1025x9", "strength_below", "attached_w"])
def test_scan_equals_the_flattened_oracle_twin_and_leaves_the_carver_unchanged(eng, lib, name, state):
    spec = CASES[name]
    c = to_state(RC.build(eng, spec), spec, state)
    twin = to_state(RC.build(L.oracle_api(), spec, L.OracleCarver), spec, state)
    flat_twin = to_state(RC.build(L.oracle_api(), spec, L.OracleCarver), spec, state)
    g = c.getters()
    size = g["height"] if g["orientation"] else g["width"]
    before = RC.observe(c, {})
    before_sizes = c.read_sizes([size])[0]
    live = lib.lqrhip_debug_pool_live()
    census(lib)
    want = {o: RC.scan(flat_twin, o, spec["strength"]) for o in (0, 1, AUTO)}          # (flattens the twin)
    for o in (0, 1, AUTO):
        launches(eng)
        ret, marked, need = c.discard_scan(o, spec["strength"])
        assert (ret, marked, need) == (L.LQR_OK,) + want[o][:2], (name, state, o)
        # the lines across the layout's rows: by column while nothing is hidden, by rank otherwise
        lying, hidden = g["orientation"], state not in ("flat", "enlarged")
        across = [0, 0, 1, 1] if hidden else [0, 1, 0, 1]
        assert launches(eng) == ([1] + across[1:] if o == AUTO else [1, 0, 0, 0] if o == lying else across), (name, state, o)
    assert want[0][0] == want[1][0]
    # unchanged: no launch of the census' kernels, no block kept, getters, what it shows, its map, the same bytes from read_sizes at its size
    assert lib.lqrhip_debug_pool_live() == live and census(lib) == [0] * 32
    after = RC.observe(c, {})
    same_state(after, before, "after the scan")
    assert np.array_equal(c.read_sizes([size])[0], before_sizes) and np.array_equal(before_sizes.reshape(before["image"].shape), before["image"])
    # ... and a following resize gives what it gives the twin that was never scanned
    to = (spec["w"] - 13, spec["h"] - 3)
    assert c.resize(*to) == twin.resize(*to) == L.LQR_OK
    same_state(RC.observe(c, {}), RC.observe(twin, {}), "the resize after the scan")
    for x in (c, twin, flat_twin):
        x.destroy()


def test_scan_of_a_carver_without_a_bias_plane_and_with_queued_xy_marks(eng):
    spec = CASES["nobias_auto"]
    c = RC.build(eng, spec)
    launches(eng)
    assert [c.discard_scan(o) for o in (0, 1, AUTO)] == [(L.LQR_OK, 0, 0)] * 3 and launches(eng) == [0, 0, 0, 0]
    # marks through _xy are queued on the host: the scan flushes the queue first
    assert c.bias_add_xy([(5, 7, -30.0), (6, 7, -30.0), (6, 8, -3.0), (40, 2, 10.0)]) == [L.LQR_OK] * 4
    assert c.discard_scan(0) == (L.LQR_OK, 3, 2) and c.discard_scan(1) == (L.LQR_OK, 3, 2) and c.discard_scan(0, 1.5) == (L.LQR_OK, 2, 2)
    assert c.discard_scan(0, 15.0) == (L.LQR_OK, 0, 0)           # -15 is not below -15
    assert c.discard_scan(1, 14.5) == (L.LQR_OK, 2, 1)
    c.destroy()


def test_scan_leaves_the_scan_cursor_where_it_was(eng):
    spec = CASES["blobs_w"]
    c = to_state(RC.build(eng, spec), spec, "shrunk")
    img, order = c.scan_ext()
    n = c.scan_partial()                        # the cursor stands inside the first line
    assert 0 < n < len(order) and c.discard_scan(AUTO, spec["strength"])[0] == L.LQR_OK
    rest, order_rest = c.scan_ext(reset=False)
    assert order_rest == order[n:] and np.array_equal(rest.reshape(-1, spec["ch"])[n:], img.reshape(-1, spec["ch"])[n:])
    c.destroy()


# ---- 3. cancel ---------------------------------------------------------------------------------------------------------------------
def test_a_cancel_in_the_second_round_leaves_the_state_of_the_first(eng):
    name = "lshape_w"
    spec, want = CASES[name], RC.model(name)
    assert len(want["rounds"]) == 2
    twin = RC.build(L.oracle_api(), spec, L.OracleCarver)
    assert twin.resize(spec["w"] - want["rounds"][0], spec["h"]) == L.LQR_OK          # the first round alone
    updates = sum(1 for e in twin.events if e[0] == "update")
    c = RC.build(eng, spec)
    c.cancel_at_update(updates + 1)                                                    # the first report of the second round
    got = call(c, spec)
    assert got["ret"] == L.LQR_USRCANCEL and c.cancel_result() == (True, L.LQR_OK) and c.cancelled() == 1
    same_state(RC.observe(c, {}), RC.observe(twin, {}), "after the cancel")
    assert call(c, spec)["ret"] == L.LQR_USRCANCEL                                     # it stays cancelled, untouched
    same_state(RC.observe(c, {}), RC.observe(twin, {}), "still cancelled")
    # cleared, the call runs from where the carver stands: what the model gives on the twin in that state
    assert c.cancel_clear() == L.LQR_OK
    c.cancel_at_update(0)
    del c.events[:], twin.events[:]
    got = RC.observe(c, call(c, spec))
    same_result(got, RC.observe(twin, RC.remove(twin, spec["o"], spec["strength"], spec["max_seams"], spec["restore"])), "after the clear")
    c.destroy()
    twin.destroy()


def test_a_carver_cancelled_beforehand_is_not_touched(eng):
    spec = CASES["pre_shrunk_w"]
    c = RC.build(eng, spec)
    c.cancel_at_update(1)
    assert c.resize(spec["w"] - 8, spec["h"]) == L.LQR_USRCANCEL and c.cancelled() == 1
    c.cancel_at_update(0)
    before = RC.observe(c, {})
    launches(eng)
    got = call(c, spec)
    assert got == dict(ret=L.LQR_USRCANCEL, orientation_used=None, seams=None, left=None) and launches(eng) == [0, 0, 0, 0]
    same_state(RC.observe(c, {}), before, "cancelled beforehand")           # not even flattened
    c.destroy()


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_device_work_with_one_line_each(eng, lib, capfd):
    spec = CASES["attached_w"]
    c = RC.build(eng, spec)
    before = RC.observe(c, {})
    raw = L.Carver.from_ext(eng, RC.make_image(spec), 0, init=False)
    thin_w = L.Carver.from_ext(eng, RC.make_image(dict(spec, w=2, h=40)), 0)
    thin_h = L.Carver.from_ext(eng, RC.make_image(dict(spec, w=40, h=2)), 0)
    for x in (raw, thin_w, thin_h):
        assert x.bias_add_f(np.ones((x.h0, x.w0)), -100) == L.LQR_OK
        x.configure(progress=True)
    capfd.readouterr()
    launches(eng)
    census(lib)
    live = lib.lqrhip_debug_pool_live()
    nothing = dict(ret=L.LQR_ERROR, orientation_used=None, seams=None, left=None)
    refused = [c.aux[0].remove_discarded(0), raw.remove_discarded(0), c.remove_discarded(2), c.remove_discarded(-2), c.remove_discarded(0, -1.0),
               c.remove_discarded(0, float("nan")), c.remove_discarded(1, float("inf")), c.remove_discarded(0, 0.0, 0), c.remove_discarded(1, 0.0, -4),
               thin_w.remove_discarded(0), thin_h.remove_discarded(1), thin_w.remove_discarded(AUTO), thin_h.remove_discarded(AUTO)]
    assert refused == [nothing] * len(refused)
    err = capfd.readouterr().err.strip().splitlines()
    assert len(err) == len(refused) and all("lqrx_carver_remove_discarded refused" in line for line in err), err
    # the scan's refusals: an attached carver, the orientation, the strength
    assert [c.aux[0].discard_scan(0)[0], c.discard_scan(2)[0], c.discard_scan(-2)[0], c.discard_scan(0, -0.5)[0], c.discard_scan(0, float("nan"))[0],
            c.discard_scan(1, float("inf"))[0]] == [L.LQR_ERROR] * 6
    assert launches(eng) == [0, 0, 0, 0] and census(lib) == [0] * 32 and lib.lqrhip_debug_pool_live() == live
    same_state(RC.observe(c, {}), before, "after the refusals")
    # the lines that are just long enough are served: 3 pixels, one marked column
    assert thin_w.remove_discarded(1)["ret"] == L.LQR_OK and thin_h.remove_discarded(0)["ret"] == L.LQR_OK
    for x in (c, raw, thin_w, thin_h):
        x.destroy()


# ---- 5. allocation failures --------------------------------------------------------------------------------------------------------
def test_an_allocation_failure_in_the_scan_leaves_nothing_live(eng, lib):
    spec = CASES["cross_300x40"]
    c = RC.build(eng, spec)
    want = c.discard_scan(AUTO)
    live = lib.lqrhip_debug_pool_live()
    lib.lqrhip_pool_trim.restype = None
    lib.lqrhip_pool_trim()                      # (the injected failure hits fresh blocks only)
    failures = 0
    for n in range(8):
        lib.lqrhip_debug_fail_alloc(n)
        got = c.discard_scan(AUTO)
        lib.lqrhip_debug_fail_alloc(-1)
        assert lib.lqrhip_debug_pool_live() == live, n
        if got[0] == L.LQR_OK:
            break
        failures += 1
        assert got[0] == L.LQR_NOMEM, (n, got)
    assert got == want and failures >= 1, (got, failures)
    c.destroy()


def test_an_allocation_failure_in_the_removal_leaves_a_state_of_the_sequence_and_the_call_again_finishes(eng, lib):
    name = "lshape_w"
    spec, want = CASES[name], RC.model(name)
    w, h = spec["w"], spec["h"]
    assert want["regrown"] and len(want["rounds"]) == 2
    steps = [(w - k, h) for k in want["rounds"]] + [(w - want["seams"], h)]           # the sizes the sequence passes through

    def twin_at(i):
        t = RC.build(L.oracle_api(), spec, L.OracleCarver)
        for size in steps[:i]:
            assert t.resize(*size) == L.LQR_OK
        del t.events[:]
        return t
    states = []
    for i in range(len(steps) + 1):
        t = twin_at(i)
        states.append(RC.observe(t, {}))
        t.destroy()
    live0 = lib.lqrhip_debug_pool_live()
    failures, seen = 0, set()
    lib.lqrhip_pool_trim.restype = None
    for n in range(200):
        c = RC.build(eng, spec)
        del c.events[:]
        lib.lqrhip_pool_trim()                  # the injected failure hits fresh blocks only
        lib.lqrhip_debug_fail_alloc(n)
        got = call(c, spec)
        lib.lqrhip_debug_fail_alloc(-1)
        if got["ret"] == L.LQR_OK:
            same_result(RC.observe(c, got), want, "no failure left to inject")
            c.destroy()
            break
        failures += 1
        assert got["ret"] == L.LQR_NOMEM, (n, got)
        now = RC.observe(c, {})
        at = [i for i, s in enumerate(states) if s["getters"] == now["getters"]]
        assert len(at) == 1, (n, now["getters"])
        same_state(now, states[at[0]], "allocation %d failed" % n)
        seen.add(at[0])
        # the call made again runs from there: what the model gives on the twin in that state
        t = twin_at(at[0])
        del c.events[:]
        same_result(RC.observe(c, call(c, spec)), RC.observe(t, RC.remove(t, spec["o"], spec["strength"], spec["max_seams"], spec["restore"])), "again after %d" % n)
        t.destroy()
        c.destroy()
        assert lib.lqrhip_debug_pool_live() == live0, n
    else:
        pytest.fail("the call never got through")
    # (the scan's result block, then the first session's planes; which later allocations are fresh ones is the pool's business)
    assert failures >= 3 and 0 in seen, (failures, seen)
    assert lib.lqrhip_debug_pool_live() == live0


# ---- 6. the seam loop is as it was ---------------------------------------------------------------------------------------------------
def test_a_plain_resize_launches_what_it_launched_and_no_scan(eng, lib):
    spec = CASES["rect_w"]
    c = RC.build(eng, spec)
    census(lib)
    launches(eng)
    assert c.resize(spec["w"] - 16, spec["h"]) == L.LQR_OK
    plain = census(lib)
    assert launches(eng) == [0, 0, 0, 0] and sum(plain) > 0
    c.destroy()
    # the removal's one round of 16 seams is that resize: the same launches in every slot of the census, plus its scans
    c = RC.build(eng, spec)
    assert RC.model("rect_w")["rounds"] == [16]
    got = call(c, spec)
    assert got["ret"] == L.LQR_OK and census(lib) == plain and launches(eng) == [2, 0, 0, 0]
    c.destroy()
