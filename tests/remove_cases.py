"""Object removal (include_ext/lqr_remove.h): THE SPECIFICATION, as a numpy model over the carver API, and the cases the engine is held to it on.

A pixel is MARKED when its bias -- the plane lqrx_carver_get_bias returns -- is below -strength (a float32 comparison).  A line is a row
of the image for orientation 0 (vertical seams, the width shrinks) and a column for orientation 1.

scan(c, orientation, strength) is lqrx_carver_discard_scan: it flattens the carver it is given (the engine's call does not: it returns
what the scan of the flattened carver returns) and counts the marked pixels and the most in one line.  With ORIENTATION_AUTO it reports
the orientation with the smaller `need`, a tie goes to 0.

remove(c, orientation, strength, max_seams, restore) is lqrx_carver_remove_discarded, composed of lqr_carver_flatten, lqr_carver_resize,
lqrx_carver_get_bias and lqr_vmap_dump alone; run on the CPU oracle it gives what the engine must give, bit for bit:

    flatten if the carver is not flat; (W0, H0) its size; pick the orientation (AUTO: scan both); L the line length
    scan: need == 0 -> seams 0, left 0
    cap = min(max_seams, L - 2); cur = 0
    while need > 0 and cur < cap:
        cur += min(max(need, MIN_STEP), cap - cur)
        lqr_carver_resize to L - cur in that orientation
        need    = the most marked pixels in one line that have no level in the dumped map
        deepest = the largest level of a marked pixel in the dumped map
    need == 0: fin = deepest; if fin < cur: lqr_carver_resize up to L - fin (served from the map); seams fin, left 0
    else (the cap was reached): seams cur, left = the marked pixels without a level
    restore: lqr_carver_flatten, lqr_carver_resize to (W0, H0)

The bias of the pixels of the starting image does not change while the carver is resized (only the pixels an enlargement inserts get
new values), so the model reads the plane once, on the flat carver, and looks at the dumped map after every round.
"""
import functools
import json

import numpy as np

import lqr_ctypes as L

F = np.float32
MIN_STEP = 16               # LQRX_REMOVE_MIN_STEP
ORIENTATION_AUTO = -1       # LQRX_ORIENTATION_AUTO


# ---- the model ----------------------------------------------------------------------------------------------------------------
def marked_of(bias, strength):
    return np.asarray(bias, F) < F(-F(strength))


def counts(marked, orientation):
    """(marked pixels, the most in one line) of an h x w boolean image"""
    if not marked.size:
        return 0, 0
    return int(marked.sum()), int(marked.sum(axis=0 if orientation else 1).max())


def pick(marked, orientation):
    """(marked, need, the orientation reported): AUTO takes the smaller need, a tie goes to 0"""
    if orientation != ORIENTATION_AUTO:
        return counts(marked, orientation) + (orientation,)
    n0, n1 = counts(marked, 0), counts(marked, 1)
    return n1 + (1,) if n1[1] < n0[1] else n0 + (0,)


def is_flat(c):
    g = c.getters()
    return g["depth"] == 0 and g["width"] == g["ref_width"] and g["height"] == g["ref_height"]


def scan(c, orientation, strength):
    """lqrx_carver_discard_scan's result for carver c, which is flattened: (marked, need, orientation reported)"""
    assert c.flatten() == L.LQR_OK
    return pick(marked_of(c.get_bias(), strength), orientation)


def remove(c, orientation, strength, max_seams, restore, min_step=MIN_STEP):
    """lqrx_carver_remove_discarded on carver c: dict(ret, orientation_used, seams, left) and, for the tests of the case list,
    rounds (the seams asked for after each round) and regrown (fin < cur)"""
    out = dict(ret=L.LQR_OK, orientation_used=None, seams=None, left=None, rounds=[], regrown=False)
    if not is_flat(c):
        assert c.flatten() == L.LQR_OK
    g = c.getters()
    W0, H0 = g["width"], g["height"]
    marked = marked_of(c.get_bias(), strength)
    _, need, o = pick(marked, orientation)
    out["orientation_used"] = o
    Ln = H0 if o else W0
    if need == 0:
        return dict(out, seams=0, left=0)
    cap, cur, deepest = min(max_seams, Ln - 2), 0, 0
    while need > 0 and cur < cap:
        cur += min(max(need, min_step), cap - cur)
        ret = c.resize(*((W0, Ln - cur) if o else (Ln - cur, H0)))
        if ret != L.LQR_OK:
            return dict(out, ret=ret)
        out["rounds"].append(cur)
        levels = c.vmap_dump()["data"]
        assert levels.shape == marked.shape
        _, need = counts(marked & (levels == 0), o)
        deepest = int(levels[marked].max())
    if need == 0:
        if deepest < cur:
            out["regrown"] = True
            ret = c.resize(*((W0, Ln - deepest) if o else (Ln - deepest, H0)))
            if ret != L.LQR_OK:
                return dict(out, ret=ret)
        out.update(seams=deepest, left=0)
    else:
        out.update(seams=cur, left=int((marked & (levels == 0)).sum()))
    if restore:
        ret = c.flatten()
        if ret == L.LQR_OK:
            ret = c.resize(W0, H0)
        out["ret"] = ret
    return out


# ---- masks: h x w arrays of 0 / 1 ------------------------------------------------------------------------------------------------
def _rect(w, h, rng):
    m = np.zeros((h, w))
    m[h // 4:h // 4 + max(h // 3, 1), w // 3:w // 3 + max(w // 7, 1)] = 1
    return m


def _diag(w, h, rng):
    """a band along the diagonal: few marked pixels in any line of either orientation, many lines"""
    m = np.zeros((h, w))
    for y in range(h):
        x = y * (w - 4) // max(h - 1, 1)
        m[y, x:x + 4] = 1
    return m


def _lshape(w, h, rng):
    m = np.zeros((h, w))
    m[h // 6:h - h // 6, w // 5:w // 5 + max(w // 12, 1)] = 1
    m[h - h // 6 - max(h // 8, 1):h - h // 6, w // 5:w // 5 + w // 2 - 2] = 1
    return m


def _blobs(w, h, rng):
    """two blobs side by side in different lines: a seam passes through one of them at a time"""
    m = np.zeros((h, w))
    m[h // 8:h // 8 + h // 3, w // 8:w // 8 + max(w // 7, 1)] = 1
    m[h // 2:h // 2 + h // 3, w // 2:w // 2 + max(w // 7, 1)] = 1
    return m


def _none(w, h, rng):
    return np.zeros((h, w))


def _one(w, h, rng):
    m = np.zeros((h, w))
    m[h // 2, w // 2] = 1
    return m


def _edges(w, h, rng):
    """marks in the first and the last column and line"""
    m = np.zeros((h, w))
    m[0, 0] = m[0, w - 1] = m[h - 1, 0] = m[h - 1, w - 1] = 1
    m[h // 2, 0] = m[h // 2, w - 1] = m[0, w // 2] = m[h - 1, w // 2] = 1
    return m


def _fullrow(w, h, rng):
    """a row marked end to end: it cannot be emptied by vertical seams"""
    m = np.zeros((h, w))
    m[h // 2, :] = 1
    return m


def _fullcol(w, h, rng):
    m = np.zeros((h, w))
    m[:, w // 2] = 1
    return m


def _square(w, h, rng):
    """as many marked pixels in a row as in a column: AUTO's tie"""
    m = np.zeros((h, w))
    s = max(min(w, h) // 4, 1)
    m[h // 2 - s // 2:h // 2 - s // 2 + s, w // 2 - s // 2:w // 2 - s // 2 + s] = 1
    return m


def _scatter(w, h, rng):
    return (rng.random((h, w)) < 0.04).astype(np.float64)


def _ticks(w, h, rng):
    """a few marks in every row: the first and the last column, the columns on either side of a multiple of 256, one that moves"""
    m = np.zeros((h, w))
    for y in range(h):
        for x in (0, w - 1, 255, 256, 1023, 1024, (y * 37 + 5) % w):
            if 0 <= x < w:
                m[y, x] = 1
    return m


def _ticks_v(w, h, rng):
    return np.ascontiguousarray(_ticks(h, w, rng).T)


MASKS = dict(rect=_rect, diag=_diag, lshape=_lshape, blobs=_blobs, none=_none, one=_one, edges=_edges, fullrow=_fullrow, fullcol=_fullcol,
             square=_square, scatter=_scatter, ticks=_ticks, ticks_v=_ticks_v)


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def make_image(spec):
    rng = np.random.default_rng(spec["seed"])
    return rng.integers(0, 256, (spec["h"], spec["w"], spec["ch"]), dtype=np.uint8)


def make_mask(spec, kind=None):
    return MASKS[kind or spec["mask"]](spec["w"], spec["h"], np.random.default_rng([spec["seed"], 9]))


def lift(img, depth):
    """the 16I / 64F twin of an 8-bit image (tests/sequence_cases.py: v * 257, v / 255.0)"""
    if depth == L.LQR_COLDEPTH_16I:
        return img.astype(np.uint16) * 257
    if depth == L.LQR_COLDEPTH_64F:
        return img.astype(np.float64) / 255.0
    assert depth == L.LQR_COLDEPTH_8I
    return img


def add_bias(c, m, factor, via):
    """mask m (0 / 1) with `factor` through one of the mask calls; every form leaves factor * m / 2 in the plane"""
    if via == "rgb":
        return c.bias_add(np.repeat((m * 255).astype(np.uint8)[:, :, None], 3, axis=2), factor)
    if via == "f":
        return c.bias_add_f(m, factor)
    if via == "xy":
        rets = c.bias_add_xy([(x, y, float(factor)) for y, x in np.argwhere(m > 0)])
        return L.LQR_OK if all(r == L.LQR_OK for r in rets) else L.LQR_ERROR
    if via == "device":                 # (the oracle has no device: its twin takes the same plane from the host)
        if isinstance(c, L.OracleCarver):
            return c.bias_add_f(m, factor)
        import torch
        return c.bias_add_device(torch.from_numpy(np.ascontiguousarray(m, np.float64)).cuda(), factor)
    raise ValueError(via)


def build(api, spec, cls=None, depth=0):
    """the carver of a spec with its masks on: the plug-in's sequence (init, bias, configure), then the state the spec asks for"""
    cls = cls or L.Carver
    img = make_image(spec)
    c = cls.from_ext(api, lift(img, depth), depth, delta_x=spec["delta"], rigidity=spec["rigidity"])
    if spec["attach"]:
        c.attach_ext(lift(make_image(dict(spec, seed=spec["seed"] + 1, ch=1)), depth), depth)
    if spec["pre"] == "transposed":             # a flat carver that lies transposed, before the masks
        assert c.resize(spec["w"], spec["h"] - 2) == L.LQR_OK and c.resize(spec["w"], spec["h"]) == L.LQR_OK
        assert c.flatten() == L.LQR_OK and c.getters()["orientation"] == 1
    if spec["preserve"]:
        assert add_bias(c, make_mask(spec, spec["preserve"][0]), spec["preserve"][1], "rgb") == L.LQR_OK
    if spec["factor"]:
        assert add_bias(c, make_mask(spec), spec["factor"], spec["via"]) == L.LQR_OK
    if spec["weak"]:                            # marks that stay above -strength
        assert add_bias(c, make_mask(spec, spec["weak"][0]), spec["weak"][1], "f") == L.LQR_OK
    c.configure(nrg_func=L.LQR_EF_GRAD_XABS, res_order=L.LQR_RES_ORDER_HOR, switch_freq=spec["switch"], enl_step=2.0, progress=True)
    if spec["pre"] == "shrunk":                 # not flat when the call comes: it is flattened first
        assert c.resize(spec["w"] - 3, spec["h"]) == L.LQR_OK
    return c


def observe(c, res):
    """everything observable at the C ABI after a call"""
    res = dict(res)
    res["getters"] = c.getters()
    res["image"] = c.scan_line_ext()[0]
    res["aux"] = [a.scan_line_ext()[0] for a in c.aux]
    res["vmap"] = c.vmap_dump()
    res["events"] = list(c.events)
    return res


def run_model(spec, min_step=MIN_STEP):
    c = build(L.oracle_api(), spec, L.OracleCarver)
    res = observe(c, remove(c, spec["o"], spec["strength"], spec["max_seams"], spec["restore"], min_step))
    if spec["restore"]:                         # (the plane is read from a flat carver)
        assert c.flatten() == L.LQR_OK
        res["bias_after"] = c.get_bias()
    c.destroy()
    return res


@functools.lru_cache(maxsize=None)
def model(name, min_step=MIN_STEP):
    """the model's result for a case of cases(), computed once and shared by the tests; nobody changes it"""
    return run_model(dict(cases())[name], min_step)


def guess_seams(spec):
    """the seams the plug-in's auto-size button asks for: the longest count of mask pixels in a line (lqrx_guess_new_size)"""
    m = np.ascontiguousarray(np.repeat((make_mask(spec) * 255).astype(np.uint8)[:, :, None], 3, axis=2))
    api = L.oracle_api()
    old = spec["h"] if spec["o"] else spec["w"]
    return old - api.lqrx_guess_new_size(m.ctypes.data, 3, spec["w"], spec["h"], 0, 0, spec["w"], spec["h"], spec["o"])


# ---- the cases ------------------------------------------------------------------------------------------------------------------
def cases():
    """(name, spec).  seed, w, h, ch: the image; mask, factor, via: the discard mask, its factor and the call it comes through; o: the
    orientation asked for; switch, delta, rigidity: the carver's side-switch frequency, delta_x and rigidity; strength, max_seams,
    restore: the call's arguments; preserve: (mask, factor) added first; weak: (mask, factor) added last, to stay above -strength;
    attach: a grey attached carver; pre: None, "transposed" or "shrunk" (the carver's
    state when the call comes)"""
    out = []

    def add(name, mask, factor, o, **more):
        spec = dict(seed=52000 + len(out), w=48, h=24, ch=3, mask=mask, factor=factor, via="rgb", o=o, switch=0, delta=1, rigidity=0.0,
                    strength=0.0, max_seams=1 << 20, restore=False, preserve=None, weak=None, attach=False, pre=None)
        spec.update(more)
        out.append((name, json.loads(json.dumps(spec))))

    # the issue's table: the guess is a lower bound
    add("blobs_w", "blobs", -1000, 0)
    add("lshape_w", "lshape", -20, 0)
    add("diag_h", "diag", -20, 1)
    add("rect_w", "rect", -1000, 0)
    add("rect_h", "rect", -1000, 1, restore=True)
    add("diag_w", "diag", -1000, 0, via="f")
    add("lshape_h", "lshape", -1000, 1, via="f", restore=True)
    # the cap: a line marked end to end, a small max_seams
    add("fullrow_w", "fullrow", -1000, 0)
    add("fullcol_h", "fullcol", -1000, 1, restore=True)
    add("lshape_w_max5", "lshape", -20, 0, max_seams=5)
    add("blobs_w_max17", "blobs", -1000, 0, max_seams=17, restore=True)
    # side switches: the rounds are part of the result
    add("lshape_w_sw2", "lshape", -20, 0, switch=2)
    add("diag_h_sw2", "diag", -20, 1, switch=2)
    add("blobs_w_sw2", "blobs", -20, 0, switch=2, restore=True)
    add("diag_w_sw2", "diag", -20, 0, switch=2)
    # delta_x 2 with rigidity
    add("lshape_w_d2", "lshape", -1000, 0, delta=2, rigidity=0.5)
    add("diag_h_d2", "diag", -20, 1, delta=2, rigidity=0.5, switch=2)
    # nothing marked, one pixel, the first and last column and line
    add("none_w", "none", -1000, 0)
    add("nobias_auto", "none", 0, ORIENTATION_AUTO)
    add("one_w", "one", -1000, 0)
    add("one_h", "one", -1000, 1, via="xy")
    add("edges_w", "edges", -1000, 0, via="xy")
    add("edges_h", "edges", -1000, 1, via="device", restore=True)
    # strength: marks only below -strength (the weak ones stay), and only above it (nothing to do)
    add("strength_below", "rect", -1000, 0, strength=100.0, weak=("blobs", -20))
    add("strength_above", "rect", -20, 0, strength=100.0)
    add("strength_exact", "rect", -200, 0, strength=100.0)          # bias -100 is not below -100
    # a preserve mask across the object's seams
    add("preserve_w", "rect", -1000, 0, preserve=("fullrow", 1000))
    add("preserve_h", "blobs", -1000, 1, preserve=("fullcol", 1000), restore=True)
    # AUTO: the smaller need, and a tie
    add("auto_rect", "rect", -1000, ORIENTATION_AUTO)
    add("auto_lshape", "lshape", -1000, ORIENTATION_AUTO, restore=True)
    add("auto_tie", "square", -1000, ORIENTATION_AUTO)
    add("auto_fullrow", "fullrow", -1000, ORIENTATION_AUTO)
    # RGBA, grey, an attached carver, the carver's state beforehand
    add("rgba_w", "blobs", -1000, 0, ch=4, via="device")
    add("grey_h", "lshape", -1000, 1, ch=1)
    add("attached_w", "lshape", -20, 0, attach=True, restore=True)
    add("attached_h", "rect", -1000, 1, attach=True)
    add("pre_transposed_w", "rect", -1000, 0, pre="transposed")
    add("pre_transposed_h", "blobs", -1000, 1, pre="transposed", restore=True)
    add("pre_transposed_auto", "lshape", -1000, ORIENTATION_AUTO, pre="transposed")
    add("pre_shrunk_w", "scatter", -1000, 0, pre="shrunk")
    # shapes at the kernels' edges (tests/test_remove_gpu.py names them): the line scan's chunk of 1024 columns and its 256 threads on
    # few lines; the shortest lines there are; the cross scan's tiles of 32 lines and its blocks of 256 columns
    for w, h in ((255, 5), (256, 6), (257, 7), (1023, 8), (1025, 9)):
        add("line_%dx%d" % (w, h), "ticks", -1000, 0, w=w, h=h)
    add("line_1025x5_v", "ticks_v", -1000, 1, w=5, h=1025, pre="transposed")
    add("short_3x40", "one", -1000, 0, w=3, h=40)
    add("short_40x3", "one", -1000, 1, w=40, h=3)
    for w, h in ((40, 31), (41, 32), (40, 33), (37, 65)):
        add("cross_%dx%d" % (w, h), "scatter", -1000, 1, w=w, h=h, max_seams=17)
    add("cross_300x40", "scatter", -1000, 1, w=300, h=40, max_seams=16)
    add("cross_40x300_auto", "edges", -1000, ORIENTATION_AUTO, w=40, h=300)
    # (added last, so that the cases above keep their seeds) side switches in a single round: the session's depth alone sets the interval
    add("rect_h_sw2", "rect", -1000, 1, switch=2, seed=53001)
    add("scatter_w_sw2", "scatter", -1000, 0, switch=2, seed=53001)
    return out
