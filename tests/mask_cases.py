"""The computed-mask cases (include/lqr_masks.h: gdouble bias / rigidity masks, single (x, y, value) calls, clears): specs, the
driver that runs one through any library whose carver class has binding.Carver's methods -- the genuine liblqr
(scripts/ref_engine/make_mask_golden.py, which records tests/golden/masks/) and the HIP engine (tests/test_masks_gpu.py, which
reproduces the records) -- and a numpy model of what the calls do to the two planes, checked against the genuine planes without a
GPU (tests/test_masks_abi.py).

A spec is a small JSON-able dict:
  seed, w, h, ch, depth (LqrColDepth), nrg, delta, rigidity, res_order      the carver, as in coldepth_cases
  late_init     the carver is created without lqr_carver_init; the op ["init"] calls it
  aux           an attached carver of the same size (ops on it: ["aux", op...])
  masks         name -> [w, h, kind]: "rand" doubles in [-1, 2), "dyadic" multiples of 1/8 in [-1, 2], "binary" 0 / 1,
                "rgb1" .. "rgb4" 8-bit masks of that many channels, "bw" a one-channel 8-bit mask of 0 / 255
  runs          name -> [kind, values, ...]: sequences of (x, y, value) in IMAGE coordinates of the carver as it is when the run
                starts: "rowmajor" / "shuffle" the full frame, "repeat" n pixels hit k times each in a seeded interleaving cut to
                `total` entries, "some" n distinct pixels; values "rand" or "dyadic"
  ops           applied in order, each return value recorded:
                ["resize", w, h] ["flatten"] ["init"] ["planes"] (a snapshot of both planes)
                ["bias_f", mask, factor, x_off, y_off] (offsets None: lqr_carver_bias_add)    ["rig_f", mask, x_off, y_off]
                ["bias_rgb", mask, factor] ["rig_rgb", mask]                                  (lqr_carver_*_add_rgb)
                ["bias_rgb_area", mask, factor, x_off, y_off] ["rig_rgb_area", mask, x_off, y_off]
                ["bias_xy", run] ["rig_xy", run] ["bias_clear"] ["rig_clear"]
  steps         [(w, h), ...] resizes after the ops; image and visibility map are recorded after each
After the ops the bias and rigidity planes (image orientation) and the energy plane (carver frame) are recorded if the carver is
flat -- every mask call that does anything flattens it.
"""
import json

import numpy as np

import coldepth_cases as CD

ROUNDING_NOTE = ("bias area: += (gfloat) ((gdouble) factor * v / 2); bias xy: += (gfloat) v / 2; rigidity area: = (gfloat) v; "
                 "rigidity xy: += (gfloat) v; each operation rounded to its C type")


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def make_mask(rng, w, h, kind):
    if kind == "rand":
        return rng.uniform(-1.0, 2.0, (h, w))
    if kind == "dyadic":
        return rng.integers(-8, 17, (h, w)).astype(np.float64) / 8.0
    if kind == "binary":
        return (rng.random((h, w)) < 0.5).astype(np.float64)
    if kind == "bw":
        return ((rng.random((h, w, 1)) < 0.5) * 255).astype(np.uint8)
    assert kind.startswith("rgb"), kind
    return rng.integers(0, 256, (h, w, int(kind[3:]))).astype(np.uint8)


def make_input(spec):
    """(image, {"aux": image, "masks": {name: array}})"""
    rng = np.random.default_rng(spec["seed"])
    img = CD.to_depth(rng, CD.base_image(rng, spec["w"], spec["h"], spec["ch"]), spec["depth"])
    extra = {"masks": {}}
    if spec.get("aux"):
        extra["aux"] = CD.base_image(rng, spec["w"], spec["h"], 2)
    for name in sorted(spec.get("masks", {})):
        w, h, kind = spec["masks"][name]
        extra["masks"][name] = make_mask(np.random.default_rng([spec["seed"], len(name), w, h]), w, h, kind)
    return img, extra


def make_run(spec, name, W, H):
    """the (x, y, value) entries of run `name` on a W x H image"""
    kind, values = spec["runs"][name][:2]
    more = spec["runs"][name][2:]
    rng = np.random.default_rng([spec["seed"], 77, len(name), W, H])
    if kind == "rowmajor":
        pix = np.arange(W * H)
    elif kind == "shuffle":
        pix = rng.permutation(W * H)
    elif kind == "some":
        pix = rng.choice(W * H, more[0], replace=False)
    else:
        assert kind == "repeat", kind
        n, k, total = more
        pix = rng.permutation(np.repeat(rng.choice(W * H, n, replace=False), k))[:total]
    if values == "dyadic":
        val = rng.integers(-8, 17, len(pix)).astype(np.float64) / 4.0
        val[val == 0] = 0.25
    else:
        val = rng.uniform(-3.0, 5.0, len(pix))
    return [(int(p % W), int(p // W), float(v)) for p, v in zip(pix, val)]


# ---- the model: what the calls do to the planes, every operation rounded to its C type ----------------------------------------
def _clip(W, H, mw, mh, xo, yo):
    x1, y1, x2, y2 = max(0, xo), max(0, yo), min(W, mw + xo), min(H, mh + yo)
    if x2 <= x1 or y2 <= y1:
        return None
    return (slice(y1, y2), slice(x1, x2)), (slice(y1 - yo, y2 - yo), slice(x1 - xo, x2 - xo))


def _rgb_value(m, factor=None):
    """the mask value of an 8-bit mask (lqr.h: mean of the colour channels / 255, times alpha / 255), as the rgb forms compute it"""
    ch = m.shape[2]
    alpha = ch in (2, 4)
    cc = ch - alpha
    s = m[:, :, :cc].astype(np.int64).sum(axis=2).astype(np.float64)
    v = s / np.float64(255 * cc) if factor is None else (np.float64(factor) * s) / np.float64(2 * 255 * cc)
    if alpha:
        v = v * (m[:, :, ch - 1].astype(np.float64) / 255.0)
    return v.astype(np.float32)


class Model:
    """bias / rig: float32 planes in image orientation, or None; valid: the planes are known (a resize of non-zero planes carves them)"""

    def __init__(self, spec, masks):
        self.spec, self.masks = spec, masks
        self.W, self.H = spec["w"], spec["h"]
        self.bias = self.rig = None
        self.valid = True
        self.active = not spec.get("late_init")

    def plane(self, which):
        p = getattr(self, which)
        return np.zeros((self.H, self.W), np.float32) if p is None else p

    def adopt(self, bias, rig):
        self.bias, self.rig, self.valid = bias.copy(), rig.copy(), True

    def _area(self, which, values, xo, yo, add):
        """values: float32, what is added / assigned"""
        mh, mw = values.shape
        if xo is None:
            assert (mw, mh) == (self.W, self.H)
            xo = yo = 0
        p = self.plane(which)
        c = _clip(self.W, self.H, mw, mh, xo, yo)
        if c:
            p[c[0]] = p[c[0]] + values[c[1]] if add else values[c[1]]
        setattr(self, which, p)

    def apply(self, op):
        """returns the LqrRetVal the call gives (1 OK, 0 ERROR), None for ops without one"""
        kind, a = op[0], op[1:]
        two = np.float32(2)
        if kind == "resize":
            if (self.bias is not None and self.bias.any()) or (self.rig is not None and self.rig.any()):
                self.valid = False
            self.W, self.H = a[0], a[1]
            for which in ("bias", "rig"):
                if getattr(self, which) is not None:
                    setattr(self, which, np.zeros((self.H, self.W), np.float32))
            return 1
        if kind in ("flatten", "planes"):
            return 1 if kind == "flatten" else None
        if kind == "init":
            self.active = True
            return 1
        if kind in ("bias_clear", "rig_clear"):
            setattr(self, kind[:-6], None)
            return None
        if kind.startswith("rig") and not self.active:
            return 0
        if kind == "bias_f":
            if a[1] != 0:
                self._area("bias", (np.float64(a[1]) * self.masks[a[0]] / 2.0).astype(np.float32), a[2], a[3], True)
        elif kind == "rig_f":
            self._area("rig", self.masks[a[0]].astype(np.float32), a[1], a[2], False)
        elif kind in ("bias_rgb", "bias_rgb_area"):
            if a[1] != 0:
                self._area("bias", _rgb_value(self.masks[a[0]], a[1]), *(a[2:] if kind.endswith("area") else (None, None)), add=True)
        elif kind in ("rig_rgb", "rig_rgb_area"):
            self._area("rig", _rgb_value(self.masks[a[0]]), *(a[1:] if kind.endswith("area") else (None, None)), add=False)
        elif kind == "bias_xy":
            for x, y, v in make_run(self.spec, a[0], self.W, self.H):
                if v != 0:
                    p = self.plane("bias")
                    p[y, x] = p[y, x] + np.float32(v) / two
                    self.bias = p
        elif kind == "rig_xy":                      # (it adds: liblqr 0.4.1's lqr_carver_rigmask_add_xy does)
            p = self.plane("rig")
            for x, y, v in make_run(self.spec, a[0], self.W, self.H):
                p[y, x] = p[y, x] + np.float32(v)
            self.rig = p
        else:
            raise ValueError(kind)
        return 1


# ---- the driver ---------------------------------------------------------------------------------------------------------------
def _is_flat(g):
    return g["depth"] == 0 and g["width"] == g["ref_width"] and g["height"] == g["ref_height"]


def _summary(rets):
    """the return values of a run of _xy calls: [[value, how often], ...]"""
    return [[int(v), int(rets.count(v))] for v in sorted(set(rets))]


def _do(c, spec, masks, op):
    kind, a = op[0], op[1:]
    if kind == "resize":
        return c.resize(a[0], a[1])
    if kind == "flatten":
        return c.flatten()
    if kind == "init":
        return c.init(spec.get("delta", 1), spec.get("rigidity", 0.0))
    if kind == "bias_f":
        return c.bias_add_f(masks[a[0]], a[1], a[2], a[3])
    if kind == "rig_f":
        return c.rigmask_add_f(masks[a[0]], a[1], a[2])
    if kind == "bias_rgb":
        return c.bias_add_rgb(masks[a[0]], a[1])
    if kind == "rig_rgb":
        return c.rigmask_add_rgb(masks[a[0]])
    if kind == "bias_rgb_area":
        return c.bias_add(masks[a[0]], a[1], a[2], a[3])
    if kind == "rig_rgb_area":
        return c.rigmask_add(masks[a[0]], a[1], a[2])
    if kind in ("bias_xy", "rig_xy"):
        g = c.getters()
        entries = make_run(spec, a[0], g["width"], g["height"])
        return _summary((c.bias_add_xy if kind == "bias_xy" else c.rigmask_add_xy)(entries))
    if kind == "bias_clear":
        return c.bias_clear()
    if kind == "rig_clear":
        return c.rigmask_clear()
    raise ValueError(kind)


def run(api, cls, spec, img=None, extra=None):
    """drive one case; returns a dict of arrays and a JSON record"""
    if img is None:
        img, extra = make_input(spec)
    masks = extra["masks"]
    c = cls.from_ext(api, img, spec["depth"], init=not spec.get("late_init"), delta_x=spec.get("delta", 1), rigidity=spec.get("rigidity", 0.0))
    aux = c.attach_ext(extra["aux"], 0) if "aux" in extra else None
    c.configure(nrg_func=spec["nrg"], res_order=spec.get("res_order", 0), switch_freq=2, enl_step=1.5)
    out, rec = {}, {"rets": [], "step_rets": [], "getters": [], "vmap_meta": []}
    for i, op in enumerate(spec["ops"]):
        if op[0] == "planes":
            out["bias@%d" % i], out["rig@%d" % i] = c.get_bias(), c.get_rigmask()
            rec["rets"].append(None)
        elif op[0] == "aux":
            rec["rets"].append(_do(aux, spec, masks, op[1:]))
        else:
            rec["rets"].append(_do(c, spec, masks, op))
    g = c.getters()
    rec["after_ops"] = g
    if _is_flat(g):
        out["bias"], out["rig"] = c.get_bias(), c.get_rigmask()
        out["energy"] = c.energy()
    for i, (w1, h1) in enumerate(spec["steps"]):
        ret = c.resize(w1, h1)
        rec["step_rets"].append(ret)
        if ret != 1:
            break
        out["image%d" % i] = c.scan_line_ext()[0]
        v = c.vmap_dump()
        out["vmap%d" % i] = v["data"]
        rec["vmap_meta"].append([v["depth"], v["orientation"]])
        rec["getters"].append(c.getters())
    c.destroy()
    out["record"] = np.array(json.dumps(rec, sort_keys=True))
    return out


assert_same_record = CD.assert_same_record


# ---- the cases ----------------------------------------------------------------------------------------------------------------
def cases():
    """the smallest shapes at which the mask code can go wrong (images around 300 x 40 and 40 x 300)"""
    out = []

    def add(name, ops, w=300, h=40, steps=None, masks=None, runs=None, **more):
        spec = dict(seed=5000 + len(out), w=w, h=h, ch=1, depth=0, nrg=2, delta=1, rigidity=0.0, ops=ops,
                    steps=[(w - 9, h)] if steps is None else steps, masks=masks or {}, runs=runs or {})
        spec.update(more)
        out.append((name, json.loads(json.dumps(spec))))        # (as it comes back from a manifest: tuples are lists)

    # row widths either side of the 256-thread row; one and two rows
    for w in (255, 256, 257, 300):
        add("width_%d" % w, [["bias_f", "b", 3, None, None], ["rig_f", "r", None, None]], w=w, h=12, rigidity=1.5,
            masks=dict(b=[w, 12, "rand"], r=[w, 12, "rand"]))
    add("image_2rows", [["bias_f", "b", 5, None, None], ["rig_f", "r", 0, 0]], w=300, h=2, rigidity=1.0, masks=dict(b=[300, 2, "rand"], r=[300, 2, "rand"]))
    add("mask_1row", [["bias_f", "b", 40, 0, 5], ["rig_f", "b", 0, 39]], rigidity=1.0, masks=dict(b=[300, 1, "rand"]))
    add("mask_2rows", [["bias_f", "b", 40, 0, 38], ["rig_f", "b", 3, 0]], rigidity=1.0, masks=dict(b=[300, 2, "rand"]))
    add("mask_1x1", [["bias_f", "b", 900, 17, 9], ["rig_f", "b", 299, 39], ["bias_f", "b", 900, 0, 0]], rigidity=2.0, masks=dict(b=[1, 1, "rand"]))
    # offsets, overhangs, larger than the image, wholly outside
    m = dict(b=[120, 20, "rand"], r=[120, 20, "rand"])
    for name, (xo, yo) in (("off_neg", (-30, -7)), ("off_pos", (200, 25)), ("over_left", (-30, 5)), ("over_right", (250, 5)),
                           ("over_top", (50, -10)), ("over_bottom", (50, 30))):
        add(name, [["bias_f", "b", 30, xo, yo], ["rig_f", "r", xo, yo]], rigidity=1.5, masks=m)
    add("larger", [["bias_f", "b", 30, -20, -5], ["rig_f", "r", -25, -9]], rigidity=1.5, masks=dict(b=[340, 50, "rand"], r=[340, 50, "rand"]))
    add("outside", [["bias_f", "b", 30, 400, 0], ["bias_f", "b", 30, -120, 3], ["bias_f", "b", 30, 0, 40], ["rig_f", "r", 0, -20], ["rig_f", "r", 300, 0]],
        rigidity=1.5, masks=m)
    add("outside_not_flat", [["resize", 290, 40], ["bias_f", "b", 30, 400, 0], ["rig_f", "r", 0, -20]], rigidity=1.5, masks=m, steps=[(280, 40)])
    # bias_factor negative, zero, large
    add("factor_negative", [["bias_f", "b", -5, None, None]], masks=dict(b=[300, 40, "rand"]))
    add("factor_zero", [["bias_f", "b", 0, None, None], ["bias_rgb", "g", 0]], masks=dict(b=[300, 40, "rand"], g=[300, 40, "rgb1"]))
    add("factor_zero_not_flat", [["resize", 290, 40], ["bias_f", "b", 0, 0, 0]], masks=dict(b=[300, 40, "rand"]), steps=[(280, 40)])
    add("factor_large", [["bias_f", "b", 1000000, None, None]], masks=dict(b=[300, 40, "rand"]))
    # a carver that is not flat when the mask arrives
    add("after_shrink", [["resize", 280, 40], ["bias_f", "b", 20, 5, 3], ["rig_f", "r", -8, 0]], rigidity=1.0, steps=[(270, 40)],
        masks=dict(b=[260, 30, "rand"], r=[280, 40, "rand"]))
    add("after_enlarge", [["resize", 330, 40], ["rig_f", "r", None, None], ["bias_f", "b", 20, 30, 3]], rigidity=1.0, steps=[(320, 40)],
        masks=dict(b=[260, 30, "rand"], r=[330, 40, "rand"]))
    add("xy_after_shrink", [["resize", 280, 40], ["bias_xy", "a"], ["rig_xy", "a"]], rigidity=1.0, steps=[(270, 40)], runs=dict(a=["some", "rand", 500]))
    # orientation 1 (a resize that ends with the height): a non-square mask, offsets, single values
    # (offsets with max(0, x_off) == max(0, y_off): elsewhere liblqr misplaces the mask, finding_cases() below)
    add("transposed", [["resize", 300, 36], ["bias_f", "b", 25, -37, -4], ["rig_f", "r", 20, 20], ["bias_xy", "a"], ["rig_xy", "c"]], rigidity=1.5,
        steps=[(300, 30)], masks=dict(b=[100, 20, "dyadic"], r=[50, 30, "dyadic"]), runs=dict(a=["some", "dyadic", 400], c=["some", "dyadic", 300]))
    add("transposed_tall", [["resize", 40, 290], ["bias_f", "b", 25, -5, -100], ["rig_f", "r", -15, -8], ["rig_f", "r", 30, 30], ["rig_xy", "c"], ["bias_rgb", "g", 70]],
        w=40, h=300, rigidity=1.5, steps=[(36, 290)], masks=dict(b=[30, 120, "dyadic"], r=[50, 30, "dyadic"], g=[40, 290, "bw"]),
        runs=dict(c=["shuffle", "dyadic"]))
    add("transposed_height_first", [["resize", 300, 36], ["bias_f", "b", 25, -40, -4], ["bias_f", "b", 25, 12, 12], ["rig_f", "r", 0, 0], ["bias_f", "r", 3, None, None]], res_order=1, rigidity=1.0,
        steps=[(294, 32)], masks=dict(b=[100, 20, "dyadic"], r=[300, 36, "dyadic"]))
    # accumulation on one pixel: values whose partial sums are exact in float
    d = dict(b=[200, 30, "dyadic"], c=[180, 25, "dyadic"], g=[300, 40, "bw"])
    add("acc_two_areas", [["bias_f", "b", 4, 20, 5], ["bias_f", "c", -2, 90, -3]], masks=d)
    add("acc_rgb_then_f", [["bias_rgb", "g", 64], ["bias_f", "b", 4, 50, 8], ["bias_rgb_area", "g", 32, 100, -10]], masks=d)
    add("acc_area_then_xy", [["bias_f", "b", 4, 0, 0], ["bias_xy", "a"]], masks=d, runs=dict(a=["shuffle", "dyadic"]))
    add("acc_xy_then_area", [["bias_xy", "a"], ["bias_f", "b", 8, 100, 10], ["bias_xy", "a"]], masks=d, runs=dict(a=["some", "dyadic", 3000]))
    add("rig_twice", [["rig_f", "b", 10, 5], ["rig_f", "c", 60, 10], ["rig_rgb_area", "g", 250, 20]], rigidity=2.0,
        masks=dict(b=[120, 20, "rand"], c=[120, 20, "rand"], g=[60, 30, "rgb2"]))
    # runs of single values
    add("xy_rowmajor", [["bias_xy", "a"], ["rig_xy", "a"]], rigidity=1.0, runs=dict(a=["rowmajor", "rand"]))
    add("xy_shuffle", [["bias_xy", "a"], ["rig_xy", "a"]], rigidity=1.0, runs=dict(a=["shuffle", "rand"]))
    add("xy_shuffle_tall", [["bias_xy", "a"]], w=40, h=300, steps=[(40, 292)], runs=dict(a=["shuffle", "rand"]))
    add("xy_repeat3", [["bias_xy", "a"], ["rig_xy", "b"]], rigidity=1.0, runs=dict(a=["repeat", "dyadic", 234, 3, 700], b=["repeat", "dyadic", 234, 3, 700]))
    add("xy_repeat3_wide", [["bias_xy", "a"], ["rig_xy", "b"]], rigidity=1.0, runs=dict(a=["repeat", "dyadic", 300, 3, 900], b=["repeat", "dyadic", 300, 3, 900]))
    add("xy_interrupted", [["bias_xy", "a"], ["rig_xy", "a"], ["resize", 290, 40], ["bias_xy", "b"], ["rig_xy", "b"]], rigidity=1.0, steps=[(284, 40)],
        runs=dict(a=["some", "dyadic", 2000], b=["some", "dyadic", 1500]))
    add("xy_interrupted_flat", [["bias_xy", "a"], ["resize", 290, 40], ["flatten"], ["planes"], ["bias_xy", "b"]], steps=[(284, 40)],
        runs=dict(a=["some", "dyadic", 2000], b=["some", "dyadic", 1500]))
    # clears
    r2 = dict(b=[300, 40, "rand"], r=[300, 40, "rand"], c=[100, 30, "rand"])
    add("unmasked", [], rigidity=1.0, seed=4999)
    add("clear_resize", [["bias_f", "b", 50, None, None], ["rig_f", "r", None, None], ["bias_xy", "a"], ["bias_clear"], ["rig_clear"]], rigidity=1.0, seed=4999,
        masks=r2, runs=dict(a=["some", "rand", 100]))
    add("clear_readd", [["bias_f", "b", 50, None, None], ["rig_f", "r", None, None], ["bias_clear"], ["rig_clear"], ["planes"], ["bias_f", "c", 9, 40, 2],
                        ["rig_f", "c", 150, 12]], rigidity=1.0, masks=r2)
    add("clear_drops_pending", [["bias_xy", "a"], ["rig_xy", "a"], ["bias_clear"], ["rig_clear"], ["bias_xy", "b"], ["rig_xy", "b"]], rigidity=1.0,
        runs=dict(a=["some", "rand", 900], b=["some", "rand", 50]))
    # delta_x and rigidity: a rigidity mask that matters switches the kernel family
    for delta in (1, 2):
        for rig in (0.0, 2.0):
            add("delta%d_rig%d" % (delta, int(rig)), [["bias_f", "b", 30, 60, 4], ["rig_f", "r", None, None]], delta=delta, rigidity=rig,
                masks=dict(b=[150, 30, "rand"], r=[300, 40, "rand"]))
    # masks are the same whatever the carver's depth
    add("depth_16i", [["bias_f", "b", 30, 60, 4], ["rig_f", "r", None, None], ["bias_xy", "a"]], ch=3, depth=1, rigidity=1.0, w=120, h=40,
        masks=dict(b=[80, 30, "dyadic"], r=[120, 40, "rand"]), runs=dict(a=["some", "dyadic", 300]))
    add("depth_32f", [["bias_f", "b", 30, 60, 4], ["rig_f", "r", None, None], ["rig_xy", "a"]], ch=4, depth=2, rigidity=1.0, w=120, h=40,
        masks=dict(b=[80, 30, "rand"], r=[120, 40, "dyadic"]), runs=dict(a=["some", "dyadic", 300]))
    # calls the library refuses: rigidity masks on an attached carver
    add("attached", [["aux", "rig_f", "r", None, None], ["aux", "rig_xy", "a"], ["aux", "rig_rgb", "g"], ["aux", "rig_rgb_area", "g", 0, 0],
                     ["bias_f", "r", 12, None, None], ["rig_f", "r", None, None]], aux=True, rigidity=1.0, w=120, h=40,
        masks=dict(r=[120, 40, "rand"], g=[120, 40, "rgb3"]), runs=dict(a=["some", "rand", 5]))
    # ... and before lqr_carver_init; the bias forms are served there
    add("late_init", [["rig_f", "r", None, None], ["rig_xy", "a"], ["rig_rgb", "g"], ["rig_rgb_area", "g", 0, 0], ["bias_f", "d", 12, None, None], ["bias_xy", "a"],
                      ["bias_rgb", "g", 90], ["planes"], ["init"], ["rig_f", "r", None, None], ["bias_f", "d", -3, 10, 10]], late_init=True, rigidity=1.0,
        w=120, h=40, masks=dict(r=[120, 40, "rand"], d=[120, 40, "dyadic"], g=[120, 40, "bw"]), runs=dict(a=["some", "dyadic", 40]))
    return out


# What the engine does not follow (include/lqr_masks.h says why) and is therefore in no case: the bias forms on an attached carver
# (liblqr keeps a plane that nothing reads), an _xy call outside the image (liblqr writes outside its plane), and
# lqr_carver_rigmask_add / _add_rgb (["rig_f", m, None, None], ["rig_rgb", m]) on a carver that is not flat or is in orientation 1
# (liblqr reads the mask with the row length of its buffers before the flattening, past the mask's end).


def finding_cases():
    """where the genuine build does something else than include/lqr_masks.h documents, recorded all the same (MANIFEST "findings"):
    a carver in orientation 1 and offsets whose positive parts differ -- liblqr adds them after it has swapped the axes, so the mask
    lands at (x + y_off, y + x_off).  Nothing is clipped in these, so the genuine planes are the model's with the offsets swapped
    (tests/test_masks_abi.py); the engine gives the model's (tests/test_masks_gpu.py)."""
    out = []
    for name, w, h, rs, ops in (
            ("transposed_offsets", 300, 40, (300, 36), [["bias_f", "b", 25, 20, 4], ["rig_f", "r", 12, 0], ["bias_rgb_area", "g", 64, 9, 20], ["rig_rgb_area", "g", 15, 7]]),
            ("transposed_offsets_tall", 40, 300, (40, 290), [["bias_f", "b", 25, 3, 15], ["rig_f", "r", 0, 20]])):
        spec = dict(seed=7000 + len(out), w=w, h=h, ch=1, depth=0, nrg=2, delta=1, rigidity=1.0, ops=[["resize"] + list(rs)] + ops,
                    steps=[(rs[0] - 4, rs[1])], masks=dict(b=[20, 12, "rand"], r=[14, 20, "rand"], g=[16, 10, "rgb2"]), runs={})
        out.append((name, json.loads(json.dumps(spec))))
    return out


def swapped_offsets(spec):
    """the spec with x_off and y_off of every area op exchanged"""
    spec = json.loads(json.dumps(spec))
    for op in spec["ops"]:
        if op[0] in ("bias_f", "bias_rgb_area"):
            op[3], op[4] = op[4], op[3]
        elif op[0] in ("rig_f", "rig_rgb_area"):
            op[2], op[3] = op[3], op[2]
    return spec
