"""The energy read-out cases (include/lqr_energy.h: lqr_carver_get_true_energy, lqr_carver_get_energy, lqr_carver_get_energy_image):
specs, the driver that runs one through any library whose carver class has binding.Carver's methods -- the genuine liblqr
(scripts/ref_engine/make_energy_golden.py, which records tests/golden/energy/) and the HIP engine (tests/test_energy_gpu.py, which
reproduces the records) -- and a numpy model of what the calls make of the true energy, checked against the genuine planes and
pictures without a GPU (tests/test_energy_abi.py).

A spec is a small JSON-able dict:
  seed, w, h, ch, depth (LqrColDepth), nrg, delta, rigidity, res_order      the carver, as in coldepth_cases
  const         every value of the (8-bit) image is this number
  type          the carver's LqrImageType, set after creation (lqr_carver_set_image_type); max_ch as in imgtype_cases
  late_init     the carver is created without lqr_carver_init; the op ["init"] calls it
  aux           an attached carver of the same size; its image is recorded after every step too
  ops           applied in order; the return value and the orientation after each are recorded:
                ["resize", w, h] ["init"]
                ["bias", kind, factor]      lqr_carver_bias_add on a mask of the carver's size: "pos" [0.1, 2), "neg" (-2, -0.1], "mixed" [-1, 1),
                                            "negconst" -1 everywhere
                ["true", o] ["norm", o]     lqr_carver_get_true_energy / lqr_carver_get_energy with orientation o
                ["image", o, depth, type]   lqr_carver_get_energy_image
                ["null", form, o]           the same calls (form 0 true, 1 norm, 2 image as GREY 8I) with a NULL buffer
                ["aux", form, o]            ... on the attached carver (finding_cases only)
  steps         [(w, h), ...] resizes after the ops; image and visibility map are recorded after each
Every read-out writes into a buffer of 0xA5 bytes that is GUARD bytes longer than the result; "norm" and "image" are preceded by a
"true" read-out of the same orientation (key "true@i"), which changes nothing the op itself would not change and is what the model
starts from.  A call that fails must leave the buffer as it was.
"""
import json

import numpy as np

import coldepth_cases as CD
import imgtype_cases as IT

GUARD = 64
DTYPES = {0: np.uint8, 1: np.uint16, 2: np.float32, 3: np.float64}
RULES_NOTE = ("s = 1 / (1 + 1 / e) (e >= 0), -1 / (1 - 1 / e) (e < 0), float operations; e_max from 0, e_min from FLT_MAX; "
              "(s - e_min) / (e_max - e_min) if e_max > e_min; pictures: the squash in double rounded to float once, the normalisation (0 if "
              "e_max == e_min) and 1 - e in double, (guchar) (v * 255), (guint16) (v * 65535), (gfloat) v, v")


# ---- the model ----------------------------------------------------------------------------------------------------------------
def squash(e):
    """float32 in, float32 out, every operation rounded to float"""
    e = np.asarray(e, np.float32)
    one = np.float32(1)
    with np.errstate(divide="ignore"):
        pos = one / (one + one / e)
        neg = -one / (one - one / e)
    return np.where(e >= 0, pos, neg).astype(np.float32)


def normalised(true):
    """lqr_carver_get_energy of a true-energy plane"""
    s = squash(true)
    e_max = np.float32(max(np.float32(0), s.max()))
    e_min = np.float32(min(np.finfo(np.float32).max, s.min()))
    if e_max > e_min:
        s = ((s - e_min) / (e_max - e_min)).astype(np.float32)
    return s


def picture(true, depth, image_type):
    """lqr_carver_get_energy_image of a true-energy plane: h x w x channels of the depth's dtype.  liblqr's picture loop is its own,
    mixed float / double code; as the 53-bit build evaluates it the squash is computed in double and rounded to float once, e_min and
    e_max are floats, and the normalisation and 1 - e stay in double; where e_max == e_min the picture is that of 0"""
    ch = IT.TYPE_CHANNELS[image_type]
    t = np.asarray(true, np.float32).astype(np.float64)
    with np.errstate(divide="ignore"):
        s = np.where(t >= 0, 1.0 / (1.0 + 1.0 / t), -1.0 / (1.0 - 1.0 / t)).astype(np.float32)
    e_max = np.float32(max(np.float32(0), s.max()))
    e_min = np.float32(min(np.finfo(np.float32).max, s.min()))
    if e_max > e_min:
        e = (s.astype(np.float64) - np.float64(e_min)) / (np.float64(e_max) - np.float64(e_min))
    else:
        e = np.zeros(s.shape, np.float64)
    inv = 1.0 - e

    def store(v):
        v = np.asarray(v, np.float64)
        if depth == 0:
            return np.trunc(v * 255.0).astype(np.uint8)
        if depth == 1:
            return np.trunc(v * 65535.0).astype(np.uint16)
        return v.astype(DTYPES[depth])

    out = np.zeros(s.shape + (ch,), DTYPES[depth])
    colour = ch - (image_type in (IT.RGBA, IT.GREYA, IT.CMYKA))
    if image_type in (IT.CMYK, IT.CMYKA):
        out[:, :, :3] = store(0.0)
        out[:, :, 3] = store(inv)
    else:
        out[:, :, :colour] = store(inv if image_type == IT.CMY else e)[:, :, None]
    if colour < ch:
        out[:, :, ch - 1] = store(1.0)
    return out


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def make_input(spec):
    rng = np.random.default_rng(spec["seed"])
    v8 = CD.base_image(rng, spec["w"], spec["h"], spec["ch"])
    if spec.get("const") is not None:
        v8[:] = spec["const"]
    img = CD.to_depth(rng, v8, spec["depth"])
    extra = {}
    if spec.get("aux"):
        extra["aux"] = CD.base_image(rng, spec["w"], spec["h"], 3)
    return img, extra


def bias_mask(spec, index, kind, w, h):
    rng = np.random.default_rng([spec["seed"], 31, index])
    if kind == "negconst":
        return np.full((h, w), -1.0)
    lo, hi = {"pos": (0.1, 2.0), "neg": (-2.0, -0.1), "mixed": (-1.0, 1.0)}[kind]
    return rng.uniform(lo, hi, (h, w))


# ---- the driver ---------------------------------------------------------------------------------------------------------------
def _readout(c, form, o, depth, image_type, null=False):
    """(ret, array or None, intact): the result shaped in image orientation when the call returned LQR_OK; intact: the guard bytes
    (after a failure: the whole buffer) are still 0xA5"""
    g = c.getters()
    w, h = g["width"], g["height"]
    dt = np.dtype(DTYPES[depth if form == 2 else 2])
    ch = IT.TYPE_CHANNELS.get(image_type, 5) if form == 2 else 1            # (LQR_CUSTOM_IMAGE: room for the widest type)
    n = w * h * ch * dt.itemsize
    ret, buf = c.energy_call(form, o, depth, image_type, nbytes=n, guard=GUARD, null=null)
    if ret != 1:
        return ret, None, bool((buf == 0xa5).all())
    arr = buf[:n].view(dt).reshape((h, w, ch) if form == 2 else (h, w)).copy()
    return ret, arr, bool((buf[n:] == 0xa5).all())


def run(api, cls, spec, img=None, extra=None):
    """drive one case; returns a dict of arrays and a JSON record"""
    if img is None:
        img, extra = make_input(spec)
    prev = None
    if spec.get("max_ch") and hasattr(api, "lqrx_set_max_channels"):
        prev = api.lqrx_set_max_channels(spec["max_ch"])
    try:
        c = cls.from_ext(api, img, spec["depth"], init=not spec.get("late_init"), delta_x=spec.get("delta", 1), rigidity=spec.get("rigidity", 0.0))
        aux = c.attach_ext(extra["aux"], 0) if "aux" in extra else None
    finally:
        if prev is not None:
            api.lqrx_set_max_channels(prev)
    if spec.get("type") is not None:
        assert c.set_image_type(spec["type"]) == 1
    c.configure(nrg_func=spec["nrg"], res_order=spec.get("res_order", 0), switch_freq=2, enl_step=1.5)
    out, rec = {}, {"rets": [], "orientation": [], "intact": [], "step_rets": [], "getters": [], "vmap_meta": []}
    for i, op in enumerate(spec["ops"]):
        kind, a = op[0], op[1:]
        intact = None
        if kind == "resize":
            ret = c.resize(a[0], a[1])
        elif kind == "init":
            ret = c.init(spec.get("delta", 1), spec.get("rigidity", 0.0))
        elif kind == "bias":
            g = c.getters()
            ret = c.bias_add_f(bias_mask(spec, i, a[0], g["width"], g["height"]), a[1])
        elif kind == "true":
            ret, arr, intact = _readout(c, 0, a[0], 2, IT.GREY)
            if arr is not None:
                out["out@%d" % i] = arr
        elif kind in ("norm", "image"):
            form, depth, image_type = (1, 2, IT.GREY) if kind == "norm" else (2, a[1], a[2])
            r0, t, i0 = _readout(c, 0, a[0], 2, IT.GREY)
            if t is not None:
                out["true@%d" % i] = t
            ret, arr, intact = _readout(c, form, a[0], depth, image_type)
            if arr is not None:
                out["out@%d" % i] = arr
            ret, intact = [r0, ret], [i0, intact]
        elif kind == "null":
            ret, _, intact = _readout(c, a[0], a[1], 0, IT.GREY, null=True)
        elif kind == "aux":
            ret, arr, intact = _readout(aux, a[0], a[1], 0, IT.GREY)
            if arr is not None:
                out["out@%d" % i] = arr
        else:
            raise ValueError(kind)
        rec["rets"].append(ret)
        rec["intact"].append(intact)
        rec["orientation"].append(c.getters()["orientation"])
    rec["after_ops"] = c.getters()
    for i, (w1, h1) in enumerate(spec["steps"]):
        ret = c.resize(w1, h1)
        rec["step_rets"].append(ret)
        if ret != 1:
            break
        out["image%d" % i] = c.scan_line_ext()[0]
        if aux is not None:
            out["aux_image%d" % i] = aux.scan_line_ext()[0]
        v = c.vmap_dump()
        out["vmap%d" % i] = v["data"]
        rec["vmap_meta"].append([v["depth"], v["orientation"]])
        rec["getters"].append(c.getters())
    c.destroy()
    out["record"] = np.array(json.dumps(rec, sort_keys=True))
    return out


assert_same_record = CD.assert_same_record


def model_check(spec, out):
    """(planes and pictures compared, keys that differ): the model applied to every recorded "true@i" against the recorded "out@i\""""
    compared, differ = 0, []
    for i, op in enumerate(spec["ops"]):
        if op[0] not in ("norm", "image") or "out@%d" % i not in out:
            continue
        t = out["true@%d" % i]
        want = normalised(t) if op[0] == "norm" else picture(t, op[2], op[3])
        got = out["out@%d" % i]
        compared += 1
        if got.dtype != want.dtype or got.shape != want.shape or not np.array_equal(CD.bits(got), CD.bits(want)):
            differ.append("out@%d" % i)
    return compared, differ


# ---- the cases ----------------------------------------------------------------------------------------------------------------
def cases():
    """small images (the widest 130 px): every rule of include/lqr_energy.h once"""
    out = []

    def add(name, ops, w=33, h=17, steps=(), **more):
        spec = dict(seed=9000 + len(out), w=w, h=h, ch=3, depth=0, nrg=2, delta=1, rigidity=0.0, ops=ops, steps=[list(s) for s in steps])
        spec.update(more)
        out.append((name, json.loads(json.dumps(spec))))

    # the seven built-in energy functions, both orientations; 0 -> 1 -> 0
    for nrg in range(7):
        add("ef%d" % nrg, [["norm", 0], ["norm", 1], ["true", 1]] + ([["norm", 0], ["true", 0]] if nrg == 2 else []), nrg=nrg)
    # carver states: shrunk and not flattened (stays as it is for its own orientation), enlarged, orientation 1 from a height change
    add("shrunk", [["resize", 57, 33], ["norm", 0], ["true", 0], ["norm", 1]], w=65, h=33, steps=[(60, 30)])
    add("shrunk_regrown", [["resize", 57, 33], ["resize", 61, 33], ["norm", 0]], w=65, h=33, steps=[(58, 33)])
    add("enlarged", [["resize", 75, 33], ["norm", 0], ["image", 1, 0, IT.RGBA]], w=65, h=33, steps=[(70, 33)])
    add("height_changed", [["resize", 65, 28], ["norm", 1], ["norm", 0], ["image", 1, 1, IT.GREYA]], w=65, h=33, steps=[(65, 25)])
    add("height_shrunk_only", [["resize", 65, 28], ["true", 1], ["norm", 1]], w=65, h=33)
    # bias: positive, all negative under LQR_EF_NULL (e_max starts at 0), mixed
    add("bias_pos", [["bias", "pos", 40], ["norm", 0], ["norm", 1]])
    add("bias_neg_null", [["bias", "neg", 40], ["norm", 0], ["norm", 1], ["image", 0, 0, IT.GREY], ["image", 1, 3, IT.CMYKA]], nrg=6)
    add("bias_mixed_null", [["bias", "mixed", 40], ["norm", 0], ["norm", 1]], nrg=6)
    add("bias_mixed", [["bias", "mixed", 60], ["norm", 1], ["norm", 0]], nrg=0)
    # constant planes
    add("const_null", [["norm", 0], ["norm", 1], ["image", 0, 0, IT.RGBA], ["image", 0, 2, IT.CMYK]], nrg=6)
    add("const_colour", [["norm", 0], ["norm", 1], ["image", 1, 1, IT.CMY]], nrg=0, const=77)
    add("const_negative", [["bias", "negconst", 12], ["norm", 0], ["norm", 1]], nrg=6)
    # the carver's own depth and type change only what the energy reads
    add("carver_16i", [["norm", 0], ["norm", 1]], depth=1, nrg=0)
    add("carver_32f", [["norm", 0], ["norm", 1]], depth=2, nrg=3, ch=4)
    add("carver_64f", [["norm", 1], ["norm", 0]], depth=3, nrg=1, ch=1)
    add("carver_cmyk", [["norm", 0], ["image", 1, 0, IT.RGB]], ch=4, type=IT.CMYK, nrg=0)
    add("carver_cmyka", [["norm", 0], ["image", 1, 2, IT.GREY]], ch=5, max_ch=5, nrg=4)
    # every output format on one tiny image, LQR_CUSTOM_IMAGE
    add("formats", [["image", (d + t) % 2, d, t] for d in range(4) for t in range(7)] + [["image", 0, 0, IT.CUSTOM], ["image", 1, 2, IT.CUSTOM]], w=7, h=5)
    # argument errors
    add("bad_arguments", [["norm", 2], ["true", -1], ["image", 3, 0, IT.RGB], ["null", 0, 0], ["null", 1, 1], ["null", 2, 0], ["norm", 0]], w=9, h=6)
    # before lqr_carver_init
    add("late_alone", [["norm", 0], ["true", 1], ["image", 1, 0, IT.RGBA]], late_init=True)
    add("late_then_resize", [["norm", 1], ["init"]], late_init=True, rigidity=1.5, steps=[(28, 17), (28, 14)])
    # a resize after the read-out, on an initialised carver
    add("then_resize", [["norm", 1]], rigidity=1.0, steps=[(27, 17)])
    add("then_resize_height", [["norm", 0]], rigidity=1.0, steps=[(33, 13)], res_order=1)
    # the root's read-out with an attached carver
    add("attached", [["norm", 1]], aux=True, steps=[(27, 17), (27, 14)])
    # degenerate sizes, a wide strip
    # (in the orientation whose frame is more than one pixel wide; the others are finding_cases)
    add("size_1xn", [["norm", 1], ["image", 1, 1, IT.RGBA]], w=1, h=9)
    add("size_nx1", [["norm", 0], ["image", 0, 2, IT.CMY]], w=9, h=1)
    add("strip_130x3", [["norm", 0], ["norm", 1]], w=130, h=3, nrg=1)
    return out


def finding_cases():
    """what include/lqr_energy.h does not follow, recorded all the same (MANIFEST "findings"):
    * the calls on an ATTACHED carver, which liblqr serves (and, where the orientation differs, transposes alone); the engine returns
      LQR_ERROR and changes nothing;
    * a frame ONE pixel wide (an image 1 wide seen by vertical seams, 1 high seen by horizontal ones): liblqr's gradient reads the
      neighbour outside the frame -- the pixel of the next row; nothing (0) after the last one -- and reports that difference; the
      engine's energy is 0 there, as its carving always had it.  What the calls make of that energy is the model's in both."""
    out = []

    def add(name, ops, w=33, h=17, **more):
        spec = dict(seed=9900 + len(out), w=w, h=h, ch=3, depth=0, nrg=2, delta=1, rigidity=0.0, ops=ops, steps=[])
        spec.update(more)
        out.append((name, json.loads(json.dumps(spec))))

    add("attached_same_orientation", [["aux", 0, 0], ["aux", 1, 0]], aux=True)
    add("attached_other_orientation", [["aux", 1, 1]], aux=True)
    add("size_1x1", [["norm", 0], ["norm", 1], ["image", 0, 0, IT.RGB]], w=1, h=1)
    add("size_1xn_o0", [["norm", 0], ["image", 0, 1, IT.RGBA]], w=1, h=9)
    add("size_nx1_o1", [["norm", 1], ["image", 1, 2, IT.CMY]], w=9, h=1)
    return out
