"""The image-type cases (include/lqr_imagetype.h: CMY, CMYK, CMYKA and custom-channel carvers): specs, the driver that runs one
through any library whose carver class has binding.Carver's methods -- the genuine liblqr (scripts/ref_engine, which records
tests/golden/imgtype/) and the HIP engine (tests/test_imgtype_gpu.py, which reproduces the records) -- and a numpy model of the
value the energy reads, checked against the genuine lqr_carver_read_brightness / lqr_carver_read_luma without a GPU.

A spec is a coldepth_cases spec (which see) plus
  type, alpha, black   set after lqr_carver_init, in this order, each if present (lqr_carver_set_image_type / _alpha_channel /
                       _black_channel)
  type_at              [[step, op], ...]: op is applied before step `step` (0: after the three above); op is a type (int), or
                       {"alpha": i} / {"black": i}; calls that the library refuses are part of it (their return value is recorded)
  aux_ops              ops applied to the attached carver
  max_ch               the channel limit the engine is given for the case (lqrx_set_max_channels; liblqr has none)
Every return value of a setter is recorded ("type_rets"), and the type read back after each.
"""
import json
import re

import numpy as np

import coldepth_cases as CD

MAX_FILE = 804240                       # bytes: the largest golden file committed before the image-type vectors

RGB, RGBA, GREY, GREYA, CMY, CMYK, CMYKA, CUSTOM = range(8)
TYPE_CHANNELS = {RGB: 3, RGBA: 4, GREY: 1, GREYA: 2, CMY: 3, CMYK: 4, CMYKA: 5}
TYPE_ROLES = {GREYA: (1, -1), RGBA: (3, -1), CMYK: (-1, 3), CMYKA: (4, 3)}      # (alpha, black); every other type: none
DEFAULT_TYPE = {1: GREY, 2: GREYA, 3: RGB, 4: RGBA, 5: CMYKA}                   # 6 and more channels: CUSTOM


# ---- the setters' rules, as the genuine code was seen to apply them -----------------------------------------------------------
class TypeState:
    """type, alpha and black channel of a carver of `ch` channels; apply(op) returns what the setter returns (1 OK, 0 ERROR)"""

    def __init__(self, ch):
        self.ch = ch
        self.type = DEFAULT_TYPE.get(ch, CUSTOM)
        self.alpha, self.black = TYPE_ROLES.get(self.type, (-1, -1))

    def apply(self, op):
        if isinstance(op, dict):
            (role, i), = op.items()
            if i >= self.ch:
                return 0
            other = "black" if role == "alpha" else "alpha"
            if i < 0:
                i = -1
            elif getattr(self, other) == i:
                setattr(self, other, -1)
            setattr(self, role, i)
            self.type = CUSTOM
            return 1
        if op != CUSTOM and TYPE_CHANNELS.get(op) != self.ch:
            return 0
        self.type = op
        self.alpha, self.black = TYPE_ROLES.get(op, (-1, -1))
        return 1

    def key(self):
        return (self.type, self.alpha, self.black)


def initial_ops(spec):
    ops = []
    if spec.get("type") is not None:
        ops.append(spec["type"])
    if spec.get("alpha") is not None:
        ops.append({"alpha": spec["alpha"]})
    if spec.get("black") is not None:
        ops.append({"black": spec["black"]})
    return ops + [op for at, op in spec.get("type_at", []) if at == 0]


def state_of(spec, before_step=0):
    """the TypeState of the spec's root carver before step `before_step`"""
    st = TypeState(spec["ch"])
    for op in initial_ops(spec):
        st.apply(op)
    for at, op in spec.get("type_at", []):
        if 0 < at <= before_step:
            st.apply(op)
    return st


# ---- the value the energy reads (lqr_imagetype.h), every operation rounded individually in double -----------------------------
def normalised(img, depth):
    img = np.asarray(img)
    if depth == 0:
        return img.astype(np.float64) / 255.0
    if depth == 1:
        return img.astype(np.float64) / 65535.0
    return img.astype(np.float64)


def model_value(img, depth, st, luma):
    """h x w float64: lqr_carver_read_brightness (luma: lqr_carver_read_luma) of every pixel of an image of type `st`"""
    n = normalised(img, depth)
    one = np.float64(1.0)
    if st.type in (GREY, GREYA):
        b = n[:, :, 0].copy()
    elif st.type == CUSTOM:
        bf = n[:, :, st.black] if st.black >= 0 else np.zeros(n.shape[:2])
        s = np.zeros(n.shape[:2])
        cnt = 0
        for k in range(n.shape[2]):
            if k in (st.alpha, st.black):
                continue
            s = s + (one - (one - n[:, :, k]) * (one - bf))
            cnt += 1
        with np.errstate(invalid="ignore", divide="ignore"):
            s = s / np.float64(cnt)
        b = one - s if st.black >= 0 else s
    else:
        r, g, bl = n[:, :, 0], n[:, :, 1], n[:, :, 2]
        if st.type in (CMY, CMYK, CMYKA):
            r, g, bl = one - r, one - g, one - bl
            if st.type != CMY:
                k = one - n[:, :, 3]
                r, g, bl = r * k, g * k, bl * k
        b = (0.2126 * r + 0.7152 * g) + 0.0722 * bl if luma else ((r + g) + bl) / 3.0
    if st.alpha >= 0:
        b = b * n[:, :, st.alpha]
    return b


# ---- the driver ---------------------------------------------------------------------------------------------------------------
def _apply(c, op):
    if isinstance(op, dict):
        (role, i), = op.items()
        return c.set_alpha_channel(i) if role == "alpha" else c.set_black_channel(i)
    return c.set_image_type(op)


def run(api, cls, spec, img=None, extra=None):
    """coldepth_cases.run with the image-type calls; returns a dict of arrays and JSON-able records"""
    if img is None:
        img, extra = CD.make_input(spec)
    prev = None
    if spec.get("max_ch") and hasattr(api, "lqrx_set_max_channels"):
        prev = api.lqrx_set_max_channels(spec["max_ch"])
    try:
        c = cls.from_ext(api, img, spec["depth"], delta_x=spec.get("delta", 1), rigidity=spec.get("rigidity", 0.0),
                         preserve=spec.get("preserve", False))
        aux = c.attach_ext(extra["aux"], spec["aux_depth"]) if "aux" in extra else None
    finally:
        if prev is not None:
            api.lqrx_set_max_channels(prev)
    before = c.input_bytes() if spec.get("preserve") else None
    rec = {"rets": [], "getters": [], "lines": [], "scan_rets": [], "type_rets": [], "aux_type_rets": []}

    def ops(carver, todo, key):
        for op in todo:
            ret = _apply(carver, op)
            rec[key].append([ret, carver.getters_ext()["image_type"]])

    rec["default_type"] = c.getters_ext()["image_type"]
    ops(c, initial_ops(spec), "type_rets")
    if aux is not None:
        rec["aux_default_type"] = aux.getters_ext()["image_type"]
        ops(aux, spec.get("aux_ops", []), "aux_type_rets")
    if "bias" in extra:
        assert c.bias_add(extra["bias"], spec.get("bias_factor", 2000)) == 1
    if "rigmask" in extra:
        assert c.rigmask_add(extra["rigmask"]) == 1
    c.configure(nrg_func=spec["nrg"], res_order=spec.get("res_order", 0), switch_freq=spec.get("switch", 2),
                enl_step=spec.get("enl_step", 1.5), dump_vmaps=spec.get("dump_vmaps", False), progress=True)
    out = {}
    for i, st in enumerate(spec["steps"]):
        ops(c, [op for at, op in spec.get("type_at", []) if at == i and i > 0], "type_rets")
        ret = c.flatten() if st == "flatten" else c.resize(st[0], st[1])
        rec["rets"].append(ret)
        if ret != 1:
            break
        im, order = c.scan_ext()
        lim, lines = c.scan_line_ext()
        assert np.array_equal(im.view(np.uint8), lim.view(np.uint8)), "scan_ext and scan_line_ext disagree"
        out["image%d" % i] = im
        out["order%d" % i] = np.array(order, np.int32).reshape(-1, 2)
        rec["lines"].append(lines)
        rec["getters"].append(c.getters_ext())
        rec["scan_rets"].append(c.scan_rets())
        v = c.vmap_dump()
        out["vmap%d" % i] = v["data"]
        rec.setdefault("vmap_meta", []).append([v["depth"], v["orientation"]])
        if aux is not None:
            out["aux%d" % i] = aux.scan_ext()[0]
            rec.setdefault("aux_types", []).append(aux.getters_ext()["image_type"])
    for k, v in enumerate(c.dumped_vmaps()):
        out["dumped%d" % k] = v["data"]
        rec.setdefault("dumped_meta", []).append([v["depth"], v["orientation"]])
    rec["events"] = [list(e) for e in c.events]
    c.destroy()
    if spec.get("preserve"):
        rec["input_unchanged"] = c.input_bytes() == before
        c.free_input()
    out["record"] = np.array(json.dumps(rec, sort_keys=True))
    return out


assert_same_record = CD.assert_same_record

# ---- the small vectors --------------------------------------------------------------------------------------------------------
# name -> (channels, the spec fields that make the layout)
LAYOUTS = [
    ("cmy", 3, dict(type=CMY)),
    ("cmyk", 4, dict(type=CMYK)),
    ("cmyka", 5, dict()),                                       # the default of five channels
    ("custom6", 6, dict()),                                     # the default of six: no alpha, no black
    ("custom_a", 4, dict(alpha=1)),
    ("custom_k", 9, dict(black=8)),
    ("custom_ak", 7, dict(alpha=5, black=2)),
    ("moved", 5, None),                                         # a role moved onto the index the other holds (both directions)
]
NRG_PAIRS = {0: (0, 3), 1: (1, 4), 2: (2, 5), 3: (0, 5)}        # per depth: one brightness-kind and one luma-kind energy


def cases():
    """types x depths x {a brightness energy, a luma energy}, the options spread over them; the refused calls; one interactive
    sequence per depth with a type change on a carver that is not flat"""
    out = []

    def add(name, **spec):
        spec.setdefault("seed", 3000 + len(out))
        if spec["ch"] > 4 or spec.get("aux_ch", 0) > 4:
            spec.setdefault("max_ch", max(spec["ch"], spec.get("aux_ch", 0)))
        out.append((name, spec))

    n = 0
    for depth in (0, 1, 2, 3):
        d = CD.DEPTH_NAMES[depth]
        for li, (lname, ch, fields) in enumerate(LAYOUTS):
            for j, nrg in enumerate(NRG_PAIRS[depth]):
                if fields is None:      # CMYKA: black takes alpha's channel 4 / alpha takes black's channel 3
                    fields_j = dict(type_at=[[0, {"black": 4}]]) if j == 0 else dict(type_at=[[0, {"alpha": 3}]])
                else:
                    fields_j = dict(fields)
                w, h = [(40, 28), (36, 24), (32, 26), (44, 20)][(li + j + depth) % 4] if depth >= 2 else [(48, 32), (40, 28), (56, 36), (36, 44)][(li + j) % 4]
                opt = n % 8
                n += 1
                spec = dict(w=w, h=h, ch=ch, depth=depth, nrg=nrg, res_order=(li + j) % 2, **fields_j)
                if opt == 0:
                    spec.update(steps=[(w - 9, h)], bias=True, rigmask=True, rigidity=2.0)
                elif opt == 1:
                    spec.update(steps=[(w - 8, h - 4)], delta=2, rigidity=0.6)
                elif opt == 2:
                    spec.update(steps=[(w + 7, h)])
                elif opt == 3:
                    spec.update(steps=[(w + 19, h)], enl_step=1.3)                 # enlargement in several steps
                elif opt == 4:
                    spec.update(steps=[(w - 6, h - 5)], preserve=True)
                elif opt == 5:
                    spec.update(steps=[(w - 10, h)], delta=5, rigidity=1.5)
                elif opt == 6:
                    spec.update(steps=[(w + 5, h - 4)], edge=True)
                else:                                                            # an attached carver of another type, depth and width
                    spec.update(steps=[(w - 7, h + 5)], aux_depth=(depth + 1 + li) % 4, aux_ch=(5, 7)[depth % 2],
                                aux_ops=[[CUSTOM], [{"alpha": 0}, {"black": 6}, CMY]][depth % 2])
                add("%s_%s_e%d" % (lname, d, nrg), **spec)
    # refused calls: a type of another channel count, an index out of range; the type stays as it was and the carve is that type's
    add("refused_8i", w=40, h=28, ch=4, depth=0, nrg=0, type=CMYK, type_at=[[0, GREY], [0, CMYKA], [0, {"alpha": 4}], [0, {"black": 9}]],
        steps=[(32, 28)])
    add("refused_32f", w=36, h=24, ch=6, depth=2, nrg=4, type_at=[[0, CMYKA], [0, {"black": 6}], [0, {"alpha": -3}], [0, RGB]], steps=[(30, 24)])
    # shrink, type change on the carver that is not flat, shrink on, flatten, enlarge
    for depth in (0, 1, 2, 3):
        w, h = (48, 32) if depth < 2 else (36, 24)
        add("interactive_%s" % CD.DEPTH_NAMES[depth], w=w, h=h, ch=5, depth=depth, nrg=(0, 4, 2, 3)[depth],
            type_at=[[1, {"alpha": -1}], [3, {"black": 1}]], steps=[(w - 8, h), (w - 14, h - 3), "flatten", (w - 4, h - 3)], dump_vmaps=True)
    # tests/c/cmyka_replay.c: an ImageMagick-style caller -- library defaults, a preserved 32F five-channel buffer
    add("cmyka_replay_32f", w=44, h=30, ch=5, depth=2, nrg=2, steps=[(35, 26)], switch=0, enl_step=2.0, preserve=True)
    return out


PLANE_CASES = ("cmy_8i_e0", "cmyk_16i_e1", "cmyka_32f_e2", "custom6_64f_e0", "custom_a_8i_e0", "custom_k_16i_e4", "custom_ak_32f_e5",
               "moved_8i_e0", "moved_64f_e5", "custom_ak_8i_e3", "cmyk_32f_e5", "custom_k_64f_e0")


def mid_cases():
    """only where the image-type code has a size boundary of its own: the 256-column rank chunks of the 8I value-plane layout and
    of the inflate and compaction passes at pixel sizes that are no power of two, the transpose of such pixels, and an 8I
    value-plane carver through a mid-session catch-up and a second block of energy rows"""
    out = []

    def add(name, **spec):
        spec.setdefault("seed", 9000 + len(out))
        if spec["ch"] > 4:
            spec.setdefault("max_ch", spec["ch"])
        out.append((name, spec))

    def seq(w, h, **more):      # all2 / all3: 38 seams, a type change on the carver that is not flat, 42 more, flatten, enlarge
        return dict(w=w, h=h, steps=[(w - 38, h), (w - 80, h), "flatten", (w - 40 + 10 * (w > 400), h)], **more)

    seq2, seq3 = seq(340, 12), seq(600, 12, dump_vmaps=True)
    # 48-byte pixels of noise-like doubles do not compress: five 600 x 12 images of them make a 1.4 MB file, over the limit of
    # MAX_FILE bytes a golden file has here.  The 64F layout therefore passes 512 columns at 6 rows, the most that fits; no pass
    # that moves pixels looks at the row count (they walk rows one by one), so the third 256-column chunk is reached all the same.
    seq3_64f = seq(600, 6, dump_vmaps=True)
    for lname, ch, depth, fields, seqs in (
            ("cmyka_8i", 5, 0, dict(), (seq2, seq3)), ("custom7_8i", 7, 0, dict(alpha=5, black=2), (seq2, seq3)),
            ("cmyka_16i", 5, 1, dict(), (seq2, seq3)), ("cmyka_32f", 5, 2, dict(), (seq2, seq3)),
            ("custom6_64f", 6, 3, dict(), (seq2, seq3_64f))):
        for k, sq in enumerate(seqs):
            add("all%d_%s" % (k + 2, lname), ch=ch, depth=depth, nrg=(0, 4)[k], type_at=[[1, {"alpha": -1}] if ch != 6 else [1, {"black": 0}]],
                edge=(k == 0), **dict(fields, **sq))
    add("enlv_cmyka_8i", w=24, h=264, ch=5, depth=0, nrg=2, steps=[(30, 300)], res_order=1)
    add("enlv_custom7_16i", w=24, h=264, ch=7, depth=1, nrg=3, alpha=6, steps=[(30, 300)], res_order=1)
    add("tall_cmyk_8i", w=90, h=140, ch=4, depth=0, nrg=1, type=CMYK, steps=[(50, 140)])
    return out


def reads_value(spec, st):
    """the engine's rule: the carver reads through the value plane.  (The same rule, in C: reads_value in csrc/lqr_shim.hip, from
    the mode that read_mode in host/lqr_carver.c hands it; test_imgtype_gpu.same_config groups by it.  Keep the three in step.)"""
    return spec["depth"] != 0 or spec["ch"] > 4 or st.key() not in ((GREY, -1, -1), (GREYA, 1, -1), (RGB, -1, -1), (RGBA, 3, -1))


WIDE_TAGS = ("inflate", "compact", "transpose")         # coldepth_cases.boundaries' labels that carry the pixel size: "<tag>:b<bytes>"


def boundaries(spec, K, group=1):
    """coldepth_cases.boundaries for a spec of this file.  That walk is liblqr's bookkeeping of sizes and sessions and knows
    nothing of types, so two things are translated for it; what it must keep doing for this to hold is asserted below.

      - A setter that changes what the energy reads between two steps invalidates the working planes exactly as
        lqrhip_carver_set_read_luma does (lqr_imagetype.h), and the walk has one notion of that: spec["nrg_at"], a change between
        a brightness and a luma energy.  Each such type change is handed over as an nrg_at entry of the other kind at its step.
        The walk looks at nrg_at for nothing but "the planes are laid out again" (relayout:cN).
      - The walk counts a carver only if depth != 0.  An 8I carver that reads through the value plane takes the same kernels, so
        it is walked as the 16I carver of its shape; of the labels only WIDE_TAGS carry the pixel size, which is put back to
        channels x 1 byte (and dropped at 4 bytes and less, where the walk drops it too)."""
    marks, luma = [], spec["nrg"] in (3, 4, 5)
    for at in sorted({at for at, _ in spec.get("type_at", []) if at > 0}):
        if state_of(spec, at).key() != state_of(spec, at - 1).key():
            luma = not luma                                                 # (each change flips the walk's flag once more)
            marks.append([at, 3 if luma else 0])
    if not reads_value(spec, state_of(spec, len(spec["steps"]))):
        return set()
    assert "nrg_at" not in spec, "a spec with energy changes of its own would need them merged with the type changes"
    got = CD.boundaries(dict(spec, depth=spec["depth"] or 1, nrg_at=marks), K, group)
    sized = {x for x in got if re.search(r":b\d+$", x) and not x.startswith("rows:")}
    assert all(x.split(":")[0] in WIDE_TAGS for x in sized), "coldepth_cases.boundaries has a pixel-size label this file does not know"
    if spec["depth"] != 0:
        return got
    out = got - sized
    if spec["ch"] > 4:
        out |= {"%s:b%d" % (x.split(":")[0], spec["ch"]) for x in sized}
    return out


# ---- seeded cases of the value-plane identity ---------------------------------------------------------------------------------
IDENTITY_LAYOUTS = [
    (0, 5, []), (2, 5, []), (1, 4, [CMYK]), (3, 3, [CMY]), (2, 6, []), (0, 7, [{"alpha": 5}, {"black": 2}]),
    (2, 4, [{"alpha": 1}]), (1, 9, [{"black": 8}]), (0, 4, [CMYK]), (0, 3, [CMY]), (3, 5, [{"black": 4}]), (1, 6, [{"alpha": 0}]),
]


def identity_case(seed, nrg, mid=False):
    """an input of a typed layout, its target size and options (coldepth_cases.lift_case's geometry), and the TypeState"""
    depth, ch, type_ops = IDENTITY_LAYOUTS[(seed + nrg) % len(IDENTITY_LAYOUTS)]
    rng = np.random.default_rng(90000 + 100 * nrg + seed + (10 ** 6 if mid else 0))
    base, nw, nh, kw, enlarge = CD.lift_case(seed, nrg, mid)
    h, w = base.shape[:2]
    img = CD.to_depth(rng, CD.base_image(rng, w, h, ch), depth, edge=(seed % 3 == 0))
    st = TypeState(ch)
    for op in type_ops:
        assert st.apply(op) == 1
    return img, depth, type_ops, st, nw, nh, kw, enlarge
