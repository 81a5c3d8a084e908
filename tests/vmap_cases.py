"""The seam-map loading cases (include/lqr_vmap.h: lqr_vmap_new, lqr_vmap_load, lqr_vmap_internal_dump): specs, the driver that runs
one through any library whose carver class has binding.Carver's methods -- the genuine liblqr (scripts/ref_engine/make_vmap_golden.py,
which records tests/golden/vmap/) and the HIP engine (tests/test_vmap_load_gpu.py, which reproduces the records) -- and a numpy model
of what a loaded map makes of an image at every size it covers, for maps that no carver produced.

A spec is a small JSON-able dict:
  seed, w, h, ch, depth (LqrColDepth), max_ch      the image, as in coldepth_cases / imgtype_cases
  map           where the map comes from:
                {"kind": "carve", "to": [w1, h1], "nrg": n}   an initialised carver of the same image is resized to w1 x h1 (one direction)
                                                              and its lqr_vmap_dump is the map; recorded in the vector as "map"
                {"kind": "perm", "d": depth, "o": orientation} every line of the carving direction holds the levels 1 .. depth at random
                                                              places (not connected seams); made from the seed alone
  aux           an attached carver of the same size (8-bit RGB); its image is recorded after every resize too
  ops           applied in order to a carver created WITHOUT lqr_carver_init and configured with enl_step 1.5; the return value and
                the getters after each are recorded:
                ["load"]            lqr_vmap_load of the map; after LQR_OK the carver's lqr_vmap_dump is recorded ("redump@i")
                ["resize", w, h]    lqr_carver_resize; after LQR_OK the image ("image@i", and "aux_image@i")
                ["init"]            lqr_carver_init (delta, rigidity of the spec)
                ["idump"]           lqr_vmap_internal_dump; the length of the carver's list and its last map ("idump@i") are recorded
                ["dump"]            lqr_vmap_dump ("dump@i", its depth and orientation)
"""
import json

import numpy as np

import coldepth_cases as CD

DTYPES = CD.DTYPES
MAX_W, MAX_H = 320, 48          # no vector is larger (the files stay small)
RULES_NOTE = ("levels v of a line, d = depth: at length - k the pixels with v == 0 or v > k are visible, in order; at length + k one pixel is "
              "inserted before every pixel with 1 <= v <= k, the channel-wise average of that pixel and its left neighbour (itself at the "
              "start of the line): integers floor((a + b) / 2), floats (a + b) * 0.5 in the type's own precision")


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def make_input(spec):
    rng = np.random.default_rng(spec["seed"])
    v8 = CD.base_image(rng, spec["w"], spec["h"], spec["ch"])
    img = CD.to_depth(rng, v8, spec["depth"])
    extra = {}
    if spec.get("aux"):
        extra["aux"] = CD.base_image(rng, spec["w"], spec["h"], 3)
    return img, extra


def perm_map(seed, w, h, d, o):
    """h x w int32 in image orientation: every line of orientation o (a row for 0, a column for 1) holds 1 .. d once, anywhere"""
    rng = np.random.default_rng([seed, 77, d, o])
    lines, length = (h, w) if o == 0 else (w, h)
    m = np.zeros((lines, length), np.int32)
    for i in range(lines):
        m[i, rng.permutation(length)[:d]] = np.arange(1, d + 1)
    return dict(data=np.ascontiguousarray(m if o == 0 else m.T), depth=d, orientation=o)


def make_map(api, cls, spec, img):
    """the map of a spec as the dict vmap_dump returns; a "carve" map needs a library that can carve (the generator records it)"""
    g = spec["map"]
    if g["kind"] == "perm":
        return perm_map(spec["seed"], spec["w"], spec["h"], g["d"], g["o"])
    prev = _raise_channels(api, spec)
    try:
        a = cls.from_ext(api, img, spec["depth"], delta_x=spec.get("delta", 1), rigidity=spec.get("rigidity", 0.0))
    finally:
        _restore_channels(api, prev)
    a.configure(nrg_func=g.get("nrg", 2), res_order=0, switch_freq=2, enl_step=2.0)
    assert a.resize(g["to"][0], g["to"][1]) == 1
    m = a.vmap_dump()
    a.destroy()
    return m


def _raise_channels(api, spec):
    if spec.get("max_ch") and hasattr(api, "lqrx_set_max_channels"):
        return api.lqrx_set_max_channels(spec["max_ch"])
    return None


def _restore_channels(api, prev):
    if prev is not None:
        api.lqrx_set_max_channels(prev)


# ---- the model ----------------------------------------------------------------------------------------------------------------
def average(a, b):
    """the pixel inflate creates between a (the left neighbour) and b, per channel, by the rule of the dtype"""
    if a.dtype.kind == "f":
        return ((a + b) * a.dtype.type(0.5)).astype(a.dtype)
    return ((a.astype(np.int64) + b.astype(np.int64)) // 2).astype(a.dtype)


def model_line(p, v, d, length1):
    """one line: pixels p (n x ch) with levels v under a map of depth d, at length1 in [n - d, n + d]"""
    n = len(p)
    k = length1 - n
    assert -d <= k <= d
    if k <= 0:
        return p[(v == 0) | (v > -k)]
    out = []
    for x in range(n):
        if 1 <= v[x] <= k:
            out.append(average(p[x - 1 if x else 0], p[x]))
        out.append(p[x])
    return np.stack(out)


def model(img, m, size):
    """the image (h x w x ch) under map m at `size` in the map's direction (a width for orientation 0, a height for 1)"""
    img = np.asarray(img)
    if img.ndim == 2:
        img = img[:, :, None]
    data, d = np.asarray(m["data"]), int(m["depth"])
    if m["orientation"]:
        return np.ascontiguousarray(np.swapaxes(model(np.swapaxes(img, 0, 1), dict(data=data.T, depth=d, orientation=0), size), 0, 1))
    return np.stack([model_line(img[y], data[y], d, size) for y in range(img.shape[0])])


def valid_map(m, w, h):
    """what include/lqr_vmap.h item 1 asks of a map for a w x h image"""
    data, d, o = np.asarray(m["data"]), int(m["depth"]), int(m["orientation"])
    if data.shape != (h, w) or o not in (0, 1) or not 0 < d < (h if o else w) or data.min() < 0 or data.max() > d:
        return False
    lines = data.T if o else data
    return all(np.array_equal(np.sort(line[line > 0]), np.arange(1, d + 1)) for line in lines)


# ---- the driver ---------------------------------------------------------------------------------------------------------------
def run(api, cls, spec, img=None, extra=None, vmap=None):
    """drive one case; returns a dict of arrays and a JSON record.  vmap: the map (a recorded one); by default made here"""
    if img is None:
        img, extra = make_input(spec)
    if vmap is None:
        vmap = make_map(api, cls, spec, img)
    prev = _raise_channels(api, spec)
    try:
        c = cls.from_ext(api, img, spec["depth"], init=False)
        aux = c.attach_ext(extra["aux"], 0) if "aux" in extra else None
    finally:
        _restore_channels(api, prev)
    c.configure(nrg_func=spec.get("nrg", 2), res_order=0, switch_freq=2, enl_step=1.5)
    out = {"map": np.ascontiguousarray(vmap["data"], dtype=np.int32)}
    rec = {"map_meta": [int(vmap["depth"]), int(vmap["orientation"])], "rets": [], "getters": [], "redump_meta": {}, "lists": {}}
    for i, op in enumerate(spec["ops"]):
        kind = op[0]
        if kind == "load":
            ret = c.vmap_load(vmap)
            if ret == 1:
                v = c.vmap_dump()
                out["redump@%d" % i] = v["data"]
                rec["redump_meta"][str(i)] = [int(v["depth"]), int(v["orientation"])]
        elif kind == "resize":
            ret = c.resize(op[1], op[2])
            if ret == 1:
                out["image@%d" % i] = c.scan_line_ext()[0]
                if aux is not None:
                    out["aux_image@%d" % i] = aux.scan_line_ext()[0]
        elif kind == "init":
            ret = c.init(spec.get("delta", 1), spec.get("rigidity", 0.0))
        elif kind == "dump":
            v = c.vmap_dump()
            ret = 1
            out["dump@%d" % i] = v["data"]
            rec["redump_meta"][str(i)] = [int(v["depth"]), int(v["orientation"])]
        elif kind == "idump":
            ret = c.vmap_internal_dump()
            maps = c.dumped_vmaps()
            rec["lists"][str(i)] = len(maps)
            if maps:
                out["idump@%d" % i] = maps[-1]["data"]
        else:
            raise ValueError(kind)
        rec["rets"].append(ret)
        g = c.getters()
        g["enl_step"] = float(g["enl_step"])
        rec["getters"].append(g)
    c.destroy()
    out["record"] = np.array(json.dumps(rec, sort_keys=True))
    return out


assert_same_record = CD.assert_same_record


def model_check(spec, img, out):
    """(images compared, keys that differ): the model applied to the recorded map against every recorded image of the ROOT carver while
    the carver shows the loaded map alone (up to a later ["init"], after which further seams are carved)"""
    m = dict(data=out["map"], depth=json.loads(str(out["record"]))["map_meta"][0], orientation=json.loads(str(out["record"]))["map_meta"][1])
    rec = json.loads(str(out["record"]))
    compared, differ, loaded = 0, [], False
    for i, op in enumerate(spec["ops"]):
        if op[0] == "load" and rec["rets"][i] == 1:
            loaded = True
        if op[0] == "init":
            break
        key = "image@%d" % i
        if op[0] != "resize" or not loaded or key not in out:
            continue
        want = model(img, m, op[2] if m["orientation"] else op[1])
        compared += 1
        if out[key].dtype != want.dtype or out[key].shape != want.shape or not np.array_equal(CD.bits(out[key]), CD.bits(want)):
            differ.append(key)
    return compared, differ


# ---- the cases ----------------------------------------------------------------------------------------------------------------
def _sizes(w, h, d, o, ks):
    return [["resize", w + k, h] if o == 0 else ["resize", w, h + k] for k in ks]


def cases():
    """what liblqr and the engine do alike (include/lqr_vmap.h, semantics); every image at most MAX_W x MAX_H"""
    out = []

    def add(name, w, h, gen, ops, **more):
        spec = dict(seed=12000 + len(out), w=w, h=h, ch=3, depth=0, nrg=2, delta=1, rigidity=0.0, map=gen, ops=ops)
        spec.update(more)
        out.append((name, json.loads(json.dumps(spec))))

    carve = lambda w1, h1, nrg=2: dict(kind="carve", to=[w1, h1], nrg=nrg)      # noqa: E731
    perm = lambda d, o: dict(kind="perm", d=d, o=o)                              # noqa: E731
    # the issue's example: 40 x 24, 10 seams; every size of the range, in any order and back; the list
    add("h_40x24_d10", 40, 24, carve(30, 24), [["load"]] + _sizes(40, 24, 10, 0, (-7, -10, 10, 0, 7, 4, -10)) + [["idump"], ["resize", 36, 24], ["idump"]])
    add("v_40x24_d8", 40, 24, carve(40, 16), [["load"]] + _sizes(40, 24, 8, 1, (-4, -8, 6, 0, 8)) + [["idump"]])
    # lqr_carver_init after a load, and the carver then refuses another map (a DEEPER resize after the init: finding_cases)
    add("init_then_load_refused", 40, 24, carve(30, 24), [["load"], ["resize", 33, 24], ["init"], ["resize", 36, 24], ["load"], ["resize", 30, 24]], rigidity=0.5)
    # depth 1, depth = length - 2, a single line
    add("depth_1", 33, 9, carve(32, 9), [["load"]] + _sizes(33, 9, 1, 0, (-1, 1, 0)))
    add("depth_len_minus_2", 12, 7, carve(2, 7), [["load"]] + _sizes(12, 7, 10, 0, (-10, -5, 10, 3)))
    add("one_row_64x1", 64, 1, carve(50, 1), [["load"]] + _sizes(64, 1, 14, 0, (-14, 14, -3)))
    add("tiny_2x3", 2, 3, perm(1, 0), [["load"]] + _sizes(2, 3, 1, 0, (-1, 1, 0)))
    # a load after a resize: back at the map's size (a carver that was resized since its last load is flattened first)
    add("load_after_resize", 40, 24, carve(30, 24), [["load"], ["resize", 33, 24], ["resize", 40, 24], ["load"], ["resize", 47, 24], ["resize", 40, 24], ["load"],
                                                      ["resize", 31, 24]])
    add("load_twice_v", 40, 24, perm(6, 1), [["load"], ["resize", 40, 20], ["resize", 40, 24], ["load"], ["resize", 40, 30]])
    # the attached carver follows
    add("attached_h", 40, 24, carve(30, 24), [["load"]] + _sizes(40, 24, 10, 0, (-6, 10, 0)), aux=True)
    add("attached_v", 37, 30, perm(9, 1), [["load"]] + _sizes(37, 30, 9, 1, (-9, 5)), aux=True)
    # other pixels: a deep carver, five channels, 16-bit grey, RGBA
    add("rgba_32f", 45, 20, carve(33, 20, 3), [["load"]] + _sizes(45, 20, 12, 0, (-12, 12, -5, 5)), ch=4, depth=2)
    add("grey_16i_v", 30, 40, carve(30, 29, 0), [["load"]] + _sizes(30, 40, 11, 1, (-11, 11, 3)), ch=1, depth=1)
    add("five_channels", 36, 18, carve(27, 18, 4), [["load"]] + _sizes(36, 18, 9, 0, (-9, 9, -2)), ch=5, max_ch=8)
    add("grey_64f", 28, 12, perm(5, 0), [["load"]] + _sizes(28, 12, 5, 0, (-5, 5)), ch=1, depth=3)
    # maps no carver made: the model's ground.  Past 256 columns (the rank carry of the inflate), both orientations
    add("perm_h_70x45", 70, 45, perm(20, 0), [["load"]] + _sizes(70, 45, 20, 0, (-20, -9, 20, 1)))
    add("perm_v_70x45", 70, 45, perm(17, 1), [["load"]] + _sizes(70, 45, 17, 1, (-17, 17, -1)))
    add("perm_h_300x37", 300, 37, perm(33, 0), [["load"]] + _sizes(300, 37, 33, 0, (-33, 33, 16)))
    add("perm_rgba_32f", 70, 45, perm(13, 0), [["load"]] + _sizes(70, 45, 13, 0, (-13, 13)), ch=4, depth=2)
    add("perm_five_channels_v", 70, 45, perm(11, 1), [["load"]] + _sizes(70, 45, 11, 1, (-11, 11)), ch=5, max_ch=8)
    add("carve_300x37_d33", 300, 37, carve(267, 37), [["load"]] + _sizes(300, 37, 33, 0, (-33, -16, 1, 33)))
    return out


def finding_cases():
    """what include/lqr_vmap.h does NOT follow, recorded all the same (MANIFEST "findings"): liblqr's returns are in the manifest, the
    engine's are asserted in tests/test_vmap_load_gpu.py
    * a resize beyond the loaded range, or in the other direction: liblqr fails part-way and refuses every later resize;
    * a second load onto a carver resized to another size: liblqr takes the map for the resized image (LQR_OK, garbage);
    * lqr_carver_init after a load and a DEEPER resize: liblqr returns LQR_OK and the depth grows, but its lqr_carver_init lays the
      carved frame out as the first columns of the inflated layout, not as the visible pixels, so the further seams are found on and
      written over the wrong pixels: the map it dumps afterwards holds levels twice and lacks others.  The engine carves the further
      seams on the visible frame (a warm start)"""
    out = []

    def add(name, ops, w=40, h=24, to=(30, 24), **more):
        spec = dict(seed=12900 + len(out), w=w, h=h, ch=3, depth=0, nrg=2, delta=1, rigidity=0.0, map=dict(kind="carve", to=list(to), nrg=2), ops=ops)
        spec.update(more)
        out.append((name, json.loads(json.dumps(spec))))

    add("beyond_range", [["load"], ["resize", 33, 24], ["resize", 51, 24], ["resize", 40, 24], ["resize", 33, 24]])
    add("below_range", [["load"], ["resize", 29, 24], ["resize", 35, 24]])
    add("other_direction", [["load"], ["resize", 35, 20], ["resize", 40, 24]])
    add("second_load_at_50", [["load"], ["resize", 50, 24], ["load"]])
    add("second_load_at_30", [["load"], ["resize", 30, 24], ["load"]])
    add("initialised", [["init"], ["load"]])
    add("init_after_load_h", [["load"], ["init"], ["resize", 25, 24], ["dump"], ["resize", 33, 24], ["load"]], rigidity=0.5)
    add("init_after_load_v", [["load"], ["init"], ["resize", 45, 28], ["dump"], ["resize", 45, 36], ["load"]], w=45, h=40, to=(45, 33))
    return out
