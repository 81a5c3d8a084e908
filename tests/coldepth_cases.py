"""The colour-depth cases (lqr_carver_new_ext): inputs made from a spec, and one driver that runs a case through any library
whose carver class has binding.Carver's colour-depth methods -- the genuine liblqr (scripts/ref_engine, which records
tests/golden/coldepth/) and the HIP engine (tests/test_coldepth_gpu.py, which reproduces the records).

A spec is a small dict: seed, w, h, ch, depth (LqrColDepth), nrg, steps [(w, h) | "flatten"], and optionally res_order,
switch, enl_step, delta, rigidity, bias, rigmask, dump_vmaps, preserve, edge, aux_depth.
"""
import json

import numpy as np

DTYPES = {0: np.uint8, 1: np.uint16, 2: np.float32, 3: np.float64}
DEPTH_NAMES = {0: "8i", 1: "16i", 2: "32f", 3: "64f"}


def base_image(rng, w, h, ch):
    """8-bit content with structure (gradients, blobs, noise): seams that are not all ties"""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.zeros((h, w, ch), np.float64)
    for k in range(ch):
        fx, fy, ph = rng.uniform(0.05, 0.4), rng.uniform(0.05, 0.4), rng.uniform(0, 6.3)
        img[:, :, k] = 127 + 90 * np.sin(fx * xx + ph) * np.cos(fy * yy) + rng.normal(0, 25, (h, w))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def to_depth(rng, v8, depth, edge=False):
    """an image of `depth` from 8-bit content; edge: the extremes of the depth (0 / 65535; values outside [0, 1], negative)"""
    if depth == 0:
        return v8.copy()
    if depth == 1:
        out = v8.astype(np.uint16) * 257 + rng.integers(0, 257, v8.shape).astype(np.uint16) * (v8 < 255)
        if edge:
            m = rng.random(v8.shape)
            out[m < 0.15] = 0
            out[m > 0.85] = 65535
        return out
    f = v8.astype(np.float64) / 255.0 + rng.normal(0, 1e-3, v8.shape)
    if edge:
        f = f * 2.5 - 0.75                      # [-0.75, 1.75]: HDR and negative values
        m = rng.random(v8.shape)
        f[m < 0.05] = -3.0
        f[m > 0.95] = 7.5
    return f.astype(DTYPES[depth])


def mask_image(rng, w, h, ch):
    m = np.zeros((h, w, ch), np.uint8)
    x0, y0 = rng.integers(0, w // 2), rng.integers(0, h // 2)
    m[y0:y0 + h // 2, x0:x0 + w // 3] = rng.integers(128, 256, ch)
    return m


def make_input(spec):
    rng = np.random.default_rng(spec["seed"])
    v8 = base_image(rng, spec["w"], spec["h"], spec["ch"])
    img = to_depth(rng, v8, spec["depth"], spec.get("edge", False))
    extra = {}
    if spec.get("bias"):
        extra["bias"] = mask_image(rng, spec["w"], spec["h"], 2)
    if spec.get("rigmask"):
        extra["rigmask"] = mask_image(rng, spec["w"], spec["h"], 1)
    if spec.get("aux_depth") is not None:
        extra["aux"] = to_depth(rng, base_image(rng, spec["w"], spec["h"], spec.get("aux_ch", 3)), spec["aux_depth"])
    return img, extra


def run(api, cls, spec, img=None, extra=None, partial=False):
    """drive one case; returns a dict of arrays and JSON-able records.  partial: before every resize a lqr_carver_scan_ext loop
    is given up near the end of the first line, and the scan after it starts from wherever the cursor is: a resize starts the
    read-out over (liblqr resets its cursor), so the record is that of the plain run"""
    if img is None:
        img, extra = make_input(spec)
    c = cls.from_ext(api, img, spec["depth"], delta_x=spec.get("delta", 1), rigidity=spec.get("rigidity", 0.0),
                     preserve=spec.get("preserve", False))
    before = c.input_bytes() if spec.get("preserve") else None
    if "bias" in extra:
        assert c.bias_add(extra["bias"], spec.get("bias_factor", 2000)) == 1
    if "rigmask" in extra:
        assert c.rigmask_add(extra["rigmask"]) == 1
    aux = c.attach_ext(extra["aux"], spec["aux_depth"]) if "aux" in extra else None
    c.configure(nrg_func=spec["nrg"], res_order=spec.get("res_order", 0), switch_freq=spec.get("switch", 2),
                enl_step=spec.get("enl_step", 1.5), dump_vmaps=spec.get("dump_vmaps", False), progress=True)
    out = {}
    rec = {"rets": [], "getters": [], "lines": [], "scan_rets": []}
    for i, st in enumerate(spec["steps"]):
        cont = partial and st != "flatten"
        if cont:
            c.scan_partial()
        ret = c.flatten() if st == "flatten" else c.resize(st[0], st[1])
        rec["rets"].append(ret)
        if ret != 1:
            break
        im, order = c.scan_ext(reset=not cont)
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


def cases():
    """the covering set: every depth x channels x energy appears; the options are spread over the depths"""
    out = []
    n = 0

    def add(name, **spec):
        nonlocal n
        spec.setdefault("seed", 1000 + n)
        n += 1
        out.append((name, spec))

    shapes = [(48, 32), (40, 28), (56, 36), (36, 44)]
    # depth x channels x energy: 4 x 4 x 7 = 112 combinations, covered by 28 cases (each energy once per depth and channel count,
    # rotating) with the resize kinds spread over them
    for depth in (1, 2, 3, 0):
        for ch in (1, 2, 3, 4):
            for j in range(7 if depth else 2):
                nrg = (j + ch) % 7 if depth else (j * 3 + ch) % 7
                if depth and j not in (ch - 1, ch + 2) and not (ch == 4 and j == 6):
                    continue
                w, h = shapes[(ch + j) % 4]
                kind = (depth + ch + j) % 4
                steps = [[(w - 9, h)], [(w + 7, h)], [(w - 6, h - 5)], [(w + 5, h - 4)]][kind]
                add("d%s_c%d_e%d" % (DEPTH_NAMES[depth], ch, nrg), w=w, h=h, ch=ch, depth=depth, nrg=nrg, steps=steps,
                    res_order=(ch + j) % 2, edge=(j % 2 == 1))
    # every energy at every deep depth on RGBA (the most common float layout)
    for depth in (1, 2, 3):
        for nrg in range(7):
            add("all_%s_e%d" % (DEPTH_NAMES[depth], nrg), w=44, h=30, ch=4, depth=depth, nrg=nrg, steps=[(36, 26)], res_order=nrg % 2)
    for depth in (1, 2, 3):
        d = DEPTH_NAMES[depth]
        add("enl_multistep_%s" % d, w=40, h=28, ch=3, depth=depth, nrg=2, steps=[(71, 28)], enl_step=1.3)
        add("enl_vert_%s" % d, w=40, h=28, ch=4, depth=depth, nrg=0, steps=[(46, 41)], res_order=1)
        add("delta2_%s" % d, w=48, h=32, ch=3, depth=depth, nrg=2, steps=[(38, 28)], delta=2, rigidity=0.6)
        add("delta5_%s" % d, w=48, h=32, ch=1, depth=depth, nrg=1, steps=[(40, 32)], delta=5, rigidity=1.5)
        add("masks_%s" % d, w=48, h=32, ch=4, depth=depth, nrg=3, steps=[(38, 32)], bias=True, rigmask=True, rigidity=2.0)
        add("switch_dump_%s" % d, w=44, h=30, ch=3, depth=depth, nrg=5, steps=[(33, 30)], switch=7, dump_vmaps=True)
        add("preserve_%s" % d, w=40, h=30, ch=4, depth=depth, nrg=2, steps=[(31, 24)], preserve=True)
        add("nopreserve_%s" % d, w=40, h=30, ch=4, depth=depth, nrg=2, steps=[(31, 24)], preserve=False)
        add("edge_%s" % d, w=40, h=30, ch=4, depth=depth, nrg=0, steps=[(32, 27), (45, 27)], edge=True)
        add("interactive_%s" % d, w=48, h=32, ch=3, depth=depth, nrg=(depth * 2) % 6,
            steps=[(40, 32), (44, 30), "flatten", (36, 28), (50, 28), (48, 32)], dump_vmaps=True)
    add("aux_8i_root_32f", w=40, h=28, ch=3, depth=0, nrg=2, steps=[(32, 28), (44, 24)], aux_depth=2, aux_ch=4)
    add("aux_32f_root_16i", w=40, h=28, ch=4, depth=2, nrg=4, steps=[(33, 25)], aux_depth=1, aux_ch=3)
    add("aux_64f_root_8i", w=40, h=28, ch=1, depth=3, nrg=1, steps=[(46, 23)], aux_depth=0, aux_ch=4)
    add("aux_16i_root_64f", w=40, h=28, ch=2, depth=1, nrg=0, steps=[(34, 30)], aux_depth=3, aux_ch=2, preserve=True)
    # tests/c/float_replay.c: an ImageMagick-style caller -- library defaults (no configuration call), a preserved 32F RGBA buffer
    add("float_replay_32f", w=48, h=32, ch=4, depth=2, nrg=2, steps=[(37, 27)], switch=0, enl_step=2.0, preserve=True, edge=True)
    return out
