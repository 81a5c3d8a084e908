"""The colour-depth cases (lqr_carver_new_ext): inputs made from a spec, and one driver that runs a case through any library
whose carver class has binding.Carver's colour-depth methods -- the genuine liblqr (scripts/ref_engine, which records
tests/golden/coldepth/) and the HIP engine (tests/test_coldepth_gpu.py, which reproduces the records).

A spec is a small dict: seed, w, h, ch, depth (LqrColDepth), nrg, steps [(w, h) | "flatten"], and optionally res_order,
switch, enl_step, delta, rigidity, bias, rigmask, dump_vmaps, preserve, edge, aux_depth, nrg_at ([[i, nrg], ...]: the energy function
is changed to nrg before step i).

cases() are the small vectors of tests/golden/coldepth/ (every depth x channel count x energy x option); mid_cases() those of
tests/golden/coldepth_mid/, sized to cross the boundaries inside the deep kernels (more than one 256-column chunk, more than one
block of energy rows, sessions longer than the frozen lag, the wide delta_x instantiations): boundaries() names what a spec crosses.
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
    nrg_at = dict((int(i), int(n)) for i, n in spec.get("nrg_at", []))
    for i, st in enumerate(spec["steps"]):
        if i in nrg_at:
            assert c.set_energy(nrg_at[i]) == 1
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


# ---- seeded cases of the lift identities (8-bit v, 16I v * 257, 64F v / 255.0 carve the same seams) ---------------------------
def lift_case(seed, nrg, mid=False):
    """mid: 257 .. 600 columns, 63 .. 200 rows, 33 .. 150 seams (past the deep kernels' chunk, block and lag boundaries)"""
    rng = np.random.default_rng(70000 + 100 * nrg + seed + (10 ** 6 if mid else 0))
    ch = 1 + seed % 4
    w, h = (int(rng.integers(257, 601)), int(rng.integers(63, 201))) if mid else (int(rng.integers(20, 44)), int(rng.integers(16, 34)))
    img = base_image(rng, w, h, ch)
    enlarge = seed % 5 == 4
    # an enlargement is carved in one direction and one step only: a second pass would read the pixels the first one inserted,
    # which each depth averages with its own rounding
    if mid:
        k = int(rng.integers(33, 151))
        nw = w + min(k, w // 2 - 2) if enlarge else w - k
        nh = h if enlarge or seed % 3 else h - int(rng.integers(33, 56))
    else:
        nw = w + int(rng.integers(1, w // 2)) if enlarge else w - int(rng.integers(1, w // 3))
        nh = h if enlarge else h - int(rng.integers(0, h // 4))
    kw = dict(nrg_func=nrg, res_order=int(seed % 2), switch_freq=int(rng.integers(0, 4)), enl_step=1.5)
    return img, nw, nh, kw, enlarge


# ---- comparing a run with a recorded vector -----------------------------------------------------------------------------------
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8) if a.dtype.kind == "f" else a


def assert_same_record(got, z, what):
    want_keys = sorted(k for k in z.files if k not in ("img", "spec") and not k.startswith("in_"))
    assert sorted(got) == want_keys, what
    for k in want_keys:
        if k == "record":
            assert json.loads(str(got[k])) == json.loads(str(z[k])), "%s: %s" % (what, k)
        else:
            assert got[k].dtype == z[k].dtype and got[k].shape == z[k].shape, "%s: %s" % (what, k)
            assert np.array_equal(bits(got[k]), bits(z[k])), "%s: %s differs" % (what, k)


# ---- the mid-size vectors -----------------------------------------------------------------------------------------------------
FAMILY = {1: 8, 2: 5, 3: 5}             # same-shape inputs per depth, carved as one group in tests/test_coldepth_mid_gpu.py
FAMILY_SHAPE = dict(w=280, h=30, ch=1, nrg=2, steps=[(140, 30)])


def family_names(depth):
    return ["fam_%s_%d" % (DEPTH_NAMES[depth], i) for i in range(FAMILY[depth])]


def mid_cases():
    """beyond 256 / 512 columns, 62 / 124 rows, 32 / 128 seams, delta_x 3 .. 10 (tests/test_coldepth_abi.py asserts what is crossed).
    Wide cases are short and tall ones narrow: 16- to 32-byte pixels of noise-like floats do not compress"""
    out = []

    def add(name, **spec):
        spec.setdefault("seed", 7000 + len(out))
        out.append((name, spec))

    for depth in (1, 2, 3):
        d = DEPTH_NAMES[depth]
        ch2, ch3 = {1: (3, 4), 2: (4, 3), 3: (4, 3)}[depth]
        # shrink, change of read value on the non-flat carver (re-layout from the visible pixels), shrink on, flatten, enlarge:
        # every pass over the base layout at two and at three 256-column chunks.  38 seams, then 42: seam step 40 exists in the
        # second session only (the fault-recovery test aims its injection there, at a carver that is not flat)
        add("all2_%s" % d, w=340, h=12, ch=ch2, depth=depth, nrg=0, nrg_at=[[1, 3]], edge=True,
            steps=[(302, 12), (260, 12), "flatten", (300, 12)])
        add("all3_%s" % d, w=600, h=12, ch=ch3, depth=depth, nrg=4, nrg_at=[[1, 1]],
            steps=[(562, 12), (520, 12), "flatten", (570, 12)], dump_vmaps=True)
        # vertical first, both directions enlarged: the inflate pass of a transposed carver
        add("enlv_%s" % d, w=24, h=264, ch={1: 3, 2: 3, 3: 2}[depth], depth=depth, nrg=2, steps=[(30, 300)], res_order=1)
    add("enlv_32f_c4", w=24, h=264, ch=4, depth=2, nrg=0, steps=[(31, 299)], res_order=1, edge=True)
    # more than one and more than two blocks of energy rows, sessions past the lag of 32
    add("tall_16i_c3", w=90, h=140, ch=3, depth=1, nrg=1, steps=[(50, 140)])
    add("tall_32f_c1_both", w=130, h=132, ch=1, depth=2, nrg=5, steps=[(92, 96)], res_order=1)
    add("tall_64f_c1", w=86, h=130, ch=1, depth=3, nrg=6, steps=[(49, 130)], edge=True)
    # delta_x 3 .. 8 and 9 .. 10
    add("d3_16i_c1", w=276, h=64, ch=1, depth=1, nrg=2, steps=[(238, 64)], delta=3, rigidity=0.5)
    add("d9_16i_c3", w=270, h=64, ch=3, depth=1, nrg=1, steps=[(235, 64)], delta=9, rigidity=1.0)
    add("d7_32f_c2", w=270, h=66, ch=2, depth=2, nrg=6, steps=[(232, 66)], delta=7, bias=True)
    add("d9_32f_c1", w=266, h=70, ch=1, depth=2, nrg=0, steps=[(229, 70)], delta=9, rigidity=0.3, edge=True)
    add("d3_64f_c2", w=264, h=24, ch=2, depth=3, nrg=5, steps=[(226, 24)], delta=3)
    add("d10_64f_c1", w=280, h=70, ch=1, depth=3, nrg=3, steps=[(240, 70)], delta=10, rigidity=0.8)
    # wide and two blocks of rows at once; masks carried through a catch-up in mid-session
    add("wide_64f_c4", w=264, h=63, ch=4, depth=3, nrg=0, steps=[(224, 63)], edge=True)
    add("masks_32f_c3", w=290, h=68, ch=3, depth=2, nrg=3, steps=[(250, 68)], bias=True, rigmask=True, rigidity=2.0)
    add("enl_multistep_32f", w=264, h=20, ch=1, depth=2, nrg=2, steps=[(400, 20)], enl_step=1.3)
    add("inter_16i", w=300, h=36, ch=3, depth=1, nrg=0, steps=[(262, 36), (280, 32), "flatten", (240, 32), (330, 32)], dump_vmaps=True)
    add("aux_32f_root_64f", w=270, h=16, ch=1, depth=2, nrg=2, steps=[(230, 16)], aux_depth=3, aux_ch=2)
    add("preserve_16i", w=270, h=16, ch=4, depth=1, nrg=1, steps=[(305, 16)], preserve=True)
    # families of one geometry: 140 seams, past the lag of 128 that a group of five or more carvers has
    for depth in (1, 2, 3):
        for name in family_names(depth):
            add(name, depth=depth, **FAMILY_SHAPE)
    return out


PLANE_SEAMS = (40, 70)


def plane_cases():
    """energy, cumulative minimum and back pointers read out of the genuine engine's memory after the full build (energy) and after
    PLANE_SEAMS incremental seams (switch_freq 0): a brightness energy, a luma energy and delta_x 9 with rigidity, per deep depth.
    The input is made from the spec (its SHA-1 is recorded with the planes)"""
    out = []
    for depth in (1, 2, 3):
        d = DEPTH_NAMES[depth]
        out.append(("planes_%s_bright" % d, dict(seed=7500 + depth, w=258, h=63, ch=4, depth=depth, nrg=0, edge=True)))
        out.append(("planes_%s_luma" % d, dict(seed=7510 + depth, w=258, h=63, ch=3, depth=depth, nrg=3)))
        out.append(("planes_%s_d9" % d, dict(seed=7520 + depth, w=258, h=63, ch=1, depth=depth, nrg=2, delta=9, rigidity=0.7)))
    return out


# ---- what a spec crosses ------------------------------------------------------------------------------------------------------
def boundaries(spec, K, group=1):
    """the structural boundaries of the deep kernels that running `spec` crosses, as a set of labels; from the spec alone, by liblqr's
    own bookkeeping (resize order, enl_step, the cached map, flatten before a transpose).  K: EU_ROWS, EU_LOGB, FROZEN_LAG_MAX and
    NT (ascending [largest delta_x, samples] pairs of k_emap_update's instantiations) as the sources define them; group:
    carvers resized together (the frozen lag is FROZEN_LAG_MAX / 4 up to 4 carvers).

      shrink:cN enlarge:cN   a session whose carved frame spans N 256-column chunks (3 = three or more)
      relayout:cN            ... that lays the value plane out again from a base layout of N chunks that is not flat
      flatten:cN readout:cN  compaction of a base layout of N chunks
      catchup:cN             a session longer than the lag: frozen planes of N chunks compacted in mid-session, epoch > 0 after it
      rows:bN                N blocks of EU_ROWS energy rows;  ntS: the S-sample instantiation;  seams>L;  ragged: length % EU_LOGB != 0
      inflate:bB compact:bB transpose:bB   pixels of B > 4 bytes through those passes at more than 256 columns (rows, transposed)
    """
    lab = set()
    px = spec["ch"] * np.dtype(DTYPES[spec["depth"]]).itemsize
    deep = spec["depth"] != 0
    lag = K["FROZEN_LAG_MAX"] // 4 if group <= 4 else K["FROZEN_LAG_MAX"]
    nt = next(s for dmax, s in K["NT"] if spec.get("delta", 1) <= dmax)
    enl = np.float32(spec.get("enl_step", 1.5))
    s = dict(w0=spec["w"], h0=spec["h"], ws=spec["w"], hs=spec["h"], w=spec["w"], h=spec["h"], ml=1, tr=0, wk=False)
    luma = [spec["nrg"] in (3, 4, 5)]

    def chunks(n):
        return min(3, -(-n // 256))

    def wide(tag, n):
        if px > 4 and n > 256:
            lab.add("%s:b%d" % (tag, px))

    def dmax_of(start):
        return max(int((enl - np.float32(1)) * np.float32(start)) - 1, 1)

    def flat():
        return s["w"] == s["w0"] and s["ml"] == 1 and s["ws"] == s["w0"]

    def flatten():
        if not flat():
            lab.add("flatten:c%d" % chunks(s["w0"]))
            wide("compact", s["w0"])
        elif s["wk"]:
            return
        s.update(w0=s["w"], h0=s["h"], ws=s["w"], hs=s["h"], ml=1, wk=False)

    def transpose():
        if not flat():
            flatten()
        if s["w0"] % 32 and s["h0"] % 32:
            wide("transpose", max(s["w0"], s["h0"]))
        s.update(w0=s["h0"], h0=s["w0"])
        s.update(w=s["w0"], h=s["h0"], ws=s["w0"], hs=s["h0"], ml=1, tr=s["tr"] ^ 1, wk=False)

    def session(depth, enlarge):
        if depth <= s["ml"]:
            return
        n, wc0 = depth - s["ml"], s["ws"] - s["ml"] + 1
        if not s["wk"]:
            if s["ml"] != 1 or s["w0"] != s["ws"]:
                lab.add("relayout:c%d" % chunks(s["w0"]))
            s["wk"] = True
        lab.add("%s:c%d" % ("enlarge" if enlarge else "shrink", chunks(wc0)))
        lab.add("rows:b%d" % min(3, -(-s["h"] // K["EU_ROWS"])))
        lab.add("nt%d" % nt)
        if n > lag:
            lab.add("seams>%d" % lag)
            lab.add("catchup:c%d" % chunks(wc0))
        if n % K["EU_LOGB"]:
            lab.add("ragged")
        wide("inflate", s["w0"])
        s["w0"] += n
        s["ml"] = depth

    def resize_dir(w1, want):
        start, cur = (s["ws"], s["w"]) if s["tr"] == want else (s["hs"], s["h"])
        delta, gamma, dmax = w1 - start, w1 - cur, dmax_of(start)
        enlarge = delta > 0
        if delta < 0:
            delta = dmax = -delta
        while gamma:
            d0 = min(delta, dmax)
            delta -= d0
            if s["tr"] != want:
                transpose()
            new_w = min(w1, s["ws"] + dmax)
            gamma = w1 - new_w
            session(d0 + 1, enlarge)
            s["w"] = new_w
            if new_w < w1:
                flatten()
                dmax = dmax_of(s["ws"])

    for i, st in enumerate(spec["steps"]):
        for at, nrg in spec.get("nrg_at", []):
            if at == i and deep and (nrg in (3, 4, 5)) != luma[0]:
                luma[0] = not luma[0]
                s["wk"] = False
        if st == "flatten":
            flatten()
        else:
            for want in ((0, 1), (1, 0))[spec.get("res_order", 0)]:
                resize_dir(st[1] if want else st[0], want)
        if not flat():                                  # the driver reads every image out
            lab.add("readout:c%d" % chunks(s["w0"]))
            wide("compact", s["w0"])
    return lab if deep else set()
