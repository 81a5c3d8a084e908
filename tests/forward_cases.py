"""Forward-energy seam maps (include_ext/lqr_forward.h): THE SPECIFICATION, as a numpy model, and the cases the engine is held to it on.

There is no liblqr counterpart.  The rule, in the frame of the carving direction (lines of length L, x along a line, y across the H
lines; I = (float) of the double the carver's energy function reads, P = bias / L in float, 0 without a bias); for seam k = 1 .. depth on
the current frame of width wc = L - k + 1:

    l = I(max(x-1,0), y)    r = I(min(x+1,wc-1), y)    u = I(x, y-1)
    CU = |r - l|     CL = CU + |u - l|     CR = CU + |u - r|
    M(x,0) = P(x,0) + CU
    M(x,y) = P(x,y) + min(M(x,y-1) + CU, M(x-1,y-1) + CL, M(x+1,y-1) + CR)         (parents outside the frame do not exist)

every operation a float32 operation rounded on its own, in the order written; ties up, then left, then right (strict <); the seam ends at
the smallest x that attains the minimum of M(., H-1) and is walked up through the stored choices; its pixels get level k at their
ORIGINAL positions and leave I and P (the part to the right moves one place left).  The map is width x height int32 in IMAGE
orientation, as lqr_vmap_dump lays one out.  The engine equals this bit for bit (tests/test_forward_gpu.py); what the rule itself is
worth -- the first seam is a cheapest one, and the one the tie rule names -- tests/test_forward_model.py checks by enumeration.
"""
import json
import os
import re

import numpy as np

import coldepth_cases as CD
import imgtype_cases as IT

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the model ----------------------------------------------------------------------------------------------------------------
def sweep(I, P):
    """the DP over one frame (H x wc float32 each): (M of the last row, the choices H x wc int8 -- -1 left, 0 up, 1 right)"""
    H, wc = I.shape
    idx = np.arange(wc)
    li, ri = np.maximum(idx - 1, 0), np.minimum(idx + 1, wc - 1)
    choice = np.zeros((H, wc), np.int8)
    M = None
    with np.errstate(all="ignore"):
        for y in range(H):
            l, r = I[y, li], I[y, ri]
            cu = np.abs(r - l)
            if y == 0:
                M = P[0] + cu
                continue
            u = I[y - 1]
            cl, cr = cu + np.abs(u - l), cu + np.abs(u - r)
            best = M + cu
            d = np.zeros(wc, np.int8)
            if wc > 1:
                left = M[:-1] + cl[1:]                      # the parent x - 1 of pixels 1 .. wc - 1
                take = left < best[1:]
                best[1:][take] = left[take]
                d[1:][take] = -1
                right = M[1:] + cr[:-1]                     # the parent x + 1 of pixels 0 .. wc - 2
                take = right < best[:-1]
                best[:-1][take] = right[take]
                d[:-1][take] = 1
            M = P[y] + best
            choice[y] = d
    assert M.dtype == F
    return M, choice


def pick(M):
    """the smallest x that attains the least M; values that compare with nothing are never taken, a row of them ends at 0"""
    ok = ~np.isnan(M)
    if not ok.any():
        return 0
    return int(np.flatnonzero(ok & (M == M[ok].min()))[0])


def seam_of(I, P):
    """the seam of one frame: its column on every line"""
    H, wc = I.shape
    M, choice = sweep(I, P)
    xs = np.zeros(H, np.int64)
    xs[H - 1] = pick(M)
    for y in range(H - 1, 0, -1):
        xs[y - 1] = xs[y] + choice[y, xs[y]]
    return xs


def levels(I, P, depth):
    """H x L int32: the levels of `depth` seams found one after the other on I (H x L float32), bias term P (H x L float32)"""
    I, P = np.ascontiguousarray(I, F), np.ascontiguousarray(P, F)
    H, L = I.shape
    assert 1 <= depth < L
    out = np.zeros((H, L), np.int32)
    pos = np.tile(np.arange(L), (H, 1))
    rows = np.arange(H)
    for k in range(1, depth + 1):
        xs = seam_of(I, P)
        out[rows, pos[rows, xs]] = k
        keep = np.ones(I.shape, bool)
        keep[rows, xs] = False
        wc = I.shape[1] - 1
        I, P, pos = I[keep].reshape(H, wc), P[keep].reshape(H, wc), pos[keep].reshape(H, wc)
    return out


def forward_map(I_img, bias_img, depth, orientation):
    """the map of an image whose energy reads I_img (h x w float32, image orientation) under the bias plane bias_img (h x w float32 or
    None): the dict lqr_vmap_dump's binding returns"""
    I_img = np.asarray(I_img, F)
    L = I_img.shape[0] if orientation else I_img.shape[1]
    with np.errstate(all="ignore"):
        P_img = np.zeros(I_img.shape, F) if bias_img is None else np.asarray(bias_img, F) / F(L)
    fr = (lambda a: a.T) if orientation else (lambda a: a)
    lv = levels(fr(I_img), fr(P_img), depth)
    return dict(data=np.ascontiguousarray(fr(lv)), depth=int(depth), orientation=int(orientation))


def intensity(img, depth, st, luma):
    """h x w float32: what the energy of a carver of type state `st` reads from img, rounded to float"""
    with np.errstate(all="ignore"):
        return IT.model_value(img, depth, st, luma).astype(F)


def valid_levels(lv, depth):
    """every level 1 .. depth once in every line, nothing else but 0"""
    want = np.arange(1, depth + 1)
    return lv.min() >= 0 and lv.max() <= depth and all(np.array_equal(np.sort(line[line > 0]), want) for line in lv)


# ---- the kernels' own constants (csrc/lqr_common.h), from which the cases' shapes are derived ---------------------------------
def kernel_constants():
    src = open(os.path.join(ROOT, "gimp-lqr-plugin_amd", "csrc", "lqr_common.h")).read()
    K = {}
    for name in ("FWD_THREADS", "FWD_MAX_PXT", "FWD_WALK_ROWS", "FWD_REMOVE_THREADS", "FWD_REMOVE_PX"):
        (K[name],) = {int(v) for v in re.findall(r"^#define\s+%s\s+(\d+)" % name, src, re.M)}
    K["LDS_ATTR_BYTES"] = 64 * 1024             # lds_needs_attr (csrc/lqr_plan.h): dynamic LDS past it needs hipFuncSetAttribute
    host = open(os.path.join(ROOT, "gimp-lqr-plugin_amd", "host", "lqr_carver.c")).read()
    (K["FWD_SLICE_SEAMS"],) = {int(v) for v in re.findall(r"^#define\s+FWD_SLICE_SEAMS\s+(\d+)", host, re.M)}
    return K


def line_shape(spec):
    """(L, H) of a spec: the line length and the number of lines in the carving direction"""
    return (spec["h"], spec["w"]) if spec["o"] else (spec["w"], spec["h"])


def boundaries(spec, K):
    """which paths of the kernels a case takes: the sweep's form (pixels per thread), the LDS attribute, walk blocks, removal rounds,
    slices of the host's loop"""
    L, H = line_shape(spec)
    out = set()
    pxt = 1
    while L > K["FWD_THREADS"] * pxt:
        pxt *= 2
    assert pxt <= K["FWD_MAX_PXT"]
    out.add("pxt%d" % pxt)
    if L == K["FWD_THREADS"] * pxt or L == K["FWD_THREADS"] * pxt // 2 + 1:
        out.add("pxt%d_edge" % pxt)
    if 2 * L * 4 > K["LDS_ATTR_BYTES"]:
        out.add("lds_attr")
    if L == K["FWD_THREADS"] * K["FWD_MAX_PXT"]:
        out.add("lds_max")
    blocks = -(-(H - 1) // K["FWD_WALK_ROWS"])
    out.add("walk_blocks_%s" % ("0" if blocks == 0 else "1" if blocks == 1 else "many"))
    if H > 1 and (H - 1) % K["FWD_WALK_ROWS"] == 0:
        out.add("walk_block_full")
    if H > 1 and (H - 1) % K["FWD_WALK_ROWS"] == 1:
        out.add("walk_block_of_one_row")
    if L - 1 > K["FWD_REMOVE_THREADS"] * K["FWD_REMOVE_PX"]:
        out.add("remove_rounds_many")
    if spec["d"] > K["FWD_SLICE_SEAMS"]:
        out.add("slices_many")
    if spec["d"] == L - 1:
        out.add("depth_max")
    if spec["d"] == 1:
        out.add("depth_1")
    return out


# ---- inputs -------------------------------------------------------------------------------------------------------------------
LEVELS4 = {0: (0, 85, 170, 255), 1: (0, 21845, 43690, 65535), 2: (0.0, 0.25, 0.5, 1.0), 3: (0.0, 0.25, 0.5, 1.0)}


def make_image(spec):
    """content "grey4": four grey levels, every channel of a pixel alike (the ties decide); "flat": all equal; "float": structure and
    noise (coldepth_cases)"""
    rng = np.random.default_rng(spec["seed"])
    w, h, ch, depth = spec["w"], spec["h"], spec["ch"], spec["depth"]
    dt = CD.DTYPES[depth]
    if spec["content"] == "float":
        return CD.to_depth(rng, CD.base_image(rng, w, h, ch), depth)
    lv = np.array(LEVELS4[depth], dt)
    pick4 = rng.integers(0, 4, (h, w)) if spec["content"] == "grey4" else np.full((h, w), 2)
    return np.ascontiguousarray(np.repeat(lv[pick4][:, :, None], ch, axis=2))


def make_bias(spec):
    """the float64 mask handed to lqr_carver_bias_add with factor spec["bias"] (None: no bias)"""
    if not spec.get("bias"):
        return None
    rng = np.random.default_rng([spec["seed"], 5])
    return np.ascontiguousarray(rng.integers(0, 4, (spec["h"], spec["w"])).astype(np.float64) / 4.0)


def type_state(spec):
    st = IT.TypeState(spec["ch"])
    if spec.get("type") is not None:
        assert st.apply(spec["type"]) == 1
    return st


def is_luma(spec):
    return 3 <= spec.get("nrg", 2) <= 5


# ---- the cases ----------------------------------------------------------------------------------------------------------------
def cases():
    """(name, spec).  w, h: the image; o: the map's orientation; d: its depth; ch, depth (LqrColDepth), type, nrg: the pixels and what
    reads them; content; bias: the factor (None: none); pre: None, "transposed" (the carver lies the other way beforehand) or
    "notflat" (it was resized beforehand); init: lqr_carver_init has seen the carver"""
    out = []

    def add(name, w, h, o, d, **more):
        spec = dict(seed=31000 + len(out), w=w, h=h, o=o, d=d, ch=3, depth=0, type=None, nrg=2, content="grey4", bias=None, pre=None, init=False)
        spec.update(more)
        out.append((name, json.loads(json.dumps(spec))))

    # line lengths across the sweep's forms (threads x pixels per thread) and the LDS attribute, few lines
    add("L2", 2, 5, 0, 1)
    add("L3", 3, 4, 0, 2)
    add("L63", 63, 8, 0, 62)
    add("L64", 64, 7, 0, 1)
    add("L65_v", 6, 65, 1, 64, ch=1)
    add("L1023", 1023, 5, 0, 3)
    add("L1024", 1024, 3, 0, 2, content="float")
    add("L1025", 1025, 4, 0, 18, ch=1)
    add("L2049_v", 3, 2049, 1, 2, ch=1)
    add("L4097", 4097, 3, 0, 2, ch=1)
    add("L8193", 8193, 2, 0, 2, ch=1)
    add("L8193_float_v", 2, 8193, 1, 1, ch=1, content="float")
    # numbers of lines across the walk's row block, short lines
    add("H1", 40, 1, 0, 5)
    add("H2", 33, 2, 0, 32)
    for H in (63, 64, 65, 66, 193):
        add("H%d" % H, 17 + H % 7, H, 0, 3, ch=1)
    add("H65_v", 65, 23, 1, 22, ch=1)
    add("H193_float", 70, 193, 0, 2, content="float")
    # pixel types
    add("grey_8i", 45, 12, 0, 9, ch=1)
    add("greya_8i", 45, 12, 1, 5, ch=2, content="float")
    add("rgb_8i_float", 70, 21, 0, 20, content="float")
    add("rgba_8i", 37, 14, 0, 6, ch=4, content="float")
    add("rgb_16i", 41, 9, 0, 7, depth=1, content="float")
    add("rgba_32f", 41, 9, 1, 4, ch=4, depth=2, content="float")
    add("grey_64f", 30, 11, 0, 8, ch=1, depth=3, content="float")
    add("cmyk_8i", 36, 10, 0, 6, ch=4, type=IT.CMYK, content="float")
    add("cmyk_32f_grey4", 36, 10, 1, 3, ch=4, type=IT.CMYK, depth=2)
    add("luma_rgb", 44, 13, 0, 8, nrg=5, content="float")
    add("luma_rgba_16i", 29, 13, 1, 6, nrg=3, ch=4, depth=1, content="float")
    # all-equal images: the tie rule alone
    add("flat_h", 19, 6, 0, 18, content="flat")
    add("flat_v", 7, 12, 1, 4, content="flat", ch=4)
    # bias, positive and negative
    add("bias_pos", 40, 15, 0, 9, bias=700, content="grey4")
    add("bias_neg_v", 40, 15, 1, 7, bias=-900, content="float")
    add("bias_neg_init", 52, 9, 0, 11, bias=-300, init=True)
    # the carver's state beforehand
    add("pre_transposed", 38, 16, 0, 7, pre="transposed", init=True)
    add("pre_transposed_v", 38, 16, 1, 7, pre="transposed", init=True, content="float")
    add("pre_notflat", 38, 16, 0, 6, pre="notflat", init=True, content="float")
    add("pre_notflat_v", 38, 16, 1, 6, pre="notflat", init=True)
    add("init_rgb", 47, 10, 0, 12, init=True, content="float")
    # (added last, so that the cases above keep their seeds) the last length of the 4-pixel form, and the widest line there is: the
    # launch with the most dynamic LDS, 2 x 16384 floats
    add("L4096", 4096, 2, 0, 2, ch=1)
    add("L16384", 16384, 2, 0, 1, ch=1)
    add("L16384_float_v", 2, 16384, 1, 2, ch=1, content="float")
    return out
