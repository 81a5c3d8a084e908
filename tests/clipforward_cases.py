"""Forward-energy seams for a clip (include_ext/lqr_clipforward.h): THE SPECIFICATION, as a numpy model, and the cases the engine is held
to it on.

There is no liblqr counterpart.  In the frame of the carving direction (lines of length L, x along a line, y across the H lines), for the
frames t = 0 .. n-1 of a clip: I_t = forward_cases.intensity (the I of lqr_forward.h), P_t = bias_t / L in float, 0 without a bias.
Planes made once, which travel with their pixels:

    T = max_{t>=1} |I_t - I_{t-1}|   (0 for n = 1)        Pm = max_t P_t        Q = fl(Pm + fl(temporal * T))

For seam k = 1 .. depth on the current frames of width wc = L - k + 1, with l_t = I_t(max(x-1,0), y), r_t = I_t(min(x+1,wc-1), y),
u_t = I_t(x, y-1):

    CU = max_t |r_t - l_t|     CL = max_t fl(|r_t - l_t| + |u_t - l_t|)     CR = max_t fl(|r_t - l_t| + |u_t - r_t|)
    M(x,0) = Q + CU
    M(x,y) = Q + min(M(x,y-1) + CU, M(x-1,y-1) + CL, M(x+1,y-1) + CR)            (parents outside the frame do not exist)

every operation a float32 operation rounded on its own, in the order written; ties up, then left, then right (strict <); the seam ends at
the smallest x that attains the minimum of M(., H-1) (forward_cases.pick) and is walked up through the stored choices; its pixels get level
k at their ORIGINAL positions and leave every frame, Q and the position plane.  levels() below forms the costs of the whole frames again for
every seam: that is the rule.  levels_two_columns() is how the engine does it -- the I planes never compacted, the pixels of the current
frame found through the position plane, and after a seam only the two columns of each line whose neighbours changed formed again --
and tests/test_clipforward_model.py holds the two equal.
"""
import json
import os
import re

import numpy as np

import forward_cases as FC
import imgtype_cases as IT

F = np.float32
ROOT = FC.ROOT
GROUP = 16          # frames per launch of k_clip_fold (csrc/lqr_common.h CLIPFWD_GROUP)


# ---- the model ----------------------------------------------------------------------------------------------------------------
def costs(Is):
    """(CU, CL, CR), H x wc float32 each, of the current frames Is (n x H x wc float32); line 0 has no CL and CR: 0"""
    n, H, wc = Is.shape
    idx = np.arange(wc)
    li, ri = np.maximum(idx - 1, 0), np.minimum(idx + 1, wc - 1)
    with np.errstate(all="ignore"):
        l, r = Is[:, :, li], Is[:, :, ri]
        a = np.abs(r - l)
        CU = a.max(axis=0)
        CL, CR = np.zeros((H, wc), F), np.zeros((H, wc), F)
        if H > 1:
            u = Is[:, :-1, :]
            CL[1:] = (a[:, 1:] + np.abs(u - l[:, 1:])).max(axis=0)
            CR[1:] = (a[:, 1:] + np.abs(u - r[:, 1:])).max(axis=0)
    assert CU.dtype == F and CL.dtype == F and CR.dtype == F
    return CU, CL, CR


def temporal_plane(Is):
    """T: H x L float32"""
    with np.errstate(all="ignore"):
        return np.abs(Is[1:] - Is[:-1]).max(axis=0) if Is.shape[0] > 1 else np.zeros(Is.shape[1:], F)


def q_plane(Is, Ps, temporal):
    """Q: H x L float32 from the frames' I and P (n x H x L float32 each)"""
    with np.errstate(all="ignore"):
        Q = Ps.max(axis=0) + F(temporal) * temporal_plane(Is)
    assert Q.dtype == F
    return Q


def sweep(CU, CL, CR, Q):
    """the DP over given cost planes (H x wc float32 each): (M of the last row, the choices H x wc int8 -- -1 left, 0 up, 1 right)"""
    H, wc = CU.shape
    choice = np.zeros((H, wc), np.int8)
    with np.errstate(all="ignore"):
        M = Q[0] + CU[0]
        for y in range(1, H):
            best = M + CU[y]
            d = np.zeros(wc, np.int8)
            if wc > 1:
                left = M[:-1] + CL[y, 1:]                   # the parent x - 1 of pixels 1 .. wc - 1
                take = left < best[1:]
                best[1:][take] = left[take]
                d[1:][take] = -1
                right = M[1:] + CR[y, :-1]                  # the parent x + 1 of pixels 0 .. wc - 2
                take = right < best[:-1]
                best[:-1][take] = right[take]
                d[:-1][take] = 1
            M = Q[y] + best
            choice[y] = d
    assert M.dtype == F
    return M, choice


def seam_of(CU, CL, CR, Q):
    """the seam under given costs: its column on every line"""
    H = CU.shape[0]
    M, choice = sweep(CU, CL, CR, Q)
    xs = np.zeros(H, np.int64)
    xs[H - 1] = FC.pick(M)
    for y in range(H - 1, 0, -1):
        xs[y - 1] = xs[y] + choice[y, xs[y]]
    return xs


def levels(Is, Ps, depth, temporal):
    """H x L int32: the levels of `depth` seams of the clip whose frames read Is under the bias terms Ps (n x H x L float32 each)"""
    Is, Ps = np.ascontiguousarray(Is, F), np.ascontiguousarray(Ps, F)
    n, H, L = Is.shape
    assert 1 <= depth < L and Ps.shape == Is.shape
    Q = q_plane(Is, Ps, temporal)
    out = np.zeros((H, L), np.int32)
    pos = np.tile(np.arange(L), (H, 1))
    rows = np.arange(H)
    for k in range(1, depth + 1):
        xs = seam_of(*costs(Is), Q)
        out[rows, pos[rows, xs]] = k
        keep = np.ones((H, Is.shape[2]), bool)
        keep[rows, xs] = False
        wc = Is.shape[2] - 1
        Is = Is[:, keep].reshape(n, H, wc)
        Q, pos = Q[keep].reshape(H, wc), pos[keep].reshape(H, wc)
    return out


def levels_two_columns(Is, Ps, depth, temporal):
    """the same levels the way the engine finds them: the I planes stay as they are, a pixel of the current frame is found through the
    position plane, and after a seam that left line y at column s only the new columns s - 1 and s of that line get new costs"""
    Is, Ps = np.ascontiguousarray(Is, F), np.ascontiguousarray(Ps, F)
    n, H, L = Is.shape
    assert 1 <= depth < L
    Q = q_plane(Is, Ps, temporal)
    CU, CL, CR = costs(Is)
    out = np.zeros((H, L), np.int32)
    pos = np.tile(np.arange(L), (H, 1))
    rows = np.arange(H)
    for k in range(1, depth + 1):
        xs = seam_of(CU, CL, CR, Q)
        out[rows, pos[rows, xs]] = k
        keep = np.ones(CU.shape, bool)
        keep[rows, xs] = False
        wn = CU.shape[1] - 1
        CU, CL, CR, Q, pos = (a[keep].reshape(H, wn) for a in (CU, CL, CR, Q, pos))
        with np.errstate(all="ignore"):
            for y in range(H):
                for x in (xs[y] - 1, xs[y]):
                    if not 0 <= x < wn:
                        continue
                    l, r = Is[:, y, pos[y, max(x - 1, 0)]], Is[:, y, pos[y, min(x + 1, wn - 1)]]
                    a = np.abs(r - l)
                    CU[y, x] = a.max()
                    if y > 0:
                        u = Is[:, y - 1, pos[y - 1, x]]
                        CL[y, x], CR[y, x] = (a + np.abs(u - l)).max(), (a + np.abs(u - r)).max()
    return out


def clip_forward_map(I_imgs, bias_imgs, depth, orientation, temporal):
    """the map of a clip whose frames' energies read I_imgs (a list of h x w float32, image orientation) under the bias planes bias_imgs
    (a list of h x w float32, or None): the dict lqr_vmap_dump's binding returns"""
    Is = np.stack([np.asarray(I, F) for I in I_imgs])
    L = Is.shape[1] if orientation else Is.shape[2]
    with np.errstate(all="ignore"):
        Ps = np.zeros(Is.shape, F) if bias_imgs is None else np.stack([np.asarray(b, F) for b in bias_imgs]) / F(L)
    if orientation:
        Is, Ps = Is.transpose(0, 2, 1), Ps.transpose(0, 2, 1)
    lv = levels(Is, Ps, depth, temporal)
    return dict(data=np.ascontiguousarray(lv.T if orientation else lv), depth=int(depth), orientation=int(orientation))


# ---- the kernels' own constants (csrc/lqr_common.h), from which the cases' shapes are derived ---------------------------------
def kernel_constants():
    K = FC.kernel_constants()
    src = open(os.path.join(ROOT, "gimp-lqr-plugin_amd", "csrc", "lqr_common.h")).read()
    for name in ("CLIPFWD_GROUP", "CLIPFWD_FOLD_THREADS", "CLIPFWD_REFRESH_THREADS"):
        (K[name],) = {int(v) for v in re.findall(r"^#define\s+%s\s+(\d+)" % name, src, re.M)}
    return K


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def make_frames(spec):
    """the n images of a spec: forward_cases.make_image with a seed per frame ("same": every frame the first one)"""
    if spec.get("same"):
        return [FC.make_image(spec)] * spec["n"]
    return [FC.make_image(dict(spec, seed=spec["seed"] * 100 + t)) for t in range(spec["n"])]


def make_biases(spec):
    """the float64 masks handed to lqr_carver_bias_add with factor spec["bias"], one per frame (None: no bias).  biaskind "random": as
    forward_cases.make_bias, a seed per frame; "last": a ramp along the lines of the carving direction, 0 at the first column and 1 at the last, on every frame (the
    bias travels with its pixel: with a negative factor that outweighs the costs every seam is the last column of its frame); "one": random on frame n // 2, 0 on the others"""
    if not spec.get("bias"):
        return None
    h, w, n = spec["h"], spec["w"], spec["n"]
    kind = spec.get("biaskind", "random")
    if kind == "last":
        m = np.tile(np.arange(w) / (w - 1.0), (h, 1)) if not spec["o"] else np.tile((np.arange(h) / (h - 1.0))[:, None], (1, w))
        return [m.copy() for _ in range(n)]
    masks = [FC.make_bias(dict(spec, seed=spec["seed"] * 100 + t)) for t in range(n)]
    if kind == "one":
        masks = [m if t == n // 2 else np.zeros((h, w)) for t, m in enumerate(masks)]
    return masks


def cases():
    """(name, spec): forward_cases' spec and n (frames), temporal, same (identical frames), biaskind"""
    out = []

    def add(name, w, h, o, d, **more):
        spec = dict(seed=52000 + len(out), w=w, h=h, o=o, d=d, n=2, temporal=1.0, ch=3, depth=0, type=None, nrg=2, content="grey4", bias=None,
                    biaskind="random", pre=None, init=False, same=False)
        spec.update(more)
        out.append((name, json.loads(json.dumps(spec))))

    # line lengths across the sweep's forms (threads x pixels per thread) and the LDS attribute; 2 - 5 lines, 2 frames
    add("L2", 2, 5, 0, 1)
    add("L3", 3, 4, 0, 2)
    add("L1023", 1023, 5, 0, 3, ch=1)
    add("L1024", 1024, 3, 0, 2, ch=1, content="float")
    add("L1025", 1025, 4, 0, 18, ch=1)
    add("L4097_v", 3, 4097, 1, 2, ch=1)
    add("L8193", 8193, 2, 0, 2, ch=1)
    add("L16384", 16384, 2, 0, 2, ch=1)
    # numbers of lines across the walk's row block, about 20 columns
    for H in (1, 2, 64, 65, 66, 193):
        add("H%d" % H, 17 + H % 7, H, 0, 3, ch=1, temporal=0.5)
    add("H65_v", 65, 21, 1, 20, ch=1)
    # numbers of frames across the fold's group, 40 x 12
    for n in (1, 2, GROUP, GROUP + 1):
        add("n%d" % n, 40, 12, 0, 9, n=n, ch=1, content="float", temporal=0.7)
    add("n%d_v" % (GROUP + 1), 40, 12, 1, 5, n=GROUP + 1, ch=1, temporal=0.25)
    add("n%d_bias" % (2 * GROUP + 1), 40, 12, 0, 7, n=2 * GROUP + 1, ch=1, bias=500, temporal=0.7)
    # depths
    add("depth_1", 31, 9, 0, 1, n=3)
    add("depth_max", 31, 9, 0, 30, n=3, content="float")
    add("depth_max_v", 9, 20, 1, 19, n=3)
    # all-equal frames: the ties alone decide, the seam is always at column 0
    add("flat", 19, 6, 0, 18, n=3, content="flat", same=True)
    # bias: drawn to the LAST column (the refresh at both borders); positive on one frame only (the maximum over frames)
    add("bias_last", 24, 10, 0, 23, n=3, bias=-4000, biaskind="last", content="float")
    add("bias_last_v", 10, 24, 1, 12, n=2, bias=-4000, biaskind="last")
    add("bias_one", 40, 15, 0, 9, n=4, bias=700, biaskind="one")
    add("bias_neg_v", 40, 15, 1, 7, n=3, bias=-900, content="float")
    add("temporal_0", 40, 15, 0, 11, n=4, temporal=0.0, content="float")
    add("temporal_5", 40, 15, 0, 11, n=4, temporal=5.0, content="float")
    # pixel types
    add("grey_8i", 45, 12, 0, 9, ch=1, n=3)
    add("rgb_8i_float", 50, 14, 0, 13, content="float", n=3)
    add("rgba_8i", 37, 14, 1, 6, ch=4, content="float", n=3)
    add("rgb_16i", 41, 9, 0, 7, depth=1, content="float", n=3)
    add("rgba_32f", 41, 9, 1, 4, ch=4, depth=2, content="float", n=3)
    add("grey_64f", 30, 11, 0, 8, ch=1, depth=3, content="float", n=3)
    add("cmyk_8i", 36, 10, 0, 6, ch=4, type=IT.CMYK, content="float", n=3)
    add("luma_rgb", 44, 13, 0, 8, nrg=5, content="float", n=3)
    # the frames' state beforehand
    add("pre_transposed", 38, 16, 0, 7, pre="transposed", init=True, n=3)
    add("pre_transposed_v", 38, 16, 1, 7, pre="transposed", init=True, content="float", n=3)
    add("pre_notflat", 38, 16, 0, 6, pre="notflat", init=True, content="float", n=3)
    add("pre_notflat_v", 38, 16, 1, 6, pre="notflat", init=True, n=3)
    add("init_rgb", 47, 10, 0, 12, init=True, content="float", n=3)
    return out


def block_hits(m, union):
    """seam pixels of a map on the positions the block of static_cases.crossing_block() visits"""
    return int((np.asarray(m["data"]) > 0)[union].sum())
