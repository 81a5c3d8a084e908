"""Static seams for a clip (include_ext/lqr_static.h): THE SPECIFICATION of the folded energy plane, as a numpy model.

There is no liblqr counterpart.  In IMAGE orientation, for frame t of a clip of n frames of one configuration:

    B_t = the double the frame's energy function reads                     (imgtype_cases.model_value)
    I_t = (float) B_t                                                      (forward_cases.intensity: the I of lqr_forward.h)
    S_t = what lqr_carver_get_true_energy(frame t, ., orientation) stores  (true_energy below: the gradient of B_t in the frame of
          the carving direction, rounded to float, plus bias / L in float)
    S = max_t S_t        T = max_{t >= 1} |I_t - I_{t-1}| (float; 0 for n = 1)
    E = fl(fl(alpha S) + fl(fl(1 - alpha) T))

every float operation rounded on its own.  The engine equals this bit for bit (tests/test_static_gpu.py).  tests/energy_cases.py models
what the read-outs make OF a true-energy plane; the plane itself -- the gradient -- had no numpy form yet, so it is written here, with
this engine's conventions at the borders and in frames one pixel wide (include/lqr_energy.h), and tests/test_static_model.py pins it to
the CPU oracle's lqr_carver_get_true_energy.  The seams are liblqr's own, found on E by an LQR_EF_NULL carver whose bias plane is E
(bias_factor 2): key_map() runs that sequence of calls on any library, the CPU oracle included.
"""
import numpy as np

import forward_cases as FC
import imgtype_cases as IT

F = np.float32
D = np.float64
GROUP = 16          # frames per launch of k_static_fold (csrc/lqr_common.h STATIC_GROUP)
TILE = 64           # its tile (STATIC_TILE)
PAPER_ALPHA = 0.3


# ---- the model ----------------------------------------------------------------------------------------------------------------
def _central(B, axis):
    """the gradient along `axis` as the engine takes it: one-sided at both ends, (next - previous) * 0.5 between, 0 on a single line"""
    B = np.moveaxis(B, axis, -1)
    g = np.zeros(B.shape, D)
    if B.shape[-1] > 1:
        g[..., 0] = B[..., 1] - B[..., 0]
        g[..., -1] = B[..., -1] - B[..., -2]
        g[..., 1:-1] = (B[..., 2:] - B[..., :-2]) * D(0.5)
    return np.moveaxis(g, -1, axis)


def gradient_energy(B, nrg, orientation):
    """h x w float32: the built-in energy function `nrg` (LqrEnergyFuncBuiltinType; 6 and more: LQR_EF_NULL) on the values B (h x w
    float64, image orientation; brightness or luma as the function asks) as seams of `orientation` see it, without the bias"""
    B = np.asarray(B, D)
    if nrg < 0 or nrg > 5:
        return np.zeros(B.shape, F)
    kind = nrg % 3
    with np.errstate(all="ignore"):
        gx = _central(B, 0 if orientation else 1)           # along the lines of the carving direction
        if kind == 2:
            g = np.abs(gx)
        else:
            gy = _central(B, 1 if orientation else 0)
            g = np.sqrt(gx * gx + gy * gy) if kind == 0 else (np.abs(gx) + np.abs(gy)) * D(0.5)
        return g.astype(F)


def true_energy(B, nrg, orientation, bias=None):
    """lqr_carver_get_true_energy of a flat carver: the gradient energy plus bias / L, a float division and a float sum"""
    e = gradient_energy(B, nrg, orientation)
    if bias is not None:
        L = B.shape[0] if orientation else B.shape[1]
        with np.errstate(all="ignore"):
            e = e + np.asarray(bias, F) / F(L)
    assert e.dtype == F
    return e


def is_luma(nrg):
    return 3 <= nrg <= 5


def planes(imgs, depth, st, nrg, orientation, biases=None):
    """(S, T) of a clip: imgs a list of h x w x ch arrays of the depth's dtype, st the frames' imgtype_cases.TypeState, biases None or
    one h x w float32 bias plane per frame"""
    S = T = prev = None
    for t, img in enumerate(imgs):
        with np.errstate(all="ignore"):
            B = IT.model_value(img, depth, st, is_luma(nrg))
        I = FC.intensity(img, depth, st, is_luma(nrg))
        St = true_energy(B, nrg, orientation, None if biases is None else biases[t])
        if t == 0:
            S, T = St, np.zeros(St.shape, F)
        else:
            with np.errstate(all="ignore"):
                S = np.maximum(S, St)
                T = np.maximum(T, np.abs(I - prev))
        prev = I
    assert S.dtype == F and T.dtype == F
    return S, T


def mix(S, T, alpha):
    a = F(alpha)
    with np.errstate(all="ignore"):
        E = (a * np.asarray(S, F)).astype(F) + ((F(1) - a) * np.asarray(T, F)).astype(F)
    assert E.dtype == F
    return E


def static_energy(imgs, depth, st, nrg, orientation, alpha, biases=None):
    """E: h x w float32 in image orientation"""
    S, T = planes(imgs, depth, st, nrg, orientation, biases)
    return mix(S, T, alpha)


# ---- the seams: liblqr's own, on any library that has the calls (the CPU oracle: lqr_carver_bias_add_area on doubles) -----------
def key_map(api, cls, E, depth, orientation, delta_x=1, rigidity=0.0):
    """the map lqrx_carvers_static_map builds from E, by the sequence of calls include_ext/lqr_static.h names: the dict vmap_dump returns"""
    E = np.asarray(E, F)
    h, w = E.shape
    c = cls(api, np.zeros((h, w, 1), np.uint8), init=False)
    try:
        c.configure(nrg_func=6, enl_step=2.0)
        assert c.bias_add_f(E.astype(D), 2) == 1                # factor 2: the bias plane is E
        assert c.init(delta_x, rigidity) == 1
        assert c.resize(w if orientation else w - depth, h - depth if orientation else h) == 1
        return c.vmap_dump()
    finally:
        c.destroy()


def seam_pixels(m):
    """the pixels of a map's seams: h x w bool"""
    return np.asarray(m["data"]) > 0


# ---- the clip of the model test: a bright block crossing a dark clip ---------------------------------------------------------------
def crossing_block(w=96, h=24, n=6, side=8, value=255):
    """n grey frames w x h, black but for a side x side block that moves left to right, and the union of its positions"""
    frames, union = [], np.zeros((h, w), bool)
    y0 = (h - side) // 2
    for t in range(n):
        x0 = 4 + t * ((w - side - 8) // max(n - 1, 1))
        f = np.zeros((h, w, 1), np.uint8)
        f[y0:y0 + side, x0:x0 + side] = value
        union[y0:y0 + side, x0:x0 + side] = True
        frames.append(f)
    return frames, union
