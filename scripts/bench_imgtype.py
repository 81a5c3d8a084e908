"""Image types on the MI355X: what a carver that reads through the value plane for its TYPE costs against the RGBA carver of the
same depth, measured in one process on one box.

Workloads (vertical seams, delta_x 1, the library's default energy), as scripts/bench_coldepth.py:
  single   one 3840 x 2160 image, 500 seams
  batch16  16 images of 3840 x 2160, 200 seams (lqrx_carver_resize_batch)
Carvers: 8I RGBA (packed pixels, fused carve + energy) and 8I CMYK (value plane); 32F RGBA and 32F CMYKA (both value plane,
16 and 20 bytes per pixel).  For each: the seam time, the upload (lqr_carver_new_ext + lqr_carver_init), the read-out
(lqrx_carver_read_image, and its device share) and, in a second run with the shim's HIP-event scopes on, the per-kernel times.

    python scripts/bench_imgtype.py [--reps 3] [--out profiles/imgtype/bench_imgtype.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import datasets as D  # noqa: E402
import lqr_ctypes as L  # noqa: E402

try:
    import torch
except Exception:           # (the device-only read-out time is then not measured)
    torch = None

SCOPES = ("vpath", "carve", "emap_update", "dp_sweep", "dp_update", "dp_update_tiled", "band_update", "band_levels")
WORKLOADS = {"single": (1, 3840, 2160, 500), "batch16": (16, 3840, 2160, 200)}
# name -> (depth, channels, image type to set or None, the carver it is compared with)
CARVERS = {"8I_RGBA": (0, 4, None, None), "8I_CMYK": (0, 4, L.LQR_CMYK_IMAGE, "8I_RGBA"),
           "32F_RGBA": (2, 4, None, None), "32F_CMYKA": (2, 5, None, "32F_RGBA")}


def image(w, h, seed, depth, ch, cmyk):
    """the RGBA photo, or the CMYK / CMYKA image of the same value (C M Y = 255 - R G B; CMYK: K = 255 - A, CMYKA: K = 0 and A):
    the energy reads the same number up to rounding, so both carvers of a pair remove seams in the same places -- k_carve moves
    the shorter side of a row, and its time depends on where the seam lies"""
    v = D.photo_like(w, h, seed, channels=4)
    if cmyk:
        a = v[:, :, 3:4]
        v = np.concatenate([255 - v[:, :, :3], 255 - a] if ch == 4 else [255 - v[:, :, :3], np.zeros_like(a), a], axis=2)
    return v if depth == 0 else (v.astype(np.float64) / 255.0).astype(L.COLDEPTH_DTYPES[depth])


def run(eng, imgs, depth, image_type, w1, h1, prof):
    lib = eng.lib
    t0 = time.perf_counter()
    cs = [L.Carver.from_ext(eng, a, depth) for a in imgs]
    for c in cs:
        if image_type is not None:
            assert c.set_image_type(image_type) == L.LQR_OK
        c.configure(nrg_func=L.LQR_EF_GRAD_XABS)
    assert lib.lqrhip_device_sync() == 0
    t_up = time.perf_counter() - t0
    if prof:
        lib.lqrhip_prof_reset()
        lib.lqrhip_prof_enable(1)
    t0 = time.perf_counter()
    ret = L.resize_batch(eng, cs, w1, h1) if len(cs) > 1 else cs[0].resize(w1, h1)
    assert lib.lqrhip_device_sync() == 0
    t_seams = time.perf_counter() - t0
    assert ret == L.LQR_OK, ret
    kernels = {}
    if prof:
        lib.lqrhip_prof_enable(0)
        for name in SCOPES:
            ms, n, by = C.c_double(), C.c_longlong(), C.c_double()
            lib.lqrhip_prof_get(name.encode(), C.byref(ms), C.byref(n), C.byref(by))
            if n.value:
                kernels[name] = dict(ms=round(ms.value, 3), launches=n.value)
    t0 = time.perf_counter()
    for c in cs:
        c.read_image_ext()
    t_read = time.perf_counter() - t0
    t_read_dev = 0.0
    if torch is not None:
        out = torch.empty(imgs[0].nbytes * w1 // imgs[0].shape[1] + 16, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for c in cs:
            assert eng.lqrx_carver_read_image_device(c.p, out.data_ptr()) == L.LQR_OK
        torch.cuda.synchronize()
        t_read_dev = time.perf_counter() - t0
    for c in cs:
        c.destroy()
    return t_up, t_seams, t_read, t_read_dev, kernels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--workloads", default="single,batch16")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    eng = L.bind_imagetype(L.engine_api())
    eng.lqrx_set_max_channels(5)
    lib = eng.lib
    lib.lqrhip_prof_get.argtypes = [C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_longlong), C.POINTER(C.c_double)]
    lib.lqrhip_prof_enable.argtypes = [C.c_int]
    result = {}
    for wl in args.workloads.split(","):
        n, w, h, seams = WORKLOADS[wl]
        for name, (depth, ch, image_type, against) in CARVERS.items():
            imgs = [image(w, h, 11 + i, depth, ch, against is not None) for i in range(n)]
            run(eng, imgs[:1], depth, image_type, w - 8, h, False)          # warm-up: allocation cache, code objects
            best = None
            for _ in range(args.reps):
                r = run(eng, imgs, depth, image_type, w - seams, h, False)
                best = r if best is None or r[1] < best[1] else best
            kernels = run(eng, imgs, depth, image_type, w - seams, h, True)[4]
            t_up, t_seams, t_read, t_read_dev, _ = best
            key = "%s_%s" % (wl, name)
            result[key] = dict(images=n, seams=seams, us_per_seam=round(1e6 * t_seams / seams, 1), upload_ms=round(1e3 * t_up, 1),
                               readout_ms=round(1e3 * t_read, 1), readout_device_ms=round(1e3 * t_read_dev, 1),
                               mb_per_image=round(imgs[0].nbytes / 1e6, 1), kernels_ms=kernels)
            if against:
                b = result["%s_%s" % (wl, against)]
                result[key].update(seam_ratio=round(result[key]["us_per_seam"] / b["us_per_seam"], 3), against=against,
                                   upload_ratio=round(result[key]["upload_ms"] / b["upload_ms"], 3),
                                   readout_ratio=round(result[key]["readout_ms"] / b["readout_ms"], 3))
            print(wl, name, json.dumps(result[key]), flush=True)
            del imgs
    line = json.dumps(result, sort_keys=True)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
