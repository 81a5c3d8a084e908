"""Colour depth on the MI355X: what a 16I / 32F / 64F carver costs against an 8-bit one, measured in one process on one box.

Workloads (all RGBA, vertical seams, delta_x 1, the library's default energy):
  single   one 3840 x 2160 image, 500 seams
  batch16  16 images of 3840 x 2160, 200 seams (lqrx_carver_resize_batch)
For every depth: the seam time (resize only: the carvers are made and uploaded before the clock starts), the upload time
(lqr_carver_new_ext + lqr_carver_init) and the read-out time (lqrx_carver_read_image; and its device share alone,
lqrx_carver_read_image_device) apart, and, in a second run with the
shim's HIP-event scopes on (lqrhip_prof_*), the per-kernel times of the seam loop.

    python scripts/bench_coldepth.py [--reps 3] [--out profiles/coldepth/bench.json]
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
DEPTHS = {"8I": 0, "16I": 1, "32F": 2, "64F": 3}


def image(w, h, seed, depth):
    v = D.photo_like(w, h, seed, channels=4)
    if depth == 0:
        return v
    if depth == 1:
        return v.astype(np.uint16) * 257
    return (v.astype(np.float64) / 255.0).astype(L.COLDEPTH_DTYPES[depth])


def run(eng, imgs, depth, w1, h1, prof):
    lib = eng.lib
    t0 = time.perf_counter()
    cs = [L.Carver.from_ext(eng, a, depth) for a in imgs]
    for c in cs:
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
    # the device's share of the read-out: the same compaction into device memory (lqrx_carver_read_image_device), no transfer to the host
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
    eng = L.bind_coldepth(L.engine_api())
    lib = eng.lib
    lib.lqrhip_prof_get.argtypes = [C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_longlong), C.POINTER(C.c_double)]
    lib.lqrhip_prof_enable.argtypes = [C.c_int]
    result = {}
    for wl in args.workloads.split(","):
        n, w, h, seams = WORKLOADS[wl]
        base = [image(w, h, 11 + i, 0) for i in range(n)]
        for dname, depth in DEPTHS.items():
            imgs = base if depth == 0 else [image(w, h, 11 + i, depth) for i in range(n)]
            run(eng, imgs[:1], depth, w - 8, h, False)          # warm-up: allocation cache, code objects
            best = None
            for _ in range(args.reps):
                r = run(eng, imgs, depth, w - seams, h, False)
                best = r if best is None or r[1] < best[1] else best
            kernels = run(eng, imgs, depth, w - seams, h, True)[4]
            t_up, t_seams, t_read, t_read_dev, _ = best
            result["%s_%s" % (wl, dname)] = dict(images=n, seams=seams, us_per_seam=round(1e6 * t_seams / seams, 1),
                                                  upload_ms=round(1e3 * t_up, 1), readout_ms=round(1e3 * t_read, 1),
                                                  readout_device_ms=round(1e3 * t_read_dev, 1),
                                                  mb_per_image=round(imgs[0].nbytes / 1e6, 1), kernels_ms=kernels)
            print(wl, dname, json.dumps(result["%s_%s" % (wl, dname)]), flush=True)
            del imgs
        for dname in ("16I", "32F", "64F"):
            a, b = result["%s_%s" % (wl, dname)], result["%s_8I" % wl]
            a["seam_ratio_vs_8I"] = round(a["us_per_seam"] / b["us_per_seam"], 3)
    line = json.dumps(result, sort_keys=True)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
