"""Computed masks on the MI355X (include/lqr_masks.h): what it costs to get a full-frame 3840 x 2160 mask into a carver, by every way in.

  rgb        lqr_carver_bias_add_rgb_area on a one-channel 8-bit mask (8 MB from host memory): the form the plug-in uses, for scale
  host64     lqr_carver_bias_add_area on gdoubles in host memory (66 MB staged to the device, then one pass)
  dev64      lqrx_carver_bias_add_area_device on a float64 tensor already on the device (one pass: 8 B read + 8 B of plane traffic per pixel)
  dev32      the same on a float32 tensor (4 B + 8 B per pixel)
  xy         one lqr_carver_bias_add_xy per pixel from a compiled C loop (what a digiKam-style caller does): the calls, and apart
             from them the flush that the next plane access triggers (upload of the queue + the scatter launches)
Each is the best of --reps on a carver that already has its plane; times are wall-clock around the call, which returns after the
device has finished.  The yardstick for the device forms is the streaming copy of lqrhip_copy_bandwidth.

    python scripts/bench_masks.py [--reps 5] [--out profiles/masks/bench.json]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import datasets as D  # noqa: E402
import lqr_ctypes as L  # noqa: E402

W, H = 3840, 2160

XY_LOOP_C = r"""
typedef int (*add_xy)(void *carver, double value, int x, int y);
/* every pixel of a w x h frame, row-major, values from `mask`; returns the number of calls that did not return LQR_OK */
int xy_loop(add_xy f, void *carver, const double *mask, int w, int h)
{
    int x, y, bad = 0;
    for (y = 0; y < h; y++)
        for (x = 0; x < w; x++) bad += f(carver, mask[(long) y * w + x], x, y) != 1;
    return bad;
}
"""


def best_of(reps, fn):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return min(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    eng = L.bind_masks(L.engine_api())
    lib = eng.lib
    lib.lqrhip_copy_bandwidth.argtypes = [C.c_ulonglong, C.c_int, C.POINTER(C.c_double)]
    tmp = tempfile.mkdtemp()
    with open(os.path.join(tmp, "xy_loop.c"), "w") as f:
        f.write(XY_LOOP_C)
    subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", os.path.join(tmp, "xy_loop.c"), "-o", os.path.join(tmp, "xy_loop.so")])
    loop = C.CDLL(os.path.join(tmp, "xy_loop.so")).xy_loop
    loop.argtypes, loop.restype = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int], C.c_int

    rng = np.random.default_rng(1)
    c = L.Carver(eng, D.photo_like(W, H, 11, channels=4))
    c.configure()
    m64 = rng.uniform(0.01, 1.0, (H, W))
    m32 = m64.astype(np.float32)
    m8 = (m64 * 255).astype(np.uint8)[:, :, None]
    t64, t32 = torch.from_numpy(m64).cuda(), torch.from_numpy(m32).cuda()
    torch.cuda.synchronize()
    px = W * H
    assert c.bias_add(m8, 3) == 1 and c.bias_add_f(m64, 3, 0, 0) == 1 and c.bias_add_device(t64, 3) == 1      # warm-up: plane, staging, code objects
    res = {"pixels": px}
    gbps = C.c_double()
    assert lib.lqrhip_copy_bandwidth(256 << 20, 10, C.byref(gbps)) == 0
    res["copy_bandwidth_gbps"] = round(gbps.value, 1)

    def row(name, seconds, bytes_in, device_bytes):
        res[name] = dict(ms=round(1e3 * seconds, 3), input_mb=round(bytes_in / 1e6, 1), input_gbps=round(bytes_in / seconds / 1e9, 2),
                         device_traffic_gbps=round(device_bytes / seconds / 1e9, 1))
        print(name, json.dumps(res[name]), flush=True)

    row("rgb", best_of(args.reps, lambda: c.bias_add(m8, 3)), px, px * 9)
    row("host64", best_of(args.reps, lambda: c.bias_add_f(m64, 3, 0, 0)), px * 8, px * 16)
    row("dev64", best_of(args.reps, lambda: c.bias_add_device(t64, 3)), px * 8, px * 16)
    row("dev32", best_of(args.reps, lambda: c.bias_add_device(t32, 3)), px * 4, px * 12)

    fn = C.cast(eng.lqr_carver_bias_add_xy, C.c_void_p)
    calls, flush, launches = [], [], []
    for _ in range(args.reps):
        n0 = eng.lqrhip_debug_mask_flushes()
        t0 = time.perf_counter()
        assert loop(fn, c.p, m64.ctypes.data, W, H) == 0
        t1 = time.perf_counter()
        assert c.flatten() == 1                     # a flat carver: nothing but the flush of what is queued
        t2 = time.perf_counter()
        calls.append(t1 - t0); flush.append(t2 - t1); launches.append(eng.lqrhip_debug_mask_flushes() - n0)
    k = int(np.argmin(np.add(calls, flush)))
    res["xy"] = dict(calls=px, calls_ms=round(1e3 * calls[k], 1), ns_per_call=round(1e9 * calls[k] / px, 1), flush_ms=round(1e3 * flush[k], 1),
                     scatter_launches=launches[k], queue_bound_entries=1 << 22,
                     note="launches and their uploads that the queue's bound forces during the calls are inside calls_ms")
    print("xy", json.dumps(res["xy"]), flush=True)
    c.destroy()
    print(json.dumps(res, sort_keys=True))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
