"""Forward-energy seams for a clip on the MI355X (include_ext/lqr_clipforward.h): what one map from 64 RGBA frames of 3840 x 2160 costs,
next to the two routes the engine had before, all on one device in one run.

  fold                   the device time of k_clip_fold's launches inside a build (lqrhip_clipfwd_fold_ms).  `bytes` is what the fold moves:
                         one float per pixel and frame read, the costs (16 bytes per pixel) written once and, per 16 frames after the
                         first, read and written again; `copy_ms` the time lqrhip_copy_bandwidth's streaming copy takes for that traffic,
                         measured in the same run; `of_copy` = copy_ms / ms
  clip_load_forward      lqrx_clip_load_forward: the I planes, the fold, `seams` seams (sweep, removal, refresh), the load into all frames
  clip_map_device        lqrx_clip_forward_map_device: the same without the load
  forward_maps_device    lqrx_carver_forward_maps_device of the same frames: a map per frame, every frame its own seams
  load_static            lqrx_carvers_load_static of the same frames (alpha 0.3): backward seams on the folded energy plane
  per_seam_ms            (clip_map_device at `seams` seams - the same at 1 seam) / (seams - 1)
Wall-clock around calls that return after the device has finished; one uncounted repetition, then the best of `reps`.

    python scripts/bench_clipforward.py [--reps 10] [--frames 64] [--out profiles/clipforward/bench.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import datasets as D  # noqa: E402
import lqr_ctypes as L  # noqa: E402
from bench_static import Shared  # noqa: E402

GROUP = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--seams", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    W, H, N, S = args.width, args.height, args.frames, args.seams
    eng = L.bind_static(L.engine_clipforward_api())
    lib = eng.lib
    lib.lqrhip_copy_bandwidth.argtypes = [C.c_ulonglong, C.c_int, C.POINTER(C.c_double)]
    lib.lqrhip_clipfwd_fold_ms.restype = C.c_double
    res = {"width": W, "height": H, "channels": 4, "frames": N, "seams": S, "reps": args.reps, "temporal": 1.0, "alpha": 0.3,
           "device": torch.cuda.get_device_name(0)}
    gbps = C.c_double(0)
    assert lib.lqrhip_copy_bandwidth(2 << 30, 10, C.byref(gbps)) == 0
    res["copy_bandwidth_gbps"] = round(gbps.value, 1)
    base = D.photo_like(W, H, 11, channels=4)
    bases = [base, np.ascontiguousarray(np.roll(base, (3, 5), (0, 1)))]

    def clip(init):
        cs = [Shared.on(eng, bases[i & 1], 0, init) for i in range(N)]
        for c in cs:
            c.configure(nrg_func=L.LQR_EF_GRAD_XABS, enl_step=2.0)
        return cs

    def best(fn, reps, setup=None, teardown=None):
        ts = []
        for rep in range(reps + 1):
            arg = setup() if setup else None
            t0 = time.perf_counter()
            fn(arg) if setup else fn()
            dt = time.perf_counter() - t0
            if teardown:
                teardown(arg)
            if rep:
                ts.append(dt)
        return dict(ms=round(1e3 * min(ts), 3), median_ms=round(1e3 * statistics.median(ts), 3), max_ms=round(1e3 * max(ts), 3), runs=len(ts))

    def check(ret):
        assert ret == L.LQR_OK, ret

    def destroy(cs):
        for c in cs:
            c.destroy()

    px = W * H
    cs = clip(False)
    m_dev = torch.empty((H, W), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    # ---- the fold: device time inside a build of one seam ----------------------------------------------------------------------------
    folds = []

    def one_seam():
        check(L.clip_forward_map_device(cs, m_dev, 1, 0, 1.0))
        folds.append(lib.lqrhip_clipfwd_fold_ms())
    res["clip_map_device_1_seam"] = best(one_seam, args.reps)
    groups = -(-N // GROUP)
    row = dict(ms=round(min(folds[1:]), 3), median_ms=round(statistics.median(folds[1:]), 3), runs=len(folds) - 1)
    row["bytes"] = N * px * 4 + px * 16 + 2 * (groups - 1) * px * 16
    row["copy_ms"] = round(row["bytes"] / (gbps.value * 1e9) * 1e3, 3)
    row["of_copy"] = round(row["copy_ms"] / row["ms"], 3)
    row["gbps"] = round(row["bytes"] / (row["ms"] * 1e-3) / 1e9, 1)
    res["fold"] = row
    print("fold", json.dumps(row), flush=True)
    # ---- the whole map, and the routes the engine had --------------------------------------------------------------------------------
    res["clip_map_device"] = best(lambda: check(L.clip_forward_map_device(cs, m_dev, S, 0, 1.0)), args.reps)
    print("clip_map_device", json.dumps(res["clip_map_device"]), flush=True)
    res["per_seam_ms"] = round((res["clip_map_device"]["ms"] - res["clip_map_device_1_seam"]["ms"]) / max(S - 1, 1), 4)
    maps = [torch.empty((H, W), dtype=torch.int32, device="cuda") for _ in range(N)]
    res["forward_maps_device"] = best(lambda: check(L.forward_maps_device(cs, maps, S, 0)), args.reps)
    print("forward_maps_device", json.dumps(res["forward_maps_device"]), flush=True)
    del maps
    destroy(cs)
    # (a load changes the frames: new ones for every repetition, made outside the clock)
    res["clip_load_forward"] = best(lambda c: check(L.clip_load_forward(c, S, 0, 1.0)), args.reps, setup=lambda: clip(False), teardown=destroy)
    print("clip_load_forward", json.dumps(res["clip_load_forward"]), flush=True)
    res["load_static"] = best(lambda c: check(L.load_static(c, S, 0, 0.3)), min(args.reps, 3), setup=lambda: clip(False), teardown=destroy)
    print("load_static", json.dumps(res["load_static"]), flush=True)
    res["clip_over_forward_maps"] = round(res["clip_load_forward"]["ms"] / res["forward_maps_device"]["ms"], 2)
    res["clip_over_static"] = round(res["clip_load_forward"]["ms"] / res["load_static"]["ms"], 2)
    print(json.dumps({k: res[k] for k in ("per_seam_ms", "clip_over_forward_maps", "clip_over_static")}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
