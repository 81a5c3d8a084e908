"""The energy read-outs on the MI355X (include/lqr_energy.h): what it costs to get the energy of a 3840 x 2160 RGBA carver out.

  image_dev_o0 / _o1   lqrx_carver_get_energy_image_device, RGBA 8-bit, into a device tensor, for seams of orientation 0 / 1
                       (the carver already lies that way: energy build + output stage; `first_o1` is the one call that also transposes)
  float_dev            lqrx_carver_get_energy_device (normalised floats into a device tensor)
  image_host           lqr_carver_get_energy_image, RGBA 8-bit, into host memory (the staging block and the pinned ring on top)
  parent               what a caller had to do before these calls existed: the test hook lqrx_carver_get_energy (w x h floats over PCIe)
                       plus the squash, the normalisation and the RGBA expansion in numpy (tests/energy_cases.py's model)
Each call returns after the device has finished, so a row's `ms` is wall-clock around the call, best of --reps.  `stage_ms` is the
output stage alone (k_energy_range + k_energy_out / k_energy_plane) between two HIP events on the engine's stream, best of --reps,
with the bytes it reads (the plane twice) and writes over that time, next to lqrhip_copy_bandwidth's streaming copy in the same run.

    python scripts/bench_energy_out.py [--reps 10] [--out profiles/energy_out/bench.json]
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
import torch  # noqa: E402

import datasets as D  # noqa: E402
import energy_cases as EC  # noqa: E402
import lqr_ctypes as L  # noqa: E402

W, H = 3840, 2160


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    eng = L.bind_energy(L.engine_api())
    lib = eng.lib
    lib.lqrhip_copy_bandwidth.argtypes = [C.c_ulonglong, C.c_int, C.POINTER(C.c_double)]
    lib.lqrhip_prof_enable.argtypes = [C.c_int]
    lib.lqrhip_prof_get.argtypes = [C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_longlong), C.POINTER(C.c_double)]

    def stage():
        """(ms, bytes) of the output-stage launches since the last reset"""
        ms, n, by = C.c_double(), C.c_longlong(), C.c_double()
        assert lib.lqrhip_prof_get(b"energy_out", C.byref(ms), C.byref(n), C.byref(by)) == 0 and n.value == 1, n.value
        lib.lqrhip_prof_reset()
        return ms.value, by.value

    def measure(fn):
        wall, st = [], []
        for _ in range(args.reps):
            lib.lqrhip_prof_reset()
            t0 = time.perf_counter()
            fn()
            wall.append(time.perf_counter() - t0)
            st.append(stage())
        ms, by = min(st)
        return dict(ms=round(1e3 * min(wall), 3), stage_ms=round(ms, 4), stage_mb=round(by / 1e6, 1), stage_gbps=round(by / ms / 1e6, 1))

    c = L.Carver(eng, D.photo_like(W, H, 11, channels=4))
    c.configure()
    px = W * H
    rgba = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    plane = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    res = {"pixels": px, "reps": args.reps, "device": torch.cuda.get_device_name(0)}
    gbps = C.c_double()
    assert lib.lqrhip_copy_bandwidth(256 << 20, 10, C.byref(gbps)) == 0
    res["copy_bandwidth_gbps"] = round(gbps.value, 1)
    lib.lqrhip_prof_enable(1)

    def row(name, d):
        res[name] = d
        print(name, json.dumps(d), flush=True)

    image = lambda o: (lambda: c.get_energy_image_device(rgba, o, L.LQR_COLDEPTH_8I, L.LQR_RGBA_IMAGE) == 1 or sys.exit("call failed"))  # noqa: E731
    image(0)()                                                      # warm-up: working planes, code objects
    row("image_dev_o0", measure(image(0)))
    lib.lqrhip_prof_reset()
    t0 = time.perf_counter()
    image(1)()
    row("first_o1", dict(ms=round(1e3 * (time.perf_counter() - t0), 3), note="includes the transposition of the carver"))
    row("image_dev_o1", measure(image(1)))
    image(0)()
    row("float_dev", measure(lambda: c.get_energy_device(plane, 0) == 1 or sys.exit("call failed")))
    row("image_host", measure(lambda: c.get_energy_image(0, L.LQR_COLDEPTH_8I, L.LQR_RGBA_IMAGE)))
    lib.lqrhip_prof_enable(0)
    want = c.get_energy_image(0, L.LQR_COLDEPTH_8I, L.LQR_RGBA_IMAGE)

    parts = []
    for _ in range(max(2, args.reps // 3)):
        t0 = time.perf_counter()
        true = c.energy()                                           # lqrx_carver_get_energy: the parent's only way out
        t1 = time.perf_counter()
        pic = EC.picture(true, L.LQR_COLDEPTH_8I, L.LQR_RGBA_IMAGE)
        t2 = time.perf_counter()
        parts.append((t2 - t0, t1 - t0, t2 - t1))
    assert np.array_equal(pic, want)                                # the same picture either way
    total, hook, model = min(parts)
    row("parent", dict(ms=round(1e3 * total, 1), hook_ms=round(1e3 * hook, 1), numpy_ms=round(1e3 * model, 1)))
    res["ratio_o1_over_o0_stage"] = round(res["image_dev_o1"]["stage_ms"] / res["image_dev_o0"]["stage_ms"], 2)
    c.destroy()
    print(json.dumps(res, sort_keys=True))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
