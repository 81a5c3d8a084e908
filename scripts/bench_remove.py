"""Object removal on the MI355X (include_ext/lqr_remove.h): what the discard scan costs next to the streaming copy of the bytes it reads, and
what a removal costs beyond the seams it carves, on a 3840 x 2160 RGBA carver with an ellipse of about 300 x 400 pixels marked, all on one
device in one run.

  copy_bandwidth_gbps    lqrhip_copy_bandwidth's streaming copy (read plus write traffic), the yardstick profiles/static/ uses
  line_scan / cross_scan lqrx_carver_discard_scan in the orientation the carver lies in / the other one: `kernel_ms` is device time between
                         events around the scan's launches (the cross scan's two), `bytes` what they read (bias0 and vs, 8 bytes per pixel,
                         and for the cross scan its counts written and read once), `copy_ms` the streaming copy's time for that traffic,
                         `of_copy` = copy_ms / kernel_ms; `call_ms` the whole call on the host's clock (result block zeroed, launches,
                         16 bytes back)
  removal                lqrx_carver_remove_discarded(orientation 0): seams, rounds, the seams the rounds carved (`carved`), ms
  resize_same_seams      the yardstick: lqr_carver_resize of the same carver by `carved` seams in one call
  per_round_ms           (removal - resize_same_seams) / rounds: what a round costs beyond its seams
  removal_step1          the same removal by a library built with LQRX_REMOVE_MIN_STEP 1 (--lib-step1; run in a child process)
Wall-clock around calls that return after the device has finished; one uncounted repetition, then the best of `reps` (scans) or of
`removal-reps` (removals and resizes: each takes a new carver).

    python scripts/bench_remove.py [--reps 10] [--removal-reps 3] [--lib-step1 PATH] [--out profiles/remove/bench.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import datasets as D  # noqa: E402
import lqr_ctypes as L  # noqa: E402


def ellipse(W, H, a, b):
    y, x = np.mgrid[0:H, 0:W]
    return ((((x - W // 2) / a) ** 2 + ((y - H // 2) / b) ** 2) <= 1.0).astype(np.float64)


def best(fn, reps):
    ts, last = [], None
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        last = fn()
        if rep:
            ts.append(time.perf_counter() - t0)
    return dict(ms=round(1e3 * min(ts), 3), median_ms=round(1e3 * statistics.median(ts), 3), runs=len(ts)), last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--removal-reps", type=int, default=3)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--lib-step1", default=None, help="a library built with -DLQRX_REMOVE_MIN_STEP=1: its removal is timed in a child process")
    ap.add_argument("--only-removal", action="store_true", help="(the child's mode) time the removal alone and print its row")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    W, H = args.width, args.height
    eng = L.engine_remove_api()
    lib = eng.lib
    img = D.photo_like(W, H, 11, channels=4)
    mask = ellipse(W, H, 150, 200)

    def fresh():
        c = L.Carver(eng, img)
        assert c.bias_add_f(mask, -1000) == L.LQR_OK
        return c.configure(nrg_func=L.LQR_EF_GRAD_XABS, switch_freq=2, enl_step=2.0)

    def removal():
        launches = (C.c_ulonglong * 4)()
        rows = []

        def once():
            c = fresh()
            eng.lqrhip_discard_launches(launches, 1)
            t0 = time.perf_counter()
            r = c.remove_discarded(0)
            dt = time.perf_counter() - t0
            eng.lqrhip_discard_launches(launches, 1)
            assert r["ret"] == L.LQR_OK and r["left"] == 0, r
            rows.append(dict(ms=dt, seams=r["seams"], rounds=int(launches[0]) - 1, carved=c.getters()["depth"]))
            c.destroy()
        for _ in range(args.removal_reps + 1):
            once()
        timed = rows[1:]
        assert len({(r["seams"], r["rounds"], r["carved"]) for r in timed}) == 1
        return dict(ms=round(1e3 * min(r["ms"] for r in timed), 3), median_ms=round(1e3 * statistics.median(r["ms"] for r in timed), 3), runs=len(timed),
                    seams=timed[0]["seams"], rounds=timed[0]["rounds"], carved=timed[0]["carved"])

    if args.only_removal:
        print(json.dumps(removal()))
        return

    lib.lqrhip_copy_bandwidth.argtypes = [C.c_ulonglong, C.c_int, C.POINTER(C.c_double)]
    lib.lqrhip_prof_enable.argtypes = [C.c_int]
    lib.lqrhip_prof_get.argtypes = [C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_longlong), C.POINTER(C.c_double)]
    res = {"width": W, "height": H, "channels": 4, "marked_ellipse": [300, 400], "marked_pixels": int(mask.sum()), "reps": args.reps,
           "removal_reps": args.removal_reps, "device": torch.cuda.get_device_name(0)}
    gbps = C.c_double(0)
    assert lib.lqrhip_copy_bandwidth(2 << 30, 10, C.byref(gbps)) == 0
    res["copy_bandwidth_gbps"] = round(gbps.value, 1)

    # ---- the scans, on the flat carver -------------------------------------------------------------------------------------------
    c = fresh()
    for o, name, prof in ((0, "line_scan", b"discard_line"), (1, "cross_scan", b"discard_cross")):
        row, got = best(lambda: c.discard_scan(o), args.reps)
        row = dict(call_ms=row["ms"], call_median_ms=row["median_ms"], runs=row["runs"], marked=got[1], need=got[2])
        lib.lqrhip_prof_enable(1)
        kernel = []
        for _ in range(args.reps + 1):
            lib.lqrhip_prof_reset()
            assert c.discard_scan(o)[0] == L.LQR_OK
            ms, n, nbytes = C.c_double(0), C.c_longlong(0), C.c_double(0)
            lib.lqrhip_prof_get(prof, C.byref(ms), C.byref(n), C.byref(nbytes))
            assert n.value == 1
            kernel.append(ms.value)
        lib.lqrhip_prof_enable(0)
        lib.lqrhip_prof_reset()
        row["kernel_ms"] = round(min(kernel[1:]), 4)
        row["kernel_median_ms"] = round(statistics.median(kernel[1:]), 4)
        row["bytes"] = int(nbytes.value)
        row["copy_ms"] = round(row["bytes"] / (gbps.value * 1e9) * 1e3, 4)
        row["of_copy"] = round(row["copy_ms"] / row["kernel_ms"], 3)
        row["gbps"] = round(row["bytes"] / (row["kernel_ms"] * 1e-3) / 1e9, 1)
        res[name] = row
        print(name, json.dumps(row), flush=True)
    res["guess_new_size_seams"] = W - eng.lqrx_guess_new_size(np.ascontiguousarray((mask * 255).astype(np.uint8)).ctypes.data, 1, W, H, 0, 0, W, H, 0)
    c.destroy()

    # ---- the removal, and the same seams in one resize ------------------------------------------------------------------------------
    res["removal"] = removal()
    print("removal", json.dumps(res["removal"]), flush=True)
    carved = res["removal"]["carved"]

    def resize():
        c = fresh()
        t0 = time.perf_counter()
        assert c.resize(W - carved, H) == L.LQR_OK
        dt = time.perf_counter() - t0
        c.destroy()
        return dt
    ts = [resize() for _ in range(args.removal_reps + 1)][1:]
    res["resize_same_seams"] = dict(ms=round(1e3 * min(ts), 3), median_ms=round(1e3 * statistics.median(ts), 3), runs=len(ts), seams=carved)
    res["per_round_ms"] = round((res["removal"]["ms"] - res["resize_same_seams"]["ms"]) / max(res["removal"]["rounds"], 1), 3)
    print("resize_same_seams", json.dumps(res["resize_same_seams"]), "per_round_ms", res["per_round_ms"], flush=True)

    if args.lib_step1:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--only-removal", "--removal-reps", str(args.removal_reps), "--width", str(W),
                              "--height", str(H)], env=dict(os.environ, LQR_HIP_LIB=os.path.abspath(args.lib_step1)), capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stderr[-2000:]
        res["removal_step1"] = json.loads(out.stdout.strip().split("\n")[-1])
        print("removal_step1", json.dumps(res["removal_step1"]), flush=True)

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
