"""Forward-energy seam maps on the MI355X (include_ext/lqr_forward.h): what it costs to find 200 forward seams of a 3840 x 2160 RGBA image,
alone and for 64 images at once, next to the backward seam loop's resize by the same number of seams on the same device in the same run.

  build_1            lqrx_carver_forward_map_device: the map of one image into device memory
  forward_resize_1   lqrx_carver_resize_forward to (width - seams): build + load + resize
  backward_1         the yardstick: lqr_carver_resize of an initialised carver to the same size
  build_N            lqrx_carver_forward_maps_device for N images
  forward_resize_N   the same build, lqrx_vmap_load_device of each map, lqrx_carver_resize_batch (the forward path has no batch form of
                     the load and the resize of its own)
  backward_N         the yardstick: lqrx_carver_resize_batch of N initialised carvers
  cancel             lqr_carver_cancel from a second thread once two slices of a build are enqueued: from the cancel to the return of
                     lqrx_carver_load_forward (LQR_USRCANCEL)
Every call returns after the device has finished, so `ms` is wall-clock around the calls, on fresh carvers (creating them is outside
the window).  The rows of a group alternate, repetition by repetition; the first repetition of each (code objects, the pinned ring,
the pool's first blocks) is not counted.  `ratio` is a forward row's best time over its yardstick's.

    python scripts/bench_forward.py [--reps 3] [--batch 64] [--out profiles/forward/bench.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import datasets as D  # noqa: E402
import forward_cases as FC  # noqa: E402
import lqr_ctypes as L  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--batch-reps", type=int, default=2)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--seams", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    W, H, S, N = args.width, args.height, args.seams, args.batch
    eng = L.bind_forward(L.bind_control(L.engine_api()))
    base = D.photo_like(W, H, 11, channels=4)
    frame = lambda i: np.ascontiguousarray(np.roll(base, (3 * i, 5 * i), (0, 1)))       # noqa: E731  (distinct images, cheaply)
    res = {"width": W, "height": H, "channels": 4, "seams": S, "orientation": 0, "batch": N, "reps": args.reps, "batch_reps": args.batch_reps,
           "device": torch.cuda.get_device_name(0), "slice_seams": FC.kernel_constants()["FWD_SLICE_SEAMS"]}      # the host's own constant, read from its source
    times = {}

    def fresh(i, init):
        c = L.Carver(eng, frame(i), init=init)
        c.configure()
        return c

    def timed(name, fn, count):
        t0 = time.perf_counter()
        fn()
        dt = time.perf_counter() - t0
        if count:
            times.setdefault(name, []).append(dt)

    # ---- one image -----------------------------------------------------------------------------------------------------------
    dev_map = torch.empty((H, W), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for rep in range(args.reps + 1):
        c = fresh(0, False)
        timed("build_1", lambda: check(c.forward_map_device(dev_map, S, 0)), rep)
        c.destroy()
        c = fresh(0, False)
        timed("forward_resize_1", lambda: check(c.resize_forward(W - S, H)), rep)
        if rep == args.reps:
            assert c.read_image().shape == (H, W - S, 4) and np.array_equal(c.vmap_dump()["data"], dev_map.cpu().numpy())
        c.destroy()
        c = fresh(0, True)
        timed("backward_1", lambda: check(c.resize(W - S, H)), rep)
        c.destroy()

    # ---- a cancel during a build -----------------------------------------------------------------------------------------------
    lat = []
    for rep in range(args.reps):
        c = fresh(0, False)
        eng.lqrhip_forward_launches(1)
        box = {}

        def other():
            while eng.lqrhip_forward_launches(0) < 1 + 2 * 2 * res["slice_seams"] and "ret" not in box:
                pass
            c.cancel()
            box["t_cancel"] = time.perf_counter()
        t = threading.Thread(target=other)
        t.start()
        box["ret"] = c.load_forward(S, 0)
        t_ret = time.perf_counter()
        t.join()
        assert box["ret"] == L.LQR_USRCANCEL, box
        lat.append(t_ret - box["t_cancel"])
        c.destroy()
    res["cancel"] = dict(ms=round(1e3 * min(lat), 3), median_ms=round(1e3 * statistics.median(lat), 3), max_ms=round(1e3 * max(lat), 3), runs=len(lat))
    print("cancel", json.dumps(res["cancel"]), flush=True)

    # ---- N images --------------------------------------------------------------------------------------------------------------
    if N > 1:
        maps = [torch.empty((H, W), dtype=torch.int32, device="cuda") for _ in range(N)]
        torch.cuda.synchronize()
        for rep in range(args.batch_reps + 1):
            cs = [fresh(i, False) for i in range(N)]
            timed("build_%d" % N, lambda: check(L.forward_maps_device(cs, maps, S, 0)), rep)
            for c in cs:
                c.destroy()
            cs = [fresh(i, False) for i in range(N)]

            def forward_all():
                check(L.forward_maps_device(cs, maps, S, 0))
                for c, m in zip(cs, maps):
                    check(c.vmap_load_device(m, S, 0))
                check(L.resize_batch(eng, cs, W - S, H))
            timed("forward_resize_%d" % N, forward_all, rep)
            for c in cs:
                c.destroy()
            cs = [fresh(i, True) for i in range(N)]
            timed("backward_%d" % N, lambda: check(L.resize_batch(eng, cs, W - S, H)), rep)
            for c in cs:
                c.destroy()
            del cs

    for name, ts in times.items():
        res[name] = dict(ms=round(1e3 * min(ts), 2), median_ms=round(1e3 * statistics.median(ts), 2), runs=len(ts),
                         ms_per_seam=round(1e3 * min(ts) / S, 4))
    for n in (1, N) if N > 1 else (1,):
        for kind in ("build", "forward_resize"):
            res["%s_%d" % (kind, n)]["ratio"] = round(min(times["%s_%d" % (kind, n)]) / min(times["backward_%d" % n]), 2)
    for name in times:
        print(name, json.dumps(res[name]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
        write_readme(res, os.path.join(os.path.dirname(os.path.abspath(args.out)), "README.md"))


def write_readme(res, path):
    """the table of a result, beside it"""
    N, S = res["batch"], res["seams"]
    rows = [("1", "build_1", "forward_resize_1", "backward_1")]
    if "build_%d" % N in res:
        rows.append((str(N), "build_%d" % N, "forward_resize_%d" % N, "backward_%d" % N))
    out = ["# Forward-energy seam maps: what a build costs", "",
           "`scripts/bench_forward.py` on one MI355X (`bench.json`; the runtime names the device \"%s\"): %d forward seams of a %d x %d image of"
           % (res["device"], S, res["width"], res["height"]),
           "%d channels, orientation 0 (`include_ext/lqr_forward.h`, DESIGN.md §3.7), next to the backward seam loop's resize by the same number of"
           % res["channels"],
           "seams -- code this feature does not touch -- on the same device in the same run, the rows alternating.  Wall-clock around calls",
           "that return after the device has finished, on fresh carvers; one uncounted repetition, then the best of %d (of %d for the batch)."
           % (res["reps"], res["batch_reps"]), "",
           "| images | build alone, ms | build + load + resize, ms | backward resize, ms | build / backward | build + load + resize / backward |",
           "|---|---|---|---|---|---|"]
    for n, b, f, y in rows:
        out.append("| %s | %.1f (%.2f per seam) | %.1f | %.1f (%.2f per seam) | %.1f | %.1f |"
                   % (n, res[b]["ms"], res[b]["ms_per_seam"], res[f]["ms"], res[y]["ms"], res[y]["ms_per_seam"], res[b]["ratio"], res[f]["ratio"]))
    b1, f1 = res["build_1"]["ms"], res["forward_resize_1"]["ms"]
    if abs(f1 - b1) < 0.01 * b1:
        out += ["",
                "For one image the two forward columns do not differ (%.2f and %.2f ms): the load and the resize from a loaded map run no DP and"
                % (b1, f1),
                "cost less than the build varies from one repetition to the next, so this run does not resolve them.  The ratios are good to",
                "the digits shown, no further."]
    out += ["",
            "One workgroup finds the seams of one image: the sweep of a single image runs on one compute unit of 256, row after row behind a",
            "workgroup barrier (a chain of dependent rows; no counters were collected).  A batch runs one such workgroup per image side by side,",
            "so its time grows far slower than its size.  Nothing gates on these ratios: the",
            "next step, several workgroups per image, is named in DESIGN.md §3.7.", "",
            "A cancel (`lqr_carver_cancel` from a second thread once two slices of %d seams are enqueued) is honoured %.1f ms later (median of %d;"
            % (res["slice_seams"], res["cancel"]["median_ms"], res["cancel"]["runs"]),
            "worst %.1f ms): the host is at most two slices ahead of the device, and the call returns once what is enqueued has run out." % res["cancel"]["max_ms"], ""]
    with open(path, "w") as f:
        f.write("\n".join(out))


def check(ret):
    assert ret == L.LQR_OK, ret


if __name__ == "__main__":
    main()
