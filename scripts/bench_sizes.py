"""A carver read at many sizes in one pass (include/lqr_sizes.h) on the MI355X, against the one-size-at-a-time way.

A 3840 x 2160 RGBA carver holds a 200-seam map (a seeded permutation map, loaded once: the read-out's cost does not depend on where the
levels lie), vertical seams for direction 0 and horizontal ones for direction 1.  K sizes spread evenly over the range are read

  new    one lqrx_carver_read_sizes_device (or lqrx_carver_read_sizes, the host form) call
  old    K x (lqr_carver_resize + lqrx_carver_read_image_device, or lqrx_carver_read_image for the host form): the only way before,
         and code this change does not touch.  In direction 1 the old device read-out leaves the image in CARVER orientation
         (transposed); the new call does the transposition too.

Rows: K = 1, 8 and 64 into device tensors in both directions, one 64F RGBA carver (32 bytes per pixel) at K = 8, and the host form at
K = 8 in direction 1.  Every call returns after the device has finished, so the time is wall-clock around the calls: one warm-up, then
the best of --reps runs (the median is kept too).  Beside each measured ratio new / old stands what the bytes alone predict: the old
way reads the base layout (pixels and levels, 8 bytes per RGBA pixel) and writes an image (4) K times, 12 K; the new one reads it
once and writes K images, 8 + 4 K, in direction 0, and writes and reads each image once more around the transposition, 8 + 12 K, in
direction 1 -- where it also makes K fewer synchronisations and delivers image orientation.

    python scripts/bench_sizes.py [--reps 10] [--out-dir profiles/sizes]

writes bench.json and the table of README.md (between the bench_sizes markers) in --out-dir.
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
import numpy as np  # noqa: E402
import torch  # noqa: E402

import datasets as D  # noqa: E402
import lqr_ctypes as L  # noqa: E402
import vmap_cases as VC  # noqa: E402

BEGIN, END = "<!-- bench_sizes: table -->", "<!-- bench_sizes: end -->"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--seams", type=int, default=200)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "sizes"))
    args = ap.parse_args()
    W, H, S = args.width, args.height, args.seams
    eng = L.bind_sizes(L.bind_vmap(L.bind_coldepth(L.engine_api())))
    res = {"width": W, "height": H, "seams": S, "reps": args.reps, "device": torch.cuda.get_device_name(0), "rows": []}
    base8 = D.photo_like(W, H, 11, channels=4)

    def carver(o, depth):
        img = base8 if depth == 0 else (base8.astype(np.float64) / 255.0)
        c = L.Carver.from_ext(eng, img, depth, init=False)
        assert c.vmap_load(VC.perm_map(1, W, H, S, o)) == 1
        assert c.size_range() == (o, (H if o else W) - S, (H if o else W) + S)
        return c, img.dtype.itemsize * 4

    def timed(fn):
        fn()                                    # warm-up: code objects, the allocation cache, the pinned ring
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return min(ts), statistics.median(ts)

    def row(o, K, depth, device):
        c, px = carver(o, depth)
        length = H if o else W
        sizes = [int(s) for s in np.linspace(length - S, length + S, K).round()] if K > 1 else [length - S // 2]
        shape = lambda s: (s, W) if o else (H, s)                                   # noqa: E731  (rows, columns)
        n_of = lambda s: shape(s)[0] * shape(s)[1] * px                            # noqa: E731
        if device:
            outs = [torch.empty(n_of(s), dtype=torch.uint8, device="cuda") for s in sizes]
            olds = [torch.empty(n_of(s), dtype=torch.uint8, device="cuda") for s in sizes]
            ptr = lambda t: t.data_ptr()                                            # noqa: E731
        else:
            outs = [np.empty(n_of(s), np.uint8) for s in sizes]
            olds = [np.empty(n_of(s), np.uint8) for s in sizes]
            ptr = lambda a: a.ctypes.data                                           # noqa: E731
        torch.cuda.synchronize()
        arr = (C.c_int * K)(*sizes)
        ptrs = (C.c_void_p * K)(*[ptr(t) for t in outs])
        new_fn = eng.lqrx_carver_read_sizes_device if device else eng.lqrx_carver_read_sizes
        old_fn = eng.lqrx_carver_read_image_device if device else eng.lqrx_carver_read_image

        def new():
            assert new_fn(c.p, arr, K, ptrs) == 1

        def old():
            for s, t in zip(sizes, olds):
                assert c.resize(W, s) == 1 if o else c.resize(s, H) == 1
                assert old_fn(c.p, ptr(t)) == 1

        new_best, new_med = timed(new)
        old_best, old_med = timed(old)
        assert c.resize(W, H) == 1
        # the same pixels (the old device read-out of direction 1 is in carver orientation: transposed)
        for s, a, b in zip(sizes[:2], outs, olds):
            a = (a.cpu().numpy() if device else a).reshape(shape(s) + (px,))
            b = (b.cpu().numpy() if device else b)
            b = b.reshape(W, s, px).swapaxes(0, 1) if (o and device) else b.reshape(shape(s) + (px,))
            assert np.array_equal(a, b), (o, K, s)
        predicted = ((px + 4) + (3 if o else 1) * px * K) / ((2 * px + 4) * K)        # RGBA: (8 + 4 K) / 12 K and (8 + 12 K) / 12 K
        r = dict(direction=o, K=K, bytes_per_pixel=px, into="device" if device else "host", new_ms=round(1e3 * new_best, 3),
                 new_median_ms=round(1e3 * new_med, 3), old_ms=round(1e3 * old_best, 3), old_median_ms=round(1e3 * old_med, 3),
                 ratio=round(new_best / old_best, 3), bytes_predict=round(predicted, 3),
                 new_gbps=round((2 * px * (W + S) * H + (3 if o else 1) * sum(n_of(s) for s in sizes)) / new_best / 1e9, 1))
        res["rows"].append(r)
        print(json.dumps(r), flush=True)
        c.destroy()
        del outs, olds
        torch.cuda.empty_cache()

    for o in (0, 1):
        for K in (1, 8, 64):
            row(o, K, 0, True)
    row(0, 8, 3, True)
    row(1, 8, 0, False)

    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    lines = [BEGIN, "%d x %d, %d seams, best of %d runs after one warm-up, ms; %s." % (W, H, S, args.reps, res["device"]), "",
             "| direction | K | pixel | into | new: one call | old: K x (resize + read-out) | new / old | bytes alone predict |", "|---|---|---|---|---|---|---|---|"]
    for r in res["rows"]:
        lines.append("| %d | %d | %d B | %s | %.3f | %.3f | %.3f | %.3f%s |" % (
            r["direction"], r["K"], r["bytes_per_pixel"], r["into"], r["new_ms"], r["old_ms"], r["ratio"], r["bytes_predict"],
            " and %d fewer synchronisations" % (r["K"] - 1) if r["direction"] and r["K"] > 1 else ""))
    lines.append(END)
    readme = os.path.join(args.out_dir, "README.md")
    text = open(readme).read() if os.path.exists(readme) else "# Reading a carver at many sizes in one pass\n\n%s\n%s\n" % (BEGIN, END)
    head, rest = text.split(BEGIN, 1)
    with open(readme, "w") as f:
        f.write(head + "\n".join(lines) + rest.split(END, 1)[1])


if __name__ == "__main__":
    main()
