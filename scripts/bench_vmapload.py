"""Seam-map loading on the MI355X (include/lqr_vmap.h): what it costs to give a 3840 x 2160 RGBA carver a 200-seam map, and to
replay one key frame's seams on 64 frames.

  load_host        lqr_vmap_load of a map in host memory into a fresh carver (upload through the pinned ring, k_vmap_check, k_inflate)
  load_device      lqrx_vmap_load_device of the same map in device memory (no copy: k_vmap_check, k_inflate)
  load_host_o1 / load_device_o1   the same for a horizontal-seam map of 200 seams (k_vmap_check_t writes the transposed plane;
                   the carver is transposed first)
  replay_64        lqrx_vmap_load_batch into 64 fresh carvers + lqrx_carver_resize_batch to the key frame's width + 64 read-outs into
                   device tensors (lqrx_carver_read_image_device)
  parent_64        what the parent commit can do for the same 64 results: 63 carvers attached to one root, the root carved (the 200
                   seams are COMPUTED here: without lqr_vmap_load there is no way to hand them over), the same 64 read-outs
Each call returns after the device has finished, so `ms` is wall-clock around the calls: the best and the median of --reps runs, each
on fresh carvers (creating them -- the upload of the frames -- is outside the window in every row).  `mb` is what the row's passes
have to move on the device, counted from the shapes (the map read by the check and by the inflate of every frame, every frame's
pixels read once and written once at the inflated width, a new visibility map per root), `gbps` that over the best time, and
`of_copy` its share of lqrhip_copy_bandwidth's streaming copy measured in the same run.

    python scripts/bench_vmapload.py [--reps 5] [--frames 64] [--out profiles/vmapload/bench.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--seams", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    W, H, S, N = args.width, args.height, args.seams, args.frames
    eng = L.bind_vmap(L.engine_api())
    lib = eng.lib
    lib.lqrhip_copy_bandwidth.argtypes = [C.c_ulonglong, C.c_int, C.POINTER(C.c_double)]
    base = D.photo_like(W, H, 11, channels=4)
    frame = lambda i: np.ascontiguousarray(np.roll(base, (3 * i, 5 * i), (0, 1)))       # noqa: E731  (distinct frames, cheaply)
    res = {"width": W, "height": H, "seams": S, "frames": N, "reps": args.reps, "device": torch.cuda.get_device_name(0)}
    gbps = C.c_double()
    assert lib.lqrhip_copy_bandwidth(256 << 20, 10, C.byref(gbps)) == 0
    res["copy_bandwidth_gbps"] = round(gbps.value, 1)

    def row(name, times, mb):
        best = min(times)
        d = dict(ms=round(1e3 * best, 3), median_ms=round(1e3 * statistics.median(times), 3), runs=len(times), mb=round(mb, 1),
                 gbps=round(mb / 1e3 / best, 1), of_copy=round(mb / 1e3 / best / gbps.value, 3))
        res[name] = d
        print(name, json.dumps(d), flush=True)

    px = W * H
    # bytes on the device: the check reads the map (an orientation-1 map is also written, transposed); the inflate of one root reads
    # the map and the pixels and writes the pixels and a visibility map at the inflated width; a transposition reads and writes the pixels
    check_mb = lambda o: 4 * px * (2 if o else 1) / 1e6                          # noqa: E731
    inflate_mb = lambda o: (4 * px + 4 * px + 2 * 4 * (px + S * (W if o else H))) / 1e6      # noqa: E731
    transpose_mb = 2 * 4 * px / 1e6

    # the key frame and its maps
    maps = {}
    for o in (0, 1):
        a = L.Carver(eng, frame(0))
        a.configure()
        t0 = time.perf_counter()
        assert a.resize(W - S, H) == 1 if o == 0 else a.resize(W, H - S) == 1
        res["carve_key_frame_o%d_ms" % o] = round(1e3 * (time.perf_counter() - t0), 1)
        maps[o] = a.vmap_dump()
        if o == 0:
            key_small = a.read_image()
        a.destroy()
        assert maps[o]["depth"] == S and maps[o]["orientation"] == o

    for o in (0, 1):
        m = maps[o]
        dev_map = torch.from_numpy(m["data"]).to("cuda")
        torch.cuda.synchronize()
        host, dev = [], []
        for rep in range(args.reps + 1):
            for kind, acc in (("host", host), ("device", dev)):
                c = L.Carver(eng, frame(1), init=False)
                v = L._b._vmap_new(eng, m)
                t0 = time.perf_counter()
                ret = eng.lqr_vmap_load(c.p, v) if kind == "host" else c.vmap_load_device(dev_map, S, o)
                dt = time.perf_counter() - t0
                eng.lqr_vmap_destroy(v)
                assert ret == 1
                if rep:                     # (the first run of each loads code objects and sizes the pinned ring)
                    acc.append(dt)
                if rep == args.reps and o == 0 and kind == "device":
                    assert c.resize(W - S, H) == 1 and c.read_image().shape == key_small.shape
                c.destroy()
        mb = check_mb(o) + inflate_mb(o) + (transpose_mb if o else 0)
        row("load_host" + ("_o1" if o else ""), host, mb)
        row("load_device" + ("_o1" if o else ""), dev, mb)
        del dev_map

    # 64 frames: one map, one batch
    m = maps[0]
    outs = [torch.empty((H, W - S, 4), dtype=torch.uint8, device="cuda") for _ in range(N)]
    torch.cuda.synchronize()

    def read_all(cs):
        for c, t in zip(cs, outs):
            assert eng.lqrx_carver_read_image_device(c.p, t.data_ptr()) == 1

    replay, parent, parts = [], [], []
    for rep in range(min(args.reps, 3) + 1):
        cs = [L.Carver(eng, frame(i), init=False) for i in range(N)]
        arr = (C.c_void_p * N)(*[c.p for c in cs])
        v = L._b._vmap_new(eng, m)
        t0 = time.perf_counter()
        assert eng.lqrx_vmap_load_batch(arr, N, v) == 1
        t1 = time.perf_counter()
        assert eng.lqrx_carver_resize_batch(arr, N, W - S, H) == 1
        t2 = time.perf_counter()
        read_all(cs)
        t3 = time.perf_counter()
        eng.lqr_vmap_destroy(v)
        if rep:
            replay.append(t3 - t0)
            parts.append([round(1e3 * (t1 - t0), 3), round(1e3 * (t2 - t1), 3), round(1e3 * (t3 - t2), 3)])
        if rep == 1:
            first = outs[0].cpu().numpy()
            assert np.array_equal(first, key_small), "frame 0 replayed is not the key frame carved"
            replay_frames = [t.cpu().numpy() for t in outs[:4]]
        for c in cs:
            c.destroy()
        del cs
    read_mb = N * (4 * px + 4 * px + 4 * (W - S) * H) / 1e6               # per read-out: pixels and map read, the visible ones written
    row("replay_%d" % N, replay, check_mb(0) + N * inflate_mb(0) + read_mb)
    res["replay_%d" % N]["load_resize_readout_ms"] = parts

    for rep in range(2):
        root = L.Carver(eng, frame(0))
        root.configure()
        aux = [root.attach(frame(i)) for i in range(1, N)]
        t0 = time.perf_counter()
        assert root.resize(W - S, H) == 1
        read_all([root] + aux)
        parent.append(time.perf_counter() - t0)
        if rep == 0:
            for k in range(4):
                assert np.array_equal(outs[k].cpu().numpy(), replay_frames[k]), "the attached carvers and the replay differ"
        root.destroy()
    res["parent_%d" % N] = dict(ms=round(1e3 * min(parent), 1), runs=len(parent), note="the root's 200 seams are computed inside the window")
    print("parent_%d" % N, json.dumps(res["parent_%d" % N]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
