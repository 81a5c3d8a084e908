"""Static seams for a clip on the MI355X (include_ext/lqr_static.h): what the fold of 64 frames of 3840 x 2160 costs, next to the
streaming copy of the same bytes and to the route the engine had before (one energy read-out per frame and a maximum), and what a
static resize of the clip costs next to the batch resize alone, all on one device in one run.

  fold_8i / fold_64f     lqrx_carvers_static_energy_device on 64 RGBA frames of 8-bit / double channels.  `bytes` is what the fold moves:
                         the frames' pixels (and bias planes) once, S, T and I_prev read and written once per 16 frames, E written once;
                         `copy_ms` the time lqrhip_copy_bandwidth's streaming copy (scripts/dbg/t_copy.hip chose its form) takes for that
                         traffic, measured in the same run; `of_copy` = copy_ms / ms
  scaling_8i             the same call on the first 1, 16, 17 and all of the 8-bit frames: whether the time is a fixed cost or the frames'
  readouts_8i            64 x lqrx_carver_get_energy_device (true energy) and a running torch.maximum: the S term alone, as the engine
                         before this feature could form it (it lays out working planes and leaves the carvers in the orientation asked for)
  static_map             lqrx_carvers_static_map: fold, the key carver's resize by `seams` seams, the dump to host memory
  load_static            lqrx_carvers_load_static: the same, and the map loaded into all 64 frames
  resize_after_load      lqrx_carver_resize_batch of the loaded frames by `seams` seams
  resize_alone           the yardstick: lqrx_carver_resize_batch of 64 initialised frames, each finding seams of its own
  map_to_host / map_to_device   the two legs of the map's trip through host memory, measured apart: lqr_vmap_dump of a carver that holds
                         the map, and a copy of as many bytes from pageable host memory to the device
Wall-clock around calls that return after the device has finished; one uncounted repetition, then the best of `reps`.

    python scripts/bench_static.py [--reps 10] [--frames 64] [--out profiles/static/bench.json]
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

GROUP = 16


class Shared(L.Carver):
    """a carver on a pixel buffer it neither owns nor copies on the host (lqr_carver_set_preserve_input_image): 64 frames of doubles would
    otherwise keep 17 GB of host memory.  The device copies are the carvers' own"""

    @classmethod
    def on(cls, api, array, depth, init):
        self = cls.__new__(cls)
        self.api, self.depth, self.buffer = api, depth, array
        self.h0, self.w0, self.ch = array.shape
        self._cbs, self.events, self.aux = [], [], []
        self.p = api.lqr_carver_new_ext(array.ctypes.data, self.w0, self.h0, self.ch, depth)
        assert self.p
        api.lqr_carver_set_preserve_input_image(self.p)
        if init:
            assert api.lqr_carver_init(self.p, 1, 0.0) == L.LQR_OK
        return self


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--resize-reps", type=int, default=3)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--seams", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    W, H, N, S = args.width, args.height, args.frames, args.seams
    eng = L.engine_static_api()
    lib = eng.lib
    lib.lqrhip_copy_bandwidth.argtypes = [C.c_ulonglong, C.c_int, C.POINTER(C.c_double)]
    res = {"width": W, "height": H, "channels": 4, "frames": N, "seams": S, "reps": args.reps, "resize_reps": args.resize_reps,
           "alpha": 0.3, "device": torch.cuda.get_device_name(0)}
    gbps = C.c_double(0)
    assert lib.lqrhip_copy_bandwidth(2 << 30, 10, C.byref(gbps)) == 0
    res["copy_bandwidth_gbps"] = round(gbps.value, 1)

    base8 = D.photo_like(W, H, 11, channels=4)
    bases = {0: [base8, np.ascontiguousarray(np.roll(base8, (3, 5), (0, 1)))]}
    bases[3] = [b.astype(np.float64) / 255.0 for b in bases[0]]

    def clip(depth, init):
        cs = [Shared.on(eng, bases[depth][i & 1], depth, init) for i in range(N)]
        for c in cs:
            c.configure(nrg_func=L.LQR_EF_GRAD_XABS, enl_step=2.0)
        return cs

    def best(fn, reps):
        ts = []
        for rep in range(reps + 1):
            t0 = time.perf_counter()
            fn()
            if rep:
                ts.append(time.perf_counter() - t0)
        return dict(ms=round(1e3 * min(ts), 3), median_ms=round(1e3 * statistics.median(ts), 3), runs=len(ts))

    def check(ret):
        assert ret == L.LQR_OK, ret

    # ---- the fold ------------------------------------------------------------------------------------------------------------------
    e_dev = torch.empty((H, W), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for depth, name in ((0, "8i"), (3, "64f")):
        cs = clip(depth, False)
        row = best(lambda: check(L.static_energy_device(cs, e_dev, 0, 0.3)), args.reps)
        groups = -(-N // GROUP)
        px = W * H
        row["bytes"] = N * px * 4 * (1, 2, 4, 8)[depth] + (2 * (groups - 1) * 3 + 1) * px * 4
        row["copy_ms"] = round(row["bytes"] / (gbps.value * 1e9) * 1e3, 3)
        row["of_copy"] = round(row["copy_ms"] / row["ms"], 3)
        row["gbps"] = round(row["bytes"] / (row["ms"] * 1e-3) / 1e9, 1)
        res["fold_" + name] = row
        print("fold_" + name, json.dumps(row), flush=True)
        if depth == 0:
            s_only = torch.empty_like(e_dev)
            check(L.static_energy_device(cs, s_only, 0, 1.0))
            run, one = torch.empty_like(e_dev), torch.empty_like(e_dev)

            def readouts():
                for i, c in enumerate(cs):
                    check(c.get_energy_device(one if i else run, 0, true=True))
                    if i:
                        torch.maximum(run, one, out=run)
                torch.cuda.synchronize()
            res["readouts_8i"] = best(readouts, min(args.reps, 3))
            assert torch.equal(run, s_only)             # the same S, bit for bit
            res["readouts_8i"]["over_fold"] = round(res["readouts_8i"]["ms"] / row["ms"], 1)
            print("readouts_8i", json.dumps(res["readouts_8i"]), flush=True)
            res["scaling_8i"] = {str(n): best(lambda: check(L.static_energy_device(cs[:n], e_dev, 0, 0.3)), 5)["ms"]
                                 for n in sorted({1, 16, 17, N})}
            print("scaling_8i", json.dumps(res["scaling_8i"]), flush=True)
        for c in cs:
            c.destroy()
        del cs

    # ---- a static resize of the clip next to the batch resize alone ------------------------------------------------------------------
    times = {}

    def timed(name, fn, count):
        t0 = time.perf_counter()
        out = fn()
        if count:
            times.setdefault(name, []).append(time.perf_counter() - t0)
        return out
    for rep in range(args.resize_reps + 1):
        cs = clip(0, True)
        m = timed("static_map", lambda: L.static_map(cs, S, 0, 0.3), rep)
        assert m is not None
        timed("load_static", lambda: check(L.load_static(cs, S, 0, 0.3)), rep)
        timed("map_to_host", lambda: cs[0].vmap_dump(), rep)
        host = np.ascontiguousarray(m["data"])
        dev = torch.empty((H, W), dtype=torch.int32, device="cuda")

        def to_device():
            dev.copy_(torch.from_numpy(host))
            torch.cuda.synchronize()
        timed("map_to_device", to_device, rep)
        timed("resize_after_load", lambda: check(L.resize_batch(eng, cs, W - S, H)), rep)
        for c in cs:
            c.destroy()
        cs = clip(0, True)
        timed("resize_alone", lambda: check(L.resize_batch(eng, cs, W - S, H)), rep)
        for c in cs:
            c.destroy()
        del cs
    for name, ts in times.items():
        res[name] = dict(ms=round(1e3 * min(ts), 2), median_ms=round(1e3 * statistics.median(ts), 2), runs=len(ts))
        print(name, json.dumps(res[name]), flush=True)
    res["static_resize_ms"] = round(res["load_static"]["ms"] + res["resize_after_load"]["ms"], 2)
    res["static_over_alone"] = round(res["static_resize_ms"] / res["resize_alone"]["ms"], 2)
    res["host_trip_share_of_load"] = round((res["map_to_host"]["ms"] + res["map_to_device"]["ms"]) / res["load_static"]["ms"], 3)
    print(json.dumps({k: res[k] for k in ("static_resize_ms", "static_over_alone", "host_trip_share_of_load")}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
        write_readme(res, os.path.join(os.path.dirname(os.path.abspath(args.out)), "README.md"))


def write_readme(res, path):
    N, S = res["frames"], res["seams"]
    out = ["# Static seams for a clip: what the fold and a static resize cost", "",
           "`scripts/bench_static.py` on one MI355X (`bench.json`; the runtime names the device \"%s\"): %d RGBA frames of %d x %d,"
           % (res["device"], N, res["width"], res["height"]),
           "`include_ext/lqr_static.h`, DESIGN.md §3.8.  Wall-clock around calls that return after the device has finished; one uncounted",
           "repetition, then the best of %d (of %d for the resize rows).  The streaming copy (`lqrhip_copy_bandwidth`, the form"
           % (res["reps"], res["resize_reps"]),
           "`scripts/dbg/t_copy.hip` chose) ran at %.0f GB/s of read-plus-write traffic in the same run." % res["copy_bandwidth_gbps"], "",
           "## The fold (`lqrx_carvers_static_energy_device`, alpha 0.3, orientation 0)", "",
           "| frames | fold, ms | bytes moved | copy of the same bytes, ms | copy / fold | fold, GB/s |", "|---|---|---|---|---|---|"]
    for name, label in (("fold_8i", "%d x 8-bit RGBA" % N), ("fold_64f", "%d x 64F RGBA" % N)):
        r = res[name]
        out.append("| %s | %.2f | %.2f GB | %.2f | %.2f | %.0f |" % (label, r["ms"], r["bytes"] / 1e9, r["copy_ms"], r["of_copy"], r["gbps"]))
    out += ["",
            "The bytes are the frames' pixels once, S, T and I_prev read and written once per 16 frames, and E written once (these frames have no",
            "bias plane).  The route the engine had before -- %d x `lqrx_carver_get_energy_device` and a running `torch.maximum`, which gives the S"
            % N,
            "term alone, lays out working planes and leaves the carvers in the orientation asked for -- takes %.1f ms for the 8-bit clip, %.1f times"
            % (res["readouts_8i"]["ms"], res["readouts_8i"]["over_fold"]),
            "the fold; its plane equals the fold's S (alpha = 1) bit for bit."]
    slow = [n for n in ("fold_8i", "fold_64f") if res[n]["of_copy"] < 0.5]
    if slow:
        out += ["",
                "Below half the copy rate: %s.  Memory does not bound the fold, and it is no fixed cost: the two clips take"
                % " and ".join("the %s clip" % ("8-bit" if n == "fold_8i" else "64F") for n in slow),
                "%.1f and %.1f ms although one brings 4 bytes per pixel and the other 32, and the time is the frames' (a clip of %s of"
                % (res["fold_8i"]["ms"], res["fold_64f"]["ms"], ", ".join(sorted(res["scaling_8i"], key=int))),
                "these 8-bit frames: %s ms; %.0f us a frame).  That is CONSISTENT WITH a bound on instruction issue: about %d issue slots per"
                % (", ".join("%.2f" % res["scaling_8i"][k] for k in sorted(res["scaling_8i"], key=int)), 1e3 * res["fold_8i"]["ms"] / N,
                   round(256 * 64 * 2.4e9 * res["fold_8i"]["ms"] * 1e-3 / (N * res["width"] * res["height"]))),
                "pixel (256 units x 64 lanes at 2.4 GHz): every value is formed in double (an 8-bit RGBA pixel: four look-ups in the LDS table of",
                "v / 255, two double additions, an IEEE double division by 3, a double product with alpha), indexed with 64-bit arithmetic,",
                "stored to and read back from LDS as a double, and its gradient taken in double before anything is rounded to float -- the",
                "arithmetic `lqr_carver_get_true_energy` is pinned to, done one pixel per thread and step (DESIGN.md §3.8 has what was tried).  The",
                "next step is `k_wk_init_emap`'s: four columns per thread, so that index arithmetic and neighbours are shared.  No counters were",
                "collected, and these timings do not separate issue from latency: this is an inference, not a measurement."]
    out += ["", "## A static resize of the clip by %d seams" % S, "",
            "| step | ms |", "|---|---|",
            "| `lqrx_carvers_static_map` (fold, the key carver's resize, the dump) | %.1f |" % res["static_map"]["ms"],
            "| `lqrx_carvers_load_static` (the same, and the load into %d frames) | %.1f |" % (N, res["load_static"]["ms"]),
            "| `lqrx_carver_resize_batch` of the loaded frames | %.1f |" % res["resize_after_load"]["ms"],
            "| load + resize | %.1f |" % res["static_resize_ms"],
            "| `lqrx_carver_resize_batch` alone: every frame finds seams of its own | %.1f |" % res["resize_alone"]["ms"], "",
            "Load + resize is %.2f times the batch resize alone: ONE image's seams are found instead of %d.  (The resize of frames that hold a"
            % (res["static_over_alone"], N),
            "map finds nothing and moves nothing: the pixels are compacted when they are read, `lqrx_carver_read_sizes` or a scan.)",
            "The map passes from the key carver to the frames through host memory: `lqr_vmap_dump` of a %d x %d map takes %.1f ms, a copy of as"
            % (res["width"], res["height"], res["map_to_host"]["ms"]),
            "many bytes from pageable host memory to the device %.1f ms -- together %.0f %% of `lqrx_carvers_load_static`.  A device-to-device"
            % (res["map_to_device"]["ms"], 100 * res["host_trip_share_of_load"]),
            "hand-over would save that; it is out of scope here.", ""]
    with open(path, "w") as f:
        f.write("\n".join(out))


if __name__ == "__main__":
    main()
