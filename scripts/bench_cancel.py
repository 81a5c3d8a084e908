"""How long lqr_carver_cancel takes to stop a resize on the MI355X (include/lqr_control.h): a 3840 x 2160 RGBA image, 500 seams, delta_x 1
and 10, cancelled at the middle of the resize.

  with_update     the caller has an update callback at liblqr's default step (0.02: a report every 10 seams).  The callback of the
                  middle report calls lqr_carver_cancel.  The host has just synchronised there, so the yardstick is ONE REPORT
                  INTERVAL of that run (what the uncancelled run takes between two update callbacks).
  without_update  no update callback: the host enqueues the whole session within milliseconds and waits at its end, so a cancel from
                  a second thread, issued when half of the uncancelled run's time has passed, is seen at the session's end.  The
                  yardstick is THE REST OF THE SESSION (what the uncancelled run still takes from that moment).

`cancel_to_return_ms` is the time from the return of lqr_carver_cancel to the return of lqr_carver_resize; `uncancelled_remainder_ms`
is what the same configuration, not cancelled, takes from the same moment to the return of lqr_carver_resize.  There is no threshold:
the numbers are written to profiles/cancel/README.md beside their yardsticks.

    python scripts/bench_cancel.py [--reps 3] [--out profiles/cancel/bench.json] [--readme profiles/cancel/README.md]
"""
import argparse
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402,F401

import datasets as D  # noqa: E402
import lqr_ctypes as L  # noqa: E402


def carver(eng, img, delta, on_update=None):
    c = L.Carver(eng, img, delta_x=delta, rigidity=0.0)
    c.configure()
    if on_update is not None:
        prog = eng.lqr_progress_new()
        cb = L.PROGRESS_UPDATE(on_update)
        c._cbs.append(cb)
        eng.lqr_progress_set_update(prog, cb)
        eng.lqr_carver_set_progress(c.p, prog)
    return c


def with_update(eng, img, w1, h, delta, reports, cancel):
    """one resize; the callback of report `reports // 2` notes the time (and cancels): (ret, ms from there to the return, median ms
    between two reports, reports seen)"""
    stamps, mark = [], {}

    def on_update(_):
        stamps.append(time.perf_counter())
        if len(stamps) == reports // 2:
            if cancel:
                assert c.cancel() == L.LQR_OK
            mark["t"] = time.perf_counter()
        return L.LQR_OK
    c = carver(eng, img, delta, on_update)
    ret = c.resize(w1, h)
    t1 = time.perf_counter()
    gaps = [b - a for a, b in zip(stamps[1:], stamps[2:])]
    c.destroy()
    return ret, 1e3 * (t1 - mark["t"]), 1e3 * statistics.median(gaps), len(stamps)


def without_update(eng, img, w1, h, delta, cancel_after_s):
    """one resize without callbacks; cancel_after_s: a second thread cancels that long after the resize began: (ret, whole ms, ms from
    the cancel's return to the resize's)"""
    c = carver(eng, img, delta)
    mark, go = {}, threading.Event()

    def other():
        go.wait()
        time.sleep(cancel_after_s)
        mark["ret"] = c.cancel()
        mark["t"] = time.perf_counter()
    t = None
    if cancel_after_s is not None:
        t = threading.Thread(target=other)
        t.start()
    t0 = time.perf_counter()
    go.set()
    ret = c.resize(w1, h)
    t1 = time.perf_counter()
    if t:
        t.join()
    c.destroy()
    return ret, 1e3 * (t1 - t0), (1e3 * (t1 - mark["t"]) if t else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--seams", type=int, default=500)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cancel", "bench.json"))
    ap.add_argument("--readme", default=None)
    args = ap.parse_args()
    W, H, S = args.width, args.height, args.seams
    eng = L.engine_control_api()
    img = D.photo_like(W, H, 11, channels=4)
    reports = len(range(0, S, max(int(S * 0.02), 1)))
    res = dict(width=W, height=H, seams=S, reps=args.reps, reports=reports, rows=[])
    med = statistics.median
    for delta in (1, 10):
        with_update(eng, img, W - S, H, delta, reports, False)          # warm-up: caches, first-launch costs
        plain = [with_update(eng, img, W - S, H, delta, reports, False) for _ in range(args.reps)]
        canc = [with_update(eng, img, W - S, H, delta, reports, True) for _ in range(args.reps)]
        assert all(r[0] == L.LQR_OK and r[3] == reports for r in plain) and all(r[0] == L.LQR_USRCANCEL and r[3] == reports // 2 for r in canc)
        res["rows"].append(dict(delta=delta, case="with_update", cancel_to_return_ms=round(med(r[1] for r in canc), 3),
                                yardstick="one report interval", yardstick_ms=round(med(r[2] for r in plain), 3),
                                uncancelled_remainder_ms=round(med(r[1] for r in plain), 3)))
        whole = [without_update(eng, img, W - S, H, delta, None) for _ in range(args.reps)]
        total = med(r[1] for r in whole)
        canc = [without_update(eng, img, W - S, H, delta, total / 2e3) for _ in range(args.reps)]
        # (the one session is past its last check point when the host waits at its end: it commits, the call returns LQR_OK with the
        # whole result, and the mark is seen by the next call; a cancel that arrives while the host is still enqueueing gives LQR_USRCANCEL)
        res["rows"].append(dict(delta=delta, case="without_update", cancel_to_return_ms=round(med(r[2] for r in canc), 3),
                                yardstick="the rest of the session", yardstick_ms=round(total / 2, 3),
                                uncancelled_remainder_ms=round(total / 2, 3), uncancelled_whole_ms=round(total, 3),
                                returned=sorted({int(r[0]) for r in canc})))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    if args.readme:
        write_readme(args.readme, res)


def write_readme(path, res, headline=None):
    rows = "\n".join("| %d | %s | %s | %s: %s | %s |" % (r["delta"], r["case"], r["cancel_to_return_ms"], r["yardstick"], r["yardstick_ms"],
                                                         r["uncancelled_remainder_ms"]) for r in res["rows"])
    text = open(path).read() if os.path.exists(path) else ""
    head, _, tail = text.partition("<!-- bench_cancel: table -->")
    _, _, tail = tail.partition("<!-- bench_cancel: end -->")
    table = ("<!-- bench_cancel: table -->\n%d x %d RGBA, %d seams, %d reports at liblqr's default step, medians of %d runs, ms.\n\n"
             "| delta_x | case | cancel -> return of lqr_carver_resize | yardstick | uncancelled remainder |\n|---|---|---|---|---|\n%s\n<!-- bench_cancel: end -->"
             % (res["width"], res["height"], res["seams"], res["reports"], res["reps"], rows))
    with open(path, "w") as f:
        f.write((head or "# lqr_carver_cancel: how fast a resize stops\n\n") + table + tail)


if __name__ == "__main__":
    main()
