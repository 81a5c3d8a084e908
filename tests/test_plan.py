"""The launch shim's planner (gimp-lqr-plugin_amd/csrc/lqr_plan.h: which kernel form a full DP and a seam step run) without a GPU.
tests/c/plan_main.cc includes the header alone -- it is plain C++17 -- and is compiled with -Werror under AddressSanitizer and
UndefinedBehaviorSanitizer.  (1) For every single-image case of tests/geometry_cases.py the counters that the plans add up to equal
census(), the Python restatement the GPU census is judged against, slot by slot.  (2) Over widths 2 .. 16384, the heights either
side of every row threshold, delta_x 0 .. 16, group sizes and spinning on / off, every plan satisfies what the launch code relies on:
a spinning grid within the residency bound it was admitted under, heights within the tags' block field, a sweep that covers the row."""
import functools
import os
import subprocess
import tempfile

import pytest

import geometry_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gimp-lqr-plugin_amd", "csrc")
SINGLE = [c["name"] for c in G.CASES if c["kind"] in ("single", "planes")]


@functools.lru_cache(maxsize=None)
def plan_program():
    """the stand-alone program, built once per test run"""
    exe = os.path.join(tempfile.mkdtemp(prefix="lqr_plan_"), "plan_main")
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "plan_main.cc"), "-o", exe], check=True)
    return exe


def run_plan(text, timeout=120):
    r = subprocess.run([plan_program()], input=text, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and not r.stderr.strip(), r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def plan_input(c):
    """the case as the program reads it: the knobs as tests/test_geometry_gpu.py's set_hooks sets them, then the launch sequences"""
    hk, kw = c["hooks"], c["kw"]
    words = ["census", hk.get("vpath", -1), 3, hk.get("sweep_threads", 256), 4, hk.get("update_mode", -1), hk.get("band_levels", -1),
             hk.get("limit", -1), hk.get("px", 0), 0 if hk.get("no_spin", 0) else 1,
             kw.get("delta_x", 1), int(kw.get("rigidity", 0.0) != 0.0), int(bool(kw.get("rigmask")))]
    lines = [" ".join(str(x) for x in words)]
    for s in G.sessions(c):
        lines.append("D %d %d" % (s["fw"], s["fh"]))
        lines += ["S %d %d %d" % (wb, s["fh"], full) for wb, _, full in G.seam_steps(c, s)]
    return "\n".join(lines) + "\n"


def test_there_are_the_62_single_image_cases():
    assert len(SINGLE) == 62


@pytest.mark.parametrize("name", SINGLE)
def test_the_plans_add_up_to_the_restated_census(name):
    c = G.BY_NAME[name]
    got = [int(x) for x in run_plan(plan_input(c)).split()]
    want = G.census(c)
    assert len(got) == G.SLOTS
    for slot in range(G.SLOTS):
        if slot != G.LDS_ATTR_COMMIT:           # k_vs_commit's LDS size: not a choice
            assert got[slot] == want[slot], (G.SLOT_NAMES.get(slot, slot), got[slot], want[slot])


def test_every_plan_keeps_what_the_launch_code_relies_on():
    out = run_plan("sweep\n", timeout=600)
    assert out.startswith("sweep ok"), out
