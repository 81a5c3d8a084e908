"""The backtrack beside the carve (k_carve_v, csrc/k_carve.hip) without a GPU: the plain C++ it rests on -- csrc/lqr_beside.h (the side
bound, the work list's entries, which entries a part of the walk allows) and the planner's flag (StepPlan::backtrack_beside in
csrc/lqr_plan.h).  tests/c/beside_main.cc includes the headers alone and is compiled with -Werror under AddressSanitizer and
UndefinedBehaviorSanitizer, as tests/test_plan.py does with its program; its own header says what each check covers."""
import functools
import os
import subprocess
import tempfile

import pytest

import geometry_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gimp-lqr-plugin_amd", "csrc")
BESIDE_MIN = 8          # profiles/backtrack_beside/README.md
CARVE_BESIDE_MIN = 8    # tests/test_plan_beside.py
MIN_ROWS, MAX_ROWS, MAX_IMAGES = 37, 4096, 1024     # three 12-row chunks of steps; the walk role's path buffer; the entry's image field
FROZEN_LAG = 128        # frozen_lag(images > 4), csrc/lqr_plan.h


@functools.lru_cache(maxsize=None)
def program():
    exe = os.path.join(tempfile.mkdtemp(prefix="lqr_beside_"), "beside_main")
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "beside_main.cc"), "-o", exe], check=True)
    return exe


def run(what, stdin=""):
    r = subprocess.run([program(), what], input=stdin, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr.strip(), r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout.strip().split("\n")


def test_header_compiles_alone_as_plain_cxx():
    """csrc/lqr_beside.h by itself, no HIP and no other header of the engine in front of it"""
    with tempfile.TemporaryDirectory(prefix="lqr_beside_h_") as tmp:
        src = os.path.join(tmp, "alone.cc")
        with open(src, "w") as f:
            f.write('#include "lqr_beside.h"\nstatic_assert(bb_side_bound(0, 0, 0, 1, 2, 1) == 1, "one row on column 0 of two: the left part moves");\n'
                    'static_assert(bb_unpack(bb_pack(5, 1, 1023, 4095, 1, 16383)).index == 4095, "");\nint main() { return 0; }\n')
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + CSRC, src], check=True)


def test_an_early_side_is_the_side_of_the_whole_path():
    assert run("bound")[-1].startswith("ok bound")


def test_the_bound_fits_64_bits_on_the_largest_frame():
    assert run("overflow")[-1].startswith("ok overflow")


def test_entries_pack_and_unpack():
    assert run("pack")[-1].startswith("ok pack")


def test_every_entry_is_pushed_once_and_never_early():
    assert run("count")[-1].startswith("ok count")


def test_the_threshold_and_the_limits_are_the_stated_ones():
    head = run("plan", "-1\n")[0]
    assert head == "min %d default -1 vpath1 %d rows %d %d images %d" % (BESIDE_MIN, G.VPATH1, MIN_ROWS, MAX_ROWS, MAX_IMAGES)


@pytest.mark.parametrize("knob", [-1, 0, 1])
def test_backtrack_beside_is_set_exactly_where_the_rule_says(knob):
    rows = [tuple(int(x) for x in row.split()) for row in run("plan", "%d\n" % knob)[1:]]
    assert len(rows) > 10000
    seen = set()
    for n, sn, delta, value, w, h, spin, lag, backtrack, carve, energy_beside, catchup, beside in rows:
        images = n // sn
        # the energy update beside the carve, as tests/test_plan_beside.py restates it (its knob is at the default here)
        fused = delta <= 2 and n <= G.FROZEN_CARVE_FUSED and w - 1 > 1 and not value
        assert bool(energy_beside) == (delta <= 2 and not value and w - 1 > 1 and not fused and sn == 1 and n >= CARVE_BESIDE_MIN)
        assert bool(catchup) == (lag > (FROZEN_LAG if images > 4 else FROZEN_LAG // 4))
        form = bool(energy_beside) and backtrack == G.VPATH1 and 1 <= delta <= 2 and MIN_ROWS <= h <= MAX_ROWS and images <= MAX_IMAGES \
            and bool(spin) and not catchup
        want = form and (knob == 1 or (knob == -1 and sn == 1 and n >= BESIDE_MIN))
        assert bool(beside) == want, (knob, n, sn, delta, value, w, h, spin, lag, backtrack, beside)
        seen.add(bool(beside))
    assert seen == ({False} if knob == 0 else {False, True})
