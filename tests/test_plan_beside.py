"""Where a seam step runs the energy update beside the carve (k_carve_u, StepPlan::energy_beside in csrc/lqr_plan.h), without a GPU.
tests/c/plan_beside_main.cc includes the header alone and is compiled with -Werror under AddressSanitizer and
UndefinedBehaviorSanitizer, as tests/test_plan.py does with its program.  For group sizes 1 .. 96 (one batch, or 2 / 4 sibling
sub-batches), delta_x 0 .. 4, value planes and packed pixels, and frames 2, 3 and 100 wide:
  * energy_beside is set exactly where the rule restated here says: never at the knob's 0; a form exists for delta_x <= 2 on packed
    pixels while a frame is left (w - 1 > 1) and the step is not k_carve_e's; the knob at 1 takes every form, the automatic choice
    the batches that have their stream to themselves from BESIDE_MIN images;
  * the census slot of the carve (StepPlan::carve) is the one the two-launch plan has: the combined launch is counted as a carve."""
import functools
import os
import subprocess
import tempfile

import pytest

import geometry_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gimp-lqr-plugin_amd", "csrc")
BESIDE_MIN = 8          # profiles/carve_beside/README.md: the smallest group run whose two runs both beat both runs of the two launches


@functools.lru_cache(maxsize=None)
def program():
    exe = os.path.join(tempfile.mkdtemp(prefix="lqr_plan_beside_"), "plan_beside_main")
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "plan_beside_main.cc"), "-o", exe], check=True)
    return exe


def plans(knob):
    r = subprocess.run([program()], input="%d\n" % knob, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr.strip(), r.stdout[-2000:] + r.stderr[-4000:]
    head, *rows = r.stdout.strip().split("\n")
    return head, [tuple(int(x) for x in row.split()) for row in rows]


def test_the_threshold_and_the_default_are_the_measured_ones():
    head, _ = plans(-1)
    assert head == "min %d default -1" % BESIDE_MIN


@pytest.mark.parametrize("knob", [-1, 0, 1])
def test_energy_beside_is_set_exactly_where_the_rule_says(knob):
    _, rows = plans(knob)
    assert len(rows) == sum(1 for n in range(1, 97) for sn in (1, 2, 4) if n % sn == 0) * 5 * 2 * 3
    seen = set()
    for n, sn, delta, value, w, carve, beside, carve0 in rows:
        fused = delta <= 2 and n <= G.FROZEN_CARVE_FUSED and w - 1 > 1 and not value
        assert carve == carve0 == (G.CARVE_E if fused else G.CARVE), (n, sn, delta, value, w, carve, carve0)
        form = delta <= 2 and not value and w - 1 > 1 and not fused
        want = form and (knob == 1 or (knob == -1 and sn == 1 and n >= BESIDE_MIN))
        assert bool(beside) == want, (knob, n, sn, delta, value, w, beside)
        seen.add(bool(beside))
    assert seen == ({False} if knob == 0 else {False, True})
