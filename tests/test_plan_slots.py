"""Slots per image of k_band_levels as the planner chooses them (gimp-lqr-plugin_amd/csrc/lqr_plan.h, plan_levels_P), without a GPU.
tests/c/plan_slots_main.cc includes the header alone and is compiled with -Werror under AddressSanitizer and
UndefinedBehaviorSanitizer, as tests/test_plan.py builds its program.  The rule is restated here independently:

  * a batch that shares its group with sibling streams asks for max(7, min(12, 384 / group)) slots per image -- the rule before a group
    alone on its stream got one of its own, so shared batches plan exactly as they did;
  * a batch alone on its stream asks for max(7, min(12, 2 * compute units / group)): 8 slots for 64 images, 10 for 48; up to 32
    images both rules give 12;
  * whatever is asked for, the plan never exceeds LV_PMAX slots, never more than the residency bound leaves every image of every
    sibling batch (wgs_levels / shared_n / images), and is 0 -- the level kernel is not used -- rather than below LV_AUTO_MIN;
  * a pinned count (lqrhip_set_band_levels) is taken as it is under the same two bounds, down to 1.
"""
import functools
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gimp-lqr-plugin_amd", "csrc")
N_CU = 256                  # the compute units tests/c/plan_slots_main.cc gives its device: an MI355X's
ALONE = 2 * N_CU            # workgroups a group alone on its stream may ask for: two per compute unit (profiles/onestream/README.md)
GROUPS = [8, 16, 32, 33, 48, 64]
BOUNDS = [768, 512, 448, 256, 100]        # an MI355X answers 768 (3 resident workgroups x 256 CUs); smaller ones make the bound bite


@functools.lru_cache(maxsize=None)
def program():
    exe = os.path.join(tempfile.mkdtemp(prefix="lqr_plan_slots_"), "plan_slots_main")
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "plan_slots_main.cc"), "-o", exe], check=True)
    return exe


def plan(rows):
    """rows of (images, shared_n, shared, wgs_levels, knob) -> (LV_PMAX, LV_AUTO_MIN, [P per row])"""
    text = "".join("%d %d %d %d %d\n" % r for r in rows)
    r = subprocess.run([program()], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr.strip(), r.stdout[-2000:] + r.stderr[-4000:]
    out = r.stdout.split()
    assert len(out) == 2 + len(rows)
    return int(out[0]), int(out[1]), [int(x) for x in out[2:]]


def expected(images, shared_n, shared, wgs, knob, pmax, auto_min):
    group = images * max(shared_n, 1)
    want = knob if knob > 0 else max(auto_min, min(12, (384 if shared else ALONE) // group))
    p = min(pmax, (wgs // max(shared_n, 1)) // images, want)
    return p if p >= (1 if knob > 0 else auto_min) else 0


def splits(group):
    """(images, shared_n) of a batch that shares a group of `group` images: two and four streams where the group divides, and the
    formula on its own (one batch flagged as shared) for every group"""
    return [(group, 1)] + [(group // n, n) for n in (2, 4) if group % n == 0]


def test_the_constants_are_the_ones_the_rule_is_restated_with():
    pmax, auto_min, _ = plan([])
    assert (pmax, auto_min) == (16, 7)
    assert ALONE == 512


@pytest.mark.parametrize("group", GROUPS)
def test_a_shared_batch_plans_as_before(group):
    rows = [(images, n, 1, wgs, -1) for images, n in splits(group) for wgs in BOUNDS]
    pmax, auto_min, got = plan(rows)
    for row, p in zip(rows, got):
        images, n, _, wgs, _ = row
        before = min(pmax, (wgs // n) // images, max(7, min(12, 384 // group)))       # the rule as it was, spelt out
        assert p == (before if before >= 7 else 0) == expected(*row, pmax, auto_min), row


@pytest.mark.parametrize("group", GROUPS)
def test_a_batch_alone_on_its_stream_gets_the_new_want(group):
    rows = [(group, 1, 0, wgs, -1) for wgs in BOUNDS]
    pmax, auto_min, got = plan(rows)
    for row, p in zip(rows, got):
        assert p == expected(*row, pmax, auto_min), row
    if group <= 32:         # the cap never bit there: alone or shared, 12 slots on an MI355X
        assert got[0] == 12 == plan([(group, 1, 1, BOUNDS[0], -1)])[2][0]
    else:
        assert got[0] == {33: 12, 48: 10, 64: 8}[group]


def test_the_bounds_hold_for_every_group_size_and_knob():
    rows = [(images, n, int(shared), wgs, knob) for images in range(1, 97) for n in (1, 2, 4) for shared in (n > 1, True)
            for wgs in BOUNDS + [0, 4096] for knob in (-1, 1, 5, 7, 9, 12, 16, 40)]
    pmax, auto_min, got = plan(rows)
    for row, p in zip(rows, got):
        images, n, _, wgs, knob = row
        assert 0 <= p <= pmax, row
        assert p * images * n <= wgs, row                   # every sibling batch's grid resident together
        assert p == 0 or p >= (1 if knob > 0 else auto_min), row
        assert p == expected(*row, pmax, auto_min), row


def test_a_count_of_zero_turns_the_level_kernel_off():
    assert plan([(16, 1, 0, 768, 0), (64, 1, 0, 768, 0)])[2] == [0, 0]
