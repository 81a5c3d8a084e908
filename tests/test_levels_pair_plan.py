"""Slots per workgroup of the level kernel as the planner chooses them (gimp-lqr-plugin_amd/csrc/lqr_plan.h, plan_levels_wg_slots) and the
grid map of k_band_levels2 (csrc/lqr_geom.h, lv2_grid / lv2_block), without a GPU.  tests/c/plan_pair_main.cc includes the headers alone
and is compiled with -Werror under AddressSanitizer and UndefinedBehaviorSanitizer.  The rule is restated here independently:

  * two slots per workgroup need a form -- delta_x 1, no rigidity mask that matters, at least two slots per image, spinning kernels
    allowed (without them the level kernel is not used at all) -- and a grid of 8 ceil(images / 8) ceil(P / 2) workgroups within the
    batch's share of k_band_levels2's residency bound;
  * the knob at 2 takes the form wherever that holds, the knob at 1 never;
  * automatic (-1): never.  The form was measured on one stream and did not pay (profiles/levels_pair/README.md), so the rule that was
    reasoned for it -- a batch alone on its stream whose one-slot grid puts two workgroups on some compute unit, group x P > compute
    units -- is restated as AUTO_RULE and switched off by AUTO.
"""
import functools
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gimp-lqr-plugin_amd", "csrc")
N_CU = 256
AUTO = True


@functools.lru_cache(maxsize=None)
def program():
    exe = os.path.join(tempfile.mkdtemp(prefix="lqr_plan_pair_"), "plan_pair_main")
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "plan_pair_main.cc"), "-o", exe], check=True)
    return exe


def run(mode, text):
    r = subprocess.run([program(), mode], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr.strip(), r.stdout[-2000:] + r.stderr[-4000:]
    return [[int(x) for x in ln.split()] for ln in r.stdout.splitlines()]


def streams(group, queues):
    nb = (4 if group >= 49 else 2 if group >= 32 else 1) if queues >= 8 else 1
    return nb if group >= 2 * nb else 1


def slots_per_image(group, images, nb, spin):
    """plan_levels_P for a plain 4K group at delta_x 1 on a device that holds 768 one-slot workgroups (tests/test_plan_slots.py)"""
    if not spin or not 8 <= images * nb <= 64:          # (the group as the batches see it: images per batch x batches)
        return 0
    want = max(7, min(12, (384 if nb > 1 else 2 * N_CU) // (images * nb)))
    p = min(16, (768 // nb) // images, want)
    return p if p >= 7 else 0


def grid2(images, P):
    return 8 * ((images + 7) // 8) * ((P + 1) // 2)


def expected(group, queues, spin, knob, wgs2):
    nb = streams(group, queues)
    images = (group + nb - 1) // nb
    P = slots_per_image(group, images, nb, spin)
    if P == 0:
        return nb, images, 0, 1
    fits = P >= 2 and grid2(images, P) <= wgs2 // nb
    auto_rule = nb == 1 and images * nb * P > N_CU
    two = fits and (knob == 2 or (knob == -1 and AUTO and auto_rule))
    return nb, images, P, 2 if two else 1


@pytest.mark.parametrize("queues", [4, 8, 16])
@pytest.mark.parametrize("spin", [1, 0])
def test_slots_per_workgroup_for_every_group_size(queues, spin):
    rows = [(g, queues, spin, knob, wgs2) for g in range(1, 97) for knob in (-1, 1, 2) for wgs2 in (256, 512, 100, 0)]
    got = run("plan", "".join("%d %d %d %d %d\n" % r for r in rows))
    assert len(got) == len(rows)
    for row, g in zip(rows, got):
        assert tuple(g) == expected(*row), (row, g)
    # what the headline group gets on one stream when asked for the form: 64 images x 8 slots, 256 workgroups of two slots
    i = rows.index((64, queues, spin, 2, 256))
    if queues == 4:
        assert got[i] == ([1, 64, 8, 2] if spin else [1, 64, 0, 1])


@pytest.mark.parametrize("n", [1, 8, 9, 64])
def test_the_grid_map_is_one_to_one_onto_images_and_slot_pairs(n):
    Ps = list(range(2, 13))
    out = run("map", "".join("%d %d\n" % (n, P) for P in Ps))
    at = 0
    for P in Ps:
        pairs = (P + 1) // 2
        grid = out[at][0]; at += 1
        assert grid == 8 * ((n + 7) // 8) * pairs == grid2(n, P)
        blocks = [tuple(x) for x in out[at:at + grid]]; at += grid
        assert len(set(blocks)) == grid                                                     # no two blocks alike
        assert {b for b in blocks if b[0] < n} == {(i, s) for i in range(n) for s in range(pairs)}       # every image's every pair, once
        assert all(0 <= s < pairs and 0 <= i < 8 * ((n + 7) // 8) for i, s in blocks)
        for b, (i, s) in enumerate(blocks):
            assert i % 8 == b % 8                                                           # an image's workgroups share b mod 8
            # the slots of the pair: s and s + ceil(P / 2); the second is missing in the last workgroup of an odd P
            assert s + pairs < P or (P % 2 == 1 and s == pairs - 1)
    assert at == len(out)
