"""What the level kernel writes back as the planner chooses it (gimp-lqr-plugin_amd/csrc/lqr_plan.h, plan_levels_store), without a GPU.
tests/c/plan_store_main.cc includes the header alone and is compiled with -Werror under AddressSanitizer and UndefinedBehaviorSanitizer.
The rule is restated here independently: only the two-slot family k_band_levels2 writes changed rows and lanes only, so a step's
store_rows is 1 exactly where the planner takes that family (a batch alone on its stream whose one-slot grid exceeds one workgroup per
compute unit: groups of 32 images and more on one stream) and the knob is not 0; groups on the one-slot family (8 and 16 images, which
lost 2.5 % with the change bits kept) and steps that do not run the level kernel get 0.  profiles/levels_store/README.md has the
measurements the rule rests on."""
import functools
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gimp-lqr-plugin_amd", "csrc")


@functools.lru_cache(maxsize=None)
def program():
    exe = os.path.join(tempfile.mkdtemp(prefix="lqr_plan_store_"), "plan_store_main")
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "plan_store_main.cc"), "-o", exe], check=True)
    return exe


N_CU = 256


def expected_store(knob, nb, images, P):
    two_slots = P >= 2 and nb == 1 and images * P > N_CU and 8 * ((images + 7) // 8) * ((P + 1) // 2) <= 256
    return 1 if two_slots and knob != 0 else 0


@pytest.mark.parametrize("queues", [4, 8, 16])
@pytest.mark.parametrize("spin", [1, 0])
def test_rows_written_back_for_every_group_size(queues, spin):
    rows = [(g, queues, spin, knob) for g in range(1, 97) for knob in (-1, 0, 1, 2, -7)]
    r = subprocess.run([program()], input="".join("%d %d %d %d\n" % x for x in rows), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr.strip(), r.stdout[-2000:] + r.stderr[-4000:]
    got = [[int(x) for x in ln.split()] for ln in r.stdout.splitlines()]
    assert len(got) == len(rows)
    ran = 0
    for (g, _, _, knob), (nb, images, P, wg, store) in zip(rows, got):
        assert store == (expected_store(knob, nb, images, P) if P > 0 else 0), ((g, queues, spin, knob), (nb, images, P, wg, store))
        assert store == 0 or wg == 2
        ran += P > 0
    # the headline group runs the level kernel on one stream, and writes the changed rows unless told otherwise
    if queues == 4 and spin:
        assert got[rows.index((64, queues, spin, -1))] == [1, 64, 8, 2, 1] and got[rows.index((64, queues, spin, 0))] == [1, 64, 8, 2, 0]
        assert got[rows.index((32, queues, spin, -1))][3:] == [2, 1] and got[rows.index((48, queues, spin, 1))][3:] == [2, 1]
        assert got[rows.index((8, queues, spin, 1))][3:] == [1, 0] and got[rows.index((16, queues, spin, -1))][3:] == [1, 0]
    assert (ran > 0) == bool(spin)
