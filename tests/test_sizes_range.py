"""lqr_geom_size_range (gimp-lqr-plugin_amd/host/lqr_sched.c), the range lqrx_carver_size_range reports, without a GPU: the C file is
compiled alone with a stand-alone main (tests/c/sizes_range_main.c) under AddressSanitizer and UndefinedBehaviorSanitizer and run as
a child process.  Over w_start 2 .. 70, every max_level, both orientations and the enlargement steps 1.01, 1.1, 1.5, 2.0 and 3.0 the
closed form must equal the sizes lqr_walk_needs_maps lets pass, found by brute force, and that set must be an interval that holds the
current width."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gimp-lqr-plugin_amd", "host")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("sizes_range") / "sizes_range_main")
    subprocess.run(["gcc", "-std=c99", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-ffp-contract=off", "-I" + HOST, os.path.join(HOST, "lqr_sched.c"), os.path.join(ROOT, "tests", "c", "sizes_range_main.c"),
                    "-o", out], check=True)
    return out


def test_closed_form_equals_the_walk_over_every_geometry(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr.strip(), r.stdout + r.stderr
    f = r.stdout.split()
    assert f[:3] == ["sizes", "range", "ok"], r.stdout
    # 69 values of w_start, sum of max_level counts 2 .. 70 = 2484, x 2 orientations x 5 steps x 5 widths
    assert int(f[3]) == 2484 * 2 * 5 * 5 and int(f[4]) > 1000
