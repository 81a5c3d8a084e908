"""The launch geometry of the clip's forward build (the clip_* functions of gimp-lqr-plugin_amd/csrc/lqr_geom.h, and k_fwd_seam's LDS
layout, which its sweep takes over) without a GPU.  tests/c/clipfwd_geom_main.cc includes the header alone and is compiled as a program of
its own with -Werror under AddressSanitizer and UndefinedBehaviorSanitizer: the values are compared with plain arithmetic written out
below, the extents -- every block of a build allocated with exactly the stated bytes, its first and last element written -- are judged
by AddressSanitizer.  The shim and the kernels must take their sizes from those functions, which the last test reads off their text."""
import functools
import os
import re
import subprocess
import tempfile

import clipforward_cases as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gimp-lqr-plugin_amd", "csrc")
LS = (2, 3, 1023, 1024, 1025, 4097, 16384)
HS = (1, 2, 65, 2160)
NS = (1, 2, 16, 17, 64)


@functools.lru_cache(maxsize=None)
def program():
    exe = os.path.join(tempfile.mkdtemp(prefix="lqr_clipfwd_geom_"), "clipfwd_geom_main")
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + CSRC, os.path.join(ROOT, "tests", "c", "clipfwd_geom_main.cc"), "-o", exe], check=True)
    return exe


def run(what):
    r = subprocess.run([program(), what], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr.strip(), r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout.strip().split("\n")


def expected_values():
    K = CC.kernel_constants()
    out = ["CLIP_COST_FLOATS 4", "CLIP_REFRESH_VALUES 6", "clip_refresh_lds_elems %d %d" % (K["CLIPFWD_REFRESH_THREADS"], K["CLIPFWD_REFRESH_THREADS"] // 64 * 6)]
    out += ["clip_fold_groups %d %d" % (n, -(-n // K["CLIPFWD_GROUP"])) for n in NS]
    for L in LS:
        out.append("fwd_lds %d %d" % (L, 2 * L * 4))
        out.append("fwd_attr %d %d" % (L, 2 * L * 4 > 64 * 1024))
        for H in HS:
            out.append("clip_cost_elems %d %d %d" % (L, H, 4 * L * H))
            out.append("clip_cost_off %d %d %d" % (L, H, 4 * (L * H - 1)))
            for n in NS:
                out.append("clip_intensity_elems %d %d %d %d" % (L, H, n, n * L * H))
                out.append("clip_frame_off %d %d %d %d" % (L, H, n, (n - 1) * L * H))
    return out


def test_values_equal_plain_arithmetic():
    assert run("values") == expected_values()


def test_extents_first_and_last_element_of_blocks_of_exactly_the_stated_size():
    out = run("extents")
    blocks = sum(1 for L in LS for H in HS for n in NS if n * L * H * 4 <= 1 << 31) + 8 * len(LS) * len(HS) + len(LS) + 1
    assert out[-1] == "ok extents %d" % blocks, out[-3:]


def test_the_programs_constants_are_the_kernels_and_both_sides_take_their_sizes_from_the_header():
    K = CC.kernel_constants()
    prog = open(os.path.join(ROOT, "tests", "c", "clipfwd_geom_main.cc")).read()
    assert re.search(r"GROUP = %d, REFRESH_THREADS = %d;" % (K["CLIPFWD_GROUP"], K["CLIPFWD_REFRESH_THREADS"]), prog)
    assert K["CLIPFWD_GROUP"] == CC.GROUP
    shim = open(os.path.join(CSRC, "lqr_shim.hip")).read()
    kern = open(os.path.join(CSRC, "k_clipfwd.hip")).read()
    for fn in ("clip_intensity_elems", "clip_cost_elems", "clip_frame_off", "fwd_lds"):
        assert re.search(r"\b%s\(" % fn, shim[shim.index("lqrhip_clipfwd_begin"):]), fn
    for fn in ("clip_frame_off", "clip_cost_off", "clip_refresh_off", "clip_refresh_lds_elems", "fwd_row_off"):
        assert re.search(r"\b%s\(" % fn, kern), fn
