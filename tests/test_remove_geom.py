"""The launch geometry of the discard scan (the discard_* functions of gimp-lqr-plugin_amd/csrc/lqr_geom.h) without a GPU.
tests/c/discard_geom_main.cc includes the header alone and is compiled as a program of its own with -Werror under AddressSanitizer and
UndefinedBehaviorSanitizer: the values are compared with plain arithmetic written out below; the extents -- the planes, the result block and
the cross scan's counts allocated with exactly the stated bytes, every access of the three kernels made by their index expressions over
their whole grids, the line scan's 16-byte reads checked to be aligned, every pixel read exactly once by each scan -- are judged by
AddressSanitizer."""
import functools
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gimp-lqr-plugin_amd", "csrc")
WS = (1, 2, 3, 5, 40, 255, 256, 257, 1023, 1024, 1025, 2049, 3840)
HS = (1, 3, 5, 9, 31, 32, 33, 65, 300)


@functools.lru_cache(maxsize=None)
def program():
    exe = os.path.join(tempfile.mkdtemp(prefix="lqr_discard_geom_"), "discard_geom_main")
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + CSRC, os.path.join(ROOT, "tests", "c", "discard_geom_main.cc"), "-o", exe], check=True)
    return exe


def run(what):
    r = subprocess.run([program(), what], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr.strip(), r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout.strip().split("\n")


def expected_values():
    out = ["DISCARD_THREADS 256", "DISCARD_CHUNK 1024", "DISCARD_ROWS 32", "DISCARD_WORDS 4", "discard_result_elems 8", "discard_result_off 0 4"]
    for w in WS:
        out.append("discard_col_blocks %d %d" % (w, -(-w // 256)))
        out.append("discard_rank_elems %d %d" % (w, w))
        for h in HS:
            tiles = -(-h // 32)
            out.append("discard_row_tiles %d %d" % (h, tiles))
            out.append("discard_partial_elems %d %d %d" % (w, h, tiles * w))
            out.append("discard_partial_off %d %d %d" % (w, h, tiles * w - 1))
            out.append("discard_lead %d %d %d" % (w, h, ((h - 1) * w) % 4))
    return out


def test_values_equal_plain_arithmetic():
    assert run("values") == expected_values()


def test_extents_every_access_of_the_three_kernels_in_blocks_of_exactly_the_stated_size():
    assert run("extents")[-1] == "ok extents %d" % (len(WS) * len(HS))


def test_the_programs_index_expressions_are_the_kernels():
    """the restated expressions must be the ones k_discard.hip has: the loop heads and the addresses, compared as text"""
    squeeze = lambda s: re.sub(r"\s+", "", s)
    prog = squeeze(open(os.path.join(ROOT, "tests", "c", "discard_geom_main.cc")).read())
    kern = squeeze(open(os.path.join(CSRC, "k_discard.hip")).read())
    for expr in ("for (int base = -discard_lead((size_t) y, w0); base < w0; base += DISCARD_CHUNK)", "const int g = base + 4 * tid;",
                 "if (g >= 0 && g + 3 < w0)", "if ((unsigned) (g + k) < (unsigned) w0)", "const size_t at = (size_t) y * w0 + x;",
                 "partial[discard_partial_off(tile, x, w0)] = count;", "for (int t = 0; t < tiles; t++) line += partial[discard_partial_off(t, x, w0)];"):
        assert squeeze(expr) in kern, expr
    for expr in ("for (int base = -discard_lead((size_t) y, w0); base < w0; base += DISCARD_CHUNK)", "const int g = base + 4 * tid;",
                 "if (g >= 0 && g + 3 < w0)", "if ((unsigned) (g + k) < (unsigned) w0)", "const size_t at = (size_t) y * w0 + x;",
                 "for (int t = 0; t < tiles; t++) line += partial[discard_partial_off(t, x, w0)];"):
        assert squeeze(expr) in prog, expr
