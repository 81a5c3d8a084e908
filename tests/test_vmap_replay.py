"""tests/c/vmap_replay.c, a C caller of include/lqr_vmap.h (a key frame's seams replayed on the next frame): compiled with -Werror
against the header, with the built-in typedefs and under a GLib stand-in (CPU); linked to the engine and run, its output equals what
the Python binding gets from the same calls (gpu)."""
import os
import subprocess

import numpy as np
import pytest

import coldepth_cases as CD
import lqr_ctypes as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "vmap_replay.c")


@pytest.mark.parametrize("glib", [False, True])
def test_vmap_replay_compiles_with_werror_against_both_headers(tmp_path, glib):
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", SRC, "-o", str(tmp_path / "vmap_replay.o")]
    if glib:        # the header under a GLib stand-in, as tests/test_c_replay.py builds the plug-in's replay
        hdr = tmp_path / "glib_standin.h"
        hdr.write_text("typedef int gint; typedef unsigned int guint; typedef unsigned char guchar; typedef char gchar;\n"
                       "typedef float gfloat; typedef double gdouble; typedef int gboolean; typedef void *gpointer;\n")
        cmd[1:1] = ["-DLQR_NO_GLIB_TYPEDEFS", "-include", str(hdr)]
    subprocess.run(cmd, check=True)


@pytest.mark.gpu
def test_vmap_replay_c_equals_the_python_binding(tmp_path):
    eng = L.bind_vmap(L.engine_api())
    w, h, ch, w1, w2 = 90, 33, 3, 71, 104
    rng = np.random.default_rng(77)
    key, nxt = CD.base_image(rng, w, h, ch), CD.base_image(rng, w, h, ch)
    d = os.path.join(ROOT, "gimp-lqr-plugin_amd")
    exe = str(tmp_path / "vmap_replay")
    subprocess.run(["gcc", "-std=c99", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), SRC, "-o", exe,
                    "-L" + d, "-l:liblqr-hip.so", "-Wl,-rpath," + d, "-lm"], check=True)
    (tmp_path / "in.bin").write_bytes(np.array([w, h, ch, w1, w2], np.int32).tobytes() + key.tobytes() + nxt.tobytes())
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    raw = (tmp_path / "out.bin").read_bytes()
    depth, orientation = np.frombuffer(raw[:8], np.int32)
    vmap = np.frombuffer(raw[8:8 + 4 * w * h], np.int32).reshape(h, w)
    small = np.frombuffer(raw[8 + 4 * w * h:8 + 4 * w * h + w1 * h * ch], np.uint8).reshape(h, w1, ch)
    large = np.frombuffer(raw[8 + 4 * w * h + w1 * h * ch:], np.uint8).reshape(h, w2, ch)
    # the same calls through the binding
    a = L.Carver(eng, key)
    assert a.resize(w1, h) == 1
    m = a.vmap_dump()
    assert (m["depth"], m["orientation"]) == (depth, orientation) == (w - w1, 0) and np.array_equal(m["data"], vmap)
    b = L.Carver(eng, nxt, init=False)
    assert b.vmap_load(m) == 1 and b.resize(w1 - 1, h) == 0
    assert b.resize(w1, h) == 1 and np.array_equal(b.read_scanlines()[0], small)
    assert b.resize(w2, h) == 1 and np.array_equal(b.read_scanlines()[0], large)
    a.destroy(); b.destroy()
