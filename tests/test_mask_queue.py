"""The host-side queue behind lqr_carver_bias_add_xy / lqr_carver_rigmask_add_xy (gimp-lqr-plugin_amd/host/lqr_mask_queue.c) without a
GPU: the C file is compiled alone with a small stand-alone main (tests/c/mask_queue_main.c) under AddressSanitizer and
UndefinedBehaviorSanitizer, and the program is run: an empty flush, a single entry, repeats that force several buckets (the packed
order must give every pixel its values in call order, and no pixel twice in a bucket), the bound, reset followed by reuse."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gimp-lqr-plugin_amd", "host")


def test_queue_program_runs_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "mask_queue_main")
    subprocess.run(["gcc", "-std=c99", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + HOST, os.path.join(HOST, "lqr_mask_queue.c"), os.path.join(ROOT, "tests", "c", "mask_queue_main.c"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "mask queue ok" and not r.stderr.strip(), r.stderr


def test_queue_source_has_no_device_or_float_arithmetic():
    """the queue is bookkeeping: no HIP header, and the caller's value is stored, never computed with"""
    src = open(os.path.join(HOST, "lqr_mask_queue.c")).read()
    assert "hip" not in src.lower() and "lqr_hip.h" not in src
    assert "value[" in src and not any(op in src for op in ("value * ", "value / ", "value + ", "/ 2", "(float)"))
