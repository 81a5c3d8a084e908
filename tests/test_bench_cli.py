"""bench.py's command line: a plain run carries the headline only, --dump-outputs writes what the last timed step computed (the
same from run to run, with or without --full), and --full keeps the figures beyond the headline."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--steps", "2", "--warmup", "1", "--images-per-gpu", "3", "--seams", "20"]


def run(args, timeout=900):
    return subprocess.run([sys.executable, "bench.py"] + args, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True, timeout=timeout)


def result_line(p):
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_refuses_arguments_it_cannot_honour():
    """no timed step, or per-kernel times without --full: refused before any GPU work"""
    for args in (["--steps", "0"], ["--warmup", "-1"], ["--kernel-times"]):
        p = run(args, timeout=120)
        assert p.returncode == 2 and "error" in p.stderr, (args, p.returncode, p.stderr[-1000:])


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_dumps_the_last_step(tmp_path):
    plain = result_line(run(SMALL + ["--dump-outputs", str(tmp_path / "plain")]))
    assert plain["steps"] == 2 and plain["warmup"] == 1 and plain["ms_per_step"] > 0
    assert (plain["metric"], plain["unit"], plain["higher_is_better"], plain["dtype"]) == ("Mseams*pixels/sec on 4K RGBA", "Mseams*px/s", True, "f32")
    work = 3 * 20 * 3840 * 2160 * 2          # images x seams x W x H x steps
    assert abs(plain["value"] - work / (plain["ms_per_step"] * 2e-3) / 1e6) < 0.01 * plain["value"]
    for k in ("roofline", "kernels_ms", "phases", "cpu_baseline", "output_checksum", "configs"):
        assert k not in plain, k

    full = result_line(run(["--full", "--no-cpu-baseline", "--no-phases", "--no-kernel-breakdown"] + SMALL
                           + ["--dump-outputs", str(tmp_path / "full")]))
    assert full["roofline"] is not None and full["kernels_ms"]["carve"]["launches"] > 0 and full["output_checksum"] > 0

    names = sorted(os.listdir(tmp_path / "plain"))
    assert names == sorted(os.listdir(tmp_path / "full")) == ["images_channel_sum.npy", "images_sample.npy"]
    assert sum(os.path.getsize(tmp_path / "plain" / n) for n in names) <= 64 << 20
    for n in names:
        a, b = np.load(tmp_path / "plain" / n), np.load(tmp_path / "full" / n)
        assert a.dtype in (np.float32, np.float64) and a.shape[0] == 3, (n, a.dtype, a.shape)
        assert np.array_equal(a, b), n
    sums = np.load(tmp_path / "plain" / "images_channel_sum.npy")
    assert sums.shape == (3, 4) and int(sums.sum()) == full["output_checksum"]
    sample = np.load(tmp_path / "plain" / "images_sample.npy")
    assert sample.shape[2] == 4 and (sample[..., 3] == 255).all() and sample.min() >= 0 and sample.max() <= 255
