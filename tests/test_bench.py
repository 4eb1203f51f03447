"""bench.py's command line: a plain run prints the headline line only, --dump-outputs writes what the last timed step
computed, from the same inputs on every run (-m gpu for the runs; the argument checks need no device)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--pairs", "96", "--points", "20000"]


def run(args, timeout=600):
    p = subprocess.run([sys.executable, "bench.py"] + args, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    return p


def bench_line(p):
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{"metric"')]
    assert len(lines) == 1, p.stdout[-3000:]
    return json.loads(lines[0])


@pytest.mark.parametrize("args", [["--steps", "0"], ["--warmup", "-1"], ["--config", "4", "--dump-outputs", "x"]])
def test_bench_refuses_bad_arguments(args):
    p = run(args, timeout=120)
    assert p.returncode == 2 and "error:" in p.stderr


@pytest.mark.gpu
def test_plain_run_and_dumped_outputs(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    line = bench_line(run(SMALL + ["--steps", "3", "--warmup", "1", "--dump-outputs", str(a)]))
    assert line["steps"] == 3 and line["warmup"] == 1 and line["value"] > 0 and line["ms_per_step"] > 0
    assert abs(line["value"] - 96 * 1e3 / line["ms_per_step"]) < 1e-6 * line["value"]
    for k in ("metric", "unit", "higher_is_better", "dtype"):
        assert k in line
    # the plain run is the headline alone: the extras need --full
    for k in ("roofline", "kernels", "steady_state", "cpu_baseline", "parity", "single_pair_latency", "dense_scene"):
        assert k not in line, k
    names = sorted(os.listdir(a))
    assert "poses.npy" in names and "result_converged.npy" in names and "result_score.npy" in names
    poses = np.load(a / "poses.npy")
    assert poses.shape == (96, 4, 4) and poses.dtype == np.float64
    assert np.allclose(poses[:, 3], [0, 0, 0, 1])
    assert np.load(a / "result_converged.npy").mean() > 0.8 and np.all(np.load(a / "result_n_target.npy") > 0)
    assert sum(os.path.getsize(a / n) for n in names) < 64 << 20
    # another run with other step counts: the same inputs, the same outputs
    bench_line(run(SMALL + ["--steps", "2", "--warmup", "0", "--dump-outputs", str(b)]))
    assert sorted(os.listdir(b)) == names
    for n in names:
        x, y = np.load(a / n), np.load(b / n)
        assert x.dtype == np.float64 and np.array_equal(x, y), n
