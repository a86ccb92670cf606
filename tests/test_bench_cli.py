"""bench.py command-line contract on CPU (tiny sizes): one JSON result line
with ms_per_step, --steps honoured, --full accepted, and --dump-outputs
writing reproducible float32 arrays."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP, BATCH = 3, 1, 8


@pytest.fixture(scope="module")
def bench_runs(tmp_path_factory):
    """Two identical tiny CPU runs, started together; the second adds --full."""
    root = tmp_path_factory.mktemp("bench")
    env = dict(os.environ, OMP_NUM_THREADS="2")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    env["CUDA_VISIBLE_DEVICES"] = ""
    env["HIP_VISIBLE_DEVICES"] = ""
    procs = []
    for name, extra in (("a", []), ("b", ["--full"])):
        out_dir = str(root / name)
        procs.append((out_dir, subprocess.Popen(
            [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1",
             "--steps", str(STEPS), "--warmup", str(WARMUP),
             "--batch", str(BATCH), "--replay", "256",
             "--dump-outputs", out_dir] + extra,
            cwd=str(root), env=env, stdout=subprocess.PIPE,
            stderr=subprocess.PIPE, text=True,
        )))
    runs = []
    for out_dir, p in procs:
        out, err = p.communicate(timeout=120)
        assert p.returncode == 0, err[-2000:]
        runs.append((out_dir, out))
    return runs


def test_result_line(bench_runs):
    for _, out in bench_runs:
        lines = [ln for ln in out.splitlines() if ln.strip()]
        assert len(lines) == 1, out
        res = json.loads(lines[0])
        for key in ("metric", "value", "unit", "higher_is_better", "dtype",
                    "ms_per_step"):
            assert key in res, key
        assert res["steps"] == STEPS and res["warmup"] == WARMUP
        # independent of the echoed argument: the learner's own step counter
        # advanced by exactly STEPS inside the timed region
        assert res["steps_run"] == STEPS
        assert res["unit"] == "frames/s" and res["higher_is_better"] is True
        assert res["ms_per_step"] > 0
        # value and ms_per_step describe the same timed region
        fps = BATCH / (res["ms_per_step"] * 1e-3)
        assert abs(fps - res["value"]) <= 0.01 * res["value"]


def test_dump_outputs_reproducible(bench_runs):
    (dir_a, _), (dir_b, _) = bench_runs
    names = sorted(os.listdir(dir_a))
    assert names == sorted(os.listdir(dir_b))
    assert {"loss.npy", "value.npy", "params.npy"} <= set(names)
    assert np.load(os.path.join(dir_a, "params.npy")).size > 1000
    total = 0
    for n in names:
        a = np.load(os.path.join(dir_a, n))
        b = np.load(os.path.join(dir_b, n))
        assert a.dtype == np.float32
        assert np.isfinite(a).all()
        assert np.array_equal(a, b), n  # same arguments -> same inputs
        total += a.nbytes
    assert total <= 64 << 20


@pytest.mark.gpu
def test_dump_outputs_reproducible_on_gpu(tmp_path):
    """Two runs of the flagship GPU benchmark with the same arguments must
    write the same outputs up to rounding.

    Bound: loss and value are fp32 means over a batch of 512 whose terms
    are summed in hardware order, so two correct runs may differ by at most
    about 512 * 2^-24 = 3e-5 relative; rtol 1e-4 (+ atol 1e-5 for a value
    near zero) leaves a factor 3.

    This guards the fixed summation order of the conv weight-grad and
    bias-grad kernels and of the sum-tree update. When those accumulated
    with float atomics in hardware order, the last-bit jitter flipped a
    bf16 weight rounding within ~10 steps, priorities moved, the sampled
    batch changed and two runs decorrelated (110 steps: loss 0.0135 vs
    0.0094). With ordered sums two runs agree to ~2e-8 after 330 steps."""
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    procs = []
    for name in ("a", "b"):
        out_dir = str(tmp_path / name)
        procs.append((out_dir, subprocess.Popen(
            [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1",
             "--steps", "100", "--warmup", "10", "--dump-outputs", out_dir],
            cwd=str(tmp_path), env=env, stdout=subprocess.PIPE,
            stderr=subprocess.PIPE, text=True,
        )))
    for _, p in procs:
        _, err = p.communicate(timeout=120)
        assert p.returncode == 0, err[-2000:]
    (dir_a, _), (dir_b, _) = procs
    for n in sorted(os.listdir(dir_a)):
        a = np.load(os.path.join(dir_a, n))
        b = np.load(os.path.join(dir_b, n))
        print(n, a, b)
        assert np.allclose(a, b, rtol=1e-4, atol=1e-5), (n, a, b)
