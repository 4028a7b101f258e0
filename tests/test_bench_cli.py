"""bench.py command line: the result line and --dump-outputs, on the tiny
CPU plumbing configuration (--cpu-smoke)."""
import json
import os
import subprocess
import sys

import numpy as np

from dist_util import REPO


def _run_bench(*extra):
    env = dict(os.environ)
    # stay on the CPU path even on a GPU box
    env.update({"HIP_VISIBLE_DEVICES": "", "ROCR_VISIBLE_DEVICES": "",
                "CUDA_VISIBLE_DEVICES": ""})
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"),
                        "--gpus", "1", "--cpu-smoke", "--batch", "2",
                        "--steps", "3", "--warmup", "1", *extra],
                       capture_output=True, text=True, env=env, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_bench_dump_outputs_repeatable(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    res = _run_bench("--dump-outputs", str(a))
    _run_bench("--full", "--dump-outputs", str(b))
    assert res["steps"] == 3 and res["warmup"] == 1
    assert res["ms_per_step"] > 0
    for key in ("metric", "value", "unit", "higher_is_better", "dtype"):
        assert key in res
    names = sorted(os.listdir(a))
    assert names == ["logits.npy", "loss.npy", "params.npy"]
    total = 0
    for n in names:
        x, y = np.load(a / n), np.load(b / n)
        assert x.dtype == np.float32 and x.size > 0
        assert np.isfinite(x).all()
        # same arguments -> same seeded weights and data -> same CPU results
        np.testing.assert_array_equal(x, y)
        total += x.nbytes
    assert total <= 64 * 2**20
    assert abs(float(np.load(a / "loss.npy")[0]) - res["config"]["loss"]) < 1e-3
