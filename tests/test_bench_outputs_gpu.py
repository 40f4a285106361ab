"""bench.py's plain run and --dump-outputs: the plain line carries the headline keys and no leg of --full; --steps sets the timed
steps; the dump holds float32 / float64 arrays within 64 MB, the same in two runs with the same arguments (the step is bitwise
deterministic), and its scalars are the ones the line reports."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "16",
           "--dump-outputs", str(out_dir), *extra]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    out = _bench(tmp_path / "a")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in out, k
    assert out["steps"] == 3 and out["warmup"] == 1 and out["dtype"] == "bf16" and out["higher_is_better"] is True
    assert abs(out["value"] - 16 / (out["ms_per_step"] * 1e-3)) < 1e-2 * out["value"]
    for k in ("secondary", "cpu_baseline", "roofline", "kernels"):
        assert k not in out, k
    a = _load(tmp_path / "a")
    assert a["fake"].shape == (16, 3, 64, 64) and "G.conv1.weight" in a and "D.conv5.weight" in a
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64_000_000
    assert np.all(np.abs(a["fake"]) <= 1.0)                               # tanh output
    for k in ("loss_d", "loss_g", "gp"):
        assert round(float(a["scalar." + k][0]), 5) == out["losses_last_step"][k], k
    _bench(tmp_path / "b")
    b = _load(tmp_path / "b")
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
