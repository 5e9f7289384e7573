"""bench.py's plain run: the headline line only (no parity gate, baselines or other configurations; those come with --full), and
--dump-outputs writes what the timed path returned in its last pass - here checked against the reference-made fixture of the metric fan."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from parity import compare_compact

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    out = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    lines = [l for l in r.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, "exactly ONE JSON line"
    d = json.loads(lines[0])
    print("plain bench:", d["value"], d["unit"], d["ms_per_step"], "ms per step")
    assert d["steps"] == 2 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["unit"] == "RK4 ray-steps/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["config"]["ray_steps_per_pass"] == 874273730
    assert not {"parity_gate", "roofline", "launch_only", "other_scalings", "cpu_baseline"} & set(d)
    assert sorted(os.listdir(out)) == ["ray_steps.npy", "records.npy"]
    rec, steps = np.load(out / "records.npy"), np.load(out / "ray_steps.npy")
    assert rec.dtype == np.float64 and rec.shape == (32400, 3, 32)
    assert steps.dtype == np.float64 and steps.tolist() == [874273730.0]
    g = np.load(os.path.join(ROOT, "tests", "golden", "full_metric.npz"))
    compare_compact(rec, g, idx=np.arange(32400))                   # every ray of the last timed pass: counts exact, values to 1e-6
