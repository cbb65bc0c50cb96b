"""GPU: bench.py --dump-outputs -- two runs with the same arguments write the same outputs (the last timed step starts
from the seeded initial state: what the steps before it leave differs from run to run, see bench.py's docstring)."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(out_dir, steps, warmup):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", str(warmup), "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    return lines[0]


def test_dumped_outputs_are_the_same_on_every_run(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    la, lb = _run(a, 6, 3), _run(b, 6, 3)
    assert la["steps"] == lb["steps"] == 6 and la["ms_per_step"] > 0
    names = sorted(os.path.basename(f) for f in glob.glob(str(a / "*.npy")))
    assert names == sorted(os.path.basename(f) for f in glob.glob(str(b / "*.npy")))
    for n in ("total_loss.npy", "xyz_recon.npy", "rot_pred.npy", "trans_pred.npy", "input_pc.npy"):
        assert n in names
    assert sum(os.path.getsize(str(a / n)) for n in names) < 64 * 10 ** 6
    for n in names:
        x, y = np.load(str(a / n)), np.load(str(b / n))
        assert x.dtype in (np.float32, np.float64) and x.shape == y.shape, n
        assert np.array_equal(x, y, equal_nan=True), n
    assert la["config"]["final_total_loss"] == lb["config"]["final_total_loss"]
