"""bench.py's plain run on the GPU: the result line, --steps as the number of timed steps, and --dump-outputs giving the
same arrays from run to run (what lets two builds be compared output for output)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir, *args):
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(ROOT, "bench.py"), "--gpus", "1",
                                                                           "--dump-outputs", str(out_dir), *args]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
@pytest.mark.parametrize("workload,batch,names", [
    ("ieee123_b8192", 256, ["obs", "reward", "terminated", "truncated", "power_flow_converged", "iterations", "episode_reward"]),
    ("ieee8500_3ph_b1024", 8, ["voltages_re", "voltages_im", "converged", "iterations", "losses", "max_mismatch"])])
def test_plain_run_line_and_reproducible_outputs(tmp_path, workload, batch, names):
    lines = [_bench(tmp_path / d, "--workload", workload, "--batch", str(batch), "--steps", "7", "--warmup", "3") for d in ("a", "b")]
    for r in lines:
        assert r["steps"] == 7 and r["warmup"] == 3 and r["ms_per_step"] > 0 and r["value"] > 0 and r["higher_is_better"] is True
        assert r["dtype"] == "f64" and r["unit"] and r["metric"]
        assert not any(k in r for k in ("regions", "also", "accuracy", "cpu_baseline_1core", "rollout"))      # --full only
    for k in names:
        a, b = np.load(tmp_path / "a" / (k + ".npy")), np.load(tmp_path / "b" / (k + ".npy"))
        assert a.dtype == np.float64 and a.shape[0] == batch and np.array_equal(a, b), k
    conv = "power_flow_converged" if "power_flow_converged" in names else "converged"
    assert np.all(np.load(tmp_path / "a" / (conv + ".npy")) == 1)
