r"""``bench.py`` as a command on one GPU: a plain run prints the headline line and nothing that takes runs of its own;
``--full`` adds the roofline / per-kernel figures and the other arithmetic modes to the same line."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "roofline_kernels", "roofline_hbm_kernels", "roofline_transition", "step_breakdown", "cpu_baseline",
             "speedup_vs_cpu", "native_fp32_mfma", "bf16x3_mode", "f16x2_mode")


def run_bench(*extra):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "tiny", "--steps", "2",
                          "--warmup", "1", *extra], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_only(tmp_path):
    out = run_bench("--dump-outputs", str(tmp_path))
    assert all(k in out for k in HEADLINE), sorted(out)
    assert out["value"] > 0 and out["ms_per_step"] > 0 and out["higher_is_better"] is True
    assert out["steps"] == 2 and out["warmup"] == 1 and out["n_gpus"] == 1
    assert not [k for k in FULL_ONLY if k in out]
    x0 = np.load(tmp_path / "x0.npy")
    assert x0.shape == (2, 3, 64, 64) and x0.dtype == np.float32 and np.isfinite(x0).all()


def test_full_run_adds_the_rest():
    out = run_bench("--full", "--no-pmc", "--no-cpu-baseline")
    assert all(k in out for k in HEADLINE), sorted(out)
    assert out["roofline"]["achieved"] > 0 and out["roofline_kernels"] and out["roofline_transition"]["achieved"] > 0
    # the two arithmetic modes beside the one that was timed (none beside a native-mode run), each with its difference to the timed x0
    others = [k for k in ("native_fp32_mfma", "bf16x3_mode", "f16x2_mode") if k in out]
    assert len(others) == (0 if out["dtype"] == "f32" else 2), sorted(out)
    assert all(out[k]["value"] > 0 and out[k]["max_abs_difference_of_x0"] < 1e-2 for k in others)
    assert "cpu_baseline" not in out
