"""bench.py on one GPU, in both forms: a plain run prints the headline line and nothing that needs a run of its own; ``--full``
(trimmed to what a test can afford: no CPU baseline, a short sustained region) adds the box calibration, the step fed from pinned
host memory, the sustained region and the per-kernel tables."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("box_calibration", "sustained", "roofline", "roofline_next", "roofline_hbm", "kernel_time_us", "cpu_baseline")


def _bench(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1"] + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_alone():
    out = _bench()
    assert out["metric"] == "images/sec U-Net/ResNet34 512x512 bs16 training step" and out["unit"] == "images/sec"
    assert out["higher_is_better"] is True and out["dtype"] == "bf16" and out["n_gpus"] == 1
    assert out["steps"] == 3 and out["warmup"] == 1 and out["value"] > 0
    assert abs(out["value"] * out["ms_per_step"] - 16e3) < 16e3 * 1e-3          # images/s = batch 16 / step time
    assert out["ms_per_step_resident"] == out["ms_per_step"] and out["step_mfma_frac"] > 0
    assert not set(FULL_ONLY) & set(out), sorted(set(FULL_ONLY) & set(out))
    assert out["ms_per_step_with_feed"] is None and out["ms_per_step_without_augmentation"] is None
    assert "dice_delta_vs_oracle" not in out["config"]


def test_full_run_adds_the_other_regions():
    out = _bench("--full", "--no-cpu-baseline", "--sustain", "0.5")
    assert out["steps"] == 3 and out["value"] > 0 and out["dtype"] == "bf16"
    assert out["box_calibration"]["mfma_tflops"] > 0 and out["box_calibration"]["copy_gbs"] > 0
    assert out["ms_per_step_with_feed"] > 0 and out["value_with_feed"] > 0
    assert out["sustained"]["steps"] >= 200 and out["sustained"]["ms_per_step"] > 0
    assert out["roofline"]["bound"] == "mfma" and out["roofline"]["achieved"] > 0 and len(out["roofline_next"]) == 3
    assert out["roofline_hbm"]["bound"] == "hbm" and out["kernel_time_us"]
    assert "cpu_baseline" not in out and "dice_delta_vs_oracle" not in out["config"]       # (--no-cpu-baseline)
