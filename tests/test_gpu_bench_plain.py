"""GPU (-m gpu): a plain `bench.py` run (no `--full`) prints the headline line and writes `--dump-outputs`, and runs none of the
untimed legs: no per-stage step, no stream check, no PCIe-inclusive, two-session or 2160p runs, no libx265 or CPU baseline.
The `--full` line is covered by tests/test_gpu_fullsize.py::test_config4_bench_two_ranks_share_device_0."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]

FULL_ONLY = ("stream_check", "stages_ms_per_picture", "roofline", "pipeline", "value_pcie_inclusive", "value_pcie_inclusive_pinned",
             "value_two_sessions", "value_one_clip_two_sessions", "configs", "libx265", "cpu_baseline")


def test_plain_run_prints_the_headline_only(tmp_path):
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "0", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["unit"] == "frames/s" and out["higher_is_better"] is True and out["dtype"] == "u8" and out["steps"] == 1
    assert abs(out["value"] - 300 / (out["ms_per_step"] / 1e3)) / out["value"] < 0.01
    assert out["stream_ok"] is None and out["quality"]["psnr_y_db"] > 30
    assert not [k for k in FULL_ONLY if k in out], out.keys()
    stats = np.load(tmp_path / "stats.npy")
    assert stats[1] == 300 and len(np.load(tmp_path / "packet_sizes.npy")) == 300        # frames_out, one packet per picture
