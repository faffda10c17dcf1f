"""GPU: a plain `bench.py --gpus 1 --steps K --warmup W` prints the headline line only -- metric, value, unit,
higher_is_better, dtype, ms_per_step and the step count it was given, none of the --full sections -- and with
--dump-outputs DIR leaves what the last timed step computed as float32 .npy files under 64 MB: the total loss, the loss
terms, and a gradient per trained parameter."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("kernels", "roofline", "roofline_gather", "roofline_gather_bwd", "dropin_msda", "msda_gpu",
             "cpu_baseline", "cpu_baseline_c_oracle")


@pytest.mark.gpu
def test_plain_bench_line_and_output_dump(tmp_path):
    out = str(tmp_path / "dump")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--videos-per-gpu", "4", "--steps", "3",
           "--warmup", "1", "--dump-outputs", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["unit"] == "videos/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["metric"].startswith("videos/sec fwd+bwd")
    assert line["ms_per_step"] > 0
    assert abs(line["value"] - 4 / (line["ms_per_step"] * 1e-3)) <= 1e-6 * line["value"]
    assert not [k for k in FULL_ONLY if k in line], "a plain run carries no --full section"
    files = sorted(glob.glob(os.path.join(out, "*.npy")))
    names = {os.path.basename(f)[:-4] for f in files}
    assert "loss_total" in names
    assert any(n.startswith("loss.") for n in names)
    grads = {n[5:] for n in names if n.startswith("grad.")}
    assert len(grads) > 100 and "query_embed.weight" in grads
    assert sum(os.path.getsize(f) for f in files) <= 64 * 2 ** 20
    for f in files:
        x = np.load(f)
        assert x.dtype == np.float32, f
        assert np.isfinite(x).all(), f
    assert float(np.load(os.path.join(out, "loss_total.npy"))[0]) > 0
