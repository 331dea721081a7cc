"""bench.py, plain run: the result line carries the headline fields and nothing that needs a run of
its own (those sit behind --full), and --dump-outputs DIR writes what the last timed step returned.
The bench's inputs and weights are seeded, so the same forward in this process must give the dumped
array bit for bit (the kernels are deterministic: tests/test_gpu_deterministic.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.test_gpu_parity import DEV

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("roofline", "roofline_secondary", "kernel_ms_per_step", "secondary_workload", "cpu_baseline", "psnr",
             "speedup_vs_cpu")


def test_plain_run_line_and_dumped_output(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    batch, steps = 2, 3
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "1", "--batch", str(batch), "--dump-outputs", str(tmp_path / "dump")],
                       cwd=ROOT, capture_output=True, text=True, timeout=170)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = lines[0]
    assert d["unit"] == "MPix/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["steps"] == steps and d["ms_per_step"] > 0
    # value and ms_per_step describe the same timed loop: steps x batch x 256 x 256 pixels in steps x ms_per_step
    assert d["value"] == pytest.approx(batch * 256 * 256 / (d["ms_per_step"] * 1e-3) / 1e6, rel=1e-3)
    assert not [k for k in FULL_ONLY if k in d]

    assert sorted(os.listdir(tmp_path / "dump")) == ["denoised.npy"]
    got = np.load(tmp_path / "dump" / "denoised.npy")
    assert got.dtype == np.float32 and got.shape == (batch, 3, 256, 256)

    import bench
    import irdu_amd
    irdu_amd.load_native()
    model = bench.build_model(DEV, trained=os.path.exists(bench.TRAINED))
    _, noisy = bench.synthetic_patches(batch, seed=2204)
    with torch.no_grad():
        want = model(noisy.to(DEV)).float().cpu().numpy()
    assert np.array_equal(got, want)
