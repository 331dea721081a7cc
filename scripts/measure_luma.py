"""Measurements of the luma kernels (csrc/metric_ops.hip) beside their RGB counterparts, one process,
one GPU.

    python scripts/measure_luma.py [--steps 20] [--size 2048] [--out profiles/restore/luma_FILE.jsonl]

Workload: one SIZE x SIZE x 3 uint8 pair, the restored side a noisy copy of the clean side.  HIP-event time per launch
(kernels.LaunchTimer: the zeroing memset and the kernel), 3 warm-up launches, then --steps launches of u8_luma_ssim,
u8_ssim, u8_luma_sse and u8_sse alternated on the same two images; one JSON line with mean and minimum of each and
the two ratios.  Every timed result is compared with the warm-up's.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_luma.py needs a GPU")
    import irdu_amd
    from irdu_amd import kernels, restore, training
    dev = torch.device("cuda:0")
    irdu_amd.load_native()

    size = args.size
    clean = restore._clean_u8(training.synthetic_clean_patch(np.random.RandomState(5), size, size, 3))
    rs = np.random.RandomState(99)
    noisy = np.clip(np.rint(clean.astype(np.float64) + rs.normal(0, 25.0, clean.shape)), 0, 255).astype(np.uint8)
    a, b = torch.from_numpy(noisy).to(dev), torch.from_numpy(clean).to(dev)
    calls = {"u8_luma_ssim": kernels.u8_luma_ssim, "u8_ssim": kernels.u8_ssim, "u8_luma_sse": kernels.u8_luma_sse,
             "u8_sse": kernels.u8_sse}
    for _ in range(3):                                              # warm-up
        first = {name: fn(a, b) for name, fn in calls.items()}
    timer = kernels.LaunchTimer()
    kernels.set_timer(timer)
    for _ in range(args.steps):                                     # alternated
        for name, fn in calls.items():
            assert fn(a, b) == first[name], name
    kernels.set_timer(None)
    torch.cuda.synchronize()
    row = {"metric": "u8_luma_ssim, us per launch (min)", "unit": "us", "n_gpus": 1,
           "config": {"workload": f"one {size}x{size}x3 uint8 pair", "steps": args.steps,
                      "luma_ssim_tile": list(kernels.LUMA_SSIM_TILE), "luma_sse_block": list(kernels.LUMA_SSE_BLOCK)},
           "bytes_read": 2 * a.numel()}
    for name in calls:
        ms = [s.elapsed_time(e) for s, e, _, _ in timer.records[name]]
        row[name] = {"launches": len(ms), "mean_us": round(float(np.mean(ms)) * 1e3, 2), "min_us": round(min(ms) * 1e3, 2)}
    row["value"] = row["u8_luma_ssim"]["min_us"]
    row["luma_ssim_over_ssim"] = round(row["u8_luma_ssim"]["min_us"] / row["u8_ssim"]["min_us"], 3)
    row["luma_sse_over_sse"] = round(row["u8_luma_sse"]["min_us"] / row["u8_sse"]["min_us"], 3)
    row["psnr_y_dB"] = round(restore._psnr_y(first["u8_luma_sse"], size * size), 4)
    row["ssim_y"] = round(restore._ssim(first["u8_luma_ssim"], kernels.luma_ssim_count(size, size)), 6)
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
