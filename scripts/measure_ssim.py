"""Measurements of the SSIM kernel (csrc/metric_ops.hip), one process, one GPU.

    python scripts/measure_ssim.py [--steps 20] [--peak-binary PATH] [--out profiles/restore/ssim_FILE.jsonl]

Workloads: 68 RGB images, 34 of 321 x 481 and 34 of 481 x 321 (bench_tiled.py --image-list 68), in one arena, the
restored side a noisy copy of the clean side; and one 2048 x 2048 x 3 pair.  One JSON line per workload:
  u8_ssim_images   HIP-event time per launch (kernels.LaunchTimer: the zeroing memset and the kernel), after
                   warm-up launches, mean and minimum over --steps
  u8_sse_segments  the same for the PSNR's sum on the same arenas: the bandwidth-bound yardstick
  fma_rate         110 float64 FMAs per value (55 horizontal, 55 vertical) over the kernel time, the bytes read
                   (both arenas once), and the share of the float64 FMA ceiling
and, for the 68 images, evaluate_metrics(across_images=True) with and without "ssim" (host clock around a device
synchronise, alternated, two repeats each) beside the time of the model calls alone (HIP events around each).
The ceiling is measured here: scripts/fp64_fma_peak.hip, built with hipcc unless --peak-binary names a build of it.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FMAS_PER_VALUE = 110


def fma_ceiling(binary):
    """TFMA/s from scripts/fp64_fma_peak.hip, in a child process of its own."""
    if binary is None:
        binary = os.path.join(tempfile.mkdtemp(prefix="fp64_peak_"), "fp64_fma_peak")
        hipcc = next(c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc") if c)
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", os.path.join(ROOT, "scripts", "fp64_fma_peak.hip"), "-o",
                        binary], check=True, timeout=600)
    out = subprocess.run([binary], check=True, capture_output=True, text=True, timeout=120).stdout
    return json.loads(out.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--peak-binary", type=str, default=None)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_ssim.py needs a GPU")
    import irdu_amd
    from irdu_amd import kernels, restore, training
    from bench import TRAINED, build_model
    dev = torch.device("cuda:0")
    irdu_amd.load_native()
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    peak = fma_ceiling(args.peak_binary)        # before this process fills the GPU
    emit(peak)

    def per_launch(records):
        torch.cuda.synchronize()
        ms = [s.elapsed_time(e) for s, e, _, _ in records]
        return {"launches": len(ms), "mean_us": round(float(np.mean(ms)) * 1e3, 2), "min_us": round(min(ms) * 1e3, 2)}

    def kernel_times(pa, pb):
        offsets = [off for off, _, _ in pa.host_table] + [pa.arena.numel()]
        for _ in range(3):                                          # warm-up
            qs = kernels.u8_ssim_images(pa, pb)
            kernels.u8_sse_segments(pa.arena, pb.arena, offsets)
        timer = kernels.LaunchTimer()
        kernels.set_timer(timer)
        for _ in range(args.steps):                                 # alternated
            assert kernels.u8_ssim_images(pa, pb) == qs
            kernels.u8_sse_segments(pa.arena, pb.arena, offsets)
        kernels.set_timer(None)
        ssim, sse = per_launch(timer.records["u8_ssim_images"]), per_launch(timer.records["u8_sse_segments"])
        values = sum(kernels.ssim_count(pa.c, h, w) for _, h, w in pa.host_table)
        nbytes = 2 * pa.arena.numel()
        rate = values * FMAS_PER_VALUE / (ssim["min_us"] * 1e-6) / 1e12
        return {"u8_ssim_images": ssim, "u8_sse_segments": sse, "values": values, "bytes_read": nbytes,
                "ssim_over_sse": round(ssim["min_us"] / sse["min_us"], 2),
                "fma_rate": {"TFMA_per_s": round(rate, 3), "GB_per_s": round(nbytes / (ssim["min_us"] * 1e-6) / 1e9, 1),
                             "share_of_measured_fp64_ceiling": round(rate / peak["value"], 3)},
                "mean_ssim": round(float(np.mean([restore._ssim(q, kernels.ssim_count(pa.c, h, w))
                                                  for q, (_, h, w) in zip(qs, pa.host_table)])), 6)}

    def noisy_u8(clean, seed):
        rs = np.random.RandomState(seed)
        return np.clip(np.rint(clean.astype(np.float64) + rs.normal(0, 25.0, clean.shape)), 0, 255).astype(np.uint8)

    # 68 images in one arena
    n, h, w = 68, 321, 481
    shapes = [(h, w) if i < (n + 1) // 2 else (w, h) for i in range(n)]
    cleans = [training.synthetic_clean_patch(np.random.RandomState(68 * 7919 + i), sh, sw, 3) for i, (sh, sw) in enumerate(shapes)]
    clean_u8 = [restore._clean_u8(c) for c in cleans]
    pa = irdu_amd.pack_images([noisy_u8(c, i) for i, c in enumerate(clean_u8)], dev)
    pb = irdu_amd.pack_images(clean_u8, dev)
    row = {"metric": "u8_ssim_images, us per launch (min)", "unit": "us", "n_gpus": 1,
           "config": {"workload": f"{n} RGB uint8 images, {(n + 1) // 2} of {h}x{w} and {n // 2} of {w}x{h}, one arena",
                      "steps": args.steps, "tile": list(kernels.SSIM_TILE)}}
    row.update(kernel_times(pa, pb))
    row["value"] = row["u8_ssim_images"]["min_us"]

    # the whole evaluation, with and without "ssim", and the model calls alone
    trained = os.path.exists(TRAINED)
    model = build_model(dev, trained=trained)
    model.eval()

    class Timed:
        """The model with HIP events around each call."""
        def __init__(self):
            self.events = []
            self.parameters = model.parameters

        def __call__(self, x):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            y = model(x)
            e.record()
            self.events.append((s, e))
            return y

    timed = Timed()

    def run(metrics):
        del timed.events[:]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = irdu_amd.evaluate_metrics(timed, cleans, sigma=25.0, across_images=True, metrics=metrics, device=dev)
        torch.cuda.synchronize()
        sec = time.perf_counter() - t0
        return sec, sum(s.elapsed_time(e) for s, e in timed.events) * 1e-3, res

    run(("psnr", "ssim"))                                           # warm-up
    runs = {"psnr": [], "psnr+ssim": [], "model_calls": []}
    for _ in range(2):
        t_p, m_p, res_p = run(("psnr",))
        t_b, m_b, res_b = run(("psnr", "ssim"))
        assert res_p["psnr"] == res_b["psnr"]
        runs["psnr"].append(round(t_p, 4))
        runs["psnr+ssim"].append(round(t_b, 4))
        runs["model_calls"] += [round(m_p, 4), round(m_b, 4)]
    row["evaluate_metrics_across_images_s"] = runs
    row["ssim_adds_s"] = round(min(runs["psnr+ssim"]) - min(runs["psnr"]), 4)
    row["model_calls_s"] = min(runs["model_calls"])
    row["ssim_costs_less_than_the_model_calls"] = bool(row["ssim_adds_s"] < row["model_calls_s"])
    row["model"] = {"what": "G=32 F=3 S=10 image filter", "weights": "trained fixture" if trained else "reference init",
                    "mean_psnr_dB": round(res_b["psnr"][0], 4), "mean_ssim": round(res_b["ssim"][0], 6)}
    emit(row)

    # one large pair
    size = 2048
    big = restore._clean_u8(training.synthetic_clean_patch(np.random.RandomState(5), size, size, 3))
    pa = irdu_amd.pack_images([noisy_u8(big, 99)], dev)
    pb = irdu_amd.pack_images([big], dev)
    row = {"metric": "u8_ssim_images, us per launch (min)", "unit": "us", "n_gpus": 1,
           "config": {"workload": f"one {size}x{size}x3 uint8 pair", "steps": args.steps, "tile": list(kernels.SSIM_TILE)}}
    row.update(kernel_times(pa, pb))
    row["value"] = row["u8_ssim_images"]["min_us"]
    single = kernels.u8_ssim(pa.image(0), pb.image(0))
    row["single_image_call_equal"] = bool([single] == kernels.u8_ssim_images(pa, pb))
    emit(row)

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
