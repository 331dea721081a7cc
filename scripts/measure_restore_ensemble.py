"""Measurements of the geometric self-ensemble of whole-image restoration, one process, one GPU.

    python scripts/measure_restore_ensemble.py [--size 2048] [--steps 3] [--out FILE.jsonl]

Workload: the C5 image filter (G = 32, S = 10, the trained fixture when it is there) on one size^2 RGB uint8
picture, at tile / halo / micro-batch 512 / 64 / 16 and 256 / 32 / 64.  One JSON line per tiling:
  (a) restore_image(ensemble=8) against the by-hand composition it replaces -- 8 x restore_image(quantise=False)
      on host-transformed copies (np.rot90 / np.flipud), the results turned back, torch.stack, mean, clamp and
      quantise on the device: ms per image and torch.cuda.max_memory_allocated, sides alternated, two repeats
      (after empty_cache each repeat makes one untimed call, so the timed steps do not pay for hipMalloc);
  (b) ensemble=8 over ensemble=1, same process, and over 8 plain calls back to back (as long a run as the
      ensemble's, since a 2 s run and a 0.1 s run need not see the same clocks);
  (c) HIP-event time, algorithmic bytes and GB/s per launch of tile_gather_d8 (even-k and odd-k calls apart),
      tile_scatter_mean, and of tile_gather / tile_scatter on the plain call's window batch;
and one line (d): evaluate() on training.SyntheticTestImages at sigma 25, ensemble 1 against 8.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def transform(a, m):
    t = np.rot90(a, m // 2)
    return np.ascontiguousarray(np.flipud(t) if m % 2 else t)


def inverse_t(t, m):
    t = torch.flip(t, (0,)) if m % 2 else t
    return torch.rot90(t, -(m // 2), (0, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    import irdu_amd
    from irdu_amd import kernels, training
    from bench import TRAINED, build_model, synthetic_patches
    dev = torch.device("cuda:0")
    irdu_amd.load_native()
    trained = os.path.exists(TRAINED)
    model = build_model(dev, trained=trained)
    _, noisy = synthetic_patches(1, seed=2204, h=args.size, w=args.size)
    img = (noisy[0].clamp(0, 1) * 255).round().to(torch.uint8).permute(1, 2, 0).contiguous().numpy()
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    def measure(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        fn()                                                         # untimed: fills the caching allocator
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            out = fn()
        torch.cuda.synchronize()
        return {"ms_per_image": round((time.perf_counter() - t0) / args.steps * 1e3, 2),
                "max_memory_allocated_MiB": round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)}, out

    def per_launch(records):
        torch.cuda.synchronize()
        ms = [s.elapsed_time(e) for s, e, _, _ in records]
        nbytes = [b for _, _, b, _ in records]
        mean_ms, mean_b = float(np.mean(ms)), float(np.mean(nbytes))
        return {"launches": len(ms), "mean_us": round(mean_ms * 1e3, 2), "MB_per_launch": round(mean_b / 1e6, 2),
                "gbps": round(mean_b / (mean_ms * 1e-3) / 1e9, 1)}

    for tile, halo, mb in ((512, 64, 16), (256, 32, 64)):
        tiling = dict(factor=16, tile=tile, halo=halo, micro_batch=mb)

        def side_a():
            return irdu_amd.restore_image(model, img, ensemble=8, **tiling)

        def side_b():
            zs = []
            for m in range(8):
                y = irdu_amd.restore_image(model, torch.from_numpy(transform(img, m)).to(dev), quantise=False, **tiling)
                zs.append(inverse_t(y, m))
            mean = torch.stack(zs).mean(0)
            return (mean.clamp(0, 1) * 255).round().to(torch.uint8).cpu().numpy()

        def plain():
            return irdu_amd.restore_image(model, img, **tiling)

        def plain_x8():
            for _ in range(8):
                out = plain()
            return out

        side_a(), side_b(), plain()                                  # warm-up
        runs = {"ensemble_8": [], "by_hand": [], "ensemble_1": [], "ensemble_1_x8": []}
        for _ in range(2):                                           # alternated, each side twice
            ra, out_a = measure(side_a)
            rb, out_b = measure(side_b)
            r1, _ = measure(plain)
            r8, _ = measure(plain_x8)
            runs["ensemble_1_x8"].append(r8)
            runs["ensemble_8"].append(ra)
            runs["by_hand"].append(rb)
            runs["ensemble_1"].append(r1)
        diff = np.abs(out_a.astype(np.int16) - out_b.astype(np.int16))
        a_ms = [r["ms_per_image"] for r in runs["ensemble_8"]]
        b_ms = [r["ms_per_image"] for r in runs["by_hand"]]
        p_ms = [r["ms_per_image"] for r in runs["ensemble_1"]]
        p8_ms = [r["ms_per_image"] for r in runs["ensemble_1_x8"]]
        timer = kernels.LaunchTimer()
        kernels.set_timer(timer)
        for _ in range(args.steps):
            side_a()
            plain()
        kernels.set_timer(None)
        d8 = timer.records["tile_gather_d8"]                         # per group: the even-k call, then the odd-k call
        launches = {"tile_gather_d8_even": per_launch(d8[0::2]), "tile_gather_d8_odd": per_launch(d8[1::2]),
                    "tile_scatter_mean": per_launch(timer.records["tile_scatter_mean"]),
                    "tile_gather": per_launch(timer.records["tile_gather"]),
                    "tile_scatter": per_launch(timer.records["tile_scatter"])}
        emit({"metric": "restore_image(ensemble=8), ms per image", "value": a_ms[-1], "unit": "ms", "n_gpus": 1,
              "config": {"workload": f"{args.size}^2 RGB uint8, tile {tile}, halo {halo}, micro-batch {mb}, "
                                     "G=32 F=3 S=10 image filter",
                         "weights": "trained fixture" if trained else "reference init", "steps": args.steps},
              "runs": runs,
              "a_not_slower_than_b": bool(max(a_ms) <= min(b_ms)),
              "b_over_a": round(min(b_ms) / max(a_ms), 4),
              "ensemble_8_over_1": round(float(np.mean(a_ms)) / float(np.mean(p_ms)), 3),
              "ensemble_8_over_8_plain_calls": round(float(np.mean(a_ms)) / float(np.mean(p8_ms)), 3),
              "a_vs_b_levels_differing": int((diff > 0).sum()), "a_vs_b_max_level_diff": int(diff.max()),
              "per_launch": launches})

    images = training.SyntheticTestImages()
    res = {}
    for ensemble in (1, 8):
        t0 = time.perf_counter()
        mean, per_image = irdu_amd.evaluate(model, images, sigma=25.0, ensemble=ensemble, device=dev)
        torch.cuda.synchronize()
        res[f"ensemble_{ensemble}"] = {"mean_psnr_dB": round(mean, 4), "per_image_dB": [round(p, 4) for p in per_image],
                                       "seconds": round(time.perf_counter() - t0, 3)}
    emit({"metric": "evaluate on SyntheticTestImages, sigma 25, mean PSNR", "unit": "dB",
          "value": res["ensemble_8"]["mean_psnr_dB"], "n_images": len(images),
          "weights": "trained fixture" if trained else "reference init", **res})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
