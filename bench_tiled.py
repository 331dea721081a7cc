"""Config C5: 2048x2048 RGB images filtered as overlap-save 256x256 windows (tiling.py) by the
10-stage G=32 image filter; one process per GPU, (image, window) units sharded over ranks -- whole
images first -- with no collective in the data path (--gather: rank 0 also receives every rank's
packed cores, each output pixel once).

    python bench_tiled.py [--images 2] [--size 2048] [--tile 256] [--halo 32] [--micro-batch 64]

Prints one JSON line: MPix/s of output image pixels (whole job), window overhead factor.

    python bench_tiled.py --image-api [--size 2048] [--tile 256] [--halo 32] [--micro-batch 64] [--steps 3]

compares, on one 8-bit size^2 RGB image and one GPU, (a) irdu_amd.restore_image with (b) the same windows
through host /255 + permute + upload, tiling.tiled_forward, clamp x255 round uint8 + permute + download:
wall time per image and torch.cuda.max_memory_allocated, the sides alternated and each run twice, then the
mean HIP-event time of the gather and scatter launches beside the float4 copy.  One JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def image_api(args):
    """restore_image (a) against host conversion + tiled_forward + ATen quantisation (b), see the module text."""
    import numpy as np
    import irdu_amd
    from irdu_amd import kernels, tiling
    from bench import TRAINED, build_model, synthetic_patches
    if args.gpus != 1:
        raise SystemExit("--image-api is a single-process comparison (--gpus 1)")
    dev = torch.device("cuda:0")
    irdu_amd.load_native()
    trained = os.path.exists(TRAINED)
    model = build_model(dev, trained=trained)
    _, noisy = synthetic_patches(1, seed=2204, h=args.size, w=args.size)
    img = (noisy[0].clamp(0, 1) * 255).round().to(torch.uint8).permute(1, 2, 0).contiguous().numpy()    # HWC uint8

    def side_a():
        return irdu_amd.restore_image(model, img, factor=16, tile=args.tile, halo=args.halo,
                                      micro_batch=args.micro_batch)

    def side_b():
        x = torch.from_numpy(img.astype(np.float32) / 255.0).permute(2, 0, 1).unsqueeze(0).to(dev)
        y = tiling.tiled_forward(model, x, tile=args.tile, halo=args.halo, align=16, micro_batch=args.micro_batch)
        return (y.clamp(0, 1) * 255).round().to(torch.uint8)[0].permute(1, 2, 0).cpu().numpy()

    def measure(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            out = fn()
        torch.cuda.synchronize()
        return {"ms_per_image": round((time.perf_counter() - t0) / args.steps * 1e3, 2),
                "max_memory_allocated_MiB": round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)}, out

    side_a(), side_b()                                           # warm-up
    runs = {"restore_image": [], "tiled_forward_route": []}
    for _ in range(2):                                           # alternated, each side twice
        ra, out_a = measure(side_a)
        rb, out_b = measure(side_b)
        runs["restore_image"].append(ra)
        runs["tiled_forward_route"].append(rb)
    diff = np.abs(out_a.astype(np.int16) - out_b.astype(np.int16))
    timer = kernels.LaunchTimer()
    kernels.set_timer(timer)
    for _ in range(args.steps):
        side_a()
    per_kernel = {k: {f: round(v[f], 4) for f in ("launches", "mean_ms", "bytes_per_launch", "gbps")}
                  for k, v in timer.summary().items() if k in ("tile_gather", "tile_scatter")}
    kernels.set_timer(None)
    n = 64 * 3 * 256 * 256
    src, dst = torch.rand(n, device=dev), torch.empty(n, device=dev)
    kernels.stream_copy(src, dst)
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(20):
        kernels.stream_copy(src, dst)
    e.record()
    torch.cuda.synchronize()
    copy_ms = s.elapsed_time(e) / 20
    print(json.dumps({"metric": "whole-image restoration, ms per image", "value": runs["restore_image"][-1]["ms_per_image"],
                      "unit": "ms", "n_gpus": 1,
                      "config": {"workload": f"{args.size}^2 RGB uint8, {args.tile}^2 windows, halo {args.halo}, "
                                             f"micro-batch {args.micro_batch}, G=32 F=3 S=10 image filter",
                                 "weights": "trained fixture" if trained else "reference init", "steps": args.steps},
                      "runs": runs, "outputs": {"levels_differing": int((diff > 0).sum()), "max_level_diff": int(diff.max())},
                      "per_kernel": per_kernel,
                      "float4_copy": {"floats": n, "mean_ms": round(copy_ms, 4),
                                      "gbps": round(8 * n / (copy_ms * 1e-3) / 1e9, 1)}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=2)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--tile", type=int, default=256)
    ap.add_argument("--halo", type=int, default=32)
    ap.add_argument("--micro-batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--gather", action="store_true")
    ap.add_argument("--gpus", type=int, default=1, help="ranks (one process per GPU; spawned when not under torchrun)")
    ap.add_argument("--dry-run", action="store_true", help="launcher check: ranks report and exit (no HIP)")
    ap.add_argument("--image-api", action="store_true",
                    help="compare restore_image with the tiled_forward route on one uint8 image (one GPU)")
    args = ap.parse_args()
    if args.image_api:
        return image_api(args)
    import benchlib
    world, rank, local = benchlib.join_or_spawn(args.gpus, dry_run=args.dry_run)
    if args.dry_run:
        benchlib.dry_run_report(world, rank, local)
        return
    dev = benchlib.init(world, local)
    ranks = benchlib.check_ranks(world, dev)     # every rank in the group, over the data backend
    import irdu_amd
    from irdu_amd import tiling
    from bench import TRAINED, build_model, synthetic_patches
    irdu_amd.load_native()
    trained = os.path.exists(TRAINED)
    model = build_model(dev, trained=trained)
    _, noisy = synthetic_patches(args.images, seed=2204, h=args.size, w=args.size)
    noisy = noisy.to(dev)
    run = lambda: tiling.tiled_forward(model, noisy, tile=args.tile, halo=args.halo, align=16,  # noqa: E731
                                       micro_batch=args.micro_batch, gather="rank0" if args.gather else "none")
    run()
    benchlib.barrier(world, dev)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        run()
    benchlib.barrier(world, dev)
    dt = benchlib.max_over_ranks(time.perf_counter() - t0, world, dev)
    nwin = len(tiling.tile_grid(args.size, args.size, args.tile, args.halo, 16))
    parity = None
    if world == 1:
        # tiled vs the whole image in one launch (image 0): the halo's effect on the output
        with torch.no_grad():
            tiled = run()[:1]
            whole = model(noisy[:1])
        ref = whole.abs().max().item()
        parity = {"image": "0 of the batch", "max_abs_err_vs_whole": (tiled - whole).abs().max().item(),
                  "rel_err_vs_whole": (tiled - whole).abs().max().item() / ref,
                  "weights": "trained fixture" if trained else "reference init"}
    if rank == 0:
        px = args.images * args.size * args.size * args.steps
        print(json.dumps({"metric": "tiled inference MPix/s (output pixels)", "value": round(px / dt / 1e6, 3),
                          "unit": "MPix/s", "n_gpus": world, "ms_per_step": round(dt / args.steps * 1e3, 2),
                          "config": {"workload": f"{args.images} x {args.size}^2 RGB, {args.tile}^2 windows, halo "
                                                 f"{args.halo}, G=32 F=3 S=10 image filter",
                                     "windows_per_image": nwin,
                                     "window_overhead": round(nwin * args.tile ** 2 / args.size ** 2, 3),
                                     "weights": "tests/golden/msgf_trained_g32_s10.safetensors" if trained
                                     else "reference init",
                                     "parallelism": f"(image, window) units sharded x{world}, "
                                                    + ("cores gathered to rank 0" if args.gather else "no collective")},
                          "tiled_vs_whole": parity, **(ranks if world > 1 else {})}), flush=True)
    benchlib.finish(world)


if __name__ == "__main__":
    main()
