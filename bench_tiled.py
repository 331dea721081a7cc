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

    python bench_tiled.py --image-list 68 [--image-list-size 321 481] [--yaml CONF.yaml] [--tile 256] [--halo 32]
                          [--micro-batch 64]

times, on one GPU, irdu_amd.evaluate over N synthetic 8-bit RGB images (half H x W, half W x H: CBSD68's two
shapes by default) as the per-image loop (across_images=False) against shared window batches
(across_images=True), same model, both sides synchronised, alternated, each twice.  The model is the image
filter of the other modes, or --yaml's model: section with its initial weights.  One JSON line: seconds per
list and images per second on each side, model calls on each side, whether restore_images' bytes equal the
per-image restore_image's and whether the PSNRs are equal; and, since evaluate() draws its noise on the host
inside the timed call, that draw's time and the two restore calls alone on the drawn images.
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


def image_list(args):
    """evaluate(across_images=False) against evaluate(across_images=True) on a list of images, see the module text."""
    import numpy as np
    import irdu_amd
    from irdu_amd import training
    from bench import TRAINED, build_model
    if args.gpus != 1:
        raise SystemExit("--image-list is a single-process comparison (--gpus 1)")
    dev = torch.device("cuda:0")
    irdu_amd.load_native()
    if args.yaml:
        torch.manual_seed(2204)
        model = training.build_model(training.parse_options(args.yaml).get("model", {})).to(dev).eval()
        what, weights = f"model: section of {os.path.basename(args.yaml)}", "initial"
    else:
        trained = os.path.exists(TRAINED)
        model = build_model(dev, trained=trained)
        what, weights = "G=32 F=3 S=10 image filter", "trained fixture" if trained else "reference init"
    h, w = args.image_list_size
    n = args.image_list
    shapes = [(h, w) if i < (n + 1) // 2 else (w, h) for i in range(n)]
    images = [training.synthetic_clean_patch(np.random.RandomState(68 * 7919 + i), sh, sw, 3)     # on the uint8 grid
              for i, (sh, sw) in enumerate(shapes)]
    tiling_args = dict(tile=args.tile, halo=args.halo, micro_batch=args.micro_batch)
    calls = []
    hook = model.register_forward_pre_hook(lambda mod, a: calls.append(int(a[0].shape[0])))

    def run(across):
        del calls[:]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        result = irdu_amd.evaluate(model, images, sigma=25.0, factor=16, seed=2204, across_images=across, **tiling_args)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, result, len(calls), max(calls)

    # warm-up, and the byte comparison: the same noisy images through both calls.  evaluate() also draws the
    # noise on the host, the same work on both sides: that time, and the two calls alone, are reported too
    rs = np.random.RandomState(2204)
    t0 = time.perf_counter()
    noisy = []
    for im in images:
        x = im.copy()
        x += rs.normal(0, 25.0 / 255.0, im.shape)
        noisy.append(x)
    noise_s = time.perf_counter() - t0

    def restore_only(across):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if across:
            out = irdu_amd.restore_images(model, noisy, factor=16, **tiling_args)
        else:
            out = [irdu_amd.restore_image(model, x, factor=16, **tiling_args) for x in noisy]
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    _, one_by_one = restore_only(False)
    _, together = restore_only(True)
    byte_equal = all(np.array_equal(a, b) for a, b in zip(one_by_one, together))
    differing = int(sum(int((a != b).sum()) for a, b in zip(one_by_one, together)))
    restore_runs = {"loop": [], "across_images": []}
    for _ in range(2):
        restore_runs["loop"].append(round(restore_only(False)[0], 4))
        restore_runs["across_images"].append(round(restore_only(True)[0], 4))
    runs = {"loop": [], "across_images": []}
    for _ in range(2):                                           # alternated, each side twice
        t_loop, res_loop, calls_loop, max_loop = run(False)
        t_across, res_across, calls_across, max_across = run(True)
        runs["loop"].append(round(t_loop, 4))
        runs["across_images"].append(round(t_across, 4))
    hook.remove()
    best = {k: min(v) for k, v in runs.items()}
    print(json.dumps({"metric": "evaluate over an image list, seconds per list", "value": best["across_images"],
                      "unit": "s", "n_gpus": 1,
                      "config": {"workload": f"{n} RGB images, {(n + 1) // 2} of {h}x{w} and {n // 2} of {w}x{h}, sigma 25, "
                                             f"tile {args.tile}, halo {args.halo}, micro-batch {args.micro_batch}",
                                 "model": what, "weights": weights,
                                 "native_convs": bool(irdu_amd.graph_filter.NATIVE_CONVS)},
                      "seconds_per_list": runs,
                      "images_per_s": {k: round(n / v, 2) for k, v in best.items()},
                      "ms_per_image": {k: round(v / n * 1e3, 2) for k, v in best.items()},
                      "host_noise_draw_s": round(noise_s, 4),
                      "restore_only_seconds_per_list": restore_runs,
                      "restore_only_ms_per_image": {k: round(min(v) / n * 1e3, 2) for k, v in restore_runs.items()},
                      "model_calls": {"loop": calls_loop, "across_images": calls_across},
                      "largest_batch": {"loop": max_loop, "across_images": max_across},
                      "outputs_byte_equal": byte_equal, "bytes_differing": differing,
                      "psnr_equal": res_loop == res_across, "mean_psnr": round(res_loop[0], 4)}), flush=True)


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
    ap.add_argument("--image-list", type=int, nargs="?", const=68, default=None, metavar="N",
                    help="time evaluate() over N images as a per-image loop against shared window batches (one GPU)")
    ap.add_argument("--image-list-size", type=int, nargs=2, default=[321, 481], metavar=("H", "W"))
    ap.add_argument("--yaml", type=str, default=None, help="--image-list: build the model from this YAML's model: section")
    args = ap.parse_args()
    if args.image_api:
        return image_api(args)
    if args.image_list is not None:
        if args.image_list < 1:
            raise SystemExit("--image-list needs at least one image")
        return image_list(args)
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
