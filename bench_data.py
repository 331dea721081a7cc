"""Batches per second of the two ways to feed training from pictures on disk (no model runs):

  host    training.ImageSuperResolution under torch's DataLoader (num_workers=4, the reference's setting), each
          batch then sent to the GPU and made planar as Trainer.step does
  device  training.DevicePatchLoader: the pictures decoded once into an arena on the GPU, one kernels.patch_batch
          call per batch (the one-off decode + pack is reported apart)

at the four shapes of the v2 curriculum (128^2 x 4, 192^2 x 3, 256^2 x 2, 384^2 x 1) and at C4's 32 x 512^2, on
synthetic PNGs written to a temporary folder, and then the device loader alone on a file count like a training
set's (8600 small pictures), where a host cost per batch that grew with the number of files would show.  Prints
one JSON line per shape and one for the many-files run.

With --paired both paths read training.PairedImageRestoration (dist_mode "none") over degraded / clean file pairs:
the host path decodes two files per sample, the device loader holds two arenas and makes each batch with one
kernels.patch_pair_batch call.  The same JSON line per shape ("bench": "data_paired", arena_mb counting both
arenas); the many-files run is the unpaired loader's and is left out.

With --pair-kernel only the two kernels are timed, in one process on one shape (B = 64, C = 3, 128^2, all eight
modes, random origins in 8 pictures of 512^2): grr_patch_pair_batch without sigma against grr_patch_batch at
sigma 25/255, device events around runs of 200 launches on preallocated outputs, the two alternating, 15 rounds.
One JSON line ("bench": "pair_kernel") with each kernel's median, fastest and slowest round in microseconds per
launch.

With --bicubic S only the synthesis of a bicubic super-resolution training set's degraded pictures is timed, on the
same synthetic pictures held in memory (no files, no model): "device" is kernels.u8_bicubic_degrade_images on the clean
arena (two launches: down into a low-resolution arena, up into the degraded one), device events around each of 20
rounds after a warm-up; "host" is the alternative the loader would otherwise run serially as it decodes, Pillow's
resize(BICUBIC) down and back up of every picture, one wall-clock pass.  One JSON line ("bench": "bicubic") with both,
the two kernels' algorithmic bytes (each input byte read once, each output byte written once) over the device time,
and grr_stream_copy's rate on a buffer of the arena's size in the same process for scale.

With --jpeg Q only the synthesis of a JPEG artifact-removal training set's degraded pictures is timed, on the same
pictures and by the same method: "device" is kernels.u8_jpeg_images on the clean arena (one launch) for gray (the
pictures' first channel), 4:4:4 and 4:2:0, device events around each of 20 calls after a warm-up; "host" is one serial
pass of Pillow's save(format="JPEG", quality=Q) and open of every picture; grr_stream_copy is timed in the same
process.  One JSON line ("bench": "jpeg") with, per mode, the times, the algorithmic GB/s (each byte in once, each
byte out once) and the kernel / copy time ratio at equal bytes, then one ("bench": "blocking") with
kernels.u8_blocking against kernels.u8_sse on one 2048 x 2048 x 3 picture, host clock around calls that end in the
sums' device-to-host copy.

With --demosaic PATTERN only the synthesis of a demosaicking training set's filled mosaics is timed, on the same
pictures and by the same method: "device" is grr_u8_demosaic_images on the clean arena (the one launch that
kernels.u8_demosaic_images issues) for each fill (zero, bilinear, malvar), device events around each of 20 calls after a warm-up, and for malvar once more on the
pictures with their last column cut off, whose odd width puts three rows in four on the byte-store path; "host" is
one serial pass of training.demosaic_degrade_u8 (numpy) over every picture; grr_stream_copy is timed in the same
process.  One JSON line ("bench": "demosaic") with, per case, the times, the algorithmic GB/s (3 bytes read and 3
written per pixel) and that rate as a share of the copy's.

With --blur SPEC (gaussian:SIDE:SIGMA, box:SIDE, motion:LENGTH:ANGLE, file:PATH.npy, or random:SIDE for a random
SIDE x SIDE table) only the synthesis of a deblurring training set's blurred pictures is timed, on the same pictures and
by the same method: "device" is grr_u8_blur_images on the clean arena (the one launch kernels.u8_blur_images issues),
device events around each of 20 calls after a warm-up; "host" is training.blur_degrade_u8 (numpy) over the first
pictures of the set -- as many as keep it to a few hundred tap passes, one picture for a 25 x 25 kernel; the line says
how many ("host_pictures") and scales their time to the arena by bytes; grr_stream_copy is timed in the same process.
One JSON line ("bench": "blur") with the times, the algorithmic GB/s (a byte read and a byte written per element), that
rate as a share of the copy's, and the multiply-adds per second (taps of the table, zeros included, per output byte)
beside the v_dot4_u32_u8 issue ceiling derived from the clock and the SIMD width, not measured.

With --raw-noise SHOT,READ only the batch kernels of the two ways to train a demosaicking model on noisy inputs are
timed, on the same pictures held in one arena, at the five shapes above with all eight modes and random origins:
grr_patch_raw_batch (joint denoising and demosaicking: the noise of variance SHOT x + (READ / 255)^2 on the mosaic,
before the malvar fill, 16 bits, clipped) against grr_patch_pair_batch with sigma READ / 255 (25 / 255 if READ is 0) over
the arena kernels.u8_demosaic_images filled beforehand -- white noise after the fill -- and grr_patch_raw_batch without a
noise table.  Device events around runs of 50 launches on preallocated outputs and uploaded tables, the three
alternating, 10 rounds.  One JSON line per shape ("bench": "raw_noise") with each kernel's median, fastest and slowest
round in microseconds per launch, its batches per second, and the normals a batch draws: (ph + 4)(pw + 4) per sample
for the new kernel, 3 ph pw for the existing noise path.

With --inpaint KEEP the inpainting batches are timed at the five shapes above: training.RandomMaskInpainting (conv fill,
flat 7 x 7) under a DataLoader and under the DevicePatchLoader, as the first paragraph times the noise set, and then the
kernels alone on one uploaded table with all eight modes and random origins -- grr_patch_mask_batch with the zero fill
and with the conv fill at sides 7 and 15, and grr_patch_batch (sigma 25 / 255) on the same arena -- device events around
runs of 50 launches on preallocated outputs, the four alternating, 10 rounds.  One JSON line per shape ("bench":
"inpaint") with both loaders' batches per second, each kernel's median, fastest and slowest round in microseconds per
launch and the ratio of each fill to grr_patch_batch.

    python bench_data.py [--paired | --pair-kernel | --bicubic S | --jpeg Q | --demosaic PATTERN | --blur SPEC | --raw-noise SHOT,READ | --inpaint KEEP] [--steps 60] [--warmup 10] [--images 12] [--side 1200] [--workers 4] [--files 8600]
"""
from __future__ import annotations

import argparse
import json
import logging
import os
import tempfile
import time

import numpy as np
import torch

SHAPES = ((4, 128), (3, 192), (2, 256), (1, 384), (32, 512))


def write_pictures(folder: str, n: int, side: int, seed: int = 7, paired: bool = False) -> str:
    """n RGB PNGs (side x side, and every third one smaller than a crop's 800-pixel threshold) and their csv:
    smooth ramps plus noise, so the files neither compress away nor decode faster than photographs do.  paired:
    each picture is a degraded file, its target_path a second file of the same kind and size."""
    from PIL import Image
    rs = np.random.RandomState(seed)
    lines = ["index,path,target_path,height,width,nchannels" if paired else "index,path,height,width,nchannels"]
    for k in range(n):
        h, w = (side, side + 64) if k % 3 else (640, 720)
        yy, xx = np.mgrid[0:h, 0:w]
        base = np.stack([(yy * (k + 1) + xx * 2) % 256, (yy + xx * (k + 2)) % 256, (yy * 3 + xx) % 256], axis=2)
        img = np.clip(base * 0.6 + rs.randint(0, 103, size=(h, w, 3)), 0, 255).astype(np.uint8)
        Image.fromarray(img).save(os.path.join(folder, f"img{k:03d}.png"))
        if paired:
            clean = np.clip(base * 0.6 + rs.randint(0, 103, size=(h, w, 3)), 0, 255).astype(np.uint8)
            Image.fromarray(clean).save(os.path.join(folder, f"clean{k:03d}.png"))
        lines.append(f"{k},img{k:03d}.png,clean{k:03d}.png,{h},{w},3" if paired else f"{k},img{k:03d}.png,{h},{w},3")
    csv_path = os.path.join(folder, "info.csv")
    with open(csv_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return csv_path


def write_small_pictures(folder: str, n: int, side: int, seed: int = 11) -> str:
    """n small RGB PNGs (side x side, shifts of one noisy ramp, lightly compressed so writing them is quick) and
    their csv: a file count like a training set's at little disk and decode cost."""
    from PIL import Image
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:side, 0:side]
    base = np.clip(np.stack([yy * 2 + xx, yy + xx * 3, yy * 3 + xx * 2], axis=2) % 256 * 0.6
                   + rs.randint(0, 103, size=(side, side, 3)), 0, 255).astype(np.uint8)
    lines = ["index,path,height,width,nchannels"]
    for k in range(n):
        Image.fromarray(np.roll(base, (k * 7) % side, axis=(k // side) % 2)).save(
            os.path.join(folder, f"s{k:05d}.png"), compress_level=1)
        lines.append(f"{k},s{k:05d}.png,{side},{side},3")
    csv_path = os.path.join(folder, "info.csv")
    with open(csv_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return csv_path


def timed(batches, warmup: int, steps: int, to_device) -> float:
    """Seconds per batch over ``steps`` batches after ``warmup`` (worker start-up and first launches excluded)."""
    it = iter(batches)
    for _ in range(warmup):
        to_device(next(it))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        to_device(next(it))
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    del it
    return dt


def pair_kernel(rounds: int = 15, launches: int = 200) -> None:
    import irdu_amd
    irdu_amd.load_native()
    from irdu_amd import _native, kernels, restore
    dev = torch.device("cuda:0")
    n, c, size, side = 64, 3, 128, 512
    rs = np.random.RandomState(3)
    packs = [restore.pack_images([rs.randint(0, 256, (side, side, c)).astype(np.uint8) for _ in range(8)], dev)
             for _ in range(2)]
    src = kernels.patch_pair_source(*packs)
    rows = np.stack([np.arange(n) % 8, rs.randint(0, side - size, n), rs.randint(0, side - size, n), np.arange(n) % 8], 1)
    table = torch.from_numpy(rows.astype(np.int32)).to(dev)
    ids = torch.arange(n, dtype=torch.int64, device=dev)
    sigma = torch.full((n,), 25.0 / 255.0, dtype=torch.float32, device=dev)
    out = [torch.empty((n, c, size, size), dtype=torch.float32, device=dev) for _ in range(2)]
    stream = torch.cuda.current_stream().cuda_stream
    arena, target = packs[0].arena, packs[1].arena
    common = (c, packs[0].table.data_ptr(), 8, table.data_ptr(), ids.data_ptr())
    tail = (n, 2204, size, size, out[0].data_ptr(), out[1].data_ptr(), stream)
    calls = {"patch_pair_batch": lambda: _native.call("grr_patch_pair_batch", arena.data_ptr(), target.data_ptr(),
                                                      arena.numel(), *common, None, *tail),
             "patch_batch": lambda: _native.call("grr_patch_batch", target.data_ptr(), target.numel(), *common,
                                                 sigma.data_ptr(), *tail)}
    # the two entry points on these tables: the pair's target is patch_batch's clean batch
    t, _ = kernels.patch_pair_batch(src, table, ids, None, 2204, size, size)
    cl, _ = kernels.patch_batch(packs[1], table, ids, sigma, 2204, size, size)
    assert torch.equal(t, cl)
    us = {k: [] for k in calls}
    for r in range(rounds + 1):                      # round 0 warms both up
        for name, call in calls.items():
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(launches):
                call()
            end.record()
            torch.cuda.synchronize()
            if r:
                us[name].append(start.elapsed_time(end) * 1e3 / launches)
    line = {"bench": "pair_kernel", "batch": n, "channels": c, "size": size, "rounds": rounds, "launches": launches}
    for name, v in us.items():
        nbytes = n * c * size * size * (10 if name == "patch_pair_batch" else 9)
        line[name] = {"median_us": round(float(np.median(v)), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2),
                      "median_gbps": round(nbytes / float(np.median(v)) / 1e3, 1)}
    print(json.dumps(line), flush=True)


def synthetic_pictures(n: int, side: int, seed: int = 7):
    """write_pictures' pictures as arrays: n RGB pictures, side x (side + 64) and every third one 640 x 720."""
    rs = np.random.RandomState(seed)
    pics = []
    for k in range(n):
        h, w = (side, side + 64) if k % 3 else (640, 720)
        yy, xx = np.mgrid[0:h, 0:w]
        base = np.stack([(yy * (k + 1) + xx * 2) % 256, (yy + xx * (k + 2)) % 256, (yy * 3 + xx) % 256], axis=2)
        pics.append(np.clip(base * 0.6 + rs.randint(0, 103, size=(h, w, 3)), 0, 255).astype(np.uint8))
    return pics


def bicubic(scale: int, images: int, side: int, rounds: int = 20) -> None:
    from PIL import Image
    import irdu_amd
    irdu_amd.load_native()
    from irdu_amd import _native, kernels, restore
    dev = torch.device("cuda:0")
    pics = synthetic_pictures(images, side)
    pack = restore.pack_images(pics, dev)
    low = kernels.u8_resize_images(pack, scale, False)                      # also the warm-up of both directions
    degraded = kernels.u8_bicubic_degrade_images(pack, scale)
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        kernels.u8_bicubic_degrade_images(pack, scale)
        end.record()
        torch.cuda.synchronize()
        ms.append(start.elapsed_time(end))
    # the float4 copy at the arena's size, for scale: bytes read plus bytes written over its time
    n_floats = pack.arena.numel() // 4
    a = torch.empty(n_floats, dtype=torch.float32, device=dev)
    b = torch.empty_like(a)
    stream = torch.cuda.current_stream().cuda_stream
    copy_ms = []
    for r in range(rounds + 1):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        _native.call("grr_stream_copy", b.data_ptr(), a.data_ptr(), n_floats, stream)
        end.record()
        torch.cuda.synchronize()
        if r:
            copy_ms.append(start.elapsed_time(end))
    assert degraded.host_table == pack.host_table
    t0 = time.perf_counter()
    for pic in pics:
        im = Image.fromarray(pic)
        small = im.resize((-(-im.width // scale), -(-im.height // scale)), Image.BICUBIC)
        np.asarray(small.resize(im.size, Image.BICUBIC))
    host_s = time.perf_counter() - t0
    # down reads the clean arena and writes the low one; up reads the low one and writes the degraded one
    nbytes = 2 * pack.arena.numel() + 2 * low.arena.numel()
    med = float(np.median(ms))
    print(json.dumps({"bench": "bicubic", "scale": scale, "images": images, "arena_mb": round(pack.arena.numel() / 2 ** 20, 1),
                      "low_mb": round(low.arena.numel() / 2 ** 20, 2), "rounds": rounds,
                      "device_ms": {"median": round(med, 3), "min": round(min(ms), 3), "max": round(max(ms), 3)},
                      "device_gbps": round(nbytes / med / 1e6, 1),
                      "stream_copy_gbps": round(8 * n_floats / float(np.median(copy_ms)) / 1e6, 1),
                      "host_pillow_s": round(host_s, 3), "host_over_device": round(host_s * 1e3 / med, 1)}), flush=True)


def device_ms(call, rounds: int):
    """Milliseconds of ``rounds`` calls, each between two device events, after one warm-up call."""
    ms = []
    for r in range(rounds + 1):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        call()
        end.record()
        torch.cuda.synchronize()
        if r:
            ms.append(start.elapsed_time(end))
    return ms


def spread(ms) -> dict:
    return {"median": round(float(np.median(ms)), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def jpeg(quality: int, images: int, side: int, rounds: int = 20) -> None:
    import io
    from PIL import Image
    import irdu_amd
    irdu_amd.load_native()
    from irdu_amd import _native, kernels, restore
    dev = torch.device("cuda:0")
    pics = synthetic_pictures(images, side)
    stream = torch.cuda.current_stream().cuda_stream
    line = {"bench": "jpeg", "quality": quality, "images": images, "rounds": rounds}
    for mode, sub, chosen in (("gray", 0, [p[:, :, :1] for p in pics]), ("444", 0, pics), ("420", 2, pics)):
        pack = restore.pack_images([np.ascontiguousarray(p) for p in chosen], dev)
        n = pack.arena.numel()
        qualities = torch.full((len(pack),), quality, dtype=torch.int32, device=dev)     # no upload in the timed call
        ms = device_ms(lambda: kernels.u8_jpeg_images(pack, qualities, sub), rounds)
        # the float4 copy of the same bytes, in the same process
        a = torch.empty(n // 4, dtype=torch.float32, device=dev)
        b = torch.empty_like(a)
        copy = device_ms(lambda: _native.call("grr_stream_copy", b.data_ptr(), a.data_ptr(), n // 4, stream), rounds)
        t0 = time.perf_counter()
        for pic in chosen:
            buf = io.BytesIO()
            Image.fromarray(pic[:, :, 0] if pic.shape[2] == 1 else pic).save(buf, format="JPEG", quality=quality,
                                                                            subsampling=sub)
            np.asarray(Image.open(io.BytesIO(buf.getvalue())))
        host_s = time.perf_counter() - t0
        med, copy_med = float(np.median(ms)), float(np.median(copy))
        line[mode] = {"arena_mb": round(n / 2 ** 20, 1), "device_ms": spread(ms),
                      "device_gbps": round(2 * n / med / 1e6, 1), "stream_copy_ms": spread(copy),
                      "stream_copy_gbps": round(8 * (n // 4) / copy_med / 1e6, 1),
                      "kernel_over_copy": round(med / copy_med, 1), "host_pillow_s": round(host_s, 3),
                      "host_over_device": round(host_s * 1e3 / med, 1)}
        del pack, a, b
    print(json.dumps(line), flush=True)
    # the blocking sums against the SSE on one large picture: host clock, each call ends in its device-to-host copy
    rs = np.random.RandomState(5)
    x = torch.from_numpy(rs.randint(0, 256, (2048, 2048, 3)).astype(np.uint8)).to(dev)
    y = torch.from_numpy(rs.randint(0, 256, (2048, 2048, 3)).astype(np.uint8)).to(dev)
    out = {"bench": "blocking", "shape": [2048, 2048, 3], "rounds": rounds}
    for name, call in (("u8_blocking", lambda: kernels.u8_blocking(x)), ("u8_sse", lambda: kernels.u8_sse(x, y))):
        call()
        us = []
        for _ in range(rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            us.append((time.perf_counter() - t0) * 1e6)
        out[name + "_us"] = spread(us)
    print(json.dumps(out), flush=True)


def demosaic(pattern: str, images: int, side: int, rounds: int = 20) -> None:
    import irdu_amd
    irdu_amd.load_native()
    from irdu_amd import _native, kernels, restore, training
    dev = torch.device("cuda:0")
    pics = synthetic_pictures(images, side)
    stream = torch.cuda.current_stream().cuda_stream
    line = {"bench": "demosaic", "pattern": pattern, "images": images, "rounds": rounds,
            "tile": list(kernels.DEMOSAIC_TILE)}
    cases = [(fill, fill, pics) for fill in kernels.DEMOSAIC_FILLS]
    cases.append(("malvar_odd_width", "malvar", [np.ascontiguousarray(p[:, :-1]) for p in pics]))
    for name, fill, chosen in cases:
        pack = restore.pack_images(chosen, dev)
        n = pack.arena.numel()
        patterns = torch.full((len(pack),), kernels._check_pattern("bench", pattern), dtype=torch.int32, device=dev)
        # the library call itself on a preallocated arena, as the copy below is timed: the wrapper's host checks of a
        # 96-image table would otherwise sit between the two events of a kernel this short
        out = torch.empty_like(pack.arena)
        max_h, max_w = max(h for _, h, _ in pack.host_table), max(w for _, _, w in pack.host_table)
        code = kernels._check_fill("bench", fill)
        assert torch.equal(kernels.u8_demosaic_images(pack, patterns, fill).arena,
                           kernels.u8_demosaic_images(pack, pattern, fill).arena)
        ms = device_ms(lambda: _native.call("grr_u8_demosaic_images", pack.arena.data_ptr(), n, pack.table.data_ptr(),
                                            len(pack), max_h, max_w, out.data_ptr(), patterns.data_ptr(), code, stream),
                       rounds)
        assert torch.equal(out, kernels.u8_demosaic_images(pack, patterns, fill).arena)
        # the float4 copy of the same bytes, in the same process
        a = torch.empty(n // 4, dtype=torch.float32, device=dev)
        b = torch.empty_like(a)
        copy = device_ms(lambda: _native.call("grr_stream_copy", b.data_ptr(), a.data_ptr(), n // 4, stream), rounds)
        t0 = time.perf_counter()
        for pic in chosen:
            training.demosaic_degrade_u8(pic, pattern, fill)
        host_s = time.perf_counter() - t0
        med, copy_med = float(np.median(ms)), float(np.median(copy))
        gbps, copy_gbps = 2 * n / med / 1e6, 8 * (n // 4) / copy_med / 1e6
        line[name] = {"arena_mb": round(n / 2 ** 20, 1), "device_ms": spread(ms), "device_gbps": round(gbps, 1),
                      "stream_copy_ms": spread(copy), "stream_copy_gbps": round(copy_gbps, 1),
                      "share_of_copy_rate": round(gbps / copy_gbps, 3), "host_numpy_s": round(host_s, 3),
                      "host_over_device": round(host_s * 1e3 / med, 1)}
        del pack, a, b, out
    print(json.dumps(line), flush=True)


def blur(spec: str, images: int, side: int, rounds: int = 20, boundary: str = "wrap") -> None:
    import irdu_amd
    irdu_amd.load_native()
    from irdu_amd import _native, kernels, restore, training
    dev = torch.device("cuda:0")
    pics = synthetic_pictures(images, side)
    stream = torch.cuda.current_stream().cuda_stream
    if spec.startswith("random:"):
        n = int(spec.split(":")[1])
        kernel = training.BlurKernel(np.random.RandomState(5).rand(n, n), spec)
    else:
        kernel = training.parse_blur_spec(spec)
    taps = kernel.kh * kernel.kw
    pack = restore.pack_images(pics, dev)
    n = pack.arena.numel()
    # the library call itself on a preallocated arena and uploaded tables, as the copy below is timed
    out = torch.empty_like(pack.arena)
    slot = np.zeros((1, kernels.MAX_BLUR_SIDE, kernels.MAX_BLUR_SIDE), np.int32)
    slot[0, :kernel.kh, :kernel.kw] = kernel.table
    weights = torch.from_numpy(slot).to(dev)
    sizes = torch.tensor([[kernel.kh, kernel.kw]], dtype=torch.int32, device=dev)
    of = torch.zeros(len(pack), dtype=torch.int32, device=dev)
    max_h, max_w = max(h for _, h, _ in pack.host_table), max(w for _, _, w in pack.host_table)
    code = kernels._check_boundary("bench", boundary)
    ms = device_ms(lambda: _native.call("grr_u8_blur_images", pack.arena.data_ptr(), n, pack.table.data_ptr(), len(pack),
                                        max_h, max_w, 3, out.data_ptr(), weights.data_ptr(), sizes.data_ptr(), 1,
                                        of.data_ptr(), code, stream), rounds)
    assert torch.equal(out, kernels.u8_blur_images(pack, kernel, 0, boundary).arena)
    # the float4 copy of the same bytes, in the same process
    a = torch.empty(n // 4, dtype=torch.float32, device=dev)
    b = torch.empty_like(a)
    copy = device_ms(lambda: _native.call("grr_stream_copy", b.data_ptr(), a.data_ptr(), n // 4, stream), rounds)
    host_pictures = max(1, min(images, 200 // taps))
    t0 = time.perf_counter()
    for i, pic in enumerate(pics[:host_pictures]):
        got = training.blur_degrade_u8(pic, kernel, boundary)
        if i == 0:
            off, h, w = pack.host_table[0]
            assert np.array_equal(got.ravel(), out[off:off + h * w * 3].cpu().numpy())      # the same bytes
    host_s = time.perf_counter() - t0
    host_arena_s = host_s * n / sum(p.size for p in pics[:host_pictures])
    med, copy_med = float(np.median(ms)), float(np.median(copy))
    gbps, copy_gbps = 2 * n / med / 1e6, 8 * (n // 4) / copy_med / 1e6
    # v_dot4_u32_u8: 4 byte multiply-adds per lane, 32 lanes per SIMD and clock, 4 SIMDs on each of 256 CUs at 2.4 GHz;
    # a tap takes two of them (low and high weight byte)
    dot4_macs = 4 * 32 * 4 * 256 * 2.4e9
    print(json.dumps({"bench": "blur", "spec": kernel.spec, "sides": [kernel.kh, kernel.kw], "boundary": boundary,
                      "images": images, "rounds": rounds, "tile": list(kernels.BLUR_TILE),
                      "arena_mb": round(n / 2 ** 20, 1), "device_ms": spread(ms), "device_gbps": round(gbps, 1),
                      "stream_copy_ms": spread(copy), "stream_copy_gbps": round(copy_gbps, 1),
                      "share_of_copy_rate": round(gbps / copy_gbps, 3), "time_over_copy": round(med / copy_med, 2),
                      "host_pictures": host_pictures, "host_numpy_s": round(host_s, 3),
                      "host_numpy_arena_s_scaled": round(host_arena_s, 2),
                      "host_over_device": round(host_arena_s * 1e3 / med, 1),
                      "tera_taps_per_s": round(n * taps / med / 1e9, 2),
                      "derived_dot4_ceiling_tera_taps_per_s": round(dot4_macs / 2 / 1e12, 1),
                      "share_of_derived_ceiling": round(n * taps / (med * 1e-3) / (dot4_macs / 2), 3)}), flush=True)


def raw_noise(spec: str, images: int, side: int, rounds: int = 10, launches: int = 50, pattern: str = "rggb") -> None:
    import irdu_amd
    irdu_amd.load_native()
    from irdu_amd import _native, kernels, restore
    dev = torch.device("cuda:0")
    shot, read = (float(v) for v in spec.split(","))
    a, b = kernels.raw_noise_pair("bench_data --raw-noise", shot, read)
    pics = synthetic_pictures(images, side)
    pack = restore.pack_images(pics, dev)
    filled = kernels.u8_demosaic_images(pack, pattern, "malvar")
    raw_src = kernels.patch_raw_source(pack, pattern)
    pair_src = kernels.patch_pair_source(filled, pack)
    hw = raw_src.hw
    stream = torch.cuda.current_stream().cuda_stream
    rs = np.random.RandomState(3)
    sigma_level = read if read > 0 else 25.0
    for n, size in SHAPES:
        img = np.arange(n) % images
        rows = np.stack([img, rs.randint(0, hw[img, 0] - size), rs.randint(0, hw[img, 1] - size), np.arange(n) % 8], 1)
        table = torch.from_numpy(rows.astype(np.int32)).to(dev)
        ids = torch.arange(n, dtype=torch.int64, device=dev)
        noise = torch.tensor([[a, b]] * n, dtype=torch.float32, device=dev)
        sigma = torch.full((n,), sigma_level / 255.0, dtype=torch.float32, device=dev)
        out = [torch.empty((n, 3, size, size), dtype=torch.float32, device=dev) for _ in range(2)]
        raw = lambda table_of_noise: _native.call(
            "grr_patch_raw_batch", pack.arena.data_ptr(), pack.arena.numel(), pack.table.data_ptr(), images,
            raw_src.patterns.data_ptr(), table.data_ptr(), ids.data_ptr(), table_of_noise, n, 2204, size, size, 2, 16, 1,
            out[0].data_ptr(), out[1].data_ptr(), stream)
        calls = {"patch_raw_batch": lambda: raw(noise.data_ptr()),
                 "patch_pair_batch_sigma": lambda: _native.call(
                     "grr_patch_pair_batch", filled.arena.data_ptr(), pack.arena.data_ptr(), pack.arena.numel(), 3,
                     pack.table.data_ptr(), images, table.data_ptr(), ids.data_ptr(), sigma.data_ptr(), n, 2204, size, size,
                     out[0].data_ptr(), out[1].data_ptr(), stream),
                 "patch_raw_batch_no_noise": lambda: raw(None)}
        # the entry points on these tables: one target, and without noise the raw input is the filled arena's up to the
        # rounding to bytes that the arena went through
        t_raw, i_raw = kernels.patch_raw_batch(raw_src, table, ids, None, 2204, size, size)
        t_pair, i_pair = kernels.patch_pair_batch(pair_src, table, ids, None, 2204, size, size)
        assert torch.equal(t_raw, t_pair) and float((i_raw.clamp(0, 1) - i_pair).abs().max()) <= 0.5 / 255 + 1e-6
        us = {k: [] for k in calls}
        for r in range(rounds + 1):                      # round 0 warms all up
            for name, call in calls.items():
                start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                for _ in range(launches):
                    call()
                end.record()
                torch.cuda.synchronize()
                if r:
                    us[name].append(start.elapsed_time(end) * 1e3 / launches)
        line = {"bench": "raw_noise", "shot": shot, "read": read, "a": a, "b": b, "pair_sigma_level": sigma_level,
                "pattern": pattern, "fill": "malvar", "bits": 16, "images": images, "arena_mb": round(pack.arena.numel() / 2 ** 20, 1),
                "batch": n, "size": size, "rounds": rounds, "launches": launches, "tile": list(kernels.RAW_NOISE_TILE),
                "normals_per_batch": {"patch_raw_batch": n * (size + 4) * (size + 4), "patch_pair_batch_sigma": n * 3 * size * size}}
        for name, v in us.items():
            med = float(np.median(v))
            line[name] = {"median_us": round(med, 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2),
                          "batches_per_s": round(1e6 / med, 1)}
        print(json.dumps(line), flush=True)


def inpaint(keep: float, images: int, side: int, steps: int, warmup: int, device_steps: int, workers: int,
            rounds: int = 10, launches: int = 50) -> None:
    import irdu_amd
    irdu_amd.load_native()
    from irdu_amd import _native, kernels, training
    dev = torch.device("cuda:0")
    log = logging.getLogger("bench_data")
    units = kernels.keep_units(keep)
    stream = torch.cuda.current_stream().cuda_stream
    tables = {"zero": (kernels.mask_weights(1), 0), "conv7": (kernels.mask_weights(7), 1), "conv15": (kernels.mask_weights(15), 1)}
    tables = {k: (torch.from_numpy(w).to(dev), w.shape[0], fill) for k, (w, fill) in tables.items()}

    def planar(pair):        # what Trainer.step does with a host batch
        return [t.to(dev, non_blocking=True).permute(0, 3, 1, 2).contiguous() for t in pair]

    shared: dict = {}
    rs = np.random.RandomState(3)
    with tempfile.TemporaryDirectory() as folder:
        csv_path = write_pictures(folder, images, side)
        for batch, size in SHAPES:
            n = (steps + warmup + 1) * batch
            ds = training.RandomMaskInpainting(csv_path=csv_path, root_folder=folder, keep=keep, fill="conv", fill_side=7,
                                               use_data_aug=True, patch_size=(size, size), max_num_patchs=n, logger=log)
            host = torch.utils.data.DataLoader(ds, sampler=training.ResumeableSampler(ds, batch), batch_size=batch,
                                               num_workers=workers)
            host_s = timed(host, warmup, steps, planar)
            del host

            def passes():
                while True:
                    yield from training.DevicePatchLoader(ds, training.ResumeableSampler(ds, batch), batch, device=dev,
                                                          shared=shared)
            dev_s = timed(passes(), warmup, device_steps, lambda pair: pair)
            # the kernels alone, on one uploaded table and preallocated outputs: the three fills and grr_patch_batch
            loader = training.DevicePatchLoader(ds, training.ResumeableSampler(ds, batch), batch, device=dev, shared=shared)
            pack = loader.prepare()
            hw, n_img = loader.source.hw, loader.source.n_img
            img = np.arange(batch) % n_img
            rows = np.stack([img, rs.randint(0, hw[img, 0] - size), rs.randint(0, hw[img, 1] - size), np.arange(batch) % 8], 1)
            table = torch.from_numpy(rows.astype(np.int32)).to(dev)
            ids = torch.arange(batch, dtype=torch.int64, device=dev)
            keeps = torch.full((batch,), units, dtype=torch.int32, device=dev)
            sigma = torch.full((batch,), 25.0 / 255.0, dtype=torch.float32, device=dev)
            out = [torch.empty((batch, 3, size, size), dtype=torch.float32, device=dev) for _ in range(2)]
            mask = torch.empty((batch, 1, size, size), dtype=torch.float32, device=dev)

            def masked(name):
                w, k, fill = tables[name]
                return lambda: _native.call(
                    "grr_patch_mask_batch", pack.arena.data_ptr(), pack.arena.numel(), 3, pack.table.data_ptr(), n_img,
                    table.data_ptr(), ids.data_ptr(), keeps.data_ptr(), batch, 2204, size, size, w.data_ptr(), k, k, fill, 128,
                    out[0].data_ptr(), out[1].data_ptr(), mask.data_ptr(), stream)
            calls = {"patch_mask_batch_" + name: masked(name) for name in tables}
            calls["patch_batch"] = lambda: _native.call(
                "grr_patch_batch", pack.arena.data_ptr(), pack.arena.numel(), 3, pack.table.data_ptr(), n_img, table.data_ptr(),
                ids.data_ptr(), sigma.data_ptr(), batch, 2204, size, size, out[0].data_ptr(), out[1].data_ptr(), stream)
            us = {k: [] for k in calls}
            for r in range(rounds + 1):                      # round 0 warms all up
                for name, call in calls.items():
                    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    start.record()
                    for _ in range(launches):
                        call()
                    end.record()
                    torch.cuda.synchronize()
                    if r:
                        us[name].append(start.elapsed_time(end) * 1e3 / launches)
            line = {"bench": "inpaint", "keep": keep, "keep_units": units, "batch": batch, "size": size, "steps": steps,
                    "device_steps": device_steps, "workers": workers, "images": images,
                    "arena_mb": round(pack.arena.numel() / 2 ** 20, 1), "rounds": rounds, "launches": launches,
                    "tile": list(kernels.MASK_TILE), "host_ms_per_batch": round(host_s * 1e3, 3),
                    "host_batches_per_s": round(1.0 / host_s, 2), "device_ms_per_batch": round(dev_s * 1e3, 4),
                    "device_batches_per_s": round(1.0 / dev_s, 1), "device_over_host": round(host_s / dev_s, 1)}
            for name, v in us.items():
                med = float(np.median(v))
                line[name] = {"median_us": round(med, 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2),
                              "batches_per_s": round(1e6 / med, 1)}
            base = line["patch_batch"]["median_us"]
            line["ratio_to_patch_batch"] = {name: round(line["patch_mask_batch_" + name]["median_us"] / base, 2) for name in tables}
            print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    # the DataLoader's workers hold up to 2 batches each in flight when the clock starts: enough timed batches
    # that those 8 are a small share
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--device-steps", type=int, default=3000, help="timed batches of the device loader")
    ap.add_argument("--images", type=int, default=12)
    ap.add_argument("--side", type=int, default=1200)
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--files", type=int, default=8600,
                    help="files of the many-files measurement of the device loader (0: skip it)")
    ap.add_argument("--small-side", type=int, default=160, help="side of its pictures")
    ap.add_argument("--paired", action="store_true",
                    help="degraded / clean file pairs: PairedImageRestoration on both paths (no many-files run)")
    ap.add_argument("--pair-kernel", action="store_true",
                    help="only time grr_patch_pair_batch (no sigma) against grr_patch_batch (sigma > 0) on one shape")
    ap.add_argument("--bicubic", type=int, default=None, metavar="S",
                    help="only time the synthesis of the degraded pictures at scale S: the device kernels against "
                         "Pillow's resize down and up on the host")
    ap.add_argument("--jpeg", type=int, default=None, metavar="Q",
                    help="only time the synthesis of the JPEG-degraded pictures at quality Q: the device kernel (gray, "
                         "4:4:4, 4:2:0) against Pillow's encode and decode on the host, then the blocking kernel")
    ap.add_argument("--demosaic", type=str, default=None, metavar="PATTERN", choices=("rggb", "grbg", "gbrg", "bggr"),
                    help="only time the synthesis of the filled Bayer mosaics with this pattern: the device kernel (each "
                         "fill) against numpy on the host")
    ap.add_argument("--blur", type=str, default=None, metavar="SPEC",
                    help="only time the synthesis of the blurred pictures with this kernel (a spec of "
                         "training.parse_blur_spec, or random:SIDE): the device kernel against numpy on the host")
    ap.add_argument("--raw-noise", type=str, default=None, metavar="SHOT,READ",
                    help="only time grr_patch_raw_batch (noise on the mosaic, before the fill) against grr_patch_pair_batch "
                         "with sigma over a pre-filled demosaic arena, at the curriculum's shapes")
    ap.add_argument("--inpaint", type=float, default=None, metavar="KEEP",
                    help="only time grr_patch_mask_batch (zero fill, conv at sides 7 and 15) with this known share against "
                         "grr_patch_batch on the same arena, and RandomMaskInpainting on both loader paths, at the "
                         "curriculum's shapes")
    args = ap.parse_args()
    if args.inpaint is not None:
        return inpaint(args.inpaint, args.images, args.side, args.steps, args.warmup, args.device_steps, args.workers)
    if args.raw_noise is not None:
        return raw_noise(args.raw_noise, args.images, args.side)
    if args.blur is not None:
        return blur(args.blur, args.images, args.side)
    if args.pair_kernel:
        return pair_kernel()
    if args.demosaic is not None:
        return demosaic(args.demosaic, args.images, args.side)
    if args.jpeg is not None:
        return jpeg(args.jpeg, args.images, args.side)
    if args.bicubic is not None:
        return bicubic(args.bicubic, args.images, args.side)
    import irdu_amd
    irdu_amd.load_native()
    from irdu_amd import kernels, training
    dev = torch.device("cuda:0")
    log = logging.getLogger("bench_data")

    def planar(pair):        # what Trainer.step does with a host batch
        return [t.to(dev, non_blocking=True).permute(0, 3, 1, 2).contiguous() for t in pair]

    shared: dict = {}        # the shapes read one set of files: one arena
    with tempfile.TemporaryDirectory() as folder:
        csv_path = write_pictures(folder, args.images, args.side, paired=args.paired)
        for batch, size in SHAPES:
            n = (args.steps + args.warmup + 1) * batch
            if args.paired:
                ds = training.PairedImageRestoration(csv_path=csv_path, root_folder=folder, use_data_aug=True,
                                                     patch_size=(size, size), max_num_patchs=n, logger=log)
            else:
                ds = training.ImageSuperResolution(csv_path=csv_path, root_folder=folder, dist_mode="addictive_noise_scale",
                                                   lambda_noise=25.0, use_data_aug=True, patch_size=(size, size),
                                                   max_num_patchs=n, logger=log)
            host = torch.utils.data.DataLoader(ds, sampler=training.ResumeableSampler(ds, batch), batch_size=batch,
                                               num_workers=args.workers)
            host_s = timed(host, args.warmup, args.steps, planar)
            del host
            loader = training.DevicePatchLoader(ds, training.ResumeableSampler(ds, batch), batch, device=dev,
                                                shared=shared)
            t0 = time.perf_counter()
            pack = loader.prepare()
            torch.cuda.synchronize()
            pack_s = time.perf_counter() - t0
            # a batch takes a fraction of a millisecond: passes over the dataset until the window is long enough
            def passes():
                while True:
                    yield from training.DevicePatchLoader(ds, training.ResumeableSampler(ds, batch), batch, device=dev,
                                                          shared=shared)
            dev_s = timed(passes(), args.warmup, args.device_steps, lambda pair: pair)
            # the kernel alone: HIP events around each launch of one more pass
            timer = kernels.LaunchTimer()
            kernels.set_timer(timer)
            for _ in training.DevicePatchLoader(ds, training.ResumeableSampler(ds, batch), batch, device=dev,
                                                shared=shared):
                pass
            kernels.set_timer(None)
            kern = timer.summary()["patch_pair_batch" if args.paired else "patch_batch"]
            arena_elems = sum(p.arena.numel() for p in pack) if args.paired else pack.arena.numel()
            print(json.dumps({"bench": "data_paired" if args.paired else "data", "batch": batch, "size": size, "steps": args.steps, "device_steps": args.device_steps,
                              "workers": args.workers, "images": args.images, "arena_mb": arena_elems / 2 ** 20,
                              "pack_s": round(pack_s, 4), "host_ms_per_batch": round(host_s * 1e3, 3),
                              "host_batches_per_s": round(1.0 / host_s, 2), "device_ms_per_batch": round(dev_s * 1e3, 4),
                              "device_batches_per_s": round(1.0 / dev_s, 1),
                              "kernel_us": round(kern["mean_ms"] * 1e3, 2), "kernel_gbps": round(kern["gbps"], 1)}),
                  flush=True)

    # The device loader's host cost per batch must not grow with the number of files: a training set's file count
    # (DFWB: 8600) of small pictures, the first curriculum shape.
    if args.files > 0 and not args.paired:
        with tempfile.TemporaryDirectory() as folder:
            csv_path = write_small_pictures(folder, args.files, args.small_side)
            batch, size = SHAPES[0]
            ds = training.ImageSuperResolution(csv_path=csv_path, root_folder=folder, dist_mode="addictive_noise_scale",
                                               lambda_noise=25.0, use_data_aug=True, patch_size=(size, size),
                                               max_num_patchs=4 * args.files, logger=log)
            many: dict = {}
            loader = training.DevicePatchLoader(ds, training.ResumeableSampler(ds, batch), batch, device=dev, shared=many)
            t0 = time.perf_counter()
            pack = loader.prepare()
            torch.cuda.synchronize()
            pack_s = time.perf_counter() - t0

            def passes():
                while True:
                    yield from training.DevicePatchLoader(ds, training.ResumeableSampler(ds, batch), batch, device=dev,
                                                          shared=many)
            dev_s = timed(passes(), args.warmup, args.device_steps, lambda pair: pair)
            print(json.dumps({"bench": "data_many_files", "files": args.files, "side": args.small_side, "batch": batch,
                              "size": size, "device_steps": args.device_steps, "arena_mb": pack.arena.numel() / 2 ** 20,
                              "pack_s": round(pack_s, 3), "device_ms_per_batch": round(dev_s * 1e3, 4),
                              "device_batches_per_s": round(1.0 / dev_s, 1)}), flush=True)


if __name__ == "__main__":
    main()
