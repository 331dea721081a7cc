"""Whole-image restoration: an H x W x C picture of any size in, the restored picture out.

The semantics are the reference's test loop as ``training.validate`` restates it (scripts_v2/...sigma25.py
:249-279): reflect-pad the bottom and right to a multiple of ``factor`` (only a side that is not one
already), filter, crop, clamp to [0, 1], quantise like ``img_as_ubyte``.  When the padded image exceeds
``tile`` on a side it runs in overlap-save windows (``tiling.tile_grid`` on the padded size).

The data movement around the model is three libgrr kernels (csrc/image_ops.hip), not ATen: the image goes
to the device once in its own dtype (uint8 stays uint8); ``kernels.tile_gather`` reads it through the
reflect rule straight into the model's planar float32 window batch; ``kernels.tile_scatter`` writes each
window's core, cropped, clamped and quantised, into the HWC output.  No float32 copy of the whole image,
padded or not, exists on either side of the model, and no per-window ATen op is issued.

Defaults: ``tile`` 512, ``halo`` 64, ``micro_batch`` 16 (as many pixels per launch as config C5's 64 windows
of 256^2).  The halo is set by the deepest model behind this call: the two-scale S = 10 image filter
reproduces the whole image to fp32 rounding at 32 pixels already (tests/test_gpu_tiling.py), but the
four-level v1.0 model does not -- measured on the GPU: 6.6e-4 relative and up to 6 uint8
levels at halo 32, 3e-5 and at most one level at halo 64.  A 512 tile keeps the window overhead of halo 64
where 256 / 32 has it ((512 / 384)^2 = 1.78).  Callers of the image filter alone may pass tile=256, halo=32.

A list of images (``restore_images``, ``evaluate(across_images=True)``) shares window batches: the images
lie back to back in one arena (``pack_images``), ``plan_images`` groups the windows of all images by window
shape into launches of one restore_image launch's pixel budget, and ``kernels.tiles_gather`` /
``tiles_scatter`` / ``u8_sse_segments`` address each window's own image through a device image table.

Geometric self-ensemble (``ensemble=8`` or a list of modes on restore_image, restore_images and evaluate): the
picture is restored under the flips and quarter turns T_m, m = 2k + f = np.rot90(a, k) then np.flipud if f (the
numbering of the reference's ``data_augmentation``), each result is turned back and the M estimates are
averaged.  The transforms act on the model's window, after the reflect rule, so the padding, the window grid,
the cores and the crop are the plain call's for every mode, and a one-window call on a picture that needs no
padding equals transforming the picture itself.  Member j is z_j = T_mj^-1(model(T_mj(window))); the result is
the float32 pairwise tree over the ascending mode list -- [z0 + z1, z2 + z3, ..., the odd one carried] until
one is left, for M = 8 ((z0+z1)+(z2+z3)) + ((z4+z5)+(z6+z7)) -- divided by float32(M), then the plain call's
crop, clamp and quantisation.  With a model that commutes with the transforms the tree gives the plain call's
result bit for bit for M = 2, 4 and 8 (sums of equal values are exact; a left-to-right sum rounds at 3v).
Per group of windows a launch runs ``kernels.tile_gather_d8`` for the even-k modes (0, 1, 4, 5), the model,
``tile_gather_d8`` for the odd-k modes (2, 3, 6, 7: windows of tw x th), the model again, and
``kernels.tile_scatter_mean``: two model calls per group, one per orientation, for square windows too.  No
transformed copy of the picture, no per-mode canvas and no ATen op per mode exists.  A group is
max(1, micro_batch // Mo) windows, Mo the larger number of modes of one orientation, so no model call is larger
than a plain call's -- except where micro_batch < Mo, when a call holds the Mo rows of one window.  The peak
memory grows by one output batch: the even-k results are alive while the odd-k ones are computed.

Metrics: ``psnr_u8`` from the exact integer SSE (``kernels.u8_sse``) and ``ssim_u8``, the 11 x 11 Gaussian-window
SSIM, from the exact integer sum of the per-pixel values quantised to 2^-32 (``kernels.u8_ssim``; float64 per
pixel on the device).  ``evaluate`` returns the PSNRs, ``evaluate_metrics`` both, from one body; with
``across_images`` each metric of all images is one launch on the restored and the clean arena.
``evaluate_pairs`` scores degraded / clean pairs of uint8 pictures with the same kernels and synthesises nothing:
each input is restored as it is and compared with its target.

Bicubic super-resolution: ``bicubic_down_u8`` / ``bicubic_up_u8`` / ``bicubic_degrade_u8`` resize uint8 pictures by an
integer scale on the device with the exact fixed-point bicubic of include/grr.h (``kernels.u8_resize``), and
``evaluate_sr`` runs the protocol of the super-resolution tables on clean pictures: mod-crop, degrade, restore, shave,
score.  The filter stays same-size-in, same-size-out: its input is the picture brought back to size by the bicubic.

JPEG compression-artifact removal: ``jpeg_degrade_u8`` is the JPEG round trip at a quality of 1..100 on the device
(``kernels.u8_jpeg``: libjpeg's integer arithmetic without a bitstream, Pillow's bytes), ``psnrb_u8`` the PSNR-B of a
picture against its reference (the "psnrb" metric of evaluate_metrics and evaluate_pairs), and ``evaluate_car``
degrades clean pictures, restores them and scores them.

Demosaicking: ``demosaic_u8`` is the Bayer mosaic of a picture (or a raw 1-channel mosaic) with its missing channels
filled by the zero, bilinear or Malvar-He-Cutler filter in exact integers (``kernels.u8_demosaic``), and
``evaluate_demosaic`` mosaics clean pictures, restores the filled ones and scores them (CPSNR, SSIM).

Deblurring: ``blur_u8`` is the convolution of a picture with an integer point-spread function under a wrap, replicate
or reflect boundary in exact integers (``kernels.u8_blur``), and ``evaluate_deblur`` blurs clean pictures, adds noise
where asked, restores and scores them.

Single process: several ranks are ``tiling.tiled_forward``'s business.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from functools import partial
from typing import Callable, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import kernels, tiling

TILE, HALO, MICRO_BATCH = 512, 64, 16


@dataclass(frozen=True)
class RestorePlan:
    """Padded size, window size and the windows (tiling.Window rows, in padded-image coordinates)."""
    h: int
    w: int
    hp: int
    wp: int
    th: int
    tw: int
    windows: Tuple[tiling.Window, ...]


def _padded(n: int, factor: int) -> int:
    return n if n % factor == 0 else (n // factor + 1) * factor


def plan(h: int, w: int, factor: int = 16, tile: int = TILE, halo: int = HALO) -> RestorePlan:
    """The windows of an h x w image (pure Python): each side grows to the next multiple of ``factor`` only
    if it is not one already, as in ``validate``; ValueError where torch's reflect pad would raise (a pad
    not smaller than its side) and where ``tiling.tile_grid`` does."""
    if factor < 1 or h < 1 or w < 1:
        raise ValueError(f"plan: h, w, factor must be positive (got {h}, {w}, {factor})")
    hp, wp = _padded(h, factor), _padded(w, factor)
    for n, p in ((h, hp), (w, wp)):
        if p - n >= n:
            raise ValueError(f"plan: reflect padding {p - n} must be smaller than the image side {n} (factor {factor})")
    wins = tiling.tile_grid(hp, wp, tile, halo, align=factor)
    return RestorePlan(h, w, hp, wp, min(tile, hp), min(tile, wp), tuple(wins))


def _ensemble_modes(who: str, ensemble) -> Tuple[int, ...]:
    """The ascending mode list of an ``ensemble`` argument: 1 or None -> (0,), 8 -> all of 0..7, else a strictly
    ascending sequence of modes of 0..7.  (0,) is the plain path.  ValueError otherwise."""
    if ensemble is None or (isinstance(ensemble, int) and not isinstance(ensemble, bool) and ensemble == 1):
        return (0,)
    if isinstance(ensemble, int) and not isinstance(ensemble, bool) and ensemble == 8:
        return tuple(range(8))
    ms = None
    if isinstance(ensemble, (tuple, list, range)) and all(isinstance(m, (int, np.integer)) and not isinstance(m, bool)
                                                          for m in ensemble):
        ms = tuple(int(m) for m in ensemble)
    if not ms or any(not 0 <= m <= 7 for m in ms) or any(b <= a for a, b in zip(ms, ms[1:])):
        raise ValueError(f"{who}: ensemble is 1, 8 or a strictly ascending sequence of modes of 0..7, got {ensemble!r}")
    return ms


def _split_modes(modes: Tuple[int, ...]) -> Tuple[Tuple[int, ...], Tuple[int, ...]]:
    """(even-k modes, odd-k modes): T_m keeps the window's shape for 0, 1, 4, 5 and turns it for 2, 3, 6, 7."""
    return tuple(m for m in modes if m // 2 % 2 == 0), tuple(m for m in modes if m // 2 % 2 == 1)


def _most_modes(modes: Tuple[int, ...]) -> int:
    """Mo: the rows one window has in the larger of a launch's two model calls."""
    return max(len(ms) for ms in _split_modes(modes))


def _checked_image(image) -> Tuple[torch.Tensor, str]:
    """The HWC image as a tensor where it is, shape and dtype checked, and what came in ("numpy", "cpu" or
    "cuda")."""
    kind = "numpy" if isinstance(image, np.ndarray) else None
    if kind:
        if image.dtype not in (np.uint8, np.float32):
            raise ValueError(f"restore_image: image dtype must be uint8 or float32, got {image.dtype}")
        t = torch.from_numpy(np.ascontiguousarray(image))
    elif isinstance(image, torch.Tensor):
        t = image
        kind = "cuda" if t.is_cuda else "cpu"
    else:
        raise ValueError(f"restore_image: expected a numpy array or a torch tensor, got {type(image).__name__}")
    if t.dim() != 3 or t.dtype not in kernels.IMAGE_DTYPES or not kernels.image_io_ok(t.shape[2], t.shape[0], t.shape[1]):
        raise ValueError("restore_image: expected an H x W x C image (C <= 4, below 2^31 elements) of uint8 or "
                         f"float32, got {tuple(t.shape)} {t.dtype}")
    return t, kind


def _to_device(t: torch.Tensor, device) -> torch.Tensor:
    """One transfer, in the image's own dtype."""
    return (t if t.is_cuda and device is None else t.to(device if device is not None else "cuda")).contiguous()


def _model_device(model):
    params = getattr(model, "parameters", None)
    if callable(params):
        for p in params():
            return p.device if p.is_cuda else None
    return None


def _core_px(rows, shapes) -> int:
    """Pixels the rows (img, wr, wc, r0, r1, c0, c1) write into images of these (h, w): the timer's byte count."""
    return sum(max(0, min(r1, shapes[i][0]) - r0) * max(0, min(c1, shapes[i][1]) - c0)
               for i, _, _, r0, r1, c0, c1 in rows)


def _run_launches(who: str, model: Callable, launches, quantise: bool, gather, alloc, scatter, modes=(0,)):
    """The one loop that calls the model: per launch gather -> model once per orientation of ``modes``, then one
    scatter, under no_grad with the model in eval mode (its mode is restored).  launches yields
    (rows, th, tw, core_px), rows a slice of the uploaded window table; gather(rows, ms, bh, bw) is the model's
    input for one orientation's modes ms (bh x bw = th x tw for the even-k ones, tw x th for the odd-k ones),
    alloc(cout, dtype) the output for the first result's channels (uint8 with quantise, else float32) and
    scatter(y0, y1, rows, modes, th, tw, out, core_px) writes both results into it (None where an orientation has
    no mode).  The plain call is modes (0,): one th x tw call per launch (_plain_io adapts its kernels).  Returns
    what alloc did."""
    was_training = bool(getattr(model, "training", False))
    if was_training:
        model.eval()
    out = cout = None
    try:
        with torch.no_grad():
            for rows, th, tw, core_px in launches:
                ys = []
                for ms, bh, bw in zip(_split_modes(modes), (th, tw), (tw, th)):
                    if not ms:
                        ys.append(None)
                        continue
                    n = rows.shape[0] * len(ms)
                    y = model(gather(rows, ms, bh, bw))
                    if y.dim() != 4 or y.shape[0] != n or tuple(y.shape[2:]) != (bh, bw) \
                            or (out is not None and y.shape[1] != cout):
                        raise ValueError(f"{who}: the model returned {tuple(y.shape)} for {n} "
                                         f"windows of {bh} x {bw}")
                    if out is None:     # every pixel of every image is written exactly once (the cores partition it): no fill
                        cout = int(y.shape[1])
                        out = alloc(cout, torch.uint8 if quantise else torch.float32)
                    ys.append(y.float().contiguous())
                scatter(ys[0], ys[1], rows, modes, th, tw, out, core_px)
    finally:
        if was_training:
            model.train()
    return out


def _plain_io(gather, scatter):
    """The plain call's gather(rows, th, tw) and scatter(y, rows, out, core_px) as _run_launches calls them with
    modes (0,): today's kernels, no transform, no mean."""
    return (lambda rows, ms, bh, bw: gather(rows, bh, bw),
            lambda y0, y1, rows, modes, th, tw, out, core_px: scatter(y0, rows, out, core_px))


def _restore_device(model: Callable, img: torch.Tensor, device, factor: int, tile: int, halo: int, micro_batch: int,
                    quantise: bool, modes: Tuple[int, ...] = (0,)) -> torch.Tensor:
    """restore_image on the checked image, sent to the device as it is: micro_batch windows per launch whatever
    the window shape (max(1, micro_batch // Mo) with modes); the result is on that device."""
    p = plan(img.shape[0], img.shape[1], factor, tile, halo)
    img = _to_device(img, device)
    if micro_batch < 1:
        raise ValueError(f"restore_image: micro_batch must be positive (got {micro_batch})")
    table = torch.tensor(p.windows, dtype=torch.int32).to(img.device)     # uploaded once per image
    plain = modes == (0,)
    group = micro_batch if plain else max(1, micro_batch // _most_modes(modes))
    launches = ((table[i:i + group], p.th, p.tw,
                 _core_px([(0,) + tuple(w) for w in p.windows[i:i + group]], [(p.h, p.w)]))
                for i in range(0, len(p.windows), group))
    gather, scatter = _plain_io(partial(kernels.tile_gather, img), kernels.tile_scatter) if plain else \
        (partial(kernels.tile_gather_d8, img), kernels.tile_scatter_mean)
    return _run_launches("restore_image", model, launches, quantise, gather,
                         lambda cout, dtype: torch.empty((p.h, p.w, cout), dtype=dtype, device=img.device), scatter, modes)


def restore_image(model: Callable, image, *, factor: int = 16, tile: int = TILE, halo: int = HALO,
                  micro_batch: int = MICRO_BATCH, quantise: bool = True, device=None, ensemble=1):
    """Restore one H x W x C image (numpy array or torch tensor, uint8 or float32 in [0, 1], host or device)
    with ``model``, any callable from float32 [n, C, th, tw] to [n, Cout, th, tw].

    Returns the H x W x Cout image of the input's kind (numpy in, numpy out; a tensor comes back on the
    input's device): uint8 with ``quantise`` (clamp, x255 in float32, round half to even -- validate()'s
    lines, bit for bit), else float32, unclamped.  If the padded image fits ``tile`` on both sides there is
    one window and the result is the whole-image one.  Runs under no_grad with the model in eval mode (its
    mode is restored).  ``device``: where to run when the image is on the host (default: the model's
    parameters' device, else the current GPU).

    ``ensemble``: 1 (default) restores once; 8 restores under all 8 flips and quarter turns of each window and
    averages the results turned back (the module docstring has the definition, the mode numbering and the
    fixed summation order); a strictly ascending sequence of modes of 0..7 takes that subset.  A launch is then
    max(1, micro_batch // Mo) windows and two model calls, one of th x tw and one of tw x th windows, so the
    model must take both; the peak memory grows by one output batch.  ``ensemble=1`` and ``(0,)`` run the plain
    path.  Anything else is a ValueError before any launch."""
    modes = _ensemble_modes("restore_image", ensemble)
    if device is None and not (isinstance(image, torch.Tensor) and image.is_cuda):
        device = _model_device(model)
    img, kind = _checked_image(image)
    out = _restore_device(model, img, device, factor, tile, halo, micro_batch, quantise, modes)
    if kind == "numpy":
        return out.cpu().numpy()
    return out.cpu() if kind == "cpu" else out


# ---------------------------------------------------------------------------
# a list of images in shared window batches
@dataclass(frozen=True)
class ImagePack:
    """The images of one call in one arena: ``arena`` is a 1-D tensor of the images' own dtype, the HWC images
    back to back with no padding (a uint8 image may start at any byte); ``table`` the device int64 [n, 3] rows
    (element offset, H, W) the kernels read; ``host_table`` the same rows as Python ints, which the wrappers
    check before a launch; ``c`` the channels all images share; ``kinds`` what each image came in as ("numpy",
    "cpu", or its GPU device)."""
    arena: torch.Tensor
    table: torch.Tensor
    host_table: Tuple[Tuple[int, int, int], ...]
    c: int
    kinds: Tuple = ()

    def __len__(self) -> int:
        return len(self.host_table)

    def shapes(self) -> List[Tuple[int, int]]:
        return [(h, w) for _, h, w in self.host_table]

    def image(self, i: int) -> torch.Tensor:
        """Image i as an H x W x C view of the arena."""
        off, h, w = self.host_table[i]
        return self.arena[off:off + h * w * self.c].view(h, w, self.c)


def _host_table(shapes: Sequence[Tuple[int, int]], c: int) -> Tuple[Tuple[Tuple[int, int, int], ...], int]:
    rows, off = [], 0
    for h, w in shapes:
        rows.append((off, int(h), int(w)))
        off += int(h) * int(w) * c
    return tuple(rows), off


def pack_images(images: Sequence, device=None) -> ImagePack:
    """Pack H x W x C images (numpy arrays or tensors, possibly of different sizes; one dtype, uint8 or float32,
    and one C) into one arena on ``device`` (default: the first device image's, else the current GPU).  Host
    images are concatenated once on the host and sent in one transfer; device images are copied device to
    device.  ValueError names the offending index."""
    if len(images) < 1:
        raise ValueError("pack_images: no images")
    ts, kinds = [], []
    for i, image in enumerate(images):
        try:
            t, kind = _checked_image(image)
        except ValueError as e:
            raise ValueError(f"pack_images: image {i}: {e}") from None
        if ts and (t.dtype != ts[0].dtype or t.shape[2] != ts[0].shape[2]):
            raise ValueError(f"pack_images: image {i} is {t.dtype} with {t.shape[2]} channel(s); image 0 is "
                             f"{ts[0].dtype} with {ts[0].shape[2]}: one dtype and one C per call")
        ts.append(t)
        kinds.append(t.device if kind == "cuda" else kind)
    if device is None:
        device = next((t.device for t in ts if t.is_cuda), "cuda")
    device = torch.device(device)
    c = int(ts[0].shape[2])
    host_table, total = _host_table([(t.shape[0], t.shape[1]) for t in ts], c)
    on_host = [i for i, t in enumerate(ts) if not t.is_cuda]
    staged = torch.cat([ts[i].reshape(-1) for i in on_host]).to(device) if on_host else None     # one transfer
    if len(on_host) == len(ts):
        arena = staged
    else:
        arena = torch.empty(total, dtype=ts[0].dtype, device=device)
        at = 0
        for i, t in enumerate(ts):
            off, n = host_table[i][0], t.numel()
            if t.is_cuda:
                arena[off:off + n].view(t.shape).copy_(t)
            else:
                arena[off:off + n].copy_(staged[at:at + n])
                at += n
    table = torch.tensor(host_table, dtype=torch.int64).to(device)
    return ImagePack(arena, table, host_table, c, tuple(kinds))


def plan_images(shapes: Sequence[Tuple[int, int]], factor: int = 16, tile: int = TILE, halo: int = HALO,
                micro_batch: int = MICRO_BATCH, modes=None) -> List[Tuple[int, int, Tuple[Tuple[int, ...], ...]]]:
    """The launches of a list of (h, w) images (pure Python): ``plan`` per image, all windows grouped by window
    shape (th, tw) in (image, window) order, each group cut into launches of at most
    max(1, micro_batch tile^2 // (th tw)) windows -- the pixels one restore_image launch has, so the peak
    memory does not grow.  ``modes`` (what ``ensemble`` takes; default: the plain call): a launch is then two
    model calls, one per orientation, and holds at most max(1, micro_batch tile^2 // (th tw Mo)) windows, Mo the
    larger number of modes of one orientation.  Returns [(th, tw, rows)], rows (img, wr, wc, r0, r1, c0, c1).
    ValueError where ``plan`` raises and for bad modes."""
    most = _most_modes(_ensemble_modes("plan_images", modes))
    if micro_batch < 1:
        raise ValueError(f"plan_images: micro_batch must be positive (got {micro_batch})")
    groups = {}
    for i, shape in enumerate(shapes):
        p = plan(int(shape[0]), int(shape[1]), factor, tile, halo)
        groups.setdefault((p.th, p.tw), []).extend((i,) + tuple(w) for w in p.windows)
    launches = []
    for (th, tw), rows in groups.items():
        cap = max(1, (micro_batch * tile * tile) // (th * tw * most))
        launches.extend((th, tw, tuple(rows[k:k + cap])) for k in range(0, len(rows), cap))
    return launches


def _restore_pack(model: Callable, pack: ImagePack, launches, quantise: bool, modes: Tuple[int, ...] = (0,)) -> ImagePack:
    """restore_images on a pack: one launch per launch of plan_images (planned with the same modes); the result
    is a pack of the same image shapes."""
    dev, shapes = pack.arena.device, pack.shapes()
    table = torch.tensor([r for _, _, rows in launches for r in rows], dtype=torch.int32).to(dev)  # one upload

    def sliced():
        at = 0
        for th, tw, rows in launches:
            yield table[at:at + len(rows)], th, tw, _core_px(rows, shapes)
            at += len(rows)

    def alloc(cout: int, dtype) -> ImagePack:
        same = cout == pack.c
        host_table, total = (pack.host_table, pack.arena.numel()) if same else _host_table(shapes, cout)
        return ImagePack(torch.empty(total, dtype=dtype, device=dev),
                         pack.table if same else torch.tensor(host_table, dtype=torch.int64).to(dev),
                         host_table, cout, pack.kinds)

    gather, scatter = _plain_io(partial(kernels.tiles_gather, pack), kernels.tiles_scatter) if modes == (0,) else \
        (partial(kernels.tiles_gather_d8, pack), kernels.tiles_scatter_mean)
    return _run_launches("restore_images", model, sliced(), quantise, gather, alloc, scatter, modes)


def restore_images(model: Callable, images: Sequence, *, factor: int = 16, tile: int = TILE, halo: int = HALO,
                   micro_batch: int = MICRO_BATCH, quantise: bool = True, device=None, ensemble=1) -> list:
    """restore_image for a list of images of possibly different sizes (one dtype, one C), with windows of
    different images sharing the model's batches: the images go to the device in one arena (pack_images), each
    launch of plan_images is one gather, one model call and one scatter, and the results come back from one
    output arena in input order and of each input's kind.  Equal to
    ``[restore_image(model, im, ...) for im in images]`` byte for byte whenever the model's result for a
    window does not depend on what else is in the batch.  ``ensemble`` as in restore_image: windows of different
    images keep sharing launches by window shape (th, tw), and each launch is one even-k and one odd-k model
    call."""
    modes = _ensemble_modes("restore_images", ensemble)
    if device is None and not any(isinstance(im, torch.Tensor) and im.is_cuda for im in images):
        device = _model_device(model)
    pack = pack_images(images, device)
    out = _restore_pack(model, pack, plan_images(pack.shapes(), factor, tile, halo, micro_batch, modes), quantise,
                        modes)
    host = out.arena.cpu() if any(isinstance(k, str) for k in out.kinds) else None      # one transfer back
    results = []
    for i, kind in enumerate(out.kinds):
        if isinstance(kind, str):
            off, h, w = out.host_table[i]
            t = host[off:off + h * w * out.c].view(h, w, out.c)
            results.append(t.numpy() if kind == "numpy" else t)
        else:
            results.append(out.image(i).to(kind))
    return results


def _as_device_u8(x, device, who: str = "psnr_u8") -> torch.Tensor:
    t = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
        raise ValueError(f"{who}: expected uint8 images, got {getattr(t, 'dtype', type(t).__name__)}")
    return t if t.is_cuda and device is None else t.to(device if device is not None else "cuda")


def _psnr(sse: int, n: int) -> float:
    """10 log10(255^2 n / sse) in float64 from an exact integer SSE over n bytes; inf for sse == 0."""
    return float("inf") if sse == 0 else float(10.0 * np.log10(255.0 ** 2 * n / sse))


def _noisy(clean: np.ndarray, sigma: float, rs) -> np.ndarray:
    noisy = clean.copy()
    noisy += rs.normal(0, sigma / 255.0, clean.shape)      # float32 += float64 draws, as validate
    return noisy


def _clean_u8(clean: np.ndarray) -> np.ndarray:
    return np.rint(clean.astype(np.float64) * 255.0).astype(np.uint8)


def _u8_pair(who: str, a, b) -> Tuple[torch.Tensor, torch.Tensor]:
    """Two uint8 images of one shape (numpy or tensor, host or device) as tensors on one GPU."""
    dev = next((t.device for t in (a, b) if isinstance(t, torch.Tensor) and t.is_cuda), None)
    ta, tb = _as_device_u8(a, dev, who), _as_device_u8(b, dev, who)
    if ta.shape != tb.shape:
        raise ValueError(f"{who}: shapes differ ({tuple(ta.shape)} vs {tuple(tb.shape)})")
    return ta, tb.to(ta.device)


def psnr_u8(a, b) -> float:
    """PSNR of two uint8 images of one shape: 10 log10(255^2 N / SSE) in float64 from the exact integer SSE
    (kernels.u8_sse), so it does not depend on any summation order; inf for equal images."""
    ta, tb = _u8_pair("psnr_u8", a, b)
    return _psnr(kernels.u8_sse(ta, tb), ta.numel())


def _ssim(q: int, n: int) -> float:
    """sum q / (2^32 n), one integer true division: the correctly rounded float64 of the exact quotient."""
    return q / (kernels.SSIM_ONE * n)


def ssim_u8(a, b) -> float:
    """SSIM of two uint8 H x W x C images of one shape (numpy or tensor, host or device), as
    ``skimage.metrics.structural_similarity(a, b, gaussian_weights=True, sigma=1.5, use_sample_covariance=False,
    data_range=255, channel_axis=2)`` defines it: 11 x 11 Gaussian window, the mean over the (H - 10)(W - 10) C
    values whose window lies inside the image.  Each value is float64 on the device, quantised to a multiple of
    2^-32 and summed as an integer (kernels.u8_ssim), so the result is within 2^-32 of the float64 mean, the same
    on every run and independent of any summation order; exactly 1.0 for equal images.  ValueError for a side
    below 11."""
    ta, tb = _u8_pair("ssim_u8", a, b)
    if ta.dim() != 3 or not kernels.ssim_ok(ta.shape[2], ta.shape[0], ta.shape[1]):
        raise ValueError(f"ssim_u8: expected H x W x C images with C <= 4 and both sides at least "
                         f"{kernels.SSIM_WINDOW}, got {tuple(ta.shape)}")
    return _ssim(kernels.u8_ssim(ta, tb), kernels.ssim_count(ta.shape[2], ta.shape[0], ta.shape[1]))


def _psnr_y(sse: int, n: int) -> float:
    """10 log10(255^2 LUMA_SCALE^2 n / sse) from the exact integer luma SSE over n pixels: one true division of
    Python ints, the correctly rounded float64 of the exact quotient, then log10; inf for sse == 0."""
    if sse == 0:
        return float("inf")
    return float(10.0 * np.log10((255 ** 2 * kernels.LUMA_SCALE ** 2 * n) / sse))


def _luma_pair(who: str, a, b, need_window: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """_u8_pair for two H x W x 3 images; everything is checked on the host, before any copy or launch."""
    for t in (a, b):
        if not (isinstance(t, (np.ndarray, torch.Tensor)) and t.dtype in (np.uint8, torch.uint8)):
            raise ValueError(f"{who}: expected uint8 images, got {getattr(t, 'dtype', type(t).__name__)}")
    shape = tuple(a.shape)
    if shape != tuple(b.shape):
        raise ValueError(f"{who}: shapes differ ({shape} vs {tuple(b.shape)})")
    if len(shape) != 3 or shape[2] != 3:
        raise ValueError(f"{who}: the luma is defined for H x W x 3 images (R, G, B), got {shape}")
    if not kernels.luma_ok(shape[0], shape[1], need_window):
        raise ValueError(f"{who}: expected H x W x 3 images with both sides at least "
                         f"{kernels.SSIM_WINDOW if need_window else 1} and below 2^31 elements, got {shape}")
    return _u8_pair(who, a, b)


def psnr_y_u8(a, b) -> float:
    """PSNR on the Y channel of two uint8 H x W x 3 RGB images of one shape (numpy or tensor, host or device): Y of
    ITU-R BT.601 "studio range" YCbCr as MATLAB's rgb2ycbcr and BasicSR's to_y_channel define it, not rounded to
    uint8, Y = 16 + (65.481 R + 128.553 G + 24.966 B) / 255; 10 log10(255^2 N / sum (Ya - Yb)^2) from the exact
    integer sum (kernels.u8_luma_sse), so it does not depend on any summation order; inf for equal images.
    ValueError for an image that is not 3-channel."""
    ta, tb = _luma_pair("psnr_y_u8", a, b, False)
    return _psnr_y(kernels.u8_luma_sse(ta, tb), ta.shape[0] * ta.shape[1])


def ssim_y_u8(a, b) -> float:
    """ssim_u8's SSIM of the single plane Y (psnr_y_u8's luma, float64) of two uint8 H x W x 3 RGB images: the mean
    over the (H - 10)(W - 10) valid positions, within 2^-32 of the float64 mean, the same on every run; exactly 1.0
    for equal images.  ValueError for an image that is not 3-channel or has a side below 11."""
    ta, tb = _luma_pair("ssim_y_u8", a, b, True)
    return _ssim(kernels.u8_luma_ssim(ta, tb), kernels.luma_ssim_count(ta.shape[0], ta.shape[1]))


def _psnrb(sse: int, h: int, w: int, c: int, sums) -> float:
    """PSNR-B from the exact integers: D_b = S_b / N_b and D_n = S_n / N_n are single true divisions of Python ints,
    BEF = (3 / log2 min(H, W)) (D_b - D_n) where D_b > D_n, else 0; 10 log10(255^2 / (SSE / (H W C) + BEF)) in
    float64, inf for a zero denominator."""
    sb, nb, sn, nn = sums
    db, dn = sb / nb, sn / nn
    bef = 3.0 / math.log2(min(h, w)) * (db - dn) if db > dn else 0.0
    den = sse / (h * w * c) + bef
    return float("inf") if den == 0 else 10.0 * math.log10(255.0 ** 2 / den)


def _check_psnrb_shape(who: str, what: str, shape) -> None:
    shape = tuple(shape)
    if len(shape) != 3 or min(shape[:2]) < kernels.PSNRB_MIN_SIDE:
        raise ValueError(f"{who}: {what} is {shape}; PSNR-B needs an H x W x C image with both sides at least "
                         f"{kernels.PSNRB_MIN_SIDE}")


def psnrb_u8(est, ref) -> float:
    """PSNR-B (Yim and Bovik) of the uint8 H x W x C picture ``est`` against ``ref`` of the same shape (numpy or
    tensor, host or device), both sides at least 16: the PSNR with the blocking effect factor of ``est`` on the
    8 x 8 grid from (0, 0) added to the mean squared error (include/grr.h has the definition; the pair counts are
    the true numbers of pairs).  From exact integers -- kernels.u8_sse and kernels.u8_blocking -- so it does not
    depend on any summation order; inf for equal pictures without blocking.  Not symmetric: the factor is ``est``'s."""
    for t in (est, ref):
        if not (isinstance(t, (np.ndarray, torch.Tensor)) and t.dtype in (np.uint8, torch.uint8)):
            raise ValueError(f"psnrb_u8: expected uint8 images, got {getattr(t, 'dtype', type(t).__name__)}")
    if tuple(est.shape) != tuple(ref.shape):
        raise ValueError(f"psnrb_u8: shapes differ ({tuple(est.shape)} vs {tuple(ref.shape)})")
    _check_psnrb_shape("psnrb_u8", "the picture", est.shape)
    ta, tb = _u8_pair("psnrb_u8", est, ref)
    h, w, c = ta.shape
    return _psnrb(kernels.u8_sse(ta, tb), h, w, c, kernels.u8_blocking(ta))


METRICS = ("psnr", "ssim", "psnr_y", "ssim_y")
BLOCKING_METRICS = ("psnrb",)       # beside them: the metric of compression-artifact removal
_SCORE = {"psnr": psnr_u8, "ssim": ssim_u8, "psnr_y": psnr_y_u8, "ssim_y": ssim_y_u8,      # per image, by name
          "psnrb": psnrb_u8}


def _check_metric_shape(who: str, what: str, shape, metrics) -> None:
    """ValueError naming the image where a metric asked for has no value on an image of this shape."""
    shape = tuple(shape)
    window = "ssim" in metrics or "ssim_y" in metrics
    if window and (len(shape) != 3 or min(shape[:2]) < kernels.SSIM_WINDOW):
        raise ValueError(f"{who}: {what} is {shape}; SSIM needs an H x W x C image with both sides at "
                         f"least {kernels.SSIM_WINDOW}")
    if ("psnr_y" in metrics or "ssim_y" in metrics) and (len(shape) != 3 or shape[2] != 3):
        raise ValueError(f"{who}: {what} is {shape}; the Y-channel metrics need an H x W x 3 image (R, G, B)")
    if "psnrb" in metrics:
        _check_psnrb_shape(who, what, shape)


def _evaluate_args(who: str, model: Callable, ensemble, metrics, tiling_args: dict, extra: Tuple[str, ...] = ()):
    """(modes, metrics, device, tile, halo, micro_batch) of an evaluate call, checked; tiling_args is emptied.
    ``extra``: metric names the caller scores itself, beside the shared ones."""
    modes = _ensemble_modes(who, ensemble)
    metrics = (metrics,) if isinstance(metrics, str) else tuple(metrics)
    names = METRICS + BLOCKING_METRICS + tuple(extra)
    if not metrics or any(m not in names for m in metrics) or len(set(metrics)) != len(metrics):
        raise ValueError(f"{who}: metrics are distinct names of {names}, got {metrics!r}")
    device = tiling_args.pop("device", None) or _model_device(model)
    tile, halo = tiling_args.pop("tile", TILE), tiling_args.pop("halo", HALO)
    micro_batch = tiling_args.pop("micro_batch", MICRO_BATCH)
    if tiling_args:
        raise TypeError(f"{who}: unexpected arguments {sorted(tiling_args)}")
    return modes, metrics, device, tile, halo, micro_batch


def _means(values: dict, metrics) -> dict:
    """{metric: (mean, per-image values)}: what every evaluate function returns."""
    return {m: (float(np.mean(values[m])), values[m]) for m in metrics}


def _evaluate(who: str, model: Callable, images, sigma: float, factor: int, seed: int, across_images: bool, ensemble,
              metrics, tiling_args: dict) -> dict:
    """The one body of evaluate and evaluate_metrics: {metric: (mean, per-image values)} for the metrics asked
    for.  The draws, the restorations and the launches of one metric do not depend on which others are asked
    for."""
    modes, metrics, device, tile, halo, micro_batch = _evaluate_args(who, model, ensemble, metrics, tiling_args)
    if set(metrics) - {"psnr"}:       # before any draw
        for i in range(len(images)):
            _check_metric_shape(who, f"image {i}", np.shape(images[i]), metrics)
    rs = np.random.RandomState(seed=seed)
    if across_images:
        values = _evaluate_across(model, images, sigma, factor, rs, tile, halo, micro_batch, device, modes, metrics)
    else:
        values = {m: [] for m in metrics}
        for i in range(len(images)):
            clean = np.asarray(images[i], dtype=np.float32)
            img, _ = _checked_image(_noisy(clean, sigma, rs))
            restored = _restore_device(model, img, device, factor, tile, halo, micro_batch, True, modes)
            clean_u8 = torch.from_numpy(_clean_u8(clean)).to(restored.device)
            for m in metrics:
                values[m].append(_SCORE[m](restored, clean_u8))
    return _means(values, metrics)


def evaluate(model: Callable, images, sigma: float = 25.0, factor: int = 16, seed: int = 2204,
             across_images: bool = False, ensemble=1, **tiling_args) -> Tuple[float, List[float]]:
    """``training.validate``'s loop on restore_image: per image, N(0, sigma/255) noise drawn on the host from
    one RandomState(seed) stream in image order, the noisy float image restored, PSNR against
    rint(clean x 255).  Returns (mean PSNR, per-image PSNRs).  tiling_args: tile, halo, micro_batch, device.

    ``across_images``: draw the noise for all images first (the same stream, so the same draws), restore them
    with restore_images in shared window batches and take every image's SSE in one launch; the same floats
    for a batch-independent model.  ``ensemble`` as in restore_image, on either branch."""
    return _evaluate("evaluate", model, images, sigma, factor, seed, across_images, ensemble, ("psnr",),
                     tiling_args)["psnr"]


def evaluate_metrics(model: Callable, images, sigma: float = 25.0, factor: int = 16, seed: int = 2204,
                     across_images: bool = False, ensemble=1, metrics=("psnr", "ssim"), **tiling_args) -> dict:
    """``evaluate`` for several metrics of the same restorations: {"psnr": (mean, per-image), "ssim": (mean,
    per-image)} for the names in ``metrics``.  The "psnr" entry is evaluate's result bit for bit (one body, the
    same draws); "ssim" is ssim_u8 of each restored image against rint(clean x 255).  With ``across_images`` the
    SSIM of all images is one kernels.u8_ssim_images launch on the restored and the clean arena.  "psnr_y" and
    "ssim_y" are psnr_y_u8 and ssim_y_u8, the two on the Y channel of RGB images, with one
    kernels.u8_luma_sse_images / u8_luma_ssim_images launch each across images; a metric's value does not depend on
    which others are asked for.  An unknown metric name, with "ssim" or "ssim_y" an image with a side below 11 and
    with a "_y" metric an image that is not 3-channel is a ValueError before any draw."""
    return _evaluate("evaluate_metrics", model, images, sigma, factor, seed, across_images, ensemble, metrics,
                     tiling_args)


def _evaluate_across(model, images, sigma, factor, rs, tile, halo, micro_batch, device, modes=(0,),
                     metrics=("psnr",)) -> dict:
    """_evaluate(across_images=True): the same draws, the same uint8 images and the same integer sums as the
    per-image loop, with the windows of all images in shared batches and one launch per metric.  Returns
    {metric: per-image values}."""
    cleans = [np.asarray(images[i], dtype=np.float32) for i in range(len(images))]
    pack = pack_images([_noisy(clean, sigma, rs) for clean in cleans], device)     # all draws first, in image order
    restored = _restore_pack(model, pack, plan_images(pack.shapes(), factor, tile, halo, micro_batch, modes), True,
                             modes)
    return _score_packs("evaluate", restored, pack_images([_clean_u8(c) for c in cleans], restored.arena.device), metrics)


def _score_packs(who: str, restored: ImagePack, clean_u8: ImagePack, metrics) -> dict:
    """{metric: per-image values} of a restored uint8 pack against the pack of what it should be: one launch per
    metric."""
    if clean_u8.host_table != restored.host_table:
        raise ValueError(f"{who}: the model returns {restored.c} channel(s) for {clean_u8.c}; no PSNR")
    values = {}
    if "psnr" in metrics:
        offsets = [off for off, _, _ in restored.host_table] + [restored.arena.numel()]
        sses = kernels.u8_sse_segments(restored.arena, clean_u8.arena, offsets)
        values["psnr"] = [_psnr(sse, h * w * restored.c) for sse, (_, h, w) in zip(sses, restored.host_table)]
    if "ssim" in metrics:
        qs = kernels.u8_ssim_images(restored, clean_u8)
        values["ssim"] = [_ssim(q, kernels.ssim_count(restored.c, h, w)) for q, (_, h, w) in zip(qs, restored.host_table)]
    if "psnr_y" in metrics:
        sses = kernels.u8_luma_sse_images(restored, clean_u8)
        values["psnr_y"] = [_psnr_y(sse, h * w) for sse, (_, h, w) in zip(sses, restored.host_table)]
    if "ssim_y" in metrics:
        qs = kernels.u8_luma_ssim_images(restored, clean_u8)
        values["ssim_y"] = [_ssim(q, kernels.luma_ssim_count(h, w)) for q, (_, h, w) in zip(qs, restored.host_table)]
    if "psnrb" in metrics:
        offsets = [off for off, _, _ in restored.host_table] + [restored.arena.numel()]
        sses = kernels.u8_sse_segments(restored.arena, clean_u8.arena, offsets)
        values["psnrb"] = [_psnrb(sse, h, w, restored.c, sums) for sse, sums, (_, h, w) in
                           zip(sses, kernels.u8_blocking_images(restored), restored.host_table)]
    return values


class _Protocol(NamedTuple):
    """A degrade-from-clean evaluation protocol: take a clean uint8 picture, crop it, degrade it on the device, restore,
    shave, score.  The record holds what evaluate_sr, evaluate_car, evaluate_demosaic and evaluate_deblur differ in
    (_sr_protocol, _car_protocol, _demosaic_protocol and _deblur_protocol build it, parameters checked);
    _evaluate_degraded is the one loop they share,
    and the restore.py command takes its crop, degradation, shave and label from the same record."""
    who: str                # the caller its refusals name
    label: str              # the protocol and its parameters in a few words: the command's "against" text
    defined_on: str         # "image i is float32; {defined_on} uint8 pictures"
    admit: Callable         # admit(i, t) raises the protocol's refusal of a uint8 H x W x C picture it does not take
    crop: Callable          # crop(h, w) -> the (h, w) kept from the top left
    shave: int              # border pixels cut from the restored and the clean picture before scoring
    left_after: str         # "image i is (shape): nothing is left {left_after}"
    scored: str             # what the metrics' refusals call the scored picture i, "image {i}" formatted
    degrade: Callable       # the cropped clean picture on the device -> the model's input, there too

    def shaved(self, a):
        """``a`` (H x W x C, array or tensor) without the shave's border: a view."""
        n = self.shave
        return a[n:a.shape[0] - n, n:a.shape[1] - n] if n else a


def _check_shave(who: str, shave) -> int:
    if isinstance(shave, bool) or not isinstance(shave, int) or shave < 0:
        raise ValueError(f"{who}: shave is a non-negative integer, got {shave!r}")
    return shave


def _sr_protocol(who: str, scale, shave) -> _Protocol:
    """Bicubic super-resolution: mod-crop to multiples of ``scale``, the bicubic down and back up, a shave of
    ``shave`` (default ``scale``)."""
    scale = kernels._check_scale(who, scale)
    shave = _check_shave(who, scale if shave is None else shave)
    return _Protocol(who, label=f"bicubic x{scale} shave {shave}", defined_on="the protocol is defined on",
                     admit=lambda i, t: None, crop=lambda h, w: (h // scale * scale, w // scale * scale), shave=shave,
                     left_after=f"after the crop to multiples of {scale} and a shave of {shave}",
                     scored="image {i} after the shave", degrade=lambda clean: kernels.u8_bicubic_degrade(clean, scale))


def _car_protocol(who: str, quality, subsampling) -> _Protocol:
    """JPEG compression-artifact removal: the whole picture through the JPEG round trip, no shave."""
    quality = kernels._check_quality(who, quality)
    subsampling = kernels._check_subsampling(who, subsampling)

    def admit(i, t):
        if not kernels.jpeg_ok(t.shape[2], t.shape[0], t.shape[1], subsampling):
            raise ValueError(f"{who}: image {i} is {tuple(t.shape)}; JPEG takes 1 or 3 channels (gray or R, G, B)")

    return _Protocol(who, label=f"jpeg q{quality} {'4:2:0' if subsampling else '4:4:4'}", defined_on="JPEG is defined on",
                     admit=admit, crop=lambda h, w: (h, w), shave=0, left_after="", scored="image {i}",
                     degrade=lambda clean: kernels.u8_jpeg(clean, quality, subsampling))


def _demosaic_protocol(who: str, pattern, fill, shave) -> _Protocol:
    """Bayer demosaicking: the whole R, G, B picture mosaicked and filled, a shave of ``shave``."""
    pattern, fill = kernels._check_pattern(who, pattern), kernels._check_fill(who, fill)
    shave = _check_shave(who, shave)

    def admit(i, t):
        if t.shape[2] != 3 or not kernels.demosaic_ok(3, t.shape[0], t.shape[1]):
            raise ValueError(f"{who}: image {i} is {tuple(t.shape)}; the protocol takes clean R, G, B pictures")

    return _Protocol(who, label=f"bayer {kernels.DEMOSAIC_PATTERNS[pattern]} {kernels.DEMOSAIC_FILLS[fill]} shave {shave}",
                     defined_on="the mosaic is defined on", admit=admit, crop=lambda h, w: (h, w), shave=shave,
                     left_after=f"after a shave of {shave}", scored="image {i} after the shave",
                     degrade=lambda clean: kernels.u8_demosaic(clean, pattern, fill))


def _evaluate_degraded(p: _Protocol, model: Callable, images, factor: int, modes, metrics, device, tile, halo,
                       micro_batch) -> dict:
    """The one body of evaluate_sr, evaluate_car and evaluate_demosaic, after _evaluate_args and the protocol's own
    checks: every picture is checked before any launch; then per picture degrade, restore, shave, score."""
    who = p.who
    if len(images) < 1:
        raise ValueError(f"{who}: no images")
    cleans = []
    for i in range(len(images)):
        try:
            t, _ = _checked_image(images[i])
        except ValueError as e:
            raise ValueError(f"{who}: image {i}: {e}") from None
        if t.dtype != torch.uint8:
            raise ValueError(f"{who}: image {i} is {t.dtype}; {p.defined_on} uint8 pictures")
        p.admit(i, t)
        h, w = p.crop(t.shape[0], t.shape[1])
        if min(h, w) <= 2 * p.shave:        # with no shave: a side the crop leaves nothing of
            raise ValueError(f"{who}: image {i} is {tuple(t.shape)}: nothing is left {p.left_after}")
        _check_metric_shape(who, p.scored.format(i=i), (h - 2 * p.shave, w - 2 * p.shave, t.shape[2]), metrics)
        plan(h, w, factor, tile, halo)                          # raises what the restoration would
        cleans.append(t[:h, :w])
    if device is None:
        device = next((t.device for t in cleans if t.is_cuda), None)
    values = {m: [] for m in metrics}
    for t in cleans:
        clean = _to_device(t, device)
        restored = _restore_device(model, p.degrade(clean), None, factor, tile, halo, micro_batch, True, modes)
        if restored.shape != clean.shape:
            raise ValueError(f"{who}: the model returns {restored.shape[2]} channel(s) for {clean.shape[2]}; no score")
        # the shave is an ATen slice and copy: a few hundred kilobytes per picture, not a hot path
        restored, clean = p.shaved(restored).contiguous(), p.shaved(clean).contiguous()
        for m in metrics:
            values[m].append(_SCORE[m](restored, clean))
    return _means(values, metrics)


def _resized_u8(who: str, a, resize):
    """``resize`` (device uint8 H x W x C -> device uint8) of a uint8 picture, numpy array or tensor, host or device;
    the result is of the input's kind and, for a tensor, on its device."""
    try:
        t, kind = _checked_image(a)
    except ValueError as e:
        raise ValueError(f"{who}: {e}") from None
    if t.dtype != torch.uint8:
        raise ValueError(f"{who}: expected a uint8 picture, got {t.dtype}")
    out = resize(_to_device(t, None))
    if kind == "numpy":
        return out.cpu().numpy()
    return out.cpu() if kind == "cpu" else out


def bicubic_down_u8(a, s: int):
    """The uint8 H x W x C picture ``a`` (numpy array or tensor) shrunk to ceil(H / s) x ceil(W / s) by the exact
    antialiased bicubic (kernels.u8_resize; include/grr.h has the definition), on the GPU."""
    return _resized_u8("bicubic_down_u8", a, lambda t: kernels.u8_resize(t, s, False))


def bicubic_up_u8(a, s: int, h: int = None, w: int = None):
    """``a`` grown to s H x s W by the exact bicubic, or to h x w with s (H - 1) < h <= s H and likewise w (the
    size a bicubic_down_u8 came from), on the GPU."""
    s = kernels._check_scale("bicubic_up_u8", s)
    return _resized_u8("bicubic_up_u8", a, lambda t: kernels.u8_resize(
        t, s, True, (s * t.shape[0] if h is None else h, s * t.shape[1] if w is None else w)))


def bicubic_degrade_u8(a, s: int):
    """The bicubic super-resolution input of ``a`` at its own size: bicubic_up_u8(bicubic_down_u8(a, s), s, H, W),
    without the round trip to the host (kernels.u8_bicubic_degrade).  training.bicubic_degrade_u8 gives the same
    bytes on the CPU."""
    return _resized_u8("bicubic_degrade_u8", a, lambda t: kernels.u8_bicubic_degrade(t, s))


def evaluate_sr(model: Callable, images, scale: int, shave: int = None, factor: int = 16, ensemble=1,
                metrics=("psnr_y", "ssim_y"), **tiling_args) -> dict:
    """Score ``model`` on the bicubic super-resolution protocol (Set5 / Set14 / B100 style) over clean uint8
    H x W x C pictures (numpy arrays or tensors, host or device).  Per picture: mod-crop it to multiples of ``scale``
    (top-left), degrade it on the device (kernels.u8_bicubic_degrade: the exact antialiased bicubic down and the
    bicubic back up), restore the degraded picture as ``restore_image(..., quantise=True)`` does, cut ``shave``
    (default ``scale``) pixels from each side of the restored and the clean picture and score them with the
    exact-integer kernels.  Returns {metric: (mean, per-image values)} as evaluate_pairs does; with ``shave=0`` on
    pictures that need no mod-crop it is evaluate_pairs(model, degraded, clean) bit for bit.  tiling_args: tile,
    halo, micro_batch, device; ``ensemble`` as in restore_image.

    Everything is checked before any launch: the scale (2..8), the shave, uint8 pictures, a picture smaller than
    ``scale`` or than the shave leaves, and what the metrics need of the shaved picture (SSIM: both sides at least
    11; the Y-channel metrics: 3 channels)."""
    modes, metrics, device, tile, halo, micro_batch = _evaluate_args("evaluate_sr", model, ensemble, metrics, tiling_args)
    return _evaluate_degraded(_sr_protocol("evaluate_sr", scale, shave), model, images, factor, modes, metrics, device,
                              tile, halo, micro_batch)


def jpeg_degrade_u8(a, quality: int, subsampling: int = 0):
    """The JPEG round trip of the uint8 H x W x C picture ``a`` (numpy array or tensor, C of 1 or 3) at ``quality``
    (1..100), on the GPU: what decoding its baseline JPEG gives, byte for byte as Pillow (libjpeg-turbo) computes
    it, without a bitstream (kernels.u8_jpeg; include/grr.h has the definition).  ``subsampling``: 0 for 4:4:4, 2 for
    4:2:0.  training.jpeg_degrade_u8 gives the same bytes on the CPU."""
    quality = kernels._check_quality("jpeg_degrade_u8", quality)           # before any transfer
    subsampling = kernels._check_subsampling("jpeg_degrade_u8", subsampling)
    return _resized_u8("jpeg_degrade_u8", a, lambda t: kernels.u8_jpeg(t, quality, subsampling))


def evaluate_car(model: Callable, images, quality: int, subsampling: int = 0, factor: int = 16, ensemble=1,
                 metrics=("psnr", "ssim", "psnrb"), **tiling_args) -> dict:
    """Score ``model`` on JPEG compression-artifact removal (the protocol of the LIVE1 / Classic5 / BSDS500 tables)
    over clean uint8 H x W x C pictures (numpy arrays or tensors, host or device; C of 1 or 3).  Per picture: the
    JPEG round trip at ``quality`` on the device (kernels.u8_jpeg), the degraded picture restored as
    ``restore_image(..., quantise=True)`` does, and the result scored against the clean picture with the
    exact-integer kernels.  Returns {metric: (mean, per-image values)} as evaluate_pairs does; it is
    evaluate_pairs(model, degraded, clean) bit for bit.  tiling_args: tile, halo, micro_batch, device; ``ensemble`` as
    in restore_image.

    Everything is checked before any launch: the quality (1..100), the subsampling (0 or 2), uint8 pictures of 1 or
    3 channels, and what the metrics need of a picture (SSIM: both sides at least 11; PSNR-B: at least 16; the
    Y-channel metrics: 3 channels)."""
    modes, metrics, device, tile, halo, micro_batch = _evaluate_args("evaluate_car", model, ensemble, metrics, tiling_args)
    return _evaluate_degraded(_car_protocol("evaluate_car", quality, subsampling), model, images, factor, modes, metrics,
                              device, tile, halo, micro_batch)


def demosaic_u8(a, pattern, fill="malvar"):
    """The Bayer mosaic of the uint8 picture ``a`` with its missing channels filled, H x W x 3, on the GPU
    (kernels.u8_demosaic; include/grr.h has the definition).  ``a``: a numpy array or a tensor, host or device, of
    H x W x 3 (R, G, B; the mosaic keeps the site's channel of each pixel) or H x W x 1 or H x W (a raw mosaic plane);
    the result is of the same kind.  ``pattern``: "rggb", "grbg", "gbrg" or "bggr" (or the code 0..3); ``fill``:
    "zero", "bilinear" or "malvar" (or 0..2).  training.demosaic_degrade_u8 gives the same bytes on the CPU."""
    pattern = kernels._check_pattern("demosaic_u8", pattern)               # before any transfer
    fill = kernels._check_fill("demosaic_u8", fill)
    if isinstance(a, (np.ndarray, torch.Tensor)) and a.ndim == 2:
        a = a[:, :, None]
    if isinstance(a, (np.ndarray, torch.Tensor)) and a.ndim == 3 and a.shape[2] not in (1, 3):
        raise ValueError(f"demosaic_u8: needs 1 channel (the mosaic) or 3 (R, G, B), got {tuple(a.shape)}")
    return _resized_u8("demosaic_u8", a, lambda t: kernels.u8_demosaic(t, pattern, fill))


def evaluate_demosaic(model: Callable, images, pattern="rggb", fill="malvar", shave: int = 0, factor: int = 16,
                      ensemble=1, metrics=("psnr", "ssim"), **tiling_args) -> dict:
    """Score ``model`` on Bayer demosaicking (the protocol of the Kodak / McMaster tables) over clean uint8
    H x W x 3 pictures (numpy arrays or tensors, host or device).  Per picture: mosaic and fill on the device
    (kernels.u8_demosaic), the filled picture restored as ``restore_image(..., quantise=True)`` does, ``shave``
    pixels cut from each side of the restored and the clean picture, and the two scored with the exact-integer
    kernels.  "psnr" is taken over the three channels together: the CPSNR of the demosaicking tables.  Returns
    {metric: (mean, per-image values)} as evaluate_pairs does; with ``shave=0`` it is
    evaluate_pairs(model, filled, clean) bit for bit.  tiling_args: tile, halo, micro_batch, device; ``ensemble`` as
    in restore_image.

    Everything is checked before any launch: the pattern, the fill, the shave, uint8 pictures of 3 channels, a
    picture smaller than the shave leaves, and what the metrics need of the shaved picture (SSIM: both sides at
    least 11; PSNR-B: at least 16)."""
    modes, metrics, device, tile, halo, micro_batch = _evaluate_args("evaluate_demosaic", model, ensemble, metrics,
                                                                     tiling_args)
    return _evaluate_degraded(_demosaic_protocol("evaluate_demosaic", pattern, fill, shave), model, images, factor, modes,
                              metrics, device, tile, halo, micro_batch)


def _raw_noise_args(who: str, pattern, fill, shot, read, bits, clip, seed):
    """(pattern code, fill code, a, b, bits, clip, seed) of a joint denoising and demosaicking call, checked in this
    order; (a, b) is the kernel's float32 noise pair of the shot gain and the read level (kernels.raw_noise_pair)."""
    pattern, fill = kernels._check_pattern(who, pattern), kernels._check_fill(who, fill)
    a, b = kernels.raw_noise_pair(who, shot, read)
    bits = kernels._check_bits(who, bits)
    if not isinstance(clip, (bool, np.bool_)):
        raise ValueError(f"{who}: clip is True or False, got {clip!r}")
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed < 2 ** 64:
        raise ValueError(f"{who}: seed is an integer of 0..2^64 - 1, got {seed!r}")
    return pattern, fill, a, b, bits, bool(clip), int(seed)


def raw_noise_demosaic_u8(a, pattern="rggb", fill="malvar", shot: float = 0.0, read: float = 0.0, bits: int = 16,
                          clip: bool = True, seed: int = 2204, sample_id: int = 0):
    """The input of joint denoising and demosaicking of the uint8 H x W x 3 picture ``a`` (numpy array or tensor, host
    or device), float32 H x W x 3 of the same kind, on the GPU (kernels.u8_raw_noise_demosaic; include/grr.h has the
    definition): the Bayer mosaic of ``a`` with sensor noise of variance ``shot`` x + (``read`` / 255)^2 on it -- ``shot``
    in 0..1, ``read`` in 8-bit levels 0..255 -- clipped to [0, 1] if ``clip``, quantised to ``bits`` (8..16) bits and
    then filled by ``fill``.  The noise is a function of (seed, sample_id, pixel) alone.  With shot = read = 0 and
    bits = 8 it is demosaic_u8 before its rounding to bytes."""
    who = "raw_noise_demosaic_u8"
    pattern, fill, na, nb, bits, clip, seed = _raw_noise_args(who, pattern, fill, shot, read, bits, clip, seed)
    if isinstance(sample_id, bool) or not isinstance(sample_id, (int, np.integer)) or not -2 ** 63 <= sample_id < 2 ** 63:
        raise ValueError(f"{who}: sample_id is a 64-bit integer, got {sample_id!r}")
    if isinstance(a, (np.ndarray, torch.Tensor)) and a.ndim == 3 and a.shape[2] != 3:
        raise ValueError(f"{who}: needs 3 channels (R, G, B), got {tuple(a.shape)}")
    return _resized_u8(who, a, lambda t: kernels.u8_raw_noise_demosaic(t, pattern, fill, na, nb, bits, clip, seed,
                                                                       int(sample_id)))


def _jdd_protocol(who: str, pattern, fill, shot, read, bits, clip, seed, shave) -> _Protocol:
    """Joint denoising and demosaicking: the whole R, G, B picture mosaicked, noised on the mosaic, quantised and
    filled, a shave of ``shave``.  The model's input is float32 and not quantised; picture i of the call has sample id
    i, so its noise is a function of (seed, i) and does not depend on the pictures before it."""
    pattern, fill, a, b, bits, clip, seed = _raw_noise_args(who, pattern, fill, shot, read, bits, clip, seed)
    shave = _check_shave(who, shave)
    count = iter(range(1 << 62))        # degrade is called once per picture, in picture order

    def admit(i, t):
        if t.shape[2] != 3 or not kernels.raw_noise_demosaic_ok(t.shape[0], t.shape[1]):
            raise ValueError(f"{who}: image {i} is {tuple(t.shape)}; the protocol takes clean R, G, B pictures")

    label = f"bayer {kernels.DEMOSAIC_PATTERNS[pattern]} {kernels.DEMOSAIC_FILLS[fill]} raw noise shot {float(shot):g} " \
            f"read {float(read):g} {bits} bits{'' if clip else ' unclipped'} shave {shave}"
    return _Protocol(who, label=label, defined_on="the mosaic is defined on", admit=admit, crop=lambda h, w: (h, w),
                     shave=shave, left_after=f"after a shave of {shave}", scored="image {i} after the shave",
                     degrade=lambda clean: kernels.u8_raw_noise_demosaic(clean, pattern, fill, a, b, bits, clip, seed,
                                                                         next(count)))


def evaluate_jdd(model: Callable, images, pattern="rggb", fill="malvar", shot: float = 0.0, read: float = 0.0,
                 bits: int = 16, clip: bool = True, seed: int = 2204, shave: int = 0, factor: int = 16, ensemble=1,
                 metrics=("psnr", "ssim"), **tiling_args) -> dict:
    """Score ``model`` on joint denoising and demosaicking (the protocol of the Gharbi et al. / Kodak / McMaster
    tables) over clean uint8 H x W x 3 pictures (numpy arrays or tensors, host or device).  Per picture i: the Bayer
    mosaic with sensor noise of variance ``shot`` x + (``read`` / 255)^2 on it (``read`` in 8-bit levels), clipped if
    ``clip``, quantised to ``bits`` bits and filled on the device (kernels.u8_raw_noise_demosaic, sample id i under
    ``seed``), that float32 picture restored as ``restore_image(..., quantise=True)`` does, ``shave`` pixels cut from
    each side of the restored and the clean picture, and the two scored with the exact-integer kernels.  "psnr" is the
    CPSNR.  Returns {metric: (mean, per-image values)} as evaluate_pairs does.  Nothing is drawn on the host: a
    picture's noise is a function of (seed, i), so a score does not depend on the pictures before it.  tiling_args:
    tile, halo, micro_batch, device; ``ensemble`` as in restore_image.

    Everything is checked before any launch: the shared arguments, then the pattern, the fill, shot, read, bits, the
    seed, the shave, uint8 pictures of 3 channels, a picture smaller than the shave leaves, and what the metrics need
    of the shaved picture."""
    modes, metrics, device, tile, halo, micro_batch = _evaluate_args("evaluate_jdd", model, ensemble, metrics, tiling_args)
    return _evaluate_degraded(_jdd_protocol("evaluate_jdd", pattern, fill, shot, read, bits, clip, seed, shave), model,
                              images, factor, modes, metrics, device, tile, halo, micro_batch)


INPAINT_METRICS = ("psnr_missing",)      # beside METRICS: the PSNR over the missing pixels alone


def _check_passes(who: str, passes) -> int:
    if isinstance(passes, (bool, np.bool_)) or not isinstance(passes, (int, np.integer)) or passes < 1:
        raise ValueError(f"{who}: passes is a positive integer, got {passes!r}")
    return int(passes)


def _mask_fill_args(who: str, fill, weights, hole, seed, sample_id, passes):
    """(weight table, fill code, hole, seed, sample id, passes) of a mask fill, checked in this order."""
    fill = kernels._check_mask_fill(who, fill)
    table = kernels._check_mask_table(who, kernels.mask_weights(7) if weights is None else weights)
    hole = kernels._check_hole(who, hole)
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed < 2 ** 64:
        raise ValueError(f"{who}: seed is an integer of 0..2^64 - 1, got {seed!r}")
    if isinstance(sample_id, bool) or not isinstance(sample_id, (int, np.integer)) or not -2 ** 63 <= sample_id < 2 ** 63:
        raise ValueError(f"{who}: sample_id is a 64-bit integer, got {sample_id!r}")
    return table, fill, hole, int(seed), int(sample_id), _check_passes(who, passes)


def _mask_fill_device(t: torch.Tensor, mask: Optional[torch.Tensor], units: int, table, fill: int, hole: int, seed: int,
                      sample_id: int, passes: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(filled, known) on the device: kernels.u8_mask_fill ``passes`` times, each pass taking the last one's picture
    and mask; ``known`` is the uint8 0 / 1 plane of what was known before the first."""
    out, code = kernels.u8_mask_fill(t, mask, units, table, fill, hole, seed, sample_id)
    known = ((code == 1) if mask is None else (mask != 0)).to(torch.uint8)
    for _ in range(passes - 1):
        out, code = kernels.u8_mask_fill(out, code, 0, table, fill, hole, seed, sample_id)
    return out, known


def mask_fill_u8(a, mask=None, keep=None, fill="conv", weights=None, hole: int = 128, seed: int = 2204,
                 sample_id: int = 0, passes: int = 1):
    """(filled, mask) of the uint8 H x W x C picture ``a`` (numpy array or tensor, host or device), both of its kind, on
    the GPU (kernels.u8_mask_fill; include/grr.h has the definition): the missing pixels of ``a`` filled for a
    restoration model.  Exactly one of ``mask`` and ``keep`` is given.  ``mask``: H x W, nonzero (or True) where the
    pixel is known -- scratches, text, a mask file.  ``keep``: the known share of 0..1; the mask is then drawn, a
    function of (seed, sample_id, pixel) alone.  ``fill``: "zero", or "conv", the normalised convolution of the known
    pixels under the uint8 table ``weights`` (kernels.mask_weights; None: flat 7 x 7), ``hole`` where no known pixel
    lies under the table.  ``passes``: each further pass takes the filled pixels as known and so grows the filled
    region by the table's radius.  The mask returned is the uint8 0 / 1 plane of the pixels known at the start."""
    who = "mask_fill_u8"
    if (mask is None) == (keep is None):
        raise ValueError(f"{who}: exactly one of mask and keep is given")
    table, fill, hole, seed, sample_id, passes = _mask_fill_args(who, fill, weights, hole, seed, sample_id, passes)
    units = 0
    if keep is not None:
        try:
            units = kernels.keep_units(keep)
        except ValueError:
            raise ValueError(f"{who}: keep is the known share, a number of 0..1, got {keep!r}") from None
    try:
        t, kind = _checked_image(a)
    except ValueError as e:
        raise ValueError(f"{who}: {e}") from None
    if t.dtype != torch.uint8:
        raise ValueError(f"{who}: expected a uint8 picture, got {t.dtype}")
    m = None
    if mask is not None:
        m = torch.from_numpy(np.ascontiguousarray(mask)) if isinstance(mask, np.ndarray) else mask
        if not isinstance(m, torch.Tensor) or m.dtype not in (torch.uint8, torch.bool) or tuple(m.shape) != tuple(t.shape[:2]):
            raise ValueError(f"{who}: a mask is uint8 or bool H x W of the picture's sides {tuple(t.shape[:2])}, got "
                             f"{getattr(m, 'dtype', type(m).__name__)} {tuple(getattr(m, 'shape', ()))}")
        m = (m != 0).to(torch.uint8)
    dev = _to_device(t, None)
    out, known = _mask_fill_device(dev, None if m is None else _to_device(m, dev.device), units, table, fill, hole, seed,
                                   sample_id, passes)
    if kind == "numpy":
        return out.cpu().numpy(), known.cpu().numpy()
    return (out.cpu(), known.cpu()) if kind == "cpu" else (out, known)


def _psnr_missing(est: torch.Tensor, ref: torch.Tensor, known: torch.Tensor) -> float:
    """10 log10(255^2 n / SSE) over the n bytes of the missing pixels of two uint8 H x W x C device pictures: the exact
    integer SSE (kernels.u8_sse) of the estimate with the known pixels put back, and n = C times the integer count of
    the zeros of ``known``; inf where nothing is missing."""
    missing = int((known == 0).sum().item())
    if missing == 0:
        return float("inf")
    merged = torch.where(known[:, :, None] != 0, ref, est).contiguous()
    return _psnr(kernels.u8_sse(merged, ref.contiguous()), missing * int(ref.shape[2]))


def psnr_missing_u8(est, ref, known) -> float:
    """PSNR of the uint8 H x W x C picture ``est`` against ``ref`` over the missing pixels alone -- those where the
    H x W plane ``known`` is zero: 10 log10(255^2 n / SSE) with the SSE and the n bytes of these pixels, exact integers
    both; inf where nothing is missing or the pixels agree."""
    who = "psnr_missing_u8"
    ta, tb = _u8_pair(who, est, ref)
    k = torch.from_numpy(np.ascontiguousarray(known)) if isinstance(known, np.ndarray) else known
    if ta.dim() != 3 or not isinstance(k, torch.Tensor) or tuple(k.shape) != tuple(ta.shape[:2]):
        raise ValueError(f"{who}: expected H x W x C pictures and an H x W plane of the known pixels, got "
                         f"{tuple(ta.shape)} and {tuple(getattr(k, 'shape', ()))}")
    return _psnr_missing(ta, tb, k.to(ta.device))


def _inpaint_table(who: str, fill_side, fill_sigma):
    try:
        return kernels.mask_weights(fill_side, fill_sigma)
    except ValueError as e:
        raise ValueError(f"{who}: {str(e).split(': ', 1)[1]}") from None


def evaluate_inpaint(model: Callable, images, keep, fill="conv", fill_side: int = 7, fill_sigma: Optional[float] = None,
                     hole: int = 128, seed: int = 2204, passes: int = 1, keep_known: bool = True, shave: int = 0,
                     factor: int = 16, ensemble=1, metrics=("psnr",), **tiling_args) -> dict:
    """Score ``model`` on inpainting (the "x % of the pixels missing" tables) over clean uint8 H x W x C pictures
    (numpy arrays or tensors, host or device).  Per picture i: a pixel is known with probability ``keep`` -- the mask
    is drawn on the device with sample id i under ``seed`` -- the missing ones are filled (kernels.u8_mask_fill:
    ``fill`` "zero" or "conv" under kernels.mask_weights(fill_side, fill_sigma), ``hole``, ``passes``), the filled
    picture is restored as ``restore_image`` does, with ``keep_known`` the known pixels are put back into the result,
    ``shave`` pixels are cut from each side, and the result is scored against the clean picture with the exact-integer
    kernels.  Metrics: those of the other protocols and "psnr_missing", the PSNR over the missing pixels alone (inf
    where none is missing).  Returns {metric: (mean, per-image values)} as evaluate_pairs does.  Nothing is drawn on
    the host: a picture's mask is a function of (seed, i).  tiling_args: tile, halo, micro_batch, device;
    ``ensemble`` as in restore_image.

    Everything is checked before any launch: the shared arguments, then keep, the fill, the table, the hole, the seed,
    passes, keep_known, the shave, uint8 pictures, a picture smaller than the shave leaves, and what the metrics need
    of the shaved picture."""
    who = "evaluate_inpaint"
    modes, metrics, device, tile, halo, micro_batch = _evaluate_args(who, model, ensemble, metrics, tiling_args,
                                                                     INPAINT_METRICS)
    try:
        units = kernels.keep_units(keep)
    except ValueError:
        raise ValueError(f"{who}: keep is the known share, a number of 0..1, got {keep!r}") from None
    fill_code = kernels._check_mask_fill(who, fill)
    table, fill_code, hole, seed, _, passes = _mask_fill_args(who, fill_code, _inpaint_table(who, fill_side, fill_sigma),
                                                              hole, seed, 0, passes)
    if not isinstance(keep_known, (bool, np.bool_)):
        raise ValueError(f"{who}: keep_known is True or False, got {keep_known!r}")
    shave = _check_shave(who, shave)
    if len(images) < 1:
        raise ValueError(f"{who}: no images")
    shared = tuple(m for m in metrics if m not in INPAINT_METRICS)
    cleans = []
    for i in range(len(images)):
        try:
            t, _ = _checked_image(images[i])
        except ValueError as e:
            raise ValueError(f"{who}: image {i}: {e}") from None
        if t.dtype != torch.uint8:
            raise ValueError(f"{who}: image {i} is {t.dtype}; the mask is defined on uint8 pictures")
        h, w = int(t.shape[0]), int(t.shape[1])
        if not kernels.mask_fill_ok(int(t.shape[2]), h, w):
            raise ValueError(f"{who}: image {i} is {tuple(t.shape)}; the fill takes pictures of 1..4 channels")
        if min(h, w) <= 2 * shave:
            raise ValueError(f"{who}: image {i} is {tuple(t.shape)}: nothing is left after a shave of {shave}")
        _check_metric_shape(who, f"image {i} after the shave", (h - 2 * shave, w - 2 * shave, t.shape[2]), shared)
        plan(h, w, factor, tile, halo)                          # raises what the restoration would
        cleans.append(t)
    if device is None:
        device = next((t.device for t in cleans if t.is_cuda), None)
    cut = (lambda a: a[shave:a.shape[0] - shave, shave:a.shape[1] - shave].contiguous()) if shave else (lambda a: a)
    values = {m: [] for m in metrics}
    for i, t in enumerate(cleans):
        clean = _to_device(t, device)
        filled, known = _mask_fill_device(clean, None, units, table, fill_code, hole, seed, i, passes)
        restored = _restore_device(model, filled, None, factor, tile, halo, micro_batch, True, modes)
        if restored.shape != clean.shape:
            raise ValueError(f"{who}: the model returns {restored.shape[2]} channel(s) for {clean.shape[2]}; no score")
        if keep_known:      # integer ATen ops: exact and order-free
            restored = torch.where(known[:, :, None] != 0, clean, restored)
        restored, clean, known = cut(restored.contiguous()), cut(clean), cut(known)
        for m in metrics:
            values[m].append(_psnr_missing(restored, clean, known) if m == "psnr_missing" else _SCORE[m](restored, clean))
    return _means(values, metrics)


def _blur_kernel(who: str, kernel):
    """The training.BlurKernel of a spec; its refusal under the caller's name."""
    from .training import parse_blur_spec
    try:
        return parse_blur_spec(kernel)
    except ValueError as e:
        raise ValueError(f"{who}: {e}") from None


def blur_u8(a, kernel, boundary="wrap"):
    """The uint8 picture ``a`` (H x W x C with C of 1..4, or H x W; a numpy array or a tensor, host or device)
    convolved with a blur kernel on the GPU, in exact integers (kernels.u8_blur; include/grr.h has the definition);
    the result is of the same kind.  ``kernel``: a spec as training.parse_blur_spec takes it ("gaussian:25:1.6",
    "motion:15:30", "box:5", "file:psf.npy", a 2-D array or a BlurKernel); ``boundary``: "wrap", "replicate" or
    "reflect" (or the code 0..2).  training.blur_degrade_u8 gives the same bytes on the CPU."""
    kernel = _blur_kernel("blur_u8", kernel)                               # before any transfer
    boundary = kernels._check_boundary("blur_u8", boundary)
    flat = isinstance(a, (np.ndarray, torch.Tensor)) and a.ndim == 2
    out = _resized_u8("blur_u8", a[:, :, None] if flat else a, lambda t: kernels.u8_blur(t, kernel, boundary))
    return out[:, :, 0] if flat else out


def _deblur_protocol(who: str, kernel, boundary, noise_sigma, seed, shave) -> _Protocol:
    """Deblurring: the whole picture blurred by ``kernel`` under ``boundary``, a shave of ``shave``.  With a positive
    ``noise_sigma`` the model's input is float32: the blurred picture / 255 plus N(0, noise_sigma / 255) noise drawn on
    the host from one RandomState(seed) stream in picture order, cast to float32 and not quantised."""
    kernel = _blur_kernel(who, kernel)
    boundary = kernels._check_boundary(who, boundary)
    if isinstance(noise_sigma, bool) or not isinstance(noise_sigma, (int, float, np.integer, np.floating)) \
            or not (np.isfinite(noise_sigma) and noise_sigma >= 0):
        raise ValueError(f"{who}: noise_sigma is a non-negative number, got {noise_sigma!r}")
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed < 2 ** 32:
        raise ValueError(f"{who}: seed is an integer of 0..2^32 - 1, got {seed!r}")
    shave = _check_shave(who, shave)
    noise_sigma = float(noise_sigma)
    rs = np.random.RandomState(seed=int(seed))

    def admit(i, t):
        if not kernels.blur_ok(t.shape[2], t.shape[0], t.shape[1]):
            raise ValueError(f"{who}: image {i} is {tuple(t.shape)}; the blur takes 1..4 channels")

    def degrade(clean):
        blurred = kernels.u8_blur(clean, kernel, boundary)
        if noise_sigma == 0:
            return blurred
        x = blurred.cpu().numpy().astype(np.float32) / np.float32(255.0)
        x += rs.normal(0, noise_sigma / 255.0, x.shape).astype(np.float32)
        return torch.from_numpy(x).to(clean.device)

    label = f"blur {kernel.spec} {kernels.BLUR_BOUNDARIES[boundary]}" + \
        (f" noise {noise_sigma:g}" if noise_sigma else "") + f" shave {shave}"
    return _Protocol(who, label=label, defined_on="the blur is defined on", admit=admit, crop=lambda h, w: (h, w),
                     shave=shave, left_after=f"after a shave of {shave}", scored="image {i} after the shave",
                     degrade=degrade)


def evaluate_deblur(model: Callable, images, kernel, boundary="wrap", noise_sigma: float = 0.0, seed: int = 2204,
                    shave: int = 0, factor: int = 16, ensemble=1, metrics=("psnr", "ssim"), **tiling_args) -> dict:
    """Score ``model`` on deblurring (the protocol of the Levin / IRCNN / DPIR tables) over clean uint8 H x W x C
    pictures (numpy arrays or tensors, host or device).  Per picture: the blur by ``kernel`` (a spec as
    training.parse_blur_spec takes it) under ``boundary`` on the device (kernels.u8_blur), the blurred picture restored
    as ``restore_image(..., quantise=True)`` does, ``shave`` pixels cut from each side of the restored and the clean
    picture, and the two scored with the exact-integer kernels.  Returns {metric: (mean, per-image values)} as
    evaluate_pairs does.  tiling_args: tile, halo, micro_batch, device; ``ensemble`` as in restore_image.

    With ``noise_sigma == 0`` the model's input is the blurred uint8 picture, and with ``shave=0`` the result is
    evaluate_pairs(model, blurred, clean) bit for bit.  With ``noise_sigma > 0`` the input is float32: blurred / 255
    plus RandomState(seed).normal(0, noise_sigma / 255, shape), drawn on the host in picture order, cast to float32
    and not quantised -- the tables' protocol.

    Everything is checked before any launch: the kernel spec first, then the boundary, the noise, the seed, the
    shave, uint8 pictures of 1..4 channels, a picture smaller than the shave leaves, and what the metrics need of the
    shaved picture (SSIM: both sides at least 11; PSNR-B: at least 16; the Y-channel metrics: 3 channels)."""
    modes, metrics, device, tile, halo, micro_batch = _evaluate_args("evaluate_deblur", model, ensemble, metrics,
                                                                     tiling_args)
    return _evaluate_degraded(_deblur_protocol("evaluate_deblur", kernel, boundary, noise_sigma, seed, shave), model,
                              images, factor, modes, metrics, device, tile, halo, micro_batch)


def evaluate_pairs(model: Callable, inputs, targets, factor: int = 16, across_images: bool = False, ensemble=1,
                   metrics=("psnr",), **tiling_args) -> dict:
    """Score ``model`` on degraded / clean picture pairs: inputs[i] and targets[i] are uint8 H x W x C images of
    one shape (numpy arrays or tensors, host or device).  Nothing is synthesised: each input goes to the device as
    uint8, is restored as ``restore_image(..., quantise=True)`` restores it, and the uint8 result is scored against
    the target with the exact-integer kernels (psnr_u8, ssim_u8, psnr_y_u8, ssim_y_u8).  Returns {metric: (mean,
    per-image values)} for the names in ``metrics``, as evaluate_metrics does.  tiling_args: tile, halo, micro_batch,
    device.

    ``across_images``: the inputs are restored by restore_images' path in shared window batches and every metric of
    all images is one launch on the restored and the target arena; the same floats for a batch-independent model.
    ``ensemble`` as in restore_image, on either branch.  A length or shape mismatch, an image that is not uint8,
    an unknown metric, with "ssim" or "ssim_y" a side below 11 and with "psnr_y" or "ssim_y" a pair that is not
    3-channel are ValueErrors before any launch."""
    who = "evaluate_pairs"
    modes, metrics, device, tile, halo, micro_batch = _evaluate_args(who, model, ensemble, metrics, tiling_args)
    if len(inputs) != len(targets) or len(inputs) < 1:
        raise ValueError(f"{who}: {len(inputs)} input(s) for {len(targets)} target(s); one target per input, at least one")
    pairs = []
    for i in range(len(inputs)):
        pair = []
        for what, image in (("input", inputs[i]), ("target", targets[i])):
            try:
                t, _ = _checked_image(image)
            except ValueError as e:
                raise ValueError(f"{who}: {what} {i}: {e}") from None
            if t.dtype != torch.uint8:
                raise ValueError(f"{who}: {what} {i} is {t.dtype}; pairs are uint8 pictures")
            pair.append(t)
        if pair[0].shape != pair[1].shape:
            raise ValueError(f"{who}: input {i} is {tuple(pair[0].shape)} and its target {tuple(pair[1].shape)}: a "
                             "pair has one shape")
        _check_metric_shape(who, f"pair {i}", pair[0].shape, metrics)
        plan(pair[0].shape[0], pair[0].shape[1], factor, tile, halo)        # raises what the restoration would
        pairs.append(pair)
    if device is None:
        device = next((t.device for pair in pairs for t in pair if t.is_cuda), None)
    if across_images:
        pack = pack_images([p[0] for p in pairs], device)
        restored = _restore_pack(model, pack, plan_images(pack.shapes(), factor, tile, halo, micro_batch, modes), True,
                                 modes)
        values = _score_packs(who, restored, pack_images([p[1] for p in pairs], restored.arena.device), metrics)
    else:
        values = {m: [] for m in metrics}
        for img, target in pairs:
            restored = _restore_device(model, img, device, factor, tile, halo, micro_batch, True, modes)
            target = target.to(restored.device)
            for m in metrics:
                values[m].append(_SCORE[m](restored, target))
    return _means(values, metrics)
