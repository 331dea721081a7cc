"""The order in which restore.evaluate_sr, evaluate_car and evaluate_demosaic refuse a call, without a GPU: the
arguments all evaluators share (ensemble, metrics, unexpected names), the protocol's own parameters in their order, the
shave, "no images", then per image in index order: not an image, not uint8, not admissible, nothing left, the
metrics' needs, ``plan``.  Each case is wrong in two adjacent ways and must raise the earlier refusal; the same call
with the earlier fault mended raises the later one.  Nothing is launched."""
import numpy as np
import pytest

from irdu_amd import kernels as K
from irdu_amd import restore


def model(x):
    return x


def zeros(h, w, c=3, dtype=np.uint8):
    return np.zeros((h, w, c), dtype)


BIG, SMALL = zeros(40, 56), zeros(12, 12)       # SSIM needs sides of 11, PSNR-B of 16


def sr(images, scale=2, **kw):
    return restore.evaluate_sr(model, images, scale, **kw)


def car(images, quality=10, subsampling=0, **kw):
    return restore.evaluate_car(model, images, quality, subsampling, **kw)


def dem(images, pattern="rggb", fill="malvar", **kw):
    return restore.evaluate_demosaic(model, images, pattern, fill, **kw)


# (id, call wrong in both ways, the earlier refusal, the call wrong in the later way only, the later refusal)
CASES = [
    # 1. the shared arguments, in _evaluate_args' order, before the protocol's parameters
    ("sr-ensemble-metrics", lambda: sr([BIG], ensemble=3, metrics=("mse",)), "evaluate_sr: ensemble",
     lambda: sr([BIG], metrics=("mse",)), "evaluate_sr: metrics"),
    ("sr-metrics-unexpected", lambda: sr([BIG], metrics=("mse",), crop=1), "evaluate_sr: metrics",
     lambda: sr([BIG], crop=1), "evaluate_sr: unexpected arguments"),
    ("sr-unexpected-scale", lambda: sr([BIG], 9, crop=1), "evaluate_sr: unexpected arguments",
     lambda: sr([BIG], 9), "evaluate_sr: the scale"),
    ("sr-metrics-scale", lambda: sr([BIG], 9, metrics=("mse",)), "evaluate_sr: metrics",
     lambda: sr([BIG], 9), "evaluate_sr: the scale"),
    ("car-metrics-quality", lambda: car([BIG], 0, metrics=()), "evaluate_car: metrics",
     lambda: car([BIG], 0), "evaluate_car: the quality"),
    ("car-unexpected-quality", lambda: car([BIG], 0, shave=2), "evaluate_car: unexpected arguments",
     lambda: car([BIG], 0), "evaluate_car: the quality"),
    ("demosaic-metrics-pattern", lambda: dem([BIG], "rgbg", metrics=("psnr", "psnr")), "evaluate_demosaic: metrics",
     lambda: dem([BIG], "rgbg"), "evaluate_demosaic: the pattern"),
    # 2. the protocol's parameters in their order, 3. then the shave
    ("car-quality-subsampling", lambda: car([BIG], 101, 1), "evaluate_car: the quality",
     lambda: car([BIG], 10, 1), "evaluate_car: the subsampling"),
    ("demosaic-pattern-fill", lambda: dem([BIG], 4, "linear"), "evaluate_demosaic: the pattern",
     lambda: dem([BIG], 3, "linear"), "evaluate_demosaic: the fill"),
    ("sr-scale-shave", lambda: sr([BIG], 1, shave=-1), "evaluate_sr: the scale",
     lambda: sr([BIG], 2, shave=-1), "evaluate_sr: shave is a non-negative integer"),
    ("demosaic-fill-shave", lambda: dem([BIG], "rggb", "linear", shave=True), "evaluate_demosaic: the fill",
     lambda: dem([BIG], "rggb", "zero", shave=True), "evaluate_demosaic: shave is a non-negative integer"),
    # 4. "no images" after them
    ("sr-shave-empty", lambda: sr([], shave=2.0), "evaluate_sr: shave", lambda: sr([]), "evaluate_sr: no images"),
    ("demosaic-shave-empty", lambda: dem([], shave=-3), "evaluate_demosaic: shave",
     lambda: dem([]), "evaluate_demosaic: no images"),
    ("car-quality-empty", lambda: car([], 0), "evaluate_car: the quality", lambda: car([]), "evaluate_car: no images"),
    ("car-subsampling-empty", lambda: car([], 10, 3), "evaluate_car: the subsampling",
     lambda: car([]), "evaluate_car: no images"),
    # 5. per image, in index order
    ("sr-image0-float-image1-small", lambda: sr([BIG.astype(np.float32), SMALL], shave=6),
     "evaluate_sr: image 0 is torch.float32; the protocol is defined on uint8 pictures",
     lambda: sr([BIG, SMALL], shave=6), "evaluate_sr: image 1 is .*nothing is left after the crop to multiples of 2 "
                                        "and a shave of 6"),
    ("car-image0-small-image1-float", lambda: car([SMALL, BIG.astype(np.float32)]),
     r"evaluate_car: image 0 is \(12, 12, 3\); PSNR-B",
     lambda: car([BIG, BIG.astype(np.float32)]), "evaluate_car: image 1 is torch.float32; JPEG is defined on uint8"),
    ("demosaic-image0-gray-image1-not-an-image", lambda: dem([zeros(40, 56, 1), BIG[0]]),
     "evaluate_demosaic: image 0 is .*clean R, G, B",
     lambda: dem([BIG, BIG[0]]), "evaluate_demosaic: image 1: restore_image: expected an H x W x C image"),
    # ... and within an image: not an image, not uint8, not admissible, nothing left, the metrics, plan
    ("sr-not-an-image-float", lambda: sr([BIG[0].astype(np.float32)]), "evaluate_sr: image 0: restore_image: expected",
     lambda: sr([BIG.astype(np.float32)]), "evaluate_sr: image 0 is torch.float32"),
    ("car-not-an-image-float", lambda: car([BIG.astype(np.float64)]), "evaluate_car: image 0: restore_image: image dtype",
     lambda: car([BIG.astype(np.float32)]), "evaluate_car: image 0 is torch.float32"),
    ("car-float-channels", lambda: car([zeros(40, 56, 2, np.float32)]), "evaluate_car: image 0 is torch.float32",
     lambda: car([zeros(40, 56, 2)]), "evaluate_car: image 0 is .*JPEG takes 1 or 3 channels"),
    ("demosaic-float-channels", lambda: dem([zeros(40, 56, 1, np.float32)]),
     "evaluate_demosaic: image 0 is torch.float32; the mosaic is defined on uint8",
     lambda: dem([zeros(40, 56, 1)]), "evaluate_demosaic: image 0 is .*the protocol takes clean R, G, B pictures"),
    ("demosaic-channels-nothing-left", lambda: dem([zeros(12, 12, 1)], shave=6), "evaluate_demosaic: image 0 is .*clean R, G, B",
     lambda: dem([SMALL], shave=6), r"evaluate_demosaic: image 0 is \(12, 12, 3\): nothing is left after a shave of 6"),
    ("car-channels-metrics", lambda: car([zeros(12, 12, 2)]), "evaluate_car: image 0 is .*1 or 3 channels",
     lambda: car([SMALL]), r"evaluate_car: image 0 is \(12, 12, 3\); PSNR-B needs"),
    ("sr-nothing-left-metrics", lambda: sr([SMALL], shave=6, metrics=("ssim",)), "evaluate_sr: image 0 is .*nothing is left",
     lambda: sr([SMALL], shave=1, metrics=("ssim",)), r"evaluate_sr: image 0 after the shave is \(10, 10, 3\); SSIM needs"),
    ("demosaic-nothing-left-metrics", lambda: dem([SMALL], shave=6, metrics=("ssim",)),
     "evaluate_demosaic: image 0 is .*nothing is left",
     lambda: dem([SMALL], shave=1, metrics=("ssim",)), r"evaluate_demosaic: image 0 after the shave is \(10, 10, 3\); SSIM"),
    ("sr-metrics-plan", lambda: sr([SMALL], shave=1, metrics=("ssim",), factor=32), "evaluate_sr: image 0 after the shave .*SSIM",
     lambda: sr([SMALL], shave=0, metrics=("ssim",), factor=32), "plan: reflect padding 20 must be smaller"),
    ("car-metrics-plan", lambda: car([SMALL], factor=32), "evaluate_car: image 0 is .*PSNR-B",
     lambda: car([SMALL], factor=32, metrics=("psnr", "ssim")), "plan: reflect padding 20 must be smaller"),
    ("demosaic-metrics-plan", lambda: dem([SMALL], metrics=("psnrb",), factor=32), "evaluate_demosaic: image 0 after the shave .*PSNR-B",
     lambda: dem([SMALL], factor=32), "plan: reflect padding 20 must be smaller"),
    # the Y-channel metrics are part of "the metrics": a gray picture passes JPEG's admission and fails there
    ("car-metrics-gray", lambda: car([zeros(40, 56, 1), SMALL], metrics=("psnr_y",)), "evaluate_car: image 0 is .*Y-channel",
     lambda: car([BIG, SMALL], metrics=("psnr_y", "psnrb")), "evaluate_car: image 1 is .*PSNR-B"),
]


def no_launch(*a, **k):
    raise AssertionError("a kernel was launched")


@pytest.mark.parametrize("both,earlier,later_only,later", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_the_earlier_refusal_wins(monkeypatch, both, earlier, later_only, later):
    monkeypatch.setattr(K, "_launch", no_launch)
    with pytest.raises((ValueError, TypeError), match=earlier):
        both()
    with pytest.raises((ValueError, TypeError), match=later):
        later_only()
