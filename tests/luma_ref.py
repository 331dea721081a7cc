"""PSNR and SSIM on the Y channel of two uint8 H x W x 3 RGB images in plain numpy, written from the definition alone.

  luma    ITU-R BT.601 "studio range", the Y of MATLAB's rgb2ycbcr, skimage.color.rgb2ycbcr and BasicSR's
          to_y_channel, not rounded to uint8: Y = 16 + (65.481 R + 128.553 G + 24.966 B) / 255 = Ny / 255000 with the
          integer Ny = 4080000 + 65481 R + 128553 G + 24966 B; each Y is the float64 double(Ny) / 255000.0, one rounding
  PSNR-Y  D = Ny(a) - Ny(b) per pixel, S = sum D^2 as a Python int (it can exceed 64 bits),
          10 log10(255^2 255000^2 N / S) with one true division of ints; inf for S == 0
  SSIM-Y  tests/ssim_ref.py's Gaussian-window SSIM (taps, C1, C2, valid positions) of the single plane Y

No torch, no scipy: the GPU tests import only this, ssim_ref and numpy.
"""
import numpy as np

from tests.ssim_ref import C1, C2, WINDOW, _filter_valid, taps

SCALE = 255000
BASE = 4080000
WEIGHTS = (65481, 128553, 24966)      # of R, G, B


def _checked(a: np.ndarray) -> np.ndarray:
    a = np.asarray(a)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"luma: expected a uint8 H x W x 3 image, got {a.shape} {a.dtype}")
    return a


def luma_int(a: np.ndarray) -> np.ndarray:
    """Ny, int64 [H, W]."""
    a = _checked(a).astype(np.int64)
    return BASE + WEIGHTS[0] * a[:, :, 0] + WEIGHTS[1] * a[:, :, 1] + WEIGHTS[2] * a[:, :, 2]


def luma(a: np.ndarray) -> np.ndarray:
    """Y, float64 [H, W]: the exact integer Ny divided once by 255000."""
    return luma_int(a).astype(np.float64) / float(SCALE)


def luma_sse(a: np.ndarray, b: np.ndarray) -> int:
    """S = sum (Ny(a) - Ny(b))^2, exact.  D^2 < 2^52 fits int64; the sum over up to 2^30 pixels does not, so the
    low 32 bits and the rest are summed apart (below 2^62 and 2^50) and joined as Python ints."""
    if np.shape(a) != np.shape(b):
        raise ValueError(f"luma_sse: shapes differ ({np.shape(a)} vs {np.shape(b)})")
    d = luma_int(a) - luma_int(b)
    d2 = d * d
    return int((d2 & 0xFFFFFFFF).sum(dtype=np.int64)) + (int((d2 >> 32).sum(dtype=np.int64)) << 32)


def psnr_y(a: np.ndarray, b: np.ndarray) -> float:
    s = luma_sse(a, b)
    n = np.shape(a)[0] * np.shape(a)[1]
    return float("inf") if s == 0 else float(10.0 * np.log10((255 ** 2 * SCALE ** 2 * n) / s))


def _filter_valid_vh(x: np.ndarray) -> np.ndarray:
    """_filter_valid in the other order: the vertical taps ascending, then the horizontal ones."""
    g = taps()
    h, w = x.shape[0], x.shape[1]
    cols = np.zeros((h - WINDOW + 1, w), dtype=np.float64)
    for k in range(WINDOW):
        cols += g[k] * x[k:k + h - WINDOW + 1]
    out = np.zeros((h - WINDOW + 1, w - WINDOW + 1), dtype=np.float64)
    for k in range(WINDOW):
        out += g[k] * cols[:, k:k + w - WINDOW + 1]
    return out


def ssim_y_map(a: np.ndarray, b: np.ndarray, vertical_first: bool = False) -> np.ndarray:
    """The per-pixel values s, [H - 10, W - 10] float64, of the luma planes of two uint8 H x W x 3 images.
    ``vertical_first`` filters in the other order (the same values up to float64 rounding)."""
    if np.shape(a) != np.shape(b):
        raise ValueError(f"ssim_y_map: shapes differ ({np.shape(a)} vs {np.shape(b)})")
    x, y = luma(a), luma(b)
    if min(x.shape) < WINDOW:
        raise ValueError(f"ssim_y_map: both sides must be at least {WINDOW} (got {x.shape})")
    f = _filter_valid_vh if vertical_first else _filter_valid
    mx, my = f(x), f(y)
    exx, eyy, exy = f(x * x), f(y * y), f(x * y)
    mxx, myy, mxy = mx * mx, my * my, mx * my
    vx, vy, vxy = exx - mxx, eyy - myy, exy - mxy
    return ((2.0 * mxy + C1) * (2.0 * vxy + C2)) / ((mxx + myy + C1) * (vx + vy + C2))


def ssim_y(a: np.ndarray, b: np.ndarray) -> float:
    """The mean of ssim_y_map."""
    return float(np.mean(ssim_y_map(a, b)))


def quantised_sum_y(a: np.ndarray, b: np.ndarray) -> int:
    """sum rint(2^32 s) as a Python int: what the device sum is, up to the few values whose float64 rounding
    differs across the quantisation step."""
    q = np.rint(ssim_y_map(a, b) * 4294967296.0).astype(np.int64)
    return int(q.sum(dtype=np.int64))
