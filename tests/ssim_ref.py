"""Gaussian-window SSIM of two uint8 H x W x C images in plain numpy float64, written from the definition alone
(Wang et al. 2004, as skimage.metrics.structural_similarity(a, b, gaussian_weights=True, sigma=1.5,
use_sample_covariance=False, data_range=255, channel_axis=2) computes it):

  window   11 x 11 separable Gaussian, taps g[k] = exp(-(k - 5)^2 / (2 x 1.5^2)) / sum, k = 0..10
  moments  per channel mx, my, E[x^2], E[y^2], E[xy], filtered with that window at the (H - 10) x (W - 10) pixels
           whose window lies inside the image (skimage filters with a reflect border and crops 5 pixels, which
           removes every pixel the border touched)
  terms    vx = E[x^2] - mx^2, vy = E[y^2] - my^2, vxy = E[xy] - mx my, C1 = (0.01 x 255)^2, C2 = (0.03 x 255)^2
  value    s = (2 mx my + C1)(2 vxy + C2) / ((mx^2 + my^2 + C1)(vx + vy + C2))
  result   the mean of s over all (H - 10)(W - 10) C values

No torch, no scipy: the GPU tests import only this and numpy.
"""
import numpy as np

WINDOW = 11
SIGMA = 1.5
C1 = (0.01 * 255.0) ** 2
C2 = (0.03 * 255.0) ** 2


def taps() -> np.ndarray:
    k = np.arange(WINDOW, dtype=np.float64)
    g = np.exp(-((k - (WINDOW - 1) // 2) ** 2) / (2.0 * SIGMA ** 2))
    return g / g.sum()


def _filter_valid(x: np.ndarray) -> np.ndarray:
    """The separable window over the two leading axes of x [H, W, C] at the valid positions: the horizontal taps
    in ascending order, then the vertical ones."""
    g = taps()
    h, w = x.shape[0], x.shape[1]
    rows = np.zeros((h, w - WINDOW + 1) + x.shape[2:], dtype=np.float64)
    for k in range(WINDOW):
        rows += g[k] * x[:, k:k + w - WINDOW + 1]
    out = np.zeros((h - WINDOW + 1,) + rows.shape[1:], dtype=np.float64)
    for k in range(WINDOW):
        out += g[k] * rows[k:k + h - WINDOW + 1]
    return out


def ssim_map(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """The per-pixel, per-channel values s, [H - 10, W - 10, C] float64, of two uint8 H x W x C images."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != np.uint8 or b.dtype != np.uint8 or a.ndim != 3 or a.shape != b.shape:
        raise ValueError(f"ssim_map: expected two uint8 H x W x C images of one shape, got {a.shape} {a.dtype} and "
                         f"{b.shape} {b.dtype}")
    if min(a.shape[:2]) < WINDOW:
        raise ValueError(f"ssim_map: both sides must be at least {WINDOW} (got {a.shape})")
    x, y = a.astype(np.float64), b.astype(np.float64)
    mx, my = _filter_valid(x), _filter_valid(y)
    exx, eyy, exy = _filter_valid(x * x), _filter_valid(y * y), _filter_valid(x * y)
    mxx, myy, mxy = mx * mx, my * my, mx * my
    vx, vy, vxy = exx - mxx, eyy - myy, exy - mxy
    return ((2.0 * mxy + C1) * (2.0 * vxy + C2)) / ((mxx + myy + C1) * (vx + vy + C2))


def ssim(a: np.ndarray, b: np.ndarray) -> float:
    """The mean of ssim_map."""
    return float(np.mean(ssim_map(a, b)))


def ssim_with_map(a: np.ndarray, b: np.ndarray):
    """(mean, map)."""
    m = ssim_map(a, b)
    return float(np.mean(m)), m


def quantised_sum(a: np.ndarray, b: np.ndarray) -> int:
    """sum rint(2^32 s) as a Python int: what the device sum is, up to the few values whose float64 rounding
    differs across the quantisation step."""
    q = np.rint(ssim_map(a, b) * 4294967296.0).astype(np.int64)
    return int(q.sum(dtype=np.int64))
