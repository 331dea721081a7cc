"""The SSIM training loss and its gradient in plain numpy float64, written from the definition alone:

  x, y     prediction and target, [B, C, H, W], data range 1, not clamped
  window   tests/ssim_ref.py's: 11 separable Gaussian taps, sigma 1.5, valid positions only
  moments  mx, my, E[x^2], E[y^2], E[xy] per plane at the (H - 10) x (W - 10) valid positions
  terms    vx = E[x^2] - mx^2, vy = E[y^2] - my^2, vxy = E[xy] - mx my, C1 = 0.01^2, C2 = 0.03^2
           A1 = 2 mx my + C1, A2 = 2 vxy + C2, B1 = mx^2 + my^2 + C1, B2 = vx + vy + C2, s = A1 A2 / (B1 B2)
  loss     1 - (sum s) / N, N = B C (H - 10)(W - 10)
  gradient ds/dE[x^2] = -s / B2, ds/dE[xy] = 2 A1 / (B1 B2),
           ds/dmx = 2 my (A2 - A1) / (B1 B2) - 2 mx s / B1 + 2 mx s / B2,
           dloss/dx = -(1 / N) (F*(ds/dmx) + 2 x F*(ds/dE[x^2]) + y F*(ds/dE[xy])),
           F* the window's adjoint: the full correlation of a valid-size plane back to H x W, zero outside

No torch: the GPU tests import only this, tests/ssim_ref.py and numpy.
"""
import numpy as np

from tests.ssim_ref import WINDOW, taps

C1 = 0.01 ** 2
C2 = 0.03 ** 2


def _filter_valid(x: np.ndarray) -> np.ndarray:
    """The separable window over the two trailing axes of x [..., H, W] at the valid positions."""
    g = taps()
    h, w = x.shape[-2:]
    rows = np.zeros(x.shape[:-1] + (w - WINDOW + 1,), dtype=np.float64)
    for k in range(WINDOW):
        rows += g[k] * x[..., :, k:k + w - WINDOW + 1]
    out = np.zeros(x.shape[:-2] + (h - WINDOW + 1, w - WINDOW + 1), dtype=np.float64)
    for k in range(WINDOW):
        out += g[k] * rows[..., k:k + h - WINDOW + 1, :]
    return out


def _adjoint(c: np.ndarray) -> np.ndarray:
    """F*: c [..., H - 10, W - 10] back to [..., H, W]; out[i, j] = sum over k, l of g[k] g[l] c[i - k, j - l]."""
    g = taps()
    vh, vw = c.shape[-2:]
    cols = np.zeros(c.shape[:-1] + (vw + WINDOW - 1,), dtype=np.float64)
    for k in range(WINDOW):
        cols[..., :, k:k + vw] += g[k] * c
    out = np.zeros(c.shape[:-2] + (vh + WINDOW - 1, vw + WINDOW - 1), dtype=np.float64)
    for k in range(WINDOW):
        out[..., k:k + vh, :] += g[k] * cols
    return out


def _check(x, y):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if x.ndim != 4 or x.shape != y.shape or min(x.shape[-2:]) < WINDOW:
        raise ValueError(f"ssim_loss_ref: expected two [B, C, H, W] arrays of one shape with H, W >= {WINDOW}, got "
                         f"{x.shape} and {y.shape}")
    return x, y


def terms(x, y, c1: float = C1, c2: float = C2):
    """(s, A1, A2, B1, B2, mx, my), each [B, C, H - 10, W - 10] float64."""
    x, y = _check(x, y)
    mx, my = _filter_valid(x), _filter_valid(y)
    exx, eyy, exy = _filter_valid(x * x), _filter_valid(y * y), _filter_valid(x * y)
    vx, vy, vxy = exx - mx * mx, eyy - my * my, exy - mx * my
    a1, a2 = 2.0 * mx * my + c1, 2.0 * vxy + c2
    b1, b2 = mx * mx + my * my + c1, vx + vy + c2
    return (a1 * a2) / (b1 * b2), a1, a2, b1, b2, mx, my


def ssim_map(x, y, c1: float = C1, c2: float = C2) -> np.ndarray:
    return terms(x, y, c1, c2)[0]


def item_means(x, y) -> np.ndarray:
    """The mean of s over each batch item's C (H - 10)(W - 10) positions, [B]."""
    return ssim_map(x, y).mean(axis=(1, 2, 3))


def loss(x, y) -> float:
    return float(1.0 - np.mean(ssim_map(x, y)))


def loss_and_grad(x, y, gout: float = 1.0):
    """(loss, gout dloss/dx): a float and a float64 [B, C, H, W] array."""
    x, y = _check(x, y)
    s, a1, a2, b1, b2, mx, my = terms(x, y)
    n = s.size
    d_mx = 2.0 * my * (a2 - a1) / (b1 * b2) - 2.0 * mx * s / b1 + 2.0 * mx * s / b2
    d_exx = -s / b2
    d_exy = 2.0 * a1 / (b1 * b2)
    g = -(_adjoint(d_mx) + 2.0 * x * _adjoint(d_exx) + y * _adjoint(d_exy)) / n
    return float(1.0 - np.mean(s)), float(gout) * g


# ---- the inputs of the tests (tests/test_ssim_loss_ref.py on the CPU, tests/test_gpu_ssim_loss.py on the GPU)
KINDS = {"noisy": [(2, 3, 11, 11), (1, 1, 12, 43), (2, 3, 43, 75)], "flat": [(1, 3, 24, 24)], "out": [(1, 3, 24, 24)],
         "equal": [(1, 2, 21, 32)]}


def pair(kind: str, shape, seed: int = 7):
    """(x, y) float32 [B, C, H, W]: noisy -- a smooth sine pattern in [0.15, 0.85] plus N(0, 25 / 255); flat --
    y = 0.5, x = y + N(0, 1e-3): heavy cancellation; out -- x = 3 y - 1 + N(0, 0.2): values outside [0, 1], negative
    s present; equal -- x = y."""
    b, c, h, w = shape
    rs = np.random.RandomState(seed + 1000 * b + 100 * c + 13 * h + w)
    ii, jj = np.mgrid[0:h, 0:w]
    base = 0.5 + 0.35 * np.sin(jj / 7.0 + 0.3 * np.arange(c)[:, None, None]) * np.cos(ii / 5.0)
    y = np.broadcast_to(base, (b, c, h, w)) * (1.0 - 0.05 * np.arange(b)[:, None, None, None])
    y = np.ascontiguousarray(y + 0.5 * 0.05 * np.arange(b)[:, None, None, None])      # still within [0.15, 0.85]
    if kind == "noisy":
        x = y + rs.normal(0.0, 25.0 / 255.0, shape)
    elif kind == "flat":
        y = np.full(shape, 0.5)
        x = y + rs.normal(0.0, 1e-3, shape)
    elif kind == "out":
        x = 3.0 * y - 1.0 + rs.normal(0.0, 0.2, shape)
    else:
        assert kind == "equal"
        x = y
    x32, y32 = x.astype(np.float32), y.astype(np.float32)
    return (y32.copy(), y32) if kind == "equal" else (x32, y32)
