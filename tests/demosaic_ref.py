"""An independent oracle of the Bayer mosaic and its initial fill (include/grr.h has the definition).  It imports
nothing of the package.  Two forms of everything: ``*_loops`` walks the pixels in Python integers, straight from
the definition; the plain names correlate the mosaic plane with 5 x 5 integer kernels through
scipy.ndimage.correlate(mode="mirror"), whose border rule is the definition's reflection, for the larger shapes.
tests/test_demosaic_ref.py holds the two to each other byte for byte."""
import numpy as np

PATTERNS = ("rggb", "grbg", "gbrg", "bggr")
FILLS = ("zero", "bilinear", "malvar")
R_SITE = {"rggb": (0, 0), "grbg": (0, 1), "gbrg": (1, 0), "bggr": (1, 1)}       # (row parity, column parity)


def site(pattern: str, y: int, x: int) -> int:
    """The channel (R 0, G 1, B 2) measured at (y, x)."""
    ry, rx = R_SITE[pattern]
    if (y % 2, x % 2) == (ry, rx):
        return 0
    if (y % 2, x % 2) == (1 - ry, 1 - rx):
        return 2
    return 1


def reflect(i: int, n: int) -> int:
    if n == 1:
        return 0
    t = i % (2 * (n - 1))
    return t if t < n else 2 * (n - 1) - t


def _checked(a):
    a = np.asarray(a)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or 0 in a.shape:
        raise ValueError(f"expected a uint8 H x W x 3 picture, got {a.dtype} {a.shape}")
    return a


# ---- the per-pixel form
def mosaic_loops(a, pattern: str) -> np.ndarray:
    a = _checked(a)
    h, w = a.shape[:2]
    return np.array([[a[y, x, site(pattern, y, x)] for x in range(w)] for y in range(h)], np.uint8).reshape(h, w)


# coefficient sets in sixteenths, as {(dy, dx): weight}
def _ring(ctr=0, cross=0, far=0, diag=0, h1=0, h2=0, v1=0, v2=0) -> dict:
    k = {(0, 0): ctr}
    for d in (-1, 1):
        k[(0, d)] = cross + h1
        k[(d, 0)] = cross + v1
        k[(0, 2 * d)] = far + h2
        k[(2 * d, 0)] = far + v2
        for e in (-1, 1):
            k[(d, e)] = diag
    return k


COEFFS = {
    "zero": dict(green=_ring(), other=_ring(), inrow=_ring(), incol=_ring()),
    "bilinear": dict(green=_ring(cross=4), other=_ring(diag=4), inrow=_ring(h1=8), incol=_ring(v1=8)),
    "malvar": dict(green=_ring(ctr=8, cross=4, far=-2), other=_ring(ctr=12, diag=4, far=-3),
                   inrow=_ring(ctr=10, h1=8, diag=-2, h2=-2, v2=1), incol=_ring(ctr=10, v1=8, diag=-2, v2=-2, h2=1)),
}


def _which(pattern: str, y: int, x: int, ch: int):
    """The coefficient set that gives channel ``ch`` at (y, x), or None where it is measured."""
    here = site(pattern, y, x)
    if ch == here:
        return None
    if ch == 1:
        return "green"
    if here != 1:
        return "other"
    # a G site: the colour lies in this row if the horizontal neighbour measures it
    return "inrow" if site(pattern, y, x + 1) == ch else "incol"


def fill_loops(m, pattern: str, fill: str) -> np.ndarray:
    m = np.asarray(m)
    h, w = m.shape
    out = np.zeros((h, w, 3), np.uint8)
    for y in range(h):
        for x in range(w):
            for ch in range(3):
                which = _which(pattern, y, x, ch)
                if which is None:
                    s = 16 * int(m[y, x])
                else:
                    s = sum(wt * int(m[reflect(y + dy, h), reflect(x + dx, w)])
                            for (dy, dx), wt in COEFFS[fill][which].items())
                out[y, x, ch] = min(max((s + 8) >> 4, 0), 255)
    return out


def degrade_loops(a, pattern: str, fill: str = "malvar") -> np.ndarray:
    return fill_loops(mosaic_loops(a, pattern), pattern, fill)


# ---- the correlation form
def _kernel(coeffs: dict) -> np.ndarray:
    k = np.zeros((5, 5), np.int64)
    for (dy, dx), wt in coeffs.items():
        k[2 + dy, 2 + dx] = wt
    return k


def _masks(pattern: str, h: int, w: int):
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    ry, rx = R_SITE[pattern]
    red = (y % 2 == ry) & (x % 2 == rx)
    blue = (y % 2 != ry) & (x % 2 != rx)
    g_red_row = (y % 2 == ry) & (x % 2 != rx)
    g_blue_row = (y % 2 != ry) & (x % 2 == rx)
    return red, blue, g_red_row, g_blue_row


def mosaic(a, pattern: str) -> np.ndarray:
    a = _checked(a)
    red, blue, _, _ = _masks(pattern, *a.shape[:2])
    return np.where(red, a[:, :, 0], np.where(blue, a[:, :, 2], a[:, :, 1]))


def fill(m, pattern: str, fill_name: str) -> np.ndarray:
    from scipy.ndimage import correlate
    m = np.asarray(m).astype(np.int64)
    h, w = m.shape
    red, blue, g_red_row, g_blue_row = _masks(pattern, h, w)
    c = {name: correlate(m, _kernel(k), mode="mirror") for name, k in COEFFS[fill_name].items()}
    s = np.zeros((h, w, 3), np.int64)
    s[:, :, 1] = np.where(red | blue, c["green"], 16 * m)
    s[:, :, 0] = np.where(red, 16 * m, np.where(blue, c["other"], np.where(g_red_row, c["inrow"], c["incol"])))
    s[:, :, 2] = np.where(blue, 16 * m, np.where(red, c["other"], np.where(g_blue_row, c["inrow"], c["incol"])))
    return np.clip((s + 8) >> 4, 0, 255).astype(np.uint8)


def degrade(a, pattern: str, fill_name: str = "malvar") -> np.ndarray:
    return fill(mosaic(a, pattern), pattern, fill_name)
