"""An independent oracle for the 2-D blur of include/grr.h, in plain numpy and plain Python, in two forms that
tests/test_blur_ref.py holds to each other:

  blur(a, table, boundary)        form A: per tap, the sum of index-gathered slices in int64
  blur_loops(a, table, boundary)  form B: a loop per output byte with its own boundary arithmetic (tiny shapes only)

and the quantiser restated (``quantise``).  Nothing here imports the library: the boundary rules, the flip of the
convolution, the rounding and the quantiser are written again from the definition.

  out[y, x, c] = (32768 + sum_{i, j} W[i][j] * a[b(y + kh // 2 - i, H), b(x + kw // 2 - j, W), c]) >> 16
"""
import math

import numpy as np

ONE = 65536
BOUNDARIES = ("wrap", "replicate", "reflect")


def index_of(t: int, n: int, boundary: str) -> int:
    """b(t, n) for one integer, by walking: no modulo, so it shares nothing with the vectorised form."""
    if boundary == "replicate":
        return 0 if t < 0 else (n - 1 if t >= n else t)
    if boundary == "wrap":
        while t < 0:
            t += n
        while t >= n:
            t -= n
        return t
    assert boundary == "reflect"
    if n == 1:
        return 0
    while t < 0 or t >= n:          # fold about the edge samples until inside
        t = -t if t < 0 else 2 * (n - 1) - t
    return t


def indices(lo: int, hi: int, n: int, boundary: str) -> np.ndarray:
    """b(t, n) for t in [lo, hi), vectorised with modulo arithmetic."""
    t = np.arange(lo, hi, dtype=np.int64)
    if boundary == "wrap":
        return np.mod(t, n)
    if boundary == "replicate":
        return np.minimum(np.maximum(t, 0), n - 1)
    assert boundary == "reflect"
    if n == 1:
        return np.zeros_like(t)
    period = 2 * (n - 1)
    m = np.mod(t, period)
    return np.where(m >= n, period - m, m)


def blur(a: np.ndarray, table: np.ndarray, boundary: str) -> np.ndarray:
    """Form A.  ``a``: uint8 H x W x C; ``table``: integer [kh, kw]."""
    a = np.asarray(a)
    assert a.dtype == np.uint8 and a.ndim == 3
    table = np.asarray(table).astype(np.int64)
    kh, kw = table.shape
    h, w = a.shape[:2]
    wide = a.astype(np.int64)
    total = np.zeros(a.shape, np.int64)
    for i in range(kh):
        rows = indices(kh // 2 - i, kh // 2 - i + h, h, boundary)
        for j in range(kw):
            if table[i, j]:
                cols = indices(kw // 2 - j, kw // 2 - j + w, w, boundary)
                total += table[i, j] * np.take(np.take(wide, rows, axis=0), cols, axis=1)
    return ((total + 32768) >> 16).astype(np.uint8)


def blur_loops(a: np.ndarray, table: np.ndarray, boundary: str) -> np.ndarray:
    """Form B: Python integers, one output byte at a time."""
    a = np.asarray(a)
    kh, kw = np.asarray(table).shape
    h, w, c = a.shape
    px, tb = a.tolist(), np.asarray(table).tolist()
    out = np.zeros(a.shape, np.uint8)
    for y in range(h):
        for x in range(w):
            for ch in range(c):
                s = 32768
                for i in range(kh):
                    yy = index_of(y + kh // 2 - i, h, boundary)
                    for j in range(kw):
                        if tb[i][j]:
                            s += tb[i][j] * px[yy][index_of(x + kw // 2 - j, w, boundary)][ch]
                out[y, x, ch] = s >> 16
    return out


def quantise(k) -> np.ndarray:
    """The quantiser of include/grr.h with Python numbers: q = k / sum(k) * 65536 in float64 (the sum correctly
    rounded), floor, then the units left over to the largest fractional parts, ties to the lower flat index."""
    k = np.asarray(k, dtype=np.float64)
    flat = [float(v) for v in k.ravel()]
    total = math.fsum(flat)
    q = [v / total * 65536.0 for v in flat]
    w = [int(math.floor(v)) for v in q]
    left = ONE - sum(w)
    assert 0 <= left <= len(w)
    by_fraction = sorted(range(len(w)), key=lambda n: (-(q[n] - w[n]), n))
    for n in by_fraction[:left]:
        w[n] += 1
    return np.array(w, dtype=np.int32).reshape(k.shape)


def random_table(rs, kh: int, kw: int) -> np.ndarray:
    """A valid table of distinct-looking weights."""
    return quantise(rs.rand(kh, kw) + 0.05)


def lone_tap(kh: int, kw: int, i: int, j: int) -> np.ndarray:
    t = np.zeros((kh, kw), np.int32)
    t[i, j] = ONE
    return t
