"""The exact bicubic resize of uint8 pictures (include/grr.h, "bicubic resize"), restated from its definition and
independent of the package: rational weights from ``fractions``, one explicit int64 multiply-add per tap.

    taps(s, up)            the quantised tap sets: one tuple per phase of (offset, q) pairs, zero taps dropped
    down(a, s)             H x W x C -> ceil(H / s) x ceil(W / s) x C
    up(a, s, h, w)         H x W x C -> h x w x C, s (H - 1) < h <= s H and likewise w (default: s H x s W)
    degrade(a, s)          up(down(a, s), s, H, W)
"""
from fractions import Fraction
from functools import lru_cache

import numpy as np

ONE = 1 << 30


def cubic(x):
    x = abs(Fraction(x))
    if x <= 1:
        return Fraction(3, 2) * x ** 3 - Fraction(5, 2) * x ** 2 + 1
    if x < 2:
        return Fraction(-1, 2) * x ** 3 + Fraction(5, 2) * x ** 2 - 4 * x + 2
    return Fraction(0)


def quantise(offsets, raw):
    """One tap set: raw / sum(raw), round half to even at 2^-30, the remainder to the largest (lowest index among
    equals), zero taps dropped."""
    total = sum(raw)
    q = [round(w / total * ONE) for w in raw]          # round() of a Fraction is half-to-even
    q[q.index(max(q))] += ONE - sum(q)
    return tuple((o, v) for o, v in zip(offsets, q) if v != 0)


@lru_cache(maxsize=None)
def taps(s, up):
    """Down: one phase, offsets from i s.  Up: s phases, offsets from b = y // s."""
    if up:
        phases = []
        for p in range(s):
            u = Fraction(2 * p + 1, 2 * s) - Fraction(1, 2)
            js = [j for j in range(-3, 4) if abs(u - j) < 2]
            phases.append(quantise(js, [cubic(u - j) for j in js]))
        return tuple(phases)
    u = Fraction(s, 2) - Fraction(1, 2)                # the centre of output 0
    js = [j for j in range(-3 * s, 4 * s) if abs(u - j) < 2 * s]
    return (quantise(js, [cubic((u - j) / s) for j in js]),)


def sym(r, n):
    t = r % (2 * n)                                    # Python's %: non-negative
    return t if t < n else 2 * n - 1 - t


def _rows(a, s, up_to):
    """One pass along axis 0 of an [n, ...] uint8 array: down (up_to None) or up to ``up_to`` rows."""
    n = a.shape[0]
    is_up = up_to is not None
    length = up_to if is_up else -(-n // s)
    if is_up and not s * (n - 1) < length <= s * n:
        raise ValueError(f"up: {length} rows from {n} at scale {s}")
    table = taps(s, is_up)
    src = a.astype(np.int64)
    out = np.empty((length,) + a.shape[1:], np.uint8)
    for y in range(length):
        phase, base = (table[y % s], y // s) if is_up else (table[0], y * s)
        acc = np.zeros(a.shape[1:], np.int64)
        for off, q in phase:
            acc += np.int64(q) * src[sym(base + off, n)]
        out[y] = np.clip((acc + (ONE >> 1)) >> 30, 0, 255).astype(np.uint8)
    return out


def _check(a, s):
    a = np.asarray(a)
    if a.dtype != np.uint8 or a.ndim != 3 or not 2 <= s <= 8:
        raise ValueError("an H x W x C uint8 picture and a scale of 2..8")
    return a


def down(a, s):
    a = _check(a, s)
    rows = _rows(a, s, None)
    return _rows(rows.transpose(1, 0, 2), s, None).transpose(1, 0, 2).copy()


def up(a, s, h=None, w=None):
    a = _check(a, s)
    h = s * a.shape[0] if h is None else h
    w = s * a.shape[1] if w is None else w
    rows = _rows(a, s, h)
    return _rows(rows.transpose(1, 0, 2), s, w).transpose(1, 0, 2).copy()


def degrade(a, s):
    a = _check(a, s)
    return up(down(a, s), s, a.shape[0], a.shape[1])
