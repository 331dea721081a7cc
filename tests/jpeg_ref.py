"""The JPEG round trip decode(encode(x)) of uint8 pictures in libjpeg's integer ("islow") arithmetic and the PSNR-B
sums (include/grr.h, "JPEG round trip"), restated from their definition and independent of the package: int64 numpy
arrays for the codec (every intermediate is far inside 63 bits), Python ints for the metric.

    table(q, chroma)       the 8 x 8 quantisation table of quality q, natural order
    degrade(a, q, sub)     H x W x C uint8 (C 1 or 3; sub 0 = 4:4:4, 2 = 4:2:0) -> the decoded picture
    blocking(est)          (S_b, N_b, S_n, N_n)
    psnrb(est, ref)        float64
"""
import math

import numpy as np

LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
        14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
        49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
          47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32

C0_298, C0_390, C0_541, C0_765, C0_899, C1_175 = 2446, 3196, 4433, 6270, 7373, 9633
C1_501, C1_847, C1_961, C2_053, C2_562, C3_072 = 12299, 15137, 16069, 16819, 20995, 25172


def table(q, chroma=False):
    if isinstance(q, bool) or not isinstance(q, (int, np.integer)) or not 1 <= q <= 100:
        raise ValueError(f"quality is an integer of 1..100, got {q!r}")
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return np.array([min(max((b * scale + 50) // 100, 1), 255) for b in (CHROMA if chroma else LUMA)],
                    np.int64).reshape(8, 8)


def descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _odd(t4, t5, t6, t7):
    """The odd part both transforms share: four inputs -> the four sums before the final shift."""
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * C1_175
    t4, t5, t6, t7 = t4 * C0_298, t5 * C2_053, t6 * C3_072, t7 * C1_501
    z1, z2, z3, z4 = z1 * -C0_899, z2 * -C2_562, z3 * -C1_961 + z5, z4 * -C0_390 + z5
    return t4 + z1 + z3, t5 + z2 + z4, t6 + z2 + z3, t7 + z1 + z4


def fdct_1d(d, first):
    """jfdctint along the last axis of an int64 [..., 8] array; ``first``: the row pass."""
    d = [d[..., k] for k in range(8)]
    t0, t7, t1, t6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    t2, t5, t3, t4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    out = [None] * 8
    out[0] = (t10 + t11) << 2 if first else descale(t10 + t11, 2)
    out[4] = (t10 - t11) << 2 if first else descale(t10 - t11, 2)
    z1 = (t12 + t13) * C0_541
    out[2] = descale(z1 + t13 * C0_765, n)
    out[6] = descale(z1 - t12 * C1_847, n)
    o7, o5, o3, o1 = _odd(t4, t5, t6, t7)
    out[7], out[5], out[3], out[1] = descale(o7, n), descale(o5, n), descale(o3, n), descale(o1, n)
    return np.stack(out, axis=-1)


def idct_1d(c, first):
    """jidctint along the last axis; ``first``: the column pass (shift 11), else the row pass (shift 18)."""
    c = [c[..., k] for k in range(8)]
    z1 = (c[2] + c[6]) * C0_541
    t2, t3 = z1 - c[6] * C1_847, z1 + c[2] * C0_765
    t0, t1 = (c[0] + c[4]) << 13, (c[0] - c[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o0, o1, o2, o3 = _odd(c[7], c[5], c[3], c[1])
    n = 11 if first else 18
    out = [t10 + o3, t11 + o2, t12 + o1, t13 + o0, t13 - o0, t12 - o1, t11 - o2, t10 - o3]
    return np.stack([descale(v, n) for v in out], axis=-1)


def plane_codec(p, tab):
    """One int64 [h, w] plane of samples 0..255 through DCT, quantiser and inverse DCT: a plane of the same size."""
    h, w = p.shape
    hp, wp = -(-h // 8) * 8, -(-w // 8) * 8
    p = np.pad(p, ((0, hp - h), (0, wp - w)), mode="edge") - 128
    b = p.reshape(hp // 8, 8, wp // 8, 8).transpose(0, 2, 1, 3)                 # [by, bx, row, col]
    b = fdct_1d(b, True)                                                        # rows: along col
    b = fdct_1d(b.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2)           # columns
    v = tab * 8
    k = np.sign(b) * ((np.abs(b) + (v >> 1)) // v)
    b = k * tab
    b = idct_1d(b.transpose(0, 1, 3, 2), True).transpose(0, 1, 3, 2)            # columns first
    b = idct_1d(b, False)
    out = np.clip(b + 128, 0, 255)
    return out.transpose(0, 2, 1, 3).reshape(hp, wp)[:h, :w]


def fix(x):
    return int(x * 65536 + 0.5)


def chroma_down(p):
    """A full-resolution int64 chroma plane -> its 4:2:0 plane of ceil(H / 2) rows and a multiple of 8 columns."""
    h, w = p.shape
    p = np.pad(p, ((0, h % 2), (0, -(-w // 16) * 16 - w)), mode="edge")
    s = p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]
    bias = np.where(np.arange(s.shape[1]) % 2 == 0, 1, 2)
    return (s + bias) >> 2


def chroma_up(c, h, w):
    """Decoded chroma of ceil(h / 2) x ceil(w / 2) -> h x w."""
    ch, cw = c.shape
    if cw <= 2:
        return np.repeat(np.repeat(c, 2, axis=0), 2, axis=1)[:h, :w]
    out = np.empty((2 * ch, 2 * cw), np.int64)
    for y in range(2 * ch):
        near = y // 2
        far = min(max(near - 1 if y % 2 == 0 else near + 1, 0), ch - 1)
        s = 3 * c[near] + c[far]
        left = np.concatenate([[4 * s[0] + 8], 3 * s[1:] + s[:-1] + 8]) >> 4
        right = np.concatenate([3 * s[:-1] + s[1:] + 7, [4 * s[-1] + 7]]) >> 4
        out[y, 0::2], out[y, 1::2] = left, right
    return out[:h, :w]


def degrade(a, q, sub=0):
    a = np.asarray(a)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] not in (1, 3) or sub not in (0, 2) or 0 in a.shape:
        raise ValueError("an H x W x 1 or H x W x 3 uint8 picture and a subsampling of 0 or 2")
    h, w, c = a.shape
    x = a.astype(np.int64)
    if c == 1:
        return plane_codec(x[..., 0], table(q)).astype(np.uint8)[..., None]
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    y = (fix(.299) * r + fix(.587) * g + fix(.114) * b + 32768) >> 16
    cb = (-fix(.16874) * r - fix(.33126) * g + fix(.5) * b + (128 << 16) + 32767) >> 16
    cr = (fix(.5) * r - fix(.41869) * g - fix(.08131) * b + (128 << 16) + 32767) >> 16
    y = plane_codec(y, table(q))
    ct = table(q, True)
    if sub == 0:
        cb, cr = plane_codec(cb, ct), plane_codec(cr, ct)
    else:
        ch, cw = -(-h // 2), -(-w // 2)
        cb, cr = (chroma_up(plane_codec(chroma_down(p), ct)[:ch, :cw], h, w) for p in (cb, cr))
    cb, cr = cb - 128, cr - 128
    out = np.stack([y + ((fix(1.402) * cr + 32768) >> 16),
                    y + ((-fix(.34414) * cb - fix(.71414) * cr + 32768) >> 16),
                    y + ((fix(1.772) * cb + 32768) >> 16)], axis=-1)
    return np.clip(out, 0, 255).astype(np.uint8)


def blocking(est):
    """(S_b, N_b, S_n, N_n) of an H x W x C uint8 picture in Python ints: the squared differences and the counts of
    the adjacent pairs that straddle a multiple-of-8 line and of those that do not."""
    est = np.asarray(est)
    h, w, c = est.shape
    v = est.tolist()
    sb = nb = sn = nn = 0
    for y in range(h):
        for x in range(w):
            for k in range(c):
                if x + 1 < w:
                    d = (v[y][x][k] - v[y][x + 1][k]) ** 2
                    if x % 8 == 7:
                        sb, nb = sb + d, nb + 1
                    else:
                        sn, nn = sn + d, nn + 1
                if y + 1 < h:
                    d = (v[y][x][k] - v[y + 1][x][k]) ** 2
                    if y % 8 == 7:
                        sb, nb = sb + d, nb + 1
                    else:
                        sn, nn = sn + d, nn + 1
    return sb, nb, sn, nn


def psnrb_from_sums(sse, h, w, c, sb, nb, sn, nn):
    db, dn = sb / nb, sn / nn
    bef = 3.0 / math.log2(min(h, w)) * (db - dn) if db > dn else 0.0
    den = sse / (h * w * c) + bef
    return math.inf if den == 0 else 10.0 * math.log10(255.0 ** 2 / den)


def psnrb(est, ref):
    est, ref = np.asarray(est), np.asarray(ref)
    h, w, c = est.shape
    if est.shape != ref.shape or min(h, w) < 16:
        raise ValueError("two pictures of one shape with both sides at least 16")
    sse = sum((int(p) - int(r)) ** 2 for p, r in zip(est.ravel().tolist(), ref.ravel().tolist()))
    return psnrb_from_sums(sse, h, w, c, *blocking(est))
