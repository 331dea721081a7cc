"""Numpy restatement of the geometric self-ensemble of irdu_amd.restore (``ensemble=``), for the tests.

Mode m = 2k + f is ``np.rot90(a, k)`` (k quarter turns counter-clockwise), then ``np.flipud`` if f; the mean is
the float32 pairwise tree over the listed order.  Built on tests/restore_ref.py's gather / scatter: nothing here
shares code with the kernels, only the plan.
"""
import numpy as np

from tests import restore_ref as R

EVEN, ODD = (0, 1, 4, 5), (2, 3, 6, 7)


def transform(a, m):
    """T_m on the last two axes of a."""
    t = np.rot90(a, m // 2, axes=(-2, -1))
    return np.ascontiguousarray(np.flip(t, axis=-2) if m % 2 else t)


def inverse(t, m):
    """T_m^-1 on the last two axes of t."""
    t = np.flip(t, axis=-2) if m % 2 else t
    return np.ascontiguousarray(np.rot90(t, -(m // 2), axes=(-2, -1)))


def split(modes):
    return tuple(m for m in modes if m in EVEN), tuple(m for m in modes if m in ODD)


def tree_mean(zs):
    """float32: [z0 + z1, z2 + z3, ..., the odd one carried] until one is left, divided by float32(M)."""
    level = [np.asarray(z, np.float32) for z in zs]
    with np.errstate(all="ignore"):
        while len(level) > 1:
            nxt = [level[k] + level[k + 1] for k in range(0, len(level) - 1, 2)]
            if len(level) % 2:
                nxt.append(level[-1])
            level = nxt
        return (level[0] / np.float32(len(zs))).astype(np.float32)


def sequential_mean(zs):
    """The left-to-right sum the kernels must NOT form (the tests show the two differ on their inputs)."""
    acc = np.asarray(zs[0], np.float32)
    with np.errstate(all="ignore"):
        for z in zs[1:]:
            acc = acc + np.asarray(z, np.float32)
        return (acc / np.float32(len(zs))).astype(np.float32)


def window_major(members):
    """[n M, ...] from M arrays [n, ...]: row w M + j is member j of window w."""
    return np.ascontiguousarray(np.stack(members, axis=1).reshape((-1,) + members[0].shape[1:]))


def gather_d8(img, p, modes, factor=16):
    """[n M, C, bh, bw] for modes of one orientation: row w M + j = T_modes[j] of window w of R.gather."""
    x = R.gather(img, p, factor)
    return window_major([transform(x, m) for m in modes])


def members_to_batches(zs, modes):
    """(y0, y1) the kernels take from the members z_j [n, C, th, tw] in the picture's frame: T_mj(z_j), the
    even-k ones in y0 and the odd-k ones in y1, window-major; None where an orientation has no mode."""
    out = []
    for ms in split(modes):
        out.append(window_major([transform(zs[modes.index(m)], m) for m in ms]) if ms else None)
    return out


def scatter_mean(y0, y1, p, modes, quantise=True):
    """The H x W x C image from the two result batches."""
    even, odd = split(modes)
    n = len(p.windows)
    zs = []
    for m in modes:
        y, ms = (y0, even) if m in even else (y1, odd)
        zs.append(inverse(y.reshape((n, len(ms)) + y.shape[1:])[:, ms.index(m)], m))
    return finish(tree_mean(zs), p, quantise)


def finish(mean, p, quantise):
    """R.scatter of the mean; a NaN writes 0 to a uint8 image."""
    return R.scatter(np.where(np.isnan(mean), np.float32(0), mean) if quantise else mean, p, quantise)


def restore(fn, img, p, modes, quantise=True, factor=16):
    """The whole call: fn maps a numpy batch to the numpy output batch and does not look across the batch."""
    x = R.gather(img, p, factor)
    zs = [inverse(np.asarray(fn(transform(x, m)), np.float32), m) for m in modes]
    return finish(tree_mean(zs), p, quantise)
