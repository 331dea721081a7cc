"""Numpy restatement of grr_patch_mask_batch / grr_u8_mask_fill (include/grr.h): the Bernoulli mask of (seed, sample
id, window element), the zero fill and the normalised convolution in exact integers, the turn by T_mode."""
import numpy as np

from tests.patch_ref import philox4x32_10, picture, sym, transform        # noqa: F401 (picture: for the tests)

HALO, MAX_SIDE, ONE = 7, 15, 1 << 24


def mask_bits(seed, sample_id, ph, pw, keep):
    """The known bits of the (ph + 14) x (pw + 14) window of a sample, bool: element e = wy (pw + 14) + wx is word
    e % 4 of Philox block e // 4 with counter (e // 4, 1, id), known if (x >> 8) < keep (clamped into [0, 2^24])."""
    keep = min(max(int(keep), 0), ONE)
    wh, ww = ph + 2 * HALO, pw + 2 * HALO
    if keep in (0, ONE):
        return np.full((wh, ww), keep == ONE)
    seed, sample_id = int(seed), int(sample_id) & ((1 << 64) - 1)
    count = wh * ww
    blocks = -(-count // 4)
    ctr = np.zeros((blocks, 4), np.uint64)
    ctr[:, 0] = np.arange(blocks, dtype=np.uint64)
    ctr[:, 1] = 1
    ctr[:, 2], ctr[:, 3] = sample_id & 0xFFFFFFFF, sample_id >> 32
    x = philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64)).reshape(-1)[:count]
    return ((x >> np.uint32(8)).astype(np.int64) < keep).reshape(wh, ww)


def window(img, row, col, ph, pw):
    """The (ph + 14) x (pw + 14) x C window of a patch: position (wy, wx) is pixel (sym(row + wy - 7), sym(col + wx - 7))."""
    h, w = img.shape[:2]
    ys = [sym(row + wy - HALO, h) for wy in range(ph + 2 * HALO)]
    xs = [sym(col + wx - HALO, w) for wx in range(pw + 2 * HALO)]
    return img[np.ix_(ys, xs)]


def fill_window(win, known, weights, fill, hole):
    """(filled core ph x pw x C uint8, code ph x pw uint8) of a window and its known bits: code 1 known, 2 filled with
    den > 0, 0 left a hole (the zero fill leaves every missing pixel 0 with code 0)."""
    ph, pw = win.shape[0] - 2 * HALO, win.shape[1] - 2 * HALO
    core = win[HALO:HALO + ph, HALO:HALO + pw].astype(np.int64)
    k = known.astype(np.int64)
    kc = k[HALO:HALO + ph, HALO:HALO + pw]
    code = kc.astype(np.uint8)
    if fill in (0, "zero"):
        return (core * kc[:, :, None]).astype(np.uint8), code
    weights = np.asarray(weights, dtype=np.int64)
    kh, kw = weights.shape
    assert kh % 2 == 1 and kw % 2 == 1 and max(kh, kw) <= MAX_SIDE
    ry, rx = kh // 2, kw // 2
    vk = win.astype(np.int64) * k[:, :, None]
    den = np.zeros((ph, pw), np.int64)
    num = np.zeros((ph, pw, win.shape[2]), np.int64)
    for i in range(kh):
        for j in range(kw):
            ys, xs = HALO + i - ry, HALO + j - rx
            den += weights[i, j] * k[ys:ys + ph, xs:xs + pw]
            num += weights[i, j] * vk[ys:ys + ph, xs:xs + pw]
    safe = np.maximum(den, 1)[:, :, None]
    value = np.where(den[:, :, None] > 0, (2 * num + den[:, :, None]) // (2 * safe), int(hole))
    out = np.where(kc[:, :, None] > 0, core, value)
    code = np.where(kc > 0, 1, np.where(den > 0, 2, 0)).astype(np.uint8)
    return out.astype(np.uint8), code


def mask_fill_patch(images, rows, sample_ids, keeps, seed, ph, pw, weights, fill, hole, bits=None):
    """(target, input, mask) of grr_patch_mask_batch, float32 [n, C, ph, pw] and [n, 1, ph, pw]; images: uint8
    H x W x C arrays; rows: (img, row, col, mode), the mode read as & 5 where ph != pw.  ``bits``: a list of window
    bit arrays to use in place of the drawn ones."""
    target, inp, mask = [], [], []
    for s, ((im, row, col, mode), sid, keep) in enumerate(zip(rows, sample_ids, keeps)):
        mode = int(mode) & 7
        if ph != pw:
            mode &= 5
        win = window(images[im], row, col, ph, pw)
        known = mask_bits(seed, sid, ph, pw, keep) if bits is None else bits[s]
        filled, code = fill_window(win, known, weights, fill, hole)
        clean = win[HALO:HALO + ph, HALO:HALO + pw]
        f32 = lambda a: (transform(a, mode).astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1)  # noqa: E731
        target.append(f32(clean))
        inp.append(f32(filled))
        mask.append(transform((code == 1)[:, :, None], mode).astype(np.float32).transpose(2, 0, 1))
    return tuple(np.ascontiguousarray(np.stack(v)) for v in (target, inp, mask))


def mask_fill_image(img, mask_in, keep, seed, sample_id, weights, fill, hole):
    """(dst H x W x C uint8, mask_out H x W uint8) of grr_u8_mask_fill: ``mask_in`` None draws the mask of (seed,
    sample_id), else nonzero means known and the values are carried through."""
    h, w = img.shape[:2]
    win = window(img, 0, 0, h, w)
    if mask_in is None:
        known = mask_bits(seed, sample_id, h, w, keep)
        carried = None
    else:
        mwin = window(np.asarray(mask_in)[:, :, None], 0, 0, h, w)[:, :, 0]
        known, carried = mwin != 0, np.asarray(mask_in)
    filled, code = fill_window(win, known, weights, fill, hole)
    if carried is not None:
        code = np.where(carried != 0, carried, code).astype(np.uint8)
    return filled, code
