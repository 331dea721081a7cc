"""An independent oracle of grr_patch_raw_batch (include/grr.h has the definition): sensor noise on the Bayer mosaic,
quantised, before the fill.  It imports nothing of the package: the Philox normals and T_mode come from
tests/patch_ref.py, the site, the reflection and the coefficient sets from tests/demosaic_ref.py.  Two forms:
``sample_loops`` walks the window and the patch in Python floats and integers, straight from the definition;
``sample`` is vectorised numpy for the larger shapes.  tests/test_raw_noise_ref.py holds the two to each other.

Both return (target, input, s, margin): target and input float32 [3, ph', pw'] after T_mode, s the int64 sums in
sixteenths [ph, pw, 3] before it, and margin = min |frac(t full) - 1/2| over the window samples the clip does not pin:
how far the sample's roundings are from a tie.  Float64 evaluation orders differ by about 1e-9 there, so a fixture with
a margin of 1e-6 has one answer."""
import math

import numpy as np

from tests import demosaic_ref as dr
from tests import patch_ref as pr

Q_MAX = 1 << 24


def f32(v) -> float:
    return float(np.float32(v))


def read_b(read: float) -> float:
    """The read-noise variance of a level in 8-bit units: float32((read / 255)^2)."""
    return f32((read / 255.0) ** 2)


def legal_mode(mode: int, ph: int, pw: int) -> int:
    mode &= 7
    return mode & 5 if (mode & 2) and ph != pw else mode


def _which(pattern: str, y: int, x: int, ch: int):
    """The coefficient set of channel ``ch`` at picture pixel (y, x), or None where it is measured."""
    here = dr.site(pattern, y, x)
    if ch == here:
        return None
    if ch == 1:
        return "green"
    if here != 1:
        return "other"
    return "inrow" if dr.site(pattern, y, x + 1) == ch else "incol"      # the row's colour at a G site


def window_normals(seed: int, sample_id: int, ph: int, pw: int) -> np.ndarray:
    """z_e of the (ph + 4) x (pw + 4) window, e = wy (pw + 4) + wx."""
    return pr.normals(seed, sample_id, (ph + 4) * (pw + 4)).reshape(ph + 4, pw + 4)


def _finish(img, ys, xs, s, full, mode, ph, pw):
    target = img[np.asarray(ys[2:-2])[:, None], np.asarray(xs[2:-2])[None, :]].astype(np.float32) / np.float32(255.0)
    inp = (s.astype(np.float64) / (16.0 * full)).astype(np.float32)
    mode = legal_mode(mode, ph, pw)
    turn = lambda a: np.ascontiguousarray(pr.transform(a, mode).transpose(2, 0, 1))
    return turn(target), turn(inp)


def sample_loops(img, pattern: str, row: int, col: int, mode: int, ph: int, pw: int, a: float, b: float, seed: int,
                 sample_id: int, fill: str = "malvar", bits: int = 16, clip: bool = True, z=None):
    img = np.asarray(img)
    h, w = img.shape[:2]
    a, b, full = f32(a), f32(b), (1 << bits) - 1
    z = window_normals(seed, sample_id, ph, pw) if z is None else z
    ys = [dr.reflect(row + wy - 2, h) for wy in range(ph + 4)]
    xs = [dr.reflect(col + wx - 2, w) for wx in range(pw + 4)]
    q = [[0] * (pw + 4) for _ in range(ph + 4)]
    margin = 0.5
    for wy in range(ph + 4):
        for wx in range(pw + 4):
            x = int(img[ys[wy], xs[wx], dr.site(pattern, ys[wy], xs[wx])]) / 255.0
            var = a * x + b
            t = x + math.sqrt(var) * float(z[wy, wx]) if var != 0 else x
            pinned = clip and not 0.0 <= t <= 1.0
            if clip:
                t = min(max(t, 0.0), 1.0)
            tf = t * full
            if not pinned:
                margin = min(margin, abs(tf - math.floor(tf) - 0.5))
            q[wy][wx] = min(max(round(tf), -Q_MAX), Q_MAX)       # Python rounds ties to even
    s = np.zeros((ph, pw, 3), np.int64)
    for i in range(ph):
        for j in range(pw):
            for ch in range(3):
                which = _which(pattern, ys[i + 2], xs[j + 2], ch)
                if which is None:
                    s[i, j, ch] = 16 * q[i + 2][j + 2]
                else:
                    s[i, j, ch] = sum(wt * q[i + 2 + dy][j + 2 + dx] for (dy, dx), wt in dr.COEFFS[fill][which].items())
    return _finish(img, ys, xs, s, full, mode, ph, pw) + (s, margin)


def sample(img, pattern: str, row: int, col: int, mode: int, ph: int, pw: int, a: float, b: float, seed: int,
           sample_id: int, fill: str = "malvar", bits: int = 16, clip: bool = True, z=None):
    img = np.asarray(img)
    h, w = img.shape[:2]
    a, b, full = f32(a), f32(b), (1 << bits) - 1
    z = window_normals(seed, sample_id, ph, pw) if z is None else z
    ys = np.array([dr.reflect(row + wy - 2, h) for wy in range(ph + 4)])
    xs = np.array([dr.reflect(col + wx - 2, w) for wx in range(pw + 4)])
    ry, rx = dr.R_SITE[pattern]
    py, px = ((ys % 2) != ry).astype(np.int64)[:, None], ((xs % 2) != rx).astype(np.int64)[None, :]
    x = img[ys[:, None], xs[None, :], py + px].astype(np.float64) / 255.0
    var = a * x + b
    with np.errstate(invalid="ignore"):
        t = np.where(var != 0, x + np.sqrt(var) * z, x)
    pinned = (t < 0.0) | (t > 1.0) if clip else np.zeros(t.shape, bool)
    if clip:
        t = np.clip(t, 0.0, 1.0)
    tf = t * full
    frac = np.abs(tf - np.floor(tf) - 0.5)
    margin = float(frac[~pinned].min()) if (~pinned).any() else 0.5
    q = np.clip(np.rint(tf), -Q_MAX, Q_MAX).astype(np.int64)
    at = lambda dy, dx: q[2 + dy:2 + dy + ph, 2 + dx:2 + dx + pw]
    corr = {name: sum(wt * at(dy, dx) for (dy, dx), wt in k.items()) + np.zeros((ph, pw), np.int64)
            for name, k in dr.COEFFS[fill].items()}
    cy, cx = py[2:-2], px[:, 2:-2]
    red, blue = (cy == 0) & (cx == 0), (cy == 1) & (cx == 1)
    g_red_row, ctr = (cy == 0) & (cx == 1), 16 * at(0, 0)
    s = np.zeros((ph, pw, 3), np.int64)
    s[:, :, 1] = np.where(red | blue, corr["green"], ctr)
    s[:, :, 0] = np.where(red, ctr, np.where(blue, corr["other"], np.where(g_red_row, corr["inrow"], corr["incol"])))
    s[:, :, 2] = np.where(blue, ctr, np.where(red, corr["other"], np.where(g_red_row, corr["incol"], corr["inrow"])))
    return _finish(img, ys, xs, s, full, mode, ph, pw) + (s, margin)


def batch(images, patterns, rows, sample_ids, noise, seed: int, ph: int, pw: int, fill: str = "malvar", bits: int = 16,
          clip: bool = True):
    """(target, input, margin) of grr_patch_raw_batch: float32 [n, 3, ph, pw] each and the smallest tie margin.
    images: uint8 H x W x 3 arrays; patterns: one name per image; rows: (img, row, col, mode); noise: (a, b) per row, or
    None."""
    targets, inputs, margin = [], [], 0.5
    for k, ((im, row, col, mode), sid) in enumerate(zip(rows, sample_ids)):
        a, b = (0.0, 0.0) if noise is None else noise[k]
        tg, inp, _, m = sample(images[im], patterns[im], int(row), int(col), int(mode), ph, pw, a, b, seed, int(sid), fill,
                               bits, clip)
        targets.append(tg)
        inputs.append(inp)
        margin = min(margin, m)
    return np.stack(targets), np.stack(inputs), margin


# ---- the fixtures of the GPU tests (tests/test_gpu_raw_noise.py); tests/test_raw_noise_ref.py checks their tie margins
SHAPES = ((1, 7), (2, 2), (5, 3), (40, 56), (100, 70))       # a side of 1, periodic reflection, two tiled pictures
SEED = 2204
SHOT, READ = 0.01, 5.0
N = 40
TIE_MARGIN = 1e-6


def pictures():
    return [pr.picture(k + 1, h, w) for k, (h, w) in enumerate(SHAPES)]


def patterns_of(shift: int):
    """One pattern per picture, all four in every call; ``shift`` moves them along the pictures."""
    return [dr.PATTERNS[(k + shift) % 4] for k in range(len(SHAPES))]


def rows_of(n: int, ph: int, pw: int):
    """n rows (img, row, col, mode): the pictures in turn, origins of every parity, all legal modes."""
    modes = list(range(8)) if ph == pw else [0, 1, 4, 5]
    rows = []
    for s in range(n):
        img = s % len(SHAPES)
        h, w = SHAPES[img]
        rows.append((img, (s // 5 * 3 + s // 10) % h, (s // 5 * 5 + s // 20) % w, modes[(s // 2) % len(modes)]))
    return rows


def ids_of(n: int):
    return np.array([(3 << 32) | (s * 11 + 1) for s in range(n)], dtype=np.int64)


def noise_of(n: int):
    """(a, b) per row: none, read only, shot only, both."""
    b = read_b(READ)
    combos = ((0.0, 0.0), (0.0, b), (SHOT, 0.0), (SHOT, b))
    return np.array([combos[(s // 3) % 4] for s in range(n)], dtype=np.float32)


# (ph, pw, fill, bits, clip, pattern shift): 16 x 16 under every fill, depth and clip; 6 x 6 (window rows that start off
# a Philox block), 16 x 32 (even modes only) and 20 x 70 (across the 16-row and 64-column tile seams)
GPU_CASES = [(16, 16, fill, bits, clip, k) for k, (fill, bits, clip) in
             enumerate((f, d, c) for f in dr.FILLS for d in (8, 12, 16) for c in (False, True))]
GPU_CASES += [(6, 6, "malvar", 16, True, 0), (6, 6, "bilinear", 8, False, 1), (6, 6, "zero", 12, True, 2),
              (16, 32, "malvar", 12, False, 3), (16, 32, "bilinear", 16, True, 0),
              (20, 70, "malvar", 16, True, 1), (20, 70, "bilinear", 12, False, 2), (20, 70, "malvar", 8, True, 3)]

_CASES = {}


def gpu_case(case):
    """What a GPU case asks and what the oracle answers, computed once: dict(images, patterns, rows, ids, noise, target,
    input, margin)."""
    if case not in _CASES:
        ph, pw, fill, bits, clip, shift = case
        images, patterns = pictures(), patterns_of(shift)
        rows, ids, noise = rows_of(N, ph, pw), ids_of(N), noise_of(N)
        target, inp, margin = batch(images, patterns, rows, ids, noise, SEED, ph, pw, fill, bits, clip)
        for v in (target, inp):
            v.setflags(write=False)
        _CASES[case] = dict(images=images, patterns=patterns, rows=rows, ids=ids, noise=noise, target=target, input=inp,
                            margin=margin)
    return _CASES[case]


# whole pictures 3 and 4 of SHAPES with sample id 0 and 1 under (SHOT, READ): the one-image form and evaluate_jdd
WHOLE_CASES = (("rggb", "malvar", 16, True), ("bggr", "bilinear", 12, False), ("grbg", "zero", 8, True))

# a training.NoisyBayerDemosaicking over patch_ref.write_pictures: per-file patterns, per-sample levels, all 8 modes
LOADER_CONF = dict(pattern=[["rggb", "grbg", "gbrg", "bggr"], [0.25, 0.25, 0.25, 0.25]], fill="malvar",
                   shot=[[0.0, 0.005, 0.02], [0.2, 0.4, 0.4]], read=[[0.0, 2.0, 8.0], [0.2, 0.4, 0.4]], bits=12, clip=True,
                   use_data_aug=True, patch_size=(16, 16), max_num_patchs=40, seed=2204)


def loader_reference(dataset, loader, epoch: int, pics):
    """(target, input, margin) of an epoch of a DevicePatchLoader over a NoisyBayerDemosaicking dataset, in dataset
    order, from what the two say they drew: the plan, the files' patterns, epoch_draws' modes and epoch_noise's pairs."""
    modes, _ = loader.epoch_draws(epoch)
    noise = loader.epoch_noise(epoch)
    rows = [(img, r, c, modes[p]) for p, (r, c, _, img) in enumerate(dataset.patchs_data)]
    ids = (epoch << 32) | np.arange(len(dataset), dtype=np.int64)
    ph, pw = dataset.out_size()
    return batch(pics, dataset.patterns, rows, ids, noise, dataset.seed, ph, pw, dataset.fill, dataset.bits, dataset.clip)
