"""CPU checks of the exact bicubic resize: the oracle tests/resize_ref.py against its own definition, a brute-force
evaluation and Pillow; kernels.resize_taps and training.bicubic_degrade_u8 against the oracle; the host path of
training.BicubicSuperResolution.  Launches nothing."""
import logging
from fractions import Fraction

import numpy as np
import pytest

from tests import patch_ref, resize_ref

SCALES = (2, 3, 4, 8)
# (H, W, C, s) of tests/test_gpu_resize.py
SHAPES = [(1, 1, 1, 2), (5, 3, 3, 4), (5, 3, 3, 8), (7, 13, 3, 3), (16, 16, 1, 2), (40, 24, 4, 8), (67, 131, 3, 4),
          (130, 70, 3, 2)]


def random_picture(h, w, c, seed=0):
    return np.random.RandomState(seed + 131 * h + w).randint(0, 256, (h, w, c)).astype(np.uint8)


def checkerboard(h, w, c):
    y, x, _ = np.meshgrid(np.arange(h), np.arange(w), np.arange(c), indexing="ij")
    return (((y + x) % 2) * 255).astype(np.uint8)


def test_tap_tables_sum_to_one_and_have_the_counts_of_the_definition():
    from irdu_amd import kernels as K
    for s, n_down in zip(SCALES, (8, 9, 16, 32)):
        (down,) = resize_ref.taps(s, False)
        assert len(down) == n_down and sum(q for _, q in down) == 1 << 30
        assert all(abs(Fraction(s - 1, 2) - o) < 2 * s for o, _ in down)
        up = resize_ref.taps(s, True)
        assert len(up) == s
        for p, phase in enumerate(up):
            assert 1 <= len(phase) <= 4 and sum(q for _, q in phase) == 1 << 30 and all(q for _, q in phase)
            assert len(phase) == (1 if s % 2 and p == s // 2 else 4)
        assert sum(abs(q) for _, q in down) <= 1.19 * (1 << 30)
        for up_ in (False, True):
            assert K.resize_taps(s, up_) == resize_ref.taps(s, up_)
            assert K.resize_taps(s, up_) is K.resize_taps(s, up_)                # cached
    for s in range(2, 9):            # every legal scale, the ones without a count above included
        for up_ in (False, True):
            assert K.resize_taps(s, up_) == resize_ref.taps(s, up_)
    for bad in (1, 9, 0):
        with pytest.raises(ValueError, match="scale"):
            K.resize_taps(bad, False)


def test_the_dense_tap_arguments_are_the_table_with_its_zeros_put_back():
    from irdu_amd import kernels as K
    for s in range(2, 9):
        for up_ in (False, True):
            n_phase, first, count, flat = K._resize_tap_args(s, up_)
            table = resize_ref.taps(s, up_)
            assert n_phase == len(table) == (s if up_ else 1)
            at = 0
            for p, phase in enumerate(table):
                dense = {first[p] + k: flat[at + k] for k in range(count[p])}
                assert {o: q for o, q in dense.items() if q} == dict(phase) and count[p] <= 4 * s
                at += count[p]
            assert at == len(flat)


@pytest.mark.parametrize("s", SCALES)
def test_a_constant_picture_is_a_fixed_point(s):
    for value in (0, 77, 255):
        a = np.full((11, 6, 3), value, np.uint8)
        assert np.array_equal(resize_ref.degrade(a, s), a)
        assert (resize_ref.down(a, s) == value).all() and (resize_ref.up(a, s) == value).all()


def brute_pass(a, s, up_to):
    """One pass along axis 0 from the definition: the input mirrored explicitly into a padded array, so no index
    arithmetic modulo 2n is shared with the oracle."""
    n = a.shape[0]
    pad = 4 * s + 2
    period = np.concatenate([a, a[::-1]])                     # abc cba, repeated: ...cba|abc|cba...
    reps = pad // (2 * n) + 2
    line = np.concatenate([period] * (2 * reps + 1))          # index 0 of ``a`` is at reps * 2n
    zero = reps * 2 * n
    is_up = up_to is not None
    length = up_to if is_up else -(-n // s)
    out = np.empty((length,) + a.shape[1:], np.uint8)
    for y in range(length):
        if is_up:
            u = Fraction(2 * (y % s) + 1, 2 * s) - Fraction(1, 2)
            js = [j for j in range(-4, 5) if abs(u - j) < 2]
            ws, at = [resize_ref.cubic(u - j) for j in js], y // s
        else:
            u = Fraction(2 * y + 1, 2) * s - Fraction(1, 2)
            js = [j for j in range(y * s - 3 * s, y * s + 4 * s) if abs(u - j) < 2 * s]
            ws, at = [resize_ref.cubic((u - j) / s) for j in js], 0
        total = sum(ws)
        q = [round(w / total * (1 << 30)) for w in ws]
        q[q.index(max(q))] += (1 << 30) - sum(q)
        acc = sum(int(qk) * line[zero + at + j].astype(np.int64) for j, qk in zip(js, q))
        out[y] = np.clip((acc + (1 << 29)) >> 30, 0, 255)
    return out


@pytest.mark.parametrize("s", (4, 8))
def test_sides_smaller_than_the_support_match_a_brute_force_evaluation(s):
    a = random_picture(5, 3, 3)
    rows = brute_pass(a, s, None)
    low = brute_pass(rows.transpose(1, 0, 2), s, None).transpose(1, 0, 2)
    assert low.shape == (-(-5 // s), 1, 3) and np.array_equal(resize_ref.down(a, s), low)
    rows = brute_pass(low, s, 5)
    back = brute_pass(rows.transpose(1, 0, 2), s, 3).transpose(1, 0, 2)
    assert np.array_equal(resize_ref.up(low, s, 5, 3), back) and np.array_equal(resize_ref.degrade(a, s), back)


@pytest.mark.parametrize("h,w,c,s", SHAPES)
def test_the_numpy_degradation_is_the_oracle_bit_for_bit(h, w, c, s):
    from irdu_amd import training as T
    for a in (random_picture(h, w, c), checkerboard(h, w, c)):
        got = T.bicubic_degrade_u8(a, s)
        assert got.dtype == np.uint8 and got.flags.c_contiguous and np.array_equal(got, resize_ref.degrade(a, s))
    with pytest.raises(ValueError, match="scale"):
        T.bicubic_degrade_u8(random_picture(4, 4, 1), 9)
    with pytest.raises(ValueError, match="uint8"):
        T.bicubic_degrade_u8(np.zeros((4, 4, 1), np.float32), 2)


def test_the_checkerboard_reaches_both_clamps():
    """The 0 / 255 checkerboard of the GPU tests does exercise both ends of the clamp: where the mirror doubles a
    border sample, an up pass' accumulator falls below 0 (two 0s between 255s) or rises above 255 (two 255s)."""
    row = checkerboard(1, 16, 1)[0, :, 0].astype(np.int64)
    accs = [sum(q * row[resize_ref.sym(b + o, 16)] for o, q in phase) for phase in resize_ref.taps(2, True)
            for b in range(16)]
    assert min(accs) < 0 and max(accs) > 255 << 30


@pytest.mark.parametrize("s", SCALES)
def test_the_oracle_is_within_one_level_of_pillow_away_from_the_border(s):
    """Pillow's resize(BICUBIC) is the same cubic (a = -0.5), centres and antialiasing with float-derived 22-bit
    weights, columns first and a clipped support renormalised at the border where the oracle mirrors.  Each of the
    two is within 0.5 (1 + sum |w|) of the unrounded value, so they can differ by 2 where both passes' roundings
    fall on opposite sides; on a picture that is smooth at the scale of each pass' support -- 1.5 and 2 periods
    across the picture whatever s, plus +-8 levels of noise -- they do not.  The border (4 output pixels down, 4 s
    up) is where the two edge rules differ: up to 4 levels there."""
    from PIL import Image
    h, w = 24 * s, 30 * s
    y, x = np.mgrid[0:h, 0:w]
    smooth = np.rint(128 + 60 * np.sin(2 * np.pi * 1.5 * y / h) + 50 * np.cos(2 * np.pi * 2 * x / w))
    a = np.clip(smooth + np.random.RandomState(s).randint(-8, 9, (h, w)), 0, 255).astype(np.uint8)
    low = resize_ref.down(a[:, :, None], s)[:, :, 0]
    pil_low = np.array(Image.fromarray(a).resize((w // s, h // s), Image.BICUBIC))
    diff = np.abs(low.astype(np.int64) - pil_low)
    print(f"s {s}: down max {diff[4:-4, 4:-4].max()} inside, {diff.max()} anywhere")
    assert diff[4:-4, 4:-4].max() <= 1
    back = resize_ref.up(low[:, :, None], s)[:, :, 0]
    pil_back = np.array(Image.fromarray(low).resize((w, h), Image.BICUBIC))
    diff = np.abs(back.astype(np.int64) - pil_back)
    print(f"s {s}: up max {diff[4 * s:-4 * s, 4 * s:-4 * s].max()} inside, {diff.max()} anywhere")
    assert diff[4 * s:-4 * s, 4 * s:-4 * s].max() <= 1


def test_the_host_dataset_returns_the_degraded_and_the_clean_patch_cut_alike(tmp_path):
    from irdu_amd import training as T
    shapes = ((70, 90), (33, 47), (130, 64))
    csv_path, pics = patch_ref.write_pictures(str(tmp_path), shapes)
    log = logging.getLogger("test")
    for scale in (2, 3):
        ds = T.BicubicSuperResolution(csv_path=csv_path, scale=scale, root_folder=str(tmp_path), patch_size=32,
                                      max_num_patchs=9, seed=5, logger=log)
        assert isinstance(ds, T.ImageSuperResolution) and T.DATASETS["BicubicSuperResolution"] is T.BicubicSuperResolution
        assert ds.dist_mode == "none" and ds.scale == scale and len(ds) == 9
        # the plan is the parent's
        parent = T.ImageSuperResolution(csv_path=csv_path, dist_mode="addictive_noise", lambda_noise=5.0,
                                        root_folder=str(tmp_path), patch_size=32, max_num_patchs=9, seed=5, logger=log)
        assert ds.patchs_data == parent.patchs_data
        degraded = [resize_ref.degrade(p, scale) for p in pics]
        for idx in range(len(ds)):
            row, col, pad, img = ds.patchs_data[idx]
            inp, tgt = ds[idx]
            assert inp.shape == tgt.shape == (32, 32, 3) and inp.dtype == tgt.dtype
            want_in = patch_ref.clean_patch(degraded[img], row, col, 32, 32).astype(np.float32) / 255.0
            want_tgt = patch_ref.clean_patch(pics[img], row, col, 32, 32).astype(np.float32) / 255.0
            assert np.array_equal(inp.numpy(), want_in) and np.array_equal(tgt.numpy(), want_tgt)
        assert len(ds._degraded) <= ds.CACHE
    noisy = T.BicubicSuperResolution(csv_path=csv_path, scale=2, dist_mode="addictive_noise", lambda_noise=10.0,
                                     root_folder=str(tmp_path), patch_size=32, max_num_patchs=4, seed=5, logger=log)
    plain = T.BicubicSuperResolution(csv_path=csv_path, scale=2, root_folder=str(tmp_path), patch_size=32,
                                     max_num_patchs=4, seed=5, logger=log)
    (n_in, n_tgt), (p_in, p_tgt) = noisy[0], plain[0]
    assert np.array_equal(n_tgt.numpy(), p_tgt.numpy()) and not np.array_equal(n_in.numpy(), p_in.numpy())
    for bad in (1, 9, 2.0, True):
        with pytest.raises(ValueError, match="scale"):
            T.BicubicSuperResolution(csv_path=csv_path, scale=bad, root_folder=str(tmp_path), logger=log)


def test_the_validation_config_with_a_scale_is_the_sr_protocol(tmp_path):
    from irdu_amd import training as T
    csv = tmp_path / "val.csv"
    csv.write_text("index,path\n0,a.png\n")
    base = dict(type="TestImagesCSV", dataset_args=dict(csv_path=str(csv), root_folder=str(tmp_path)))
    ds, args = T.create_val_dataset(dict(datasets=dict(val=dict(base, scale=4, tile=64, halo=16, metric="psnr_y"))))
    assert isinstance(ds, T.TestImagesCSV) and args == dict(scale=4, factor=16, tile=64, halo=16, metric="psnr_y")
    ds, args = T.create_val_dataset(dict(datasets=dict(val=dict(base, sigma=15.0))))       # without scale: unchanged
    assert args == dict(sigma=15.0, factor=16)
    with pytest.raises(ValueError, match="metric"):
        T.create_val_dataset(dict(datasets=dict(val=dict(base, scale=2, metric="ssim"))))
