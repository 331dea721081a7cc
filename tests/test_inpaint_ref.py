"""The oracle of inpainting (tests/inpaint_ref.py) against itself, against tests/patch_ref.py and against the host path
of training.RandomMaskInpainting.  No GPU."""
import numpy as np
import pytest

from irdu_amd import kernels as K
from irdu_amd import training as T
from tests import inpaint_ref as ref, patch_ref

SEED = 99
FLAT3 = np.full((3, 3), 255, np.uint8)
RS = np.random.RandomState(3)
ASYM = RS.randint(0, 256, (5, 9)).astype(np.uint8)


def test_every_pixel_known_gives_the_clean_patch():
    img = patch_ref.picture(1, 20, 30)
    for (row, col, mode), (ph, pw) in (((3, 4, 0), (8, 12)), ((15, 25, 5), (8, 12)), ((0, 0, 3), (16, 16)), ((19, 29, 6), (16, 16))):
        for fill in ("zero", "conv"):
            t, i, m = ref.mask_fill_patch([img], [(0, row, col, mode)], [5], [ref.ONE], SEED, ph, pw, ASYM, fill, 9)
            want = patch_ref.transform(patch_ref.clean_patch(img, row, col, ph, pw), mode).astype(np.float32) / np.float32(255)
            assert np.array_equal(t[0], want.transpose(2, 0, 1)) and np.array_equal(i, t) and (m == 1).all()


def test_a_constant_picture_stays_constant_under_conv_where_den_is_positive():
    img = np.full((12, 17, 3), 0, np.uint8)
    img[:, :, 0], img[:, :, 1], img[:, :, 2] = 7, 200, 255
    for keep in (ref.ONE // 2, ref.ONE // 5, ref.ONE // 50):
        known = ref.mask_bits(SEED, 4, 12, 17, keep)
        out, code = ref.fill_window(ref.window(img, 0, 0, 12, 17), known, ASYM, "conv", 99)
        assert (code == 2).any()
        assert np.array_equal(out[code > 0], img[code > 0])                     # (2 c den + den) // (2 den) == c
        assert (out[code == 0] == 99).all()


def test_the_mask_is_a_function_of_seed_id_and_sides_alone():
    a = ref.mask_bits(SEED, 4, 9, 13, ref.ONE // 2)
    assert a.shape == (23, 27) and 0.35 < a.mean() < 0.65
    assert np.array_equal(a, ref.mask_bits(SEED, 4, 9, 13, ref.ONE // 2))
    assert not np.array_equal(a, ref.mask_bits(SEED + 1, 4, 9, 13, ref.ONE // 2))
    assert not np.array_equal(a, ref.mask_bits(SEED, 5, 9, 13, ref.ONE // 2))
    assert not np.array_equal(a, ref.mask_bits(SEED, 4 + (1 << 32), 9, 13, ref.ONE // 2))
    # a smaller share knows a subset: the bit is a threshold on one word
    assert not (ref.mask_bits(SEED, 4, 9, 13, ref.ONE // 5) & ~a).any()
    assert ref.mask_bits(SEED, 4, 9, 13, ref.ONE + 7).all() and not ref.mask_bits(SEED, 4, 9, 13, -3).any()
    # the mask of the patch does not change with the table's sides or the fill
    img = patch_ref.picture(2, 20, 30)
    masks = [ref.mask_fill_patch([img], [(0, 2, 3, 0)], [4], [ref.ONE // 2], SEED, 9, 13, w, fill, 0)[2]
             for w, fill in ((FLAT3, "conv"), (ASYM, "conv"), (np.full((15, 15), 1, np.uint8), "conv"), (FLAT3, "zero"))]
    assert all(np.array_equal(m, masks[0]) for m in masks) and np.array_equal(masks[0][0, 0], a[7:16, 7:20].astype(np.float32))
    # the second counter word is 1: the stream is not the noise's
    x0 = patch_ref.philox4x32_10(np.array([[0, 0, 4, 0]], np.uint64), np.array([SEED, 0], np.uint64))
    x1 = patch_ref.philox4x32_10(np.array([[0, 1, 4, 0]], np.uint64), np.array([SEED, 0], np.uint64))
    assert np.array_equal((x1[0] >> 8) < ref.ONE // 2, a.reshape(-1)[:4]) and not np.array_equal(x0, x1)


def test_nothing_known_gives_the_hole_and_a_1x1_table_never_fills():
    img = patch_ref.picture(3, 10, 14)
    t, i, m = ref.mask_fill_patch([img], [(0, 1, 2, 0)], [1], [0], SEED, 8, 8, ASYM, "conv", 200)
    assert (m == 0).all() and np.array_equal(i, np.full_like(i, np.float32(200) / np.float32(255)))
    t, i, m = ref.mask_fill_patch([img], [(0, 1, 2, 0)], [1], [0], SEED, 8, 8, ASYM, "zero", 200)
    assert (i == 0).all()
    one = np.full((1, 1), 255, np.uint8)
    t, i, m = ref.mask_fill_patch([img], [(0, 1, 2, 0)], [1], [ref.ONE // 2], SEED, 8, 8, one, "conv", 77)
    missing = np.broadcast_to(m == 0, i.shape)
    assert missing.any() and np.array_equal(i[missing], np.full(missing.sum(), np.float32(77) / np.float32(255)))
    assert np.array_equal(i[~missing], t[~missing])


def test_the_rounding_is_to_nearest_with_halves_up():
    """Two known neighbours 0 and 1 under a flat row: (2 * 255 + 510) // 1020 = 1; 0 and 2 with weights 3 : 1 give
    (2 * 2 + 4) // 8 = 1 from 0.5."""
    win = np.zeros((15, 17, 1), np.uint8)
    known = np.zeros((15, 17), bool)
    known[7, 7], known[7, 9] = True, True
    win[7, 9, 0] = 1
    out, code = ref.fill_window(win, known, np.full((1, 3), 255, np.uint8), "conv", 0)
    assert out[0, 1, 0] == 1 and code[0, 1] == 2
    win[7, 9, 0] = 2
    out, _ = ref.fill_window(win, known, np.array([[3, 0, 1]], np.uint8), "conv", 0)
    assert out[0, 1, 0] == 1


def test_a_given_mask_is_carried_through_and_passes_grow_by_a_radius():
    img = patch_ref.picture(4, 12, 40)
    mask = np.ones((12, 40), np.uint8)
    mask[:, 10:30] = 0
    mask[mask > 0] = 201
    cur_img, cur_mask, left = img, mask, []
    for _ in range(4):
        cur_img, cur_mask = ref.mask_fill_image(cur_img, cur_mask, 0, SEED, 0, np.full((7, 7), 255, np.uint8), "conv", 128)
        left.append(int((cur_mask == 0).sum()))
        assert (cur_mask[mask > 0] == 201).all() and np.array_equal(cur_img[mask > 0], img[mask > 0])
    assert left == [12 * 14, 12 * 8, 12 * 2, 0] and set(np.unique(cur_mask)) == {2, 201}


@pytest.mark.parametrize("aug,fill,keep", [(True, "conv", 0.4), (False, "zero", [[0.2, 0.9], [0.5, 0.5]]), (True, "conv", 1.0)])
def test_the_host_path_is_the_oracle_with_its_own_bits(tmp_path, aug, fill, keep):
    shapes = ((40, 56), (20, 17), (33, 47))
    csv_path, pics = patch_ref.write_pictures(str(tmp_path), shapes)
    ds = T.RandomMaskInpainting(csv_path, keep=keep, fill=fill, fill_side=5, fill_sigma=1.2, hole=31, use_data_aug=aug,
                                patch_size=(32, 32), max_num_patchs=6, root_folder=str(tmp_path), seed=11)
    assert np.array_equal(ds.weights, K.mask_weights(5, 1.2)) and ds.weights.dtype == np.uint8 and ds.weights[2, 2] == 255
    for idx in range(len(ds)):
        rs = np.random.RandomState()
        rs.set_state(ds.random_state.get_state())
        inp, tgt = ds[idx]
        mode = rs.randint(0, 7) if aug else 0
        level = float(T._draw_levels(rs, keep, 1)[0])
        bits = rs.random_sample((32 + 14, 32 + 14)) < level
        row, col, _, img = ds.patchs_data[idx]
        t, i, m = ref.mask_fill_patch(pics, [(img, row, col, mode)], [0], [0], 0, 32, 32, ds.weights, fill, 31, bits=[bits])
        assert inp.dtype == tgt.dtype and tuple(inp.shape) == (32, 32, 3)
        assert np.array_equal(tgt.numpy().transpose(2, 0, 1), t[0]) and np.array_equal(inp.numpy().transpose(2, 0, 1), i[0])
        if keep == 1.0:
            assert np.array_equal(inp.numpy(), tgt.numpy())


def test_the_dataset_refuses_what_it_cannot_make(tmp_path):
    csv_path, _ = patch_ref.write_pictures(str(tmp_path), ((40, 56),))
    make = lambda **kw: T.RandomMaskInpainting(csv_path, root_folder=str(tmp_path), max_num_patchs=2, **kw)   # noqa: E731
    for bad, message in ((dict(keep=1.5), "RandomMaskInpainting: keep is a number of 0..1"),
                         (dict(keep=[[0.5, 2.0], [0.5, 0.5]]), "RandomMaskInpainting: keep is a number of 0..1"),
                         (dict(fill="bilinear"), r"RandomMaskInpainting: fill is one of \('zero', 'conv'\)"),
                         (dict(fill_side=6), "RandomMaskInpainting: .*sides are odd and lie in 1..15"),
                         (dict(fill_side=17), "RandomMaskInpainting: .*sides are odd and lie in 1..15"),
                         (dict(fill_sigma=0), "RandomMaskInpainting: .*sigma is a positive number or None"),
                         (dict(hole=256), "RandomMaskInpainting: .*the hole is an integer of 0..255"),
                         (dict(dist_mode="addictive_noise", lambda_noise=25.0), "RandomMaskInpainting: dist_mode must be 'none'")):
        with pytest.raises(ValueError, match=message):
            make(**bad)
    assert T.DATASETS["RandomMaskInpainting"] is T.RandomMaskInpainting
    with pytest.raises(ValueError, match="RandomMaskInpainting"):
        T.create_dataset(dict(type="Nope", dataset_args={}), {})


def test_weights_and_units():
    assert K.keep_units(0) == 0 and K.keep_units(1) == 1 << 24 and K.keep_units(0.5) == 1 << 23 and K.keep_units(0.2) == 3355443
    for bad in (-0.1, 1.01, float("nan"), "0.5", True, None):
        with pytest.raises(ValueError, match="keep_units: the known share is a number of 0..1"):
            K.keep_units(bad)
    flat = K.mask_weights(7)
    assert flat.shape == (7, 7) and flat.dtype == np.uint8 and (flat == 255).all()
    g = K.mask_weights((3, 5), 1.0)
    assert g.shape == (3, 5) and g[1, 2] == 255 and g[1, 1] == round(255 * np.exp(-0.5)) and g[0, 0] == round(255 * np.exp(-2.5))
    assert np.array_equal(g, g[::-1, ::-1])
    for bad in (0, 2, 17, (3, 4), 3.0, True):
        with pytest.raises(ValueError, match="mask_weights: a weight table's sides"):
            K.mask_weights(bad)
    for bad in (0, -1.0, float("inf"), "1", True):
        with pytest.raises(ValueError, match="mask_weights: sigma"):
            K.mask_weights(3, bad)
