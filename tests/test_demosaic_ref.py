"""CPU checks of the Bayer mosaic and its fill: the two forms of the oracle tests/demosaic_ref.py against each other,
training.demosaic_degrade_u8 against the oracle, the properties the definition promises, values computed by hand,
the coefficient sums and the bound, the host path of training.BayerDemosaicking and the validation routing.
Launches nothing.  The shape list and the contents are shared with the GPU tests."""
import logging

import numpy as np
import pytest

from tests import demosaic_ref as ref, patch_ref

TILE = (16, 64)         # kernels.DEMOSAIC_TILE; tests/test_gpu_demosaic.py asserts it
SMALL_SHAPES = [(1, 1), (1, 2), (2, 1), (2, 2), (1, 7), (7, 1), (2, 9), (3, 5), (7, 13), (33, 31)]


def shapes(tile):
    """The small shapes, then the ones that straddle a tile of (rows, columns) both ways."""
    r, c = tile
    across = [(h, w) for h in (r - 1, r, r + 1, r + 2, r + 3) for w in (c + 1, 2 * c + 3)]
    down = [(h, w) for w in (c - 1, c, c + 1, c + 2, c + 3) for h in (r + 1, 2 * r + 3)]
    return SMALL_SHAPES + across + down


def contents(h, w):
    """Random bytes, a smooth picture, and random 0 / 255, which reaches both clamps."""
    rs = np.random.RandomState(17 + 131 * h + w)
    y, x, k = np.meshgrid(np.arange(h), np.arange(w), np.arange(3), indexing="ij")
    smooth = np.rint(128 + 60 * np.sin(0.21 * y + k) + 50 * np.cos(0.13 * x - k))
    return {"random": rs.randint(0, 256, (h, w, 3)).astype(np.uint8),
            "smooth": np.clip(smooth + rs.randint(-3, 4, (h, w, 3)), 0, 255).astype(np.uint8),
            "binary": (rs.randint(0, 2, (h, w, 3)) * 255).astype(np.uint8)}


@pytest.mark.parametrize("k,hw", list(enumerate(shapes(TILE))))
def test_the_two_oracle_forms_agree_byte_for_byte(k, hw):
    # every pattern on the small shapes; on the tile shapes one pattern each, in turn: the loops are slow
    pats = ref.PATTERNS if hw in SMALL_SHAPES else (ref.PATTERNS[k % 4],)
    for name, a in contents(*hw).items():
        if hw not in SMALL_SHAPES and name == "smooth":
            continue
        for pat in pats:
            m = ref.mosaic_loops(a, pat)
            assert np.array_equal(m, ref.mosaic(a, pat))
            for fill in ref.FILLS:
                assert np.array_equal(ref.fill_loops(m, pat, fill), ref.fill(m, pat, fill)), (hw, name, pat, fill)


@pytest.mark.parametrize("hw", shapes(TILE))
def test_the_numpy_degradation_is_the_oracle_bit_for_bit(hw):
    from irdu_amd import training as T
    for name, a in contents(*hw).items():
        for code, pat in enumerate(ref.PATTERNS):
            for fcode, fill in enumerate(ref.FILLS):
                want = ref.degrade(a, pat, fill)
                got = T.demosaic_degrade_u8(a, pat, fill)
                assert got.dtype == np.uint8 and np.array_equal(got, want), (hw, name, pat, fill)
                assert np.array_equal(T.demosaic_degrade_u8(a, code, fcode), want)          # codes for names
            m = ref.mosaic(a, pat)
            want = ref.degrade(a, pat, "malvar")
            assert np.array_equal(T.demosaic_degrade_u8(m, pat), want)                      # H x W: already the mosaic
            assert np.array_equal(T.demosaic_degrade_u8(m[:, :, None], pat), want)


@pytest.mark.parametrize("hw", SMALL_SHAPES + [(TILE[0] + 1, TILE[1] + 1)])
def test_measured_samples_pass_and_gray_is_kept(hw):
    h, w = hw
    pics = contents(h, w)
    gray = np.full((h, w, 3), 77, np.uint8)
    flat = np.broadcast_to(np.array([200, 90, 31], np.uint8), (h, w, 3)).copy()
    for pat in ref.PATTERNS:
        for fill in ref.FILLS:
            for a in pics.values():
                out, m = ref.degrade(a, pat, fill), ref.mosaic(a, pat)
                for y in range(h):
                    for x in range(w):
                        assert out[y, x, ref.site(pat, y, x)] == m[y, x] == a[y, x, ref.site(pat, y, x)]
            if fill != "zero":
                assert np.array_equal(ref.degrade(gray, pat, fill), gray)
        if min(h, w) >= 2:      # with a side of 1 the reflection does not keep the parity, so not the colour either
            assert np.array_equal(ref.degrade(flat, pat, "bilinear"), flat)
        masked = ref.degrade(flat, pat, "zero")
        assert sorted(set(masked.reshape(-1).tolist()) - {0}) == sorted({int(flat[y, x, ref.site(pat, y, x)])
                                                                          for y in range(h) for x in range(w)})


def test_binary_pictures_reach_both_clamps():
    a = contents(33, 31)["binary"]
    m = ref.mosaic(a, "rggb").astype(np.int64)
    out = ref.degrade(a, "rggb", "malvar")
    assert 0.15 < (out == 0).mean() < 0.45 and 0.15 < (out == 255).mean() < 0.45
    # and some sums do lie outside 0..255 * 16 before the clamp
    from scipy.ndimage import correlate
    s = correlate(m, ref._kernel(ref.COEFFS["malvar"]["other"]), mode="mirror")
    assert s.min() < 0 and s.max() > 255 * 16


# a 5 x 5 mosaic plane: linear but for two samples, so that the row and the column sums differ
HAND = np.array([[1, 2, 3, 4, 5],
                 [6, 7, 8, 9, 10],
                 [11, 12, 100, 30, 15],
                 [16, 17, 18, 19, 20],
                 [21, 22, 23, 24, 25]], np.uint8)


def test_values_computed_by_hand():
    """At the centre: ctr 100, h1 12 + 30 = 42, v1 8 + 18 = 26, cross 68, h2 11 + 15 = 26, v2 3 + 23 = 26, far 52,
    diag 7 + 9 + 17 + 19 = 52.
    malvar:   green 800 + 272 - 104 = 968 -> (968 + 8) >> 4 = 61;  other 1200 + 208 - 156 = 1252 -> 78;
              in row 1000 + 336 - 104 - 52 + 26 = 1206 -> 75;  in column 1000 + 208 - 104 - 52 + 26 = 1078 -> 67.
    bilinear: green 272 -> 17;  other 208 -> 13;  in row 336 -> 21;  in column 208 -> 13."""
    from irdu_amd import training as T
    want = {"malvar": dict(green=61, other=78, inrow=75, incol=67),
            "bilinear": dict(green=17, other=13, inrow=21, incol=13),
            "zero": dict(green=0, other=0, inrow=0, incol=0)}
    for fill, v in want.items():
        # the centre is the R site of rggb, a G site of an R row of grbg, of a B row of gbrg, the B site of bggr
        centre = {"rggb": (100, v["green"], v["other"]), "grbg": (v["inrow"], 100, v["incol"]),
                  "gbrg": (v["incol"], 100, v["inrow"]), "bggr": (v["other"], v["green"], 100)}
        for pat, rgb in centre.items():
            for out in (ref.fill_loops(HAND, pat, fill), ref.fill(HAND, pat, fill), T.demosaic_degrade_u8(HAND, pat, fill)):
                assert tuple(int(c) for c in out[2, 2]) == rgb, (fill, pat)
    # a corner, through the reflection: at (0, 0) of rggb the neighbours at -1 and -2 are those at 1 and 2
    # green: 8 * 1 + 4 * (2 + 2 + 6 + 6) - 2 * (3 + 3 + 11 + 11) = 8 + 64 - 56 = 16 -> 1
    # other: 12 * 1 + 4 * (7 * 4) - 3 * 28 = 12 + 112 - 84 = 40 -> (40 + 8) >> 4 = 3
    assert tuple(int(c) for c in ref.fill_loops(HAND, "rggb", "malvar")[0, 0]) == (1, 1, 3)
    assert tuple(int(c) for c in T.demosaic_degrade_u8(HAND, "rggb", "malvar")[0, 0]) == (1, 1, 3)


def test_coefficient_sums_and_the_bound():
    worst = 0
    for fill in ("bilinear", "malvar"):
        for name, k in ref.COEFFS[fill].items():
            assert sum(k.values()) == 16, (fill, name)
            worst = max(worst, 255 * sum(v for v in k.values() if v > 0), 255 * -sum(v for v in k.values() if v < 0))
    assert all(v == 0 for k in ref.COEFFS["zero"].values() for v in k.values())
    # |s| <= 2 * 20 * 255: it fits a 16-bit integer, and (s + 8) >> 4 an int32 with room to spare
    assert worst == 28 * 255 <= 2 * 20 * 255 < 2 ** 15


def test_refusals():
    from irdu_amd import training as T
    a = contents(9, 10)["random"]
    for bad in ("rgbg", "RGGB", 4, -1, True, None, 1.0):
        with pytest.raises(ValueError, match="demosaic_degrade_u8: the pattern"):
            T.demosaic_degrade_u8(a, bad)
    for bad in ("linear", 3, -1, False, None):
        with pytest.raises(ValueError, match="demosaic_degrade_u8: the fill"):
            T.demosaic_degrade_u8(a, "rggb", bad)
    for bad in (a[:, :, :2], a.astype(np.float32), np.zeros((0, 4, 3), np.uint8), np.zeros((2, 2, 3, 1), np.uint8)):
        with pytest.raises(ValueError, match="demosaic_degrade_u8: expected a uint8"):
            T.demosaic_degrade_u8(bad, "rggb")


def test_the_host_dataset_draws_one_pattern_per_file_and_cuts_both_patches_alike(tmp_path):
    from irdu_amd import training as T
    shapes_ = ((70, 90), (33, 47), (130, 64), (40, 25))
    csv_path, pics = patch_ref.write_pictures(str(tmp_path), shapes_)
    log = logging.getLogger("test")
    common = dict(csv_path=csv_path, root_folder=str(tmp_path), patch_size=32, max_num_patchs=9, seed=5, logger=log)
    names = [["rggb", "grbg", "gbrg", "bggr"], [0.1, 0.2, 0.3, 0.4]]
    for pattern, fill in (("grbg", "malvar"), (names, "bilinear")):
        ds = T.BayerDemosaicking(pattern=pattern, fill=fill, **common)
        assert isinstance(ds, T.ImageSuperResolution) and T.DATASETS["BayerDemosaicking"] is T.BayerDemosaicking
        assert ds.dist_mode == "none" and ds.fill == fill and len(ds) == 9
        if pattern == "grbg":
            assert ds.patterns == ["grbg"] * 4
        else:       # one draw per file, in file order, from RandomState(seed): fixed for the run
            want = np.random.RandomState(5).choice(4, p=names[1], size=4)
            assert ds.patterns == [names[0][int(k)] for k in want] and len(set(ds.patterns)) > 1
            again = T.BayerDemosaicking(pattern=pattern, fill=fill, **dict(common, max_num_patchs=3))
            assert again.patterns == ds.patterns
            other = T.BayerDemosaicking(pattern=pattern, fill=fill, **dict(common, seed=6))
            assert other.patterns != ds.patterns
        parent = T.ImageSuperResolution(dist_mode="addictive_noise", lambda_noise=5.0, **common)
        assert ds.patchs_data == parent.patchs_data                # the plan is the parent's
        degraded = [ref.degrade(p, q, fill) for p, q in zip(pics, ds.patterns)]
        for idx in range(len(ds)):
            row, col, pad, img = ds.patchs_data[idx]
            inp, tgt = ds[idx]
            assert inp.shape == tgt.shape == (32, 32, 3) and inp.dtype == tgt.dtype
            want_in = patch_ref.clean_patch(degraded[img], row, col, 32, 32).astype(np.float32) / 255.0
            want_tgt = patch_ref.clean_patch(pics[img], row, col, 32, 32).astype(np.float32) / 255.0
            assert np.array_equal(inp.numpy(), want_in) and np.array_equal(tgt.numpy(), want_tgt)
        assert len(ds._degraded) <= ds.CACHE
        assert ds.synthetic_key([0, 2]) == ("bayer", (ds.patterns[0], ds.patterns[2]), fill)
    assert T.BayerDemosaicking(**common).patterns == ["rggb"] * 4 and T.BayerDemosaicking(**common).fill == "malvar"
    noisy = T.BayerDemosaicking(dist_mode="addictive_noise", lambda_noise=10.0, **common)
    plain = T.BayerDemosaicking(**common)
    (n_in, n_tgt), (p_in, p_tgt) = noisy[0], plain[0]
    assert np.array_equal(n_tgt.numpy(), p_tgt.numpy()) and not np.array_equal(n_in.numpy(), p_in.numpy())
    for bad in ("rgbg", 0, True, None, [["rggb", "bggr"], [1.0]], [["rggb", "xxxx"], [0.5, 0.5]], [[], []],
                ["rggb", "bggr", "grbg"], ["rggb", [1.0]]):
        with pytest.raises(ValueError, match="pattern"):
            T.BayerDemosaicking(pattern=bad, **common)
    for bad in ("linear", 2, True, None):
        with pytest.raises(ValueError, match="fill"):
            T.BayerDemosaicking(fill=bad, **common)
    for c in (1, 4):
        with pytest.raises(ValueError, match="n_channels"):
            T.BayerDemosaicking(n_channels=c, **common)


def test_the_validation_config_with_a_bayer_key_is_demosaicking(tmp_path):
    from irdu_amd import training as T
    csv = tmp_path / "val.csv"
    csv.write_text("index,path\n0,a.png\n")
    base = dict(type="TestImagesCSV", dataset_args=dict(csv_path=str(csv), root_folder=str(tmp_path)))
    ds, args = T.create_val_dataset(dict(datasets=dict(val=dict(base, bayer="gbrg", fill="bilinear", shave=4, tile=64,
                                                                 metric="ssim"))))
    assert isinstance(ds, T.TestImagesCSV)
    assert args == dict(bayer="gbrg", fill="bilinear", shave=4, factor=16, tile=64, metric="ssim")
    ds, args = T.create_val_dataset(dict(datasets=dict(val=dict(base, bayer="rggb"))))
    assert args == dict(bayer="rggb", factor=16)
    ds, args = T.create_val_dataset(dict(datasets=dict(val=dict(base, sigma=15.0))))       # without the key: unchanged
    assert args == dict(sigma=15.0, factor=16)
    ds, args = T.create_val_dataset(dict(datasets=dict(val=dict(base, jpeg_quality=10))))
    assert args == dict(jpeg_quality=10, factor=16)
    for bad in (dict(bayer="rgbg"), dict(bayer="rggb", fill="linear"), dict(bayer="rggb", metric="psnrb")):
        with pytest.raises(ValueError, match="datasets.val"):
            T.create_val_dataset(dict(datasets=dict(val=dict(base, **bad))))
    assert T.VAL_DEMOSAIC_METRICS == ("psnr", "psnr_y", "ssim")
    with pytest.raises(ValueError, match="validate_demosaic: metric"):
        T.validate_demosaic(None, [], "rggb", metric="psnrb")


def test_the_example_yaml_names_registered_types():
    import os
    from irdu_amd import training as T
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    conf = T.parse(os.path.join(root, "experiment_conf", "demosaic_rggb_example.yaml"))
    stages = T.train_stage_confs(conf)
    assert len(stages) == 2 and all(st["type"] == "BayerDemosaicking" and st["device_resident"] for st in stages)
    assert all(st["type"] in T.DATASETS and st["dataset_args"]["pattern"] == "rggb" for st in stages)
    assert len({st["dataset_args"]["csv_path"] for st in stages}) == 1          # one csv: the stages share the arenas
    val = conf["datasets"]["val"]
    assert val["type"] == "TestImagesCSV" and val["bayer"] == "rggb" and conf["train"]["val_every"] > 0
