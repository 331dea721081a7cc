"""The oracle of joint denoising and demosaicking (tests/raw_noise_ref.py) against itself, against the demosaic oracle,
against the noise model and against training.raw_noise_demosaic_patch, without a GPU; and the tie margin of every
fixture tests/test_gpu_raw_noise.py compares bit for bit."""
import numpy as np
import pytest

from tests import demosaic_ref as dr, patch_ref, raw_noise_ref as ref

SEED = ref.SEED


def equal(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


@pytest.mark.parametrize("fill", dr.FILLS)
@pytest.mark.parametrize("pattern", dr.PATTERNS)
def test_the_loop_form_is_the_vectorised_form(pattern, fill):
    """On every picture of the GPU fixtures, a side of 1 and the periodic reflection included, under turns, depths, both
    clips and all four noise pairs; a 5 x 7 patch under an odd mode is read as mode & 5 by both."""
    b = ref.read_b(ref.READ)
    for k, img in enumerate(ref.pictures()):
        h, w = img.shape[:2]
        for j, (a_, b_) in enumerate(((0.0, 0.0), (0.0, b), (ref.SHOT, 0.0), (ref.SHOT, b))):
            args = (img, pattern, (3 * k + j) % h, (5 * k + j) % w, (k + 2 * j) % 8, 6, 6, a_, b_, SEED, 100 * k + j, fill,
                    (8, 12, 16, 10)[j], bool((k + j) % 2))
            assert equal(ref.sample_loops(*args), ref.sample(*args)), (k, j)
        args = (img, pattern, 0, 0, 3, 5, 7, ref.SHOT, b, SEED, k, fill)
        odd, legal = ref.sample(*args), ref.sample(*(args[:4] + (1,) + args[5:]))
        assert equal(ref.sample_loops(*args), odd) and equal(odd, legal) and odd[0].shape == (3, 5, 7)


def demosaic_sums(img, pattern, fill):
    """demosaic_ref's sums in sixteenths, before its rounding to bytes."""
    from scipy.ndimage import correlate
    m = dr.mosaic(img, pattern).astype(np.int64)
    red, blue, g_red_row, g_blue_row = dr._masks(pattern, *m.shape)
    c = {name: correlate(m, dr._kernel(k), mode="mirror") for name, k in dr.COEFFS[fill].items()}
    s = np.zeros(m.shape + (3,), np.int64)
    s[:, :, 1] = np.where(red | blue, c["green"], 16 * m)
    s[:, :, 0] = np.where(red, 16 * m, np.where(blue, c["other"], np.where(g_red_row, c["inrow"], c["incol"])))
    s[:, :, 2] = np.where(blue, 16 * m, np.where(red, c["other"], np.where(g_blue_row, c["inrow"], c["incol"])))
    return s


@pytest.mark.parametrize("fill", dr.FILLS)
@pytest.mark.parametrize("pattern", dr.PATTERNS)
def test_without_noise_at_8_bits_it_is_the_demosaic_oracle(pattern, fill):
    for img in (patch_ref.picture(2, 40, 56), patch_ref.picture(3, 5, 3), patch_ref.picture(4, 1, 7)):
        h, w = img.shape[:2]
        target, inp, s, margin = ref.sample(img, pattern, 0, 0, 0, h, w, 0.0, 0.0, SEED, 0, fill, bits=8)
        assert np.array_equal(s, demosaic_sums(img, pattern, fill))
        assert np.array_equal(np.clip((s + 8) >> 4, 0, 255).astype(np.uint8), dr.degrade(img, pattern, fill))
        assert np.array_equal(target, (img.astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1))
        assert np.array_equal(inp, (s / (16.0 * 255.0)).astype(np.float32).transpose(2, 0, 1)) and margin > 0.49


@pytest.mark.parametrize("a,b", [(0.0, ref.read_b(25.0)), (0.02, 0.0), (ref.SHOT, ref.read_b(ref.READ))])
def test_the_noise_has_the_mean_and_the_variance_of_the_model(a, b):
    """On a gray picture x = 128 / 255 with the zero fill, q is the sum of a pixel's sixteenths / 16.  n = 102400
    samples at 16 bits, unclipped: the mean of q / full - x lies within 5 sqrt(var / n) of 0 and the sample variance
    within 5 var sqrt(2 / n) of var = a x + b (the quantiser adds 1 / (12 full^2) = 2e-11)."""
    side, full = 320, 65535
    img = np.full((side, side, 3), 128, np.uint8)
    _, _, s, _ = ref.sample(img, "grbg", 0, 0, 0, side, side, a, b, SEED, 7, "zero", 16, False)
    x = 128 / 255.0
    d = s.sum(axis=2) / 16.0 / full - x
    n, var = d.size, ref.f32(a) * x + ref.f32(b)
    assert n >= 10 ** 5
    print(f"mean {d.mean():.3e} (5 se {5 * np.sqrt(var / n):.3e}), variance {d.var():.6e} of {var:.6e} "
          f"(5 se {5 * var * np.sqrt(2 / n):.3e})")
    assert abs(d.mean()) <= 5 * np.sqrt(var / n)
    assert abs(d.var() - var) <= 5 * var * np.sqrt(2.0 / n)


def test_the_training_function_is_the_oracle_on_the_oracle_normals():
    from irdu_amd import training as T
    b = ref.read_b(ref.READ)
    for k, img in enumerate(ref.pictures()):
        h, w = img.shape[:2]
        for j, pattern in enumerate(dr.PATTERNS):
            for fill in dr.FILLS:
                ph, pw = ((16, 16), (6, 10), (20, 70), (5, 7))[j]
                row, col, sid = (7 * k + j) % h, (3 * k + j) % w, 10 * k + j
                a_, b_ = ((ref.SHOT, b), (0.0, b), (ref.SHOT, 0.0), (0.0, 0.0))[(k + j) % 4]
                bits, clip = (16, 12, 8, 10)[(j + k) % 4], bool(j % 2)
                want = ref.sample(img, pattern, row, col, 0, ph, pw, a_, b_, SEED, sid, fill, bits, clip)
                z = ref.window_normals(SEED, sid, ph, pw)
                target, inp = T.raw_noise_demosaic_patch(img, pattern, row, col, ph, pw, a_, b_, z, fill, bits, clip)
                assert target.dtype == inp.dtype == np.float32
                assert np.array_equal(target.transpose(2, 0, 1), want[0]) and np.array_equal(inp.transpose(2, 0, 1), want[1])
    img = ref.pictures()[3]
    quiet = T.raw_noise_demosaic_patch(img, "rggb", 3, 4, 16, 16, 0.0, 0.0, None, "malvar", 8)
    assert np.array_equal(quiet[1].transpose(2, 0, 1), ref.sample(img, "rggb", 3, 4, 0, 16, 16, 0, 0, SEED, 0, bits=8)[1])


@pytest.mark.parametrize("case", ref.GPU_CASES, ids=[f"{c[0]}x{c[1]}-{c[2]}-{c[3]}-{int(c[4])}" for c in ref.GPU_CASES])
def test_every_gpu_fixture_keeps_away_from_the_rounding_ties(case):
    """A condition on the inputs, not a tolerance on the device: float64 evaluation of t full below 2^20 differs between
    correct implementations by about 1e-9, so a margin of 1e-6 leaves one answer."""
    k = ref.gpu_case(case)
    print(f"{case}: tie margin {k['margin']:.3e}")
    assert k["margin"] >= ref.TIE_MARGIN
    rows, noise = k["rows"], k["noise"]
    assert {(r[1] % 2, r[2] % 2) for r in rows if r[0] >= 3} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {r[0] for r in rows} == set(range(5)) and set(k["patterns"]) == set(dr.PATTERNS)
    assert {r[3] for r in rows} == (set(range(8)) if case[0] == case[1] else {0, 1, 4, 5})
    assert {(a > 0, b > 0) for a, b in noise} == {(False, False), (False, True), (True, False), (True, True)}


def test_the_fixtures_of_the_other_gpu_tests_keep_away_from_the_ties_too():
    """test_gpu_raw_noise's whole-picture form, test_gpu_jdd_eval's pictures and test_gpu_raw_noise_loader's epoch."""
    b = ref.read_b(ref.READ)
    for i, img in enumerate(ref.pictures()[3:]):
        h, w = img.shape[:2]
        for pattern, fill, bits, clip in ref.WHOLE_CASES:
            assert ref.sample(img, pattern, 0, 0, 0, h, w, ref.SHOT, b, SEED, i, fill, bits, clip)[3] >= ref.TIE_MARGIN


def test_the_loader_fixture_keeps_away_from_the_ties_and_draws_after_the_existing_draws(tmp_path):
    import logging
    from irdu_amd import training as T
    csv_path, pics = patch_ref.write_pictures(str(tmp_path))
    ds = T.NoisyBayerDemosaicking(csv_path=csv_path, root_folder=str(tmp_path), logger=logging.getLogger("test"),
                                  **ref.LOADER_CONF)
    loader = T.DevicePatchLoader(ds, T.ResumeableSampler(ds, 4, 0, 1), 4)
    plain = T.ImageSuperResolution(csv_path=csv_path, root_folder=str(tmp_path), logger=logging.getLogger("test"),
                                   dist_mode="addictive_noise_scale", lambda_noise=25.0, use_data_aug=True,
                                   patch_size=(16, 16), max_num_patchs=40, seed=2204)
    assert np.array_equal(ds.plan, plain.plan)                         # the parent's plan
    assert len(set(ds.patterns)) > 1 and ds.patterns == T.BayerDemosaicking(
        csv_path=csv_path, root_folder=str(tmp_path), logger=logging.getLogger("test"), pattern=ref.LOADER_CONF["pattern"],
        patch_size=(16, 16), max_num_patchs=40, seed=2204).patterns   # the sibling's per-file draw
    for epoch in (1, 2):
        ds.random_permute(2024 + epoch)
        modes, sigma = loader.epoch_draws(epoch)
        noise = loader.epoch_noise(epoch)
        rs = np.random.RandomState((ds.seed * 1000003 + epoch) % 2 ** 32)
        assert np.array_equal(modes, rs.randint(0, 8, len(ds))) and not sigma.any()
        shot = rs.choice(ref.LOADER_CONF["shot"][0], p=ref.LOADER_CONF["shot"][1], size=len(ds))
        read = rs.choice(ref.LOADER_CONF["read"][0], p=ref.LOADER_CONF["read"][1], size=len(ds))
        assert noise.dtype == np.float32 and noise.shape == (len(ds), 2)
        assert np.array_equal(noise[:, 0], shot.astype(np.float32))
        assert np.array_equal(noise[:, 1], ((read / 255.0) ** 2).astype(np.float32))
        assert ref.loader_reference(ds, loader, epoch, pics)[2] >= ref.TIE_MARGIN
    # the host path: the same formula, its own normals; shapes, dtypes and the clean target
    inp, tgt = ds[0]
    assert tuple(inp.shape) == tuple(tgt.shape) == (16, 16, 3) and inp.dtype == tgt.dtype
    with pytest.raises(ValueError, match="dist_mode must be 'none'"):
        T.NoisyBayerDemosaicking(csv_path=csv_path, root_folder=str(tmp_path), dist_mode="addictive_noise", lambda_noise=5.0)
    assert not issubclass(T.NoisyBayerDemosaicking, T._DegradedFromClean) and "NoisyBayerDemosaicking" in T.DATASETS
