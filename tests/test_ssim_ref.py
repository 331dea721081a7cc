"""The numpy restatement of the Gaussian-window SSIM (tests/ssim_ref.py) against scipy's filter, the closed form
for constant images and the exact 1.0 of equal images (CPU only)."""
import numpy as np
import pytest

from tests import ssim_ref

SHAPES = [(11, 11, 1), (11, 29, 3), (29, 11, 2), (37, 53, 3), (64, 70, 4)]


def _pair(shape, seed):
    rs = np.random.RandomState(seed)
    h, w, c = shape
    yy, xx = np.mgrid[0:h, 0:w]
    smooth = 127.5 + 90.0 * np.sin(xx / 7.0)[..., None] * np.cos(yy / 5.0)[..., None] + 10.0 * np.arange(c)
    a = np.clip(np.rint(smooth), 0, 255).astype(np.uint8)
    b = np.clip(np.rint(a + rs.normal(0, 25.0, a.shape)), 0, 255).astype(np.uint8)
    return a, b


@pytest.mark.parametrize("shape", SHAPES)
def test_restatement_matches_scipy_gaussian_filter(shape):
    """skimage's route: gaussian_filter(sigma 1.5, truncate 3.5, reflect) over each moment, then the 5-pixel crop."""
    ndimage = pytest.importorskip("scipy.ndimage")
    a, b = _pair(shape, 7)
    x, y = a.astype(np.float64), b.astype(np.float64)

    def filt(v):
        out = np.stack([ndimage.gaussian_filter(v[..., ch], 1.5, truncate=3.5, mode="reflect")
                        for ch in range(v.shape[2])], axis=2)
        return out[5:-5, 5:-5]

    mx, my, exx, eyy, exy = filt(x), filt(y), filt(x * x), filt(y * y), filt(x * y)
    vx, vy, vxy = exx - mx * mx, eyy - my * my, exy - mx * my
    want = ((2 * mx * my + ssim_ref.C1) * (2 * vxy + ssim_ref.C2)) / \
        ((mx ** 2 + my ** 2 + ssim_ref.C1) * (vx + vy + ssim_ref.C2))
    mean, got = ssim_ref.ssim_with_map(a, b)
    assert got.shape == (shape[0] - 10, shape[1] - 10, shape[2]) == want.shape
    # the mean: 1e-13.  A single value: E[x^2] - mx^2 cancels at up to 65025; two orders of the 22 window
    # operations differ there by about 8 roundings, 65025 x 8 x 2^-53 = 6e-11, against a factor of at least
    # C2 = 58.5 and a value of at most 1: 1e-12, doubled for the second such factor.
    print(f"{shape}: map {np.abs(got - want).max():.3e} mean {abs(mean - float(want.mean())):.3e}")
    assert np.abs(got - want).max() <= 2e-12
    assert abs(mean - float(want.mean())) <= 1e-13


def test_taps_are_the_normalised_gaussian():
    g = ssim_ref.taps()
    assert g.shape == (11,) and g.dtype == np.float64
    assert abs(g.sum() - 1.0) <= 2e-16 and np.array_equal(g, g[::-1])
    assert abs(g[5] - 0.26601172) <= 1e-8 and abs(g[0] - 0.00102838) <= 1e-8


@pytest.mark.parametrize("p,q", [(0, 255), (255, 0), (200, 201), (17, 230), (128, 128)])
def test_constant_images_have_the_closed_form(p, q):
    """a = p, b = q everywhere: the variances vanish and s = (2 p q + C1) / (p^2 + q^2 + C1)."""
    a = np.full((20, 23, 3), p, dtype=np.uint8)
    b = np.full((20, 23, 3), q, dtype=np.uint8)
    want = (2.0 * p * q + ssim_ref.C1) / (p * p + q * q + ssim_ref.C1)
    mean, m = ssim_ref.ssim_with_map(a, b)
    assert np.abs(m - want).max() <= 1e-12
    assert abs(mean - want) <= 1e-12
    if (p, q) == (0, 255):
        assert abs(mean - 9.999000099991e-05) <= 1e-16


@pytest.mark.parametrize("shape", SHAPES)
def test_equal_images_give_exactly_one_everywhere(shape):
    a, _ = _pair(shape, 3)
    mean, m = ssim_ref.ssim_with_map(a, a.copy())
    assert np.all(m == 1.0) and mean == 1.0
    assert ssim_ref.quantised_sum(a, a) == m.size << 32


def test_sides_below_the_window_raise():
    for shape in [(10, 11, 1), (11, 10, 3)]:
        z = np.zeros(shape, dtype=np.uint8)
        with pytest.raises(ValueError):
            ssim_ref.ssim_map(z, z)
    with pytest.raises(ValueError):
        ssim_ref.ssim_map(np.zeros((12, 12, 1), dtype=np.float32), np.zeros((12, 12, 1), dtype=np.float32))


def test_quantised_sum_is_within_half_a_step_per_value_of_the_mean():
    for shape in SHAPES:
        a, b = _pair(shape, 11)
        mean, m = ssim_ref.ssim_with_map(a, b)
        assert abs(ssim_ref.quantised_sum(a, b) / (m.size * 2.0 ** 32) - mean) <= 2.0 ** -33 + 1e-12
