"""CPU checks of tests/luma_ref.py, the numpy restatement the GPU luma tests compare against: the luma against the
textbook formula, the integer SSE against hand-made differences, and the float64 rounding of the SSIM-Y map, which
is what lets tests/test_gpu_luma.py keep the 2^-32 bound of the RGB SSIM."""
import numpy as np
import pytest

from tests import luma_ref, ssim_ref


def smooth(h, w, c):
    yy, xx = np.mgrid[0:h, 0:w]
    v = 127.5 + 90.0 * np.sin(xx / 7.0)[..., None] * np.cos(yy / 5.0)[..., None] + 10.0 * np.arange(c)
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def noisy_pair(shape, seed=5):
    """The "noisy" kind of tests/test_gpu_ssim.py: a smooth pattern against itself plus N(0, 25) noise."""
    h, w, c = shape
    rs = np.random.RandomState(seed + h * 131 + w * 7 + c)
    a = smooth(h, w, c)
    return a, np.clip(np.rint(a + rs.normal(0, 25.0, a.shape)), 0, 255).astype(np.uint8)


def test_luma_is_the_textbook_formula():
    rs = np.random.RandomState(0)
    a = rs.randint(0, 256, (64, 80, 3)).astype(np.uint8)
    x = a.astype(np.float64)
    textbook = 16.0 + (65.481 * x[:, :, 0] + 128.553 * x[:, :, 1] + 24.966 * x[:, :, 2]) / 255.0
    y = luma_ref.luma(a)
    assert y.dtype == np.float64 and y.shape == (64, 80)
    err = float(np.abs(y - textbook).max())
    print(f"luma against the float formula: {err:.3e}")
    assert err <= 1e-12
    assert 16.0 <= y.min() and y.max() <= 235.0


def test_luma_integers_at_the_ends_of_the_range():
    px = lambda r, g, b: np.array([[[r, g, b]]], dtype=np.uint8)      # noqa: E731
    assert int(luma_ref.luma_int(px(0, 0, 0))[0, 0]) == 4080000
    assert int(luma_ref.luma_int(px(255, 255, 255))[0, 0]) == 59925000
    assert luma_ref.luma(px(0, 0, 0))[0, 0] == 16.0 and luma_ref.luma(px(255, 255, 255))[0, 0] == 235.0
    assert sum(luma_ref.WEIGHTS) == 219000 and luma_ref.SCALE == 255000
    assert int(luma_ref.luma_int(px(1, 0, 0))[0, 0]) - 4080000 == 65481       # R first
    assert int(luma_ref.luma_int(px(0, 0, 1))[0, 0]) - 4080000 == 24966
    with pytest.raises(ValueError):
        luma_ref.luma(np.zeros((4, 4), dtype=np.uint8))
    with pytest.raises(ValueError):
        luma_ref.luma(np.zeros((4, 4, 4), dtype=np.uint8))
    with pytest.raises(ValueError):
        luma_ref.luma(np.zeros((4, 4, 3), dtype=np.float32))


def test_sse_of_single_channel_differences():
    rs = np.random.RandomState(1)
    a = rs.randint(0, 200, (23, 31, 3)).astype(np.uint8)
    for ch, coeff in enumerate(luma_ref.WEIGHTS):
        d = rs.randint(0, 56, a.shape[:2])
        b = a.copy()
        b[:, :, ch] = (a[:, :, ch].astype(np.int64) + d).astype(np.uint8)
        want = coeff ** 2 * int((d.astype(np.int64) ** 2).sum())
        assert luma_ref.luma_sse(a, b) == want == luma_ref.luma_sse(b, a), ch
    assert luma_ref.luma_sse(a, a) == 0 and luma_ref.psnr_y(a, a) == float("inf")
    # beyond 64 bits: 0 against 255 over 80 x 80 pixels
    z, f = np.zeros((80, 80, 3), dtype=np.uint8), np.full((80, 80, 3), 255, dtype=np.uint8)
    assert luma_ref.luma_sse(z, f) == 6400 * 55845000 ** 2 > 1 << 64
    # 0 against 255 is a luma step of 219: PSNR_Y = 20 log10(255 / 219)
    assert abs(luma_ref.psnr_y(z, f) - 20.0 * np.log10(255.0 / 219.0)) <= 1e-12


def test_ssim_y_map_in_either_filter_order():
    """Horizontal-then-vertical against vertical-then-horizontal: the two differ by float64 rounding alone, far
    below the half quantisation step 2^-33 that the device's integer sum may move the mean by."""
    worst = 0.0
    for shape in [(11, 11, 3), (11, 29, 3), (29, 11, 3), (37, 53, 3), (100, 140, 3), (300, 700, 3)]:
        a, b = noisy_pair(shape)
        hv = luma_ref.ssim_y_map(a, b)
        vh = luma_ref.ssim_y_map(a, b, vertical_first=True)
        assert hv.shape == (shape[0] - 10, shape[1] - 10)
        diff = float(np.abs(hv - vh).max())
        worst = max(worst, diff)
        assert diff < 2.0 ** -34, (shape, diff)
        assert abs(luma_ref.ssim_y(a, b) - float(np.mean(vh))) < 2.0 ** -34
        assert abs(luma_ref.quantised_sum_y(a, b) / (2.0 ** 32 * hv.size) - luma_ref.ssim_y(a, b)) <= 2.0 ** -33
    print(f"SSIM-Y map, the two filter orders: worst {worst:.3e}")


def test_ssim_y_of_simple_pictures():
    a, b = noisy_pair((37, 53, 3))
    assert luma_ref.ssim_y(a, a) == 1.0 and luma_ref.quantised_sum_y(a, a) == 27 * 43 << 32
    assert 0.2 < luma_ref.ssim_y(a, b) < 0.8
    # a grey picture's luma is 16 + 219 v / 255: SSIM-Y of R = G = B pictures is no plain SSIM of the plane
    z, f = np.zeros((20, 20, 3), dtype=np.uint8), np.full((20, 20, 3), 255, dtype=np.uint8)
    want = (2 * 16.0 * 235.0 + ssim_ref.C1) * ssim_ref.C2 / ((16.0 ** 2 + 235.0 ** 2 + ssim_ref.C1) * ssim_ref.C2)
    assert abs(luma_ref.ssim_y(z, f) - want) <= 1e-12
    assert abs(want - 0.135643201818) <= 1e-12
    flat = np.full((20, 20, 3), 200, dtype=np.uint8)
    bump = flat.copy()
    bump[10, 10, 1] = 201
    assert abs(luma_ref.ssim_y(flat, bump) - 0.99995820398) <= 1e-10
    with pytest.raises(ValueError):
        luma_ref.ssim_y(np.zeros((10, 20, 3), dtype=np.uint8), np.zeros((10, 20, 3), dtype=np.uint8))


def test_luma_against_skimage():
    color = pytest.importorskip("skimage.color")
    rs = np.random.RandomState(2)
    a = rs.randint(0, 256, (32, 48, 3)).astype(np.uint8)
    assert float(np.abs(color.rgb2ycbcr(a)[:, :, 0] - luma_ref.luma(a)).max()) <= 1e-10
