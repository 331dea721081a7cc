"""tests/ssim_loss_ref.py, the numpy float64 restatement of the SSIM training loss and its closed-form gradient,
held to torch float64 autograd of the composed definition (five grouped 11 x 11 convolutions) and to
tests/ssim_ref.py's map.  CPU only: the reference alone.

Bounds: loss within 1e-12, gradient within 1e-11 max|g| -- both sides are float64 evaluations of one formula in
different orders; the values measured are <= 7.5e-14 and <= 3e-13 max|g|."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import ssim_loss_ref as R
from tests import ssim_ref

CASES = [(kind, shape) for kind, shapes in R.KINDS.items() for shape in shapes]


def composed_loss(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    c = x.shape[1]
    g = torch.from_numpy(ssim_ref.taps())
    win = (g[:, None] * g[None, :]).expand(c, 1, 11, 11).contiguous()

    def filt(t):
        return F.conv2d(t, win, groups=c)
    mx, my = filt(x), filt(y)
    vx, vy, vxy = filt(x * x) - mx * mx, filt(y * y) - my * my, filt(x * y) - mx * my
    s = ((2 * mx * my + R.C1) * (2 * vxy + R.C2)) / ((mx * mx + my * my + R.C1) * (vx + vy + R.C2))
    return 1.0 - s.mean()


@pytest.mark.parametrize("kind,shape", CASES)
def test_loss_and_gradient_equal_float64_autograd(kind, shape):
    x32, y32 = R.pair(kind, shape)
    assert x32.dtype == np.float32 and x32.shape == shape
    x = torch.from_numpy(x32).double().requires_grad_(True)
    y = torch.from_numpy(y32).double()
    ref = composed_loss(x, y)
    ref.backward()
    g_ref = x.grad.numpy()
    loss, g = R.loss_and_grad(x32, y32)
    scale = np.abs(g_ref).max()
    e_loss, e_grad = abs(loss - float(ref.detach())),np.abs(g - g_ref).max()
    print(f"{kind} {shape}: loss {loss:.12f} err {e_loss:.2e}; max|g| {scale:.3e} err {e_grad:.2e} "
          f"({e_grad / scale if scale else 0.0:.2e} of it)")
    assert e_loss <= 1e-12
    if kind == "equal":      # the analytic gradient is 0: both sides are what cancelling terms of size <= 2 / C2 leave
        n = shape[0] * shape[1] * (shape[2] - 10) * (shape[3] - 10)
        assert loss == 0.0 and np.abs(g).max() <= 1e-10 / n and scale <= 1e-10 / n
    else:
        assert e_grad <= 1e-11 * scale
    assert R.loss(x32, y32) == loss
    # a scaled incoming gradient scales the result
    assert np.array_equal(R.loss_and_grad(x32, y32, 0.5)[1], 0.5 * g)


def test_input_kinds_are_what_they_claim():
    x, y = R.pair("noisy", (2, 3, 43, 75))
    assert 0.14 < y.min() and y.max() < 0.86 and 0.3 < 1.0 - R.loss(x, y) < 0.8
    x, y = R.pair("out", (1, 3, 24, 24))
    assert x.min() < 0.0 and x.max() > 1.0 and R.ssim_map(x, y).min() < 0.0
    x, y = R.pair("flat", (1, 3, 24, 24))
    assert np.all(y == 0.5) and np.abs(x - y).max() < 1e-2
    x, y = R.pair("equal", (1, 2, 21, 32))
    assert np.array_equal(x, y) and R.loss(x, y) == 0.0 and np.all(R.ssim_map(x, y) == 1.0)
    assert np.abs(R.ssim_map(*R.pair("out", (1, 3, 24, 24)))).max() <= 1.0


def test_map_equals_the_uint8_restatement_on_integer_planes():
    """The same formulas: s of exact-integer float planes with C1, C2 scaled by 255^2 is ssim_ref.ssim_map."""
    rs = np.random.RandomState(3)
    for h, w, c in [(11, 11, 1), (23, 37, 3), (40, 12, 4)]:
        a = rs.randint(0, 256, (h, w, c)).astype(np.uint8)
        b = np.clip(a + rs.normal(0, 25, a.shape), 0, 255).astype(np.uint8)
        want = ssim_ref.ssim_map(a, b)                                        # [H - 10, W - 10, C]
        x = a.transpose(2, 0, 1)[None].astype(np.float64)
        y = b.transpose(2, 0, 1)[None].astype(np.float64)
        got = R.ssim_map(x, y, c1=ssim_ref.C1, c2=ssim_ref.C2)[0].transpose(1, 2, 0)
        assert np.abs(got - want).max() <= 1e-12
    assert R.C1 * 255.0 ** 2 == pytest.approx(ssim_ref.C1, rel=1e-15)
    assert R.C2 * 255.0 ** 2 == pytest.approx(ssim_ref.C2, rel=1e-15)


def test_gradient_against_central_differences():
    """An independent check of the closed form's sign and scale (loose: finite differences in float64)."""
    x32, y32 = R.pair("noisy", (1, 1, 12, 13))
    x, y = x32.astype(np.float64), y32.astype(np.float64)
    _, g = R.loss_and_grad(x, y)
    eps = 1e-6
    for idx in [(0, 0, 0, 0), (0, 0, 5, 6), (0, 0, 11, 12), (0, 0, 3, 9)]:
        xp, xm = x.copy(), x.copy()
        xp[idx] += eps
        xm[idx] -= eps
        fd = (R.loss(xp, y) - R.loss(xm, y)) / (2 * eps)
        assert abs(fd - g[idx]) <= 1e-6 * np.abs(g).max() + 1e-9
