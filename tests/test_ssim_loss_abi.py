"""CPU-only checks of the SSIM training loss's entry points (csrc/ssim_loss_ops.hip: grr_ssim_loss_supported,
grr_ssim_loss_forward, grr_ssim_loss_backward), their wrappers and losses.ssim_loss: the header's signatures,
argument validation and the Python mirror of the shape query.  Loads the library, launches nothing."""
import os
import re

import pytest
import torch

import irdu_amd
from irdu_amd import _native, losses
from irdu_amd import kernels as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, UNSUPPORTED = 1, 3
PTR = 0x1000        # never dereferenced: validation fails first


@pytest.fixture(scope="module")
def lib():
    return _native.load()


def fwd_args(x=PTR, y=PTR, b=2, c=3, h=16, w=16, qsum=PTR, coef=PTR):
    return (x, y, b, c, h, w, qsum, coef, None)


def bwd_args(x=PTR, y=PTR, coef=PTR, gout=PTR, gx=PTR, b=2, c=3, h=16, w=16):
    return (x, y, coef, gout, gx, b, c, h, w, None)


def test_symbols_exist_with_the_headers_signatures(lib):
    src = open(os.path.join(ROOT, "include", "grr.h")).read()
    flat = re.sub(r"\s+", " ", src)
    assert "int grr_ssim_loss_supported(int B, int C, int H, int W);" in flat
    assert ("grr_status grr_ssim_loss_forward(const float* x, const float* y, int B, int C, int H, int W, int64_t* qsum, "
            "double* coef, void* stream);") in flat
    assert ("grr_status grr_ssim_loss_backward(const float* x, const float* y, const double* coef, const float* gout, "
            "float* gx, int B, int C, int H, int W, void* stream);") in flat
    P, I = _native.P, _native.I
    assert _native.SIGNATURES["grr_ssim_loss_supported"] == [I, I, I, I]
    assert _native.SIGNATURES["grr_ssim_loss_forward"] == [P, P, I, I, I, I, P, P, P]
    assert _native.SIGNATURES["grr_ssim_loss_backward"] == [P, P, P, P, P, I, I, I, I, P]
    for name in ("grr_ssim_loss_supported", "grr_ssim_loss_forward", "grr_ssim_loss_backward"):
        assert getattr(lib, name) is not None


def test_python_mirror_of_the_query(lib):
    """kernels.ssim_loss_ok is what the wrappers enforce; grr_ssim_loss_supported is what the entry points do."""
    planes = K.MAX_SSIM_LOSS_PLANES
    table = [(1, 1, 10, 11), (1, 1, 11, 10), (1, 1, 11, 11), (1, 1, 10, 10), (2, 3, 16, 16), (0, 3, 16, 16),
             (2, 0, 16, 16), (-1, 3, 16, 16), (1, 1, 11, 0), (1, 1, -11, -11),
             (planes, 1, 11, 11), (planes + 1, 1, 11, 11), (1, planes, 11, 11), (1, planes + 1, 11, 11),
             (255, 257, 11, 11), (256, 256, 11, 11),                      # B C = 65535, 65536
             (1, 1, 46340, 46340), (1, 1, 46341, 46341),                  # H W just below and above 2^31
             (32, 3, 4729, 4729), (32, 3, 4730, 4730),                    # 96 H W just below and above 2^31
             (1, 1, 1 << 15, 1 << 16), (1, 2, 1 << 15, (1 << 15) - 1), (2, 1, 1 << 15, 1 << 15),   # 2^31, 2^31 - 2^16, 2^31
             (1, 1, 11, (1 << 31) // 11), (1, 1, 11, (1 << 31) // 11 + 1), (32, 3, 512, 512)]
    seen = set()
    for b, c, h, w in table:
        got = bool(lib.grr_ssim_loss_supported(b, c, h, w))
        assert K.ssim_loss_ok(b, c, h, w) == got, (b, c, h, w)
        seen.add(got)
    assert seen == {True, False}
    assert K.ssim_loss_ok(1, 1, 11, 11) and not K.ssim_loss_ok(1, 1, 10, 11) and not K.ssim_loss_ok(1, 1, 11, 10)
    assert K.ssim_loss_ok(255, 257, 11, 11) and not K.ssim_loss_ok(256, 256, 11, 11)
    assert not K.ssim_loss_ok(1, 1, 1 << 15, 1 << 16) and K.ssim_loss_ok(1, 2, 1 << 15, (1 << 15) - 1)
    assert K.ssim_loss_count(2, 3, 11, 11) == 6 and K.ssim_loss_count(1, 1, 20, 31) == 10 * 21
    rows, cols = K.SSIM_LOSS_TILE
    assert (rows, cols) == K.SSIM_TILE and cols % 64 == 0


def test_bad_pointers_and_sizes_are_invalid_args(lib):
    for name in ("x", "y", "qsum"):
        assert lib.grr_ssim_loss_forward(*fwd_args(**{name: None})) == INVALID_ARG, name
        assert b"grr_ssim_loss_forward: bad args" in lib.grr_last_error()
    for name in ("x", "y", "coef", "gout", "gx"):
        assert lib.grr_ssim_loss_backward(*bwd_args(**{name: None})) == INVALID_ARG, name
        assert b"grr_ssim_loss_backward: bad args" in lib.grr_last_error()
    # 4-byte alignment for the float32 operands, 8-byte for the int64 and float64 buffers
    for bad in (dict(x=PTR + 2), dict(y=PTR + 1), dict(qsum=PTR + 4), dict(coef=PTR + 4)):
        assert lib.grr_ssim_loss_forward(*fwd_args(**bad)) == INVALID_ARG, bad
    for bad in (dict(x=PTR + 2), dict(y=PTR + 3), dict(coef=PTR + 4), dict(gout=PTR + 2), dict(gx=PTR + 1)):
        assert lib.grr_ssim_loss_backward(*bwd_args(**bad)) == INVALID_ARG, bad
    for bad in (dict(b=0), dict(c=0), dict(h=0), dict(w=-3), dict(b=-1)):
        assert lib.grr_ssim_loss_forward(*fwd_args(**bad)) == INVALID_ARG, bad
        assert lib.grr_ssim_loss_backward(*bwd_args(**bad)) == INVALID_ARG, bad


def test_unsupported_shapes(lib):
    # float32 operands one float past a 16-byte boundary are taken: these fail on the shape alone
    for bad in (dict(h=10), dict(w=10), dict(b=256, c=256), dict(b=32, c=3, h=4730, w=4730)):
        assert lib.grr_ssim_loss_forward(*fwd_args(x=PTR + 4, y=PTR + 12, **bad)) == UNSUPPORTED, bad
        assert b"grr_ssim_loss_forward: needs H and W >= 11" in lib.grr_last_error()
        assert lib.grr_ssim_loss_backward(*bwd_args(x=PTR + 4, gx=PTR + 4, coef=PTR + 8, **bad)) == UNSUPPORTED, bad
        assert b"grr_ssim_loss_backward: needs H and W >= 11" in lib.grr_last_error()
    # no coefficient planes is a valid request, not a bad argument: the shape decides
    assert lib.grr_ssim_loss_forward(*fwd_args(coef=None, h=10)) == UNSUPPORTED


def test_wrappers_refuse_bad_operands_before_any_launch(monkeypatch):
    def no_launch(*a, **k):
        raise AssertionError("a kernel was launched")
    monkeypatch.setattr(K, "_launch", no_launch)
    f = lambda *s: torch.zeros(*s)      # noqa: E731
    def reverse(x, y):      # well-formed planes and incoming gradient: x and y decide
        planes = torch.zeros((3,) + tuple(x.shape[:-2]) + tuple(max(s - 10, 0) for s in x.shape[-2:]), dtype=torch.float64)
        return K.ssim_loss_backward(x, y, planes, torch.ones(()))
    for fn in (lambda x, y: K.ssim_loss_forward(x, y, True), reverse, losses.ssim_loss, irdu_amd.ssim_loss_sums, irdu_amd.SSIMLoss()):
        with pytest.raises(ValueError, match=r"\[B, C, H, W\]"):
            fn(f(3, 16, 16), f(3, 16, 16))
        with pytest.raises(ValueError, match="float32"):
            fn(f(1, 3, 16, 16).double(), f(1, 3, 16, 16).double())
        with pytest.raises(ValueError, match="must match"):
            fn(f(1, 3, 16, 16), f(1, 3, 16, 17))
        for shape in [(1, 3, 10, 16), (2, 1, 16, 10)]:
            with pytest.raises(ValueError, match="at least 11"):
                fn(f(*shape), f(*shape))
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(f(1, 3, 16, 16), f(1, 3, 16, 16))
    for fn in (lambda x, y: K.ssim_loss_forward(x, y, False), lambda x, y: K.ssim_loss_backward(x, y, None, None)):
        with pytest.raises(ValueError, match="contiguous"):
            fn(f(1, 3, 16, 32)[..., ::2], f(1, 3, 16, 16))
    with pytest.raises(ValueError, match="B C <= 65535"):
        K.ssim_loss_forward(torch.empty(256, 256, 11, 11), torch.empty(256, 256, 11, 11), False)
    # the reverse's own operands
    x = f(1, 3, 16, 16)
    with pytest.raises(ValueError, match="coef must be"):
        K.ssim_loss_backward(x, x, torch.zeros(3, 1, 3, 6, 6), torch.ones(()))             # float32 planes
    with pytest.raises(ValueError, match="coef must be"):
        K.ssim_loss_backward(x, x, torch.zeros(3, 1, 3, 6, 5, dtype=torch.float64), torch.ones(()))
    with pytest.raises(ValueError, match="gout must be one float32"):
        K.ssim_loss_backward(x, x, torch.zeros(3, 1, 3, 6, 6, dtype=torch.float64), torch.ones(2))
    with pytest.raises(ValueError, match="gout must be one float32"):
        K.ssim_loss_backward(x, x, torch.zeros(3, 1, 3, 6, 6, dtype=torch.float64), torch.ones((), dtype=torch.float64))
    # the target takes no gradient
    with pytest.raises(ValueError, match="target takes no gradient"):
        losses.ssim_loss(x, x.clone().requires_grad_(True))


def test_public_names():
    assert irdu_amd.ssim_loss is losses.ssim_loss and irdu_amd.SSIMLoss is losses.SSIMLoss
    assert irdu_amd.ssim_loss_sums is losses.ssim_loss_sums
    from irdu_amd import train_ops
    assert train_ops.OPAQUE["ssim_loss"] is losses.SSIM_LOSS and losses.SSIM_LOSS.n_out == 1
