"""CPU-only checks of the SSIM entry points (csrc/metric_ops.hip: grr_u8_ssim_supported, grr_u8_ssim,
grr_u8_ssim_images), their wrappers and evaluate_metrics: argument validation and the Python mirror of the shape
query.  Loads the library, launches nothing."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import irdu_amd
from irdu_amd import _native, restore
from irdu_amd import kernels as K

INVALID_ARG, UNSUPPORTED = 1, 3
PTR = 0x1000        # never dereferenced: validation fails first


@pytest.fixture(scope="module")
def lib():
    return _native.load()


def one_args(a=PTR, b=PTR, h=16, w=16, c=3, out=PTR):
    return (a, b, h, w, c, out, None)


def images_args(a=PTR, b=PTR, elems=768, c=3, img_table=PTR, n_img=1, max_h=16, max_w=16, out=PTR):
    return (a, b, elems, c, img_table, n_img, max_h, max_w, out, None)


def test_null_and_misaligned_pointers_are_invalid_args(lib):
    for name in ("a", "b", "out"):
        assert lib.grr_u8_ssim(*one_args(**{name: None})) == INVALID_ARG, name
        assert b"grr_u8_ssim: bad args" in lib.grr_last_error()
    for name in ("a", "b", "img_table", "out"):
        assert lib.grr_u8_ssim_images(*images_args(**{name: None})) == INVALID_ARG, name
        assert b"grr_u8_ssim_images: bad args" in lib.grr_last_error()
    assert lib.grr_u8_ssim(*one_args(out=PTR + 4)) == INVALID_ARG                 # sum not 8-byte aligned
    assert lib.grr_u8_ssim_images(*images_args(out=PTR + 4)) == INVALID_ARG
    assert lib.grr_u8_ssim_images(*images_args(img_table=PTR + 4)) == INVALID_ARG   # int64 rows 8-byte aligned
    assert lib.grr_u8_ssim(*one_args(a=PTR + 1, b=PTR + 7, h=0)) == INVALID_ARG     # images may start at any byte
    with pytest.raises(_native.GrrError):
        _native.call("grr_u8_ssim", None, None, 16, 16, 3, None, None)


def test_non_positive_sizes_are_invalid_args(lib):
    for bad in (dict(h=0), dict(h=-4), dict(w=0), dict(c=0), dict(c=-1)):
        assert lib.grr_u8_ssim(*one_args(**bad)) == INVALID_ARG, bad
    for bad in (dict(elems=0), dict(elems=-1), dict(c=0), dict(n_img=0), dict(n_img=-2), dict(max_h=0), dict(max_w=0),
                dict(max_w=-11)):
        assert lib.grr_u8_ssim_images(*images_args(**bad)) == INVALID_ARG, bad


def test_unsupported_shapes(lib):
    assert lib.grr_u8_ssim(*one_args(c=5)) == UNSUPPORTED
    assert b"C <= 4" in lib.grr_last_error()
    assert lib.grr_u8_ssim(*one_args(h=10)) == UNSUPPORTED                       # a side below the window
    assert b">= 11" in lib.grr_last_error()
    assert lib.grr_u8_ssim(*one_args(w=10)) == UNSUPPORTED
    assert lib.grr_u8_ssim(*one_args(h=26755, w=26755, c=3)) == UNSUPPORTED     # H W C >= 2^31
    assert lib.grr_u8_ssim_images(*images_args(c=5)) == UNSUPPORTED
    assert lib.grr_u8_ssim_images(*images_args(n_img=769)) == UNSUPPORTED       # more images than elements
    assert lib.grr_u8_ssim_images(*images_args(elems=1 << 20, n_img=K.MAX_SSIM_IMAGES + 1)) == UNSUPPORTED
    assert b"65535" in lib.grr_last_error()                                     # one grid row per image


def test_python_mirror_of_the_ssim_query(lib):
    """kernels.ssim_ok is what the wrappers enforce; grr_u8_ssim_supported is what grr_u8_ssim enforces."""
    table = [(1, 10, 11), (1, 11, 10), (1, 11, 11), (5, 11, 11), (3, 26755, 26755), (0, 11, 11), (-1, 64, 64),
             (4, 11, 11), (3, 481, 321), (3, 2048, 2048), (1, 46340, 46340), (1, 46341, 46341), (4, 23170, 23170),
             (4, 23171, 23171), (2, 11, 0), (2, -11, -11), (3, 26754, 26754), (1, 1, 1 << 30), (1, 11, (1 << 31) // 11)]
    seen = set()
    for c, h, w in table:
        got = bool(lib.grr_u8_ssim_supported(c, h, w))
        assert K.ssim_ok(c, h, w) == got, (c, h, w)
        seen.add(got)
    assert seen == {True, False}
    assert K.ssim_ok(1, 11, 11) and not K.ssim_ok(1, 10, 11) and not K.ssim_ok(1, 11, 10) and not K.ssim_ok(5, 11, 11)
    assert not K.ssim_ok(3, 26755, 26755) and K.ssim_ok(3, 26754, 26754)
    assert K.ssim_count(3, 11, 11) == 3 and K.ssim_count(1, 20, 31) == 10 * 21
    assert K.SSIM_ONE == 1 << 32 and K.SSIM_WINDOW == 11
    rows, cols = K.SSIM_TILE
    assert rows >= 1 and cols % 64 == 0


def pack_of(host_table, c=3, **over):
    elems = sum(h * w * c for _, h, w in host_table)
    fields = dict(arena=torch.zeros(elems, dtype=torch.uint8), table=torch.tensor(host_table, dtype=torch.int64).reshape(-1, 3),
                  host_table=tuple(host_table), c=c)
    fields.update(over)
    return SimpleNamespace(**fields)


GOOD = ((0, 16, 16), (768, 17, 31))


def test_wrappers_refuse_bad_operands_before_any_launch(monkeypatch):
    def no_launch(*a, **k):
        raise AssertionError("a kernel was launched")
    monkeypatch.setattr(K, "_launch", no_launch)
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)      # noqa: E731
    with pytest.raises(ValueError, match="uint8"):
        K.u8_ssim(torch.zeros(16, 16, 3), torch.zeros(16, 16, 3))
    with pytest.raises(ValueError, match="H x W x C"):
        K.u8_ssim(u8(16, 16), u8(16, 16))
    with pytest.raises(ValueError, match="must match"):
        K.u8_ssim(u8(16, 16, 3), u8(16, 17, 3))
    for shape in [(10, 16, 3), (16, 10, 3), (16, 16, 5)]:
        with pytest.raises(ValueError, match="at least 11"):
            K.u8_ssim(u8(*shape), u8(*shape))
    with pytest.raises(RuntimeError, match="no CPU path"):
        K.u8_ssim(u8(16, 16, 3), u8(16, 16, 3))
    # packs
    with pytest.raises(ValueError, match="same images"):
        K.u8_ssim_images(pack_of(GOOD), pack_of(((0, 16, 16), (768, 31, 17))))
    with pytest.raises(ValueError, match="same images"):
        K.u8_ssim_images(pack_of(GOOD), pack_of(GOOD[:1]))
    small = ((0, 16, 16), (768, 10, 31))
    with pytest.raises(ValueError, match="image 1 needs both sides at least 11"):
        K.u8_ssim_images(pack_of(small), pack_of(small))
    with pytest.raises(ValueError, match="uint8 arenas"):
        K.u8_ssim_images(pack_of(GOOD, arena=torch.zeros(2349)), pack_of(GOOD, arena=torch.zeros(2349)))
    with pytest.raises(ValueError, match="int64"):
        K.u8_ssim_images(pack_of(GOOD), pack_of(GOOD, table=torch.zeros(2, 3, dtype=torch.int32)))
    with pytest.raises(RuntimeError, match="GPU"):
        K.u8_ssim_images(pack_of(GOOD), pack_of(GOOD))


def test_ssim_u8_checks_its_images_before_any_launch(monkeypatch):
    def no_launch(*a, **k):
        raise AssertionError("a kernel was launched")
    monkeypatch.setattr(K, "_launch", no_launch)
    assert irdu_amd.ssim_u8 is restore.ssim_u8 and irdu_amd.evaluate_metrics is restore.evaluate_metrics
    with pytest.raises(ValueError, match="ssim_u8: expected uint8"):
        restore.ssim_u8(np.zeros((16, 16, 3), dtype=np.float32), np.zeros((16, 16, 3), dtype=np.float32))
    with pytest.raises(ValueError, match="ssim_u8: expected uint8"):
        restore.ssim_u8(torch.zeros(16, 16, 3), torch.zeros(16, 16, 3))
    # sum q / (2^32 N) is one correctly rounded division of Python ints
    assert restore._ssim(5 << 32, 5) == 1.0 and restore._ssim(-(3 << 31), 3) == -0.5
    assert restore._ssim((1 << 32) + 1, 1) == 1.0 + 2.0 ** -32
    assert restore._ssim(1, 3) == 1 / (3 * 2 ** 32)
    big = (1 << 62) + 1          # float(big) would already round
    assert restore._ssim(big, 1 << 30) == float(np.float64(1.0))


def test_evaluate_metrics_refuses_bad_requests_before_any_draw(monkeypatch):
    def no_draw(*a, **k):
        raise AssertionError("noise was drawn")

    def no_launch(*a, **k):
        raise AssertionError("a kernel was launched")
    monkeypatch.setattr(restore, "_noisy", no_draw)
    monkeypatch.setattr(K, "_launch", no_launch)
    ok = [np.zeros((16, 16, 3), dtype=np.float32)]
    for across in (False, True):
        for bad in (("psnr", "mse"), ("SSIM",), (), ("psnr", "psnr"), "lpips"):
            with pytest.raises(ValueError, match="evaluate_metrics: metrics"):
                restore.evaluate_metrics(lambda x: x, ok, metrics=bad, across_images=across)
        for shape in [(10, 16, 3), (16, 10, 3), (16, 16)]:
            images = ok + [np.zeros(shape, dtype=np.float32)]
            with pytest.raises(ValueError, match="evaluate_metrics: image 1"):
                restore.evaluate_metrics(lambda x: x, images, across_images=across)
            with pytest.raises(ValueError, match="image 1"):
                restore.evaluate_metrics(lambda x: x, images, metrics=("ssim",), across_images=across)
        with pytest.raises(ValueError, match="ensemble"):
            restore.evaluate_metrics(lambda x: x, ok, ensemble=3, across_images=across)
        with pytest.raises(TypeError, match="evaluate_metrics: unexpected arguments"):
            restore.evaluate_metrics(lambda x: x, ok, tiles=4, across_images=across)
