"""CPU-only checks of the luma entry points (csrc/metric_ops.hip: grr_u8_luma_supported, grr_u8_luma_sse,
grr_u8_luma_sse_images, grr_u8_luma_ssim, grr_u8_luma_ssim_images), their wrappers, psnr_y_u8 / ssim_y_u8 and the
"_y" metrics of evaluate_metrics / evaluate_pairs / validate_pairs: argument validation and the Python mirror of the
shape query.  Loads the library, launches nothing."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import irdu_amd
from irdu_amd import _native, restore, training
from irdu_amd import kernels as K

INVALID_ARG, UNSUPPORTED = 1, 3
PTR = 0x1000        # never dereferenced: validation fails first


@pytest.fixture(scope="module")
def lib():
    return _native.load()


def one_args(a=PTR, b=PTR, h=16, w=16, out=PTR):
    return (a, b, h, w, out, None)


def sse_images_args(a=PTR, b=PTR, elems=768, img_table=PTR, n_img=1, out=PTR):
    return (a, b, elems, img_table, n_img, out, None)


def ssim_images_args(a=PTR, b=PTR, elems=768, img_table=PTR, n_img=1, max_h=16, max_w=16, out=PTR):
    return (a, b, elems, img_table, n_img, max_h, max_w, out, None)


ONE = ("grr_u8_luma_sse", "grr_u8_luma_ssim")
IMAGES = (("grr_u8_luma_sse_images", sse_images_args), ("grr_u8_luma_ssim_images", ssim_images_args))


def test_null_and_misaligned_pointers_are_invalid_args(lib):
    for fn in ONE:
        for name in ("a", "b", "out"):
            assert getattr(lib, fn)(*one_args(**{name: None})) == INVALID_ARG, (fn, name)
            assert f"{fn}: bad args".encode() in lib.grr_last_error()
        assert getattr(lib, fn)(*one_args(out=PTR + 4)) == INVALID_ARG              # sums not 8-byte aligned
        assert getattr(lib, fn)(*one_args(a=PTR + 1, b=PTR + 7, h=0)) == INVALID_ARG  # images may start at any byte
    for fn, args in IMAGES:
        for name in ("a", "b", "img_table", "out"):
            assert getattr(lib, fn)(*args(**{name: None})) == INVALID_ARG, (fn, name)
            assert f"{fn}: bad args".encode() in lib.grr_last_error()
        assert getattr(lib, fn)(*args(out=PTR + 4)) == INVALID_ARG
        assert getattr(lib, fn)(*args(img_table=PTR + 4)) == INVALID_ARG            # int64 rows 8-byte aligned
    with pytest.raises(_native.GrrError):
        _native.call("grr_u8_luma_sse", None, None, 16, 16, None, None)


def test_non_positive_sizes_are_invalid_args(lib):
    for fn in ONE:
        for bad in (dict(h=0), dict(h=-4), dict(w=0), dict(w=-16)):
            assert getattr(lib, fn)(*one_args(**bad)) == INVALID_ARG, (fn, bad)
    for fn, args in IMAGES:
        for bad in (dict(elems=0), dict(elems=-1), dict(n_img=0), dict(n_img=-2)):
            assert getattr(lib, fn)(*args(**bad)) == INVALID_ARG, (fn, bad)
    for bad in (dict(max_h=0), dict(max_w=0), dict(max_w=-11)):
        assert lib.grr_u8_luma_ssim_images(*ssim_images_args(**bad)) == INVALID_ARG, bad


def test_unsupported_shapes(lib):
    for fn in ONE:
        assert getattr(lib, fn)(*one_args(h=26755, w=26755)) == UNSUPPORTED         # H W 3 >= 2^31
        assert b"2^31" in lib.grr_last_error()
    assert lib.grr_u8_luma_ssim(*one_args(h=10)) == UNSUPPORTED                     # a side below the window
    assert b">= 11" in lib.grr_last_error()
    assert lib.grr_u8_luma_ssim(*one_args(w=10)) == UNSUPPORTED
    for fn, args in IMAGES:
        assert getattr(lib, fn)(*args(n_img=769)) == UNSUPPORTED                    # more images than elements
        assert getattr(lib, fn)(*args(elems=1 << 20, n_img=K.MAX_SSIM_IMAGES + 1)) == UNSUPPORTED
        assert b"65535" in lib.grr_last_error()                                     # one grid row per image


def test_python_mirror_of_the_luma_query(lib):
    """kernels.luma_ok is what the wrappers enforce; grr_u8_luma_supported is what the entry points enforce."""
    table = [(1, 1), (0, 5), (5, 0), (-3, 7), (10, 11), (11, 10), (11, 11), (481, 321), (2048, 2048), (26754, 26754),
             (26755, 26755), (1, (1 << 31) // 3), (1, (1 << 31) // 3 + 1), (11, 65075262), (11, 65075263), (1, 1 << 30),
             (-11, -11), (10, 10)]
    seen = set()
    for h, w in table:
        for window in (False, True):
            got = bool(lib.grr_u8_luma_supported(h, w, int(window)))
            assert K.luma_ok(h, w, window) == got, (h, w, window)
            seen.add((window, got))
    assert seen == {(False, True), (False, False), (True, True), (True, False)}
    assert K.luma_ok(1, 1) and not K.luma_ok(1, 1, True) and K.luma_ok(11, 11, True) and not K.luma_ok(10, 11, True)
    assert K.luma_ok(26754, 26754) and not K.luma_ok(26755, 26755)
    assert K.luma_ssim_count(11, 11) == 1 and K.luma_ssim_count(20, 31) == 10 * 21
    assert K.LUMA_SCALE == 255000 and sum(K.LUMA_WEIGHTS) == 219000
    rows, cols = K.LUMA_SSIM_TILE
    assert rows >= 1 and cols % 64 == 0
    group, lane = K.LUMA_SSE_BLOCK
    assert lane >= 1 and group % lane == 0 and (group // lane) % 64 == 0 and K.LUMA_SSE_MAX_BLOCKS >= 1
    # the two words of an SSE join into one Python int beyond 64 bits
    assert K._luma_sse_of([(1 << 62) - 1, (1 << 50) - 1]) == (1 << 62) - 1 + (((1 << 50) - 1) << 32)
    # PSNR-Y is one true division of ints, then log10
    assert restore._psnr_y(0, 100) == float("inf")
    assert restore._psnr_y(6400 * 55845000 ** 2, 6400) == float(10.0 * np.log10((255 ** 2 * 255000 ** 2) / 55845000 ** 2))


def pack_of(host_table, c=3, **over):
    elems = sum(h * w * c for _, h, w in host_table)
    fields = dict(arena=torch.zeros(elems, dtype=torch.uint8), table=torch.tensor(host_table, dtype=torch.int64).reshape(-1, 3),
                  host_table=tuple(host_table), c=c)
    fields.update(over)
    return SimpleNamespace(**fields)


GOOD = ((0, 16, 16), (768, 17, 31))


def no_launch(*a, **k):
    raise AssertionError("a kernel was launched")


def no_draw(*a, **k):
    raise AssertionError("noise was drawn")


def test_wrappers_refuse_bad_operands_before_any_launch(monkeypatch):
    monkeypatch.setattr(K, "_launch", no_launch)
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)      # noqa: E731
    for fn in (K.u8_luma_sse, K.u8_luma_ssim):
        with pytest.raises(ValueError, match="uint8"):
            fn(torch.zeros(16, 16, 3), torch.zeros(16, 16, 3))
        with pytest.raises(ValueError, match="H x W x 3"):
            fn(u8(16, 16), u8(16, 16))
        for c in (1, 2, 4):
            with pytest.raises(ValueError, match="H x W x 3"):
                fn(u8(16, 16, c), u8(16, 16, c))
        with pytest.raises(ValueError, match="must match"):
            fn(u8(16, 16, 3), u8(16, 17, 3))
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(u8(16, 16, 3), u8(16, 16, 3))
    for shape in [(10, 16, 3), (16, 10, 3)]:
        with pytest.raises(ValueError, match="at least 11"):
            K.u8_luma_ssim(u8(*shape), u8(*shape))
        with pytest.raises(RuntimeError, match="no CPU path"):      # the SSE has no window
            K.u8_luma_sse(u8(*shape), u8(*shape))
    # packs
    for fn in (K.u8_luma_sse_images, K.u8_luma_ssim_images):
        with pytest.raises(ValueError, match="same images"):
            fn(pack_of(GOOD), pack_of(((0, 16, 16), (768, 31, 17))))
        with pytest.raises(ValueError, match="same images"):
            fn(pack_of(GOOD), pack_of(GOOD[:1]))
        for c in (1, 4):
            rows = ((0, 16, 16), (256 * c, 17, 31))
            with pytest.raises(ValueError, match="H x W x 3"):
                fn(pack_of(rows, c=c), pack_of(rows, c=c))
        with pytest.raises(ValueError, match="uint8 arenas"):
            fn(pack_of(GOOD, arena=torch.zeros(2349)), pack_of(GOOD, arena=torch.zeros(2349)))
        with pytest.raises(ValueError, match="int64"):
            fn(pack_of(GOOD), pack_of(GOOD, table=torch.zeros(2, 3, dtype=torch.int32)))
        with pytest.raises(RuntimeError, match="GPU"):
            fn(pack_of(GOOD), pack_of(GOOD))
    small = ((0, 16, 16), (768, 10, 31))
    with pytest.raises(ValueError, match="image 1 needs both sides at least 11"):
        K.u8_luma_ssim_images(pack_of(small), pack_of(small))
    with pytest.raises(RuntimeError, match="GPU"):
        K.u8_luma_sse_images(pack_of(small), pack_of(small))


def test_psnr_y_and_ssim_y_check_their_images_before_any_launch(monkeypatch):
    monkeypatch.setattr(K, "_launch", no_launch)
    assert irdu_amd.psnr_y_u8 is restore.psnr_y_u8 and irdu_amd.ssim_y_u8 is restore.ssim_y_u8
    assert restore.METRICS == ("psnr", "ssim", "psnr_y", "ssim_y")
    for name, fn in (("psnr_y_u8", restore.psnr_y_u8), ("ssim_y_u8", restore.ssim_y_u8)):
        with pytest.raises(ValueError, match=f"{name}: expected uint8"):
            fn(np.zeros((16, 16, 3), dtype=np.float32), np.zeros((16, 16, 3), dtype=np.float32))
        with pytest.raises(ValueError, match=f"{name}: expected uint8"):
            fn(torch.zeros(16, 16, 3), torch.zeros(16, 16, 3))
        with pytest.raises(ValueError, match=f"{name}: shapes differ"):
            fn(np.zeros((16, 16, 3), dtype=np.uint8), np.zeros((16, 17, 3), dtype=np.uint8))
        for shape in [(16, 16), (16, 16, 1), (16, 16, 4)]:
            with pytest.raises(ValueError, match=f"{name}: the luma is defined for H x W x 3"):
                fn(np.zeros(shape, dtype=np.uint8), np.zeros(shape, dtype=np.uint8))
    for shape in [(10, 16, 3), (16, 10, 3)]:
        with pytest.raises(ValueError, match="ssim_y_u8: .*at least 11"):
            restore.ssim_y_u8(np.zeros(shape, dtype=np.uint8), np.zeros(shape, dtype=np.uint8))


def test_evaluate_metrics_refuses_bad_requests_before_any_draw(monkeypatch):
    monkeypatch.setattr(restore, "_noisy", no_draw)
    monkeypatch.setattr(K, "_launch", no_launch)
    ok = [np.zeros((16, 16, 3), dtype=np.float32)]
    for across in (False, True):
        for bad in (("psnr", "mse"), ("SSIM",), (), ("psnr", "psnr"), "lpips", ("psnr_y", "psnr_y"), ("PSNR_Y",),
                    ("ssim_y", "y"), "psnr-y"):
            with pytest.raises(ValueError, match="evaluate_metrics: metrics"):
                restore.evaluate_metrics(lambda x: x, ok, metrics=bad, across_images=across)
        for metrics in (("psnr_y",), ("ssim_y",), ("psnr", "ssim", "psnr_y", "ssim_y"), "psnr_y"):
            for shape in [(16, 16, 1), (16, 16, 4), (16, 16)]:
                images = ok + [np.zeros(shape, dtype=np.float32)]
                with pytest.raises(ValueError, match="evaluate_metrics: image 1"):
                    restore.evaluate_metrics(lambda x: x, images, metrics=metrics, across_images=across)
        for shape in [(10, 16, 3), (16, 10, 3)]:
            images = ok + [np.zeros(shape, dtype=np.float32)]
            with pytest.raises(ValueError, match="evaluate_metrics: image 1 .*at least 11"):
                restore.evaluate_metrics(lambda x: x, images, metrics=("ssim_y",), across_images=across)
            with pytest.raises(ValueError, match="evaluate_metrics: image 1 .*at least 11"):
                restore.evaluate_metrics(lambda x: x, images, metrics=("psnr_y", "ssim_y"), across_images=across)
        with pytest.raises(ValueError, match="ensemble"):
            restore.evaluate_metrics(lambda x: x, ok, ensemble=3, metrics=("psnr_y",), across_images=across)


def test_evaluate_pairs_and_validate_pairs_refuse_bad_requests_before_any_launch(monkeypatch):
    monkeypatch.setattr(K, "_launch", no_launch)
    u8 = lambda *s: np.zeros(s, dtype=np.uint8)      # noqa: E731
    ok = [u8(16, 16, 3)]
    for across in (False, True):
        for bad in (("psnr", "mse"), ("SSIM",), (), ("psnr_y", "psnr_y"), "lpips"):
            with pytest.raises(ValueError, match="evaluate_pairs: metrics"):
                restore.evaluate_pairs(lambda x: x, ok, ok, metrics=bad, across_images=across)
        for metrics in (("psnr_y",), ("ssim_y",), ("psnr", "psnr_y")):
            for shape in [(16, 16, 1), (16, 16, 4)]:
                both = ok + [u8(*shape)]
                with pytest.raises(ValueError, match="evaluate_pairs: pair 1 .*H x W x 3"):
                    restore.evaluate_pairs(lambda x: x, both, both, metrics=metrics, across_images=across)
        both = ok + [u8(10, 16, 3)]
        with pytest.raises(ValueError, match="evaluate_pairs: pair 1 .*at least 11"):
            restore.evaluate_pairs(lambda x: x, both, both, metrics=("ssim_y",), across_images=across)
        with pytest.raises(ValueError, match="one shape"):
            restore.evaluate_pairs(lambda x: x, ok, [u8(16, 17, 3)], metrics=("psnr_y",), across_images=across)
        with pytest.raises(ValueError, match="uint8"):
            restore.evaluate_pairs(lambda x: x, [np.zeros((16, 16, 3), dtype=np.float32)], ok, metrics=("psnr_y",),
                                   across_images=across)
    with pytest.raises(ValueError, match="validate_pairs: metric"):
        training.validate_pairs(torch.nn.Identity(), [(ok[0], ok[0])], metric="ssim_y")
    with pytest.raises(ValueError, match="validate_pairs: metric"):
        training.validate_pairs(torch.nn.Identity(), [(ok[0], ok[0])], metric="PSNR")


def test_the_validation_config_passes_the_metric_through(monkeypatch):
    monkeypatch.setitem(training.VAL_DATASETS, "TestPairsCSV", training.TestPairsCSV)
    monkeypatch.setattr(training.TestPairsCSV, "__init__", lambda self, **kw: None)
    val = {"type": "TestPairsCSV", "factor": 16, "tile": 64, "dataset_args": {}}
    _, args = training.create_val_dataset({"datasets": {"val": dict(val)}})
    assert args == {"tile": 64, "factor": 16}                       # no metric: validate_pairs' default
    _, args = training.create_val_dataset({"datasets": {"val": dict(val, metric="psnr_y")}})
    assert args == {"tile": 64, "factor": 16, "metric": "psnr_y"}
    with pytest.raises(ValueError, match="datasets.val.metric"):
        training.create_val_dataset({"datasets": {"val": dict(val, metric="ssim")}})
