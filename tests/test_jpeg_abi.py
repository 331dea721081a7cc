"""CPU-only checks of grr_u8_jpeg / grr_u8_jpeg_images (csrc/jpeg_ops.hip), grr_u8_blocking / grr_u8_blocking_images
(csrc/metric_ops.hip) and their wrappers: the Python mirror of the shape query on both sides of every bound, every
refusal with its status and entry-point name, and the wrappers' host checks.  Launches nothing."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import irdu_amd
from irdu_amd import _native, restore
from irdu_amd import kernels as K

INVALID_ARG, SHAPE, UNSUPPORTED = 1, 2, 3
PTR = 0x1000        # never dereferenced: validation fails first


@pytest.fixture(scope="module")
def lib():
    return _native.load()


def one(src=PTR, h=8, w=12, c=3, dst=PTR + 0x1000, quality=10, sub=0):
    return (src, h, w, c, dst, quality, sub, None)


def many(arena=PTR, elems=288, c=3, table=PTR, n_img=1, max_h=8, max_w=12, dst=PTR + 0x1000, qualities=PTR, sub=0):
    return (arena, elems, c, table, n_img, max_h, max_w, dst, qualities, sub, None)


def blocking_one(est=PTR, h=16, w=16, c=3, out=PTR + 0x1000):
    return (est, h, w, c, out, None)


def blocking_many(est=PTR, elems=768, c=3, table=PTR, n_img=1, max_h=16, max_w=16, out=PTR + 0x1000):
    return (est, elems, c, table, n_img, max_h, max_w, out, None)


def failed(lib, name, args):
    st = getattr(lib, name)(*args)
    return st, lib.grr_last_error() or b""


def test_python_mirror_of_the_shape_query(lib):
    """A call on each side of every bound of grr_u8_jpeg_supported."""
    big = (1 << 31) - 1
    cases = [(c, 8, 12, sub) for c in (0, 1, 2, 3, 4) for sub in (-1, 0, 1, 2, 3)]
    cases += [(3, 0, 12, 0), (3, 8, 0, 2), (1, 1, 1, 0), (3, 1, 1, 2), (3, -1, 4, 0)]
    cases += [(1, 1, big, 0), (1, 2, 1 << 30, 0), (1, big, 1, 2), (3, 1, 715827882, 0), (3, 1, 715827883, 0),
              (3, 1 << 15, 21845, 2), (3, 1 << 15, 21846, 2), (1, big, big, 0)]
    seen = set()
    for case in cases:
        got = bool(lib.grr_u8_jpeg_supported(*case))
        assert K.jpeg_ok(*case) == got, case
        seen.add(got)
    assert seen == {True, False}
    assert K.jpeg_ok(1, 1, big, 0) and not K.jpeg_ok(1, 2, 1 << 30, 0)
    assert K.jpeg_ok(3, 1, 715827882, 2) and not K.jpeg_ok(3, 1, 715827883, 2)
    assert K.JPEG_TILE == 32 and K.JPEG_TILE % 16 == 0


@pytest.mark.parametrize("name,args", [("grr_u8_jpeg", one), ("grr_u8_jpeg_images", many)])
def test_bad_arguments_report_their_status_without_a_launch(lib, name, args):
    label = name.encode()
    nulls = ("src", "dst") if args is one else ("arena", "dst", "table", "qualities")
    for null in nulls:
        st, msg = failed(lib, name, args(**{null: None}))
        assert st == INVALID_ARG and label + b": bad args" in msg, null
    for c in (2, 4, 5):
        st, msg = failed(lib, name, args(c=c))
        assert st == UNSUPPORTED and label in msg and b"C of 1 or 3" in msg, c
    for sub in (-1, 1, 3):
        st, msg = failed(lib, name, args(sub=sub))
        assert st == UNSUPPORTED and label in msg and b"subsampling" in msg, sub
    st, msg = failed(lib, name, args(c=0))
    assert st == INVALID_ARG and label + b": bad args" in msg
    with pytest.raises(_native.GrrError, match=name):
        _native.call(name, *args(c=0))


def test_the_single_image_form_checks_the_quality_and_the_size(lib):
    for q in (0, 101, -5):
        st, msg = failed(lib, "grr_u8_jpeg", one(quality=q))
        assert st == INVALID_ARG and b"grr_u8_jpeg: the quality is 1..100" in msg, q
    for bad in (dict(h=0), dict(w=-1)):
        st, msg = failed(lib, "grr_u8_jpeg", one(**bad))
        assert st == INVALID_ARG and b"grr_u8_jpeg: bad args" in msg, bad
    st, msg = failed(lib, "grr_u8_jpeg", one(h=1 << 15, w=21846))
    assert st == UNSUPPORTED and b"grr_u8_jpeg" in msg and b"2^31" in msg
    assert lib.grr_u8_jpeg_supported(3, 1 << 15, 21845, 0) == 1


def test_the_arena_form_checks_its_tables_and_bounds(lib):
    name = "grr_u8_jpeg_images"
    st, msg = failed(lib, name, many(n_img=65536, elems=1 << 20))
    assert st == UNSUPPORTED and b"65535" in msg and name.encode() in msg
    st, msg = failed(lib, name, many(n_img=289))
    assert st == UNSUPPORTED and name.encode() in msg
    st, msg = failed(lib, name, many(elems=2, n_img=1))                # fewer elements than one pixel has
    assert st == UNSUPPORTED and name.encode() in msg
    for bad in (dict(table=PTR + 4), dict(qualities=PTR + 2)):
        st, msg = failed(lib, name, many(**bad))
        assert st == INVALID_ARG and b"aligned" in msg, bad
    st, msg = failed(lib, name, many(max_h=1 << 15, max_w=21846))
    assert st == UNSUPPORTED and b"2^31" in msg
    for bad in (dict(elems=0), dict(n_img=0), dict(max_h=0), dict(max_w=-1)):
        st, msg = failed(lib, name, many(**bad))
        assert st == INVALID_ARG and b"grr_u8_jpeg_images: bad args" in msg, bad


def test_the_blocking_entry_points_refuse_without_a_launch(lib):
    for name, args in (("grr_u8_blocking", blocking_one), ("grr_u8_blocking_images", blocking_many)):
        label = name.encode()
        for null in ("est", "out") + (("table",) if args is blocking_many else ()):
            st, msg = failed(lib, name, args(**{null: None}))
            assert st == INVALID_ARG and label + b": bad args" in msg, null
        st, msg = failed(lib, name, args(out=PTR + 4))
        assert st == INVALID_ARG and label + b": bad args" in msg
        st, msg = failed(lib, name, args(c=5))
        assert st == UNSUPPORTED and label in msg and b"C <= 4" in msg
    st, msg = failed(lib, "grr_u8_blocking", blocking_one(h=1 << 15, w=1 << 16, c=1))
    assert st == UNSUPPORTED and b"2^31" in msg
    st, msg = failed(lib, "grr_u8_blocking_images", blocking_many(max_h=1 << 15, max_w=1 << 16, c=1, elems=1 << 40))
    assert st == UNSUPPORTED and b"2^31" in msg
    st, msg = failed(lib, "grr_u8_blocking_images", blocking_many(n_img=65536, elems=1 << 20))
    assert st == UNSUPPORTED and b"65535" in msg
    st, msg = failed(lib, "grr_u8_blocking_images", blocking_many(table=PTR + 4))
    assert st == INVALID_ARG


def pack_of(host_table=((0, 8, 12), (288, 5, 7)), c=3, dtype=torch.uint8):
    elems = max(off + h * w * c for off, h, w in host_table)
    return SimpleNamespace(arena=torch.zeros(elems, dtype=dtype), host_table=tuple(host_table), c=c, kinds=("numpy",) * 2,
                           table=torch.tensor(host_table, dtype=torch.int64).reshape(-1, 3))


def no_launch(*a, **k):
    raise AssertionError("a kernel was launched")


def test_wrappers_refuse_before_any_launch(monkeypatch):
    monkeypatch.setattr(K, "_launch", no_launch)
    img = torch.zeros((8, 12, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="GPU"):
        K.u8_jpeg(img, 10)
    with pytest.raises(RuntimeError, match="GPU"):
        K.u8_jpeg_images(pack_of(), 10)
    with pytest.raises(RuntimeError, match="GPU"):
        K.u8_blocking(torch.zeros((16, 16, 3), dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="GPU"):
        K.u8_blocking_images(pack_of())
    for bad in (0, 101, 10.0, True, "10", None):
        with pytest.raises(ValueError, match="u8_jpeg: the quality"):
            K.u8_jpeg(img, bad)
        with pytest.raises(ValueError, match="u8_jpeg_images: the quality"):
            K.u8_jpeg_images(pack_of(), [10, bad])
        with pytest.raises(ValueError, match="jpeg_degrade_u8: the quality"):
            irdu_amd.jpeg_degrade_u8(np.zeros((8, 12, 3), np.uint8), bad)
    for bad in (1, 3, True, "420", 2.0):
        with pytest.raises(ValueError, match="u8_jpeg: the subsampling"):
            K.u8_jpeg(img, 10, bad)
        with pytest.raises(ValueError, match="u8_jpeg_images: the subsampling"):
            K.u8_jpeg_images(pack_of(), 10, bad)
    for c in (2, 4):
        with pytest.raises(ValueError, match="u8_jpeg: needs 1 or 3 channels"):
            K.u8_jpeg(torch.zeros((8, 12, c), dtype=torch.uint8), 10)
    with pytest.raises(ValueError, match="uint8"):
        K.u8_jpeg(img.float(), 10)
    with pytest.raises(ValueError, match="H x W x C"):
        K.u8_jpeg(img[0], 10)
    with pytest.raises(ValueError, match="uint8"):
        K.u8_blocking(torch.zeros((16, 16, 3)))
    monkeypatch.setattr(K, "_check_placed", lambda *a: None)
    with pytest.raises(ValueError, match="uint8"):
        K.u8_jpeg_images(pack_of(dtype=torch.float32), 10)
    with pytest.raises(ValueError, match="1 qualities for 2 images"):
        K.u8_jpeg_images(pack_of(), [10])
    with pytest.raises(ValueError, match="image 0 needs 1 or 3 channels"):
        K.u8_jpeg_images(pack_of(((0, 8, 12), (192, 5, 7)), c=2), 10)
    with pytest.raises(ValueError, match=r"quality tensor is int32 \[2\]"):
        K.u8_jpeg_images(pack_of(), torch.tensor([10, 20], dtype=torch.int64))
    with pytest.raises(ValueError, match="uint8"):
        K.u8_blocking_images(pack_of(dtype=torch.float32))


def test_psnrb_and_evaluate_car_check_before_any_launch(monkeypatch):
    monkeypatch.setattr(K, "_launch", no_launch)
    assert irdu_amd.psnrb_u8 is restore.psnrb_u8 and irdu_amd.evaluate_car is restore.evaluate_car
    assert restore.BLOCKING_METRICS == ("psnrb",) and K.PSNRB_MIN_SIDE == 16
    z = np.zeros((16, 16, 3), np.uint8)
    with pytest.raises(ValueError, match="psnrb_u8: expected uint8"):
        restore.psnrb_u8(z.astype(np.float32), z.astype(np.float32))
    with pytest.raises(ValueError, match="psnrb_u8: shapes differ"):
        restore.psnrb_u8(z, np.zeros((16, 17, 3), np.uint8))
    for shape in ((15, 16, 3), (16, 15, 1), (16, 16)):
        with pytest.raises(ValueError, match="psnrb_u8: .*at least 16"):
            restore.psnrb_u8(np.zeros(shape, np.uint8), np.zeros(shape, np.uint8))
    model = lambda x: x
    for metrics_fn, args in ((restore.evaluate_metrics, ([z.astype(np.float32), np.zeros((15, 20, 3), np.float32)],)),
                             (restore.evaluate_pairs, ([z, np.zeros((15, 20, 3), np.uint8)],) * 2)):
        with pytest.raises(ValueError, match="1 .*PSNR-B needs.*at least 16"):
            metrics_fn(model, *args, metrics=("psnr", "psnrb"), device="cpu")
    car = restore.evaluate_car
    for bad in (0, 101, True, 10.0):
        with pytest.raises(ValueError, match="evaluate_car: the quality"):
            car(model, [z], bad)
    with pytest.raises(ValueError, match="evaluate_car: the subsampling"):
        car(model, [z], 10, 1)
    with pytest.raises(ValueError, match="evaluate_car: no images"):
        car(model, [], 10)
    with pytest.raises(ValueError, match="evaluate_car: image 1 is torch.float32"):
        car(model, [z, z.astype(np.float32)], 10)
    with pytest.raises(ValueError, match="evaluate_car: image 0 is .*1 or 3 channels"):
        car(model, [np.zeros((16, 16, 2), np.uint8)], 10)
    with pytest.raises(ValueError, match="evaluate_car: image 0 .*at least 16"):
        car(model, [np.zeros((12, 16, 3), np.uint8)], 10)
    with pytest.raises(ValueError, match="evaluate_car: image 0 .*Y-channel"):
        car(model, [np.zeros((16, 16, 1), np.uint8)], 10, metrics=("psnr_y",))
    with pytest.raises(ValueError, match="evaluate_car: metrics"):
        car(model, [z], 10, metrics=("psnrc",))
    with pytest.raises(TypeError, match="evaluate_car: unexpected arguments"):
        car(model, [z], 10, shave=2)


def test_wrapper_launch_arguments(monkeypatch):
    """What reaches the library: both arenas under one table, the bounds, the qualities, read + written bytes."""
    sent = []
    monkeypatch.setattr(K, "_check_placed", lambda *a: None)
    monkeypatch.setattr(K, "_stream", lambda dev: None)
    monkeypatch.setattr(K, "_launch", lambda kind, nbytes, name, *a, **k: sent.append((kind, nbytes, name, a)))
    pack = pack_of()
    out = K.u8_jpeg_images(pack, [10, 40], 2)
    assert out.table is pack.table and out.host_table == pack.host_table and out.c == 3 and out.kinds == pack.kinds
    assert out.arena.numel() == pack.arena.numel() and out.arena is not pack.arena and out.arena.dtype == torch.uint8
    kind, nbytes, name, a = sent[0]
    assert (kind, name) == ("u8_jpeg_images", "grr_u8_jpeg_images") and nbytes == 2 * (288 + 105)
    assert a[:8] == (pack.arena.data_ptr(), 393, 3, pack.table.data_ptr(), 2, 8, 12, out.arena.data_ptr()) and a[9] == 2
    img = torch.zeros((8, 12, 1), dtype=torch.uint8)
    monkeypatch.setattr(K, "_check_image", lambda name, t: tuple(t.shape))
    res = K.u8_jpeg(img, 75)
    assert res.shape == img.shape and sent[1][2] == "grr_u8_jpeg" and sent[1][1] == 2 * 96
    assert sent[1][3][:4] == (img.data_ptr(), 8, 12, 1) and sent[1][3][5:7] == (75, 0)
