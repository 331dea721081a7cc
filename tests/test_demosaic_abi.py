"""CPU-only checks of grr_u8_demosaic / grr_u8_demosaic_images (csrc/demosaic_ops.hip) and their wrappers: the header's
declarations against the bindings, the Python mirror of the shape query on both sides of every bound, every refusal
with its status and entry-point name, the wrappers' host checks before any transfer, and the restore.py options.
Launches nothing."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import irdu_amd
from irdu_amd import _native, restore
from irdu_amd import kernels as K

INVALID_ARG, SHAPE, UNSUPPORTED = 1, 2, 3
PTR = 0x1000        # never dereferenced: validation fails first
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return _native.load()


def one(src=PTR, h=8, w=12, src_c=3, dst=PTR + 0x1000, pattern=0, fill=2):
    return (src, h, w, src_c, dst, pattern, fill, None)


def many(arena=PTR, elems=288, table=PTR, n_img=1, max_h=8, max_w=12, dst=PTR + 0x1000, patterns=PTR, fill=2):
    return (arena, elems, table, n_img, max_h, max_w, dst, patterns, fill, None)


def failed(lib, name, args):
    st = getattr(lib, name)(*args)
    return st, lib.grr_last_error() or b""


def test_the_header_declares_what_is_bound():
    text = open(os.path.join(ROOT, "include", "grr.h")).read()
    flat = re.sub(r"\s+", " ", text)
    assert "int grr_u8_demosaic_supported(int src_c, int H, int W);" in flat
    assert ("grr_status grr_u8_demosaic(const uint8_t* src, int H, int W, int src_c, uint8_t* dst, int pattern, int fill, "
            "void* stream);") in flat
    assert ("grr_status grr_u8_demosaic_images(const uint8_t* arena, int64_t elems, const int64_t* table, int n_img, "
            "int max_h, int max_w, uint8_t* dst_arena, const int32_t* patterns, int fill, void* stream);") in flat
    I, L, P = _native.SIGNATURES["grr_u8_demosaic_supported"][0], _native.c_int64, _native.c_void_p
    assert _native.SIGNATURES["grr_u8_demosaic_supported"] == [I, I, I]
    assert _native.SIGNATURES["grr_u8_demosaic"] == [P, I, I, I, P, I, I, P]
    assert _native.SIGNATURES["grr_u8_demosaic_images"] == [P, L, P, I, I, I, P, P, I, P]
    # the definition is written out above them: the codes, the border rule, the rounding, the bound
    for phrase in ("rggb = 0, grbg = 1, gbrg = 2, bggr = 3", "i mod 2(n - 1)", "clamp((s + 8) >> 4, 0, 255)",
                   "8 ctr + 4 cross - 2 far", "10 ctr + 8 h1 - 2 diag - 2 h2 + v2", "10 ctr + 8 v1 - 2 diag - 2 v2 + h2",
                   "12 ctr + 4 diag - 3 far", "2 * 20 * 255"):
        assert phrase in flat, phrase
    assert "demosaic_ops.hip" in open(os.path.join(ROOT, "imagerestoration-development-unrolling_amd",
                                                   "build_native.py")).read()


def test_python_mirror_of_the_shape_query(lib):
    """A call on each side of every bound of grr_u8_demosaic_supported."""
    big = (1 << 31) - 1
    cases = [(c, 8, 12) for c in (-1, 0, 1, 2, 3, 4)]
    cases += [(3, 0, 12), (3, 8, 0), (1, 1, 1), (3, 1, 1), (3, -1, 4), (1, 4, -1)]
    cases += [(1, 1, 715827882), (1, 1, 715827883), (3, 1, 715827882), (3, 1, 715827883), (3, 1 << 15, 21845),
              (3, 1 << 15, 21846), (1, 1 << 15, 21846), (1, big, big), (3, 1, big)]
    seen = set()
    for case in cases:
        got = bool(lib.grr_u8_demosaic_supported(*case))
        assert K.demosaic_ok(*case) == got, case
        seen.add(got)
    assert seen == {True, False}
    assert K.demosaic_ok(1, 1, 715827882) and not K.demosaic_ok(1, 1, 715827883)        # the output has 3 channels
    assert K.DEMOSAIC_PATTERNS == ("rggb", "grbg", "gbrg", "bggr") and K.DEMOSAIC_FILLS == ("zero", "bilinear", "malvar")
    rows, cols = K.DEMOSAIC_TILE
    assert rows >= 1 and cols % 4 == 0 and K.MAX_DEMOSAIC_IMAGES == 65535


@pytest.mark.parametrize("name,args", [("grr_u8_demosaic", one), ("grr_u8_demosaic_images", many)])
def test_bad_arguments_report_their_status_without_a_launch(lib, name, args):
    label = name.encode()
    nulls = ("src", "dst") if args is one else ("arena", "dst", "table", "patterns")
    for null in nulls:
        st, msg = failed(lib, name, args(**{null: None}))
        assert st == INVALID_ARG and label + b": bad args" in msg, null
    for fill in (-1, 3, 7):
        st, msg = failed(lib, name, args(fill=fill))
        assert st == INVALID_ARG and label + b": the fill is 0 (zero), 1 (bilinear) or 2 (malvar)" in msg, fill
    with pytest.raises(_native.GrrError, match=name):
        _native.call(name, *args(fill=3))


def test_the_single_image_form_checks_the_pattern_the_channels_and_the_size(lib):
    name = "grr_u8_demosaic"
    for pattern in (-1, 4, 100):
        st, msg = failed(lib, name, one(pattern=pattern))
        assert st == INVALID_ARG and b"grr_u8_demosaic: the pattern is 0 (rggb)" in msg, pattern
    for c in (2, 4, 5):
        st, msg = failed(lib, name, one(src_c=c))
        assert st == UNSUPPORTED and b"grr_u8_demosaic: needs a source of 1 or 3 channels" in msg, c
    for bad in (dict(h=0), dict(w=-1), dict(src_c=0)):
        st, msg = failed(lib, name, one(**bad))
        assert st == INVALID_ARG and b"grr_u8_demosaic: bad args" in msg, bad
    for c in (1, 3):
        st, msg = failed(lib, name, one(h=1 << 15, w=21846, src_c=c))
        assert st == UNSUPPORTED and b"grr_u8_demosaic" in msg and b"2^31" in msg
    assert lib.grr_u8_demosaic_supported(3, 1 << 15, 21845) == 1


def test_the_arena_form_checks_its_tables_and_bounds(lib):
    name = "grr_u8_demosaic_images"
    st, msg = failed(lib, name, many(n_img=65536, elems=1 << 20))
    assert st == UNSUPPORTED and b"65535" in msg and name.encode() in msg
    st, msg = failed(lib, name, many(n_img=289))                       # more images than pixels
    assert st == UNSUPPORTED and name.encode() in msg
    st, msg = failed(lib, name, many(elems=2, n_img=1))                # fewer elements than one pixel has
    assert st == UNSUPPORTED and name.encode() in msg
    for bad in (dict(table=PTR + 4), dict(patterns=PTR + 2)):
        st, msg = failed(lib, name, many(**bad))
        assert st == INVALID_ARG and b"aligned" in msg, bad
    st, msg = failed(lib, name, many(max_h=1 << 15, max_w=21846))
    assert st == UNSUPPORTED and b"2^31" in msg
    for bad in (dict(elems=0), dict(n_img=0), dict(n_img=-3), dict(max_h=0), dict(max_w=-1)):
        st, msg = failed(lib, name, many(**bad))
        assert st == INVALID_ARG and b"grr_u8_demosaic_images: bad args" in msg, bad


def pack_of(host_table=((0, 8, 12), (288, 5, 7)), c=3, dtype=torch.uint8):
    elems = max(off + h * w * c for off, h, w in host_table)
    return SimpleNamespace(arena=torch.zeros(elems, dtype=dtype), host_table=tuple(host_table), c=c, kinds=("numpy",) * 2,
                           table=torch.tensor(host_table, dtype=torch.int64).reshape(-1, 3))


def no_launch(*a, **k):
    raise AssertionError("a kernel was launched")


def test_wrappers_refuse_before_any_launch_or_transfer(monkeypatch):
    monkeypatch.setattr(K, "_launch", no_launch)
    monkeypatch.setattr(restore, "_to_device", no_launch)
    img = torch.zeros((8, 12, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="GPU"):
        K.u8_demosaic(img, "rggb")
    with pytest.raises(RuntimeError, match="GPU"):
        K.u8_demosaic(img[:, :, 0], 3, 0)
    with pytest.raises(RuntimeError, match="GPU"):
        K.u8_demosaic_images(pack_of(), "rggb")
    for bad in ("rgbg", "RGGB", 4, -1, True, 1.0, None):
        with pytest.raises(ValueError, match="u8_demosaic: the pattern"):
            K.u8_demosaic(img, bad)
        with pytest.raises(ValueError, match="u8_demosaic_images: the pattern"):
            K.u8_demosaic_images(pack_of(), ["rggb", bad])
        with pytest.raises(ValueError, match="demosaic_u8: the pattern"):
            irdu_amd.demosaic_u8(np.zeros((8, 12, 3), np.uint8), bad)
        with pytest.raises(ValueError, match="evaluate_demosaic: the pattern"):
            irdu_amd.evaluate_demosaic(lambda x: x, [np.zeros((16, 16, 3), np.uint8)], bad)
    for bad in ("linear", 3, -1, False, None):
        with pytest.raises(ValueError, match="u8_demosaic: the fill"):
            K.u8_demosaic(img, "rggb", bad)
        with pytest.raises(ValueError, match="u8_demosaic_images: the fill"):
            K.u8_demosaic_images(pack_of(), "rggb", bad)
        with pytest.raises(ValueError, match="demosaic_u8: the fill"):
            irdu_amd.demosaic_u8(np.zeros((8, 12, 3), np.uint8), "rggb", bad)
    assert [K._check_pattern("t", p) for p in K.DEMOSAIC_PATTERNS] == [0, 1, 2, 3] == [K._check_pattern("t", k) for k in range(4)]
    assert [K._check_fill("t", f) for f in K.DEMOSAIC_FILLS] == [0, 1, 2] and K._check_fill("t", np.int64(1)) == 1
    for c in (2, 4):
        with pytest.raises(ValueError, match="u8_demosaic: needs 1 channel"):
            K.u8_demosaic(torch.zeros((8, 12, c), dtype=torch.uint8), 0)
        with pytest.raises(ValueError, match="demosaic_u8: needs 1 channel"):
            irdu_amd.demosaic_u8(np.zeros((8, 12, c), np.uint8), 0)
    with pytest.raises(ValueError, match="uint8"):
        K.u8_demosaic(img.float(), 0)
    with pytest.raises(ValueError, match="demosaic_u8: expected a uint8"):
        irdu_amd.demosaic_u8(np.zeros((8, 12, 3), np.float32), 0)
    with pytest.raises(ValueError, match="H x W x C"):
        K.u8_demosaic(img[0, 0], 0)
    monkeypatch.setattr(K, "_check_placed", lambda *a: None)
    with pytest.raises(ValueError, match="uint8"):
        K.u8_demosaic_images(pack_of(dtype=torch.float32), 0)
    with pytest.raises(ValueError, match="1 patterns for 2 images"):
        K.u8_demosaic_images(pack_of(), ["rggb"])
    with pytest.raises(ValueError, match="takes R, G, B pictures, got 1 channel"):
        K.u8_demosaic_images(pack_of(((0, 8, 12), (96, 5, 7)), c=1), 0)
    with pytest.raises(ValueError, match=r"pattern tensor is int32 \[2\]"):
        K.u8_demosaic_images(pack_of(), torch.tensor([0, 1], dtype=torch.int64))


def test_evaluate_demosaic_checks_before_any_launch(monkeypatch):
    monkeypatch.setattr(K, "_launch", no_launch)
    monkeypatch.setattr(restore, "_to_device", no_launch)
    assert irdu_amd.demosaic_u8 is restore.demosaic_u8 and irdu_amd.evaluate_demosaic is restore.evaluate_demosaic
    assert restore.METRICS == ("psnr", "ssim", "psnr_y", "ssim_y")
    ev, model, z = restore.evaluate_demosaic, (lambda x: x), np.zeros((16, 16, 3), np.uint8)
    with pytest.raises(ValueError, match="evaluate_demosaic: the fill"):
        ev(model, [z], "rggb", "linear")
    for bad in (-1, True, 1.0):
        with pytest.raises(ValueError, match="evaluate_demosaic: shave"):
            ev(model, [z], shave=bad)
    with pytest.raises(ValueError, match="evaluate_demosaic: no images"):
        ev(model, [])
    with pytest.raises(ValueError, match="evaluate_demosaic: image 1 is torch.float32"):
        ev(model, [z, z.astype(np.float32)])
    for c in (1, 2, 4):
        with pytest.raises(ValueError, match="evaluate_demosaic: image 0 is .*clean R, G, B"):
            ev(model, [np.zeros((16, 16, c), np.uint8)])
    with pytest.raises(ValueError, match="evaluate_demosaic: image 1 is .*nothing is left after a shave of 8"):
        ev(model, [np.zeros((40, 40, 3), np.uint8), z], shave=8)
    with pytest.raises(ValueError, match="evaluate_demosaic: image 0 after the shave .*at least 11"):
        ev(model, [z], shave=3)                                         # 10 x 10 is left: too small for SSIM
    with pytest.raises(ValueError, match="evaluate_demosaic: metrics"):
        ev(model, [z], metrics=("cpsnr",))
    with pytest.raises(TypeError, match="evaluate_demosaic: unexpected arguments"):
        ev(model, [z], scale=2)
    assert "CPSNR" in ev.__doc__


def test_wrapper_launch_arguments(monkeypatch):
    """What reaches the library: both arenas under one table, the bounds, the fill, read + written bytes."""
    sent = []
    monkeypatch.setattr(K, "_check_placed", lambda *a: None)
    monkeypatch.setattr(K, "_stream", lambda dev: None)
    monkeypatch.setattr(K, "_launch", lambda kind, nbytes, name, *a, **k: sent.append((kind, nbytes, name, a)))
    pack = pack_of()
    out = K.u8_demosaic_images(pack, ["grbg", 3], "bilinear")
    assert out.table is pack.table and out.host_table == pack.host_table and out.c == 3 and out.kinds == pack.kinds
    assert out.arena.numel() == pack.arena.numel() and out.arena is not pack.arena and out.arena.dtype == torch.uint8
    kind, nbytes, name, a = sent[0]
    assert (kind, name) == ("u8_demosaic_images", "grr_u8_demosaic_images") and nbytes == 2 * (288 + 105)
    assert a[:7] == (pack.arena.data_ptr(), 393, pack.table.data_ptr(), 2, 8, 12, out.arena.data_ptr()) and a[8] == 1
    monkeypatch.setattr(K, "_check_image", lambda name, t: tuple(t.shape))
    for img, c in ((torch.zeros((8, 12, 1), dtype=torch.uint8), 1), (torch.zeros((8, 12), dtype=torch.uint8), 1),
                   (torch.zeros((8, 12, 3), dtype=torch.uint8), 3)):
        sent.clear()
        res = K.u8_demosaic(img, "bggr")
        assert tuple(res.shape) == (8, 12, 3) and res.dtype == torch.uint8
        assert sent[0][2] == "grr_u8_demosaic" and sent[0][1] == 96 * c + 288
        assert sent[0][3][:4] == (img.data_ptr(), 8, 12, c) and sent[0][3][5:7] == (3, 2)
    view = torch.zeros((8, 24, 3), dtype=torch.uint8)[:, ::2]          # not contiguous: copied first
    sent.clear()
    K.u8_demosaic(view, 0, 0)
    assert sent[0][3][0] != view.data_ptr() and sent[0][3][5:7] == (0, 0)


def cli():
    from tests.test_restore_ref import _cli
    return _cli()


def test_restore_command_options():
    command = cli()
    base = ["-yaml_path", "conf.yaml", "--input", "in", "--output", "out"]
    args = command.parse_args(base + ["--bayer", "grbg", "--ssim", "--y-channel", "--batch-images", "--self-ensemble"])
    assert args.bayer == "grbg" and args.scored and args.shave == 0 and args.demosaic_fill == "malvar"
    assert args.ensemble == 8 and args.raw is None
    args = command.parse_args(base + ["--bayer", "rggb", "--shave", "4", "--demosaic-fill", "bilinear"])
    assert args.shave == 4 and args.demosaic_fill == "bilinear"
    args = command.parse_args(base + ["--raw", "bggr", "--demosaic-fill", "zero", "--ensemble-modes", "0,1"])
    assert args.raw == "bggr" and not args.scored and args.shave is None and args.ensemble == (0, 1)
    plain = command.parse_args(base + ["--sigma", "25"])
    assert plain.bayer is None and plain.raw is None and plain.demosaic_fill == "malvar"
    for bad in (["--bayer", "rgbg"], ["--raw", "RGGB"], ["--bayer", "rggb", "--raw", "rggb"],
                ["--bayer", "rggb", "--sigma", "5"], ["--bayer", "rggb", "--jpeg-quality", "10"],
                ["--raw", "rggb", "--scale", "2"], ["--raw", "rggb", "--reference", "refs"],
                ["--demosaic-fill", "malvar"], ["--sigma", "5", "--demosaic-fill", "zero"],
                ["--bayer", "rggb", "--demosaic-fill", "linear"], ["--bayer", "rggb", "--psnrb"],
                ["--raw", "rggb", "--ssim"], ["--raw", "rggb", "--y-channel"], ["--raw", "rggb", "--shave", "2"],
                ["--bayer", "rggb", "--shave", "-1"], ["--bayer", "rggb", "--jpeg-subsampling", "420"]):
        with pytest.raises(SystemExit):
            command.parse_args(base + bad)
