"""CPU-only checks of grr_u8_blur / grr_u8_blur_images (csrc/blur_ops.hip) and their wrappers: the header's declarations
against the bindings, the Python mirror of the shape query on both sides of every bound, every refusal with its status
and entry-point name, the wrappers' host checks before any launch or transfer, what a wrapper sends to the library, and
the restore.py options.  Launches nothing."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import irdu_amd
from irdu_amd import _native, restore
from irdu_amd import kernels as K
from irdu_amd import training as T

INVALID_ARG, SHAPE, UNSUPPORTED = 1, 2, 3
PTR = 0x1000        # never dereferenced: validation fails first
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return _native.load()


def one(src=PTR, h=8, w=12, c=3, dst=PTR + 0x1000, weights=PTR, kh=3, kw=5, boundary=0):
    return (src, h, w, c, dst, weights, kh, kw, boundary, None)


def many(arena=PTR, elems=288, table=PTR, n_img=1, max_h=8, max_w=12, c=3, dst=PTR + 0x1000, weights=PTR, sizes=PTR,
         n_kernels=1, kernel_of=PTR, boundary=0):
    return (arena, elems, table, n_img, max_h, max_w, c, dst, weights, sizes, n_kernels, kernel_of, boundary, None)


def failed(lib, name, args):
    st = getattr(lib, name)(*args)
    return st, lib.grr_last_error() or b""


def test_the_header_declares_what_is_bound():
    text = open(os.path.join(ROOT, "include", "grr.h")).read()
    flat = re.sub(r"\s+", " ", text)
    assert "int grr_u8_blur_supported(int C, int H, int W);" in flat
    assert ("grr_status grr_u8_blur(const uint8_t* src, int H, int W, int C, uint8_t* dst, const int32_t* weights, int kh, "
            "int kw, int boundary, void* stream);") in flat
    assert ("grr_status grr_u8_blur_images(const uint8_t* arena, int64_t elems, const int64_t* table, int n_img, int max_h, "
            "int max_w, int C, uint8_t* dst_arena, const int32_t* weights, const int32_t* sizes, int n_kernels, "
            "const int32_t* kernel_of, int boundary, void* stream);") in flat
    I, L, P = _native.SIGNATURES["grr_u8_blur_supported"][0], _native.c_int64, _native.c_void_p
    assert _native.SIGNATURES["grr_u8_blur_supported"] == [I, I, I]
    assert _native.SIGNATURES["grr_u8_blur"] == [P, I, I, I, P, P, I, I, I, P]
    assert _native.SIGNATURES["grr_u8_blur_images"] == [P, L, P, I, I, I, I, P, P, P, I, P, I, P]
    # the definition is written out above them: the constants, the sum, the flip, the boundaries, the quantiser
    for phrase in ("#define GRR_BLUR_MAX_SIDE 31", "#define GRR_BLUR_ONE 65536",
                   "(32768 + sum_{i<kh, j<kw} W[i][j] * src[b(y + kh/2 - i, H), b(x + kw/2 - j, W), c]) >> 16",
                   "the kernel is flipped", "wrap (0)", "replicate (1)", "reflect (2)", "m = t mod 2(n - 1)",
                   "W = floor(q)", "ties to the lower flat index", "255 * 65536 < 2^24"):
        assert phrase in flat, phrase
    assert "blur_ops.hip" in open(os.path.join(ROOT, "imagerestoration-development-unrolling_amd", "build_native.py")).read()


def test_python_mirror_of_the_shape_query(lib):
    """A call on each side of every bound of grr_u8_blur_supported."""
    big = (1 << 31) - 1
    cases = [(c, 8, 12) for c in (-1, 0, 1, 2, 3, 4, 5)]
    cases += [(3, 0, 12), (3, 8, 0), (1, 1, 1), (4, 1, 1), (3, -1, 4), (1, 4, -1)]
    cases += [(1, 1, big), (1, 2, 1 << 30), (3, 1, 715827882), (3, 1, 715827883), (4, 1 << 15, (1 << 14) - 1),
              (4, 1 << 15, 1 << 14), (2, 1 << 15, (1 << 15) - 1), (2, 1 << 15, 1 << 15), (1, big, big), (4, big, 1)]
    seen = set()
    for case in cases:
        got = bool(lib.grr_u8_blur_supported(*case))
        assert K.blur_ok(*case) == got, case
        seen.add(got)
    assert seen == {True, False}
    assert K.blur_ok(1, 1, big) and not K.blur_ok(1, 2, 1 << 30) and K.blur_ok(3, 1, 715827882)
    assert K.BLUR_BOUNDARIES == ("wrap", "replicate", "reflect") == T.BLUR_BOUNDARIES
    assert K.MAX_BLUR_SIDE == 31 == T.MAX_BLUR_SIDE and K.MAX_BLUR_KERNELS == 16 == T.MAX_BLUR_KERNELS
    assert K.BLUR_ONE == 65536 == T.BLUR_ONE and K.MAX_BLUR_IMAGES == 65535
    rows, cols = K.BLUR_TILE
    assert rows >= 1 and cols % 4 == 0


@pytest.mark.parametrize("name,args", [("grr_u8_blur", one), ("grr_u8_blur_images", many)])
def test_bad_arguments_report_their_status_without_a_launch(lib, name, args):
    label = name.encode()
    nulls = ("src", "dst", "weights") if args is one else ("arena", "dst", "table", "weights", "sizes", "kernel_of")
    for null in nulls:
        st, msg = failed(lib, name, args(**{null: None}))
        assert st == INVALID_ARG and label + b": bad args" in msg, null
    for boundary in (-1, 3, 7):
        st, msg = failed(lib, name, args(boundary=boundary))
        assert st == INVALID_ARG and label + b": the boundary is 0 (wrap), 1 (replicate) or 2 (reflect)" in msg, boundary
    with pytest.raises(_native.GrrError, match=name):
        _native.call(name, *args(boundary=3))


def test_the_single_image_form_checks_the_kernel_the_channels_and_the_size(lib):
    name = "grr_u8_blur"
    for bad in (dict(kh=0), dict(kh=2), dict(kw=4), dict(kh=33), dict(kw=32), dict(kw=-1), dict(kh=30, kw=30)):
        st, msg = failed(lib, name, one(**bad))
        assert st == INVALID_ARG and b"grr_u8_blur: the kernel's sides are odd and in 1..31" in msg, bad
    st, msg = failed(lib, name, one(kh=2, boundary=5))          # the sides before the boundary
    assert st == INVALID_ARG and b"sides" in msg
    st, msg = failed(lib, name, one(c=5))
    assert st == UNSUPPORTED and b"grr_u8_blur: needs 1..4 channels" in msg
    for bad in (dict(h=0), dict(w=-1), dict(c=0)):
        st, msg = failed(lib, name, one(**bad))
        assert st == INVALID_ARG and b"grr_u8_blur: bad args" in msg, bad
    st, msg = failed(lib, name, one(weights=PTR + 2))
    assert st == INVALID_ARG and b"aligned" in msg
    st, msg = failed(lib, name, one(h=1 << 15, w=1 << 14, c=4))
    assert st == UNSUPPORTED and b"grr_u8_blur" in msg and b"2^31" in msg
    assert lib.grr_u8_blur_supported(4, 1 << 15, (1 << 14) - 1) == 1


def test_the_arena_form_checks_its_tables_and_bounds(lib):
    name = "grr_u8_blur_images"
    st, msg = failed(lib, name, many(n_img=65536, elems=1 << 20))
    assert st == UNSUPPORTED and b"65535" in msg and name.encode() in msg
    st, msg = failed(lib, name, many(n_kernels=17))
    assert st == UNSUPPORTED and b"at most 16 kernels" in msg and name.encode() in msg
    st, msg = failed(lib, name, many(n_img=289))                       # more images than pixels
    assert st == UNSUPPORTED and name.encode() in msg
    st, msg = failed(lib, name, many(c=5))
    assert st == UNSUPPORTED and b"1..4 channels" in msg
    for bad in (dict(table=PTR + 4), dict(weights=PTR + 2), dict(sizes=PTR + 1), dict(kernel_of=PTR + 2)):
        st, msg = failed(lib, name, many(**bad))
        assert st == INVALID_ARG and b"aligned" in msg, bad
    st, msg = failed(lib, name, many(max_h=1 << 15, max_w=21846))
    assert st == UNSUPPORTED and b"2^31" in msg
    for bad in (dict(elems=0), dict(n_img=0), dict(n_img=-3), dict(max_h=0), dict(max_w=-1), dict(c=0), dict(n_kernels=0)):
        st, msg = failed(lib, name, many(**bad))
        assert st == INVALID_ARG and b"grr_u8_blur_images: bad args" in msg, bad


def pack_of(host_table=((0, 8, 12), (288, 5, 7)), c=3, dtype=torch.uint8):
    elems = max(off + h * w * c for off, h, w in host_table)
    return SimpleNamespace(arena=torch.zeros(elems, dtype=dtype), host_table=tuple(host_table), c=c, kinds=("numpy",) * 2,
                           table=torch.tensor(host_table, dtype=torch.int64).reshape(-1, 3))


def no_launch(*a, **k):
    raise AssertionError("a kernel was launched")


BOX = np.full((3, 3), 7281, np.int32) + (np.arange(9).reshape(3, 3) < 7)        # sums to 65536
BAD_TABLES = [np.ones((3, 3), np.int32), BOX - (np.arange(9).reshape(3, 3) == 0) * 7283 + (np.arange(9).reshape(3, 3) == 1) * 7283,
              np.full((2, 2), 16384, np.int32), np.full((1, 33), 0, np.int32), BOX.astype(np.float32), BOX.ravel(),
              np.zeros((0, 3), np.int32), "box:3", None]


def test_wrappers_refuse_before_any_launch_or_transfer(monkeypatch):
    monkeypatch.setattr(K, "_launch", no_launch)
    monkeypatch.setattr(restore, "_to_device", no_launch)
    assert int(BOX.sum()) == 65536 and BAD_TABLES[1].min() < 0 and int(BAD_TABLES[1].sum()) == 65536
    img = torch.zeros((8, 12, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="GPU"):
        K.u8_blur(img, BOX)
    with pytest.raises(RuntimeError, match="GPU"):
        K.u8_blur(img[:, :, 0], T.box_kernel(3), 2)
    with pytest.raises(RuntimeError, match="GPU"):
        K.u8_blur_images(pack_of(), [BOX], 0)
    for bad in BAD_TABLES:
        with pytest.raises(ValueError, match="u8_blur: a blur kernel"):
            K.u8_blur(img, bad)
        with pytest.raises(ValueError, match="u8_blur_images: a blur kernel"):
            K.u8_blur_images(pack_of(), [BOX, bad], [0, 1])
    for bad in ("circular", "WRAP", 3, -1, True, 1.0, None):
        with pytest.raises(ValueError, match="u8_blur: the boundary"):
            K.u8_blur(img, BOX, bad)
        with pytest.raises(ValueError, match="u8_blur_images: the boundary"):
            K.u8_blur_images(pack_of(), BOX, 0, bad)
        with pytest.raises(ValueError, match="blur_u8: the boundary"):
            irdu_amd.blur_u8(np.zeros((8, 12, 3), np.uint8), "box:3", bad)
        with pytest.raises(ValueError, match="evaluate_deblur: the boundary"):
            irdu_amd.evaluate_deblur(lambda x: x, [np.zeros((16, 16, 3), np.uint8)], "box:3", bad)
    assert [K._check_boundary("t", b) for b in K.BLUR_BOUNDARIES] == [0, 1, 2] == [K._check_boundary("t", k) for k in range(3)]
    assert K._check_boundary("t", np.int64(1)) == 1
    for bad in ("gauss:3:1", "box:4", 5, None):
        with pytest.raises(ValueError, match="blur_u8: "):
            irdu_amd.blur_u8(np.zeros((8, 12, 3), np.uint8), bad)
    with pytest.raises(ValueError, match="uint8"):
        K.u8_blur(img.float(), BOX)
    with pytest.raises(ValueError, match="blur_u8: expected a uint8"):
        irdu_amd.blur_u8(np.zeros((8, 12, 3), np.float32), "box:3")
    with pytest.raises(ValueError, match="H x W x C"):
        K.u8_blur(img[0, 0], BOX)
    with pytest.raises(ValueError, match="C <= 4"):
        K.u8_blur(torch.zeros((8, 12, 5), dtype=torch.uint8), BOX)
    with pytest.raises(ValueError, match="u8_blur_images: takes 1..16 kernels, got 17"):
        K.u8_blur_images(pack_of(), [BOX] * 17, 0)
    with pytest.raises(ValueError, match="u8_blur_images: takes 1..16 kernels, got 0"):
        K.u8_blur_images(pack_of(), [], 0)
    monkeypatch.setattr(K, "_check_placed", lambda *a: None)
    with pytest.raises(ValueError, match="uint8"):
        K.u8_blur_images(pack_of(dtype=torch.float32), BOX, 0)
    with pytest.raises(ValueError, match="1 kernel indices for 2 images"):
        K.u8_blur_images(pack_of(), BOX, [0])
    for bad in (1, -1, True, 0.0, None):
        with pytest.raises(ValueError, match="u8_blur_images: a kernel index is an integer of 0..0"):
            K.u8_blur_images(pack_of(), BOX, [0, bad])
    with pytest.raises(ValueError, match=r"kernel-index tensor is int32 \[2\]"):
        K.u8_blur_images(pack_of(), BOX, torch.tensor([0, 0], dtype=torch.int64))


def test_evaluate_deblur_checks_before_any_launch(monkeypatch):
    monkeypatch.setattr(K, "_launch", no_launch)
    monkeypatch.setattr(restore, "_to_device", no_launch)
    assert irdu_amd.blur_u8 is restore.blur_u8 and irdu_amd.evaluate_deblur is restore.evaluate_deblur
    for name in ("GaussianMotionDeblurring", "BlurKernel", "blur_degrade_u8", "box_kernel", "gaussian_kernel", "motion_kernel",
                 "parse_blur_spec", "quantise_blur_kernel"):
        assert getattr(irdu_amd, name) is getattr(T, name)
    ev, model, z = restore.evaluate_deblur, (lambda x: x), np.zeros((16, 16, 3), np.uint8)
    # the shared arguments, then the spec, the boundary, the noise, the seed, the shave, then the pictures
    with pytest.raises(ValueError, match="evaluate_deblur: metrics"):
        ev(model, [z], "gauss:3:1", metrics=("mse",))
    with pytest.raises(TypeError, match="evaluate_deblur: unexpected arguments"):
        ev(model, [z], "gauss:3:1", scale=2)
    with pytest.raises(ValueError, match="evaluate_deblur: parse_blur_spec"):
        ev(model, [z], "gauss:3:1", "circular")
    with pytest.raises(ValueError, match="evaluate_deblur: the boundary"):
        ev(model, [z], "box:3", "circular", noise_sigma=-1)
    for bad in (-1, float("nan"), float("inf"), True, "2", None):
        with pytest.raises(ValueError, match="evaluate_deblur: noise_sigma"):
            ev(model, [z], "box:3", noise_sigma=bad, seed=-1)
    for bad in (-1, 2 ** 32, 1.0, True, None):
        with pytest.raises(ValueError, match="evaluate_deblur: seed"):
            ev(model, [z], "box:3", seed=bad, shave=-1)
    for bad in (-1, True, 1.0):
        with pytest.raises(ValueError, match="evaluate_deblur: shave"):
            ev(model, [], "box:3", shave=bad)
    with pytest.raises(ValueError, match="evaluate_deblur: no images"):
        ev(model, [], "box:3")
    with pytest.raises(ValueError, match="evaluate_deblur: image 1 is torch.float32; the blur is defined on uint8"):
        ev(model, [z, z.astype(np.float32)], "box:3")
    with pytest.raises(ValueError, match="evaluate_deblur: image 1 is .*nothing is left after a shave of 8"):
        ev(model, [np.zeros((40, 40, 3), np.uint8), z], "box:3", shave=8)
    with pytest.raises(ValueError, match="evaluate_deblur: image 0 after the shave .*at least 11"):
        ev(model, [z], "box:3", shave=3)                                # 10 x 10 is left: too small for SSIM
    with pytest.raises(ValueError, match="evaluate_deblur: image 0 after the shave .*Y-channel"):
        ev(model, [z[:, :, :1]], "box:3", metrics=("psnr_y",))
    with pytest.raises(ValueError, match="validate_deblur: metric"):
        T.validate_deblur(None, [], "box:3", metric="psnrb")
    assert T.VAL_DEBLUR_METRICS == ("psnr", "psnr_y", "ssim")


def test_wrapper_launch_arguments(monkeypatch):
    """What reaches the library: both arenas under one table, the bounds, the kernels' slots, read + written bytes."""
    sent = []
    monkeypatch.setattr(K, "_check_placed", lambda *a: None)
    monkeypatch.setattr(K, "_stream", lambda dev: None)
    monkeypatch.setattr(K, "_launch", lambda kind, nbytes, name, *a, **k: sent.append((kind, nbytes, name, a)))
    pack = pack_of()
    out = K.u8_blur_images(pack, [BOX, T.motion_kernel(5, 0)], [1, 0], "reflect")
    assert out.table is pack.table and out.host_table == pack.host_table and out.c == 3 and out.kinds == pack.kinds
    assert out.arena.numel() == pack.arena.numel() and out.arena is not pack.arena and out.arena.dtype == torch.uint8
    kind, nbytes, name, a = sent[0]
    assert (kind, name) == ("u8_blur_images", "grr_u8_blur_images") and nbytes == 2 * (288 + 105) and len(sent) == 1
    assert a[:8] == (pack.arena.data_ptr(), 393, pack.table.data_ptr(), 2, 8, 12, 3, out.arena.data_ptr())
    assert a[10] == 2 and a[12] == 2 and len(a) == 14
    # the chunking: one launch per MAX_BLUR_IMAGES images, the table and the kernel list advanced alike
    monkeypatch.setattr(K, "MAX_BLUR_IMAGES", 1)
    sent.clear()
    K.u8_blur_images(pack, BOX, 0)
    assert len(sent) == 2 and [s[3][3] for s in sent] == [1, 1]
    assert sent[1][3][2] - sent[0][3][2] == 24 and sent[1][3][11] - sent[0][3][11] == 4
    assert [s[3][4:6] for s in sent] == [(8, 12), (5, 7)] and [s[1] for s in sent] == [2 * 288, 2 * 105]
    monkeypatch.setattr(K, "_check_image", lambda name, t: tuple(t.shape))
    for img, c in ((torch.zeros((8, 12, 1), dtype=torch.uint8), 1), (torch.zeros((8, 12), dtype=torch.uint8), 1),
                   (torch.zeros((8, 12, 4), dtype=torch.uint8), 4)):
        sent.clear()
        res = K.u8_blur(img, T.motion_kernel(5, 0), "replicate")
        assert res.shape == img.shape and res.dtype == torch.uint8
        assert sent[0][2] == "grr_u8_blur" and sent[0][1] == 2 * 96 * c
        assert sent[0][3][:4] == (img.data_ptr(), 8, 12, c) and sent[0][3][6:9] == (5, 5, 1)
    view = torch.zeros((8, 24, 3), dtype=torch.uint8)[:, ::2]          # not contiguous: copied first
    sent.clear()
    K.u8_blur(view, BOX)
    assert sent[0][3][0] != view.data_ptr() and sent[0][3][6:9] == (3, 3, 0)


def cli():
    from tests.test_restore_ref import _cli
    return _cli()


def test_restore_command_options():
    command = cli()
    base = ["-yaml_path", "conf.yaml", "--input", "in", "--output", "out"]
    args = command.parse_args(base + ["--blur", "gaussian:25:1.6", "--ssim", "--y-channel", "--batch-images", "--self-ensemble"])
    assert args.blur == "gaussian:25:1.6" and args.scored and args.shave == 0 and args.blur_boundary == "wrap"
    assert args.blur_noise == 0.0 and args.ensemble == 8 and args.bayer is None
    args = command.parse_args(base + ["--blur", "motion:15:30", "--shave", "4", "--blur-boundary", "reflect", "--blur-noise",
                                      "2.55", "--seed", "7"])
    assert args.shave == 4 and args.blur_boundary == "reflect" and args.blur_noise == 2.55 and args.seed == 7
    plain = command.parse_args(base + ["--sigma", "25"])
    assert plain.blur is None and plain.blur_boundary == "wrap" and plain.blur_noise == 0.0 and plain.shave is None
    for bad in (["--blur", "box:3", "--sigma", "5"], ["--blur", "box:3", "--jpeg-quality", "10"], ["--blur", "box:3", "--bayer", "rggb"],
                ["--blur", "box:3", "--scale", "2"], ["--blur", "box:3", "--reference", "refs"], ["--blur", "box:3", "--raw", "rggb"],
                ["--blur", "box:3", "--upscale", "2"], ["--blur-boundary", "wrap"], ["--sigma", "5", "--blur-noise", "1"],
                ["--blur", "box:3", "--blur-boundary", "circular"], ["--blur", "box:3", "--blur-noise", "-1"],
                ["--blur", "box:3", "--blur-noise", "nan"], ["--blur", "box:3", "--psnrb"], ["--blur", "box:3", "--shave", "-1"],
                ["--blur", "box:3", "--demosaic-fill", "zero"], ["--blur", "box:3", "--jpeg-subsampling", "420"]):
        with pytest.raises(SystemExit):
            command.parse_args(base + bad)
