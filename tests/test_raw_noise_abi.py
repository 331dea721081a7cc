"""CPU-only checks of grr_patch_raw_batch / grr_u8_raw_noise_demosaic (csrc/rawnoise_ops.hip) and what is built on
them: the header's declarations against the bindings, the Python mirrors of the shape queries on both sides of every
bound, every refusal with its status and entry-point name, the wrappers' host checks before any transfer, the restore.py
options, the ``raw_noise`` validation row and the order in which restore.evaluate_jdd refuses.  Launches nothing."""
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

INVALID_ARG, UNSUPPORTED = 1, 3
PTR = 0x1000        # never dereferenced: validation fails first
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return _native.load()


def many(arena=PTR, elems=288, img_table=PTR, n_img=1, patterns=PTR, table=PTR, ids=PTR, noise=PTR, n=2, seed=7, ph=16,
         pw=16, fill=2, bits=16, clip=1, target=PTR, inp=PTR + 0x10000):
    return (arena, elems, img_table, n_img, patterns, table, ids, noise, n, seed, ph, pw, fill, bits, clip, target, inp, None)


def one(src=PTR, h=8, w=12, dst=PTR + 0x1000, pattern=0, fill=2, a=0.01, b=0.0004, bits=16, clip=1, seed=7, sample_id=0):
    return (src, h, w, dst, pattern, fill, a, b, bits, clip, seed, sample_id, None)


def failed(lib, name, args):
    st = getattr(lib, name)(*args)
    return st, lib.grr_last_error() or b""


def test_the_header_declares_what_is_bound():
    flat = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "grr.h")).read())
    assert "int grr_patch_raw_batch_supported(int n_img, int64_t arena_elems, int n, int ph, int pw);" in flat
    assert ("grr_status grr_patch_raw_batch(const uint8_t* arena, int64_t arena_elems, const int64_t* img_table, int n_img, "
            "const int32_t* patterns, const int32_t* table, const int64_t* sample_ids, const float* noise /* [n, 2] or NULL "
            "*/, int n, uint64_t seed, int ph, int pw, int fill, int bits, int clip, float* target, float* input, "
            "void* stream);") in flat
    assert "int grr_u8_raw_noise_demosaic_supported(int H, int W);" in flat
    assert ("grr_status grr_u8_raw_noise_demosaic(const uint8_t* src, int H, int W, float* dst /* float32 H x W x 3, HWC */, "
            "int pattern, int fill, float a, float b, int bits, int clip, uint64_t seed, int64_t sample_id, "
            "void* stream);") in flat
    I, L, P, F, U = _native.I, _native.L, _native.P, _native.Fl, _native.ctypes.c_uint64
    assert _native.SIGNATURES["grr_patch_raw_batch_supported"] == [I, L, I, I, I]
    assert _native.SIGNATURES["grr_patch_raw_batch"] == [P, L, P, I, P, P, P, P, I, U, I, I, I, I, I, P, P, P]
    assert _native.SIGNATURES["grr_u8_raw_noise_demosaic_supported"] == [I, I]
    assert _native.SIGNATURES["grr_u8_raw_noise_demosaic"] == [P, I, I, P, I, I, F, F, I, I, U, L, P]
    # the definition is written out above them
    for phrase in ("(ph + 4) x (pw + 4)", "Y = row + wy - 2, X = col + wx - 2", "var = a x + b",
                   "t = x + sqrt(var) z_e", "e = wy (pw + 4) + wx", "block e / 4, lane e % 4", "ties to even",
                   "clamped to +-2^24", "a NaN gives 0", "Where var == 0 no random number is computed",
                   "(float)((double)s / (16.0 full))", "|s| <= 40 * 2^24", "mode & 5", "noise == NULL means a = b = 0",
                   "No atomics"):
        assert phrase in flat, phrase
    build = open(os.path.join(ROOT, "imagerestoration-development-unrolling_amd", "build_native.py")).read()
    assert '"rawnoise_ops.hip"' in build
    csrc = os.path.join(ROOT, "imagerestoration-development-unrolling_amd", "csrc")
    moved = ("void philox4x32_10(", "void box_muller(", "struct NoiseKey", "void normals4(", "double normal_at(")
    device_h, image_ops = open(os.path.join(csrc, "grr_device.h")).read(), open(os.path.join(csrc, "image_ops.hip")).read()
    assert all(name in device_h and name not in image_ops for name in moved)


def test_python_mirrors_of_the_shape_queries(lib):
    """A call on each side of every bound of the two queries."""
    big = (1 << 31) - 1
    cases = [(1, 288, 2, 16, 16), (0, 288, 2, 16, 16), (-1, 288, 2, 16, 16), (289, 288, 2, 16, 16), (1, 2, 1, 1, 1),
             (1, 3, 1, 1, 1), (1, 0, 1, 1, 1), (1, 1 << 62, 1, 1, 1), (1, (1 << 62) - 1, 1, 1, 1),
             (1, 288, 0, 16, 16), (1, 288, 2, 0, 16), (1, 288, 2, 16, 0), (1, 288, -2, 16, 16),
             (1, 288, 1, 1, 715827882), (1, 288, 1, 1, 715827883), (1, 288, 715827882, 1, 1), (1, 288, 715827883, 1, 1),
             (1, 288, 1, 1 << 15, 21845), (1, 288, 1, 1 << 15, 21846), (1, 288, 2, 1 << 14, 21845), (1, 288, 2, 1 << 14, 21846),
             (1, 288, 1, 1, 429496725), (1, 288, 1, 1, 429496726), (1, 288, 1, 429496725, 1), (1, 288, 1, 429496726, 1),
             (1, 288, big, big, big), (1, 288, 1, big, 1), (1, 288, 1, 1, big)]
    seen = set()
    for case in cases:
        got = bool(lib.grr_patch_raw_batch_supported(*case))
        assert K.patch_raw_batch_ok(*case) == got, case
        seen.add(got)
    assert seen == {True, False}
    # the window (H + 4)(W + 4) < 2^31 binds on thin pictures (5 x 429496730 = 2^31 + 2), 3 H W < 2^31 on the others
    shapes = [(8, 12), (0, 12), (8, 0), (-1, 4), (1, 1), (1, 429496725), (1, 429496726), (429496725, 1), (429496726, 1),
              (1, 715827882), (715827882, 1),
              (1 << 15, 21845), (1 << 15, 21846), (big, big), (1, big), (46340, 15446), (26754, 26754), (26755, 26755)]
    seen = set()
    for h, w in shapes:
        got = bool(lib.grr_u8_raw_noise_demosaic_supported(h, w))
        assert K.raw_noise_demosaic_ok(h, w) == got, (h, w)
        seen.add(got)
    assert seen == {True, False}
    assert K.raw_noise_demosaic_ok(1, 429496725) and not K.raw_noise_demosaic_ok(1, 429496726)
    assert K.raw_noise_demosaic_ok(1 << 15, 21845) and not K.raw_noise_demosaic_ok(1 << 15, 21846)
    rows, cols = K.RAW_NOISE_TILE
    assert rows >= 1 and cols % 4 == 0 and K.RAW_NOISE_BITS == (8, 16) == T.RAW_NOISE_BITS


@pytest.mark.parametrize("name,args", [("grr_patch_raw_batch", many), ("grr_u8_raw_noise_demosaic", one)])
def test_bad_arguments_report_their_status_without_a_launch(lib, name, args):
    label = name.encode()
    nulls = ("src", "dst") if args is one else ("arena", "img_table", "patterns", "table", "ids", "target", "inp")
    for null in nulls:
        st, msg = failed(lib, name, args(**{null: None}))
        assert st == INVALID_ARG and label + b": bad args" in msg, null
    for fill in (-1, 3, 7):
        st, msg = failed(lib, name, args(fill=fill))
        assert st == INVALID_ARG and label + b": the fill is 0 (zero), 1 (bilinear) or 2 (malvar)" in msg, fill
    for bits in (7, 17, 0, -8, 32):
        st, msg = failed(lib, name, args(bits=bits))
        assert st == INVALID_ARG and label + b": bits is 8..16" in msg, bits
    for clip in (-1, 2):
        st, msg = failed(lib, name, args(clip=clip))
        assert st == INVALID_ARG and label + b": clip is 0 or 1" in msg, clip
    # fill before bits before clip
    st, msg = failed(lib, name, args(fill=3, bits=7, clip=2))
    assert st == INVALID_ARG and b"the fill" in msg
    st, msg = failed(lib, name, args(bits=7, clip=2))
    assert st == INVALID_ARG and b"bits is" in msg
    with pytest.raises(_native.GrrError, match=name):
        _native.call(name, *args(fill=3))


def test_the_patch_form_checks_its_tables_and_bounds(lib):
    name = "grr_patch_raw_batch"
    for bad in (dict(elems=0), dict(n_img=0), dict(n=0), dict(n=-1), dict(ph=0), dict(pw=-3)):
        st, msg = failed(lib, name, many(**bad))
        assert st == INVALID_ARG and b"grr_patch_raw_batch: bad args" in msg, bad
    st, msg = failed(lib, name, many(n_img=289))                       # more images than elements
    assert st == UNSUPPORTED and name.encode() in msg and b"arena elements" in msg
    st, msg = failed(lib, name, many(elems=2))                         # fewer elements than one pixel has
    assert st == UNSUPPORTED and name.encode() in msg
    for bad in (dict(n=715827883, ph=1, pw=1), dict(n=1, ph=1 << 15, pw=21846), dict(n=(1 << 31) - 1, ph=(1 << 31) - 1, pw=4)):
        st, msg = failed(lib, name, many(**bad))
        assert st == UNSUPPORTED and b"grr_patch_raw_batch: patch batch 3 n ph pw" in msg and b"2^31" in msg, bad
    for bad in (dict(table=PTR + 2), dict(patterns=PTR + 1), dict(noise=PTR + 2), dict(target=PTR + 2), dict(inp=PTR + 1)):
        st, msg = failed(lib, name, many(**bad))
        assert st == INVALID_ARG and b"4-byte aligned" in msg, bad
    for bad in (dict(img_table=PTR + 4), dict(ids=PTR + 4)):
        st, msg = failed(lib, name, many(**bad))
        assert st == INVALID_ARG and b"8-byte aligned" in msg, bad


def test_the_one_image_form_checks_the_pattern_the_noise_and_the_size(lib):
    name = "grr_u8_raw_noise_demosaic"
    for pattern in (-1, 4, 100):
        st, msg = failed(lib, name, one(pattern=pattern))
        assert st == INVALID_ARG and b"grr_u8_raw_noise_demosaic: the pattern is 0 (rggb)" in msg, pattern
    for bad in (dict(h=0), dict(w=-1)):
        st, msg = failed(lib, name, one(**bad))
        assert st == INVALID_ARG and b"grr_u8_raw_noise_demosaic: bad args" in msg, bad
    for bad in (dict(a=-0.5), dict(a=1.5), dict(b=-1e-3), dict(b=2.0), dict(a=float("nan")), dict(b=float("inf"))):
        st, msg = failed(lib, name, one(**bad))
        assert st == INVALID_ARG and b"grr_u8_raw_noise_demosaic: the noise pair (a, b) lies in [0, 1]" in msg, bad
    st, msg = failed(lib, name, one(h=1 << 15, w=21846))
    assert st == UNSUPPORTED and b"grr_u8_raw_noise_demosaic" in msg and b"2^31" in msg
    st, msg = failed(lib, name, one(dst=PTR + 2))
    assert st == INVALID_ARG and b"4-byte aligned" in msg
    st, msg = failed(lib, name, one(pattern=4, fill=3))                # the pattern before the fill
    assert b"the pattern" in msg


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
    u8 = np.zeros((8, 12, 3), np.uint8)
    with pytest.raises(RuntimeError, match="GPU"):
        K.u8_raw_noise_demosaic(img, "rggb")
    with pytest.raises(RuntimeError, match="GPU"):
        K.patch_raw_source(pack_of(), "rggb")
    for bad in ("rgbg", 4, -1, True, None):
        with pytest.raises(ValueError, match="u8_raw_noise_demosaic: the pattern"):
            K.u8_raw_noise_demosaic(img, bad)
        with pytest.raises(ValueError, match="patch_raw_batch: the pattern"):
            K.patch_raw_source(pack_of(), ["rggb", bad])
        with pytest.raises(ValueError, match="raw_noise_demosaic_u8: the pattern"):
            irdu_amd.raw_noise_demosaic_u8(u8, bad)
    for bad in ("linear", 3, False):
        with pytest.raises(ValueError, match="u8_raw_noise_demosaic: the fill"):
            K.u8_raw_noise_demosaic(img, 0, bad)
        with pytest.raises(ValueError, match="raw_noise_demosaic_u8: the fill"):
            irdu_amd.raw_noise_demosaic_u8(u8, 0, bad)
    for bad in (7, 17, 12.0, True, None):
        with pytest.raises(ValueError, match="u8_raw_noise_demosaic: bits"):
            K.u8_raw_noise_demosaic(img, 0, bits=bad)
        with pytest.raises(ValueError, match="raw_noise_demosaic_u8: bits"):
            irdu_amd.raw_noise_demosaic_u8(u8, bits=bad)
    for bad in (-0.1, 1.5, float("nan"), "0.1", True):
        with pytest.raises(ValueError, match="u8_raw_noise_demosaic: a is"):
            K.u8_raw_noise_demosaic(img, 0, a=bad)
        with pytest.raises(ValueError, match="u8_raw_noise_demosaic: b is"):
            K.u8_raw_noise_demosaic(img, 0, b=bad)
        with pytest.raises(ValueError, match="raw_noise_demosaic_u8: shot is"):
            irdu_amd.raw_noise_demosaic_u8(u8, shot=bad)
    for bad in (-1, 256.0, float("inf"), None):
        with pytest.raises(ValueError, match="raw_noise_demosaic_u8: read is"):
            irdu_amd.raw_noise_demosaic_u8(u8, read=bad)
    for bad in (0, 1, "yes", None):
        with pytest.raises(ValueError, match="clip is True or False"):
            K.u8_raw_noise_demosaic(img, 0, clip=bad)
        with pytest.raises(ValueError, match="raw_noise_demosaic_u8: clip"):
            irdu_amd.raw_noise_demosaic_u8(u8, clip=bad)
    for bad in (-1, 1 << 64, 2.0, True):
        with pytest.raises(ValueError, match="seed"):
            K.u8_raw_noise_demosaic(img, 0, seed=bad)
        with pytest.raises(ValueError, match="raw_noise_demosaic_u8: seed"):
            irdu_amd.raw_noise_demosaic_u8(u8, seed=bad)
    for bad in (1 << 63, -(1 << 63) - 1, 0.0):
        with pytest.raises(ValueError, match="sample_id"):
            K.u8_raw_noise_demosaic(img, 0, sample_id=bad)
        with pytest.raises(ValueError, match="raw_noise_demosaic_u8: sample_id"):
            irdu_amd.raw_noise_demosaic_u8(u8, sample_id=bad)
    for c in (1, 2, 4):
        with pytest.raises(ValueError, match="u8_raw_noise_demosaic: needs 3 channels"):
            K.u8_raw_noise_demosaic(torch.zeros((8, 12, c), dtype=torch.uint8), 0)
        with pytest.raises(ValueError, match="raw_noise_demosaic_u8: needs 3 channels"):
            irdu_amd.raw_noise_demosaic_u8(np.zeros((8, 12, c), np.uint8))
    with pytest.raises(ValueError, match="uint8"):
        K.u8_raw_noise_demosaic(img.float(), 0)
    with pytest.raises(ValueError, match="raw_noise_demosaic_u8: expected a uint8"):
        irdu_amd.raw_noise_demosaic_u8(u8.astype(np.float32))
    # the noise pair: a = float32(shot), b = float32((read / 255)^2)
    assert K.raw_noise_pair("t", 0.01, 5.0) == (float(np.float32(0.01)), float(np.float32((5.0 / 255.0) ** 2)))
    assert K.raw_noise_pair("t", 0, 0) == (0.0, 0.0) and K.raw_noise_pair("t", 1, 255) == (1.0, 1.0)
    # the pack and the pattern list
    monkeypatch.setattr(K, "_check_placed", lambda *a: None)
    with pytest.raises(ValueError, match="patch_raw_batch: the arena must be uint8"):
        K.patch_raw_source(pack_of(dtype=torch.float32), 0)
    with pytest.raises(ValueError, match="made from R, G, B pictures, got 1 channel"):
        K.patch_raw_source(pack_of(((0, 8, 12), (96, 5, 7)), c=1), 0)
    with pytest.raises(ValueError, match="1 patterns for 2 images"):
        K.patch_raw_source(pack_of(), ["rggb"])
    src = K.patch_raw_source(pack_of(), ["grbg", 3])
    assert src.host_patterns == (1, 3) and src.patterns.dtype == torch.int32 and src.n_img == 2
    assert src.hw.tolist() == [[8, 12], [5, 7]]
    # the batch: what patch_batch refuses, and the noise table
    rows, ids, noise = [(0, 1, 2, 0), (1, 4, 6, 5)], [5, 6], [(0.01, 0.0), (0.0, 0.001)]
    with pytest.raises(ValueError, match="patch_raw_batch: source is what patch_raw_source returns"):
        K.patch_raw_batch(pack_of(), rows, ids, noise, 7, 16, 16)
    for bad, message in ((dict(fill="linear"), "the fill"), (dict(bits=20), "bits"), (dict(clip=1), "clip is True or False")):
        with pytest.raises(ValueError, match="patch_raw_batch: " + message):
            K.patch_raw_batch(src, rows, ids, noise, 7, 16, 16, **bad)
    for bad in ([(0.01, 0.0)], [(0.01, 0.0, 0.0)] * 2, [(-0.01, 0.0), (0, 0)], [(0.0, 1.5), (0, 0)], [(np.nan, 0.0), (0, 0)]):
        with pytest.raises(ValueError, match=r"patch_raw_batch: noise is \[n, 2\] rows \(a, b\) of \[0, 1\]"):
            K.patch_raw_batch(src, rows, ids, bad, 7, 16, 16)
    with pytest.raises(ValueError, match="image indices"):
        K.patch_raw_batch(src, [(2, 0, 0, 0)], [1], None, 7, 16, 16)
    with pytest.raises(ValueError, match="inside the row's image"):
        K.patch_raw_batch(src, [(1, 5, 0, 0)], [1], None, 7, 16, 16)
    with pytest.raises(ValueError, match="modes must lie in 0..7"):
        K.patch_raw_batch(src, [(0, 0, 0, 8)], [1], None, 7, 16, 16)
    with pytest.raises(ValueError, match="need a square patch"):
        K.patch_raw_batch(src, [(0, 0, 0, 2)], [1], None, 7, 16, 32)
    with pytest.raises(ValueError, match="seed must fit 64 bits"):
        K.patch_raw_batch(src, rows, ids, noise, -1, 16, 16)
    with pytest.raises(ValueError, match="must have 1..2\\^31-1 elements"):
        K.patch_raw_batch(src, rows, ids, noise, 7, 1 << 15, 1 << 15)
    with pytest.raises(ValueError, match=r"patch_raw_batch: the window \(1 \+ 4\) x \(429496726 \+ 4\) must have fewer than 2\^31"):
        K.patch_raw_batch(src, [(0, 0, 0, 0)], [1], None, 7, 1, 429496726)


def test_wrapper_launch_arguments(monkeypatch):
    """What reaches the library: the arena and its table, the pattern list, the three tables, the call-wide codes."""
    sent = []
    monkeypatch.setattr(K, "_check_placed", lambda *a: None)
    monkeypatch.setattr(K, "_stream", lambda dev: None)
    monkeypatch.setattr(K, "_launch", lambda kind, nbytes, name, *a, **k: sent.append((kind, nbytes, name, a)))
    pack = pack_of()
    src = K.patch_raw_source(pack, ["grbg", "bggr"])
    rows, ids = [(0, 1, 2, 0), (1, 4, 6, 5), (0, 7, 11, 3)], [5, 6, (3 << 32) | 1]
    target, inp = K.patch_raw_batch(src, rows, ids, [(0.01, 0.0), (0.0, 0.001), (0, 0)], 9, 16, 16, "bilinear", 12, False)
    assert tuple(target.shape) == tuple(inp.shape) == (3, 3, 16, 16) and target.dtype == inp.dtype == torch.float32
    kind, nbytes, name, a = sent[0]
    assert (kind, name) == ("patch_raw_batch", "grr_patch_raw_batch") and nbytes == 2 * 3 * 3 * 256 * 4 + 3 * 400
    assert a[:5] == (pack.arena.data_ptr(), 393, pack.table.data_ptr(), 2, src.patterns.data_ptr())
    assert a[7] is not None and a[8:15] == (3, 9, 16, 16, 1, 12, 0) and a[15:17] == (target.data_ptr(), inp.data_ptr())
    sent.clear()
    K.patch_raw_batch(src, [r[:3] + (r[3] & 5,) for r in rows], ids, None, 9, 16, 32)
    assert sent[0][3][7] is None and sent[0][3][8:15] == (3, 9, 16, 32, 2, 16, 1)
    monkeypatch.setattr(K, "_check_image", lambda name, t: tuple(t.shape))
    img = torch.zeros((8, 12, 3), dtype=torch.uint8)
    sent.clear()
    out = K.u8_raw_noise_demosaic(img, "bggr", "zero", 0.25, 0.5, 10, False, 11, -2)
    assert tuple(out.shape) == (8, 12, 3) and out.dtype == torch.float32
    assert sent[0][2] == "grr_u8_raw_noise_demosaic" and sent[0][1] == 288 + 4 * 288
    assert sent[0][3][:12] == (img.data_ptr(), 8, 12, out.data_ptr(), 3, 0, 0.25, 0.5, 10, 0, 11, -2)


def cli():
    from tests.test_restore_ref import _cli
    return _cli()


def test_restore_command_options():
    command = cli()
    base = ["-yaml_path", "conf.yaml", "--input", "in", "--output", "out"]
    args = command.parse_args(base + ["--bayer", "grbg", "--raw-noise", "0.01,5", "--ssim"])
    assert args.bayer == "grbg" and args.raw_noise == (0.01, 5.0) and args.scored and args.shave == 0
    assert args.raw_bits == 16 and not args.raw_no_clip and args.raw_seed == 2204 and args.demosaic_fill == "malvar"
    args = command.parse_args(base + ["--bayer", "rggb", "--raw-noise", "0,0", "--raw-bits", "12", "--raw-no-clip",
                                      "--raw-seed", "5", "--shave", "4", "--demosaic-fill", "bilinear", "--batch-images"])
    assert args.raw_noise == (0.0, 0.0) and args.raw_bits == 12 and args.raw_no_clip and args.raw_seed == 5 and args.shave == 4
    plain = command.parse_args(base + ["--bayer", "rggb"])            # --bayer alone stays evaluate_demosaic
    assert plain.raw_noise is None and plain.bayer == "rggb"
    for bad in (["--raw-noise", "0.01,5"], ["--raw", "rggb", "--raw-noise", "0.01,5"], ["--sigma", "5", "--raw-noise", "0,0"],
                ["--bayer", "rggb", "--raw-noise", "0.01"], ["--bayer", "rggb", "--raw-noise", "a,b"],
                ["--bayer", "rggb", "--raw-noise", "0.01,5,1"], ["--bayer", "rggb", "--raw-noise", "1.5,5"],
                ["--bayer", "rggb", "--raw-noise", "0.01,256"], ["--bayer", "rggb", "--raw-noise", "-0.1,5"],
                ["--bayer", "rggb", "--raw-bits", "12"], ["--bayer", "rggb", "--raw-no-clip"],
                ["--bayer", "rggb", "--raw-seed", "3"], ["--bayer", "rggb", "--raw-noise", "0,0", "--raw-bits", "7"],
                ["--bayer", "rggb", "--raw-noise", "0,0", "--raw-bits", "17"],
                ["--bayer", "rggb", "--raw-noise", "0,0", "--raw-seed", "-1"],
                ["--bayer", "rggb", "--raw-noise", "0,0", "--psnrb"]):
        with pytest.raises(SystemExit):
            command.parse_args(base + bad)
    p = restore._jdd_protocol("--bayer", "grbg", "malvar", 0.01, 5.0, 12, False, 2204, 4)
    assert p.label == "bayer grbg malvar raw noise shot 0.01 read 5 12 bits unclipped shave 4" and p.shave == 4
    assert restore._jdd_protocol("--bayer", 0, 1, 0, 0, 16, True, 1, 0).label == \
        "bayer rggb bilinear raw noise shot 0 read 0 16 bits shave 0"


@pytest.fixture(scope="module")
def clean_set(tmp_path_factory):
    d = tmp_path_factory.mktemp("val")
    (d / "clean.csv").write_text("index,path\n0,a.png\n")
    (d / "pairs.csv").write_text("index,path,target_path\n0,a.png,b.png\n")
    return dict(clean=dict(type="TestImagesCSV", dataset_args=dict(csv_path=str(d / "clean.csv"), root_folder=str(d))),
                pairs=dict(type="TestPairsCSV", dataset_args=dict(csv_path=str(d / "pairs.csv"), root_folder=str(d))))


VAL_CONFIGS = [
    ("defaults", "clean", dict(raw_noise=[0.01, 5]), dict(raw_noise=[0.01, 5.0], factor=16), "validate_jdd"),
    ("all-keys", "clean", dict(raw_noise=(0, 2.5), bayer="gbrg", fill="bilinear", shave="4", bits="12", tile=64, halo=16,
                               micro_batch=1, metric="ssim", factor=8, subsampling=2, noise_sigma=3.0),
     dict(raw_noise=[0.0, 2.5], bayer="gbrg", fill="bilinear", shave=4, bits=12, tile=64, halo=16, micro_batch=1,
          metric="ssim", factor=8), "validate_jdd"),
    ("raw-noise-over-bayer", "clean", dict(bayer="bggr", raw_noise=[0.02, 0]), dict(raw_noise=[0.02, 0.0], bayer="bggr", factor=16),
     "validate_jdd"),
    ("raw-noise-over-scale-and-blur", "clean", dict(scale=2, blur="box:3", raw_noise=[0, 0], shave=2),
     dict(raw_noise=[0.0, 0.0], shave=2, factor=16), "validate_jdd"),
    ("jpeg-over-raw-noise", "clean", dict(jpeg_quality=10, raw_noise=[0.01, 5], bits=12), dict(jpeg_quality=10, factor=16),
     "validate_car"),
    ("bayer-alone", "clean", dict(bayer="rggb", bits=12), dict(bayer="rggb", factor=16), "validate_demosaic"),
    ("pairs-over-raw-noise", "pairs", dict(raw_noise=[0.01, 5]), dict(factor=16), "validate_pairs"),
]


@pytest.mark.parametrize("which,extra,want,check", [c[1:] for c in VAL_CONFIGS], ids=[c[0] for c in VAL_CONFIGS])
def test_the_raw_noise_validation_row(clean_set, which, extra, want, check):
    val_set, val_args = T.create_val_dataset(dict(datasets=dict(val=dict(clean_set[which], **extra))))
    assert val_args == want and all(type(val_args[k]) is type(want[k]) for k in want)
    assert T.val_check(val_set, val_args) is getattr(T, check)


def test_the_raw_noise_row_stands_directly_before_the_bayer_row_and_refuses_in_order(clean_set):
    keys = [p.key for p in T._val_protocols()]
    assert keys.index("raw_noise") + 1 == keys.index("bayer")
    assert [k for k in keys if k != "raw_noise"] == [p.key for p in T._VAL_PROTOCOLS]      # the other rows as they were
    row = list(T._val_protocols())[keys.index("raw_noise")]
    assert row is T._VAL_RAW_NOISE
    assert row.int_keys == ("shave", "bits") and set(row.choices) == {"bayer", "fill"} and row.float_keys == ()
    assert row.metrics == T.VAL_DEMOSAIC_METRICS and row.validator is T.validate_jdd and row.dataset is T.TestImagesCSV
    refusals = [
        (dict(raw_noise=[0, 0], bayer="rgbg", fill="linear"), r"datasets.val.bayer is one of \('rggb', 'grbg', 'gbrg', 'bggr'\)"),
        (dict(raw_noise=[0, 0], fill="linear", metric="psnrb"), r"datasets.val.fill is one of \('zero', 'bilinear', 'malvar'\)"),
        (dict(raw_noise=[0, 0], metric="psnrb"), r"datasets.val.metric is one of \('psnr', 'psnr_y', 'ssim'\), got 'psnrb'"),
        (dict(raw_noise=0.01), r"datasets.val.raw_noise is \[shot, read\]"),
        (dict(raw_noise=[0.01, 5, 1]), r"datasets.val.raw_noise is \[shot, read\]"),
        (dict(raw_noise=[1.5, 5]), r"datasets.val.raw_noise: shot is a number of 0..1"),
        (dict(raw_noise=[0.5, 256]), r"datasets.val.raw_noise: read is a number of 0..255"),
    ]
    for extra, message in refusals:
        with pytest.raises(ValueError, match=message):
            T.create_val_dataset(dict(datasets=dict(val=dict(clean_set["clean"], **extra))))


def test_validate_jdd_passes_its_arguments_and_refuses_without_a_launch(monkeypatch):
    monkeypatch.setattr(K, "_launch", no_launch)
    seen = {}

    def evaluate(model, images, **kw):
        seen.update(kw, n=len(images))
        return {kw["metrics"][0]: (1.5, [1.0, 2.0])}
    monkeypatch.setattr(restore, "evaluate_jdd", evaluate)
    pics = [np.zeros((20, 24, 3), np.uint8), np.zeros((20, 24, 3), np.float32)]
    got = T.validate_jdd(lambda x: x, pics, [0.01, 5.0], "gbrg", "bilinear", 12, False, 9, shave=2, factor=8, device="cpu",
                         metric="ssim", tile=64)
    assert got == 1.5 and seen == dict(n=2, device="cpu", metrics=("ssim",), pattern="gbrg", fill="bilinear", shot=0.01,
                                       read=5.0, bits=12, clip=False, seed=9, shave=2, factor=8, tile=64)
    monkeypatch.undo()
    monkeypatch.setattr(K, "_launch", no_launch)
    with pytest.raises(ValueError, match="validate_jdd: metric is one of"):
        T.validate_jdd(lambda x: x, pics, metric="psnrb", device="cpu")
    with pytest.raises(ValueError, match=r"validate_jdd: raw_noise is \(shot, read\)"):
        T.validate_jdd(lambda x: x, pics, 0.01, device="cpu")
    with pytest.raises(ValueError, match=r"evaluate_jdd: image 0 is \(20, 24, 1\); the protocol takes clean R, G, B"):
        T.validate_jdd(lambda x: x, [np.zeros((20, 24), np.uint8)], device="cpu")


def model(x):
    return x


BIG, SMALL = np.zeros((40, 56, 3), np.uint8), np.zeros((12, 12, 3), np.uint8)


def jdd(images, pattern="rggb", fill="malvar", shot=0.0, read=0.0, bits=16, clip=True, seed=2204, **kw):
    return restore.evaluate_jdd(model, images, pattern, fill, shot, read, bits, clip, seed, **kw)


# (id, call wrong in both ways, the earlier refusal, the call wrong in the later way only, the later refusal): the
# two-adjacent-faults style of tests/test_protocol_order.py
ORDER = [
    ("ensemble-metrics", lambda: jdd([BIG], ensemble=3, metrics=("mse",)), "evaluate_jdd: ensemble",
     lambda: jdd([BIG], metrics=("mse",)), "evaluate_jdd: metrics"),
    ("metrics-unexpected", lambda: jdd([BIG], metrics=("mse",), crop=1), "evaluate_jdd: metrics",
     lambda: jdd([BIG], crop=1), "evaluate_jdd: unexpected arguments"),
    ("unexpected-pattern", lambda: jdd([BIG], "rgbg", crop=1), "evaluate_jdd: unexpected arguments",
     lambda: jdd([BIG], "rgbg"), "evaluate_jdd: the pattern"),
    ("pattern-fill", lambda: jdd([BIG], 4, "linear"), "evaluate_jdd: the pattern",
     lambda: jdd([BIG], 3, "linear"), "evaluate_jdd: the fill"),
    ("fill-shot", lambda: jdd([BIG], fill="linear", shot=2.0), "evaluate_jdd: the fill",
     lambda: jdd([BIG], shot=2.0), "evaluate_jdd: shot is a number of 0..1"),
    ("shot-read", lambda: jdd([BIG], shot=-1, read=300), "evaluate_jdd: shot",
     lambda: jdd([BIG], read=300), "evaluate_jdd: read is a number of 0..255"),
    ("read-bits", lambda: jdd([BIG], read=True, bits=7), "evaluate_jdd: read",
     lambda: jdd([BIG], bits=7), "evaluate_jdd: bits is an integer of 8..16"),
    ("bits-seed", lambda: jdd([BIG], bits=17, seed=-1), "evaluate_jdd: bits",
     lambda: jdd([BIG], seed=-1), "evaluate_jdd: seed is an integer of 0..2\\^64 - 1"),
    ("seed-shave", lambda: jdd([BIG], seed=1 << 64, shave=-1), "evaluate_jdd: seed",
     lambda: jdd([BIG], shave=-1), "evaluate_jdd: shave is a non-negative integer"),
    ("shave-empty", lambda: jdd([], shave=2.0), "evaluate_jdd: shave", lambda: jdd([]), "evaluate_jdd: no images"),
    ("image0-float-image1-small", lambda: jdd([BIG.astype(np.float32), SMALL], shave=6),
     "evaluate_jdd: image 0 is torch.float32; the mosaic is defined on uint8 pictures",
     lambda: jdd([BIG, SMALL], shave=6), r"evaluate_jdd: image 1 is \(12, 12, 3\): nothing is left after a shave of 6"),
    ("image0-gray-image1-not-an-image", lambda: jdd([BIG[:, :, :1], BIG[0]]), "evaluate_jdd: image 0 is .*clean R, G, B",
     lambda: jdd([BIG, BIG[0]]), "evaluate_jdd: image 1: restore_image: expected an H x W x C image"),
    ("float-channels", lambda: jdd([BIG[:, :, :1].astype(np.float32)]), "evaluate_jdd: image 0 is torch.float32",
     lambda: jdd([BIG[:, :, :1]]), "evaluate_jdd: image 0 is .*the protocol takes clean R, G, B pictures"),
    ("nothing-left-metrics", lambda: jdd([SMALL], shave=6, metrics=("ssim",)), "evaluate_jdd: image 0 is .*nothing is left",
     lambda: jdd([SMALL], shave=1, metrics=("ssim",)), r"evaluate_jdd: image 0 after the shave is \(10, 10, 3\); SSIM"),
    ("metrics-plan", lambda: jdd([SMALL], metrics=("psnrb",), factor=32), "evaluate_jdd: image 0 after the shave .*PSNR-B",
     lambda: jdd([SMALL], factor=32), "plan: reflect padding 20 must be smaller"),
]


@pytest.mark.parametrize("both,earlier,later_only,later", [c[1:] for c in ORDER], ids=[c[0] for c in ORDER])
def test_evaluate_jdd_refuses_in_order(monkeypatch, both, earlier, later_only, later):
    monkeypatch.setattr(K, "_launch", no_launch)
    monkeypatch.setattr(restore, "_to_device", no_launch)
    with pytest.raises((ValueError, TypeError), match=earlier):
        both()
    with pytest.raises((ValueError, TypeError), match=later):
        later_only()
    assert irdu_amd.evaluate_jdd is restore.evaluate_jdd and irdu_amd.raw_noise_demosaic_u8 is restore.raw_noise_demosaic_u8
    assert irdu_amd.NoisyBayerDemosaicking is T.NoisyBayerDemosaicking


def test_the_example_yaml_names_registered_types_and_resolves_to_validate_jdd():
    conf = T.parse(os.path.join(ROOT, "experiment_conf", "jdd_rggb_example.yaml"))
    stages = T.train_stage_confs(conf)
    assert len(stages) == 2 and all(st["type"] == "NoisyBayerDemosaicking" and st["device_resident"] for st in stages)
    assert all(st["type"] in T.DATASETS for st in stages)
    assert len({st["dataset_args"]["csv_path"] for st in stages}) == 1          # one csv: the stages share the one arena
    for st in stages:
        args = st["dataset_args"]
        T._check_bayer_args("yaml", args["pattern"], args["fill"], 3)
        T._check_levels("yaml", "shot", args["shot"], 1.0)
        T._check_levels("yaml", "read", args["read"], 255.0)
        assert abs(sum(args["shot"][1]) - 1) < 1e-12 and abs(sum(args["read"][1]) - 1) < 1e-12
    val = conf["datasets"]["val"]
    assert val["type"] == "TestImagesCSV" and val["raw_noise"] == [0.01, 5.0] and conf["train"]["val_every"] > 0
    row = next(p for p in T._val_protocols() if p.key is not None and val.get(p.key) is not None)
    assert row.validator is T.validate_jdd
