"""CPU-only checks of grr_patch_mask_batch / grr_u8_mask_fill (csrc/inpaint_ops.hip) and what is built on them: the
header's declarations against the bindings, the Python mirrors of the shape queries on both sides of every bound, every
refusal with its status and entry-point name, the wrappers' host checks before any transfer, the restore.py options and
the ``inpaint_keep`` validation row.  Launches nothing."""
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


def many(arena=PTR, elems=288, c=3, img_table=PTR, n_img=1, table=PTR, ids=PTR, keep=PTR, n=2, seed=7, ph=16, pw=16,
         weights=PTR, kh=7, kw=7, fill=1, hole=128, target=PTR, inp=PTR + 0x10000, mask=PTR + 0x20000):
    return (arena, elems, c, img_table, n_img, table, ids, keep, n, seed, ph, pw, weights, kh, kw, fill, hole, target, inp,
            mask, None)


def one(src=PTR, mask_in=None, h=8, w=12, c=3, keep=1 << 23, seed=7, sample_id=0, weights=PTR, kh=7, kw=7, fill=1, hole=128,
        dst=PTR + 0x1000, mask_out=PTR + 0x2000):
    return (src, mask_in, h, w, c, keep, seed, sample_id, weights, kh, kw, fill, hole, dst, mask_out, None)


def failed(lib, name, args):
    st = getattr(lib, name)(*args)
    return st, lib.grr_last_error() or b""


def test_the_header_declares_what_is_bound():
    flat = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "grr.h")).read())
    assert "int grr_patch_mask_batch_supported(int C, int n_img, int64_t arena_elems, int n, int ph, int pw);" in flat
    assert ("grr_status grr_patch_mask_batch(const uint8_t* arena, int64_t arena_elems, int C, const int64_t* img_table, "
            "int n_img, const int32_t* table, const int64_t* sample_ids, const int32_t* keep /* int32 [n] */, int n, "
            "uint64_t seed, int ph, int pw, const uint8_t* weights /* uint8 [kh kw] */, int kh, int kw, int fill, int hole, "
            "float* target, float* input, float* mask /* or NULL */, void* stream);") in flat
    assert "int grr_u8_mask_fill_supported(int C, int H, int W);" in flat
    assert ("grr_status grr_u8_mask_fill(const uint8_t* src, const uint8_t* mask_in /* uint8 H x W, or NULL */, int H, int W, "
            "int C, int keep, uint64_t seed, int64_t sample_id, const uint8_t* weights, int kh, int kw, int fill, int hole, "
            "uint8_t* dst /* uint8 HWC */, uint8_t* mask_out /* uint8 H x W */, void* stream);") in flat
    for define in ("#define GRR_MASK_HALO 7", "#define GRR_MASK_MAX_SIDE 15", "#define GRR_MASK_ONE (1 << 24)"):
        assert define in flat
    I, L, P, U = _native.I, _native.L, _native.P, _native.ctypes.c_uint64
    assert _native.SIGNATURES["grr_patch_mask_batch_supported"] == [I, I, L, I, I, I]
    assert _native.SIGNATURES["grr_patch_mask_batch"] == [P, L, I, P, I, P, P, P, I, U, I, I, P, I, I, I, I, P, P, P, P]
    assert _native.SIGNATURES["grr_u8_mask_fill_supported"] == [I, I, I]
    assert _native.SIGNATURES["grr_u8_mask_fill"] == [P, P, I, I, I, I, U, L, P, I, I, I, I, P, P, P]
    # the definition is written out above them
    for phrase in ("No floating point appears in the definition", "(ph + 14) x (pw + 14)", "Y = row + wy - 7, X = col + wx - 7",
                   "e = wy (pw + 14) + wx", "counter (e / 4, 1, low32(id), high32(id))", "(x_{e % 4} >> 8) < keep[s]",
                   "in both cases no generator runs", "A mirrored position draws its own bit",
                   "(2 num_c + den) / (2 den)", "otherwise hole", "den <= 225 * 255", "mode & 5", "mask == NULL skips it",
                   "A sample does not depend on the batch it is in", "2 where this call filled a pixel with den > 0",
                   "nonzero means known", "No atomics"):
        assert phrase in flat, phrase
    build = open(os.path.join(ROOT, "imagerestoration-development-unrolling_amd", "build_native.py")).read()
    assert '"inpaint_ops.hip"' in build
    assert (K.MASK_HALO, K.MAX_MASK_SIDE, K.MASK_ONE, K.MASK_FILLS) == (7, 15, 1 << 24, ("zero", "conv"))
    assert T.MASK_FILLS == K.MASK_FILLS and T.MASK_HALO == K.MASK_HALO
    rows, cols = K.MASK_TILE
    assert rows >= 1 and cols % 4 == 0


def test_python_mirrors_of_the_shape_queries(lib):
    """A call on each side of every bound of the two queries."""
    big = (1 << 31) - 1
    cases = [(3, 1, 288, 2, 16, 16), (0, 1, 288, 2, 16, 16), (5, 1, 288, 2, 16, 16), (4, 1, 288, 2, 16, 16),
             (3, 0, 288, 2, 16, 16), (3, 289, 288, 2, 16, 16), (3, 1, 0, 1, 1, 1), (3, 1, 1 << 62, 1, 1, 1),
             (3, 1, (1 << 62) - 1, 1, 1, 1), (3, 1, 288, 0, 16, 16), (3, 1, 288, 2, 0, 16), (3, 1, 288, 2, 16, 0),
             (3, 1, 288, 1, 1, 715827882), (3, 1, 288, 1, 1, 715827883), (1, 1, 288, 1, 1, 143165562), (1, 1, 288, 1, 1, 143165563),
             (1, 1, 288, 1, 143165562, 1), (1, 1, 288, 1, 143165563, 1), (1, 1, 288, 1, 46326, 46326), (1, 1, 288, 1, 46327, 46327),
             (4, 1, 288, 1, 1 << 14, 1 << 15), (1, 1, 288, 4, 1 << 14, 1 << 15), (1, 1, 288, 3, 1 << 14, 1 << 15),
             (3, 1, 288, big, big, big), (1, 1, 288, 1, big, 1), (1, 1, 288, 1, 1, big)]
    seen = set()
    for case in cases:
        got = bool(lib.grr_patch_mask_batch_supported(*case))
        assert K.patch_mask_batch_ok(*case) == got, case
        seen.add(got)
    assert seen == {True, False}
    # the window (ph + 14)(pw + 14) < 2^31 binds on thin patches: 15 * 143165577 = 2^31 + 7
    assert K.patch_mask_batch_ok(1, 1, 288, 1, 1, 143165562) and not K.patch_mask_batch_ok(1, 1, 288, 1, 1, 143165563)
    assert K.patch_batch_ok(1, 1, 288, 1, 1, 143165563)
    shapes = [(3, 8, 12), (0, 8, 12), (5, 8, 12), (3, 0, 12), (3, 8, 0), (3, -1, 4), (4, 1, 1), (1, 1, 143165562), (1, 1, 143165563),
              (1, 143165562, 1), (1, 143165563, 1), (3, 1 << 15, 21845), (3, 1 << 15, 21846), (1, 46326, 46326), (1, 46327, 46327),
              (1, big, big), (1, 1, big)]
    seen = set()
    for c, h, w in shapes:
        got = bool(lib.grr_u8_mask_fill_supported(c, h, w))
        assert K.mask_fill_ok(c, h, w) == got, (c, h, w)
        seen.add(got)
    assert seen == {True, False}
    assert K.mask_fill_ok(1, 1, 143165562) and not K.mask_fill_ok(1, 1, 143165563)


@pytest.mark.parametrize("name,args", [("grr_patch_mask_batch", many), ("grr_u8_mask_fill", one)])
def test_bad_arguments_report_their_status_without_a_launch(lib, name, args):
    label = name.encode()
    nulls = ("src", "weights", "dst", "mask_out") if args is one else ("arena", "img_table", "table", "ids", "keep", "weights",
                                                                       "target", "inp")
    for null in nulls:
        st, msg = failed(lib, name, args(**{null: None}))
        assert st == INVALID_ARG and label + b": bad args" in msg, null
    for c in (0, 5, -1):
        st, msg = failed(lib, name, args(c=c))
        assert st == INVALID_ARG and label + b": C is 1..4" in msg, c
    for c in (1, 4):
        st, msg = failed(lib, name, args(c=c, fill=2))                  # C passes: the next refusal speaks
        assert b"the fill" in msg
    for sides in (dict(kh=0), dict(kh=2), dict(kh=16), dict(kh=17), dict(kw=0), dict(kw=6), dict(kw=16), dict(kw=-1)):
        st, msg = failed(lib, name, args(**sides))
        assert st == INVALID_ARG and label + b": the weight table's sides are odd and lie in 1..15" in msg, sides
    for sides in (dict(kh=1, kw=15), dict(kh=15, kw=1)):
        st, msg = failed(lib, name, args(fill=2, **sides))              # the sides pass
        assert b"the fill" in msg
    for fill in (-1, 2, 7):
        st, msg = failed(lib, name, args(fill=fill))
        assert st == INVALID_ARG and label + b": the fill is 0 (zero) or 1 (conv)" in msg, fill
    for hole in (-1, 256, 1000):
        st, msg = failed(lib, name, args(hole=hole))
        assert st == INVALID_ARG and label + b": the hole is a byte 0..255" in msg, hole
    for hole in (0, 255):
        st, msg = failed(lib, name, args(hole=hole, c=9))
        assert b"C is" in msg
    # C before the sides before the fill before the hole
    st, msg = failed(lib, name, args(c=5, kh=2, fill=3, hole=-1))
    assert b"C is" in msg
    st, msg = failed(lib, name, args(kh=2, fill=3, hole=-1))
    assert b"sides" in msg
    st, msg = failed(lib, name, args(fill=3, hole=-1))
    assert b"the fill" in msg
    with pytest.raises(_native.GrrError, match=name):
        _native.call(name, *args(fill=3))


def test_the_patch_form_checks_its_tables_and_bounds(lib):
    name = "grr_patch_mask_batch"
    for bad in (dict(elems=0), dict(n_img=0), dict(n=0), dict(n=-1), dict(ph=0), dict(pw=-3)):
        st, msg = failed(lib, name, many(**bad))
        assert st == INVALID_ARG and b"grr_patch_mask_batch: bad args" in msg, bad
    st, msg = failed(lib, name, many(n_img=289))                       # more images than elements
    assert st == UNSUPPORTED and name.encode() in msg and b"arena elements" in msg
    for bad in (dict(n=715827883, ph=1, pw=1), dict(n=1, ph=1 << 15, pw=21846), dict(n=1, c=1, ph=1, pw=143165563),
                dict(n=1, c=1, ph=46327, pw=46327)):
        st, msg = failed(lib, name, many(**bad))
        assert st == UNSUPPORTED and b"grr_patch_mask_batch: patch batch n C ph pw and the window (ph + 14)(pw + 14)" in msg \
            and b"2^31" in msg, bad
    for bad in (dict(table=PTR + 2), dict(keep=PTR + 1), dict(target=PTR + 2), dict(inp=PTR + 1), dict(mask=PTR + 2)):
        st, msg = failed(lib, name, many(**bad))
        assert st == INVALID_ARG and b"4-byte aligned" in msg, bad
    for bad in (dict(img_table=PTR + 4), dict(ids=PTR + 4)):
        st, msg = failed(lib, name, many(**bad))
        assert st == INVALID_ARG and b"8-byte aligned" in msg, bad


def test_the_one_picture_form_checks_keep_and_the_size(lib):
    name = "grr_u8_mask_fill"
    for keep in (-1, (1 << 24) + 1, 1 << 30):
        st, msg = failed(lib, name, one(keep=keep))
        assert st == INVALID_ARG and b"grr_u8_mask_fill: keep lies in [0, 2^24]" in msg, keep
    for keep in (0, 1 << 24):
        st, msg = failed(lib, name, one(keep=keep, h=1 << 15, w=21846))          # keep passes: the size speaks
        assert st == UNSUPPORTED and b"grr_u8_mask_fill" in msg and b"2^31" in msg
    for bad in (dict(h=0), dict(w=-1)):
        st, msg = failed(lib, name, one(**bad))
        assert st == INVALID_ARG and b"grr_u8_mask_fill: bad args" in msg, bad
    st, msg = failed(lib, name, one(c=1, h=1, w=143165563))
    assert st == UNSUPPORTED and b"(H + 14)(W + 14) < 2^31" in msg
    st, msg = failed(lib, name, one(hole=300, keep=-1))                           # the hole before keep
    assert b"the hole" in msg


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
        K.u8_mask_fill(img)
    for bad in ("mean", 2, -1, True, None):
        with pytest.raises(ValueError, match="u8_mask_fill: the fill"):
            K.u8_mask_fill(img, fill=bad)
        with pytest.raises(ValueError, match="mask_fill_u8: the fill"):
            irdu_amd.mask_fill_u8(u8, keep=0.5, fill=bad)
        with pytest.raises(ValueError, match="evaluate_inpaint: the fill"):
            irdu_amd.evaluate_inpaint(lambda x: x, [u8], 0.5, fill=bad, device="cpu")
    for bad in (np.zeros((3, 3), np.int32), np.zeros((2, 3), np.uint8), np.zeros((3, 17), np.uint8), np.zeros(9, np.uint8)):
        with pytest.raises(ValueError, match="u8_mask_fill: a weight table"):
            K.u8_mask_fill(img, weights=bad)
        with pytest.raises(ValueError, match="mask_fill_u8: a weight table"):
            irdu_amd.mask_fill_u8(u8, keep=0.5, weights=bad)
    for bad in (-1, 256, 128.0, True, None):
        with pytest.raises(ValueError, match="u8_mask_fill: the hole is an integer of 0..255"):
            K.u8_mask_fill(img, hole=bad)
        with pytest.raises(ValueError, match="mask_fill_u8: the hole"):
            irdu_amd.mask_fill_u8(u8, keep=0.5, hole=bad)
    for bad in (-1, (1 << 24) + 1, 0.5, True):
        with pytest.raises(ValueError, match="u8_mask_fill: keep is an integer of 0..2\\^24"):
            K.u8_mask_fill(img, keep=bad)
    for bad in (-0.1, 1.5, float("nan"), "0.5", True):
        with pytest.raises(ValueError, match="mask_fill_u8: keep is the known share"):
            irdu_amd.mask_fill_u8(u8, keep=bad)
        with pytest.raises(ValueError, match="evaluate_inpaint: keep is the known share"):
            irdu_amd.evaluate_inpaint(lambda x: x, [u8], bad, device="cpu")
    for bad in (-1, 1 << 64, 2.0, True):
        with pytest.raises(ValueError, match="seed"):
            K.u8_mask_fill(img, seed=bad)
        with pytest.raises(ValueError, match="mask_fill_u8: seed"):
            irdu_amd.mask_fill_u8(u8, keep=0.5, seed=bad)
    for bad in (1 << 63, -(1 << 63) - 1, 0.0):
        with pytest.raises(ValueError, match="sample_id"):
            K.u8_mask_fill(img, sample_id=bad)
        with pytest.raises(ValueError, match="mask_fill_u8: sample_id"):
            irdu_amd.mask_fill_u8(u8, keep=0.5, sample_id=bad)
    for bad in (0, -1, 1.0, True):
        with pytest.raises(ValueError, match="mask_fill_u8: passes is a positive integer"):
            irdu_amd.mask_fill_u8(u8, keep=0.5, passes=bad)
        with pytest.raises(ValueError, match="evaluate_inpaint: passes is a positive integer"):
            irdu_amd.evaluate_inpaint(lambda x: x, [u8], 0.5, passes=bad, device="cpu")
    with pytest.raises(ValueError, match="mask_fill_u8: exactly one of mask and keep"):
        irdu_amd.mask_fill_u8(u8)
    with pytest.raises(ValueError, match="mask_fill_u8: exactly one of mask and keep"):
        irdu_amd.mask_fill_u8(u8, mask=np.ones((8, 12), np.uint8), keep=0.5)
    for bad in (np.ones((8, 11), np.uint8), np.ones((8, 12), np.float32), np.ones((8, 12, 1), np.uint8)):
        with pytest.raises(ValueError, match="mask_fill_u8: a mask is uint8 or bool H x W"):
            irdu_amd.mask_fill_u8(u8, mask=bad)
    with pytest.raises(ValueError, match="uint8"):
        K.u8_mask_fill(img.float())
    with pytest.raises(ValueError, match="mask_fill_u8: expected a uint8"):
        irdu_amd.mask_fill_u8(u8.astype(np.float32), keep=0.5)
    with pytest.raises(ValueError, match="u8_mask_fill: a mask is a uint8 H x W tensor"):
        K.u8_mask_fill(img, torch.zeros((8, 11), dtype=torch.uint8))
    with pytest.raises(ValueError, match="evaluate_inpaint: .*sides are odd"):
        irdu_amd.evaluate_inpaint(lambda x: x, [u8], 0.5, fill_side=4, device="cpu")
    with pytest.raises(ValueError, match="evaluate_inpaint: keep_known is True or False"):
        irdu_amd.evaluate_inpaint(lambda x: x, [u8], 0.5, keep_known=1, device="cpu")
    with pytest.raises(ValueError, match="evaluate_inpaint: shave"):
        irdu_amd.evaluate_inpaint(lambda x: x, [u8], 0.5, shave=-1, device="cpu")
    with pytest.raises(ValueError, match="evaluate_inpaint: metrics"):
        irdu_amd.evaluate_inpaint(lambda x: x, [u8], 0.5, metrics=("mse",), device="cpu")
    with pytest.raises(ValueError, match="evaluate_inpaint: no images"):
        irdu_amd.evaluate_inpaint(lambda x: x, [], 0.5, device="cpu")
    with pytest.raises(ValueError, match="evaluate_inpaint: image 0 is torch.float32; the mask is defined on uint8"):
        irdu_amd.evaluate_inpaint(lambda x: x, [u8.astype(np.float32)], 0.5, device="cpu")
    with pytest.raises(ValueError, match=r"evaluate_inpaint: image 0 is \(8, 12, 3\): nothing is left after a shave of 4"):
        irdu_amd.evaluate_inpaint(lambda x: x, [u8], 0.5, shave=4, device="cpu")
    with pytest.raises(ValueError, match="evaluate_inpaint: image 0 after the shave is .*SSIM"):
        irdu_amd.evaluate_inpaint(lambda x: x, [u8], 0.5, metrics=("psnr_missing", "ssim"), device="cpu")
    # the batch: what patch_batch refuses, and the keep list
    monkeypatch.setattr(K, "_check_placed", lambda *a: None)
    src = K.patch_source(pack_of())
    rows, ids, keep = [(0, 1, 2, 0), (1, 4, 6, 5)], [5, 6], [1 << 23, 0]
    for bad, message in ((dict(fill="mean"), "the fill"), (dict(hole=256), "the hole"),
                         (dict(weights=np.zeros((2, 2), np.uint8)), "a weight table")):
        with pytest.raises(ValueError, match="patch_mask_batch: " + message):
            K.patch_mask_batch(src, rows, ids, keep, 7, 16, 16, **bad)
    for bad in ([1 << 23], [0.5, 0.5], [-1, 0], [(1 << 24) + 1, 0], [[1, 2], [3, 4]]):
        with pytest.raises(ValueError, match=r"patch_mask_batch: keep is integers of 0..2\^24, one per row \(2\)"):
            K.patch_mask_batch(src, rows, ids, bad, 7, 16, 16)
    with pytest.raises(ValueError, match="image indices"):
        K.patch_mask_batch(src, [(2, 0, 0, 0)], [1], [0], 7, 16, 16)
    with pytest.raises(ValueError, match="inside the row's image"):
        K.patch_mask_batch(src, [(1, 5, 0, 0)], [1], [0], 7, 16, 16)
    with pytest.raises(ValueError, match="modes must lie in 0..7"):
        K.patch_mask_batch(src, [(0, 0, 0, 8)], [1], [0], 7, 16, 16)
    with pytest.raises(ValueError, match="need a square patch"):
        K.patch_mask_batch(src, [(0, 0, 0, 2)], [1], [0], 7, 16, 32)
    with pytest.raises(ValueError, match="seed must fit 64 bits"):
        K.patch_mask_batch(src, rows, ids, keep, -1, 16, 16)
    with pytest.raises(ValueError, match="must have 1..2\\^31-1 elements"):
        K.patch_mask_batch(src, rows, ids, keep, 7, 1 << 15, 1 << 15)
    with pytest.raises(ValueError, match=r"patch_mask_batch: the window \(1 \+ 14\) x \(143165563 \+ 14\) must have fewer than 2\^31"):
        K.patch_mask_batch(src, [(0, 0, 0, 0)], [1], [0], 7, 1, 143165563)


def test_wrapper_launch_arguments(monkeypatch):
    """What reaches the library: the arena and its table, the three tables, the weight table and the call-wide codes."""
    sent = []
    monkeypatch.setattr(K, "_check_placed", lambda *a: None)
    monkeypatch.setattr(K, "_stream", lambda dev: None)
    monkeypatch.setattr(K, "_launch", lambda kind, nbytes, name, *a, **k: sent.append((kind, nbytes, name, a)))
    pack = pack_of()
    rows, ids = [(0, 1, 2, 0), (1, 4, 6, 5), (0, 7, 11, 3)], [5, 6, (3 << 32) | 1]
    target, inp, mask = K.patch_mask_batch(pack, rows, ids, [0, 1 << 24, 5], 9, 16, 16, np.ones((3, 5), np.uint8), "conv", 17)
    assert tuple(target.shape) == tuple(inp.shape) == (3, 3, 16, 16) and tuple(mask.shape) == (3, 1, 16, 16)
    assert target.dtype == inp.dtype == mask.dtype == torch.float32
    kind, nbytes, name, a = sent[0]
    assert (kind, name) == ("patch_mask_batch", "grr_patch_mask_batch")
    assert a[:5] == (pack.arena.data_ptr(), 393, 3, pack.table.data_ptr(), 2)
    assert a[8:12] == (3, 9, 16, 16) and a[13:17] == (3, 5, 1, 17)
    assert a[17:20] == (target.data_ptr(), inp.data_ptr(), mask.data_ptr())
    sent.clear()
    out = K.patch_mask_batch(pack, [r[:3] + (r[3] & 5,) for r in rows], ids, [1, 2, 3], 9, 16, 32, None, "zero", with_mask=False)
    assert out[2] is None and sent[0][3][19] is None and sent[0][3][8:12] == (3, 9, 16, 32) and sent[0][3][13:17] == (7, 7, 0, 128)
    monkeypatch.setattr(K, "_check_image", lambda name, t: tuple(t.shape))
    img = torch.zeros((8, 12, 3), dtype=torch.uint8)
    sent.clear()
    out, mask_out = K.u8_mask_fill(img, None, 77, np.ones((1, 3), np.uint8), "conv", 3, 11, -2)
    assert tuple(out.shape) == (8, 12, 3) and out.dtype == torch.uint8 and tuple(mask_out.shape) == (8, 12)
    a = sent[0][3]
    assert sent[0][2] == "grr_u8_mask_fill" and a[:8] == (img.data_ptr(), None, 8, 12, 3, 77, 11, -2)
    assert a[9:15] == (1, 3, 1, 3, out.data_ptr(), mask_out.data_ptr())
    given = torch.ones((8, 12), dtype=torch.uint8)
    sent.clear()
    K.u8_mask_fill(img, given, 0, None, "zero")
    assert sent[0][3][1] == given.data_ptr() and sent[0][3][9:13] == (7, 7, 0, 128)


def cli():
    from tests.test_restore_ref import _cli
    return _cli()


def test_restore_command_options():
    command = cli()
    base = ["-yaml_path", "conf.yaml", "--input", "in", "--output", "out"]
    args = command.parse_args(base + ["--inpaint-keep", "0.2", "--ssim"])
    assert args.inpaint_keep == 0.2 and args.scored and args.inpaint and args.mask is None
    assert (args.mask_fill, args.mask_fill_side, args.mask_fill_sigma, args.mask_fill_passes, args.mask_seed) == ("conv", 7, None, 1, 2204)
    assert not args.no_keep_known
    args = command.parse_args(base + ["--inpaint-keep", "1", "--mask-fill", "conv", "--mask-fill-side", "15", "--mask-fill-sigma", "2.5",
                                      "--mask-fill-passes", "3", "--mask-seed", "5", "--no-keep-known", "--batch-images"])
    assert (args.mask_fill_side, args.mask_fill_sigma, args.mask_fill_passes, args.mask_seed) == (15, 2.5, 3, 5) and args.no_keep_known
    args = command.parse_args(base + ["--inpaint-keep", "0", "--mask-fill", "zero"])
    assert args.mask_fill == "zero" and args.inpaint_keep == 0.0
    args = command.parse_args(base + ["--mask", "masks"])
    assert args.mask == "masks" and args.inpaint and not args.scored and not args.mask_white_missing
    args = command.parse_args(base + ["--mask", "masks", "--reference", "truth", "--mask-white-missing", "--mask-fill-passes", "4"])
    assert args.scored and args.mask_white_missing and args.mask_fill_passes == 4
    for bad in (["--inpaint-keep", "1.5"], ["--inpaint-keep", "-0.1"], ["--inpaint-keep", "x"],
                ["--inpaint-keep", "0.2", "--sigma", "5"], ["--inpaint-keep", "0.2", "--reference", "d"],
                ["--inpaint-keep", "0.2", "--scale", "2"], ["--inpaint-keep", "0.2", "--bayer", "rggb"],
                ["--inpaint-keep", "0.2", "--blur", "box:3"], ["--inpaint-keep", "0.2", "--jpeg-quality", "10"],
                ["--inpaint-keep", "0.2", "--mask", "m"], ["--mask", "m", "--sigma", "5"], ["--mask", "m", "--scale", "2"],
                ["--mask", "m", "--upscale", "2"], ["--mask", "m", "--raw", "rggb"], ["--mask", "m", "--blur", "box:3"],
                ["--mask", "m", "--jpeg-quality", "10"], ["--mask", "m", "--bayer", "rggb"], ["--mask", "m", "--mask-seed", "3"],
                ["--mask-fill", "conv"], ["--mask-fill-side", "7"], ["--mask-fill-sigma", "1"], ["--mask-fill-passes", "2"],
                ["--mask-seed", "3"], ["--no-keep-known"], ["--mask-white-missing"],
                ["--inpaint-keep", "0.2", "--mask-white-missing"], ["--inpaint-keep", "0.2", "--mask-fill", "mean"],
                ["--inpaint-keep", "0.2", "--mask-fill-side", "6"], ["--inpaint-keep", "0.2", "--mask-fill-side", "17"],
                ["--inpaint-keep", "0.2", "--mask-fill-sigma", "0"], ["--inpaint-keep", "0.2", "--mask-fill-passes", "0"],
                ["--inpaint-keep", "0.2", "--mask-seed", "-1"], ["--inpaint-keep", "0.2", "--mask-fill", "zero", "--mask-fill-side", "5"],
                ["--inpaint-keep", "0.2", "--mask-fill", "zero", "--mask-fill-sigma", "1"], ["--inpaint-keep", "0.2", "--shave", "2"],
                ["--inpaint-keep", "0.2", "--psnrb"]):
        with pytest.raises(SystemExit):
            command.parse_args(base + bad)


@pytest.fixture(scope="module")
def clean_set(tmp_path_factory):
    d = tmp_path_factory.mktemp("val")
    (d / "clean.csv").write_text("index,path\n0,a.png\n")
    (d / "pairs.csv").write_text("index,path,target_path\n0,a.png,b.png\n")
    return dict(clean=dict(type="TestImagesCSV", dataset_args=dict(csv_path=str(d / "clean.csv"), root_folder=str(d))),
                pairs=dict(type="TestPairsCSV", dataset_args=dict(csv_path=str(d / "pairs.csv"), root_folder=str(d))))


VAL_CONFIGS = [
    ("defaults", "clean", dict(inpaint_keep=0.2), dict(inpaint_keep=0.2, factor=16), "validate_inpaint"),
    ("all-keys", "clean", dict(inpaint_keep=1, fill="zero", fill_side="5", fill_sigma="1.5", hole=0, passes=2, seed=7, shave="4",
                               tile=64, halo=16, micro_batch=1, metric="psnr_missing", factor=8, sigma=3.0, boundary="wrap"),
     dict(inpaint_keep=1.0, fill="zero", fill_side=5, fill_sigma=1.5, hole=0, passes=2, seed=7, shave=4, tile=64, halo=16,
          micro_batch=1, metric="psnr_missing", factor=8), "validate_inpaint"),
    ("over-every-other-row", "clean", dict(inpaint_keep=0.5, jpeg_quality=10, raw_noise=[0.01, 5], bayer="rggb", scale=2,
                                           blur="box:3"), dict(inpaint_keep=0.5, factor=16), "validate_inpaint"),
    ("pairs-over-inpaint", "pairs", dict(inpaint_keep=0.5), dict(factor=16), "validate_pairs"),
    ("bayer-alone", "clean", dict(bayer="rggb"), dict(bayer="rggb", factor=16), "validate_demosaic"),
    ("noise", "clean", dict(sigma=15), dict(sigma=15.0, factor=16), "validate"),
]


@pytest.mark.parametrize("which,extra,want,check", [c[1:] for c in VAL_CONFIGS], ids=[c[0] for c in VAL_CONFIGS])
def test_the_inpaint_validation_row(clean_set, which, extra, want, check):
    val_set, val_args = T.create_val_dataset(dict(datasets=dict(val=dict(clean_set[which], **extra))))
    assert val_args == want and all(type(val_args[k]) is type(want[k]) for k in want)
    assert T.val_check(val_set, val_args) is getattr(T, check)


def test_the_inpaint_row_stands_first_and_leaves_the_others_as_they_were(clean_set):
    rows = list(T._val_rows())
    assert rows[0] is T._VAL_INPAINT and rows[1:] == list(T._val_protocols())
    row = rows[0]
    assert row.key == "inpaint_keep" and row.dataset is T.TestImagesCSV and row.validator is T.validate_inpaint
    assert row.int_keys == ("shave", "fill_side", "hole", "passes", "seed") and row.float_keys == ("fill_sigma",)
    assert row.choices == {"fill": ("zero", "conv")} and row.metrics == T.VAL_INPAINT_METRICS == ("psnr", "psnr_y", "ssim", "psnr_missing")
    refusals = [
        (dict(inpaint_keep=0.5, fill="malvar"), r"datasets.val.fill is one of \('zero', 'conv'\)"),
        (dict(inpaint_keep=0.5, metric="psnrb"), r"datasets.val.metric is one of \('psnr', 'psnr_y', 'ssim', 'psnr_missing'\)"),
        (dict(inpaint_keep=1.5), "datasets.val.inpaint_keep is the known share"),
        (dict(inpaint_keep="half"), "datasets.val.inpaint_keep is the known share"),
    ]
    for extra, message in refusals:
        with pytest.raises(ValueError, match=message):
            T.create_val_dataset(dict(datasets=dict(val=dict(clean_set["clean"], **extra))))


def test_validate_inpaint_passes_its_arguments_and_refuses_without_a_launch(monkeypatch):
    monkeypatch.setattr(K, "_launch", no_launch)
    seen = {}

    def evaluate(model, images, **kw):
        seen.update(kw, n=len(images))
        return {kw["metrics"][0]: (1.5, [1.0, 2.0])}
    monkeypatch.setattr(restore, "evaluate_inpaint", evaluate)
    pics = [np.zeros((20, 24, 3), np.uint8), np.zeros((20, 24, 3), np.float32)]
    got = T.validate_inpaint(lambda x: x, pics, 0.3, "zero", 5, 1.5, 9, 3, 2, shave=2, factor=8, device="cpu",
                             metric="psnr_missing", tile=64)
    assert got == 1.5 and seen == dict(n=2, device="cpu", metrics=("psnr_missing",), keep=0.3, fill="zero", fill_side=5,
                                       fill_sigma=1.5, hole=9, seed=3, passes=2, shave=2, factor=8, tile=64)
    monkeypatch.undo()
    monkeypatch.setattr(K, "_launch", no_launch)
    with pytest.raises(ValueError, match="validate_inpaint: metric is one of"):
        T.validate_inpaint(lambda x: x, pics, metric="psnrb", device="cpu")
    assert irdu_amd.evaluate_inpaint is restore.evaluate_inpaint and irdu_amd.mask_fill_u8 is restore.mask_fill_u8
    assert irdu_amd.psnr_missing_u8 is restore.psnr_missing_u8 and irdu_amd.RandomMaskInpainting is T.RandomMaskInpainting


def test_the_example_yaml_names_registered_types_and_resolves_to_validate_inpaint():
    conf = T.parse(os.path.join(ROOT, "experiment_conf", "inpaint_example.yaml"))
    stages = T.train_stage_confs(conf)
    assert len(stages) == 2 and all(st["type"] == "RandomMaskInpainting" and st["device_resident"] for st in stages)
    assert all(st["type"] in T.DATASETS for st in stages)
    assert len({st["dataset_args"]["csv_path"] for st in stages}) == 1          # one csv: the stages share the one arena
    for st in stages:
        args = st["dataset_args"]
        T._check_levels("yaml", "keep", args["keep"], 1.0)
        assert abs(sum(args["keep"][1]) - 1) < 1e-12 and args["fill"] in T.MASK_FILLS
        K.mask_weights(args["fill_side"], args.get("fill_sigma"))
    val = conf["datasets"]["val"]
    assert val["type"] == "TestImagesCSV" and val["inpaint_keep"] == 0.2 and conf["train"]["val_every"] > 0
    row = next(p for p in T._val_rows() if p.key is not None and val.get(p.key) is not None)
    assert row.validator is T.validate_inpaint
