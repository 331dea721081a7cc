"""CPU-only checks of grr_u8_resize / grr_u8_resize_images (csrc/resize_ops.hip) and their wrappers: the Python mirror
of the shape query, argument validation before any launch, and the wrappers' host checks.  Launches nothing."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

from irdu_amd import _native
from irdu_amd import kernels as K

INVALID_ARG, SHAPE, UNSUPPORTED = 1, 2, 3
PTR = 0x1000        # never dereferenced: validation fails first


@pytest.fixture(scope="module")
def lib():
    return _native.load()


def arr(values):
    return (ctypes.c_int32 * len(values))(*values)


def one(src=PTR, h=8, w=12, c=3, dst=PTR + 0x1000, ho=None, wo=None, s=2, up=0, taps=None):
    """The arguments of grr_u8_resize for an 8 x 12 x 3 image; taps: (n_phase, first, count, flat) or the legal ones."""
    n_phase, first, count, flat = K._resize_tap_args(s, bool(up)) if taps is None else taps
    if ho is None:
        ho = s * h if up else -(-h // s)
    if wo is None:
        wo = s * w if up else -(-w // s)
    return (src, h, w, c, dst, ho, wo, s, up, n_phase, first, count, flat, None)


def many(src=PTR, src_elems=288, src_table=PTR, dst=PTR + 0x1000, dst_elems=72, dst_table=PTR, c=3, n_img=1, max_ho=4,
         max_wo=6, s=2, up=0, taps=None):
    n_phase, first, count, flat = K._resize_tap_args(s, bool(up)) if taps is None else taps
    return (src, src_elems, src_table, dst, dst_elems, dst_table, c, n_img, max_ho, max_wo, s, up, n_phase, first, count,
            flat, None)


def test_python_mirror_of_the_shape_query(lib):
    """A call on each side of every bound of grr_u8_resize_supported."""
    big = (1 << 31) - 1
    cases = [(c, 8, 12, 2, up) for c in (0, 1, 4, 5) for up in (0, 1)]
    cases += [(3, 8, 12, s, up) for s in (1, 2, 8, 9) for up in (0, 1)]
    cases += [(3, 0, 12, 2, 0), (3, 8, 0, 2, 1), (3, 1, 1, 2, 0), (3, -1, 4, 2, 0)]
    # the input's element count at 2^31 - 1 and 2^31 (down), the output's at and around 2^31 (up)
    cases += [(1, 1, big, 2, 0), (1, 2, 1 << 30, 2, 0), (1, big, 1, 8, 0), (3, 1, 715827882, 2, 0), (3, 1, 715827883, 2, 0),
              (4, 1 << 15, 1 << 14, 2, 0), (4, (1 << 15) - 1, 1 << 14, 2, 0),
              (1, 1 << 14, 1 << 15, 2, 1), (1, (1 << 14) - 1, 1 << 15, 2, 1), (1, 1 << 14, (1 << 15) - 1, 2, 1),
              (1, 1, (1 << 25) - 1, 8, 1), (1, 1, 1 << 25, 8, 1), (4, 1, 1 << 23, 8, 1), (4, 1, (1 << 23) - 1, 8, 1),
              (1, big, big, 8, 1), (2, 1, 1 << 29, 2, 1), (2, 1, (1 << 28) - 1, 2, 1), (2, 1, 1 << 28, 2, 1)]
    seen = set()
    for case in cases:
        got = bool(lib.grr_u8_resize_supported(*case))
        assert K.resize_ok(*case) == got, case
        seen.add(got)
    assert seen == {True, False}
    assert K.resize_ok(1, 1, big, 2, False) and not K.resize_ok(1, 2, 1 << 30, 2, False)
    assert K.resize_ok(1, (1 << 14) - 1, 1 << 15, 2, True) and not K.resize_ok(1, 1 << 14, 1 << 15, 2, True)


def failed(lib, name, args):
    st = getattr(lib, name)(*args)
    return st, lib.grr_last_error() or b""


@pytest.mark.parametrize("name,args", [("grr_u8_resize", one), ("grr_u8_resize_images", many)])
def test_bad_arguments_report_their_status_without_a_launch(lib, name, args):
    label = name.encode()
    nulls = ("src", "dst") if args is one else ("src", "dst", "src_table", "dst_table")
    for null in nulls:
        st, msg = failed(lib, name, args(**{null: None}))
        assert st == INVALID_ARG and label + b": bad args" in msg, null
    for up in (0, 1):
        n_phase, first, count, flat = K._resize_tap_args(2, bool(up))
        for k, null in enumerate(("first", "count", "taps")):
            taps = [n_phase, first, count, flat]
            taps[1 + k] = None
            st, msg = failed(lib, name, args(up=up, taps=tuple(taps)))
            assert st == INVALID_ARG and label + b": bad args" in msg, null
        # a phase that does not sum to 2^30
        wrong = list(flat)
        wrong[1] += 1
        st, msg = failed(lib, name, args(up=up, taps=(n_phase, first, count, arr(wrong))))
        assert st == INVALID_ARG and label in msg and b"sum" in msg
        # more than 4 s taps in a phase: the legal taps with zeros and a +1 / -1 pair appended keep their sum
        n0 = count[0]
        fat = list(flat[:n0]) + [0] * (4 * 2 - n0) + [1] + list(flat[n0:])
        fat[0] -= 1
        st, msg = failed(lib, name, args(up=up, taps=(n_phase, first, arr([9] + list(count[1:])), arr(fat))))
        assert st == INVALID_ARG and label in msg and b"taps" in msg
        # a tap outside the offsets the definition can give
        st, msg = failed(lib, name, args(up=up, taps=(n_phase, arr([first[0] - 40] + list(first[1:])), count, flat)))
        assert st == INVALID_ARG and label in msg and b"support" in msg
        # the wrong number of phases for the direction
        st, msg = failed(lib, name, args(up=up, taps=K._resize_tap_args(2, not up)))
        assert st == INVALID_ARG and label in msg and b"phase" in msg
    for s in (1, 9):
        st, msg = failed(lib, name, args(taps=K._resize_tap_args(2, False), s=s, ho=4, wo=6) if args is one else
                         args(taps=K._resize_tap_args(2, False), s=s))
        assert st == UNSUPPORTED and label in msg and b"scale" in msg
    st, msg = failed(lib, name, args(c=5))
    assert st == UNSUPPORTED and label in msg and b"C <= 4" in msg
    st, msg = failed(lib, name, args(c=0))
    assert st == INVALID_ARG and label + b": bad args" in msg
    with pytest.raises(_native.GrrError, match=name):
        _native.call(name, *args(c=0))


def test_output_sides_are_checked_against_the_input(lib):
    for ho, wo in ((3, 6), (5, 6), (4, 5), (4, 7)):                   # down: exactly ceil(n / s)
        st, msg = failed(lib, "grr_u8_resize", one(ho=ho, wo=wo))
        assert st == SHAPE and b"grr_u8_resize" in msg and b"4 x 6" in msg
    for ho, wo in ((14, 24), (17, 24), (16, 22), (16, 25), (0, 24)):  # up: in (s (n - 1), s n]
        st, msg = failed(lib, "grr_u8_resize", one(up=1, ho=ho, wo=wo))
        assert st == (SHAPE if ho else INVALID_ARG) and b"grr_u8_resize" in msg
    # legal sides pass the checks and reach the launch; nothing may be launched here, so the last legal step is the
    # shape query itself
    assert lib.grr_u8_resize_supported(3, 8, 12, 2, 1) == 1
    # an image whose output has 2^31 elements
    st, msg = failed(lib, "grr_u8_resize", one(h=1 << 14, w=1 << 15, c=1, up=1))
    assert st == UNSUPPORTED and b"2^31" in msg
    # the arena form: too many images, more images than elements, a misaligned table, an output bound of 2^31
    st, msg = failed(lib, "grr_u8_resize_images", many(n_img=65536, src_elems=1 << 20, dst_elems=1 << 20))
    assert st == UNSUPPORTED and b"65535" in msg
    st, msg = failed(lib, "grr_u8_resize_images", many(n_img=73))
    assert st == UNSUPPORTED and b"grr_u8_resize_images" in msg
    for bad in (dict(src_table=PTR + 4), dict(dst_table=PTR + 4)):
        st, msg = failed(lib, "grr_u8_resize_images", many(**bad))
        assert st == INVALID_ARG and b"aligned" in msg
    st, msg = failed(lib, "grr_u8_resize_images", many(max_ho=1 << 16, max_wo=1 << 15, c=1))
    assert st == UNSUPPORTED and b"2^31" in msg
    for bad in (dict(src_elems=0), dict(dst_elems=0), dict(n_img=0), dict(max_ho=0), dict(max_wo=-1)):
        st, msg = failed(lib, "grr_u8_resize_images", many(**bad))
        assert st == INVALID_ARG and b"grr_u8_resize_images: bad args" in msg, bad


def pack_of(host_table=((0, 8, 12), (288, 5, 7)), c=3, dtype=torch.uint8):
    elems = max(off + h * w * c for off, h, w in host_table)
    return SimpleNamespace(arena=torch.zeros(elems, dtype=dtype), host_table=tuple(host_table), c=c, kinds=("numpy",) * 2,
                           table=torch.tensor(host_table, dtype=torch.int64).reshape(-1, 3))


def test_wrappers_refuse_before_any_launch(monkeypatch):
    def no_launch(*a, **k):
        raise AssertionError("a kernel was launched")
    monkeypatch.setattr(K, "_launch", no_launch)
    img = torch.zeros((8, 12, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="GPU"):
        K.u8_resize(img, 2, False)
    with pytest.raises(RuntimeError, match="GPU"):
        K.u8_resize_images(pack_of(), 2, False)
    for bad in (1, 9, 2.0, True, "2"):
        with pytest.raises(ValueError, match="u8_resize: the scale"):
            K.u8_resize(img, bad, False)
        with pytest.raises(ValueError, match="u8_resize_images: the scale"):
            K.u8_resize_images(pack_of(), bad, True)
    with pytest.raises(ValueError, match="uint8"):
        K.u8_resize(img.float(), 2, False)
    with pytest.raises(ValueError, match="H x W x C"):
        K.u8_resize(img[0], 2, False)
    # the output sides of an 8 x 12 image
    assert K.resize_out_hw("t", 8, 12, 2, False) == (4, 6) and K.resize_out_hw("t", 7, 13, 3, False) == (3, 5)
    assert K.resize_out_hw("t", 8, 12, 2, True) == (16, 24) and K.resize_out_hw("t", 8, 12, 2, True, (15, 23)) == (15, 23)
    with pytest.raises(ValueError, match="shrinks to 4 x 6"):
        K.resize_out_hw("t", 8, 12, 2, False, (4, 5))
    for out_hw in ((14, 24), (16, 25), (17, 24), (16, 22)):
        with pytest.raises(ValueError, match="grows to"):
            K.resize_out_hw("t", 8, 12, 2, True, out_hw)
    monkeypatch.setattr(K, "_check_placed", lambda *a: None)
    with pytest.raises(ValueError, match="uint8"):
        K.u8_resize_images(pack_of(dtype=torch.float32), 2, False)
    with pytest.raises(ValueError, match="1 output shapes for 2 images"):
        K.u8_resize_images(pack_of(), 2, True, [(16, 24)])
    with pytest.raises(ValueError, match=r"grows to.*image 1"):
        K.u8_resize_images(pack_of(), 2, True, [(16, 24), (10, 15)])


def test_wrapper_launch_arguments(monkeypatch):
    """What reaches the library: both arenas and tables, the output bound, the dense taps, read + written bytes."""
    sent = []
    monkeypatch.setattr(K, "_check_placed", lambda *a: None)
    monkeypatch.setattr(K, "_stream", lambda dev: None)
    monkeypatch.setattr(K, "_launch", lambda kind, nbytes, name, *a, **k: sent.append((kind, nbytes, name, a)))
    pack = pack_of()
    low = K.u8_resize_images(pack, 2, False)
    assert low.host_table == ((0, 4, 6), (72, 3, 4)) and low.c == 3 and low.arena.numel() == 72 + 36
    assert low.arena.dtype == torch.uint8 and low.kinds == pack.kinds
    kind, nbytes, name, a = sent[0]
    assert (kind, name) == ("u8_resize_images", "grr_u8_resize_images") and nbytes == 288 + 105 + 72 + 36
    assert a[:12] == (pack.arena.data_ptr(), 393, pack.table.data_ptr(), low.arena.data_ptr(), 108, low.table.data_ptr(),
                      3, 2, 4, 6, 2, 0)
    assert a[12] == 1 and list(a[13]) == [-3] and list(a[14]) == [8] and sum(a[15]) == 1 << 30
    back = K.u8_resize_images(low, 2, True, [(8, 12), (5, 7)])
    assert back.host_table == pack.host_table
    assert sent[1][3][8:12] == (8, 12, 2, 1) and sent[1][3][12] == 2
    # the degraded pack shares the clean pack's device table
    sent.clear()
    degraded = K.u8_bicubic_degrade_images(pack, 2)
    assert len(sent) == 2 and degraded.table is pack.table and degraded.host_table == pack.host_table
    assert degraded.arena.numel() == pack.arena.numel() and degraded.arena is not pack.arena
