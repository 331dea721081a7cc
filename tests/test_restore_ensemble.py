"""CPU-only checks of the geometric self-ensemble (irdu_amd.restore ``ensemble=``): the index map, the
planner with modes, and the argument validation of the four entry points of csrc/image_ops.hip
(grr_tile_gather_d8, grr_tiles_gather_d8, grr_tile_scatter_mean, grr_tiles_scatter_mean) and their wrappers.
Loads the library, launches nothing."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from irdu_amd import _native, restore
from irdu_amd import kernels as K
from tests import restore_ensemble_ref as E

INVALID_ARG, UNSUPPORTED = 1, 3
PTR = 0x1000        # never dereferenced: validation fails first
SHAPES = [(1, 1), (1, 5), (5, 7), (16, 48)]


@pytest.fixture(scope="module")
def lib():
    return _native.load()


# ---- 1. the index map
@pytest.mark.parametrize("m", range(8))
def test_dihedral_index_is_rot90_then_flipud(m):
    for th, tw in SHAPES:
        a = np.arange(th * tw).reshape(th, tw)
        t = np.rot90(a, m // 2)
        t = np.flipud(t) if m % 2 else t
        assert t.shape == ((th, tw) if m in E.EVEN else (tw, th))
        assert np.array_equal(t, E.transform(a, m))
        seen = set()
        for i in range(th):
            for j in range(tw):
                p, q = K.dihedral_index(m, th, tw, i, j)
                assert t[p, q] == a[i, j], (m, th, tw, i, j)
                seen.add((p, q))
        assert len(seen) == th * tw
        assert np.array_equal(E.inverse(E.transform(a, m), m), a)          # T_m^-1 T_m is the identity
        b = np.arange(2 * 3 * th * tw).reshape(2, 3, th, tw)               # ... on the last two axes of a batch
        assert np.array_equal(E.inverse(E.transform(b, m), m), b)
        assert np.array_equal(E.transform(b, m)[1, 2], E.transform(b[1, 2], m))
    for bad in (-1, 8):
        with pytest.raises(ValueError):
            K.dihedral_index(bad, 4, 4, 0, 0)


def test_the_tree_is_not_the_sequential_sum():
    """Eight values that show the order: 0.0 under the tree, 2.25 left to right; three equal
    values round only in the sequential sum's 3v."""
    zs = [np.float32(v) for v in (1e8, 1, -1e8, 1, 0.5, 3e7, -3e7, 0.25)]
    assert E.tree_mean(zs) == np.float32(0.0) and E.sequential_mean(zs) == np.float32(2.25 / 8)
    v = np.float32(0.1)
    for m in (2, 4, 8):
        assert E.tree_mean([v] * m) == v
    assert E.tree_mean([v, v, v]) == ((v + v) + v) / np.float32(3)


# ---- 2. the planner
IMAGES = [(48, 80), (80, 48), (48, 48), (100, 140), (37, 53), (53, 37)]


@pytest.mark.parametrize("modes", [8, (0, 3), (2, 6), (0, 1, 2), (0, 1, 4, 5), (0,), None])
@pytest.mark.parametrize("micro_batch", [1, 3, 16])
@pytest.mark.parametrize("tile,halo", [(48, 16), (256, 32)])
def test_plan_images_with_modes_follows_the_group_rule(tile, halo, micro_batch, modes):
    ms = restore._ensemble_modes("test", modes)
    most = max(len(part) for part in E.split(ms))
    assert most == {8: 4, (0, 3): 1, (2, 6): 2, (0, 1, 2): 2, (0, 1, 4, 5): 4, (0,): 1, None: 1}[modes]
    launches = restore.plan_images(IMAGES, 16, tile, halo, micro_batch, modes=modes)
    if most == 1:
        assert launches == restore.plan_images(IMAGES, 16, tile, halo, micro_batch)
    by_shape, per_image = {}, [[] for _ in IMAGES]
    for th, tw, rows in launches:
        by_shape.setdefault((th, tw), []).append(len(rows))
        for row in rows:
            p = restore.plan(*IMAGES[row[0]], 16, tile, halo)
            assert (p.th, p.tw) == (th, tw)
            per_image[row[0]].append(tuple(row[1:]))
    if tile == 256:             # one window per image: windows of both orientations and square ones in one call
        assert list(by_shape) == [(48, 80), (80, 48), (48, 48), (112, 144), (48, 64), (64, 48)]
    else:
        assert list(by_shape) == [(48, 48)] and sum(by_shape[48, 48]) > 20
    for (th, tw), counts in by_shape.items():
        cap = max(1, (micro_batch * tile * tile) // (th * tw * most))
        assert all(c == cap for c in counts[:-1]) and 1 <= counts[-1] <= cap, (th, tw, counts)
    for i, (h, w) in enumerate(IMAGES):                              # every window once, in the plan's order
        assert per_image[i] == [tuple(w_) for w_ in restore.plan(h, w, 16, tile, halo).windows]


@pytest.mark.parametrize("bad", [0, 2, 7, -1, True, 8.0, "8", "01", (), [], (8,), (-1, 0), (0, 0), (1, 0), (0, 2, 1),
                                 (0, 1.0), (0.0,), (True,), {0, 1}, tuple(range(9))])
def test_bad_ensemble_values_raise_before_anything_else(bad, monkeypatch):
    def no_launch(*a, **k):
        raise AssertionError("a kernel was launched")
    monkeypatch.setattr(K, "_launch", no_launch)
    img = np.zeros((16, 16, 3), np.uint8)
    with pytest.raises(ValueError, match="ensemble"):
        restore.restore_image(lambda x: x, img, ensemble=bad)
    with pytest.raises(ValueError, match="ensemble"):
        restore.restore_images(lambda x: x, [img], ensemble=bad)
    with pytest.raises(ValueError, match="ensemble"):
        restore.evaluate(lambda x: x, [img.astype(np.float32)], ensemble=bad)
    with pytest.raises(ValueError, match="ensemble"):
        restore.evaluate(lambda x: x, [img.astype(np.float32)], across_images=True, ensemble=bad)
    with pytest.raises(ValueError, match="ensemble"):
        restore.plan_images([(16, 16)], modes=bad)


def test_good_ensemble_values():
    assert restore._ensemble_modes("t", 1) == (0,) == restore._ensemble_modes("t", (0,)) == restore._ensemble_modes("t", None)
    assert restore._ensemble_modes("t", 8) == tuple(range(8)) == restore._ensemble_modes("t", range(8))
    assert restore._ensemble_modes("t", [np.int64(1), 4]) == (1, 4)


# ---- 3. the C ABI
def modes_of(*ms):
    return (ctypes.c_int32 * max(1, len(ms)))(*ms)


def gather(lib, arena, modes=(0, 1), img=PTR, f32=0, h=16, w=16, c=3, table=PTR, n=1, n_modes=None, bh=16, bw=16, out=PTR,
           elems=768, img_table=PTR, n_img=1):
    ms = None if modes is None else modes_of(*modes)
    n_modes = (0 if modes is None else len(modes)) if n_modes is None else n_modes
    if arena:
        return lib.grr_tiles_gather_d8(img, elems, f32, c, img_table, n_img, table, n, ms, n_modes, bh, bw, out, None)
    return lib.grr_tile_gather_d8(img, f32, h, w, c, table, n, ms, n_modes, bh, bw, out, None)


def mean(lib, arena, modes=(0, 2), y0=PTR, y1=PTR, table=PTR, n=1, n_modes=None, n_even=None, n_odd=None, th=16, tw=16,
         img=PTR, f32=0, h=16, w=16, c=3, elems=768, img_table=PTR, n_img=1):
    ms = None if modes is None else modes_of(*modes)
    listed = () if modes is None else modes
    n_modes = len(listed) if n_modes is None else n_modes
    n_even = sum(m in E.EVEN for m in listed) if n_even is None else n_even
    n_odd = sum(m in E.ODD for m in listed) if n_odd is None else n_odd
    if arena:
        return lib.grr_tiles_scatter_mean(y0, y1, table, n, ms, n_modes, n_even, n_odd, th, tw, img, elems, f32, c,
                                          img_table, n_img, None)
    return lib.grr_tile_scatter_mean(y0, y1, table, n, ms, n_modes, n_even, n_odd, th, tw, img, f32, h, w, c, None)


NAMES = {(gather, False): b"grr_tile_gather_d8", (gather, True): b"grr_tiles_gather_d8",
         (mean, False): b"grr_tile_scatter_mean", (mean, True): b"grr_tiles_scatter_mean"}
ENTRIES = sorted(NAMES, key=NAMES.get)


@pytest.mark.parametrize("fn,arena", ENTRIES, ids=[NAMES[e].decode() for e in ENTRIES])
def test_entry_points_refuse_bad_arguments(lib, fn, arena):
    name = NAMES[fn, arena]

    def refused(status, **over):
        assert fn(lib, arena, **over) == status, over
        msg = lib.grr_last_error()
        assert msg.startswith(name + b": "), msg
        return msg

    # NULLs
    for ptr in ("img", "table", "modes") + (("out",) if fn is gather else ("y0", "y1")) + (("img_table",) if arena else ()):
        assert b"bad args" in refused(INVALID_ARG, **{ptr: None}), ptr
    # sizes and the dtype selector
    for bad in (dict(f32=2), dict(f32=-1), dict(c=0), dict(n=0), dict(n=-2)) + \
            ((dict(bh=0), dict(bw=-1)) if fn is gather else (dict(th=0), dict(tw=-1))) + \
            ((dict(elems=0), dict(n_img=0)) if arena else (dict(h=0), dict(w=0))):
        refused(INVALID_ARG, **bad)
    refused(INVALID_ARG, table=PTR + 2)
    refused(INVALID_ARG, img=PTR + 2, f32=1)
    if fn is gather:
        refused(INVALID_ARG, out=PTR + 2)
    else:
        refused(INVALID_ARG, y0=PTR + 2)
        refused(INVALID_ARG, y1=PTR + 1)
    # C = 5
    assert b"C <= 4" in refused(UNSUPPORTED, c=5)
    # the mode list
    assert b"outside 0..7" in refused(INVALID_ARG, modes=(8,))
    assert b"outside 0..7" in refused(INVALID_ARG, modes=(-1,))
    assert b"ascending" in refused(INVALID_ARG, modes=(4, 1))
    assert b"ascending" in refused(INVALID_ARG, modes=(1, 1))
    assert b"1..8 modes" in refused(INVALID_ARG, modes=(0,), n_modes=0)                 # M = 0
    assert b"1..8 modes" in refused(INVALID_ARG, modes=(0,), n_modes=-1)
    assert b"1..8 modes" in refused(INVALID_ARG, modes=tuple(range(8)) + (8,), n_modes=9)
    if fn is gather:
        assert b"orientation" in refused(INVALID_ARG, modes=(0, 2))                    # mixed orientation
        assert b"orientation" in refused(INVALID_ARG, modes=(1, 4, 7))
    else:
        assert b"M0 + M1" in refused(INVALID_ARG, modes=(0, 2), n_even=1, n_odd=2)       # M0 + M1 != M
        assert b"M0 + M1" in refused(INVALID_ARG, modes=(0, 2), n_even=2, n_odd=0)       # the sum is M, the split is not
        assert b"M0 + M1" in refused(INVALID_ARG, modes=(0, 1), n_even=1, n_odd=1)
        refused(INVALID_ARG, modes=(0, 1), y0=None)                                      # a batch that is needed
        refused(INVALID_ARG, modes=(2,), y1=None)
    # one element past the 2^31 window-batch bound: n M C th tw = 2^31, and the largest batch that passes the
    # bound is refused only later, for the arguments behind it
    size = dict(bh=512, bw=512) if fn is gather else dict(th=512, tw=512)
    even4, even2 = (0, 1, 4, 5), (0, 1)
    full = dict(modes=even4) if fn is gather else dict(modes=(0, 1, 2, 4, 5))
    assert b"window batch" in refused(UNSUPPORTED, c=4, n=512, **size, **full)          # 512 x 4 x 4 x 512 x 512
    assert b"window batch" in refused(UNSUPPORTED, c=4, n=1024, modes=even2, **size)
    assert b"window batch" in refused(UNSUPPORTED, c=1, n=1 << 30, modes=even2, **size)  # n M alone reaches 2^31
    assert b"window batch" not in refused(INVALID_ARG, c=4, n=511, f32=2, **size, **full)


def test_a_call_without_modes_it_needs_not_is_taken_up_to_the_launch(lib):
    """An orientation without a mode needs no batch: NULL y1 with even modes only is not an argument error (the
    image pointers are; nothing is launched)."""
    assert mean(lib, False, modes=(0, 1), y1=None, img=None) == INVALID_ARG
    assert b"bad args" in lib.grr_last_error()
    assert mean(lib, False, modes=(2, 3), y0=None, img=None) == INVALID_ARG
    assert mean(lib, False, modes=(0, 1), y1=None, c=5) == UNSUPPORTED


# ---- the wrappers
def pack_of(dtype=torch.uint8):
    host = ((0, 16, 16), (768, 17, 31))
    return SimpleNamespace(arena=torch.zeros(768 + 17 * 31 * 3, dtype=dtype), table=torch.tensor(host, dtype=torch.int64),
                           host_table=host, c=3)


ROWS6, ROWS7 = torch.zeros(1, 6, dtype=torch.int32), torch.zeros(1, 7, dtype=torch.int32)


def test_wrappers_refuse_cpu_tensors_and_wrong_dtypes_before_any_launch(monkeypatch):
    def no_launch(*a, **k):
        raise AssertionError("a kernel was launched")
    monkeypatch.setattr(K, "_launch", no_launch)
    img = torch.zeros(16, 16, 3, dtype=torch.uint8)
    y0, y1 = torch.zeros(2, 3, 16, 32), torch.zeros(1, 3, 32, 16)
    with pytest.raises(RuntimeError, match="GPU"):
        K.tile_gather_d8(img, ROWS6, (0, 1), 16, 16)
    with pytest.raises(RuntimeError, match="GPU"):
        K.tiles_gather_d8(pack_of(), ROWS7, (2,), 16, 16)
    with pytest.raises(RuntimeError, match="GPU"):
        K.tile_scatter_mean(y0, y1, ROWS6, (0, 1, 2), 16, 32, img)
    with pytest.raises(RuntimeError, match="GPU"):
        K.tiles_scatter_mean(y0, y1, ROWS7, (0, 1, 2), 16, 32, pack_of())
    # dtypes and shapes
    with pytest.raises(ValueError, match="uint8 or float32"):
        K.tile_gather_d8(img.to(torch.int16), ROWS6, (0,), 16, 16)
    with pytest.raises(ValueError, match="uint8 or float32"):
        K.tile_scatter_mean(y0, y1, ROWS6, (0, 1, 2), 16, 32, img.to(torch.float64))
    with pytest.raises(ValueError, match="arena"):
        K.tiles_gather_d8(pack_of(torch.int16), ROWS7, (0,), 16, 16)
    with pytest.raises(ValueError, match="C <= 4"):
        K.tile_gather_d8(torch.zeros(16, 16, 5, dtype=torch.uint8), ROWS6, (0,), 16, 16)
    for fn, first in ((K.tile_gather_d8, img), (K.tiles_gather_d8, pack_of())):
        rows = ROWS6 if fn is K.tile_gather_d8 else ROWS7
        for bad in ((), (8,), (1, 0), (0, 0), (0, 2), (0, 1, 3), 3, (0, 1, 4, 5, 6)):
            with pytest.raises(ValueError, match="modes"):
                fn(first, rows, bad, 16, 16)
    for fn, last in ((K.tile_scatter_mean, img), (K.tiles_scatter_mean, pack_of())):
        rows = ROWS6 if fn is K.tile_scatter_mean else ROWS7
        for bad in ((), (8,), (1, 0), (0, 0), None):
            with pytest.raises(ValueError, match="modes"):
                fn(y0, y1, rows, bad, 16, 32, last)
