"""CPU-only checks of the image-arena entry points (csrc/image_ops.hip: grr_tiles_gather, grr_tiles_scatter,
grr_u8_sse_segments, grr_image_arena_supported) and their wrappers: argument validation and the Python mirror
of the shape query.  Loads the library, launches nothing."""
from types import SimpleNamespace

import pytest
import torch

from irdu_amd import _native
from irdu_amd import kernels as K

INVALID_ARG, UNSUPPORTED = 1, 3
PTR = 0x1000        # never dereferenced: validation fails first


@pytest.fixture(scope="module")
def lib():
    return _native.load()


def gather_args(arena=PTR, elems=768, f32=0, c=3, img_table=PTR, n_img=1, table=PTR, n=1, th=16, tw=16, out=PTR):
    return (arena, elems, f32, c, img_table, n_img, table, n, th, tw, out, None)


def scatter_args(y=PTR, table=PTR, n=1, th=16, tw=16, arena=PTR, elems=768, f32=0, c=3, img_table=PTR, n_img=1):
    return (y, table, n, th, tw, arena, elems, f32, c, img_table, n_img, None)


def test_null_pointers_are_invalid_args(lib):
    for name in ("arena", "img_table", "table", "out"):
        assert lib.grr_tiles_gather(*gather_args(**{name: None})) == INVALID_ARG, name
        assert b"grr_tiles_gather: bad args" in lib.grr_last_error()
    for name in ("y", "table", "arena", "img_table"):
        assert lib.grr_tiles_scatter(*scatter_args(**{name: None})) == INVALID_ARG, name
        assert b"grr_tiles_scatter: bad args" in lib.grr_last_error()
    for args in [(None, PTR, 4, PTR, 1, PTR, None), (PTR, None, 4, PTR, 1, PTR, None), (PTR, PTR, 4, None, 1, PTR, None),
                 (PTR, PTR, 4, PTR, 1, None, None)]:
        assert lib.grr_u8_sse_segments(*args) == INVALID_ARG
    with pytest.raises(_native.GrrError):
        _native.call("grr_u8_sse_segments", None, None, 4, None, 1, None, None)


def test_bad_sizes_are_invalid_args(lib):
    assert lib.grr_tiles_gather(*gather_args(f32=2)) == INVALID_ARG            # dtype selector
    assert lib.grr_tiles_scatter(*scatter_args(f32=-1)) == INVALID_ARG
    for bad in (dict(n_img=0), dict(n_img=-3), dict(elems=0), dict(elems=-1), dict(n=0), dict(th=0), dict(tw=0), dict(c=0)):
        assert lib.grr_tiles_gather(*gather_args(**bad)) == INVALID_ARG, bad
        assert lib.grr_tiles_scatter(*scatter_args(**bad)) == INVALID_ARG, bad
    assert lib.grr_tiles_gather(*gather_args(arena=PTR + 2, f32=1)) == INVALID_ARG     # float arena at 2 mod 4
    assert lib.grr_tiles_gather(*gather_args(img_table=PTR + 4)) == INVALID_ARG        # int64 rows 8-byte aligned
    assert lib.grr_tiles_scatter(*scatter_args(table=PTR + 2)) == INVALID_ARG
    assert lib.grr_u8_sse_segments(PTR, PTR, 0, PTR, 1, PTR, None) == INVALID_ARG
    assert lib.grr_u8_sse_segments(PTR, PTR, 4, PTR, 0, PTR, None) == INVALID_ARG
    assert lib.grr_u8_sse_segments(PTR, PTR, 4, PTR, 1, PTR + 4, None) == INVALID_ARG   # sums not 8-byte aligned
    assert lib.grr_u8_sse_segments(PTR, PTR, 4, PTR + 4, 1, PTR, None) == INVALID_ARG   # offsets not 8-byte aligned


def test_unsupported_shapes(lib):
    assert lib.grr_tiles_gather(*gather_args(c=5)) == UNSUPPORTED
    assert b"C <= 4" in lib.grr_last_error()
    assert lib.grr_tiles_scatter(*scatter_args(c=5)) == UNSUPPORTED
    assert lib.grr_tiles_gather(*gather_args(n_img=769)) == UNSUPPORTED         # more images than elements
    assert lib.grr_tiles_scatter(*scatter_args(elems=1 << 62)) == UNSUPPORTED
    # the window batch at 2^31 elements
    assert lib.grr_tiles_gather(*gather_args(c=4, n=2048, th=512, tw=512)) == UNSUPPORTED
    assert b"window batch" in lib.grr_last_error()
    assert lib.grr_tiles_scatter(*scatter_args(c=4, n=8192, th=256, tw=256)) == UNSUPPORTED
    # one grid row per segment
    assert lib.grr_u8_sse_segments(PTR, PTR, 1 << 20, PTR, K.MAX_SSE_SEGMENTS + 1, PTR, None) == UNSUPPORTED
    assert b"65535" in lib.grr_last_error()


def test_python_mirror_of_the_arena_query(lib):
    """kernels.image_arena_ok is what the wrappers enforce; grr_image_arena_supported is what the entry points
    enforce.  A shape on each side of every bound; an arena of more than 2^31 elements is taken."""
    table = [(1, 1, 1), (3, 68, 68 * 481 * 321 * 3), (4, 1, 16), (5, 1, 16), (0, 1, 16), (-1, 1, 16),
             (3, 0, 16), (3, -1, 16), (3, 16, 16), (3, 17, 16), (3, 1, 0), (3, 1, -5),
             (1, 1, 1 << 31), (4, 1000, (1 << 40) + 1), (3, 1, (1 << 62) - 1), (3, 1, 1 << 62),
             (1, (1 << 31) - 1, (1 << 31) - 1), (1, (1 << 31) - 1, (1 << 31) - 2)]
    seen = set()
    for c, n_img, elems in table:
        got = bool(lib.grr_image_arena_supported(c, n_img, elems))
        assert K.image_arena_ok(c, n_img, elems) == got, (c, n_img, elems)
        seen.add(got)
    assert seen == {True, False}
    assert K.image_arena_ok(4, 1000, (1 << 40) + 1) and not K.image_arena_ok(3, 17, 16)


def pack_of(host_table, c=3, elems=None, dtype=torch.uint8, **over):
    elems = sum(h * w * c for _, h, w in host_table) if elems is None else elems
    fields = dict(arena=torch.zeros(elems, dtype=dtype), table=torch.tensor(host_table, dtype=torch.int64).reshape(-1, 3),
                  host_table=tuple(host_table), c=c)
    fields.update(over)
    return SimpleNamespace(**fields)


GOOD = ((0, 16, 16), (768, 17, 31))
ROWS = torch.zeros(1, 7, dtype=torch.int32)


@pytest.mark.parametrize("bad,match", [
    (dict(host_table=((0, 16, 16), (767, 17, 31))), "increasing"),            # overlaps image 0
    (dict(host_table=((-1, 16, 16), (768, 17, 31))), "non-negative"),
    (dict(host_table=((768, 17, 31), (0, 16, 16))), "increasing"),
    (dict(host_table=((0, 16, 16), (769, 17, 31))), "ends at element"),       # one element past the arena
    (dict(host_table=((0, 16, 16), (768, 0, 31))), "image 1"),
    (dict(host_table=()), "images"),
    (dict(c=5), "C <= 4"),
    (dict(arena=torch.zeros(2349, dtype=torch.int16)), "arena"),
    (dict(arena=torch.zeros(2349, 1, dtype=torch.uint8)), "arena"),
    (dict(table=torch.zeros(2, 3, dtype=torch.int32)), "int64"),
    (dict(table=torch.zeros(3, 3, dtype=torch.int64)), "int64"),
])
def test_wrappers_refuse_a_bad_pack_before_any_launch(monkeypatch, bad, match):
    def no_launch(*a, **k):
        raise AssertionError("a kernel was launched")
    monkeypatch.setattr(K, "_launch", no_launch)
    fields = dict(host_table=GOOD)
    fields.update(bad)
    host = fields.pop("host_table")
    pack = pack_of(GOOD, **fields)
    pack.host_table = host
    with pytest.raises(ValueError, match=match):
        K.tiles_gather(pack, ROWS, 16, 16)
    with pytest.raises(ValueError, match=match):
        K.tiles_scatter(torch.zeros(1, 3, 16, 16), ROWS, pack)


def test_wrappers_refuse_cpu_tensors_and_bad_tables():
    pack = pack_of(GOOD)
    with pytest.raises(RuntimeError, match="GPU"):
        K.tiles_gather(pack, ROWS, 16, 16)
    with pytest.raises(RuntimeError, match="GPU"):
        K.tiles_scatter(torch.zeros(1, 3, 16, 16), ROWS, pack)
    with pytest.raises(RuntimeError, match="GPU"):
        K.u8_sse_segments(torch.zeros(8, dtype=torch.uint8), torch.zeros(8, dtype=torch.uint8), [0, 3, 8])
    for offsets in ([0, 5, 3], [-1, 4], [0, 9], [0], []):
        with pytest.raises(ValueError):
            K.u8_sse_segments(torch.zeros(8, dtype=torch.uint8), torch.zeros(8, dtype=torch.uint8), offsets)
    with pytest.raises(ValueError):
        K.u8_sse_segments(torch.zeros(8), torch.zeros(8), [0, 8])
    with pytest.raises(ValueError):
        K.u8_sse_segments(torch.zeros(8, dtype=torch.uint8), torch.zeros(9, dtype=torch.uint8), [0, 8])
    with pytest.raises(ValueError):
        K.u8_sse_segments(torch.zeros(1 << 17, dtype=torch.uint8), torch.zeros(1 << 17, dtype=torch.uint8),
                          list(range(K.MAX_SSE_SEGMENTS + 2)))
