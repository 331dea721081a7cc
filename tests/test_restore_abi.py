"""CPU-only checks of the whole-image I/O entry points (csrc/image_ops.hip): argument validation and the
shape query's Python mirror.  Loads the library, launches nothing."""
import pytest
import torch

from irdu_amd import _native
from irdu_amd import kernels as K

INVALID_ARG, UNSUPPORTED = 1, 3
PTR = 0x1000        # never dereferenced: validation fails first


@pytest.fixture(scope="module")
def lib():
    return _native.load()


def test_null_pointers_are_invalid_args(lib):
    for args in [(None, 0, 16, 16, 3, PTR, 1, 16, 16, PTR, None), (PTR, 0, 16, 16, 3, None, 1, 16, 16, PTR, None),
                 (PTR, 0, 16, 16, 3, PTR, 1, 16, 16, None, None)]:
        assert lib.grr_tile_gather(*args) == INVALID_ARG
        assert b"grr_tile_gather: bad args" in lib.grr_last_error()
    for args in [(None, PTR, 1, 16, 16, PTR, 0, 16, 16, 3, None), (PTR, None, 1, 16, 16, PTR, 0, 16, 16, 3, None),
                 (PTR, PTR, 1, 16, 16, None, 0, 16, 16, 3, None)]:
        assert lib.grr_tile_scatter(*args) == INVALID_ARG
        assert b"grr_tile_scatter: bad args" in lib.grr_last_error()
    for args in [(None, PTR, 4, PTR, None), (PTR, None, 4, PTR, None), (PTR, PTR, 4, None, None)]:
        assert lib.grr_u8_sse(*args) == INVALID_ARG
    with pytest.raises(_native.GrrError):
        _native.call("grr_u8_sse", None, None, 4, None, None)


def test_bad_sizes_are_invalid_args(lib):
    assert lib.grr_tile_gather(PTR, 2, 16, 16, 3, PTR, 1, 16, 16, PTR, None) == INVALID_ARG     # dtype selector
    assert lib.grr_tile_gather(PTR, 0, 0, 16, 3, PTR, 1, 16, 16, PTR, None) == INVALID_ARG
    assert lib.grr_tile_gather(PTR, 0, 16, 16, 3, PTR, 0, 16, 16, PTR, None) == INVALID_ARG
    assert lib.grr_tile_scatter(PTR, PTR, 1, 16, 0, PTR, 0, 16, 16, 3, None) == INVALID_ARG
    assert lib.grr_u8_sse(PTR, PTR, 0, PTR, None) == INVALID_ARG
    assert lib.grr_u8_sse(PTR, PTR, 4, PTR + 4, None) == INVALID_ARG                            # sum not 8-byte aligned
    assert lib.grr_tile_gather(PTR + 2, 1, 16, 16, 3, PTR, 1, 16, 16, PTR, None) == INVALID_ARG  # float image at 2 mod 4


def test_unsupported_shapes(lib):
    assert lib.grr_tile_gather(PTR, 0, 16, 16, 5, PTR, 1, 16, 16, PTR, None) == UNSUPPORTED
    assert b"C <= 4" in lib.grr_last_error()
    assert lib.grr_tile_scatter(PTR, PTR, 1, 16, 16, PTR, 1, 16, 16, 5, None) == UNSUPPORTED
    # the image bound and the window-batch bound, one element past each
    assert lib.grr_tile_gather(PTR, 0, 32768, 16384, 4, PTR, 1, 16, 16, PTR, None) == UNSUPPORTED
    assert lib.grr_tile_gather(PTR, 0, 16, 16, 4, PTR, 2048, 512, 512, PTR, None) == UNSUPPORTED
    assert lib.grr_tile_scatter(PTR, PTR, 8192, 256, 256, PTR, 0, 16, 16, 4, None) == UNSUPPORTED
    assert lib.grr_u8_sse(PTR, PTR, 1 << 31, PTR, None) == UNSUPPORTED


def test_python_mirror_of_the_shape_query(lib):
    """kernels.image_io_ok is what the wrappers and restore_image enforce; grr_image_io_supported is what the
    entry points enforce.  A shape on each side of every bound."""
    table = [(1, 1, 1), (3, 481, 321), (4, 4000, 3000), (4, 16, 16), (5, 16, 16), (0, 16, 16), (-1, 16, 16),
             (3, 0, 16), (3, 16, 0), (3, -4, 16),
             (1, 32768, 65535), (1, 32768, 65536),            # H W C = 2^31 - 32768 | 2^31
             (4, 16384, 32767), (4, 16384, 32768), (3, 26755, 26755), (3, 26754, 26755),
             (1, 1, (1 << 31) - 1), (2, 1, 1 << 30), (2, 1, (1 << 30) - 1),
             (4, 2048 * 512, 511), (4, 2048 * 512, 512)]      # a window batch as (C, n th, tw)
    seen = set()
    for c, h, w in table:
        got = bool(lib.grr_image_io_supported(c, h, w))
        assert K.image_io_ok(c, h, w) == got, (c, h, w)
        seen.add(got)
    assert seen == {True, False}
    assert not K.image_io_ok(3, 26755, 26755) and K.image_io_ok(3, 26754, 26755)


def test_wrappers_refuse_before_any_launch():
    with pytest.raises(ValueError, match="C <= 4"):
        K.tile_gather(torch.zeros(16, 16, 5, dtype=torch.uint8), torch.zeros(1, 6, dtype=torch.int32), 16, 16)
    with pytest.raises(ValueError, match="dtype"):
        K.tile_gather(torch.zeros(16, 16, 3, dtype=torch.int16), torch.zeros(1, 6, dtype=torch.int32), 16, 16)
    with pytest.raises(ValueError, match="dtype"):
        K.tile_scatter(torch.zeros(1, 3, 16, 16), torch.zeros(1, 6, dtype=torch.int32),
                       torch.zeros(16, 16, 3, dtype=torch.float64))
    with pytest.raises(ValueError):
        K.u8_sse(torch.zeros(4), torch.zeros(4))
    with pytest.raises(RuntimeError, match="GPU"):
        K.tile_gather(torch.zeros(16, 16, 3, dtype=torch.uint8), torch.zeros(1, 6, dtype=torch.int32), 16, 16)
