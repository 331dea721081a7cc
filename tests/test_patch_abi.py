"""CPU-only checks of grr_patch_batch (csrc/image_ops.hip) and kernels.patch_batch: the Python mirror of the
shape query, argument validation before any launch, and the wrapper's host checks.  Launches nothing."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from irdu_amd import _native
from irdu_amd import kernels as K

INVALID_ARG, UNSUPPORTED = 1, 3
PTR = 0x1000        # never dereferenced: validation fails first


@pytest.fixture(scope="module")
def lib():
    return _native.load()


def args(arena=PTR, elems=768, c=3, img_table=PTR, n_img=1, table=PTR, ids=PTR, sigma=PTR, n=1, seed=2204, ph=16, pw=16,
         clean=PTR, noisy=PTR):
    return (arena, elems, c, img_table, n_img, table, ids, sigma, n, seed, ph, pw, clean, noisy, None)


def test_python_mirror_of_the_shape_query(lib):
    """A call on each side of every bound of grr_patch_batch_supported."""
    cases = [(3, 1, 768, 1, 16, 16), (1, 1, 1, 1, 1, 1), (4, 1, 16, 1, 16, 16), (5, 1, 16, 1, 16, 16),
             (0, 1, 16, 1, 16, 16), (3, 0, 16, 1, 16, 16), (3, 16, 16, 1, 16, 16), (3, 17, 16, 1, 16, 16),
             (3, 1, 0, 1, 16, 16), (3, 1, (1 << 62) - 1, 1, 16, 16), (3, 1, 1 << 62, 1, 16, 16),
             (3, 1, 768, 0, 16, 16), (3, 1, 768, -1, 16, 16), (3, 1, 768, 1, 0, 16), (3, 1, 768, 1, 16, 0),
             (3, 1, 768, 1, -16, 16), (3, 1, 768, 32, 512, 512),
             (4, 1, 768, 2048, 512, 512), (4, 1, 768, 2047, 512, 512), (1, 1, 768, 8192, 512, 512),
             (1, 1, 768, 8191, 512, 512), (1, 1, 768, 1, 1, (1 << 31) - 1), (1, 1, 768, 1, 2, 1 << 30),
             (3, 1, 768, 1, 1, 715827882), (3, 1, 768, 1, 1, 715827883), (2, 1, 768, 65536, 128, 128),
             (2, 1, 768, 65535, 128, 128), (1, 1, 768, (1 << 31) - 1, (1 << 31) - 1, (1 << 31) - 1),
             (4, 1, 768, 1 << 16, 1 << 15, 1)]
    seen = set()
    for case in cases:
        got = bool(lib.grr_patch_batch_supported(*case))
        assert K.patch_batch_ok(*case) == got, case
        seen.add(got)
    assert seen == {True, False}
    assert K.patch_batch_ok(3, 1, 768, 32, 512, 512) and not K.patch_batch_ok(4, 1, 768, 2048, 512, 512)


def test_bad_arguments_report_their_status_without_a_launch(lib):
    assert lib.grr_patch_batch(*args(c=5)) == UNSUPPORTED
    assert b"grr_patch_batch" in lib.grr_last_error() and b"C <= 4" in lib.grr_last_error()
    for bad in (dict(n=0), dict(ph=0), dict(pw=0), dict(c=0), dict(n_img=0), dict(elems=0), dict(n=-1)):
        assert lib.grr_patch_batch(*args(**bad)) == INVALID_ARG, bad
        assert b"grr_patch_batch: bad args" in lib.grr_last_error()
    for name in ("arena", "img_table", "table", "ids", "sigma", "clean", "noisy"):
        assert lib.grr_patch_batch(*args(**{name: None})) == INVALID_ARG, name
        assert b"grr_patch_batch: bad args" in lib.grr_last_error()
    # n C ph pw = 2^31
    assert lib.grr_patch_batch(*args(c=4, n=2048, ph=512, pw=512)) == UNSUPPORTED
    assert b"below 2^31" in lib.grr_last_error()
    assert lib.grr_patch_batch(*args(c=1, n=8192, ph=512, pw=512)) == UNSUPPORTED
    assert lib.grr_patch_batch(*args(n_img=769)) == UNSUPPORTED           # more images than elements
    assert lib.grr_patch_batch(*args(elems=1 << 62)) == UNSUPPORTED
    for bad in (dict(table=PTR + 2), dict(sigma=PTR + 2), dict(clean=PTR + 2), dict(noisy=PTR + 1),
                dict(ids=PTR + 4), dict(img_table=PTR + 4)):
        assert lib.grr_patch_batch(*args(**bad)) == INVALID_ARG, bad
        assert b"aligned" in lib.grr_last_error()
    with pytest.raises(_native.GrrError):
        _native.call("grr_patch_batch", *args(n=0))


def pack_of(host_table=((0, 16, 16), (768, 5, 7)), c=3, dtype=torch.uint8):
    elems = sum(h * w * c for _, h, w in host_table)
    return SimpleNamespace(arena=torch.zeros(elems, dtype=dtype), host_table=tuple(host_table), c=c,
                           table=torch.tensor(host_table, dtype=torch.int64).reshape(-1, 3))


@pytest.mark.parametrize("rows,ids,sigma,ph,pw,match", [
    ([(2, 0, 0, 0)], [0], [0.1], 16, 16, "image indices"),
    ([(-1, 0, 0, 0)], [0], [0.1], 16, 16, "image indices"),
    ([(1, 5, 0, 0)], [0], [0.1], 16, 16, "inside"),
    ([(1, 0, 7, 0)], [0], [0.1], 16, 16, "inside"),
    ([(0, 0, -1, 0)], [0], [0.1], 16, 16, "inside"),
    ([(0, 0, 0, 8)], [0], [0.1], 16, 16, "modes"),
    ([(0, 0, 0, -1)], [0], [0.1], 16, 16, "modes"),
    ([(0, 0, 0, 1), (0, 0, 0, 2)], [0, 1], [0.1, 0.1], 16, 32, "square"),
    ([(0, 0, 0, 7)], [0], [0.1], 32, 16, "square"),
    ([(0, 0, 0, 0)], [0, 1], [0.1], 16, 16, "one entry per row"),
    ([(0, 0, 0, 0)], [0], [0.1, 0.2], 16, 16, "one entry per row"),
    ([(0, 0, 0, 0)], [0], [-0.1], 16, 16, "sigma"),
    ([(0, 0, 0, 0)], [0], [float("nan")], 16, 16, "sigma"),
    ([(0, 0, 0)], [0], [0.1], 16, 16, "rows"),
    ([(0, 0, 0, 0)], [0], [0.1], 0, 16, "elements"),
    ([(0, 0, 0, 0)] * 2048, list(range(2048)), [0.1] * 2048, 1024, 1024, "elements"),
])
def test_wrapper_refuses_bad_host_tables_before_any_launch(monkeypatch, rows, ids, sigma, ph, pw, match):
    def no_launch(*a, **k):
        raise AssertionError("a kernel was launched")
    monkeypatch.setattr(K, "_launch", no_launch)
    monkeypatch.setattr(K, "_check_placed", lambda *a: None)       # the pack is on the host here
    with pytest.raises(ValueError, match=match):
        K.patch_batch(pack_of(), np.array(rows), np.array(ids), sigma, 2204, ph, pw)


def test_wrapper_refuses_cpu_and_float_arenas(monkeypatch):
    rows = np.array([(0, 0, 0, 0)])
    with pytest.raises(RuntimeError, match="GPU"):
        K.patch_batch(pack_of(), rows, [0], [0.1], 2204, 16, 16)
    monkeypatch.setattr(K, "_check_placed", lambda *a: None)
    with pytest.raises(ValueError, match="uint8"):
        K.patch_batch(pack_of(dtype=torch.float32), rows, [0], [0.1], 2204, 16, 16)
    with pytest.raises(ValueError, match="seed"):
        K.patch_batch(pack_of(), rows, [0], [0.1], 1 << 64, 16, 16)
