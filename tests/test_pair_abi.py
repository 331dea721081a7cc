"""CPU-only checks of grr_patch_pair_batch (csrc/image_ops.hip) and kernels.patch_pair_batch: the Python mirror of
the shape query, argument validation before any launch, and the wrapper's host checks.  Launches nothing."""
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


def args(input_arena=PTR, target_arena=PTR + 0x1000, elems=768, c=3, img_table=PTR, n_img=1, table=PTR, ids=PTR,
         sigma=PTR, n=1, seed=2204, ph=16, pw=16, target=PTR, input=PTR):
    return (input_arena, target_arena, elems, c, img_table, n_img, table, ids, sigma, n, seed, ph, pw, target, input, None)


def test_python_mirror_of_the_shape_query(lib):
    """A call on each side of every bound of grr_patch_pair_batch_supported."""
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
        got = bool(lib.grr_patch_pair_batch_supported(*case))
        assert K.patch_pair_batch_ok(*case) == got, case
        assert got == bool(lib.grr_patch_batch_supported(*case)), case
        seen.add(got)
    assert seen == {True, False}
    assert K.patch_pair_batch_ok(3, 1, 768, 32, 512, 512) and not K.patch_pair_batch_ok(4, 1, 768, 2048, 512, 512)


def test_bad_arguments_report_their_status_without_a_launch(lib):
    assert lib.grr_patch_pair_batch(*args(c=5)) == UNSUPPORTED
    assert b"grr_patch_pair_batch" in lib.grr_last_error() and b"C <= 4" in lib.grr_last_error()
    for bad in (dict(n=0), dict(ph=0), dict(pw=0), dict(c=0), dict(n_img=0), dict(elems=0), dict(n=-1)):
        assert lib.grr_patch_pair_batch(*args(**bad)) == INVALID_ARG, bad
        assert b"grr_patch_pair_batch: bad args" in lib.grr_last_error()
    for name in ("input_arena", "target_arena", "img_table", "table", "ids", "target", "input"):
        assert lib.grr_patch_pair_batch(*args(**{name: None})) == INVALID_ARG, name
        assert b"grr_patch_pair_batch: bad args" in lib.grr_last_error()
    # a null sigma is legal (no noise): the call gets past "bad args" to the next check that fails
    assert lib.grr_patch_pair_batch(*args(sigma=None, c=5)) == UNSUPPORTED
    assert lib.grr_patch_pair_batch(*args(sigma=None, table=PTR + 2)) == INVALID_ARG
    assert b"aligned" in lib.grr_last_error()
    # the same arena twice is legal too
    assert lib.grr_patch_pair_batch(*args(target_arena=PTR, ids=PTR + 4)) == INVALID_ARG
    assert b"aligned" in lib.grr_last_error()
    # n C ph pw = 2^31
    assert lib.grr_patch_pair_batch(*args(c=4, n=2048, ph=512, pw=512)) == UNSUPPORTED
    assert b"below 2^31" in lib.grr_last_error()
    assert lib.grr_patch_pair_batch(*args(c=1, n=8192, ph=512, pw=512)) == UNSUPPORTED
    assert lib.grr_patch_pair_batch(*args(n_img=769)) == UNSUPPORTED           # more images than elements
    assert lib.grr_patch_pair_batch(*args(elems=1 << 62)) == UNSUPPORTED
    for bad in (dict(table=PTR + 2), dict(sigma=PTR + 2), dict(target=PTR + 2), dict(input=PTR + 1),
                dict(ids=PTR + 4), dict(img_table=PTR + 4)):
        assert lib.grr_patch_pair_batch(*args(**bad)) == INVALID_ARG, bad
        assert b"aligned" in lib.grr_last_error()
    with pytest.raises(_native.GrrError):
        _native.call("grr_patch_pair_batch", *args(n=0))
    # the entry point it shares its checks with keeps its own name and still needs a sigma
    assert lib.grr_patch_batch(PTR, 768, 3, PTR, 1, PTR, PTR, None, 1, 2204, 16, 16, PTR, PTR, None) == INVALID_ARG
    assert b"grr_patch_batch: bad args" in lib.grr_last_error()


def pack_of(host_table=((0, 16, 16), (768, 5, 7)), c=3, dtype=torch.uint8):
    elems = sum(h * w * c for _, h, w in host_table)
    return SimpleNamespace(arena=torch.zeros(elems, dtype=dtype), host_table=tuple(host_table), c=c,
                           table=torch.tensor(host_table, dtype=torch.int64).reshape(-1, 3))


def test_wrapper_refuses_packs_that_are_no_pair(monkeypatch):
    with pytest.raises(RuntimeError, match="GPU"):           # a CPU arena
        K.patch_pair_source(pack_of(), pack_of())
    monkeypatch.setattr(K, "_check_placed", lambda *a: None)
    src = K.patch_pair_source(pack_of(), pack_of())
    assert isinstance(src, K.PatchPairSource) and src.n_img == 2 and src.c == 3
    assert np.array_equal(src.hw, [(16, 16), (5, 7)])
    one = pack_of()
    assert K.patch_pair_source(one, one).input is one           # the same pack twice is legal
    for first, second in ((pack_of(dtype=torch.float32), pack_of()), (pack_of(), pack_of(dtype=torch.float32))):
        with pytest.raises(ValueError, match="uint8"):
            K.patch_pair_source(first, second)
    with pytest.raises(ValueError, match="image 1 "):        # the second image is turned
        K.patch_pair_source(pack_of(), pack_of(((0, 16, 16), (768, 7, 5))))
    with pytest.raises(ValueError, match="image 0 "):
        K.patch_pair_source(pack_of(((0, 8, 32), (768, 5, 7))), pack_of())
    with pytest.raises(ValueError, match="image 1 .*one pack only"):
        K.patch_pair_source(pack_of(), pack_of(((0, 16, 16),)))
    with pytest.raises(ValueError, match="image 0 .*channel"):
        K.patch_pair_source(pack_of(), pack_of(((0, 16, 16), (256, 5, 7)), c=1))
    with pytest.raises(ValueError, match="patch_pair_source"):
        K.patch_pair_batch(pack_of(), np.array([(0, 0, 0, 0)]), [0], None, 2204, 16, 16)


@pytest.mark.parametrize("rows,ids,sigma,ph,pw,match", [
    ([(2, 0, 0, 0)], [0], [0.1], 16, 16, "image indices"),
    ([(1, 5, 0, 0)], [0], None, 16, 16, "inside"),
    ([(0, 0, -1, 0)], [0], [0.1], 16, 16, "inside"),
    ([(0, 0, 0, 8)], [0], None, 16, 16, "modes"),
    ([(0, 0, 0, 1), (0, 0, 0, 2)], [0, 1], None, 16, 32, "square"),
    ([(0, 0, 0, 0)], [0, 1], None, 16, 16, "one entry per row"),
    ([(0, 0, 0, 0)], [0], [0.1, 0.2], 16, 16, "one entry per row"),
    ([(0, 0, 0, 0)], [0], [-0.1], 16, 16, "sigma"),
    ([(0, 0, 0)], [0], None, 16, 16, "rows"),
    ([(0, 0, 0, 0)], [0], None, 0, 16, "elements"),
    ([(0, 0, 0, 0)] * 2048, list(range(2048)), None, 1024, 1024, "elements"),
])
def test_wrapper_refuses_bad_host_tables_before_any_launch(monkeypatch, rows, ids, sigma, ph, pw, match):
    def no_launch(*a, **k):
        raise AssertionError("a kernel was launched")
    monkeypatch.setattr(K, "_launch", no_launch)
    monkeypatch.setattr(K, "_check_placed", lambda *a: None)       # the packs are on the host here
    src = K.patch_pair_source(pack_of(), pack_of())
    with pytest.raises(ValueError, match="patch_pair_batch.*" + match):
        K.patch_pair_batch(src, np.array(rows), np.array(ids), sigma, 2204, ph, pw)
    with pytest.raises(ValueError, match="seed"):
        K.patch_pair_batch(src, np.array([(0, 0, 0, 0)]), [0], None, 1 << 64, 16, 16)


def test_wrapper_launch_arguments(monkeypatch):
    """What reaches the library: the input arena first, one table, a null sigma for None, numel * 10 bytes."""
    sent = []
    monkeypatch.setattr(K, "_check_placed", lambda *a: None)
    monkeypatch.setattr(K, "_stream", lambda dev: None)
    monkeypatch.setattr(K, "_launch", lambda kind, nbytes, name, *a, **k: sent.append((kind, nbytes, name, a)))
    inp, tgt = pack_of(), pack_of()
    src = K.patch_pair_source(inp, tgt)
    target, got = K.patch_pair_batch(src, np.array([(0, 1, 2, 3), (1, 4, 6, 0)]), [7, 8], None, 2204, 16, 16)
    assert tuple(target.shape) == tuple(got.shape) == (2, 3, 16, 16) and target.dtype == torch.float32
    kind, nbytes, name, a = sent[0]
    assert (kind, nbytes, name) == ("patch_pair_batch", 2 * 3 * 16 * 16 * 10, "grr_patch_pair_batch")
    assert a[:6] == (inp.arena.data_ptr(), tgt.arena.data_ptr(), tgt.arena.numel(), 3, tgt.table.data_ptr(), 2)
    assert a[8] is None and a[9:13] == (2, 2204, 16, 16) and a[13:15] == (target.data_ptr(), got.data_ptr())
    K.patch_pair_batch(src, np.array([(0, 1, 2, 3)]), [7], [0.5], 2204, 16, 16)
    assert sent[1][3][8] is not None
