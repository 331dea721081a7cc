"""grr_u8_resize / grr_u8_resize_images on the GPU against the oracle tests/resize_ref.py: down, up and degrade are
bit-exact, any mismatching byte is a failure.

Shapes: the issue's eight, then one case on each side of the kernel's 32 x 32 output tile in both directions (outputs
of 32 x 33 and 33 x 32, down and up), and 264 x 272 at s = 8, whose down pass fills a whole tile at the largest scale
(the widest span of input columns a block stages: 280 of the 289 it has room for).  Contents: random bytes and a
0 / 255 checkerboard, which overshoots below 0 and above 255 (tests/test_resize_ref.py shows it does)."""
import numpy as np
import pytest
import torch

from tests import resize_ref
from tests.test_resize_ref import SHAPES, checkerboard, random_picture

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TILE_EDGES = [(64, 66, 3, 2), (66, 64, 1, 2), (32, 33, 3, 2), (33, 32, 1, 3), (264, 272, 1, 8)]


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import irdu_amd
    irdu_amd.load_native()
    from irdu_amd import kernels, restore
    assert kernels.RESIZE_TILE == 32            # TILE_EDGES straddle it
    return type("G", (), dict(K=kernels, R=restore, I=irdu_amd))


_REF = {}


def ref(kind, h, w, c, s, content):
    """The oracle's down / up / degrade of one case, computed once and read-only."""
    key = (kind, h, w, c, s, content)
    if key not in _REF:
        a = pictures(h, w, c)[content]
        out = {"down": resize_ref.down, "up": resize_ref.up, "degrade": resize_ref.degrade}[kind](a, s)
        out.setflags(write=False)
        _REF[key] = out
    return _REF[key]


def pictures(h, w, c):
    return {"random": random_picture(h, w, c), "checker": checkerboard(h, w, c)}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def mismatches(got, want):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.uint8, (got.shape, want.shape)
    return int(np.count_nonzero(got != want))


@pytest.mark.parametrize("h,w,c,s", SHAPES + TILE_EDGES)
def test_down_up_and_degrade_are_the_oracle_bit_for_bit(G, h, w, c, s):
    for content, a in pictures(h, w, c).items():
        t = dev(a)
        low = G.K.u8_resize(t, s, False)
        assert tuple(low.shape) == (-(-h // s), -(-w // s), c)
        assert mismatches(low, ref("down", h, w, c, s, content)) == 0, ("down", content)
        assert mismatches(G.K.u8_resize(t, s, True), ref("up", h, w, c, s, content)) == 0, ("up", content)
        want = ref("degrade", h, w, c, s, content)
        assert mismatches(G.K.u8_resize(low, s, True, (h, w)), want) == 0, ("up to H x W", content)
        assert mismatches(G.K.u8_bicubic_degrade(t, s), want) == 0, ("degrade", content)


def test_restore_entry_points_take_numpy_and_tensors_and_return_their_kind(G):
    h, w, c, s = 67, 131, 3, 4
    a = random_picture(h, w, c)
    low = G.R.bicubic_down_u8(a, s)
    assert isinstance(low, np.ndarray) and np.array_equal(low, ref("down", h, w, c, s, "random"))
    back = G.R.bicubic_up_u8(torch.from_numpy(low), s, h, w)
    assert isinstance(back, torch.Tensor) and not back.is_cuda
    assert np.array_equal(back.numpy(), ref("degrade", h, w, c, s, "random"))
    full = G.I.bicubic_up_u8(dev(a), s)
    assert full.is_cuda and mismatches(full, ref("up", h, w, c, s, "random")) == 0
    assert np.array_equal(G.I.bicubic_degrade_u8(a, s), ref("degrade", h, w, c, s, "random"))
    # a view that is not contiguous is copied first
    wide = dev(np.concatenate([a, a], axis=1))
    assert mismatches(G.K.u8_resize(wide[:, :w], s, False), ref("down", h, w, c, s, "random")) == 0
    with pytest.raises(ValueError, match="bicubic_down_u8.*uint8"):
        G.R.bicubic_down_u8(a.astype(np.float32), s)
    with pytest.raises(ValueError, match="scale"):
        G.R.bicubic_up_u8(a, 9)


ARENA = [(7, 13), (67, 131), (5, 3)]         # the second image starts at byte 273: an odd address


@pytest.mark.parametrize("s", (3, 4))
def test_the_arena_form_is_the_single_image_result_whatever_else_it_holds(G, s):
    c = 3
    pics = [random_picture(h, w, c, seed=k) for k, (h, w) in enumerate(ARENA)]
    pack = G.R.pack_images(pics, DEV)
    assert [off for off, _, _ in pack.host_table] == [0, 273, 26604]
    low = G.K.u8_resize_images(pack, s, False)
    full = G.K.u8_resize_images(pack, s, True)
    degraded = G.K.u8_bicubic_degrade_images(pack, s)
    assert degraded.host_table == pack.host_table and degraded.table is pack.table
    for i, a in enumerate(pics):
        assert mismatches(low.image(i), resize_ref.down(a, s)) == 0
        assert mismatches(full.image(i), resize_ref.up(a, s)) == 0
        want = resize_ref.degrade(a, s)
        assert mismatches(degraded.image(i), want) == 0
        assert torch.equal(degraded.image(i), G.K.u8_bicubic_degrade(dev(a), s))
    # the same pictures in another order, with another one among them
    other = [pics[2], checkerboard(40, 24, c), pics[0], pics[1]]
    again = G.K.u8_bicubic_degrade_images(G.R.pack_images(other, DEV), s)
    for i, k in ((0, 2), (2, 0), (3, 1)):
        assert torch.equal(again.image(i), degraded.image(k))
    assert mismatches(again.image(1), resize_ref.degrade(other[1], s)) == 0
    # a pack whose images do not lie back to back keeps its own table
    gap = G.R.ImagePack(torch.cat([pack.arena, pack.arena]), torch.tensor([(5, 7, 13)], dtype=torch.int64).to(DEV),
                        ((5, 7, 13),), c)
    moved = G.K.u8_bicubic_degrade_images(gap, s)
    assert moved.host_table == ((0, 7, 13),) and moved.table is not gap.table
    assert mismatches(moved.image(0), resize_ref.degrade(gap.image(0).cpu().numpy(), s)) == 0


def test_two_runs_are_identical(G):
    a = dev(random_picture(130, 70, 3))
    runs = [G.K.u8_bicubic_degrade(a, 2) for _ in range(2)]
    assert torch.equal(runs[0], runs[1])
    pack = G.R.pack_images([random_picture(h, w, 3, seed=k) for k, (h, w) in enumerate(ARENA)], DEV)
    packs = [G.K.u8_bicubic_degrade_images(pack, 4) for _ in range(2)]
    assert torch.equal(packs[0].arena, packs[1].arena)
