"""grr_u8_demosaic / grr_u8_demosaic_images on the GPU against the oracle tests/demosaic_ref.py (whose two forms
tests/test_demosaic_ref.py holds to each other): the operator is exact integer arithmetic, so any mismatching byte is a
failure.

Shapes (tests/test_demosaic_ref.py lists them): from 1 x 1, where the reflection folds every neighbour onto the one
sample, over thin and odd pictures to every combination of rows around one tile with columns beyond one and two tiles,
and the transposed set -- the kernel's tile comes from kernels.DEMOSAIC_TILE.  Odd widths put most rows of the output
at addresses that are no multiple of 4 (the byte path); widths that are multiples of 4 take the packed stores.  All 4
patterns, all 3 fills; random bytes, a smooth picture, and random 0 / 255, which reaches both clamps."""
import numpy as np
import pytest
import torch

from irdu_amd import kernels
from tests import demosaic_ref as ref
from tests.test_demosaic_ref import contents, shapes

TILE = kernels.DEMOSAIC_TILE        # the shapes straddle the kernel's own tile

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import irdu_amd
    irdu_amd.load_native()
    from irdu_amd import kernels, restore
    return type("G", (), dict(K=kernels, R=restore, I=irdu_amd))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def mismatches(got, want):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.uint8, (got.shape, want.shape)
    return int(np.count_nonzero(got != want))


@pytest.mark.parametrize("hw", shapes(TILE) + [(TILE[0] + 3, 2 * TILE[1] + 8)])
def test_the_filled_mosaic_is_the_oracle_bit_for_bit(G, hw):
    for content, a in contents(*hw).items():
        t = dev(a)
        for pat in ref.PATTERNS:
            for fill in ref.FILLS:
                bad = mismatches(G.K.u8_demosaic(t, pat, fill), ref.degrade(a, pat, fill))
                print(f"{hw} {pat} {fill} {content}: {bad} mismatching bytes")
                assert bad == 0, (content, pat, fill)


@pytest.mark.parametrize("hw", [(1, 1), (2, 9), (7, 13), (TILE[0] + 1, TILE[1] + 4), (TILE[0] + 2, 2 * TILE[1] + 3)])
def test_a_mosaic_plane_gives_what_its_picture_gives(G, hw):
    a = contents(*hw)["random"]
    for code, pat in enumerate(ref.PATTERNS):
        m = ref.mosaic(a, pat).astype(np.uint8)
        for fcode, fill in enumerate(ref.FILLS):
            want = G.K.u8_demosaic(dev(a), pat, fill)
            assert mismatches(want, ref.degrade(a, pat, fill)) == 0
            assert torch.equal(G.K.u8_demosaic(dev(m), code, fcode), want)                 # H x W, codes for names
            assert torch.equal(G.K.u8_demosaic(dev(m[:, :, None]), pat, fill), want)       # H x W x 1
    assert torch.equal(G.K.u8_demosaic(dev(a), "grbg"), G.K.u8_demosaic(dev(a), "grbg", "malvar"))      # the default


def test_restore_entry_point_takes_numpy_and_tensors_and_returns_their_kind(G):
    a = contents(50, 70)["smooth"]
    want = ref.degrade(a, "gbrg", "malvar")
    out = G.R.demosaic_u8(a, "gbrg")
    assert isinstance(out, np.ndarray) and np.array_equal(out, want)
    out = G.I.demosaic_u8(torch.from_numpy(a), "gbrg", "malvar")
    assert isinstance(out, torch.Tensor) and not out.is_cuda and np.array_equal(out.numpy(), want)
    out = G.I.demosaic_u8(dev(a), 2, 2)
    assert out.is_cuda and mismatches(out, want) == 0
    # a view that is not contiguous is copied first, as a tensor and as an array
    wide = np.concatenate([a, a], axis=1)
    assert mismatches(G.K.u8_demosaic(dev(wide)[:, :70], "gbrg"), want) == 0
    assert mismatches(G.I.demosaic_u8(dev(wide)[:, :70], "gbrg"), want) == 0
    assert np.array_equal(G.I.demosaic_u8(wide[:, :70], "gbrg"), want)
    assert np.array_equal(G.I.demosaic_u8(wide[::2, ::2], "rggb", "bilinear"),
                          ref.degrade(np.ascontiguousarray(wide[::2, ::2]), "rggb", "bilinear"))
    # a raw plane, 2-D and 3-D, of each kind
    m = ref.mosaic(a, "bggr").astype(np.uint8)
    want = ref.degrade(a, "bggr", "bilinear")
    out = G.I.demosaic_u8(m, "bggr", "bilinear")
    assert isinstance(out, np.ndarray) and out.shape == (50, 70, 3) and np.array_equal(out, want)
    out = G.I.demosaic_u8(torch.from_numpy(m[:, :, None]), "bggr", "bilinear")
    assert isinstance(out, torch.Tensor) and not out.is_cuda and np.array_equal(out.numpy(), want)
    assert mismatches(G.I.demosaic_u8(dev(m), "bggr", "bilinear"), want) == 0


ARENA = [(7, 13), (67, 131), (5, 3), (40, 25)]         # the second image starts at byte 273: an odd address
ARENA_P = ["gbrg", "rggb", "bggr", "grbg"]


@pytest.mark.parametrize("fill", ref.FILLS)
def test_the_arena_form_is_the_single_image_result_with_a_pattern_per_image(G, fill):
    pics = [contents(h, w)["random" if k % 2 else "binary"] for k, (h, w) in enumerate(ARENA)]
    pack = G.R.pack_images(pics, DEV)
    assert pack.host_table[1][0] % 2 == 1
    out = G.K.u8_demosaic_images(pack, ARENA_P, fill)
    assert out.host_table == pack.host_table and out.table is pack.table and out.arena is not pack.arena
    for i, (a, p) in enumerate(zip(pics, ARENA_P)):
        bad = mismatches(out.image(i), ref.degrade(a, p, fill))
        print(f"arena {fill} image {i} {a.shape[:2]} {p}: {bad} mismatching bytes")
        assert bad == 0, i
        assert torch.equal(out.image(i), G.K.u8_demosaic(dev(a), p, fill))
    # one pattern for all, by name and by code, and the patterns as a device tensor, whose values the kernel clamps
    same = G.K.u8_demosaic_images(pack, "grbg", fill)
    coded = G.K.u8_demosaic_images(pack, [1, 1, 1, 1], fill)
    loose = G.K.u8_demosaic_images(pack, torch.tensor([2, 250, -3, 1], dtype=torch.int32, device=DEV), fill)
    assert torch.equal(same.arena, coded.arena)
    for i, (a, p) in enumerate(zip(pics, ["gbrg", "bggr", "rggb", "grbg"])):
        assert mismatches(same.image(i), ref.degrade(a, "grbg", fill)) == 0
        assert mismatches(loose.image(i), ref.degrade(a, p, fill)) == 0
    # a pack whose images do not lie back to back: the bytes between them stay 0
    gap = G.R.ImagePack(torch.cat([pack.arena, pack.arena]), torch.tensor([(5, 7, 13)], dtype=torch.int64).to(DEV),
                        ((5, 7, 13),), 3)
    moved = G.K.u8_demosaic_images(gap, ["bggr"], fill)
    assert mismatches(moved.image(0), ref.degrade(gap.image(0).cpu().numpy(), "bggr", fill)) == 0
    assert int(moved.arena[:5].max()) == 0 and int(moved.arena[5 + 7 * 13 * 3:].max()) == 0


def test_two_runs_are_identical(G):
    a = dev(contents(130, 70)["random"])
    runs = [G.K.u8_demosaic(a, "rggb") for _ in range(2)]
    assert torch.equal(runs[0], runs[1])
    pack = G.R.pack_images([contents(h, w)["random"] for h, w in ARENA], DEV)
    packs = [G.K.u8_demosaic_images(pack, ARENA_P) for _ in range(2)]
    assert torch.equal(packs[0].arena, packs[1].arena)
