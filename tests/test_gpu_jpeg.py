"""grr_u8_jpeg / grr_u8_jpeg_images and grr_u8_blocking on the GPU against the oracle tests/jpeg_ref.py (which
tests/test_jpeg_ref.py holds to Pillow byte for byte): the round trip is bit-exact, any mismatching byte is a failure;
the blocking sums are equal as integers and PSNR-B is within 1e-12 relative of the restatement's float64.

Shapes (tests/test_jpeg_ref.py lists them): gray and 4:4:4 from 1 x 1 over sides that are no multiples of 8 to one case
on each side of the kernel's 32 x 32 tile in both directions; 4:2:0 on both sides of the chroma-width rule (replication
for a chroma width <= 2), odd sides, 40 x 25 -- which tells the padding columns (the last full-resolution column) from
the padding rows (the last chroma row) -- thin pictures and the tile-straddling ones, where the triangle filter reads
the recomputed halo.  Qualities 1, 10, 50, 90, 100; random bytes and the 0 / 255 checkerboard, which reaches both
clamps."""
import numpy as np
import pytest
import torch

from tests import jpeg_ref
from tests.test_jpeg_ref import MODES, QUALITIES, TILE, hand_picture, pictures, random_picture, smooth_picture, tent_picture

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import irdu_amd
    irdu_amd.load_native()
    from irdu_amd import kernels, restore
    assert kernels.JPEG_TILE == TILE            # the shapes of tests/test_jpeg_ref.py straddle it
    return type("G", (), dict(K=kernels, R=restore, I=irdu_amd))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def mismatches(got, want):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.uint8, (got.shape, want.shape)
    return int(np.count_nonzero(got != want))


@pytest.mark.parametrize("c,sub,hw", MODES)
def test_the_round_trip_is_the_oracle_bit_for_bit(G, c, sub, hw):
    for content, a in pictures(*hw, c).items():
        t = dev(a)
        for q in QUALITIES:
            bad = mismatches(G.K.u8_jpeg(t, q, sub), jpeg_ref.degrade(a, q, sub))
            print(f"{hw} C {c} sub {sub} q {q} {content}: {bad} mismatching bytes")
            assert bad == 0, (content, q)


def test_restore_entry_point_takes_numpy_and_tensors_and_returns_their_kind(G):
    a = smooth_picture(50, 70, 3)
    want = jpeg_ref.degrade(a, 20, 2)
    out = G.R.jpeg_degrade_u8(a, 20, 2)
    assert isinstance(out, np.ndarray) and np.array_equal(out, want)
    out = G.I.jpeg_degrade_u8(torch.from_numpy(a), 20, 2)
    assert isinstance(out, torch.Tensor) and not out.is_cuda and np.array_equal(out.numpy(), want)
    out = G.I.jpeg_degrade_u8(dev(a), 20, 2)
    assert out.is_cuda and mismatches(out, want) == 0
    # a view that is not contiguous is copied first; a gray picture ignores the subsampling
    wide = dev(np.concatenate([a, a], axis=1))
    assert mismatches(G.K.u8_jpeg(wide[:, :70], 20, 2), want) == 0
    gray = a[:, :, :1]
    assert mismatches(G.K.u8_jpeg(dev(gray), 30, 2), jpeg_ref.degrade(gray, 30, 0)) == 0


ARENA = [(7, 13), (67, 131), (5, 3), (40, 25)]         # the second image starts at byte 273: an odd address
ARENA_Q = [10, 90, 1, 40]


@pytest.mark.parametrize("c,sub", [(1, 0), (3, 0), (3, 2)])
def test_the_arena_form_is_the_single_image_result_with_a_quality_per_image(G, c, sub):
    pics = [random_picture(h, w, c, seed=k) for k, (h, w) in enumerate(ARENA)]
    pack = G.R.pack_images(pics, DEV)
    out = G.K.u8_jpeg_images(pack, ARENA_Q, sub)
    assert out.host_table == pack.host_table and out.table is pack.table and out.arena is not pack.arena
    for i, (a, q) in enumerate(zip(pics, ARENA_Q)):
        assert mismatches(out.image(i), jpeg_ref.degrade(a, q, sub)) == 0, i
        assert torch.equal(out.image(i), G.K.u8_jpeg(dev(a), q, sub))
    # one quality for all, and the qualities as a device tensor, whose values the kernel clamps into 1..100
    same = G.K.u8_jpeg_images(pack, 10, sub)
    loose = G.K.u8_jpeg_images(pack, torch.tensor([10, 250, -3, 40], dtype=torch.int32, device=DEV), sub)
    for i, (a, q) in enumerate(zip(pics, [10, 100, 1, 40])):
        assert mismatches(same.image(i), jpeg_ref.degrade(a, 10, sub)) == 0
        assert mismatches(loose.image(i), jpeg_ref.degrade(a, q, sub)) == 0
    # a pack whose images do not lie back to back: the bytes between them stay 0
    gap = G.R.ImagePack(torch.cat([pack.arena, pack.arena]), torch.tensor([(5, 7, 13)], dtype=torch.int64).to(DEV),
                        ((5, 7, 13),), c)
    moved = G.K.u8_jpeg_images(gap, [50], sub)
    assert mismatches(moved.image(0), jpeg_ref.degrade(gap.image(0).cpu().numpy(), 50, sub)) == 0
    assert int(moved.arena[:5].max()) == 0 and int(moved.arena[5 + 7 * 13 * c:].max()) == 0


def test_two_runs_are_identical(G):
    a = dev(random_picture(130, 70, 3))
    runs = [G.K.u8_jpeg(a, 10, 2) for _ in range(2)]
    assert torch.equal(runs[0], runs[1])
    pack = G.R.pack_images([random_picture(h, w, 3, seed=k) for k, (h, w) in enumerate(ARENA)], DEV)
    packs = [G.K.u8_jpeg_images(pack, ARENA_Q, 2) for _ in range(2)]
    assert torch.equal(packs[0].arena, packs[1].arena)
    sums = [G.K.u8_blocking(runs[0]) for _ in range(2)]
    assert sums[0] == sums[1]


BLOCKING = [("hand", hand_picture(1)), ("hand3", hand_picture(3)), ("tent", tent_picture(17, 23, 3)),
            ("degraded", None), ("random", random_picture(37, 51, 1)), ("rows", random_picture(300, 9, 3)),
            ("thin", random_picture(1, 40, 3))]


def blocking_picture(name, a):
    return jpeg_ref.degrade(smooth_picture(64, 66, 3), 10, 0) if a is None else a


@pytest.mark.parametrize("name,a", BLOCKING)
def test_the_blocking_sums_are_the_restatement_as_integers(G, name, a):
    a = blocking_picture(name, a)
    want = jpeg_ref.blocking(a)
    got = G.K.u8_blocking(dev(a))
    print(f"{name}: {got}")
    assert got == want and all(isinstance(v, int) for v in got)


def test_the_arena_form_of_the_blocking_sums(G):
    pics = [blocking_picture(n, a) for n, a in BLOCKING if blocking_picture(n, a).shape[2] == 3]
    got = G.K.u8_blocking_images(G.R.pack_images(pics, DEV))
    assert got == [jpeg_ref.blocking(a) for a in pics]


def test_psnrb_is_the_restatement_within_1e_12(G):
    clean = smooth_picture(64, 66, 3)
    est = jpeg_ref.degrade(clean, 10, 0)
    tent = tent_picture(17, 23, 3)
    other = tent.copy()
    other[5, 7, 1] ^= 16
    for a, b in ((est, clean), (tent, other), (hand_picture(3), np.zeros((16, 16, 3), np.uint8))):
        want, got = jpeg_ref.psnrb(a, b), G.R.psnrb_u8(a, b)
        print(f"psnrb {got!r} against {want!r}")
        assert abs(got - want) <= 1e-12 * abs(want)
        assert G.I.psnrb_u8(dev(a), torch.from_numpy(b)) == got
    assert G.R.psnrb_u8(tent, tent) == float("inf")
