"""grr_u8_blur / grr_u8_blur_images on the GPU against the oracle tests/blur_ref.py (whose two forms
tests/test_blur_ref.py holds to each other): the operator is exact integer arithmetic, so any mismatching byte is a
failure -- there is no tolerance.

Shapes (tests/test_blur_ref.py lists them): heights of 1, 2, 3, 7, 15, 16, 17, 31, 33 by widths of 1, 2, 5, 63, 64, 65,
129 -- below, at and above the kernel's 16 x 64 tile, more than one tile each way, widths that are no multiple of a
lane's 4 bytes, and pictures narrower than a kernel's radius (2 x 2 under 31 x 31: several folds of every boundary).
Every kernel of KERNELS under every boundary runs every shape; the channel count (1, 3, 4) and the byte offsets of the
source and the destination from an aligned base (0 or 1 each) rotate with the shape, so that each case sees all of them.
The library is called on buffers with a guard of eight bytes at either end, which must stay as they were."""
import numpy as np
import pytest
import torch

from irdu_amd import kernels
from tests import blur_ref as ref
from tests.test_blur_ref import CHANNELS, KERNELS, SHAPES, picture, table_of

TILE = kernels.BLUR_TILE

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD, MARK = 8, 0xA5


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import irdu_amd
    irdu_amd.load_native()
    from irdu_amd import _native, kernels, restore, training
    return type("G", (), dict(K=kernels, R=restore, I=irdu_amd, N=_native, T=training))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def mismatches(got, want):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == np.uint8, (got.shape, want.shape)
    return int(np.count_nonzero(got != want))


def blur_at(G, a, table, boundary, src_off=0, dst_off=0):
    """grr_u8_blur itself on ``a`` placed src_off bytes into an aligned buffer, the result dst_off bytes into another;
    the guards of both buffers are checked."""
    h, w, c = a.shape
    n = a.size
    src = np.full(n + 2 * GUARD, MARK, np.uint8)
    src[GUARD + src_off:GUARD + src_off + n] = a.ravel()
    s, d = dev(src), torch.full((n + 2 * GUARD,), MARK, dtype=torch.uint8, device=DEV)
    assert s.data_ptr() % 16 == 0 and d.data_ptr() % 16 == 0
    wd = dev(np.ascontiguousarray(table, dtype=np.int32))
    G.N.call("grr_u8_blur", s.data_ptr() + GUARD + src_off, h, w, c, d.data_ptr() + GUARD + dst_off, wd.data_ptr(),
             table.shape[0], table.shape[1], ref.BOUNDARIES.index(boundary), torch.cuda.current_stream().cuda_stream)
    out = d.cpu().numpy()
    assert np.array_equal(s.cpu().numpy(), src)                                    # the source is not written
    assert (out[:GUARD + dst_off] == MARK).all() and (out[GUARD + dst_off + n:] == MARK).all()
    return out[GUARD + dst_off:GUARD + dst_off + n].reshape(a.shape)


@pytest.mark.parametrize("boundary", ref.BOUNDARIES)
@pytest.mark.parametrize("name", list(KERNELS))
def test_the_blurred_picture_is_the_oracle_bit_for_bit(G, name, boundary):
    table = table_of(name)
    ki, bi = list(KERNELS).index(name), ref.BOUNDARIES.index(boundary)
    seen = set()
    total = 0
    for si, (h, w) in enumerate(SHAPES):
        c = CHANNELS[(si + ki) % 3]
        src_off, dst_off = (si + bi) & 1, ((si + bi) >> 1) & 1
        seen.add((c, src_off, dst_off))
        a = picture(si, h, w, c)
        bad = mismatches(blur_at(G, a, table, boundary, src_off, dst_off), ref.blur(a, table, boundary))
        total += bad
        assert bad == 0, (name, boundary, h, w, c, src_off, dst_off)
    print(f"{name} {boundary}: {len(SHAPES)} shapes, {total} mismatching bytes")
    assert {s[0] for s in seen} == set(CHANNELS) and {s[1:] for s in seen} == {(0, 0), (0, 1), (1, 0), (1, 1)}


@pytest.mark.parametrize("boundary", ref.BOUNDARIES)
def test_the_identity_a_shift_and_constant_pictures(G, boundary):
    a = picture(5, 33, 65, 3)
    assert mismatches(blur_at(G, a, KERNELS["identity"], boundary, 1, 1), a) == 0          # the output is the input
    # the lone tap at (0, 2) of a 3 x 3 table: out[y, x] = src[y + 1, x - 1]; a correlation would go the other way
    got = blur_at(G, a, KERNELS["shift"], boundary)
    rows = ref.indices(1, 34, 33, boundary)
    cols = ref.indices(-1, 64, 65, boundary)
    assert mismatches(got, a[rows][:, cols]) == 0
    if boundary == "wrap":
        assert mismatches(got, np.roll(a, (-1, 1), axis=(0, 1))) == 0
    for value in (0, 255):
        for (h, w, c) in ((2, 2, 3), (17, 65, 4), (33, 129, 1)):
            flat = np.full((h, w, c), value, np.uint8)
            for name in ("random31x31", "gaussian:25:1.6", "motion:15:30", "distinct3x5"):
                assert mismatches(blur_at(G, flat, table_of(name), boundary, 1, 0), flat) == 0, (value, name, h, w, c)


def test_the_wrappers_take_tensors_arrays_and_kernel_records(G):
    a = picture(9, 50, 70, 3)
    k = G.T.parse_blur_spec("motion:15:30")
    want = ref.blur(a, np.array(k.table), "reflect")
    assert mismatches(G.K.u8_blur(dev(a), k, "reflect"), want) == 0
    assert mismatches(G.K.u8_blur(dev(a), np.array(k.table), 2), want) == 0
    assert mismatches(G.K.u8_blur(dev(a[:, :, 0]), k, "reflect"), want[:, :, 0]) == 0       # H x W
    out = G.R.blur_u8(a, "motion:15:30", "reflect")
    assert isinstance(out, np.ndarray) and np.array_equal(out, want)
    out = G.I.blur_u8(torch.from_numpy(a), k, "reflect")
    assert isinstance(out, torch.Tensor) and not out.is_cuda and np.array_equal(out.numpy(), want)
    out = G.I.blur_u8(dev(a), k.table, 2)
    assert out.is_cuda and mismatches(out, want) == 0
    assert np.array_equal(G.I.blur_u8(a[:, :, 1], k, "reflect"), want[:, :, 1])
    assert np.array_equal(G.I.blur_u8(a, k), ref.blur(a, np.array(k.table), "wrap"))      # the default boundary
    wide = np.concatenate([a, a], axis=1)                   # a view that is not contiguous is copied first
    assert mismatches(G.K.u8_blur(dev(wide)[:, :70], k, "reflect"), want) == 0
    assert np.array_equal(G.T.blur_degrade_u8(a, k, "reflect"), want)


ARENA = [(7, 13), (67, 131), (5, 3), (40, 25), (1, 1), (33, 65), (2, 2)]      # the second image starts at an odd byte
ARENA_K = ["distinct3x5", "column31x1", "gaussian:25:1.6"]                     # three kernels of unlike sides
ARENA_OF = [0, 2, 1, 1, 2, 0, 1]


@pytest.mark.parametrize("c", (3, 1))
@pytest.mark.parametrize("boundary", ref.BOUNDARIES)
def test_the_arena_form_is_the_single_image_result_with_a_kernel_per_image(G, boundary, c, monkeypatch):
    pics = [picture(40 + k, h, w, c) for k, (h, w) in enumerate(ARENA)]
    tables = [table_of(name) for name in ARENA_K]
    want = [ref.blur(a, tables[k], boundary) for a, k in zip(pics, ARENA_OF)]
    pack = G.R.pack_images(pics, DEV)
    assert pack.host_table[1][0] % 2 == 1
    out = G.K.u8_blur_images(pack, tables, ARENA_OF, boundary)
    assert out.host_table == pack.host_table and out.table is pack.table and out.arena is not pack.arena and out.c == c
    for i in range(len(pics)):
        bad = mismatches(out.image(i), want[i])
        print(f"arena {boundary} C {c} image {i} {pics[i].shape[:2]} kernel {ARENA_K[ARENA_OF[i]]}: {bad} mismatching bytes")
        assert bad == 0, i
    # kernel records for tables, one kernel for all, and the indices as a device tensor, whose values the kernel clamps
    records = [G.T.BlurKernel(t) for t in tables]
    assert torch.equal(G.K.u8_blur_images(pack, records, ARENA_OF, boundary).arena, out.arena)
    same = G.K.u8_blur_images(pack, records[0], 0, boundary)
    loose = G.K.u8_blur_images(pack, tables, torch.tensor([0, 250, -3, 1, 2, 0, 1], dtype=torch.int32, device=DEV), boundary)
    for i, (a, k) in enumerate(zip(pics, [0, 2, 0, 1, 2, 0, 1])):
        assert mismatches(same.image(i), ref.blur(a, tables[0], boundary)) == 0
        assert mismatches(loose.image(i), ref.blur(a, tables[k], boundary)) == 0
    # the chunks of at most MAX_BLUR_IMAGES images, with the limit patched down: the same arena from four launches
    sent = []
    launch = G.K._launch
    monkeypatch.setattr(G.K, "_launch", lambda *a, **k: (sent.append(a[3 + 3]), launch(*a, **k)))
    monkeypatch.setattr(G.K, "MAX_BLUR_IMAGES", 2)
    assert torch.equal(G.K.u8_blur_images(pack, tables, ARENA_OF, boundary).arena, out.arena) and sent == [2, 2, 2, 1]


def test_the_arena_form_leaves_every_byte_outside_the_images_untouched(G):
    """The library call itself on a destination arena full of a mark: images that do not lie back to back."""
    pics = [picture(60 + k, h, w, 3) for k, (h, w) in enumerate(ARENA)]
    tables = [table_of(name) for name in ARENA_K]
    offsets, at = [], 5
    for a in pics:
        offsets.append(at)
        at += a.size + 3
    elems = at + 11
    host = np.full(elems, MARK, np.uint8)
    for a, off in zip(pics, offsets):
        host[off:off + a.size] = a.ravel()
    rows = tuple((off, a.shape[0], a.shape[1]) for a, off in zip(pics, offsets))
    src, dst = dev(host), torch.full((elems,), MARK, dtype=torch.uint8, device=DEV)
    table = torch.tensor(rows, dtype=torch.int64).to(DEV)
    slots = np.zeros((3, 31, 31), np.int32)
    for slot, t in zip(slots, tables):
        slot[:t.shape[0], :t.shape[1]] = t
    weights, sizes = dev(slots), dev(np.array([t.shape for t in tables], np.int32))
    of = dev(np.array(ARENA_OF, np.int32))
    G.N.call("grr_u8_blur_images", src.data_ptr(), elems, table.data_ptr(), len(pics), max(r[1] for r in rows),
             max(r[2] for r in rows), 3, dst.data_ptr(), weights.data_ptr(), sizes.data_ptr(), 3, of.data_ptr(), 1,
             torch.cuda.current_stream().cuda_stream)
    out = dst.cpu().numpy()
    inside = np.zeros(elems, bool)
    for a, off, k in zip(pics, offsets, ARENA_OF):
        inside[off:off + a.size] = True
        assert mismatches(out[off:off + a.size].reshape(a.shape), ref.blur(a, tables[k], "replicate")) == 0
    assert (out[~inside] == MARK).all() and np.array_equal(src.cpu().numpy(), host)
    # through the wrapper the bytes between the images are 0
    gap = G.R.ImagePack(src, table, rows, 3)
    moved = G.K.u8_blur_images(gap, tables, ARENA_OF, "replicate")
    assert np.array_equal(moved.arena.cpu().numpy()[inside], out[inside]) and int(moved.arena.cpu().numpy()[~inside].max()) == 0


def test_two_runs_are_identical(G):
    a = dev(picture(3, 130, 70, 3))
    runs = [G.K.u8_blur(a, table_of("random31x31"), "wrap") for _ in range(2)]
    assert torch.equal(runs[0], runs[1])
