"""The single-image and the arena entry points of csrc/image_ops.hip are instances of one gather body, one
scatter body and one SSE kernel: on one image, with the same legal window rows, they agree bit for bit
(torch.equal on the bytes throughout).

Window rows come from restore.plan at tile 48 with the two halos that tile_grid takes there -- (factor 8,
halo 8) and (factor 16, halo 16); plan(h, w, 16, tile=48, halo=8) itself is a ValueError, the halo being no
multiple of the factor -- and one hand-made 5 x 18 window that crosses the bottom and the right edge (the
scalar planar path, tw % 4 != 0, and the reflected-column path)."""
import numpy as np
import pytest
import torch

from tests.test_gpu_parity import DEV

pytestmark = pytest.mark.gpu

SIZES = [(17, 31), (33, 100), (48, 64)]
CHANNELS = (1, 3, 4)
PLANS = [(8, 48, 8), (16, 48, 16)]          # (factor, tile, halo)
IMAGES = [("uint8", 0), ("uint8", 1), ("float32", 0)]       # dtype, and where in a larger buffer the image starts
GUARD = 16                                   # elements of the buffer behind the image
SSE_NS = (1, 15, 16, 17, 4099)
SSE_PHASES = [(0, 0), (1, 1), (3, 8)]        # both 16-byte aligned; one shared phase; different phases


@pytest.fixture(scope="module")
def irdu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import irdu_amd
    irdu_amd.load_native()
    return irdu_amd


def row_groups(irdu, h, w):
    """[(th, tw, rows6)]: the plans' windows and the hand-made one."""
    groups = []
    for factor, tile, halo in PLANS:
        p = irdu.plan(h, w, factor, tile=tile, halo=halo)
        groups.append((p.th, p.tw, list(p.windows)))
    wr, wc = h - 3, w - 10                   # rows to h + 1 and columns to w + 7: reflect pads smaller than the sides
    groups.append((5, 18, [(wr, wc, wr, wr + 5, wc, wc + 18)]))
    return groups


def tables(rows6):
    t6 = torch.tensor(rows6, dtype=torch.int32).to(DEV)
    t7 = torch.tensor([(0,) + tuple(r) for r in rows6], dtype=torch.int32).to(DEV)
    return t6, t7


def image_in_buffer(h, w, c, dtype, off, fill):
    """(buffer, its H x W x C view that starts ``off`` elements in), the buffer filled with ``fill``."""
    tdtype = torch.uint8 if dtype == "uint8" else torch.float32
    buf = torch.full((h * w * c + off + GUARD,), fill, dtype=tdtype, device=DEV)
    img = buf[off:off + h * w * c].view(h, w, c)
    assert img.data_ptr() == buf.data_ptr() + off * buf.element_size()
    return buf, img


def pack_of(irdu, img):
    """The pack whose arena is this one image's own memory."""
    h, w, c = img.shape
    host = ((0, h, w),)
    return irdu.ImagePack(img.reshape(-1), torch.tensor(host, dtype=torch.int64).to(DEV), host, c)


def raw(t):
    return t.contiguous().view(torch.uint8)


@pytest.mark.parametrize("dtype,off", IMAGES)
@pytest.mark.parametrize("h,w", SIZES)
def test_gather_instances_agree(irdu, h, w, dtype, off):
    K = irdu.kernels
    rs = np.random.RandomState(h + w + off)
    for c in CHANNELS:
        _, img = image_in_buffer(h, w, c, dtype, off, 0)
        src = rs.randint(0, 256, (h, w, c)).astype(np.uint8) if dtype == "uint8" \
            else (rs.rand(h, w, c) * 1.5 - 0.25).astype(np.float32)
        img.copy_(torch.from_numpy(src))
        pack = pack_of(irdu, img)
        assert pack.arena.data_ptr() == img.data_ptr()
        for th, tw, rows6 in row_groups(irdu, h, w):
            t6, t7 = tables(rows6)
            one = K.tile_gather(img, t6, th, tw)
            many = K.tiles_gather(pack, t7, th, tw)
            assert one.shape == (len(rows6), c, th, tw)
            assert torch.equal(raw(one), raw(many)), (c, th, tw)


@pytest.mark.parametrize("dtype,off", IMAGES)
@pytest.mark.parametrize("h,w", SIZES)
def test_scatter_instances_agree_on_every_byte(irdu, h, w, dtype, off):
    K = irdu.kernels
    rs = np.random.RandomState(3 * h + w + off)
    fill = 171 if dtype == "uint8" else -123.0
    for c in CHANNELS:
        for th, tw, rows6 in row_groups(irdu, h, w):
            t6, t7 = tables(rows6)
            y = (rs.rand(len(rows6), c, th, tw) * 3.0 - 1.0).astype(np.float32)      # below 0, above 1
            y[rs.rand(*y.shape) < 0.05] = np.nan
            y[0, 0, th // 2, tw // 2 - 1:tw // 2 + 2] = (-0.5, 1.5, np.nan)
            assert (y < 0).any() and (y > 1).any() and np.isnan(y).any()
            y = torch.from_numpy(y).to(DEV)
            buf_one, img_one = image_in_buffer(h, w, c, dtype, off, fill)
            buf_many, img_many = image_in_buffer(h, w, c, dtype, off, fill)
            K.tile_scatter(y, t6, img_one)
            K.tiles_scatter(y, t7, pack_of(irdu, img_many))
            assert torch.equal(raw(buf_one), raw(buf_many)), (c, th, tw)
            assert not torch.equal(raw(buf_one), raw(torch.full_like(buf_one, fill)))       # something was written
            for buf in (buf_one, buf_many):                                                  # and only in the image
                assert torch.equal(raw(buf[:off]), raw(torch.full_like(buf[:off], fill)))
                assert torch.equal(raw(buf[-GUARD:]), raw(torch.full_like(buf[-GUARD:], fill)))


@pytest.mark.parametrize("n", SSE_NS)
def test_sse_instances_agree_and_are_the_integer_sum(irdu, n):
    K = irdu.kernels
    rs = np.random.RandomState(n)
    for sa, sb in SSE_PHASES:
        ha, hb = (rs.randint(0, 256, n).astype(np.uint8) for _ in range(2))
        ha[0], hb[0] = 255, 0                # the largest difference occurs
        bufa, bufb = (torch.zeros(n + 16, dtype=torch.uint8, device=DEV) for _ in range(2))
        a, b = bufa[sa:sa + n], bufb[sb:sb + n]
        assert a.data_ptr() % 16 == sa and b.data_ptr() % 16 == sb
        a.copy_(torch.from_numpy(ha))
        b.copy_(torch.from_numpy(hb))
        want = int(((ha.astype(np.int64) - hb.astype(np.int64)) ** 2).sum())
        one = K.u8_sse(a, b)
        many = K.u8_sse_segments(a, b, [0, n])[0]
        assert one == many == want, (sa, sb)
