"""CPU-only checks of the host side of restore_images (irdu_amd.restore): plan_images and pack_images."""
import numpy as np
import pytest
import torch

import irdu_amd
from irdu_amd import restore

SIZES = [(16, 16), (17, 31), (31, 17), (37, 53), (37, 53), (9, 100)]    # the list every restore_images test uses
TILINGS = [(48, 16), (256, 32)]


@pytest.mark.parametrize("tile,halo", TILINGS)
@pytest.mark.parametrize("micro_batch", [1, 3, 16])
def test_plan_images_owns_every_pixel_once_within_the_budget(tile, halo, micro_batch):
    launches = restore.plan_images(SIZES, 16, tile, halo, micro_batch)
    owned = [np.zeros(s, np.int64) for s in SIZES]
    per_image = [[] for _ in SIZES]
    seen_shapes = []
    for th, tw, rows in launches:
        assert 1 <= len(rows) <= max(1, (micro_batch * tile * tile) // (th * tw))        # the pixel budget
        for row in rows:
            assert len(row) == 7
            i, wr, wc, r0, r1, c0, c1 = row
            p = restore.plan(*SIZES[i], 16, tile, halo)
            assert (p.th, p.tw) == (th, tw)                                               # one window shape
            assert wr <= r0 < r1 <= wr + th and wc <= c0 < c1 <= wc + tw
            owned[i][r0:r1, c0:c1] += 1                                                   # numpy cuts it to H x W
            per_image[i].append(tuple(row[1:]))
        if (th, tw) not in seen_shapes:
            seen_shapes.append((th, tw))
    for i, (h, w) in enumerate(SIZES):
        assert (owned[i] == 1).all(), i
        assert per_image[i] == [tuple(w_) for w_ in restore.plan(h, w, 16, tile, halo).windows]
    # within a group the order is (image, window): a group's launches concatenate to its images in order
    for shape in seen_shapes:
        rows = [r for th, tw, rs in launches if (th, tw) == shape for r in rs]
        want = [(i,) + tuple(w_) for i, s in enumerate(SIZES)
                for p in [restore.plan(*s, 16, tile, halo)] if (p.th, p.tw) == shape for w_ in p.windows]
        assert rows == want


def test_launches_of_one_group_are_full_but_the_last():
    launches = restore.plan_images(SIZES, 16, 48, 16, 3)
    by_shape = {}
    for th, tw, rows in launches:
        by_shape.setdefault((th, tw), []).append(len(rows))
    for (th, tw), counts in by_shape.items():
        cap = max(1, (3 * 48 * 48) // (th * tw))
        assert all(c == cap for c in counts[:-1]) and 1 <= counts[-1] <= cap


def test_a_launch_holds_windows_of_two_images():
    launches = restore.plan_images(SIZES, 16, 48, 16, 3)
    assert any(len({row[0] for row in rows}) > 1 for _, _, rows in launches)
    # one window per image at tile 256: the two 37 x 53 images share theirs
    launches = restore.plan_images(SIZES, 16, 256, 32, 3)
    assert [sorted({row[0] for row in rows}) for th, tw, rows in launches if (th, tw) == (48, 64)] == [[3, 4]]
    assert [(th, tw) for th, tw, _ in launches] == [(16, 16), (32, 32), (48, 64), (16, 112)]    # first appearance


def test_plan_images_raises_where_plan_does():
    for bad in ([(16, 16), (5, 32)], [(0, 16)], [(16, 16), (32, 7)]):
        with pytest.raises(ValueError):
            restore.plan(*bad[-1])
        with pytest.raises(ValueError):
            restore.plan_images(bad)
    with pytest.raises(ValueError):
        restore.plan_images(SIZES, micro_batch=0)
    with pytest.raises(ValueError):
        restore.plan_images([(100, 100)], tile=48, halo=24)         # tile_grid: no core left
    assert restore.plan_images([]) == []


def images(dtype, c, seed=0):
    rs = np.random.RandomState(seed)
    if dtype == np.uint8:
        return [rs.randint(0, 256, (h, w, c)).astype(np.uint8) for h, w in SIZES]
    return [rs.rand(h, w, c).astype(np.float32) for h, w in SIZES]


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("c", [1, 3, 4])
def test_pack_images_is_the_concatenation(dtype, c):
    imgs = images(dtype, c)
    imgs[1] = torch.from_numpy(imgs[1])                                    # a host tensor among arrays
    imgs[2] = np.asfortranarray(imgs[2])                                   # a non-contiguous array
    pack = irdu_amd.pack_images(imgs, device="cpu")
    flat = np.concatenate([np.asarray(im).reshape(-1) for im in imgs])
    assert pack.arena.dtype == (torch.uint8 if dtype == np.uint8 else torch.float32) and pack.arena.dim() == 1
    assert np.array_equal(pack.arena.numpy().view(np.uint8), flat.view(np.uint8))
    offs = np.concatenate([[0], np.cumsum([h * w * c for h, w in SIZES])])
    assert pack.host_table == tuple((int(o), h, w) for o, (h, w) in zip(offs, SIZES))
    assert pack.table.dtype == torch.int64 and pack.table.tolist() == [list(r) for r in pack.host_table]
    assert pack.c == c and len(pack) == len(SIZES) and pack.kinds == ("numpy", "cpu") + ("numpy",) * 4
    if c == 3 and dtype == np.uint8:
        assert pack.host_table[2][0] % 2 == 1                              # 17 31 3 is odd: an odd byte
    for i, im in enumerate(imgs):
        assert np.array_equal(pack.image(i).numpy(), np.asarray(im))


def test_pack_images_names_the_offending_image():
    imgs = images(np.uint8, 3)
    with pytest.raises(ValueError, match="image 2"):
        irdu_amd.pack_images(imgs[:2] + [imgs[2].astype(np.float32)] + imgs[3:], device="cpu")
    with pytest.raises(ValueError, match="image 4"):
        irdu_amd.pack_images(imgs[:4] + [imgs[4][:, :, :1]] + imgs[5:], device="cpu")
    with pytest.raises(ValueError, match="image 1"):
        irdu_amd.pack_images([imgs[0], imgs[1].astype(np.int16)], device="cpu")
    with pytest.raises(ValueError, match="image 0"):
        irdu_amd.pack_images([imgs[0][:, :, 0]], device="cpu")
    with pytest.raises(ValueError):
        irdu_amd.pack_images([], device="cpu")


def test_the_package_exports_the_new_calls():
    for name in ("restore_images", "pack_images", "plan_images"):
        assert getattr(irdu_amd, name) is getattr(restore, name)
