"""The geometric self-ensemble of whole-image restoration on the GPU (irdu_amd.restore ``ensemble=``,
csrc/image_ops.hip's gather_d8 / scatter_mean kernels) against the numpy restatement
(tests/restore_ensemble_ref.py: np.rot90 / np.flip around tests/restore_ref.py, and the pairwise tree)."""
import os

import numpy as np
import pytest
import torch

from tests import restore_ensemble_ref as E
from tests import restore_ref as R
from tests.test_gpu_parity import DEV, perturb_mixture, rel_err
from tests.test_gpu_restore import adversarial_values, bits, fill_windows, make_image, offset_view, table_of

pytestmark = pytest.mark.gpu

SIZES = [(16, 16), (17, 31), (37, 53), (100, 140)]
TILINGS = [(48, 16), (256, 32)]
# (h, w, factor, tile, halo): test_gpu_restore.py's sizes at factor 16, and windows smaller than the kernels' 32-row tile
# with tw % 4 != 0 in both orientations at factor 1 (one window of 5 x 3 / 17 x 31, and 12 x 12 windows)
CASES = [(h, w, 16, t, hl) for h, w in SIZES for t, hl in TILINGS] + \
        [(5, 3, 1, 256, 32), (17, 31, 1, 256, 32), (17, 31, 1, 12, 4)]
CHANNELS = (1, 3, 4)
MODE_SETS = [E.EVEN, E.ODD, (2,), (1, 4)]
ALL = tuple(range(8))
ORDER_VALUES = (1e8, 1, -1e8, 1, 0.5, 3e7, -3e7, 0.25)      # 0.0 under the tree, 2.25 / 8 left to right


@pytest.fixture(scope="module")
def irdu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import irdu_amd
    irdu_amd.load_native()
    return irdu_amd


def batch_shape(p, modes):
    return (p.th, p.tw) if modes[0] in E.EVEN else (p.tw, p.th)


# ---- 5. gather_d8
@pytest.mark.parametrize("dtype", ("uint8", "float32"))
@pytest.mark.parametrize("h,w,factor,tile,halo", CASES)
def test_gather_d8_is_the_restatement_bitwise(irdu, h, w, factor, tile, halo, dtype):
    K = irdu.kernels
    p = irdu.plan(h, w, factor, tile, halo)
    tab = table_of(p)
    for c in CHANNELS:
        img = make_image(h, w, c, dtype, seed=h * 7 + c) if h * w * c >= 256 else \
            make_image(16, 16, c, dtype, seed=c)[:h, :w].copy()
        views = [offset_view(img, off) for off in (range(4) if dtype == "uint8" else (0, 1))]
        for modes in MODE_SETS:
            bh, bw = batch_shape(p, modes)
            want = E.gather_d8(img, p, modes, factor)
            assert want.shape == (len(p.windows) * len(modes), c, bh, bw)
            for off, view in enumerate(views):
                got = K.tile_gather_d8(view, tab, modes, bh, bw).cpu().numpy()
                assert got.shape == want.shape
                assert np.array_equal(bits(got), bits(want)), (c, modes, off)
            if len(p.windows) > 3:          # a few windows at a time, from a table view that starts mid-table
                got = K.tile_gather_d8(views[1], tab[2:5], modes, bh, bw).cpu().numpy()
                assert np.array_equal(bits(got), bits(want[2 * len(modes):5 * len(modes)])), (c, modes)


def test_gather_d8_of_one_window_without_padding_transforms_the_picture(irdu):
    """The frame: a one-window call on a picture that needs no padding equals transforming the picture itself,
    and mode 0 is tile_gather."""
    img = make_image(48, 80, 3, "float32", seed=4)
    p = irdu.plan(48, 80, 16, 256, 32)
    assert len(p.windows) == 1
    dev, tab = torch.from_numpy(img).to(DEV), table_of(p)
    chw = img.transpose(2, 0, 1)
    for m in ALL:
        bh, bw = batch_shape(p, (m,))
        got = irdu.kernels.tile_gather_d8(dev, tab, (m,), bh, bw).cpu().numpy()[0]
        want = np.rot90(chw, m // 2, axes=(1, 2))
        want = want[:, ::-1] if m % 2 else want
        assert np.array_equal(bits(got), bits(np.ascontiguousarray(want))), m
    assert torch.equal(irdu.kernels.tile_gather_d8(dev, tab, (0,), 48, 80), irdu.kernels.tile_gather(dev, tab, 48, 80))


@pytest.mark.parametrize("dtype", ("uint8", "float32"))
def test_arena_gather_d8_equals_the_one_image_entry_point(irdu, dtype):
    K = irdu.kernels
    for c in CHANNELS:
        imgs = [make_image(37, 53, c, dtype, seed=1 + c), make_image(100, 75, c, dtype, seed=2 + c)]
        pack = irdu.pack_images(imgs, DEV)
        for tile, halo in TILINGS:
            launches = irdu.plan_images(pack.shapes(), 16, tile, halo, 4, modes=8)
            table = torch.tensor([r for _, _, rows in launches for r in rows], dtype=torch.int32).to(DEV)
            at = 0
            for th, tw, rows in launches:
                view = table[at:at + len(rows)]
                at += len(rows)
                for modes in MODE_SETS:
                    bh, bw = (th, tw) if modes[0] in E.EVEN else (tw, th)
                    got = K.tiles_gather_d8(pack, view, modes, bh, bw)
                    for k, row in enumerate(rows):
                        one = K.tile_gather_d8(pack.image(row[0]), view[k:k + 1, 1:].contiguous(), modes, bh, bw)
                        assert torch.equal(got[k * len(modes):(k + 1) * len(modes)].view(torch.int32),
                                           one.view(torch.int32)), (c, tile, modes, row)


# ---- 6. scatter_mean
def member_fields(p, c, modes, finite, seed):
    """The members z_j [n, C, th, tw] in the picture's frame: in the first half of the windows all members are
    one adversarial field (their mean is that field for M = 2, 4, 8: the (k + 0.5) / 255 ties are hit exactly),
    in the rest each member is its own field; one window's members are the order-revealing constants."""
    vals = adversarial_values()
    if finite:          # a float32 result is compared bit for bit: no inf - inf, whose NaN's sign is the adder's
        vals = vals[np.isfinite(vals) & (np.abs(vals) < 1e30)]
    n = len(p.windows)
    base = fill_windows(p, c, vals, seed)
    zs = []
    for j in range(len(modes)):
        z = fill_windows(p, c, vals, seed + 17 * (j + 1))
        z[:(n + 1) // 2] = base[:(n + 1) // 2]
        z[n - 1, :, :p.th // 2] = np.float32(ORDER_VALUES[j])
        zs.append(z)
    return zs


def mean_into_view(K, y0, y1, p, modes, c, np_dtype, off):
    """tile_scatter_mean into an H x W x C view ``off`` units into a sentinel-filled buffer; the image, and
    whether the buffer outside the view kept its sentinel."""
    numel = p.h * p.w * c
    sentinel = 171 if np_dtype == np.uint8 else -123.0
    buf = torch.full((numel + 8,), sentinel, dtype=torch.uint8 if np_dtype == np.uint8 else torch.float32, device=DEV)
    out = buf[off:off + numel].view(p.h, p.w, c)
    dev = [None if y is None else torch.from_numpy(y).to(DEV) for y in (y0, y1)]
    K.tile_scatter_mean(dev[0], dev[1], table_of(p), modes, p.th, p.tw, out)
    whole = buf.cpu().numpy()
    guard = np.concatenate([whole[:off], whole[off + numel:]])
    return out.cpu().numpy(), bool((guard == sentinel).all())


@pytest.mark.parametrize("np_dtype", (np.uint8, np.float32))
@pytest.mark.parametrize("modes", [ALL, (0, 3), (2, 6), (0, 1, 2)])
def test_scatter_mean_is_the_restatement_bitwise(irdu, modes, np_dtype):
    quantise = np_dtype == np.uint8
    for h, w, factor, tile, halo in [(37, 31, 16, 48, 16), (37, 53, 16, 48, 16), (100, 140, 16, 256, 32),
                                     (17, 31, 1, 256, 32), (17, 31, 1, 12, 4)]:
        p = irdu.plan(h, w, factor, tile, halo)
        for c in CHANNELS:
            zs = member_fields(p, c, modes, finite=not quantise, seed=w + c)
            if quantise:        # NaN -> 0
                zs[0][np.random.RandomState(c).rand(*zs[0].shape) < 0.05] = np.nan
            y0, y1 = E.members_to_batches(zs, modes)
            want = E.finish(E.tree_mean(zs), p, quantise)
            assert np.array_equal(bits(want), bits(E.scatter_mean(y0, y1, p, modes, quantise)))
            if len(modes) == 8:     # the inputs tell the tree from a left-to-right sum
                seq = E.finish(E.sequential_mean(zs), p, quantise)
                assert not np.array_equal(bits(want), bits(seq))
            for off in ((0, 1, 2, 3) if c == 3 else (1,)):
                got, guard_ok = mean_into_view(irdu.kernels, y0, y1, p, modes, c, np_dtype, off)
                assert guard_ok, "wrote outside the image"
                assert np.array_equal(bits(got), bits(want)), (h, w, tile, c, off)


def test_scatter_mean_forms_the_tree_in_the_listed_order(irdu):
    """Constant members 1e8, 1, -1e8, 1, 0.5, 3e7, -3e7, 0.25: ((z0+z1)+(z2+z3)) + ((z4+z5)+(z6+z7)) is 0.0, a
    left-to-right sum 2.25; a wrong order or a wrong mode-to-slot map gives neither 0.0 nor the subsets' values."""
    p = irdu.plan(37, 53, 16, 48, 16)
    n = len(p.windows)
    f = np.float32
    carried = ((f(1) + f(-1e8)) + f(0.25)) / f(3)           # modes (1, 2, 7): [z0 + z1, z2 carried], float32 steps
    assert carried == f(-1e8) / f(3)
    for modes, want in [(ALL, 0.0), ((0, 1, 2, 3), 0.0), ((4, 5, 6, 7), 0.0), ((1, 2, 7), carried)]:
        zs = [np.full((n, 3, p.th, p.tw), ORDER_VALUES[m], np.float32) for m in modes]
        y0, y1 = E.members_to_batches(zs, modes)
        got, guard_ok = mean_into_view(irdu.kernels, y0, y1, p, modes, 3, np.float32, 0)
        ref = E.tree_mean([np.float32(ORDER_VALUES[m]) for m in modes])
        assert guard_ok and ref == np.float32(want)
        assert np.array_equal(bits(got), bits(np.full((37, 53, 3), ref, np.float32))), modes


@pytest.mark.parametrize("h,w", SIZES)
def test_scatter_mean_ownership_is_the_plans(irdu, h, w):
    """Every (window, mode) is a distinct constant: each output pixel shows the mean of the members of the one
    window whose core owns it."""
    for tile, halo in TILINGS:
        p = irdu.plan(h, w, 16, tile, halo)
        n = len(p.windows)
        own = R.owner_map(p)
        for modes in (ALL, (0, 1, 2), (3, 6)):
            consts = np.arange(n * len(modes), dtype=np.float32).reshape(n, len(modes)) * np.float32(3) + np.float32(1)
            zs = [np.broadcast_to(consts[:, j].reshape(n, 1, 1, 1), (n, 3, p.th, p.tw)).copy() for j in range(len(modes))]
            y0, y1 = E.members_to_batches(zs, modes)
            means = E.tree_mean([consts[:, j] for j in range(len(modes))])
            assert len(set(means.tolist())) == n
            got, guard_ok = mean_into_view(irdu.kernels, y0, y1, p, modes, 3, np.float32, 1)
            assert guard_ok and np.array_equal(got, np.repeat(means[own][:, :, None], 3, axis=2)), (tile, modes)
            zs8 = [z / np.float32(4 * n * len(modes)) for z in zs]
            y0, y1 = E.members_to_batches(zs8, modes)
            got, guard_ok = mean_into_view(irdu.kernels, y0, y1, p, modes, 3, np.uint8, 3)
            assert guard_ok and np.array_equal(got, E.finish(E.tree_mean(zs8), p, True)), (tile, modes)


def test_arena_scatter_mean_equals_the_one_image_entry_point(irdu):
    K = irdu.kernels
    shapes = [(37, 53), (100, 75)]
    for c, dtype in ((3, torch.uint8), (4, torch.float32), (1, torch.uint8)):
        for modes in (ALL, (0, 1, 2)):
            even, odd = E.split(modes)
            host_table, total = irdu.restore._host_table(shapes, c)
            pack = irdu.ImagePack(torch.full((total,), 7, dtype=dtype, device=DEV),
                                  torch.tensor(host_table, dtype=torch.int64).to(DEV), host_table, c)
            ones = [torch.full((h, w, c), 7, dtype=dtype, device=DEV) for h, w in shapes]
            launches = irdu.plan_images(shapes, 16, 48, 16, 4, modes=modes)
            table = torch.tensor([r for _, _, rows in launches for r in rows], dtype=torch.int32).to(DEV)
            at = 0
            gen = torch.Generator(device="cpu").manual_seed(c)
            for th, tw, rows in launches:
                view = table[at:at + len(rows)]
                at += len(rows)
                y0 = torch.rand((len(rows) * len(even), c, th, tw), generator=gen).to(DEV) if even else None
                y1 = torch.rand((len(rows) * len(odd), c, tw, th), generator=gen).to(DEV) if odd else None
                K.tiles_scatter_mean(y0, y1, view, modes, th, tw, pack)
                for k, row in enumerate(rows):
                    K.tile_scatter_mean(None if y0 is None else y0[k * len(even):(k + 1) * len(even)],
                                        None if y1 is None else y1[k * len(odd):(k + 1) * len(odd)],
                                        view[k:k + 1, 1:].contiguous(), modes, th, tw, ones[row[0]])
            for i, one in enumerate(ones):
                assert torch.equal(pack.image(i), one), (c, modes, i)


def test_wrappers_refuse_wrong_batches_before_any_launch(irdu, monkeypatch):
    K = irdu.kernels
    img = torch.zeros(16, 32, 3, dtype=torch.uint8, device=DEV)
    rows = torch.zeros(1, 6, dtype=torch.int32, device=DEV)
    y0, y1 = torch.zeros(2, 3, 16, 32, device=DEV), torch.zeros(1, 3, 32, 16, device=DEV)
    K.tile_scatter_mean(y0, y1, rows, (0, 1, 2), 16, 32, img)           # the good call

    def no_launch(*a, **k):
        raise AssertionError("a kernel was launched")
    monkeypatch.setattr(K, "_launch", no_launch)
    with pytest.raises(ValueError, match="batch"):
        K.tile_scatter_mean(y0, y1, rows, (0, 2), 16, 32, img)            # y0 holds two even members, the list has one
    with pytest.raises(ValueError, match="batch"):
        K.tile_scatter_mean(y0, y1.reshape(1, 3, 16, 32), rows, (0, 1, 2), 16, 32, img)      # y1 is tw x th
    with pytest.raises(ValueError, match="batch"):
        K.tile_scatter_mean(y0, None, rows, (0, 1, 2), 16, 32, img)
    with pytest.raises(ValueError, match="no mode"):
        K.tile_scatter_mean(y0, y1, rows, (0, 1), 16, 32, img)
    with pytest.raises(TypeError):
        K.tile_scatter_mean(y0.double(), y1, rows, (0, 1, 2), 16, 32, img)
    with pytest.raises(ValueError, match="window table"):
        K.tile_scatter_mean(y0, y1, torch.zeros(1, 7, dtype=torch.int32, device=DEV), (0, 1, 2), 16, 32, img)
    with pytest.raises(ValueError, match="window table"):
        K.tile_gather_d8(img, rows.cpu(), (0,), 16, 32)
    with pytest.raises(ValueError, match="orientation"):
        K.tile_gather_d8(img, rows, (0, 2), 16, 32)


# ---- 7. restore_image(ensemble=8)
def model_t(x):
    """Batch-independent, deterministic, and it does not commute with the flips and turns.  Every operation is
    one correctly rounded float32 step, in numpy as on the GPU."""
    r2 = torch.roll(x, 1, 2)
    return x * 0.5 + 0.25 * torch.roll(x, 1, 3) + 0.125 * (r2 * r2)


def model_np(x):
    r2 = np.roll(x, 1, 2)
    return x * np.float32(0.5) + np.float32(0.25) * np.roll(x, 1, 3) + np.float32(0.125) * (r2 * r2)


def test_the_test_model_does_not_commute_with_the_modes():
    x = np.random.RandomState(0).rand(1, 1, 6, 6).astype(np.float32)
    for m in range(1, 8):
        assert not np.array_equal(E.inverse(model_np(E.transform(x, m)), m), model_np(x)), m
    pointwise = lambda a: a * a + np.float32(0.1)  # noqa: E731
    for m in range(8):
        assert np.array_equal(E.inverse(pointwise(E.transform(x, m)), m), pointwise(x))


@pytest.mark.parametrize("dtype", ("uint8", "float32"))
@pytest.mark.parametrize("h,w,tile,halo", [(37, 53, 48, 16), (100, 140, 48, 16), (100, 140, 256, 32)])
def test_restore_image_ensemble_is_the_restatement_bitwise(irdu, h, w, tile, halo, dtype):
    img = make_image(h, w, 3, dtype, seed=h + 1)
    p = irdu.plan(h, w, 16, tile, halo)
    assert (len(p.windows) == 1) == (tile == 256)
    for quantise in (True, False):
        want = E.restore(model_np, img, p, ALL, quantise)
        for mb in (16, 3):
            got = irdu.restore_image(model_t, img, tile=tile, halo=halo, micro_batch=mb, quantise=quantise, ensemble=8)
            assert isinstance(got, np.ndarray) and got.dtype == want.dtype
            assert np.array_equal(bits(got), bits(want)), (quantise, mb)
        t = torch.from_numpy(img)
        got = irdu.restore_image(model_t, t, tile=tile, halo=halo, quantise=quantise, ensemble=8, device=DEV)
        assert isinstance(got, torch.Tensor) and not got.is_cuda and np.array_equal(bits(got.numpy()), bits(want))
        got = irdu.restore_image(model_t, t.to(DEV), tile=tile, halo=halo, quantise=quantise, ensemble=range(8))
        assert got.is_cuda and np.array_equal(bits(got.cpu().numpy()), bits(want))
    for modes in ((0, 3), (2, 6), (0, 1, 2), (5,)):
        got = irdu.restore_image(model_t, img, tile=tile, halo=halo, quantise=False, ensemble=modes)
        assert np.array_equal(bits(got), bits(E.restore(model_np, img, p, modes, False))), modes


@pytest.mark.parametrize("dtype", ("uint8", "float32"))
def test_an_equivariant_pointwise_model_gives_the_plain_result_bit_for_bit(irdu, dtype):
    pointwise = lambda x: x * x + 0.1  # noqa: E731
    for h, w, tile, halo in [(37, 53, 48, 16), (100, 140, 48, 16), (100, 140, 256, 32)]:
        img = make_image(h, w, 3, dtype, seed=w)
        for quantise in (True, False):
            plain = irdu.restore_image(pointwise, img, tile=tile, halo=halo, quantise=quantise)
            for ensemble in (8, (0, 1), (2, 3, 6, 7), (1, 6)):
                got = irdu.restore_image(pointwise, img, tile=tile, halo=halo, quantise=quantise, ensemble=ensemble)
                assert np.array_equal(bits(got), bits(plain)), (h, tile, quantise, ensemble)


def test_the_model_sees_two_calls_per_group_within_the_plain_batch(irdu):
    img = make_image(100, 140, 3, "uint8", seed=3)
    p = irdu.plan(100, 140, 16, 48, 16)
    n = len(p.windows)
    for mb, modes in ((16, ALL), (3, ALL), (5, (0, 1, 2)), (4, (2, 6))):
        seen = []

        def recording(x):
            seen.append(tuple(x.shape))
            return model_t(x)
        irdu.restore_image(recording, img, tile=48, halo=16, micro_batch=mb, ensemble=modes)
        even, odd = E.split(modes)
        most = max(len(even), len(odd))
        group = max(1, mb // most)
        want = []
        for i in range(0, n, group):
            g = min(group, n - i)
            want += [(g * len(ms), 3, 48, 48) for ms in (even, odd) if ms]
        assert seen == want
        assert all(s[0] <= max(mb, most) for s in seen)       # no call larger than a plain call's, unless mb < Mo


# ---- 8. restore_images / evaluate
def test_restore_images_ensemble_equals_the_per_image_loop(irdu):
    shapes = [(37, 53), (53, 37), (100, 140), (48, 48)]
    for dtype in ("uint8", "float32"):
        imgs = [make_image(h, w, 3, dtype, seed=5 + i) for i, (h, w) in enumerate(shapes)]
        imgs[1] = np.ascontiguousarray(imgs[0].transpose(1, 0, 2))           # two are transposes of each other
        for tile, halo, mb in ((48, 16, 3), (256, 32, 16)):
            calls = []

            def counting(x):
                calls.append(tuple(x.shape))
                return model_t(x)
            got = irdu.restore_images(counting, imgs, tile=tile, halo=halo, micro_batch=mb, ensemble=8)
            launches = irdu.plan_images(shapes, 16, tile, halo, mb, modes=8)
            assert calls == [(4 * len(rows), 3) + s for th, tw, rows in launches for s in ((th, tw), (tw, th))]
            for im, out in zip(imgs, got):
                one = irdu.restore_image(model_t, im, tile=tile, halo=halo, micro_batch=mb, ensemble=8)
                assert out.dtype == np.uint8 and np.array_equal(out, one)
            got = irdu.restore_images(model_t, imgs, tile=tile, halo=halo, micro_batch=mb, quantise=False, ensemble=(1, 2, 7))
            for im, out in zip(imgs, got):
                one = irdu.restore_image(model_t, im, tile=tile, halo=halo, quantise=False, ensemble=(1, 2, 7))
                assert np.array_equal(bits(out), bits(one))


def test_evaluate_ensemble_gives_the_same_floats_on_both_branches(irdu):
    rs = np.random.RandomState(8)
    images = [rs.rand(h, w, 3).astype(np.float32) for h, w in [(37, 53), (53, 37), (100, 140), (48, 48)]]
    args = dict(sigma=25.0, tile=48, halo=16, micro_batch=3, device=DEV)
    mean8, per8 = irdu.evaluate(model_t, images, ensemble=8, **args)
    mean8a, per8a = irdu.evaluate(model_t, images, ensemble=8, across_images=True, **args)
    assert per8 == per8a and mean8 == mean8a
    mean1, per1 = irdu.evaluate(model_t, images, **args)
    assert per1 != per8                                         # the argument reaches the kernels
    noisy = irdu.restore._noisy(images[0], 25.0, np.random.RandomState(seed=2204))
    out = irdu.restore_image(model_t, noisy, tile=48, halo=16, micro_batch=3, ensemble=8)
    assert per8[0] == irdu.psnr_u8(out, irdu.restore._clean_u8(images[0]))


# ---- 9. the real filter
def test_real_filter_ensemble_against_eight_plain_calls(irdu):
    """ensemble=8 on one unpadded 48 x 80 window against the tree mean of eight plain restore_image calls on
    numpy-transformed pictures, turned back with numpy: the project's 1e-5 relative for the same filter under a
    different batch (here 4 windows per call against 1), not bitwise by contract."""
    torch.manual_seed(31)
    m = irdu.MultiScaleGraphFilter(3, 3, ngraphs=4, n_cgd_iters=3)
    perturb_mixture(m.localfilter, 91)
    m = m.to(DEV).eval()
    img = np.random.RandomState(6).rand(48, 80, 3).astype(np.float32)
    assert len(irdu.plan(48, 80).windows) == 1
    got = irdu.restore_image(m, img, quantise=False, ensemble=8)
    zs = []
    for mode in ALL:
        chw = E.transform(img.transpose(2, 0, 1), mode)
        y = irdu.restore_image(m, np.ascontiguousarray(chw.transpose(1, 2, 0)), quantise=False)
        zs.append(E.inverse(y.transpose(2, 0, 1), mode))
    want = E.tree_mean(zs).transpose(1, 2, 0)
    err = rel_err(torch.from_numpy(got), want)
    print("ensemble=8 vs eight plain calls: rel err", err, "bitwise", bool(np.array_equal(bits(got), bits(want))))
    assert got.shape == (48, 80, 3) and err <= 1e-5
    plain = irdu.restore_image(m, img, quantise=False)
    print("ensemble=8 vs plain: rel diff", rel_err(torch.from_numpy(got), plain))
    assert not np.array_equal(got, plain)


# ---- 10. ensemble=1 and (0,), and the command line
def test_ensemble_1_is_todays_path(irdu, monkeypatch):
    K = irdu.kernels
    imgs = [make_image(37, 53, 3, "uint8", seed=1), make_image(100, 140, 3, "uint8", seed=2)]
    flt = make_image(37, 53, 3, "float32", seed=3)
    before = [irdu.restore_image(model_t, im, tile=48, halo=16, micro_batch=5) for im in imgs]
    before_f = irdu.restore_image(model_t, flt, tile=48, halo=16, quantise=False)

    def forbidden(*a, **k):
        raise AssertionError("an ensemble kernel was launched")
    for name in ("tile_gather_d8", "tiles_gather_d8", "tile_scatter_mean", "tiles_scatter_mean"):
        monkeypatch.setattr(K, name, forbidden)
    for ensemble in (1, (0,), [0], None):
        for im, want in zip(imgs, before):
            got = irdu.restore_image(model_t, im, tile=48, halo=16, micro_batch=5, ensemble=ensemble)
            assert np.array_equal(got, want) and np.array_equal(got, R.restore(model_np, im, irdu.plan(*im.shape[:2], 16, 48, 16)))
        assert np.array_equal(bits(irdu.restore_image(model_t, flt, tile=48, halo=16, quantise=False, ensemble=ensemble)),
                              bits(before_f))
        for got, want in zip(irdu.restore_images(model_t, imgs, tile=48, halo=16, micro_batch=5, ensemble=ensemble), before):
            assert np.array_equal(got, want)
        images = [flt.clip(0, 1)]
        assert irdu.evaluate(model_t, images, tile=48, halo=16, ensemble=ensemble, device=DEV) == \
            irdu.evaluate(model_t, images, tile=48, halo=16, device=DEV)
        assert irdu.evaluate(model_t, images, tile=48, halo=16, ensemble=ensemble, across_images=True, device=DEV) == \
            irdu.evaluate(model_t, images, tile=48, halo=16, across_images=True, device=DEV)
    with pytest.raises(AssertionError, match="ensemble kernel"):
        irdu.restore_image(model_t, imgs[0], ensemble=(1,))


def test_cli_self_ensemble_writes_restore_images_bytes(irdu, tmp_path, capsys):
    from PIL import Image
    from irdu_amd import training as T
    from tests.test_restore_ref import _cli
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    yaml_path = os.path.join(root, "experiment_conf", "example_v1x0_small.yaml")
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    images = {"a": make_image(37, 53, 3, "uint8", 1), "b": make_image(48, 80, 3, "uint8", 2)}
    for name, img in images.items():
        Image.fromarray(img).save(src / f"{name}.png")
    torch.manual_seed(21)
    model = T.build_model(T.parse_options(yaml_path)["model"])
    torch.save({"i": 0, "model": model.state_dict()}, tmp_path / "ckpt.pt")
    model = model.to(DEV).eval()
    cli = _cli()
    base = ["-yaml_path", yaml_path, "--ckpt", str(tmp_path / "ckpt.pt"), "--input", str(src), "--output", str(dst)]

    cli.main(base + ["--self-ensemble"])
    out = capsys.readouterr().out
    for name, img in images.items():
        want = irdu.restore_image(model, img, ensemble=8)
        assert np.array_equal(np.array(Image.open(dst / f"{name}.png")), want)
        assert f"{name}.png  {img.shape[0]}x{img.shape[1]}x3" in out                     # the plain call's line
        assert not np.array_equal(want, irdu.restore_image(model, img))
    cli.main(base + ["--ensemble-modes", "0,1,4,5", "--batch-images"])
    for name, want in zip(images, irdu.restore_images(model, list(images.values()), ensemble=(0, 1, 4, 5))):
        assert np.array_equal(np.array(Image.open(dst / f"{name}.png")), want)
    with pytest.raises(SystemExit):
        cli.main(base + ["--self-ensemble", "--ensemble-modes", "0,1"])
    with pytest.raises(SystemExit):
        cli.main(base + ["--ensemble-modes", "1,0"])
    capsys.readouterr()
