"""Lists of images in shared window batches on the GPU (irdu_amd.restore_images, csrc/image_ops.hip's arena
kernels) against the numpy restatement looped per image (tests/restore_ref.py) and, byte for byte, against the
per-image call."""
import numpy as np
import pytest
import torch

from tests import restore_ref as R
from tests.test_gpu_parity import DEV, perturb_mixture
from tests.test_gpu_restore import adversarial_values, bits, fill_windows, make_image

pytestmark = pytest.mark.gpu

SIZES = [(16, 16), (17, 31), (31, 17), (37, 53), (37, 53), (9, 100)]
TILINGS = [(48, 16), (256, 32)]
CHANNELS = (1, 3, 4)
DTYPES = ("uint8", "float32")
MICRO_BATCH = 3         # at tile 48 the two 37 x 53 images then share a launch (tests/test_restore_images_plan.py)


@pytest.fixture(scope="module")
def irdu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import irdu_amd
    irdu_amd.load_native()
    return irdu_amd


def image_set(c, dtype, seed=0):
    return [make_image(h, w, c, dtype, seed=seed + 11 * i + c) for i, (h, w) in enumerate(SIZES)]


def pack_at(irdu, images_or_total, c, np_dtype, off, fill=0, guard=64):
    """An ImagePack whose arena starts ``guard`` bytes plus ``off`` elements into a byte buffer filled with
    ``fill``; (pack, buffer, arena's byte range).  images_or_total: images to copy in, or SIZES' shapes alone."""
    item = np.dtype(np_dtype).itemsize
    host_table, total = irdu.restore._host_table(SIZES, c)
    buf = torch.full((2 * guard + (total + 4) * item,), fill, dtype=torch.uint8, device=DEV)
    lo = guard + off * item
    arena = buf[lo:lo + total * item].view(torch.uint8 if item == 1 else torch.float32)
    if images_or_total is not None:
        arena.copy_(torch.from_numpy(np.concatenate([im.reshape(-1) for im in images_or_total])))
    assert arena.data_ptr() == buf.data_ptr() + lo and arena.numel() == total
    table = torch.tensor(host_table, dtype=torch.int64).to(DEV)
    return irdu.ImagePack(arena, table, host_table, c), buf, (lo, lo + total * item)


def launch_tables(launches):
    """One device table for all launches, and each launch's view of it (views that start mid-table)."""
    table = torch.tensor([r for _, _, rows in launches for r in rows], dtype=torch.int32).to(DEV)
    views, at = [], 0
    for _, _, rows in launches:
        views.append(table[at:at + len(rows)])
        at += len(rows)
    return views


# ---- 1. gather
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tile,halo", TILINGS)
def test_gather_is_the_restatement_per_image_bitwise(irdu, tile, halo, dtype):
    K = irdu.kernels
    launches = irdu.plan_images(SIZES, 16, tile, halo, MICRO_BATCH)
    views = launch_tables(launches)
    assert any(v.data_ptr() != views[0].data_ptr() for v in views)
    for c in CHANNELS:
        imgs = image_set(c, dtype)
        want = [R.gather(im, irdu.plan(*s, 16, tile, halo)) for im, s in zip(imgs, SIZES)]
        for off in range(4):
            pack, _, _ = pack_at(irdu, imgs, c, imgs[0].dtype, off)
            got = [[] for _ in SIZES]
            for (th, tw, rows), view in zip(launches, views):
                out = K.tiles_gather(pack, view, th, tw).cpu().numpy()
                assert out.shape == (len(rows), c, th, tw)
                for k, row in enumerate(rows):
                    got[row[0]].append(out[k])
            for i in range(len(SIZES)):
                assert np.array_equal(bits(np.stack(got[i])), bits(want[i])), (c, off, i)
        # part of a launch, from a view that starts mid-launch
        th, tw, rows = max(launches, key=lambda l: len(l[2]))
        view = views[launches.index((th, tw, rows))]
        if len(rows) > 1:
            out = K.tiles_gather(pack, view[1:], th, tw).cpu().numpy()
            full = K.tiles_gather(pack, view, th, tw).cpu().numpy()
            assert np.array_equal(bits(out), bits(full[1:]))


# ---- 2. scatter
def window_batches(irdu, launches, c, tile, halo, with_nan, seed):
    """Adversarial values per image window, the launches' batches made of them, and what each image must hold
    (the restatement on the NaN-free values: NaN writes 0)."""
    vals = adversarial_values()
    plans = [irdu.plan(*s, 16, tile, halo) for s in SIZES]
    ys = [fill_windows(p, c, vals, seed + i) for i, p in enumerate(plans)]
    if with_nan:
        for i, y in enumerate(ys):
            y[np.random.RandomState(seed + 100 + i).rand(*y.shape) < 0.1] = np.nan
    nxt = [0] * len(SIZES)
    batches = []
    for th, tw, rows in launches:
        batch = []
        for row in rows:
            assert tuple(row[1:]) == tuple(plans[row[0]].windows[nxt[row[0]]])
            batch.append(ys[row[0]][nxt[row[0]]])
            nxt[row[0]] += 1
        batches.append(torch.from_numpy(np.stack(batch)).to(DEV))
    return plans, ys, batches


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tile,halo", TILINGS)
def test_scatter_writes_every_byte_once_as_the_restatement(irdu, tile, halo, dtype):
    K = irdu.kernels
    np_dtype = np.uint8 if dtype == "uint8" else np.float32
    launches = irdu.plan_images(SIZES, 16, tile, halo, MICRO_BATCH)
    views = launch_tables(launches)
    for c in CHANNELS:
        plans, ys, batches = window_batches(irdu, launches, c, tile, halo, with_nan=dtype == "uint8", seed=7 * c)
        if dtype == "uint8":
            want = [R.scatter(np.where(np.isnan(y), np.float32(0), y), p) for y, p in zip(ys, plans)]
        else:
            want = [R.scatter(y, p, quantise=False) for y, p in zip(ys, plans)]
        want = np.concatenate([w.reshape(-1) for w in want])
        for off in (0, 3):
            arenas = []
            for fill in (0x00, 0xFF):
                pack, buf, (lo, hi) = pack_at(irdu, None, c, np_dtype, off, fill=fill)
                for (th, tw, rows), view, y in zip(launches, views, batches):
                    K.tiles_scatter(y, view, pack)
                whole = buf.cpu().numpy()
                assert lo >= 64 and len(whole) - hi >= 64
                assert (whole[:lo] == fill).all() and (whole[hi:] == fill).all(), "wrote outside the arena"
                arenas.append(whole[lo:hi])
            assert np.array_equal(arenas[0], arenas[1]), "a byte of the arena was not written"
            assert np.array_equal(arenas[0], want.view(np.uint8)), (c, off)


# ---- 3. segmented SSE
def test_u8_sse_segments_is_exact_and_repeats(irdu):
    K = irdu.kernels
    lengths = [1, 15, 16, 17, 4099, 70000, 3]
    offsets = np.concatenate([[0], np.cumsum(lengths)])
    assert [int(o) % 2 for o in offsets[1:6]] == [1, 0, 0, 1, 0] and offsets[5] % 16 != 0
    rs = np.random.RandomState(4)
    a = rs.randint(0, 256, offsets[-1] + 1).astype(np.uint8)
    b = rs.randint(0, 256, offsets[-1] + 1).astype(np.uint8)
    a[offsets[5]:offsets[6]], b[offsets[5]:offsets[6]] = 255, 0
    want = [int(np.square(a[lo:hi].astype(np.int64) - b[lo:hi].astype(np.int64)).sum())
            for lo, hi in zip(offsets[:-1], offsets[1:])]
    assert want[5] == 4_551_750_000 > 1 << 32
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    n = int(offsets[-1])
    first = K.u8_sse_segments(ta[:n], tb[:n], [int(o) for o in offsets])
    assert first == want and all(isinstance(v, int) for v in first)
    assert K.u8_sse_segments(ta[:n], tb[:n], [int(o) for o in offsets]) == first
    # device offsets; arrays one byte into their buffers (the 16-byte words then start elsewhere); arrays of
    # different phase (every byte on its own)
    assert K.u8_sse_segments(ta[:n], tb[:n], torch.from_numpy(offsets.astype(np.int64)).to(DEV)) == want
    for sa, sb in ((1, 1), (1, 0)):
        shifted = [int(np.square(a[sa + lo:sa + hi].astype(np.int64) - b[sb + lo:sb + hi].astype(np.int64)).sum())
                   for lo, hi in zip(offsets[:-1], offsets[1:])]
        assert K.u8_sse_segments(ta[sa:sa + n], tb[sb:sb + n], [int(o) for o in offsets]) == shifted
    # segments need not cover the arrays; an empty one sums to 0
    assert K.u8_sse_segments(ta[:n], tb[:n], [5, 5, 40]) == \
        [0, int(np.square(a[5:40].astype(np.int64) - b[5:40].astype(np.int64)).sum())]
    assert K.u8_sse_segments(ta[:n], ta[:n], [int(o) for o in offsets]) == [0] * len(lengths)


# ---- 4. the whole call against the per-image call
class Counting:
    """Counts the calls of a model and records their batch sizes."""

    def __init__(self, model):
        self.model, self.batches = model, []

    def __call__(self, x):
        self.batches.append(int(x.shape[0]))
        return self.model(x)


@pytest.fixture(scope="module")
def models(irdu):
    torch.manual_seed(13)
    m = irdu.MultiScaleGraphFilter(3, 3, ngraphs=4, n_cgd_iters=1)
    perturb_mixture(m.localfilter, 77)
    return {"pointwise": lambda x: x * x * 0.75 + 0.125,
            "roll": lambda x: torch.roll(x, shifts=(1, 2), dims=(2, 3)),
            "msgf": m.to(DEV).eval()}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["pointwise", "roll", "msgf"])
def test_restore_images_equals_restore_image_byte_for_byte(irdu, models, name, dtype):
    model = models[name]
    imgs = image_set(3, dtype, seed=5)
    for tile, halo in TILINGS:
        launches = irdu.plan_images(SIZES, 16, tile, halo, MICRO_BATCH)
        for quantise in (True, False):
            counted = Counting(model)
            got = irdu.restore_images(counted, imgs, tile=tile, halo=halo, micro_batch=MICRO_BATCH, quantise=quantise)
            assert counted.batches == [len(rows) for _, _, rows in launches]        # one model call per launch
            assert len(counted.batches) < sum(len(irdu.plan(*s, 16, tile, halo).windows) for s in SIZES)
            assert any(len({r[0] for r in rows}) > 1 for _, _, rows in launches)    # windows of two images in one
            assert len(got) == len(imgs)
            for i, im in enumerate(imgs):
                want = irdu.restore_image(model, im, tile=tile, halo=halo, quantise=quantise)
                assert isinstance(got[i], np.ndarray) and got[i].dtype == want.dtype and got[i].shape == want.shape
                assert np.array_equal(bits(got[i]), bits(want)), (name, tile, quantise, i)
    # at tile 256 six images are four model calls: fewer than any per-image loop makes
    counted = Counting(model)
    irdu.restore_images(counted, imgs, tile=256, halo=32, micro_batch=MICRO_BATCH)
    assert len(counted.batches) == 4 < len(imgs)


def test_restore_images_returns_each_inputs_kind_and_restores_the_mode(irdu, models):
    imgs = image_set(3, "uint8", seed=9)
    mixed = [imgs[0], torch.from_numpy(imgs[1]), torch.from_numpy(imgs[2]).to(DEV)] + imgs[3:]
    out = irdu.restore_images(lambda x: x, mixed, tile=48, halo=16)
    assert isinstance(out[0], np.ndarray) and isinstance(out[1], torch.Tensor) and not out[1].is_cuda and out[2].is_cuda
    for o, im in zip(out, imgs):
        assert np.array_equal(o.cpu().numpy() if isinstance(o, torch.Tensor) else o, im)
    m = models["msgf"]
    modes = []
    hook = m.register_forward_pre_hook(lambda mod, args: modes.append(mod.training))
    m.train()
    try:
        irdu.restore_images(m, imgs[:2])
        assert m.training, "the model's mode was not restored"
    finally:
        hook.remove()
        m.eval()
    assert modes and not any(modes), "the model did not run in eval mode"
    with pytest.raises(ValueError, match="returned"):
        irdu.restore_images(lambda x: x[:, :, :8], imgs[:2])
    with pytest.raises(ValueError, match="image 1"):
        irdu.restore_images(lambda x: x, [imgs[0], imgs[1].astype(np.float32)])


# ---- 5. evaluate
def test_evaluate_across_images_returns_the_same_floats(irdu, models):
    from irdu_amd import training as T
    big, small = T.SyntheticTestImages(n_images=3), T.SyntheticTestImages(n_images=3, height=37, width=53, seed=5)
    images = [big[0], small[0], small[1], big[1], small[2], big[2]]
    m = models["msgf"]
    args = dict(sigma=25.0, factor=16, seed=2204, tile=48, halo=16, micro_batch=MICRO_BATCH)
    mean, per_image = irdu.evaluate(m, images, **args)
    mean_b, per_image_b = irdu.evaluate(m, images, across_images=True, **args)
    print("per image:", per_image, "across images:", per_image_b)
    assert len(per_image_b) == 6 and per_image_b == per_image and mean_b == mean
    assert all(np.isfinite(p) for p in per_image)
    assert irdu.evaluate(m, images, across_images=True, **dict(args, tile=256, halo=32)) == \
        irdu.evaluate(m, images, **dict(args, tile=256, halo=32))


# ---- 6. the command line
def test_cli_batch_images_writes_the_same_files_and_lines(irdu, tmp_path, capsys):
    import os
    from PIL import Image
    from irdu_amd import training as T
    from tests.test_restore_ref import _cli
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    yaml_path = os.path.join(root, "experiment_conf", "example_v1x0_small.yaml")
    src = tmp_path / "in"
    src.mkdir()
    for name, (h, w) in {"a": (37, 53), "b": (100, 140), "c": (53, 37)}.items():
        Image.fromarray(make_image(h, w, 3, "uint8", h + w)).save(src / f"{name}.png")
    torch.manual_seed(21)
    model = T.build_model(T.parse_options(yaml_path)["model"])
    torch.save({"i": 0, "model": model.state_dict()}, tmp_path / "ckpt.pt")
    cli = _cli()
    base = ["-yaml_path", yaml_path, "--ckpt", str(tmp_path / "ckpt.pt"), "--input", str(src)]
    for extra in ([], ["--sigma", "25", "--seed", "7"]):
        outs = {}
        for flag in ([], ["--batch-images"]):
            dst = tmp_path / ("out" + "_".join(extra + flag).replace("--", ""))
            cli.main(base + ["--output", str(dst)] + extra + flag)
            outs[bool(flag)] = (capsys.readouterr().out.replace(str(dst), "DST"),
                                {f: (dst / f).read_bytes() for f in sorted(os.listdir(dst))})
        assert sorted(outs[True][1]) == ["a.png", "b.png", "c.png"]
        assert outs[True][1] == outs[False][1]
        assert outs[True][0] == outs[False][0]
        assert ("PSNR" in outs[True][0]) == bool(extra)
