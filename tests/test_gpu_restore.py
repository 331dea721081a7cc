"""Whole-image restoration on the GPU (irdu_amd.restore, csrc/image_ops.hip) against the numpy restatement
(tests/restore_ref.py) and against training.validate()."""
import numpy as np
import pytest
import torch
from torch import nn

from tests import restore_ref as R
from tests.test_gpu_parity import DEV, perturb_mixture, rel_err

pytestmark = pytest.mark.gpu

SIZES = [(16, 16), (17, 31), (37, 53), (100, 140)]
TILINGS = [(48, 16), (256, 32)]        # windows of 48 with 16-pixel halos; one tile that holds every padded image
CHANNELS = (1, 3, 4)
DTYPES = ("uint8", "float32")


@pytest.fixture(scope="module")
def irdu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import irdu_amd
    irdu_amd.load_native()
    return irdu_amd


def make_image(h, w, c, dtype, seed):
    rs = np.random.RandomState(seed)
    if dtype == "uint8":
        img = rs.randint(0, 256, (h, w, c)).astype(np.uint8)
        img.reshape(-1)[:256] = np.arange(256)          # every value occurs
        return img
    img = (rs.rand(h, w, c) * 1.5 - 0.25).astype(np.float32)      # a noisy image leaves [0, 1]
    img.reshape(-1)[:4] = [np.float32(-0.0), np.float32(1e-42), np.float32(3.0), np.float32(-7.5)]
    return img


def offset_view(img, off):
    """A contiguous device copy of img that starts ``off`` units into a larger buffer: bytes for uint8 (any
    byte address); elements for float32, whose tensors cannot sit at an odd byte (4-byte steps walk the four
    16-byte phases instead)."""
    t = torch.from_numpy(img)
    buf = torch.zeros(t.numel() + 8, dtype=t.dtype, device=DEV)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() == buf.data_ptr() + off * t.element_size()
    return v


def table_of(p):
    return torch.tensor(p.windows, dtype=torch.int32).to(DEV)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


# ---- 1. gather
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("h,w", SIZES)
def test_gather_is_the_restatement_bitwise(irdu, h, w, dtype):
    K = irdu.kernels
    for c in CHANNELS:
        img = make_image(h, w, c, dtype, seed=h * 7 + c)
        for tile, halo in TILINGS:
            p = irdu.plan(h, w, 16, tile, halo)
            want = R.gather(img, p)
            tab = table_of(p)
            for off in range(4):
                got = K.tile_gather(offset_view(img, off), tab, p.th, p.tw).cpu().numpy()
                assert got.shape == want.shape
                assert np.array_equal(bits(got), bits(want)), (c, tile, off)
            # a few windows at a time, from a table view that starts mid-table
            if len(p.windows) > 3:
                got = K.tile_gather(offset_view(img, 1), tab[2:5], p.th, p.tw).cpu().numpy()
                assert np.array_equal(bits(got), bits(want[2:5]))
            # a non-contiguous image is copied
            wide = torch.from_numpy(np.concatenate([img, img], axis=1)).to(DEV)
            got = K.tile_gather(wide[:, :w], tab, p.th, p.tw).cpu().numpy()
            assert np.array_equal(bits(got), bits(want))


def test_gather_converts_every_uint8_value_by_a_rounded_division(irdu):
    img = np.arange(256, dtype=np.uint8).reshape(16, 16, 1)
    p = irdu.plan(16, 16)
    got = irdu.kernels.tile_gather(torch.from_numpy(img).to(DEV), table_of(p), 16, 16).cpu().numpy().reshape(-1)
    want = np.arange(256).astype(np.float32) / np.float32(255)
    assert np.array_equal(bits(got), bits(want))


# ---- 2. scatter
def adversarial_values():
    k = np.arange(256, dtype=np.float64)
    ties = ((k + 0.5) / 255.0).astype(np.float32)
    vals = [ties, np.nextafter(ties, np.float32(-np.inf)), np.nextafter(ties, np.float32(np.inf)),
            (k / 255.0).astype(np.float32),
            np.array([-0.0, 0.0, -1e-3, -5.0, -3e38, 1.0, 1.0000001, 1.5, 300.0, 3e38, np.inf, -np.inf,
                      1e-45, -1e-45, 1e-39, 1.1754942e-38, 0.5, 0.49999997, 0.50000006], dtype=np.float32)]
    return np.concatenate(vals).astype(np.float32)


def fill_windows(p, c, values, seed):
    n = len(p.windows) * c * p.th * p.tw
    rs = np.random.RandomState(seed)
    y = values[rs.randint(0, len(values), n)]
    y[:len(values)] = values[:n]
    return rs.permutation(y).reshape(len(p.windows), c, p.th, p.tw).astype(np.float32)


def scatter_into_view(K, y, p, c, np_dtype, off):
    """tile_scatter into an H x W x C view ``off`` units into a sentinel-filled buffer; the image, and whether
    the buffer outside the view kept its sentinel."""
    numel = p.h * p.w * c
    sentinel = 171 if np_dtype == np.uint8 else -123.0
    buf = torch.full((numel + 8,), sentinel, dtype=torch.uint8 if np_dtype == np.uint8 else torch.float32, device=DEV)
    out = buf[off:off + numel].view(p.h, p.w, c)
    K.tile_scatter(torch.from_numpy(y).to(DEV), table_of(p), out)
    whole = buf.cpu().numpy()
    guard = np.concatenate([whole[:off], whole[off + numel:]])
    return out.cpu().numpy(), bool((guard == sentinel).all())


@pytest.mark.parametrize("w", [16, 31, 53])
def test_scatter_uint8_is_img_as_ubyte_of_the_clamped_value_bitwise(irdu, w):
    vals = adversarial_values()
    for c in CHANNELS:
        for tile, halo in TILINGS:
            p = irdu.plan(37, w, 16, tile, halo)
            y = fill_windows(p, c, vals, seed=w + c)
            want = R.scatter(y, p)
            for off in range(4):
                got, guard_ok = scatter_into_view(irdu.kernels, y, p, c, np.uint8, off)
                assert guard_ok, "wrote outside the image"
                assert np.array_equal(got, want), (c, tile, off)


def test_scatter_uint8_writes_zero_for_nan(irdu):
    p = irdu.plan(37, 53, 16, 48, 16)
    y = fill_windows(p, 3, adversarial_values(), seed=9)
    nan = np.random.RandomState(3).rand(*y.shape) < 0.2
    want = R.scatter(np.where(nan, np.float32(0), y), p)
    y[nan] = np.nan
    got, guard_ok = scatter_into_view(irdu.kernels, y, p, 3, np.uint8, 1)
    assert guard_ok and np.array_equal(got, want)


@pytest.mark.parametrize("h,w", SIZES)
def test_scatter_ownership_is_the_plans(irdu, h, w):
    """Windows that are distinct constants: each output pixel shows the one window whose core owns it."""
    for tile, halo in TILINGS:
        p = irdu.plan(h, w, 16, tile, halo)
        n = len(p.windows)
        assert n <= 255
        own = R.owner_map(p)
        idx = np.arange(n, dtype=np.float32).reshape(n, 1, 1, 1)
        y = np.broadcast_to(idx / np.float32(255), (n, 3, p.th, p.tw)).copy()
        got, guard_ok = scatter_into_view(irdu.kernels, y, p, 3, np.uint8, 3)
        assert guard_ok and np.array_equal(got, np.repeat(own[:, :, None], 3, axis=2).astype(np.uint8))
        y = np.broadcast_to(idx, (n, 3, p.th, p.tw)).copy()
        got, guard_ok = scatter_into_view(irdu.kernels, y, p, 3, np.float32, 1)
        assert guard_ok and np.array_equal(got, np.repeat(own[:, :, None], 3, axis=2).astype(np.float32))


@pytest.mark.parametrize("w", [16, 31, 53])
def test_scatter_float32_is_a_bitwise_unclamped_copy(irdu, w):
    vals = adversarial_values()
    for c in CHANNELS:
        for tile, halo in TILINGS:
            p = irdu.plan(37, w, 16, tile, halo)
            y = fill_windows(p, c, vals, seed=2 * w + c)
            want = R.scatter(y, p, quantise=False)
            for off in range(4):
                got, guard_ok = scatter_into_view(irdu.kernels, y, p, c, np.float32, off)
                assert guard_ok and np.array_equal(bits(got), bits(want)), (c, tile, off)


# ---- 3. identity round trip
@pytest.mark.parametrize("h,w", SIZES)
def test_identity_round_trip(irdu, h, w):
    for c in CHANNELS:
        img = make_image(h, w, c, "uint8", seed=h + c)
        flt = make_image(h, w, c, "float32", seed=h + c + 1)
        for tile, halo in TILINGS:
            for mb in (64, 5):
                out = irdu.restore_image(lambda x: x, img, tile=tile, halo=halo, micro_batch=mb)
                assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and np.array_equal(out, img)
            out = irdu.restore_image(lambda x: x, flt, tile=tile, halo=halo, quantise=False)
            assert out.dtype == np.float32 and np.array_equal(bits(out), bits(flt))
            # quantising a float image: the restatement's own round trip
            out = irdu.restore_image(lambda x: x, flt, tile=tile, halo=halo)
            assert np.array_equal(out, R.restore(lambda x: x, flt, irdu.plan(h, w, 16, tile, halo)))
    # the result is of the input's kind
    t = torch.from_numpy(img)
    out = irdu.restore_image(lambda x: x, t)
    assert isinstance(out, torch.Tensor) and not out.is_cuda and torch.equal(out, t)
    out = irdu.restore_image(lambda x: x, t.to(DEV))
    assert out.is_cuda and torch.equal(out.cpu(), t)


# ---- 4. u8_sse
@pytest.mark.parametrize("n", [1, 3, 17, 4099])
def test_u8_sse_is_exact(irdu, n):
    rs = np.random.RandomState(n)
    a, b = rs.randint(0, 256, n + 1).astype(np.uint8), rs.randint(0, 256, n + 1).astype(np.uint8)
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    for sa, sb in ((0, 0), (1, 1), (0, 1)):        # 16-byte aligned operands, and views one byte in
        want = int(np.square(a[sa:sa + n].astype(np.int64) - b[sb:sb + n].astype(np.int64)).sum())
        assert irdu.kernels.u8_sse(ta[sa:sa + n], tb[sb:sb + n]) == want
    assert irdu.kernels.u8_sse(ta, ta) == 0


def test_u8_sse_needs_its_64_bit_sum_and_repeats(irdu):
    n = (1 << 22) + 3
    a = torch.zeros(n, dtype=torch.uint8, device=DEV)
    b = torch.full((n,), 255, dtype=torch.uint8, device=DEV)
    want = n * 255 * 255
    assert want > 1 << 32
    first, second = irdu.kernels.u8_sse(a, b), irdu.kernels.u8_sse(a, b)
    assert first == want and second == want
    assert irdu.kernels.u8_sse(a[1:], b[1:]) == (n - 1) * 255 * 255
    img = np.random.RandomState(0).randint(0, 256, (37, 53, 3)).astype(np.uint8)
    other = np.random.RandomState(1).randint(0, 256, (37, 53, 3)).astype(np.uint8)
    sse = int(np.square(img.astype(np.int64) - other).sum())
    assert irdu.psnr_u8(img, other) == pytest.approx(10 * np.log10(255.0 ** 2 * img.size / sse), rel=0, abs=1e-9)
    assert irdu.psnr_u8(img, img) == float("inf")


# ---- 5 / 6. against validate()
def validate_lines(model, noisy_raw, factor=16):
    """training.validate's lines for one noisy H x W x C float image: the padded model input (on the host) and
    the uint8 result."""
    from irdu_amd.training import _img_as_ubyte
    noisy = torch.from_numpy(noisy_raw).permute(2, 0, 1).unsqueeze(0)
    h, w = noisy.shape[2], noisy.shape[3]
    H, W = ((h + factor) // factor) * factor, ((w + factor) // factor) * factor
    padh = H - h if h % factor != 0 else 0
    padw = W - w if w % factor != 0 else 0
    noisy = nn.functional.pad(noisy, (0, padw, 0, padh), "reflect")
    with torch.no_grad():
        restored = model(noisy.to(DEV).contiguous())[:, :, :h, :w]
    restored = torch.clamp(restored, 0, 1).cpu().permute(0, 2, 3, 1).squeeze(0).numpy()
    return noisy, _img_as_ubyte(restored)


def noisy_images(images, sigma=25.0, seed=2204):
    rs = np.random.RandomState(seed=seed)
    out = []
    for i in range(len(images)):
        img = np.asarray(images[i], dtype=np.float32)
        noisy = img.copy()
        noisy += rs.normal(0, sigma / 255.0, img.shape)
        out.append(noisy)
    return out


def test_model_input_is_validates_padded_tensor(irdu):
    from irdu_amd import training as T
    torch.manual_seed(11)
    m = irdu.AbtractMultiScaleGraphFilter(
        3, 3, dims=[8, 16, 16, 32], hidden_dims=[16, 32, 32, 64], nsubnets=[1, 1, 1, 1], ngraphs=[2, 4, 4, 8],
        num_blocks=[1, 1, 1, 1], num_blocks_out=1, n_cgd_iters=1).to(DEV).eval()
    seen = []

    def recording(x):
        seen.append(x.clone())
        return m(x)

    noisy = noisy_images(T.SyntheticTestImages(n_images=1))[0]
    assert noisy.shape == (100, 140, 3)
    out = irdu.restore_image(recording, noisy, factor=16)
    want_in, want_out = validate_lines(m, noisy)
    assert len(seen) == 1 and tuple(seen[0].shape) == (1, 3, 112, 144)
    assert np.array_equal(bits(seen[0].cpu().numpy()), bits(want_in.numpy()))
    assert np.array_equal(out, want_out)


def test_end_to_end_equals_validate(irdu):
    from irdu_amd import training as T
    torch.manual_seed(12)
    m = irdu.MultiScaleGraphFilter(3, 3, ngraphs=4, n_cgd_iters=3)
    perturb_mixture(m.localfilter, 66)
    m = m.to(DEV)
    images = T.SyntheticTestImages(n_images=2)
    modes = []
    hook = m.register_forward_pre_hook(lambda mod, args: modes.append(mod.training))
    m.train()
    for noisy in noisy_images(images):
        out = irdu.restore_image(m, noisy)
        assert m.training, "the model's mode was not restored"
        m.eval()
        _, want = validate_lines(m, noisy)
        m.train()
        assert out.dtype == np.uint8 and np.array_equal(out, want)
    hook.remove()
    assert modes and not any(modes[::2]), "the model did not run in eval mode"
    m.eval()
    mean, per_image = irdu.evaluate(m, images, sigma=25.0, factor=16, seed=2204)
    ref = T.validate(m, images, sigma=25.0, factor=16, seed=2204)
    print(f"evaluate {mean:.6f} dB, validate {ref:.6f} dB, per image {per_image}")
    assert len(per_image) == 2 and mean == pytest.approx(float(np.mean(per_image)))
    assert abs(mean - ref) <= 1e-4


# ---- 7. tiled against whole
def test_tiled_equals_whole(irdu):
    """S = 1 image filter: by DESIGN.md §5's count its receptive field is 20 px (b_A 13, x_1 20), under the
    32-pixel halo, so windows of 128 reproduce the one-window result to the project's 1e-5 (the kernels differ
    between the window width and the image width, hence not bit for bit)."""
    torch.manual_seed(13)
    m = irdu.MultiScaleGraphFilter(3, 3, ngraphs=4, n_cgd_iters=1)
    perturb_mixture(m.localfilter, 77)
    m = m.to(DEV).eval()
    img = np.random.RandomState(5).rand(150, 203, 3).astype(np.float32)
    assert len(irdu.plan(150, 203, 16, 128, 32).windows) > 1 and len(irdu.plan(150, 203, 16, 256, 32).windows) == 1
    whole = irdu.restore_image(m, img, tile=256, halo=32, quantise=False)
    tiled = irdu.restore_image(m, img, tile=128, halo=32, micro_batch=4, quantise=False)
    err = rel_err(torch.from_numpy(tiled), whole)
    print("tiled vs whole rel err:", err)
    assert err <= 1e-5
    whole8 = irdu.restore_image(m, img, tile=256, halo=32)
    tiled8 = irdu.restore_image(m, img, tile=128, halo=32, micro_batch=4)
    diff = np.abs(whole8.astype(np.int16) - tiled8.astype(np.int16))
    print("uint8 levels that differ:", int((diff > 0).sum()), "of", diff.size)
    assert diff.max() <= 1


# ---- 8. errors
def test_bad_images_raise_before_any_launch(irdu, monkeypatch):
    def no_launch(*a, **k):
        raise AssertionError("a kernel was launched")
    monkeypatch.setattr(irdu.kernels, "_launch", no_launch)
    ident = lambda x: x  # noqa: E731
    for bad in (np.zeros((32, 32, 5), np.uint8), np.zeros((32, 32, 3), np.int16), torch.zeros(8, 32, 32, device=DEV),
                np.zeros((5, 32, 3), np.uint8), torch.zeros(32, 32, 3, dtype=torch.float64, device=DEV)):
        with pytest.raises(ValueError):
            irdu.restore_image(ident, bad)
    with pytest.raises(ValueError):
        irdu.kernels.tile_gather(torch.zeros(16, 16, 5, dtype=torch.uint8, device=DEV),
                                 torch.zeros(1, 6, dtype=torch.int32, device=DEV), 16, 16)
    with pytest.raises(ValueError):
        irdu.kernels.u8_sse(torch.zeros(4, device=DEV), torch.zeros(4, device=DEV))


# ---- the command line
def test_cli_restores_files_and_reports_psnr(irdu, tmp_path, capsys):
    import os
    from PIL import Image
    from irdu_amd import training as T
    from tests.test_restore_ref import _cli
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    yaml_path = os.path.join(root, "experiment_conf", "example_v1x0_small.yaml")
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    images = {"a": make_image(37, 53, 3, "uint8", 1), "b": make_image(100, 140, 3, "uint8", 2)}
    for name, img in images.items():
        Image.fromarray(img).save(src / f"{name}.png")
    torch.manual_seed(21)
    model = T.build_model(T.parse_options(yaml_path)["model"])
    torch.save({"i": 0, "model": model.state_dict()}, tmp_path / "ckpt.pt")
    model = model.to(DEV).eval()
    cli = _cli()

    cli.main(["-yaml_path", yaml_path, "--ckpt", str(tmp_path / "ckpt.pt"), "--input", str(src), "--output", str(dst)])
    assert "weights: " + str(tmp_path / "ckpt.pt") in capsys.readouterr().out
    for name, img in images.items():
        assert np.array_equal(np.array(Image.open(dst / f"{name}.png")), irdu.restore_image(model, img))

    cli.main(["-yaml_path", yaml_path, "--ckpt", str(tmp_path / "ckpt.pt"), "--input", str(src), "--output", str(dst),
              "--sigma", "25", "--seed", "7"])
    out = capsys.readouterr().out
    rs = np.random.RandomState(7)
    psnrs = []
    for name in ("a", "b"):                                   # file order, one noise stream
        noisy = images[name].astype(np.float32) / 255.0
        noisy += rs.normal(0, 25.0 / 255.0, noisy.shape)
        want = irdu.restore_image(model, noisy)
        assert np.array_equal(np.array(Image.open(dst / f"{name}.png")), want)
        psnrs.append(irdu.psnr_u8(want, images[name]))
        assert f"PSNR {psnrs[-1]:.4f} dB" in out
    assert f"mean PSNR over 2 image(s): {np.mean(psnrs):.4f} dB" in out

    cli.main(["-yaml_path", yaml_path, "--input", str(src / "a.png"), "--output", str(dst)])
    assert "initial weights" in capsys.readouterr().out
