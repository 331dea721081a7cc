"""restore.evaluate_sr, training.validate_sr and restore.py --scale / --upscale on the GPU, with cheap callable models
(the identity and a fixed 3 x 3 blur, as the restoration tests use) and the oracle tests/resize_ref.py for the
degradation."""
import os
import re

import numpy as np
import pytest
import torch

from tests import patch_ref, resize_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TILING = dict(factor=16, tile=64, halo=16, device=DEV)
ALL = ("psnr", "ssim", "psnr_y", "ssim_y")


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import irdu_amd
    irdu_amd.load_native()
    from irdu_amd import kernels, restore, training
    return type("G", (), dict(K=kernels, R=restore, T=training, I=irdu_amd))


def identity(x):
    return x


def blur(x):
    """A fixed 3 x 3 box blur: batch-independent, any window size."""
    return torch.nn.functional.avg_pool2d(torch.nn.functional.pad(x, (1, 1, 1, 1), mode="replicate"), 3, 1)


def cleans(s):
    """Pictures whose sides are multiples of s; the second exceeds the 64-pixel tile."""
    return [patch_ref.picture(k, h * s, w * s) for k, (h, w) in enumerate(((20, 28), (36, 22), (16, 16)))]


_DEGRADED = {}


def degraded(s):
    if s not in _DEGRADED:
        _DEGRADED[s] = [resize_ref.degrade(a, s) for a in cleans(s)]
    return _DEGRADED[s]


@pytest.mark.parametrize("model", [identity, blur])
@pytest.mark.parametrize("s", (2, 3))
def test_without_shave_it_is_evaluate_pairs_on_the_oracle_degraded_inputs(G, model, s):
    got = G.R.evaluate_sr(model, cleans(s), s, shave=0, metrics=ALL, **TILING)
    want = G.R.evaluate_pairs(model, degraded(s), cleans(s), metrics=ALL, **TILING)
    assert got == want and all(np.isfinite(v) for m in ALL for v in got[m][1])
    # the defaults: the two Y-channel metrics, a shave of s
    short = G.I.evaluate_sr(model, cleans(s), s, **TILING)
    assert set(short) == {"psnr_y", "ssim_y"} and short == G.R.evaluate_sr(model, cleans(s), s, shave=s, **TILING)
    assert short["psnr_y"][1] != got["psnr_y"][1]


@pytest.mark.parametrize("s,shave", [(2, 2), (4, 4), (3, 5)])
def test_with_a_shave_it_is_the_metric_functions_on_numpy_cropped_pictures(G, s, shave):
    got = G.R.evaluate_sr(blur, cleans(s), s, shave=shave, metrics=ALL, ensemble=(0, 1), **TILING)
    for k, (clean, low) in enumerate(zip(cleans(s), degraded(s))):
        restored = G.R.restore_image(blur, low, ensemble=(0, 1), **TILING)
        a = np.ascontiguousarray(restored[shave:-shave, shave:-shave])
        b = np.ascontiguousarray(clean[shave:-shave, shave:-shave])
        assert a.shape == (clean.shape[0] - 2 * shave, clean.shape[1] - 2 * shave, 3)
        for name, fn in (("psnr", G.R.psnr_u8), ("ssim", G.R.ssim_u8), ("psnr_y", G.R.psnr_y_u8), ("ssim_y", G.R.ssim_y_u8)):
            assert got[name][1][k] == fn(a, b), (name, k)
    for name in ALL:
        assert got[name][0] == float(np.mean(got[name][1]))


def test_sides_that_are_no_multiple_of_the_scale_are_cropped_at_the_top_left(G):
    s = 4
    whole = [patch_ref.picture(5, 83, 66), patch_ref.picture(6, 80, 67)]
    cropped = [np.ascontiguousarray(whole[0][:80, :64]), np.ascontiguousarray(whole[1][:80, :64])]
    got = G.R.evaluate_sr(blur, whole, s, metrics=ALL, **TILING)
    assert got == G.R.evaluate_sr(blur, cropped, s, metrics=ALL, **TILING)
    assert got != G.R.evaluate_sr(blur, [w[3:, 2:] for w in whole], s, metrics=ALL, **TILING)
    # tensors, on the host and on the device, are taken as they are
    mixed = [torch.from_numpy(whole[0]), torch.from_numpy(whole[1]).to(DEV)]
    assert G.R.evaluate_sr(blur, mixed, s, metrics=ALL, **TILING) == got


def test_it_refuses_before_any_launch(G, monkeypatch):
    def no_launch(*a, **k):
        raise AssertionError("a kernel was launched")
    monkeypatch.setattr(G.K, "_launch", no_launch)
    pics = cleans(2)
    for bad in (1, 9, 2.0):
        with pytest.raises(ValueError, match="scale"):
            G.R.evaluate_sr(identity, pics, bad, **TILING)
    with pytest.raises(ValueError, match="shave"):
        G.R.evaluate_sr(identity, pics, 2, shave=-1, **TILING)
    with pytest.raises(ValueError, match="image 1 .*uint8"):
        G.R.evaluate_sr(identity, [pics[0], pics[1].astype(np.float32)], 2, **TILING)
    with pytest.raises(ValueError, match="image 2 .*nothing is left"):
        G.R.evaluate_sr(identity, pics, 2, shave=16, metrics=("psnr",), **TILING)
    with pytest.raises(ValueError, match="image 2 after the shave .*SSIM"):
        G.R.evaluate_sr(identity, pics, 2, shave=11, **TILING)
    with pytest.raises(ValueError, match="Y-channel"):
        G.R.evaluate_sr(identity, [p[:, :, :1] for p in pics], 2, **TILING)
    with pytest.raises(ValueError, match="metrics"):
        G.R.evaluate_sr(identity, pics, 2, metrics=("mse",), **TILING)
    with pytest.raises(ValueError, match="no images"):
        G.R.evaluate_sr(identity, [], 2, **TILING)


class Blur(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.bias = torch.nn.Parameter(torch.zeros(1))

    def forward(self, x):
        return blur(x) + self.bias


def test_validate_sr_is_the_mean_of_evaluate_sr_on_what_the_csv_dataset_yields(G, tmp_path):
    from PIL import Image
    pics = cleans(2)[:2]
    lines = ["index,path"]
    for k, a in enumerate(pics):
        Image.fromarray(a).save(tmp_path / f"hr{k}.png")
        lines.append(f"{k},hr{k}.png")
    (tmp_path / "val.csv").write_text("\n".join(lines) + "\n")
    conf = dict(datasets=dict(val=dict(type="TestImagesCSV", scale=2, tile=64, halo=16,
                                       dataset_args=dict(csv_path=str(tmp_path / "val.csv"), root_folder=str(tmp_path)))))
    val_set, val_args = G.T.create_val_dataset(conf)
    model = Blur().to(DEV)
    got = G.T.validate_sr(model, val_set, device=torch.device(DEV), **val_args)
    want = G.R.evaluate_sr(model, pics, 2, metrics=("psnr_y",), **TILING)["psnr_y"]
    assert got == want[0] and np.isfinite(got)
    rgb = G.T.validate_sr(model, val_set, device=torch.device(DEV), metric="psnr", shave=0, **val_args)
    assert rgb == G.R.evaluate_sr(model, pics, 2, shave=0, metrics=("psnr",), **TILING)["psnr"][0] and rgb != got


def test_restore_command_scale_and_upscale(G, tmp_path, capsys):
    """restore.py --upscale writes model(up(file)) at S times the size; --scale prints the protocol's scores of the
    files it writes."""
    from PIL import Image
    from tests.test_restore_ref import _cli
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    yaml_path = os.path.join(root, "experiment_conf", "example.yaml")       # a one-channel model, no checkpoint
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    low = patch_ref.picture(3, 20, 30, 1)
    Image.fromarray(low[:, :, 0]).save(src / "low.png")
    cli = _cli()
    s = 3
    base = ["-yaml_path", yaml_path, "--input", str(src), "--output", str(dst), "--tile", "64", "--halo", "16"]
    torch.manual_seed(3)
    cli.main(base + ["--upscale", str(s)])
    assert f"{20 * s}x{30 * s}x1" in capsys.readouterr().out
    written = np.array(Image.open(dst / "low.png"))
    assert written.shape == (20 * s, 30 * s)
    torch.manual_seed(3)
    model = G.T.build_model(G.T.parse_options(yaml_path)["model"]).to(DEV).eval()
    want = G.R.restore_image(model, resize_ref.up(low, s), factor=16, tile=64, halo=16)
    assert np.array_equal(written[:, :, None], want)
    # --scale on a clean file whose sides are no multiples of S
    os.remove(src / "low.png")
    clean = patch_ref.picture(4, 50, 67, 1)
    Image.fromarray(clean[:, :, 0]).save(src / "hr.png")
    torch.manual_seed(3)
    cli.main(base + ["--scale", str(s), "--ssim"])
    out = capsys.readouterr().out
    written = np.array(Image.open(dst / "hr.png"))[:, :, None]
    crop = np.ascontiguousarray(clean[:48, :66])
    assert np.array_equal(written, G.R.restore_image(model, resize_ref.degrade(crop, s), factor=16, tile=64, halo=16))
    m = re.search(r"bicubic x3 shave 3  PSNR (\d+\.\d{4}) dB  SSIM (-?\d\.\d{4})$", out.splitlines()[1])
    assert m, out
    a, b = np.ascontiguousarray(written[s:-s, s:-s]), np.ascontiguousarray(crop[s:-s, s:-s])
    assert m.group(1) == f"{G.R.psnr_u8(a, b):.4f}" and m.group(2) == f"{G.R.ssim_u8(a, b):.4f}"
    assert m.group(1) == f"{G.R.evaluate_sr(model, [clean], s, metrics=('psnr',), **TILING)['psnr'][0]:.4f}"
    for bad in (["--scale", "9"], ["--upscale", "1"], ["--shave", "2"], ["--scale", "2", "--upscale", "2"],
                ["--scale", "2", "--sigma", "5"]):
        with pytest.raises(SystemExit):
            cli.main(base + bad)
    capsys.readouterr()
