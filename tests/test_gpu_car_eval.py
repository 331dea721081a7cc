"""restore.evaluate_car, the "psnrb" metric of evaluate_pairs / evaluate_metrics, training.validate_car and
restore.py --jpeg-quality / --psnrb on the GPU, with cheap callable models (the identity and a fixed 3 x 3 blur, as the
restoration tests use) and the oracle tests/jpeg_ref.py for the degradation and the metric."""
import os
import re

import numpy as np
import pytest
import torch

from tests import jpeg_ref, patch_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TILING = dict(factor=16, tile=64, halo=16, device=DEV)
ALL = ("psnr", "ssim", "psnr_y", "ssim_y", "psnrb")


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


def cleans():
    """Three pictures; the second exceeds the 64-pixel tile, the third has odd sides."""
    return [patch_ref.picture(k, h, w) for k, (h, w) in enumerate(((40, 56), (72, 44), (33, 47)))]


_DEGRADED = {}


def degraded(q, sub):
    if (q, sub) not in _DEGRADED:
        _DEGRADED[q, sub] = [jpeg_ref.degrade(a, q, sub) for a in cleans()]
    return _DEGRADED[q, sub]


@pytest.mark.parametrize("model", [identity, blur])
@pytest.mark.parametrize("q,sub", [(10, 0), (40, 2)])
def test_it_is_evaluate_pairs_on_the_oracle_degraded_inputs(G, model, q, sub):
    got = G.R.evaluate_car(model, cleans(), q, sub, metrics=ALL, **TILING)
    want = G.R.evaluate_pairs(model, degraded(q, sub), cleans(), metrics=ALL, **TILING)
    assert got == want and all(np.isfinite(v) for m in ALL for v in got[m][1])
    for name in ALL:
        assert got[name][0] == float(np.mean(got[name][1]))
    # the defaults: PSNR, SSIM and PSNR-B at 4:4:4
    short = G.I.evaluate_car(model, cleans(), q, **TILING)
    assert set(short) == {"psnr", "ssim", "psnrb"}
    assert short == G.R.evaluate_car(model, cleans(), q, 0, metrics=("psnr", "ssim", "psnrb"), **TILING)
    if model is identity:       # the restored picture is the degraded one: PSNR-B is the restatement's
        for k, (a, b) in enumerate(zip(degraded(q, sub), cleans())):
            assert abs(got["psnrb"][1][k] - jpeg_ref.psnrb(a, b)) <= 1e-12 * jpeg_ref.psnrb(a, b)
        # BEF >= 0; where it is 0 the two logarithms are of quotients formed in another order: equal to rounding
        assert all(pb <= p + 1e-12 for pb, p in zip(got["psnrb"][1], got["psnr"][1]))


def test_psnrb_per_image_and_across_images_agree_and_tensors_are_taken_as_they_are(G):
    q, sub = 10, 2
    per_image = G.R.evaluate_pairs(blur, degraded(q, sub), cleans(), metrics=ALL, **TILING)
    across = G.R.evaluate_pairs(blur, degraded(q, sub), cleans(), metrics=ALL, across_images=True, **TILING)
    assert per_image == across
    mixed = [torch.from_numpy(cleans()[0]), torch.from_numpy(cleans()[1]).to(DEV), cleans()[2]]
    assert G.R.evaluate_car(blur, mixed, q, sub, metrics=ALL, **TILING) == per_image
    # evaluate_metrics scores the same name on its noisy restorations
    floats = [c.astype(np.float32) / 255.0 for c in cleans()]
    noisy = G.R.evaluate_metrics(blur, floats, sigma=15.0, metrics=("psnr", "psnrb"), **TILING)
    both = G.R.evaluate_metrics(blur, floats, sigma=15.0, metrics=("psnr", "psnrb"), across_images=True, **TILING)
    assert noisy == both and noisy["psnr"] == G.R.evaluate_metrics(blur, floats, sigma=15.0, metrics=("psnr",), **TILING)["psnr"]
    assert all(pb <= p + 1e-12 for pb, p in zip(noisy["psnrb"][1], noisy["psnr"][1]))


class Blur(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.bias = torch.nn.Parameter(torch.zeros(1))

    def forward(self, x):
        return blur(x) + self.bias


def test_validate_car_is_the_mean_of_evaluate_car_on_what_the_csv_dataset_yields(G, tmp_path):
    from PIL import Image
    pics = cleans()[:2]
    lines = ["index,path"]
    for k, a in enumerate(pics):
        Image.fromarray(a).save(tmp_path / f"hq{k}.png")
        lines.append(f"{k},hq{k}.png")
    (tmp_path / "val.csv").write_text("\n".join(lines) + "\n")
    conf = dict(datasets=dict(val=dict(type="TestImagesCSV", jpeg_quality=10, subsampling=2, tile=64, halo=16,
                                       dataset_args=dict(csv_path=str(tmp_path / "val.csv"), root_folder=str(tmp_path)))))
    val_set, val_args = G.T.create_val_dataset(conf)
    model = Blur().to(DEV)
    got = G.T.validate_car(model, val_set, device=torch.device(DEV), **val_args)
    want = G.R.evaluate_car(model, pics, 10, 2, metrics=("psnr", "psnr_y", "psnrb"), **TILING)
    assert got == want["psnr"][0] and np.isfinite(got)
    for metric in ("psnrb", "psnr_y"):
        assert G.T.validate_car(model, val_set, device=torch.device(DEV), metric=metric, **val_args) == want[metric][0]
    assert want["psnr_y"][0] != got and want["psnrb"][0] <= got + 1e-12


def test_restore_command_jpeg_quality_and_psnrb(G, tmp_path, capsys):
    """restore.py --jpeg-quality prints the scores of the files it writes; --psnrb also works with --reference."""
    from PIL import Image
    from tests.test_restore_ref import _cli
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    yaml_path = os.path.join(root, "experiment_conf", "example.yaml")       # a one-channel model, no checkpoint
    src, dst, ref = tmp_path / "in", tmp_path / "out", tmp_path / "ref"
    src.mkdir()
    ref.mkdir()
    pics = {"a": patch_ref.picture(3, 40, 50, 1), "b": patch_ref.picture(4, 33, 47, 1)}
    for name, a in pics.items():
        Image.fromarray(a[:, :, 0]).save(src / f"{name}.png")
    cli = _cli()
    q = 20
    base = ["-yaml_path", yaml_path, "--input", str(src), "--output", str(dst), "--tile", "64", "--halo", "16"]
    torch.manual_seed(3)
    cli.main(base + ["--jpeg-quality", str(q), "--psnrb", "--ssim"])
    out = capsys.readouterr().out.splitlines()
    torch.manual_seed(3)
    model = G.T.build_model(G.T.parse_options(yaml_path)["model"]).to(DEV).eval()
    scores = []
    for line, (name, clean) in zip(out[1:], sorted(pics.items())):
        written = np.array(Image.open(dst / f"{name}.png"))[:, :, None]
        want = G.R.restore_image(model, jpeg_ref.degrade(clean, q, 0), factor=16, tile=64, halo=16)
        assert np.array_equal(written, want)
        m = re.search(r"jpeg q20 4:4:4  PSNR (\d+\.\d{4}) dB  SSIM (-?\d\.\d{4})  PSNR-B (\d+\.\d{4}) dB$", line)
        assert m, line
        assert m.group(1) == f"{G.R.psnr_u8(written, clean):.4f}" and m.group(2) == f"{G.R.ssim_u8(written, clean):.4f}"
        assert m.group(3) == f"{jpeg_ref.psnrb(written, clean):.4f}"
        scores.append(jpeg_ref.psnrb(written, clean))
    assert out[-1] == f"mean PSNR-B over 2 image(s): {float(np.mean(scores)):.4f} dB"
    car = G.R.evaluate_car(model, [pics["a"], pics["b"]], q, metrics=("psnrb",), **TILING)["psnrb"]
    assert out[-1].endswith(f"{car[0]:.4f} dB")
    # --psnrb with --reference: the inputs are degraded files, scored against the clean ones
    for name, a in pics.items():
        Image.fromarray(jpeg_ref.degrade(a, q, 0)[:, :, 0]).save(ref / f"{name}.png")
    torch.manual_seed(3)
    cli.main(["-yaml_path", yaml_path, "--input", str(ref), "--output", str(dst), "--tile", "64", "--halo", "16",
              "--reference", str(src), "--psnrb"])
    again = capsys.readouterr().out.splitlines()
    assert again[-1] == out[-1] and all("PSNR-B" in line for line in again[1:3])
    for bad in (["--jpeg-quality", "0"], ["--jpeg-quality", "101"], ["--psnrb"], ["--jpeg-subsampling", "420"],
                ["--jpeg-quality", "10", "--sigma", "5"], ["--jpeg-quality", "10", "--jpeg-subsampling", "422"]):
        with pytest.raises(SystemExit):
            cli.main(base + bad)
    capsys.readouterr()
