"""restore.evaluate_demosaic, training.validate_demosaic and restore.py --bayer / --raw on the GPU, with cheap callable
models (the identity and a fixed 3 x 3 blur, as the restoration tests use) and the oracle tests/demosaic_ref.py for the
mosaic and its fill."""
import os
import re

import numpy as np
import pytest
import torch

from tests import demosaic_ref as ref, patch_ref

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


_CLEANS = [patch_ref.picture(k, h, w) for k, (h, w) in enumerate(((40, 56), (72, 44), (33, 47)))]
_FILLED = {}


def cleans():
    """Three pictures; the second exceeds the 64-pixel tile, the third has odd sides."""
    return _CLEANS


def filled(pattern, fill):
    if (pattern, fill) not in _FILLED:
        _FILLED[pattern, fill] = [ref.degrade(a, pattern, fill) for a in cleans()]
    return _FILLED[pattern, fill]


@pytest.mark.parametrize("model", [identity, blur])
@pytest.mark.parametrize("pattern,fill", [("rggb", "malvar"), ("gbrg", "bilinear"), ("bggr", "zero")])
def test_without_a_shave_it_is_evaluate_pairs_on_the_oracle_filled_inputs(G, model, pattern, fill):
    got = G.R.evaluate_demosaic(model, cleans(), pattern, fill, metrics=ALL, **TILING)
    want = G.R.evaluate_pairs(model, filled(pattern, fill), cleans(), metrics=ALL, **TILING)
    assert got == want and all(np.isfinite(v) for m in ALL for v in got[m][1])
    for name in ALL:
        assert got[name][0] == float(np.mean(got[name][1]))
    if model is identity:       # the restored picture is the filled one: the CPSNR is the plain PSNR of the oracle's
        for k, (a, b) in enumerate(zip(filled(pattern, fill), cleans())):
            assert got["psnr"][1][k] == G.R.psnr_u8(a, b)
    if pattern == "rggb":       # the defaults: rggb, malvar, no shave, PSNR and SSIM
        short = G.I.evaluate_demosaic(model, cleans(), **TILING)
        assert set(short) == {"psnr", "ssim"} and short == {m: got[m] for m in ("psnr", "ssim")}
        codes = G.R.evaluate_demosaic(model, cleans(), 0, 2, shave=0, metrics=("psnr", "ssim"), **TILING)
        assert codes == short


@pytest.mark.parametrize("shave", [2, 5])
def test_with_a_shave_it_is_the_metric_functions_on_numpy_cropped_pictures(G, shave):
    got = G.R.evaluate_demosaic(blur, cleans(), "grbg", "malvar", shave=shave, metrics=ALL, ensemble=(0, 1), **TILING)
    for k, (clean, low) in enumerate(zip(cleans(), filled("grbg", "malvar"))):
        restored = G.R.restore_image(blur, low, ensemble=(0, 1), **TILING)
        a = np.ascontiguousarray(restored[shave:-shave, shave:-shave])
        b = np.ascontiguousarray(clean[shave:-shave, shave:-shave])
        assert a.shape == (clean.shape[0] - 2 * shave, clean.shape[1] - 2 * shave, 3)
        for name, fn in (("psnr", G.R.psnr_u8), ("ssim", G.R.ssim_u8), ("psnr_y", G.R.psnr_y_u8), ("ssim_y", G.R.ssim_y_u8)):
            assert got[name][1][k] == fn(a, b), (name, k)
    for name in ALL:
        assert got[name][0] == float(np.mean(got[name][1]))
    assert got != G.R.evaluate_demosaic(blur, cleans(), "grbg", "malvar", metrics=ALL, ensemble=(0, 1), **TILING)
    # tensors, on the host and on the device, are taken as they are
    mixed = [torch.from_numpy(cleans()[0].copy()), torch.from_numpy(cleans()[1].copy()).to(DEV), cleans()[2]]
    assert G.R.evaluate_demosaic(blur, mixed, "grbg", "malvar", shave=shave, metrics=ALL, ensemble=(0, 1), **TILING) == got


def test_it_refuses_before_any_launch(G, monkeypatch):
    def no_launch(*a, **k):
        raise AssertionError("a kernel was launched")
    monkeypatch.setattr(G.K, "_launch", no_launch)
    pics = cleans()
    for bad in ("rgbg", 4, None):
        with pytest.raises(ValueError, match="pattern"):
            G.R.evaluate_demosaic(identity, pics, bad, **TILING)
    with pytest.raises(ValueError, match="fill"):
        G.R.evaluate_demosaic(identity, pics, "rggb", "linear", **TILING)
    with pytest.raises(ValueError, match="shave"):
        G.R.evaluate_demosaic(identity, pics, shave=-1, **TILING)
    with pytest.raises(ValueError, match="image 1 .*uint8"):
        G.R.evaluate_demosaic(identity, [pics[0], pics[1].astype(np.float32)], **TILING)
    with pytest.raises(ValueError, match="image 1 .*clean R, G, B"):
        G.R.evaluate_demosaic(identity, [pics[0], pics[1][:, :, :1]], **TILING)
    with pytest.raises(ValueError, match="image 2 .*nothing is left"):
        G.R.evaluate_demosaic(identity, pics, shave=17, metrics=("psnr",), **TILING)
    with pytest.raises(ValueError, match="image 2 after the shave .*SSIM"):
        G.R.evaluate_demosaic(identity, pics, shave=12, **TILING)
    with pytest.raises(ValueError, match="metrics"):
        G.R.evaluate_demosaic(identity, pics, metrics=("cpsnr",), **TILING)
    with pytest.raises(ValueError, match="no images"):
        G.R.evaluate_demosaic(identity, [], **TILING)
    with pytest.raises(ValueError, match="demosaic_u8: the pattern"):
        G.I.demosaic_u8(torch.zeros((8, 8, 3), dtype=torch.uint8, device=DEV), "rgbg")


class Blur(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.bias = torch.nn.Parameter(torch.zeros(1))

    def forward(self, x):
        return blur(x) + self.bias


def test_validate_demosaic_is_the_mean_of_evaluate_demosaic_on_what_the_csv_dataset_yields(G, tmp_path):
    from PIL import Image
    pics = cleans()[:2]
    lines = ["index,path"]
    for k, a in enumerate(pics):
        Image.fromarray(a).save(tmp_path / f"hq{k}.png")
        lines.append(f"{k},hq{k}.png")
    (tmp_path / "val.csv").write_text("\n".join(lines) + "\n")
    conf = dict(datasets=dict(val=dict(type="TestImagesCSV", bayer="gbrg", fill="bilinear", shave=3, tile=64, halo=16,
                                       dataset_args=dict(csv_path=str(tmp_path / "val.csv"), root_folder=str(tmp_path)))))
    val_set, val_args = G.T.create_val_dataset(conf)
    assert val_args == dict(bayer="gbrg", fill="bilinear", shave=3, tile=64, halo=16, factor=16)
    model = Blur().to(DEV)
    got = G.T.validate_demosaic(model, val_set, device=torch.device(DEV), **val_args)
    want = G.R.evaluate_demosaic(model, pics, "gbrg", "bilinear", shave=3, metrics=G.T.VAL_DEMOSAIC_METRICS, **TILING)
    assert got == want["psnr"][0] and np.isfinite(got)
    for metric in ("psnr_y", "ssim"):
        assert G.T.validate_demosaic(model, val_set, device=torch.device(DEV), metric=metric, **val_args) == want[metric][0]
    assert want["psnr_y"][0] != got
    plain = G.T.validate_demosaic(model, val_set, "rggb", device=torch.device(DEV), tile=64, halo=16)
    assert plain == G.R.evaluate_demosaic(model, pics, metrics=("psnr",), **TILING)["psnr"][0] and plain != got


MODEL_YAML = """name: demosaic_tool
manual_seed: 2204
model:
  type: GLRImageFilter
  args: {n_channels_in: 3, n_channels_out: 3, ngraphs: 4, n_cgd_iters: 1}
"""


def test_restore_command_bayer_and_raw(G, tmp_path, capsys):
    """restore.py --bayer prints the protocol's scores of the files it writes; --raw writes model(fill(mosaic file))
    as RGB."""
    from PIL import Image
    from tests.test_restore_ref import _cli
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    yaml_path = tmp_path / "rgb.yaml"
    yaml_path.write_text(MODEL_YAML)
    src, raw, dst = tmp_path / "in", tmp_path / "raw", tmp_path / "out"
    src.mkdir()
    raw.mkdir()
    pics = {"a": patch_ref.picture(3, 40, 50), "b": patch_ref.picture(4, 33, 47)}
    for name, a in pics.items():
        Image.fromarray(a).save(src / f"{name}.png")
        Image.fromarray(ref.mosaic(a, "grbg").astype(np.uint8)).save(raw / f"{name}.png")
    cli = _cli()
    base = ["-yaml_path", str(yaml_path), "--input", str(src), "--output", str(dst), "--tile", "64", "--halo", "16"]
    torch.manual_seed(3)
    cli.main(base + ["--bayer", "grbg", "--ssim", "--shave", "4"])
    out = capsys.readouterr().out.splitlines()
    torch.manual_seed(3)
    model = G.T.build_model(G.T.parse_options(str(yaml_path))["model"]).to(DEV).eval()
    scores, restored = [], {}
    for line, (name, clean) in zip(out[1:], sorted(pics.items())):
        written = np.array(Image.open(dst / f"{name}.png"))
        want = G.R.restore_image(model, ref.degrade(clean, "grbg", "malvar"), factor=16, tile=64, halo=16)
        assert np.array_equal(written, want)
        restored[name] = written
        m = re.search(r"bayer grbg malvar shave 4  PSNR (\d+\.\d{4}) dB  SSIM (-?\d\.\d{4})$", line)
        assert m, line
        a, b = np.ascontiguousarray(written[4:-4, 4:-4]), np.ascontiguousarray(clean[4:-4, 4:-4])
        assert m.group(1) == f"{G.R.psnr_u8(a, b):.4f}" and m.group(2) == f"{G.R.ssim_u8(a, b):.4f}"
        scores.append(G.R.psnr_u8(a, b))
    assert out[-2] == f"mean PSNR over 2 image(s): {float(np.mean(scores)):.4f} dB"
    ev = G.R.evaluate_demosaic(model, [pics["a"], pics["b"]], "grbg", shave=4, metrics=("psnr",), **TILING)["psnr"]
    assert out[-2].endswith(f"{ev[0]:.4f} dB")
    # other flags: the Y channel, the batch of images, the ensemble, another fill
    torch.manual_seed(3)
    cli.main(base + ["--bayer", "grbg", "--y-channel", "--batch-images", "--ensemble-modes", "0,1",
                     "--demosaic-fill", "bilinear"])
    other = capsys.readouterr().out
    assert other.count("bayer grbg bilinear shave 0  PSNR-Y") == 2 and "mean PSNR-Y over 2 image(s)" in other
    # --raw: the mosaic files give the pictures --bayer wrote from the clean ones
    torch.manual_seed(3)
    cli.main(["-yaml_path", str(yaml_path), "--input", str(raw), "--output", str(dst), "--tile", "64", "--halo", "16",
              "--raw", "grbg"])
    said = capsys.readouterr().out
    assert "40x50x3" in said and "PSNR" not in said
    for name in pics:
        written = np.array(Image.open(dst / f"{name}.png"))
        assert written.shape == pics[name].shape and np.array_equal(written, restored[name])
    # refusals: parsing, a 1-channel model, files of the wrong kind
    for bad in (["--bayer", "rgbg"], ["--bayer", "rggb", "--raw", "rggb"], ["--bayer", "rggb", "--sigma", "5"],
                ["--demosaic-fill", "zero"], ["--raw", "rggb", "--ssim"], ["--bayer", "rggb", "--psnrb"]):
        with pytest.raises(SystemExit):
            cli.main(base + bad)
    capsys.readouterr()
    with pytest.raises(SystemExit, match="--bayer: the model"):
        cli.main(["-yaml_path", os.path.join(root, "experiment_conf", "example.yaml")] + base[2:] + ["--bayer", "rggb"])
    with pytest.raises(SystemExit, match=r"--raw: .*a\.png has 3 channel"):
        cli.main(base + ["--raw", "rggb"])
    with pytest.raises(SystemExit, match=r"--bayer: .*a\.png has 1 channel"):
        cli.main(["-yaml_path", str(yaml_path), "--input", str(raw), "--output", str(dst), "--bayer", "rggb"])
    with pytest.raises(SystemExit, match="nothing is left"):
        cli.main(base + ["--bayer", "rggb", "--shave", "17"])
    capsys.readouterr()
