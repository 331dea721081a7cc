"""restore.evaluate_deblur, training.validate_deblur and restore.py --blur on the GPU, with cheap callable models (the
identity and a fixed 3 x 3 blur, as the restoration tests use) and the oracle tests/blur_ref.py for the degradation.
The noisy input of the blur-plus-noise protocol is made again here, from the oracle's blurred picture and numpy's
RandomState."""
import re

import numpy as np
import pytest
import torch

from tests import blur_ref as ref, patch_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TILING = dict(factor=16, tile=64, halo=16, device=DEV)
ALL = ("psnr", "ssim", "psnr_y", "ssim_y")
CASES = [("gaussian:9:1.6", "wrap"), ("motion:15:30", "reflect"), ("box:5", "replicate")]


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


def smooth(x):
    """A fixed 3 x 3 box blur: batch-independent, any window size."""
    return torch.nn.functional.avg_pool2d(torch.nn.functional.pad(x, (1, 1, 1, 1), mode="replicate"), 3, 1)


_CLEANS = [patch_ref.picture(k, h, w) for k, (h, w) in enumerate(((40, 56), (72, 44), (33, 47)))]
_BLURRED = {}


def cleans():
    """Three pictures; the second exceeds the 64-pixel tile, the third has odd sides."""
    return _CLEANS


def blurred(G, spec, boundary):
    """The oracle's blur of the three pictures, computed once per case; the table is the library's quantised one."""
    if (spec, boundary) not in _BLURRED:
        table = np.array(G.T.parse_blur_spec(spec).table)
        _BLURRED[spec, boundary] = [ref.blur(a, table, boundary) for a in cleans()]
        for a in _BLURRED[spec, boundary]:
            a.setflags(write=False)
    return _BLURRED[spec, boundary]


@pytest.mark.parametrize("model", [identity, smooth])
@pytest.mark.parametrize("spec,boundary", CASES)
def test_without_noise_or_shave_it_is_evaluate_pairs_on_the_oracle_blurred_inputs(G, model, spec, boundary):
    got = G.R.evaluate_deblur(model, cleans(), spec, boundary, metrics=ALL, **TILING)
    want = G.R.evaluate_pairs(model, blurred(G, spec, boundary), cleans(), metrics=ALL, **TILING)
    assert got == want and all(np.isfinite(v) for m in ALL for v in got[m][1])
    for name in ALL:
        assert got[name][0] == float(np.mean(got[name][1]))
    if model is identity:       # the restored picture is the blurred one: the PSNR of the oracle's blur against the clean
        for k, (a, b) in enumerate(zip(blurred(G, spec, boundary), cleans())):
            assert got["psnr"][1][k] == G.R.psnr_u8(a, b)
    if boundary == "wrap":      # the defaults: wrap, no noise, no shave, PSNR and SSIM; a kernel record for the spec
        short = G.I.evaluate_deblur(model, cleans(), G.T.parse_blur_spec(spec), **TILING)
        assert set(short) == {"psnr", "ssim"} and short == {m: got[m] for m in ("psnr", "ssim")}
        assert G.R.evaluate_deblur(model, cleans(), spec, 0, noise_sigma=0, shave=0, metrics=("psnr", "ssim"), **TILING) == short


@pytest.mark.parametrize("shave", [0, 5])
def test_with_a_shave_it_is_the_metric_functions_on_numpy_cropped_pictures(G, shave):
    spec, boundary = CASES[1]
    got = G.R.evaluate_deblur(smooth, cleans(), spec, boundary, shave=shave, metrics=ALL, ensemble=(0, 1), **TILING)
    for k, (clean, low) in enumerate(zip(cleans(), blurred(G, spec, boundary))):
        restored = G.R.restore_image(smooth, low, ensemble=(0, 1), **TILING)
        h, w = clean.shape[:2]
        a = np.ascontiguousarray(restored[shave:h - shave, shave:w - shave])
        b = np.ascontiguousarray(clean[shave:h - shave, shave:w - shave])
        assert a.shape == (h - 2 * shave, w - 2 * shave, 3)
        for name, fn in (("psnr", G.R.psnr_u8), ("ssim", G.R.ssim_u8), ("psnr_y", G.R.psnr_y_u8), ("ssim_y", G.R.ssim_y_u8)):
            assert got[name][1][k] == fn(a, b), (name, k)
    for name in ALL:
        assert got[name][0] == float(np.mean(got[name][1]))
    # tensors, on the host and on the device, are taken as they are
    mixed = [torch.from_numpy(cleans()[0].copy()), torch.from_numpy(cleans()[1].copy()).to(DEV), cleans()[2]]
    assert G.R.evaluate_deblur(smooth, mixed, spec, boundary, shave=shave, metrics=ALL, ensemble=(0, 1), **TILING) == got


def noisy_inputs(G, spec, boundary, sigma, seed):
    """The protocol's inputs made again: blurred / 255 plus the draws of one RandomState(seed) stream in picture order,
    cast to float32 and not quantised."""
    rs = np.random.RandomState(seed)
    out = []
    for low in blurred(G, spec, boundary):
        x = low.astype(np.float32) / np.float32(255.0)
        out.append(x + rs.normal(0, sigma / 255.0, x.shape).astype(np.float32))
    return out


@pytest.mark.parametrize("model", [identity, smooth])
@pytest.mark.parametrize("shave", [0, 3])
def test_with_noise_the_input_is_the_blurred_picture_plus_the_seeded_draws(G, model, shave):
    spec, boundary = CASES[0]
    sigma, seed = 7.65, 11
    got = G.R.evaluate_deblur(model, cleans(), spec, boundary, noise_sigma=sigma, seed=seed, shave=shave, metrics=ALL, **TILING)
    for k, (clean, x) in enumerate(zip(cleans(), noisy_inputs(G, spec, boundary, sigma, seed))):
        assert x.dtype == np.float32 and x.shape == clean.shape
        restored = G.R.restore_image(model, x, **TILING)
        h, w = clean.shape[:2]
        a = np.ascontiguousarray(restored[shave:h - shave, shave:w - shave])
        b = np.ascontiguousarray(clean[shave:h - shave, shave:w - shave])
        for name, fn in (("psnr", G.R.psnr_u8), ("ssim", G.R.ssim_u8), ("psnr_y", G.R.psnr_y_u8), ("ssim_y", G.R.ssim_y_u8)):
            assert got[name][1][k] == fn(a, b), (name, k)
    # the same seed gives the same scores, another seed and no noise give others
    again = G.R.evaluate_deblur(model, cleans(), spec, boundary, noise_sigma=sigma, seed=seed, shave=shave, metrics=ALL, **TILING)
    assert again == got
    other = G.R.evaluate_deblur(model, cleans(), spec, boundary, noise_sigma=sigma, seed=seed + 1, shave=shave, metrics=ALL, **TILING)
    plain = G.R.evaluate_deblur(model, cleans(), spec, boundary, shave=shave, metrics=ALL, **TILING)
    assert other["psnr"][1] != got["psnr"][1] and plain["psnr"][1] != got["psnr"][1]


def test_it_refuses_before_any_launch(G, monkeypatch):
    def no_launch(*a, **k):
        raise AssertionError("a kernel was launched")
    monkeypatch.setattr(G.K, "_launch", no_launch)
    pics = cleans()
    for bad in ("gauss:3:1", "box:4", 4, None):
        with pytest.raises(ValueError, match="evaluate_deblur: parse_blur_spec|evaluate_deblur: box_kernel"):
            G.R.evaluate_deblur(identity, pics, bad, **TILING)
    with pytest.raises(ValueError, match="boundary"):
        G.R.evaluate_deblur(identity, pics, "box:3", "circular", **TILING)
    with pytest.raises(ValueError, match="noise_sigma"):
        G.R.evaluate_deblur(identity, pics, "box:3", noise_sigma=-1.0, **TILING)
    with pytest.raises(ValueError, match="shave"):
        G.R.evaluate_deblur(identity, pics, "box:3", shave=-1, **TILING)
    with pytest.raises(ValueError, match="image 1 .*uint8"):
        G.R.evaluate_deblur(identity, [pics[0], pics[1].astype(np.float32)], "box:3", **TILING)
    with pytest.raises(ValueError, match="image 2 .*nothing is left"):
        G.R.evaluate_deblur(identity, pics, "box:3", shave=17, metrics=("psnr",), **TILING)
    with pytest.raises(ValueError, match="image 2 after the shave .*SSIM"):
        G.R.evaluate_deblur(identity, pics, "box:3", shave=12, **TILING)
    with pytest.raises(ValueError, match="no images"):
        G.R.evaluate_deblur(identity, [], "box:3", **TILING)
    with pytest.raises(ValueError, match="blur_u8: the boundary"):
        G.I.blur_u8(torch.zeros((8, 8, 3), dtype=torch.uint8, device=DEV), "box:3", "circular")


class Smooth(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.bias = torch.nn.Parameter(torch.zeros(1))

    def forward(self, x):
        return smooth(x) + self.bias


def test_validate_deblur_is_the_mean_of_evaluate_deblur_on_what_the_csv_dataset_yields(G, tmp_path):
    from PIL import Image
    pics = cleans()[:2]
    lines = ["index,path"]
    for k, a in enumerate(pics):
        Image.fromarray(a).save(tmp_path / f"hq{k}.png")
        lines.append(f"{k},hq{k}.png")
    (tmp_path / "val.csv").write_text("\n".join(lines) + "\n")
    conf = dict(datasets=dict(val=dict(type="TestImagesCSV", blur="motion:15:30", boundary="reflect", noise_sigma=2.55, shave=3,
                                       tile=64, halo=16,
                                       dataset_args=dict(csv_path=str(tmp_path / "val.csv"), root_folder=str(tmp_path)))))
    val_set, val_args = G.T.create_val_dataset(conf)
    assert val_args == dict(blur="motion:15:30", boundary="reflect", noise_sigma=2.55, shave=3, tile=64, halo=16, factor=16)
    assert G.T.val_check(val_set, val_args) is G.T.validate_deblur
    model = Smooth().to(DEV)
    got = G.T.validate_deblur(model, val_set, device=torch.device(DEV), **val_args)
    want = G.R.evaluate_deblur(model, pics, "motion:15:30", "reflect", noise_sigma=2.55, shave=3,
                               metrics=G.T.VAL_DEBLUR_METRICS, **TILING)
    assert got == want["psnr"][0] and np.isfinite(got)
    for metric in ("psnr_y", "ssim"):
        assert G.T.validate_deblur(model, val_set, device=torch.device(DEV), metric=metric, **val_args) == want[metric][0]
    assert want["psnr_y"][0] != got
    plain = G.T.validate_deblur(model, val_set, "motion:15:30", device=torch.device(DEV), tile=64, halo=16)
    assert plain == G.R.evaluate_deblur(model, pics, "motion:15:30", metrics=("psnr",), **TILING)["psnr"][0] and plain != got


MODEL_YAML = """name: deblur_tool
manual_seed: 2204
model:
  type: GLRImageFilter
  args: {n_channels_in: 3, n_channels_out: 3, ngraphs: 4, n_cgd_iters: 1}
"""


def test_restore_command_blur(G, tmp_path, capsys):
    """restore.py --blur prints the protocol's scores of the files it writes, without and with noise."""
    from PIL import Image
    from tests.test_restore_ref import _cli
    yaml_path = tmp_path / "rgb.yaml"
    yaml_path.write_text(MODEL_YAML)
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    pics = {"a": patch_ref.picture(3, 40, 50), "b": patch_ref.picture(4, 33, 47)}
    for name, a in pics.items():
        Image.fromarray(a).save(src / f"{name}.png")
    cli = _cli()
    base = ["-yaml_path", str(yaml_path), "--input", str(src), "--output", str(dst), "--tile", "64", "--halo", "16"]
    table = np.array(G.T.parse_blur_spec("motion:7:45").table)
    torch.manual_seed(3)
    cli.main(base + ["--blur", "motion:7:45", "--blur-boundary", "reflect", "--ssim", "--shave", "4"])
    out = capsys.readouterr().out.splitlines()
    torch.manual_seed(3)
    model = G.T.build_model(G.T.parse_options(str(yaml_path))["model"]).to(DEV).eval()
    scores = []
    for line, (name, clean) in zip(out[1:], sorted(pics.items())):
        written = np.array(Image.open(dst / f"{name}.png"))
        want = G.R.restore_image(model, ref.blur(clean, table, "reflect"), factor=16, tile=64, halo=16)
        assert np.array_equal(written, want)
        m = re.search(r"blur motion:7:45 reflect shave 4  PSNR (\d+\.\d{4}) dB  SSIM (-?\d\.\d{4})$", line)
        assert m, line
        a, b = np.ascontiguousarray(written[4:-4, 4:-4]), np.ascontiguousarray(clean[4:-4, 4:-4])
        assert m.group(1) == f"{G.R.psnr_u8(a, b):.4f}" and m.group(2) == f"{G.R.ssim_u8(a, b):.4f}"
        scores.append(G.R.psnr_u8(a, b))
    assert out[-2] == f"mean PSNR over 2 image(s): {float(np.mean(scores)):.4f} dB"
    ev = G.R.evaluate_deblur(model, [pics["a"], pics["b"]], "motion:7:45", "reflect", shave=4, metrics=("psnr",), **TILING)
    assert out[-2].endswith(f"{ev['psnr'][0]:.4f} dB")
    # with noise: the scores of evaluate_deblur under the same seed
    torch.manual_seed(3)
    cli.main(base + ["--blur", "motion:7:45", "--blur-noise", "5", "--seed", "9", "--y-channel"])
    other = capsys.readouterr().out
    assert other.count("blur motion:7:45 wrap noise 5 shave 0  PSNR-Y") == 2
    ev = G.R.evaluate_deblur(model, [pics["a"], pics["b"]], "motion:7:45", noise_sigma=5.0, seed=9, metrics=("psnr_y",), **TILING)
    assert f"mean PSNR-Y over 2 image(s): {ev['psnr_y'][0]:.4f} dB" in other
    for bad in (["--blur", "gauss:3:1"], ["--blur", "box:4"], ["--blur", "box:3", "--sigma", "5"], ["--blur-noise", "2"],
                ["--blur", "box:3", "--blur-boundary", "circular"], ["--blur", "box:3", "--psnrb"]):
        with pytest.raises(SystemExit):
            cli.main(base + bad)
    with pytest.raises(SystemExit, match="nothing is left"):
        cli.main(base + ["--blur", "box:3", "--shave", "17"])
    capsys.readouterr()
