"""restore.evaluate_jdd and training.validate_jdd on the GPU with the identity model, against PSNR and SSIM computed from
the oracle's input (tests/raw_noise_ref.py) quantised by the _img_as_ubyte rule.  Two pictures, 40 x 56 and 100 x 70 (the
second exceeds the 64-pixel tile); picture i has sample id i.  tests/test_raw_noise_ref.py holds these fixtures away from
the rounding ties of the raw samples."""
import numpy as np
import pytest
import torch

from tests import raw_noise_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TILING = dict(factor=16, tile=64, halo=16, device=DEV)


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


def cleans():
    return ref.pictures()[3:]


@pytest.mark.parametrize("pattern,fill,bits,clip", ref.WHOLE_CASES)
def test_the_scores_are_those_of_the_oracle_input_quantised(G, pattern, fill, bits, clip):
    got = G.R.evaluate_jdd(identity, cleans(), pattern, fill, ref.SHOT, ref.READ, bits, clip, ref.SEED, **TILING)
    assert set(got) == {"psnr", "ssim"}
    psnrs, ssims = [], []
    for i, clean in enumerate(cleans()):
        h, w = clean.shape[:2]
        want = ref.sample(clean, pattern, 0, 0, 0, h, w, ref.SHOT, ref.read_b(ref.READ), ref.SEED, i, fill, bits, clip)
        assert want[3] >= ref.TIE_MARGIN
        shown = G.T._img_as_ubyte(np.clip(want[1].transpose(1, 2, 0), 0.0, 1.0))
        psnrs.append(G.R.psnr_u8(shown, clean))
        ssims.append(G.R.ssim_u8(shown, clean))
    assert got["psnr"][1] == psnrs and got["ssim"][1] == ssims
    assert got["psnr"][0] == float(np.mean(psnrs)) and got["ssim"][0] == float(np.mean(ssims))
    # a picture's noise is a function of (seed, its index): the second alone, as picture 0, scores differently
    alone = G.R.evaluate_jdd(identity, cleans()[1:], pattern, fill, ref.SHOT, ref.READ, bits, clip, ref.SEED, **TILING)
    assert alone["psnr"][1][0] != got["psnr"][1][1]
    mean = G.T.validate_jdd(identity, cleans(), [ref.SHOT, ref.READ], pattern, fill, bits, clip, ref.SEED,
                            device=torch.device(DEV), tile=64, halo=16)
    assert mean == got["psnr"][0]
    assert G.T.validate_jdd(identity, cleans(), [ref.SHOT, ref.READ], pattern, fill, bits, clip, ref.SEED, metric="ssim",
                            device=torch.device(DEV), tile=64, halo=16) == got["ssim"][0]


def test_without_noise_at_8_bits_it_is_close_to_evaluate_demosaic_and_noise_lowers_the_psnr(G):
    quiet = G.I.evaluate_jdd(identity, cleans(), "rggb", "malvar", bits=8, shave=2, **TILING)
    plain = G.R.evaluate_demosaic(identity, cleans(), "rggb", "malvar", shave=2, **TILING)
    noisy = G.R.evaluate_jdd(identity, cleans(), "rggb", "malvar", 0.02, 10.0, shave=2, **TILING)
    # the same sums, rounded to bytes once (x 255 / 4080) in place of (s + 8) >> 4: the same picture up to ties
    assert abs(quiet["psnr"][0] - plain["psnr"][0]) < 0.05
    # independent zero-mean noise of variance >= (10 / 255)^2 under the fill adds its filtered variance to the MSE of
    # each of the 2 x 6720 + 2 x 21000 scored values: hundreds of standard errors, so the PSNR is strictly lower
    assert all(n < q for n, q in zip(noisy["psnr"][1], quiet["psnr"][1]))


MODEL_YAML = """name: jdd_tool
manual_seed: 2204
model:
  type: GLRImageFilter
  args: {n_channels_in: 3, n_channels_out: 3, ngraphs: 4, n_cgd_iters: 1}
"""


def test_restore_command_raw_noise(G, tmp_path, capsys):
    """restore.py --bayer P --raw-noise SHOT,READ prints evaluate_jdd's scores of the files it writes: file i has sample
    id i, with and without --batch-images."""
    import re
    from PIL import Image
    from tests.test_restore_ref import _cli
    yaml_path = tmp_path / "rgb.yaml"
    yaml_path.write_text(MODEL_YAML)
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    pics = {"a": cleans()[0], "b": cleans()[1]}
    for name, a in pics.items():
        Image.fromarray(a).save(src / f"{name}.png")
    cli = _cli()
    base = ["-yaml_path", str(yaml_path), "--input", str(src), "--output", str(dst), "--tile", "64", "--halo", "16"]
    flags = ["--bayer", "grbg", "--raw-noise", "0.01,5", "--raw-bits", "12", "--raw-seed", "9", "--ssim", "--shave", "4"]
    torch.manual_seed(3)
    model = G.T.build_model(G.T.parse_options(str(yaml_path))["model"]).to(DEV).eval()
    want = G.R.evaluate_jdd(model, [pics["a"], pics["b"]], "grbg", "malvar", 0.01, 5.0, 12, True, 9, shave=4, **TILING)
    for extra in ([], ["--batch-images"]):
        torch.manual_seed(3)
        cli.main(base + flags + extra)
        out = capsys.readouterr().out.splitlines()
        for k, (line, name) in enumerate(zip(out[1:], sorted(pics))):
            m = re.search(r"bayer grbg malvar raw noise shot 0.01 read 5 12 bits shave 4  PSNR (\d+\.\d{4}) dB  "
                          r"SSIM (-?\d\.\d{4})$", line)
            assert m, line
            if extra:       # windows of both files share the model's batches: the same lines, not the same floats
                continue
            assert m.group(1) == f"{want['psnr'][1][k]:.4f}" and m.group(2) == f"{want['ssim'][1][k]:.4f}"
            written = np.array(Image.open(dst / f"{name}.png"))
            filled = G.R.raw_noise_demosaic_u8(pics[name], "grbg", "malvar", 0.01, 5.0, 12, True, 9, k)
            assert np.array_equal(written, G.R.restore_image(model, filled, factor=16, tile=64, halo=16))
        if not extra:
            assert out[-2] == f"mean PSNR over 2 image(s): {want['psnr'][0]:.4f} dB"
    with pytest.raises(SystemExit):
        cli.main(base + ["--raw-noise", "0.01,5"])
    capsys.readouterr()
