"""restore.evaluate_inpaint, restore.mask_fill_u8, training.validate_inpaint and restore.py --inpaint-keep / --mask on the
GPU, with cheap callable models (the identity and a fixed 3 x 3 blur, as the restoration tests use) and the oracle
tests/inpaint_ref.py for the mask and the fill.  Every score is compared with == : the sums are exact integers."""
import re

import numpy as np
import pytest
import torch

from tests import inpaint_ref as ref, patch_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TILING = dict(factor=16, tile=64, halo=16, device=DEV)
SEED = 2204


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


CLEANS = [patch_ref.picture(k, h, w) for k, (h, w) in enumerate(((40, 56), (72, 44), (33, 47)))]


def psnr(sse, n):
    return float("inf") if sse == 0 else float(10.0 * np.log10(255.0 ** 2 * n / sse))


def sse_of(a, b):
    return int(((a.astype(np.int64) - b.astype(np.int64)) ** 2).sum())


def oracle_fill(G, clean, i, keep, fill, side, sigma, hole, passes=1, seed=SEED):
    """(filled, known 0 / 1) of picture i of a call from the oracle."""
    table = G.K.mask_weights(side, sigma)
    filled, code = ref.mask_fill_image(clean, None, G.K.keep_units(keep), seed, i, table, fill, hole)
    known = (code == 1).astype(np.uint8)
    for _ in range(passes - 1):
        filled, code = ref.mask_fill_image(filled, code, 0, seed, i, table, fill, hole)
    return filled, known


@pytest.mark.parametrize("model", [identity, smooth])
@pytest.mark.parametrize("keep,fill,side,sigma,passes,keep_known,shave", [
    (0.2, "conv", 7, None, 1, True, 0), (0.5, "conv", 5, 1.2, 2, True, 3), (0.05, "conv", 3, None, 3, False, 0),
    (0.8, "zero", 7, None, 1, True, 2)])
def test_the_scores_are_those_of_the_oracles_filled_pictures(G, model, keep, fill, side, sigma, passes, keep_known, shave):
    metrics = ("psnr", "psnr_missing", "ssim", "psnr_y")
    got = G.R.evaluate_inpaint(model, CLEANS, keep, fill, side, sigma, 99, SEED, passes, keep_known, shave, metrics=metrics,
                               **TILING)
    for i, clean in enumerate(CLEANS):
        filled, known = oracle_fill(G, clean, i, keep, fill, side, sigma, 99, passes)
        restored = filled if model is identity else G.R.restore_image(model, filled, factor=16, tile=64, halo=16)
        if keep_known:
            restored = np.where(known[:, :, None] != 0, clean, restored)
        cut = (lambda a: np.ascontiguousarray(a[shave:a.shape[0] - shave, shave:a.shape[1] - shave])) if shave else (lambda a: a)
        r, c, k = cut(restored), cut(clean), cut(known)
        assert got["psnr"][1][i] == psnr(sse_of(r, c), c.size) == G.R.psnr_u8(r, c)
        assert got["ssim"][1][i] == G.R.ssim_u8(r, c) and got["psnr_y"][1][i] == G.R.psnr_y_u8(r, c)
        merged = np.where(k[:, :, None] != 0, c, r)
        missing = int((k == 0).sum())
        assert 0 < missing < k.size
        assert got["psnr_missing"][1][i] == psnr(sse_of(merged, c), 3 * missing) == G.R.psnr_missing_u8(r, c, k)
        if keep_known:      # one SSE, two counts: the two differ by the missing share exactly as defined
            sse = sse_of(r, c)
            assert got["psnr_missing"][1][i] == psnr(sse, 3 * missing) and got["psnr"][1][i] == psnr(sse, 3 * k.size)
            assert got["psnr_missing"][1][i] < got["psnr"][1][i]
    for name in metrics:
        assert got[name][0] == float(np.mean(got[name][1]))


def test_everything_known_scores_inf_and_defaults(G):
    got = G.I.evaluate_inpaint(smooth, CLEANS, 1.0, metrics=("psnr", "psnr_missing"), **TILING)
    assert got["psnr"][1] == [float("inf")] * 3 and got["psnr_missing"][1] == [float("inf")] * 3
    loose = G.R.evaluate_inpaint(smooth, CLEANS, 1.0, keep_known=False, metrics=("psnr", "psnr_missing"), **TILING)
    assert all(np.isfinite(v) for v in loose["psnr"][1]) and loose["psnr_missing"][1] == [float("inf")] * 3
    short = G.R.evaluate_inpaint(identity, CLEANS, 0.3, **TILING)
    assert set(short) == {"psnr"}
    assert short == G.R.evaluate_inpaint(identity, CLEANS, 0.3, "conv", 7, None, 128, 2204, 1, True, 0, 16, 1, ("psnr",),
                                         tile=64, halo=16, device=DEV)
    val = G.T.validate_inpaint(identity, CLEANS, 0.3, device=DEV, tile=64, halo=16)
    assert val == short["psnr"][0]
    val = G.T.validate_inpaint(identity, [c.astype(np.float32) / 255.0 for c in CLEANS], 0.3, metric="psnr_missing", device=DEV,
                               tile=64, halo=16)
    assert val == G.R.evaluate_inpaint(identity, CLEANS, 0.3, metrics=("psnr_missing",), **TILING)["psnr_missing"][0]


def test_mask_fill_u8_kinds_and_passes(G):
    clean = CLEANS[0]
    filled, known = G.I.mask_fill_u8(clean, keep=0.3, seed=5, sample_id=2)
    want, code = ref.mask_fill_image(clean, None, G.K.keep_units(0.3), 5, 2, G.K.mask_weights(7), "conv", 128)
    assert isinstance(filled, np.ndarray) and np.array_equal(filled, want) and np.array_equal(known, (code == 1).astype(np.uint8))
    t = torch.from_numpy(clean)
    for kind in (t, t.to(DEV)):
        f, k = G.I.mask_fill_u8(kind, keep=0.3, seed=5, sample_id=2)
        assert f.device == kind.device and k.device == kind.device and np.array_equal(f.cpu().numpy(), want)
    given = np.ones(clean.shape[:2], bool)
    given[:, 20:40] = False
    table = G.K.mask_weights(7, 2.0)
    cur, cur_mask = clean, given.astype(np.uint8)
    for passes in (1, 2, 4):
        f, k = G.I.mask_fill_u8(clean, mask=given, weights=table, hole=7, passes=passes)
        cur, cur_mask = clean, given.astype(np.uint8)
        for _ in range(passes):
            cur, cur_mask = ref.mask_fill_image(cur, cur_mask, 0, 0, 0, table, "conv", 7)
        assert np.array_equal(f, cur) and np.array_equal(k, given.astype(np.uint8))
        assert ((f[:, 29:31] == 7).all()) == (passes < 4)                        # the middle of the hole closes last
    as_u8 = G.I.mask_fill_u8(clean, mask=given.astype(np.uint8) * 255, weights=table, hole=7, passes=4)
    assert np.array_equal(as_u8[0], cur)


MODEL_YAML = """
name: rgb
manual_seed: 2204
model:
  type: GLRImageFilter
  args: {n_channels_in: 3, n_channels_out: 3, ngraphs: 4, n_cgd_iters: 1}
"""


def test_restore_command_inpaint_keep_and_mask(G, tmp_path, capsys):
    """restore.py --inpaint-keep prints the protocol's scores of the files it writes; --mask fills, restores and puts the
    known pixels of the input back."""
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
    torch.manual_seed(3)
    cli.main(base + ["--inpaint-keep", "0.25", "--mask-fill-side", "5", "--mask-seed", "9"])
    out = capsys.readouterr().out.splitlines()
    torch.manual_seed(3)
    model = G.T.build_model(G.T.parse_options(str(yaml_path))["model"]).to(DEV).eval()
    scores, missing = [], []
    for i, (line, (name, clean)) in enumerate(zip(out[1:], sorted(pics.items()))):
        written = np.array(Image.open(dst / f"{name}.png"))
        filled, known = oracle_fill(G, clean, i, 0.25, "conv", 5, None, 128, seed=9)
        want = np.where(known[:, :, None] != 0, clean, G.R.restore_image(model, filled, factor=16, tile=64, halo=16))
        assert np.array_equal(written, want)
        m = re.search(r"inpaint keep 0.25 conv seed 9  PSNR (\d+\.\d{4}) dB  PSNR-missing (\d+\.\d{4}) dB$", line)
        assert m, line
        assert m.group(1) == f"{G.R.psnr_u8(written, clean):.4f}"
        assert m.group(2) == f"{G.R.psnr_missing_u8(written, clean, known):.4f}"
        scores.append(G.R.psnr_u8(written, clean))
        missing.append(G.R.psnr_missing_u8(written, clean, known))
    assert out[-2] == f"mean PSNR over 2 image(s): {float(np.mean(scores)):.4f} dB"
    assert out[-1] == f"mean PSNR-missing over 2 image(s): {float(np.mean(missing)):.4f} dB"
    ev = G.R.evaluate_inpaint(model, [pics["a"], pics["b"]], 0.25, fill_side=5, seed=9, metrics=("psnr", "psnr_missing"), **TILING)
    assert out[-2].endswith(f"{ev['psnr'][0]:.4f} dB") and out[-1].endswith(f"{ev['psnr_missing'][0]:.4f} dB")
    # --mask: pictures with holes and the files that say where
    holes, masks, truth = tmp_path / "holes", tmp_path / "masks", tmp_path / "truth"
    for d in (holes, masks, truth):
        d.mkdir()
    knowns = {}
    for name, clean in pics.items():
        known = np.ones(clean.shape[:2], bool)
        known[5:9, :] = False                  # a scratch
        known[20:30, 10:22] = False            # a block
        knowns[name] = known
        Image.fromarray(clean * known[:, :, None].astype(np.uint8)).save(holes / f"{name}.png")
        Image.fromarray(known.astype(np.uint8) * 255).save(masks / f"{name}.png")
        Image.fromarray(clean).save(truth / f"{name}.png")
    dst2 = tmp_path / "out2"
    mask_base = ["-yaml_path", str(yaml_path), "--input", str(holes), "--output", str(dst2), "--tile", "64", "--halo", "16",
                 "--mask", str(masks), "--mask-fill-passes", "3"]
    torch.manual_seed(3)
    cli.main(mask_base)
    plain = capsys.readouterr().out
    assert "PSNR" not in plain
    table = G.K.mask_weights(7)
    for name, clean in sorted(pics.items()):
        written = np.array(Image.open(dst2 / f"{name}.png"))
        known = knowns[name]
        given = clean * known[:, :, None].astype(np.uint8)
        assert np.array_equal(written[known], given[known])                      # the known pixels are the input's
        cur, cur_mask = given, known.astype(np.uint8)
        for _ in range(3):
            cur, cur_mask = ref.mask_fill_image(cur, cur_mask, 0, 0, 0, table, "conv", 128)
        assert (cur_mask != 0).all()
        want = np.where(known[:, :, None], given, G.R.restore_image(model, cur, factor=16, tile=64, halo=16))
        assert np.array_equal(written, want)
    torch.manual_seed(3)
    cli.main(mask_base + ["--reference", str(truth)])
    scored = capsys.readouterr().out
    assert scored.count("PSNR-missing") == 3 and "mean PSNR over 2 image(s)" in scored
    for name, clean in pics.items():
        written = np.array(Image.open(dst2 / f"{name}.png"))
        assert f"PSNR {G.R.psnr_u8(written, clean):.4f} dB  PSNR-missing {G.R.psnr_missing_u8(written, clean, knowns[name]):.4f} dB" in scored
    # nonzero means missing with --mask-white-missing: the inverted files give the same pictures
    inverted, dst3 = tmp_path / "inverted", tmp_path / "out3"
    inverted.mkdir()
    for name, known in knowns.items():
        Image.fromarray((~known).astype(np.uint8) * 255).save(inverted / f"{name}.png")
    torch.manual_seed(3)
    cli.main(["-yaml_path", str(yaml_path), "--input", str(holes), "--output", str(dst3), "--tile", "64", "--halo", "16",
              "--mask", str(inverted), "--mask-white-missing", "--mask-fill-passes", "3"])
    capsys.readouterr()
    for name in pics:
        assert np.array_equal(np.array(Image.open(dst3 / f"{name}.png")), np.array(Image.open(dst2 / f"{name}.png")))
    (masks / "b.png").unlink()
    with pytest.raises(SystemExit, match="--mask: .*b.png has no mask"):
        cli.main(mask_base)
    Image.fromarray(np.zeros((5, 5), np.uint8)).save(masks / "b.png")
    with pytest.raises(SystemExit, match="a mask is a 1-channel file of the input's size"):
        cli.main(mask_base)
    capsys.readouterr()
