"""The scores of the three degrade-from-clean protocols on gfx950, pinned: every float that restore.evaluate_sr,
evaluate_car and evaluate_demosaic and training.validate_sr, validate_car and validate_demosaic return, as float.hex(),
against tests/golden/protocol_scores_gfx950.json, which scripts/record_protocol_scores.py wrote from the build of the
commit named in the file.  The scores come from exact integer sums, so they are compared for equality; a change to the
host code around the kernels that is meant to keep behaviour passes unchanged.

  pictures    patch_ref.picture(k, h, w) for (40, 56), (72, 44: beyond the 64-pixel tile) and (33, 47: odd sides, so
              the x4 mod-crop cuts both)
  models      the identity and the fixed 3 x 3 box blur of the evaluation tests; tile 64, halo 16, factor 16
  metrics     psnr, ssim, psnr_y, ssim_y, and psnrb for JPEG
  parameters  SR x2 with the default shave and x4 with shave 0; JPEG quality 10 at 4:4:4 and 40 at 4:2:0; demosaic
              rggb / malvar with shave 0 and gbrg / bilinear with shave 3; ensemble 1, and (0, 1) once per protocol
  validators  each metric of VAL_*_METRICS on the first parameter set, on uint8 pictures and on float32 ones in [0, 1]
"""
import json
import os

import numpy as np
import pytest
import torch

from tests import patch_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ARCH = "gfx950"
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "protocol_scores_gfx950.json")
TILING = dict(factor=16, tile=64, halo=16, device=DEV)
ALL = ("psnr", "ssim", "psnr_y", "ssim_y")


def device_arch():
    return torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]


def identity(x):
    return x


def blur(x):
    """A fixed 3 x 3 box blur: batch-independent, any window size."""
    return torch.nn.functional.avg_pool2d(torch.nn.functional.pad(x, (1, 1, 1, 1), mode="replicate"), 3, 1)


MODELS = {"identity": identity, "blur": blur}


def cleans():
    return [patch_ref.picture(k, h, w) for k, (h, w) in enumerate(((40, 56), (72, 44), (33, 47)))]


def hexed(scores):
    """{metric: (mean, values)} with every float as float.hex()."""
    return {m: [float(mean).hex(), [float(v).hex() for v in values]] for m, (mean, values) in scores.items()}


def _group(evaluate, validate, val_metrics, metrics, param_sets):
    """One protocol's scores: every parameter set under both models, the first once more with ensemble (0, 1), and the
    validator's mean for each of its metrics on uint8 and on float32 pictures."""
    pics, out = cleans(), {}
    for tag, args, kw in param_sets:
        for name, model in MODELS.items():
            out[f"{tag}/{name}/e1"] = hexed(evaluate(model, pics, *args, metrics=metrics, ensemble=1, **kw, **TILING))
    tag, args, kw = param_sets[0]
    out[f"{tag}/blur/e01"] = hexed(evaluate(blur, pics, *args, metrics=metrics, ensemble=(0, 1), **kw, **TILING))
    floats = [p.astype(np.float32) / 255.0 for p in pics]
    for metric in val_metrics:
        for kind, images in (("u8", pics), ("f32", floats)):
            out[f"validate/{tag}/{metric}/{kind}"] = float(validate(
                blur, images, *args, factor=16, device=torch.device(DEV), metric=metric, tile=64, halo=16)).hex()
    return out


def sr_scores(R, T):
    return _group(R.evaluate_sr, T.validate_sr, T.VAL_SR_METRICS, ALL,
                  [("sr/x2-shave-default", (2,), {}), ("sr/x4-shave0", (4,), dict(shave=0))])


def car_scores(R, T):
    return _group(R.evaluate_car, T.validate_car, T.VAL_CAR_METRICS, ALL + ("psnrb",),
                  [("car/q10-444", (10, 0), {}), ("car/q40-420", (40, 2), {})])


def demosaic_scores(R, T):
    return _group(R.evaluate_demosaic, T.validate_demosaic, T.VAL_DEMOSAIC_METRICS, ALL,
                  [("demosaic/rggb-malvar-shave0", ("rggb", "malvar"), dict(shave=0)),
                   ("demosaic/gbrg-bilinear-shave3", ("gbrg", "bilinear"), dict(shave=3))])


GROUPS = {"sr": sr_scores, "car": car_scores, "demosaic": demosaic_scores}


def all_scores(R, T):
    """Every pinned score, {name: hex strings} (scripts/record_protocol_scores.py writes these into the fixture)."""
    out = {}
    for fn in GROUPS.values():
        out.update(fn(R, T))
    return out


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if device_arch() != ARCH:
        pytest.skip(f"the scores are {ARCH}'s (this device: {device_arch()})")
    import irdu_amd
    irdu_amd.load_native()
    from irdu_amd import restore, training
    return restore, training


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        fx = json.load(f)
    assert fx["arch"] == ARCH and len(fx["commit"]) == 40, fx
    return fx


def test_fixture_names_every_score(golden):
    names = set(golden["scores"])
    assert len(names) == 3 * (2 * 2 + 1) + 2 * (2 + 3 + 3)
    assert {n.split("/")[0] for n in names} == {"sr", "car", "demosaic", "validate"}


@pytest.mark.parametrize("group", list(GROUPS))
def test_scores_unchanged(G, golden, group):
    got = GROUPS[group](*G)
    for name, score in got.items():
        print(f"{name}: {score}  (recorded at {golden['commit'][:12]}: {golden['scores'].get(name)})")
    bad = [name for name, score in got.items() if golden["scores"].get(name) != score]
    assert not bad, f"scores moved against commit {golden['commit'][:12]}: {bad}"
