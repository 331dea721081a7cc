"""train.ssim_weight on the CPU: at 0 or absent the Trainer's loss is the parent formula bit for bit and
losses.ssim_loss is never reached; a bad weight raises at construction; a weight > 0 reaches the HIP wrapper, which
has no CPU path and refuses patches smaller than the window.  tests/test_gpu_ssim_loss.py runs the weighted loss."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

from irdu_amd import losses
from irdu_amd import training as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class TinyModel(torch.nn.Module):       # tests/test_training.py's stand-in
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Conv2d(3, 4, 3, padding=1, bias=False)
        self.b = torch.nn.Conv2d(4, 3, 1, bias=False)

    def encode(self, x):
        return (self.a(x),)

    def decode(self, lat):
        return self.b(lat[0])

    def forward(self, x):
        return self.decode(self.encode(x))


def parent_loss(tr, noisy, clean):
    """Trainer.loss as it was before train.ssim_weight existed."""
    m = tr.model
    loss = F.l1_loss(m(noisy), clean)
    latent = m.encode(clean)
    rec = m.decode(latent)
    disturbed = m.decode(tuple(t + torch.normal(0.0, tr.latent_noise, size=t.shape, device=t.device) for t in latent))
    loss = loss + tr.w_encdec * F.mse_loss(rec, clean)
    return loss + tr.w_perturb * F.mse_loss(rec, disturbed)


@pytest.mark.parametrize("tconf", [{}, {"ssim_weight": 0}, {"ssim_weight": 0.0}, {"ssim_weight": None}])
def test_zero_or_absent_weight_is_the_parent_loss_and_never_calls_the_op(monkeypatch, tconf):
    calls = []
    monkeypatch.setattr(losses, "ssim_loss", lambda *a, **k: calls.append(a) or torch.zeros(()))
    torch.manual_seed(3)
    tr = T.Trainer(TinyModel(), dict(tconf), torch.device("cpu"))
    assert tr.w_ssim == 0.0
    noisy, clean = torch.rand(2, 3, 16, 16), torch.rand(2, 3, 16, 16)
    torch.manual_seed(11)          # the latent-perturbation term draws noise
    got = tr.loss(noisy, clean)
    torch.manual_seed(11)
    want = parent_loss(tr, noisy, clean)
    assert torch.equal(got, want) and got.dtype == torch.float32
    hwc = lambda t: t.permute(0, 2, 3, 1).contiguous()      # noqa: E731
    assert math.isfinite(tr.step(hwc(noisy), hwc(clean)))
    assert calls == []


def test_positive_weight_adds_the_weighted_op(monkeypatch):
    calls = []

    def fake(out, clean):
        calls.append((out, clean))
        return (out - clean).pow(2).mean()
    monkeypatch.setattr(losses, "ssim_loss", fake)
    torch.manual_seed(3)
    tr = T.Trainer(TinyModel(), {"ssim_weight": 0.25, "loss02_weight": 0.0, "loss03_weight": 0.0}, torch.device("cpu"))
    noisy, clean = torch.rand(2, 3, 16, 16), torch.rand(2, 3, 16, 16)
    got = tr.loss(noisy, clean)
    out = tr.model(noisy)
    assert torch.equal(got, F.l1_loss(out, clean) + 0.25 * fake(out, clean))
    assert len(calls) == 2 and calls[0][1] is clean and calls[0][0].requires_grad


@pytest.mark.parametrize("bad", [-0.1, -1, float("nan"), float("inf"), -float("inf"), "-0.2"])
def test_negative_or_non_finite_weight_raises_at_construction(bad):
    with pytest.raises(ValueError, match="ssim_weight"):
        T.Trainer(TinyModel(), {"ssim_weight": bad}, torch.device("cpu"))


def test_positive_weight_on_the_cpu_has_no_path_and_small_patches_are_refused():
    tr = T.Trainer(TinyModel(), {"ssim_weight": 0.2}, torch.device("cpu"))
    assert tr.w_ssim == 0.2
    with pytest.raises(RuntimeError, match="no CPU path"):
        tr.loss(torch.rand(2, 3, 16, 16), torch.rand(2, 3, 16, 16))
    with pytest.raises(ValueError, match="at least 11"):
        tr.loss(torch.rand(2, 3, 10, 16), torch.rand(2, 3, 10, 16))
    with pytest.raises(ValueError, match="at least 11"):
        tr.step(torch.rand(2, 16, 8, 3), torch.rand(2, 16, 8, 3))


def test_example_yaml_is_the_paired_example_plus_the_weight():
    conf = T.parse_options(os.path.join(ROOT, "experiment_conf", "ssim_loss_example.yaml"))
    base = T.parse_options(os.path.join(ROOT, "experiment_conf", "paired_example.yaml"))
    assert conf["train"].pop("ssim_weight") == 0.2 and conf.pop("name") == "ssim_loss_example"
    base.pop("name")
    assert conf == base
