"""A compiled ``l1 + 0.2 ssim_loss`` training step on CPU fake tensors, graphs only (the recording backend of
tests/test_compile_training.py): the loss reaches AOTAutograd as one opaque ``irdu::ssim_loss`` node in the forward
graph and one ``irdu::ssim_loss_backward`` node in the backward graph, and no convolution appears for the window.
No kernel runs here; tests/test_gpu_ssim_loss.py runs the op."""
import torch
import torch.nn.functional as F

import irdu_amd
from tests.test_compile_training import _record, _targets


class Scale(torch.nn.Module):           # no convolution of its own: any aten.convolution would be the loss's
    def __init__(self):
        super().__init__()
        self.gain = torch.nn.Parameter(torch.full((1, 3, 1, 1), 0.9))
        self.bias = torch.nn.Parameter(torch.zeros(1, 3, 1, 1))

    def forward(self, x):
        return x * self.gain + self.bias


def test_compiled_step_keeps_the_loss_opaque():
    torch._dynamo.reset()
    backend, graphs = _record()
    m = Scale()

    def objective(x, c):
        out = m(x)
        return F.l1_loss(out, c) + 0.2 * irdu_amd.ssim_loss(out, c)

    loss = torch.compile(objective, backend=backend)(torch.rand(2, 3, 32, 40), torch.rand(2, 3, 32, 40))
    assert loss.shape == () and loss.dtype == torch.float32
    loss.backward()
    fw, bw = _targets(graphs["fw"]), _targets(graphs["bw"])
    assert fw.get("irdu.ssim_loss.default") == 1, fw
    assert bw.get("irdu.ssim_loss_backward.default") == 1, bw
    assert "irdu.ssim_loss_backward.default" not in fw and "irdu.ssim_loss.default" not in bw
    for name in ("aten.convolution", "aten.conv2d", "aten._convolution"):
        assert not any(k.startswith(name) for k in list(fw) + list(bw)), name
    assert m.gain.grad is not None and m.gain.grad.shape == m.gain.shape and m.bias.grad is not None


def test_fake_kernels_give_the_shapes_of_the_real_ones():
    op = irdu_amd.losses.SSIM_LOSS
    x = torch.empty(2, 3, 32, 40, device="meta")
    outs, saved = op.fake([1], x, x)
    assert outs[0].shape == () and outs[0].dtype == torch.float32
    assert saved[0].shape == (3, 2, 3, 22, 30) and saved[0].dtype == torch.float64
    outs, saved = op.fake([0], x, x)
    assert saved[0].numel() == 0 and saved[0].dtype == torch.float64       # no planes without a gradient
