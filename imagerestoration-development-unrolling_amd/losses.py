"""Training losses on the HIP kernels.

``ssim_loss(pred, target)`` is ``1 - SSIM``: the index ``restore.ssim_u8`` and the validators score with (11 x 11
Gaussian window, sigma 1.5, valid positions only), on the model's own float32 planar ``[B, C, H, W]`` batches of
data range 1, neither operand clamped, so the loss has a gradient wherever the model's output lies.  Forward and
reverse are one HIP kernel each (``csrc/ssim_loss_ops.hip``; ``include/grr.h`` has the definition), float64 from the
float32 operands up to the one rounding of the result:

* forward: the exact integer sum of ``q = rint(2^32 s)`` per batch item, the same on every run and independent of the
  grid, and three float64 coefficient planes ``[3, B, C, H - 10, W - 10]``, written only where the prediction takes a
  gradient.  The loss ``1 - sum q / (2^32 N)`` is formed in float64 on the device (no synchronisation) and rounded
  once to the prediction's dtype; equal operands give exactly 0.
* reverse: a gather over the coefficient planes, no atomics: bitwise repeatable.  The incoming gradient is read from
  the device.

The pair is a ``train_ops.OpaqueFunction``: under ``model.compile()`` it reaches AOTAutograd as one
``irdu::ssim_loss`` node and one ``irdu::ssim_loss_backward`` node.  Only the prediction takes a gradient; a target
that requires one is an error.  There is no CPU path.
"""
from typing import List

import torch
from torch import Tensor, nn

from . import kernels as K
from .train_ops import OpaqueFunction


def _shape(x: Tensor):
    b, c, h, w = x.shape
    return (3, b, c, h - K.SSIM_WINDOW + 1, w - K.SSIM_WINDOW + 1)


# consts = [want_coef]: 1 where the prediction takes a gradient; else the saved tensor is an empty placeholder
def _ssim_fwd(consts, x: Tensor, y: Tensor):
    qsum, coef = K.ssim_loss_forward(x, y, bool(consts[0]))
    n = K.ssim_loss_count(*x.shape)
    # sum q is an exact int64; N 2^32 is exact in float64 (N < 2^31), so equal operands give 1 - 1
    loss = (1.0 - qsum.sum().double() / float(K.SSIM_ONE * n)).to(x.dtype)
    return [loss], [coef if coef is not None else x.new_empty(0, dtype=torch.float64)]


def _ssim_bwd(consts, inputs, outs, saved, gouts, needs):
    x, y = inputs
    if len(needs) > 1 and needs[1]:
        raise ValueError("ssim_loss: the target takes no gradient")
    if not needs[0]:
        return None, None
    if not consts[0]:
        raise RuntimeError("ssim_loss: the forward ran without the coefficient planes")
    return K.ssim_loss_backward(x, y, saved[0], gouts[0].contiguous()), None


def _ssim_fake(consts, x: Tensor, y: Tensor):
    return [x.new_empty(())], [x.new_empty(_shape(x) if consts[0] else (0,), dtype=torch.float64)]


SSIM_LOSS = OpaqueFunction("ssim_loss", 1, _ssim_fwd, _ssim_bwd, _ssim_fake)


def ssim_loss(pred: Tensor, target: Tensor) -> Tensor:
    """1 - SSIM(pred, target) of two float32 ``[B, C, H, W]`` device batches with H, W >= 11, as a 0-dim tensor of
    ``pred``'s dtype; differentiable in ``pred``.  ValueError on a shape or dtype the kernels do not take (a side
    below the window's 11 among them) and on a target that requires grad; RuntimeError off the GPU."""
    if isinstance(target, Tensor) and target.requires_grad:
        raise ValueError("ssim_loss: the target takes no gradient (detach it)")
    if not (isinstance(pred, Tensor) and isinstance(target, Tensor)):
        raise ValueError("ssim_loss: expected two tensors")
    want = int(pred.requires_grad and torch.is_grad_enabled())
    pred, target = pred.contiguous(), target.contiguous()
    K._check_ssim_loss("ssim_loss", pred, target, placed=False)      # the wrapper checks the device at the launch
    return SSIM_LOSS([want], pred, target)


class SSIMLoss(nn.Module):
    """``ssim_loss`` as a module: ``SSIMLoss()(pred, target)``."""

    def forward(self, pred: Tensor, target: Tensor) -> Tensor:
        return ssim_loss(pred, target)


def ssim_loss_sums(pred: Tensor, target: Tensor) -> List[int]:
    """The exact per-item sums of q = rint(2^32 s) as Python ints (synchronises; for tests and logging): item b's
    SSIM is sums[b] / (2^32 C (H - 10)(W - 10))."""
    qsum, _ = K.ssim_loss_forward(pred.detach().contiguous(), target.detach().contiguous(), False)
    return [int(v) for v in qsum.tolist()]
