"""The SSIM training loss on the GPU (csrc/ssim_loss_ops.hip through irdu_amd.ssim_loss) against the numpy float64
restatement tests/ssim_loss_ref.py alone: no torch reference, nothing read from outside the repository.

Bounds.
  forward   |sum q / (2^32 N) - mean of the restatement's s| <= 2^-32: each q = rint(2^32 s) is within half a step of
            2^32 s, the integer sum is exact, and the device's and numpy's float64 s differ by rounding order, orders
            of magnitude below the step (tests/test_gpu_ssim.py derives the same bound for the uint8 metric).
  reverse   |g - g_ref| <= 2^-24 |g_ref| + 1e-11 max|g_ref| elementwise: the single rounding to float32 plus the
            float64 order term, whose reference-alone size tests/test_ssim_loss_ref.py measures (<= 3e-13 max|g|).
  equal     x = y: exactly N 2^32 per item, loss exactly 0.0, max|g| <= 1e-10 / N (the analytic gradient is 0; terms of
            size <= 2 / C2 cancel in float64).
"""
import numpy as np
import pytest
import torch

from tests import ssim_loss_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
STEP = 2.0 ** -32
ONE = 1 << 32


@pytest.fixture(scope="module")
def irdu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import irdu_amd
    irdu_amd.load_native()
    return irdu_amd


def edge_shapes():
    """From the kernels' tile: one below, at and one above a tile in the valid width and height (forward) and in
    the full width and height (reverse), the other side at 11..13, B = C = 1; one valid position; two tiles both
    ways with several planes."""
    from irdu_amd import kernels as K
    rows, cols = K.SSIM_LOSS_TILE
    shapes = [(1, 1, 12, cols + 10 + d) for d in (-1, 0, 1)] + [(1, 1, rows + 10 + d, 13) for d in (-1, 0, 1)]
    shapes += [(1, 1, 11, cols + d) for d in (-1, 0, 1)] + [(1, 1, rows + d, 12) for d in (-1, 0, 1)]
    shapes += [(1, 1, 11, 11), (2, 3, rows + 13, cols + 14)]
    return shapes


CASES = [(kind, shape) for kind, shapes in R.KINDS.items() for shape in shapes]
CASES += [("noisy", shape) for shape in edge_shapes()]
_REF = {}


def reference(kind, shape):
    """(x, y, loss, gradient, per-item means of s) of the restatement, computed once per case and left unchanged."""
    key = (kind, tuple(shape))
    if key not in _REF:
        x, y = R.pair(kind, shape)
        loss, g = R.loss_and_grad(x, y)
        for a in (x, y, g):
            a.setflags(write=False)
        _REF[key] = (x, y, loss, g, R.item_means(x, y))
    return _REF[key]


def dev_at(a, off=0):
    """A contiguous float32 device copy of a that starts ``off`` floats into a fresh allocation."""
    buf = torch.zeros(off + a.size + 4, dtype=torch.float32, device=DEV)
    view = buf[off:off + a.size].view(a.shape)
    view.copy_(torch.from_numpy(np.array(a)))
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + 4 * off
    return view


def item_count(shape):
    return shape[1] * (shape[2] - 10) * (shape[3] - 10)


def run(irdu, x, y, scale=None):
    """(loss tensor, gradient as float32 numpy, per-item sums) of one forward and reverse."""
    xt = dev_at(x).requires_grad_(True)
    yt = dev_at(y)
    loss = irdu.ssim_loss(xt, yt)
    (loss if scale is None else scale * loss).backward()
    return loss.detach(), xt.grad.cpu().numpy(), irdu.ssim_loss_sums(xt, yt)


def check_gradient(g, g_ref, what):
    top = np.abs(g_ref).max()
    err = np.abs(g.astype(np.float64) - g_ref)
    bound = 2.0 ** -24 * np.abs(g_ref) + 1e-11 * top
    worst = float((err / bound).max())
    print(f"{what}: max|g_ref| {top:.3e}, max err {err.max():.3e}, worst err / bound {worst:.3f}")
    assert np.all(err <= bound), (what, worst)


@pytest.mark.parametrize("kind,shape", CASES, ids=[f"{k}-{'x'.join(map(str, s))}" for k, s in CASES])
def test_forward_and_reverse_against_the_restatement(irdu, kind, shape):
    x, y, loss_ref, g_ref, means = reference(kind, shape)
    loss, g, sums = run(irdu, x, y)
    assert loss.shape == () and loss.dtype == torch.float32 and g.shape == tuple(shape) and len(sums) == shape[0]
    n_item = item_count(shape)
    for b, q in enumerate(sums):
        err = abs(q / (ONE * n_item) - float(means[b]))
        print(f"{kind} {shape} item {b}: mean s {float(means[b]):.12f}, err {err:.3e} of {STEP:.3e}")
        assert err <= STEP
    mean = sum(sums) / (ONE * n_item * shape[0])
    assert abs(mean - (1.0 - loss_ref)) <= STEP
    # the returned loss: 1 - mean in float64, rounded once to float32
    assert float(loss) == float(np.float32(1.0 - mean)), (float(loss), 1.0 - mean)
    if kind == "equal":
        assert sums == [n_item * ONE] * shape[0] and float(loss) == 0.0
        top = float(np.abs(g).max())
        print(f"equal {shape}: max|g| {top:.3e} of {1e-10 / (n_item * shape[0]):.3e}")
        assert top <= 1e-10 / (n_item * shape[0])
    else:
        check_gradient(g, g_ref, f"{kind} {shape}")
    if kind == "out":
        assert min(sums) < n_item * ONE and R.ssim_map(x, y).min() < 0.0 and np.isfinite(g).all()


def test_two_runs_give_the_same_bits(irdu):
    for kind, shape in [("noisy", (2, 3, 43, 75)), ("flat", (1, 3, 24, 24)), ("noisy", edge_shapes()[-1])]:
        x, y = reference(kind, shape)[:2]
        l1, g1, s1 = run(irdu, x, y)
        l2, g2, s2 = run(irdu, x, y)
        assert s1 == s2 and torch.equal(l1, l2)
        assert np.array_equal(g1.view(np.uint32), g2.view(np.uint32))


def test_a_batch_gives_the_sums_of_its_items_alone(irdu):
    for shape in [(2, 3, 43, 75), edge_shapes()[-1]]:
        x, y = reference("noisy", shape)[:2]
        whole = irdu.ssim_loss_sums(dev_at(x), dev_at(y))
        alone = [irdu.ssim_loss_sums(dev_at(x[b:b + 1]), dev_at(y[b:b + 1]))[0] for b in range(shape[0])]
        assert whole == alone and len(set(whole)) == shape[0]


def test_a_scaled_loss_scales_the_gradient_through_the_device_scalar(irdu):
    K = irdu.kernels
    kind, shape = "noisy", (2, 3, 43, 75)
    x, y, _, g_ref, _ = reference(kind, shape)
    g = run(irdu, x, y, scale=0.3)[1]
    w = float(np.float32(0.3))
    check_gradient(g, w * g_ref, "0.3 loss")
    # the same bits as the reverse kernel given gout = 0.3 on the device
    xt, yt = dev_at(x), dev_at(y)
    _, coef = K.ssim_loss_forward(xt, yt, True)
    assert coef.dtype == torch.float64 and tuple(coef.shape) == (3, 2, 3, 33, 65)
    direct = K.ssim_loss_backward(xt, yt, coef, torch.tensor(0.3, dtype=torch.float32, device=DEV))
    assert np.array_equal(direct.cpu().numpy().view(np.uint32), g.view(np.uint32))


def test_no_coefficient_planes_without_a_gradient(irdu, monkeypatch):
    K = irdu.kernels
    seen = []
    real = K.ssim_loss_forward

    def spy(x, y, want_coef):
        qsum, coef = real(x, y, want_coef)
        seen.append((want_coef, coef))
        return qsum, coef
    monkeypatch.setattr(K, "ssim_loss_forward", spy)
    x, y, loss_ref = reference("noisy", (2, 3, 43, 75))[:3]
    xt, yt = dev_at(x), dev_at(y)
    plain = irdu.ssim_loss(xt, yt)                              # requires_grad False
    with torch.no_grad():
        muted = irdu.ssim_loss(xt.clone().requires_grad_(True), yt)
    assert [(w, c) for w, c in seen] == [(False, None), (False, None)]
    assert not plain.requires_grad and not muted.requires_grad and torch.equal(plain, muted)
    wanted = irdu.ssim_loss(xt.clone().requires_grad_(True), yt)
    assert seen[2][0] is True and seen[2][1].dtype == torch.float64 and wanted.requires_grad
    assert torch.equal(wanted.detach(), plain) and abs(float(plain) - loss_ref) <= 2.0 ** -24 + STEP
    assert irdu.SSIMLoss()(xt, yt).item() == plain.item()


def test_operands_one_float_past_a_16_byte_boundary(irdu):
    K = irdu.kernels
    for kind, shape in [("noisy", (2, 3, 43, 75)), ("noisy", edge_shapes()[2])]:
        x, y = reference(kind, shape)[:2]
        gout = torch.ones((), dtype=torch.float32, device=DEV)
        results = []
        for ox, oy in [(0, 0), (1, 1), (1, 3), (2, 0)]:
            xt, yt = dev_at(x, ox), dev_at(y, oy)
            assert (xt.data_ptr() - 4 * ox) % 16 == 0
            qsum, coef = K.ssim_loss_forward(xt, yt, True)
            gx = K.ssim_loss_backward(xt, yt, coef, gout)
            results.append((qsum.tolist(), coef.cpu().numpy(), gx.cpu().numpy()))
        for q, c, g in results[1:]:
            assert q == results[0][0]
            assert np.array_equal(c.view(np.uint64), results[0][1].view(np.uint64))
            assert np.array_equal(g.view(np.uint32), results[0][2].view(np.uint32))


class TinyModel(torch.nn.Module):       # tests/test_training.py's two-layer stand-in
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Conv2d(3, 4, 3, padding=1, bias=False)
        self.b = torch.nn.Conv2d(4, 3, 1, bias=False)

    def forward(self, x):
        return self.b(self.a(x))


def test_trainer_adds_the_weighted_loss_and_steps(irdu):
    from irdu_amd import training as T
    torch.manual_seed(5)
    tr = T.Trainer(TinyModel(), {"ssim_weight": 0.2}, torch.device(DEV))
    _, clean = R.pair("noisy", (2, 3, 32, 32))
    noisy = (clean + np.random.RandomState(9).normal(0.0, 25.0 / 255.0, clean.shape)).astype(np.float32)
    noisy_t, clean_t = torch.from_numpy(noisy).to(DEV), torch.from_numpy(clean).to(DEV)
    outs = []
    got = float(tr.loss(noisy_t, clean_t, outs).detach())
    out = outs[0].detach()
    l1 = float(torch.nn.functional.l1_loss(out, clean_t))
    want = l1 + 0.2 * R.loss(out.cpu().numpy(), clean)
    print(f"trainer: loss {got:.9f}, l1 + 0.2 ref {want:.9f}, err {abs(got - want):.3e} of "
          f"{2.0 ** -24 * abs(want) + 0.2 * STEP:.3e}")
    assert abs(got - want) <= 2.0 ** -24 * abs(want) + 0.2 * STEP
    before = [p.detach().clone() for p in tr.model.parameters()]
    hwc = lambda t: t.permute(0, 2, 3, 1).contiguous()      # noqa: E731
    assert np.isfinite(tr.step(hwc(noisy_t), hwc(clean_t)))
    for p, old in zip(tr.model.parameters(), before):
        assert torch.isfinite(p).all() and not torch.equal(p.detach(), old)
    # weight 0: the same model and batch give the L1 loss alone, and the op is not called
    tr0 = T.Trainer(TinyModel(), {}, torch.device(DEV))
    tr0.model.load_state_dict(tr.model.state_dict())
    assert float(tr0.loss(noisy_t, clean_t)) == float(torch.nn.functional.l1_loss(tr.model(noisy_t), clean_t))
