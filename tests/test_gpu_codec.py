"""The v1.0 model's encoder / decoder convolutions on libgrr (csrc/codec_ops.hip, grr_conv1x1_cat2) against
float64 references, their bitwise guarantees, and the model with the NATIVE_CONVS switch on: golden parity,
enc_dec against float64 autograd through the oracle, patch independence, run-to-run equality, the op census (no
library convolution or GEMM in a training step) and model.compile().
"""
import pytest
import torch
import torch.nn.functional as F
from torch.utils._python_dispatch import TorchDispatchMode

from oracle import graph_oracle as O
from tests.golden_io import load_golden, params_of
from tests.test_gpu_parity import DEV, assert_close, rand, rel_err

pytestmark = pytest.mark.gpu

GRAD_TOL = 2e-4     # the project's gradient tolerance (relative to max |ref|)


@pytest.fixture(scope="module")
def irdu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import irdu_amd
    irdu_amd.load_native()
    return irdu_amd


@pytest.fixture
def native_on(irdu):
    from irdu_amd import graph_filter as GF
    old = GF.NATIVE_CONVS
    irdu.native_convs(True)
    yield
    irdu.native_convs(old)


def fp32_class(got, ref64, ref32):
    """The project's fp32-class bound (test_x3_gemm_is_fp32_accurate): the error against float64 is at most
    four times that of the CPU's own fp32 evaluation, plus 1e-7."""
    err32 = rel_err(ref32, ref64)
    err = rel_err(got, ref64)
    print(f"err {err:.3e}  err32 {err32:.3e}")
    assert err <= 4 * err32 + 1e-7, (err, err32)


def embed_ref(x, w):
    return F.conv2d(F.pad(x, (1, 1, 1, 1), mode="replicate"), w)


# ---- 3x3 embedding -----------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 3, 48, 16, 20), (1, 1, 48, 1, 1), (1, 3, 48, 1, 70), (1, 3, 48, 5, 1),
                                   (1, 4, 64, 3, 257), (2, 3, 128, 9, 130), (1, 3, 5, 8, 8)])
def test_embed_forward(irdu, shape):
    b, cin, m, h, w = shape
    x = rand(b, cin, h, w, seed=41, scale=2.0, offset=0.3)
    wt = rand(m, cin, 3, 3, seed=42) * 0.3
    K = irdu.kernels
    xd, wd = x.to(DEV), wt.to(DEV)
    got = K.conv3x3_embed(xd, wd)
    fp32_class(got, embed_ref(x.double(), wt.double()), embed_ref(x, wt))
    assert torch.equal(K.conv3x3_embed(xd, wd), got)                  # run to run
    for i in range(b):                                                # a patch does not see its batch
        assert torch.equal(K.conv3x3_embed(xd[i:i + 1].contiguous(), wd)[0], got[i])


@pytest.mark.parametrize("shape", [(2, 3, 48, 6, 10), (1, 3, 48, 1, 1), (1, 4, 16, 3, 70)])
def test_embed_reverse(irdu, shape):
    b, cin, m, h, w = shape
    from irdu_amd import solver_grad as SG
    x = rand(b, cin, h, w, seed=43, scale=2.0, offset=0.3)
    wt = rand(m, cin, 3, 3, seed=44) * 0.3
    lw = rand(b, m, h, w, seed=45)
    x64, w64 = x.double().requires_grad_(), wt.double().requires_grad_()
    (embed_ref(x64, w64) * lw.double()).sum().backward()

    def run():
        xd, wd = x.to(DEV).requires_grad_(), wt.to(DEV).requires_grad_()
        (SG.Conv3x3EmbedFn.apply(xd, wd) * lw.to(DEV)).sum().backward()
        return xd.grad, wd.grad

    gx, gw = run()
    ex, ew = rel_err(gx, x64.grad), rel_err(gw, w64.grad)
    print(f"gx {ex:.3e}  gw {ew:.3e}")
    assert ex <= GRAD_TOL and ew <= GRAD_TOL, (ex, ew)
    gx2, gw2 = run()
    assert torch.equal(gw2, gw) and torch.equal(gx2, gx)
    # needs_input_grad: an image without a gradient gets none (and the data-gradient kernel does not run)
    xd, wd = x.to(DEV), wt.to(DEV).requires_grad_()
    (SG.Conv3x3EmbedFn.apply(xd, wd) * lw.to(DEV)).sum().backward()
    assert xd.grad is None and torch.equal(wd.grad, gw)


# ---- transposed 2x2 / stride 2 -----------------------------------------------------------------
CONVT_SHAPES = [(2, 96, 48, 8, 10), (1, 384, 192, 4, 4), (1, 8, 5, 1, 1), (1, 64, 48, 3, 129), (1, 130, 96, 2, 6)]


@pytest.mark.parametrize("shape", CONVT_SHAPES)
def test_convt2x2s2_forward(irdu, shape):
    b, k, m, h, w = shape
    x = rand(b, k, h, w, seed=51, scale=2.0, offset=0.3)
    wt = rand(k, m, 2, 2, seed=52) * 0.2
    K = irdu.kernels
    xd, wd = x.to(DEV), wt.to(DEV)
    got = K.convt2x2s2(xd, wd)
    assert got.shape == (b, m, 2 * h, 2 * w)
    fp32_class(got, F.conv_transpose2d(x.double(), wt.double(), stride=2), F.conv_transpose2d(x, wt, stride=2))
    assert torch.equal(K.convt2x2s2(xd, wd), got)
    for i in range(b):
        assert torch.equal(K.convt2x2s2(xd[i:i + 1].contiguous(), wd)[0], got[i])


@pytest.mark.parametrize("shape", [CONVT_SHAPES[0], CONVT_SHAPES[2]])
def test_convt2x2s2_reverse(irdu, shape):
    b, k, m, h, w = shape
    from irdu_amd import solver_grad as SG
    x = rand(b, k, h, w, seed=53, scale=2.0, offset=0.3)
    wt = rand(k, m, 2, 2, seed=54) * 0.2
    lw = rand(b, m, 2 * h, 2 * w, seed=55)
    x64, w64 = x.double().requires_grad_(), wt.double().requires_grad_()
    (F.conv_transpose2d(x64, w64, stride=2) * lw.double()).sum().backward()
    xd, wd = x.to(DEV).requires_grad_(), wt.to(DEV).requires_grad_()
    (SG.ConvT2x2s2Fn.apply(xd, wd) * lw.to(DEV)).sum().backward()
    ex, ew = rel_err(xd.grad, x64.grad), rel_err(wd.grad, w64.grad)
    print(f"gx {ex:.3e}  gw {ew:.3e}")
    assert ex <= GRAD_TOL and ew <= GRAD_TOL, (ex, ew)


# ---- concat-free combine -----------------------------------------------------------------------
@pytest.mark.parametrize("kkm", [(48, 48, 48), (96, 96, 96), (192, 192, 192)])
def test_conv1x1_cat2_is_bitwise_the_concatenated_conv(irdu, kkm):
    ka, kb, m = kkm
    K = irdu.kernels
    assert K.conv1x1_cat2_ok(ka, kb, m, 9 * 37)
    a = rand(2, ka, 9, 37, seed=61, scale=2.0, offset=0.3).to(DEV)
    b = rand(2, kb, 9, 37, seed=62, scale=2.0, offset=-0.2).to(DEV)
    wt = (rand(m, ka + kb, 1, 1, seed=63) * 0.2).to(DEV)
    got = K.conv1x1_cat2(a, b, wt)
    assert torch.equal(got, K.conv1x1(torch.cat([a, b], 1), wt))
    assert_close(got, F.conv2d(torch.cat([a, b], 1).double().cpu(), wt.double().cpu()), rtol=1e-5)


def test_conv1x1_cat2_fallback_shape(irdu):
    K = irdu.kernels
    ka, kb, m = 40, 24, 16
    assert not K.conv1x1_cat2_ok(ka, kb, m, 7 * 11)
    a, b = rand(2, ka, 7, 11, seed=64).to(DEV), rand(2, kb, 7, 11, seed=65).to(DEV)
    wt = (rand(m, ka + kb, 1, 1, seed=66) * 0.2).to(DEV)
    assert_close(K.conv1x1_cat2(a, b, wt), F.conv2d(torch.cat([a, b], 1).double().cpu(), wt.double().cpu()), rtol=1e-5)


def test_conv1x1_cat2_reverse(irdu):
    from irdu_amd import solver_grad as SG
    ka, kb, m = 48, 48, 48
    a, b = rand(2, ka, 6, 10, seed=67, scale=2.0), rand(2, kb, 6, 10, seed=68, scale=2.0)
    wt = rand(m, ka + kb, 1, 1, seed=69) * 0.2
    lw = rand(2, m, 6, 10, seed=70)
    a64, b64, w64 = (t.double().requires_grad_() for t in (a, b, wt))
    (F.conv2d(torch.cat([a64, b64], 1), w64) * lw.double()).sum().backward()
    ad, bd, wd = (t.to(DEV).requires_grad_() for t in (a, b, wt))
    (SG.Conv1x1Cat2Fn.apply(ad, bd, wd) * lw.to(DEV)).sum().backward()
    errs = [rel_err(ad.grad, a64.grad), rel_err(bd.grad, b64.grad), rel_err(wd.grad, w64.grad)]
    print("ga %.3e  gb %.3e  gw %.3e" % tuple(errs))
    assert max(errs) <= GRAD_TOL, errs


# ---- the model with the switch on ----------------------------------------------------------------
def _golden_model(irdu):
    d = load_golden("abstract_v1.npz")
    cfg = {k[5:]: d[k] for k in d.files if k.startswith("meta/") and k != "meta/n_state_keys"}
    m = irdu.AbtractMultiScaleGraphFilter(
        n_channels_in=3, n_channels_out=3, dims=cfg["dims"].tolist(), hidden_dims=cfg["hidden_dims"].tolist(),
        nsubnets=cfg["nsubnets"].tolist(), ngraphs=cfg["ngraphs"].tolist(), num_blocks=cfg["num_blocks"].tolist(),
        num_blocks_out=int(cfg["num_blocks_out"]))
    m.load_state_dict(params_of(d, ""))
    return m.to(DEV), d, cfg


def test_model_golden_native(irdu, native_on):
    m, d, _ = _golden_model(irdu)
    img = torch.from_numpy(d["in/noisy"]).to(DEV)
    with torch.no_grad():
        filt = m.filtering(m.encode(img))
        y = m(img)
    for i in range(4):
        assert_close(filt[i], d[f"out/filtered{i}"])
    assert_close(y, d["out/y"])


def test_enc_dec_and_gradients_vs_float64_oracle(irdu, native_on):
    m, d, cfg = _golden_model(irdu)
    m.train()
    nb, nbo, ns = cfg["num_blocks"].tolist(), int(cfg["num_blocks_out"]), cfg["nsubnets"].tolist()
    img = torch.from_numpy(d["in/noisy"])
    p64 = {k: v.detach().cpu().double().requires_grad_() for k, v in m.state_dict().items()}
    ref = O.abstract_decode(O.abstract_encode(img.double(), p64, nb, ns), p64, nb, nbo, ns)
    lw = rand(*ref.shape, seed=71)
    (ref * lw.double()).sum().backward()
    out = m.enc_dec(img.to(DEV))
    (out * lw.to(DEV)).sum().backward()
    e = rel_err(out, ref.detach())
    print(f"enc_dec output err {e:.3e}")
    assert e <= 1e-5, e
    touched = 0
    for k, p in m.named_parameters():
        if p64[k].grad is None:
            assert p.grad is None, k                     # the filter blocks are not on this path
            continue
        touched += 1
        eg = rel_err(p.grad, p64[k].grad)
        assert eg <= GRAD_TOL, (k, eg)
    assert touched > 20


def _grads(m, x, lw):
    m.zero_grad(set_to_none=True)
    (m(x) * lw).sum().backward()
    return {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}


def test_model_is_patch_independent_and_reproducible(irdu, native_on):
    """With every convolution on libgrr the whole model keeps the kernels' guarantees: a patch's output does
    not depend on its batch, and two identical training steps give bitwise equal gradients."""
    m, d, _ = _golden_model(irdu)
    x = torch.rand(4, 3, 32, 32, generator=torch.Generator().manual_seed(72)).to(DEV)
    m.eval()
    with torch.no_grad():
        y = m(x)
        for i in range(4):
            assert torch.equal(m(x[i:i + 1])[0], y[i]), i
    m.train()
    lw = rand(4, 3, 32, 32, seed=73).to(DEV)
    g1, g2 = _grads(m, x, lw), _grads(m, x, lw)
    assert g1.keys() == g2.keys() and len(g1) == len(list(m.parameters()))
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k


class _Census(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.seen = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.seen.append(func)
        return func(*args, **(kwargs or {}))


def _census(m, x):
    m.zero_grad(set_to_none=True)
    with _Census() as c:
        m(x).square().mean().backward()
    return c.seen


def test_op_census_training_step_has_no_library_conv_or_gemm(irdu, native_on):
    from irdu_amd import stream_guard
    m, d, _ = _golden_model(irdu)
    m.train()
    x = torch.from_numpy(d["in/noisy"]).to(DEV)
    seen = _census(m, x)
    assert len(seen) > 50
    bad = sorted({str(f) for f in seen if not stream_guard.allowed(f)})
    assert not bad, bad
    names = {f._schema.name for f in seen}
    for n in ("aten::convolution", "aten::convolution_backward", "aten::mm", "aten::addmm", "aten::bmm"):
        assert n not in names, n
    # the census is able to see one: the same step with the switch off runs the stock convolutions
    irdu.native_convs(False)
    names_off = {f._schema.name for f in _census(m, x)}
    assert "aten::convolution" in names_off and "aten::convolution_backward" in names_off


def test_find_db_warning_stays_silent_when_covered(irdu, native_on, monkeypatch):
    """No MIOpen call is left with the switch on, so the training-mode forward does not ask for
    miopen_training_defaults(); with the switch off the model is not covered and the warning path is taken."""
    import warnings
    from irdu_amd import graph_filter as GF
    m, d, _ = _golden_model(irdu)
    m.train()
    x = torch.from_numpy(d["in/noisy"]).to(DEV)
    monkeypatch.delenv("MIOPEN_DEBUG_DISABLE_FIND_DB", raising=False)
    monkeypatch.setattr(GF, "_MIOPEN_CHECKED", False)
    assert m._native_covered(x)
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message="irdu_amd: training AbtractMultiScaleGraphFilter")
        m(x)
    assert GF._MIOPEN_CHECKED is False          # the check was never reached
    irdu.native_convs(False)
    assert not m._native_covered(x)


def test_compiled_model_equals_eager_native(irdu, native_on):
    import torch._inductor.metrics as metrics
    torch._dynamo.reset()
    m, d, _ = _golden_model(irdu)
    m.eval()
    x = torch.from_numpy(d["in/noisy"]).to(DEV)
    with torch.no_grad():
        ref = m(x)
        metrics.reset()
        m.compile()
        got = m(x)
    assert metrics.generated_kernel_count == 0, metrics.generated_kernel_count
    assert torch.equal(got, ref)
    torch._dynamo.reset()
