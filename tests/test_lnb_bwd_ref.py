"""CPU checks of tests/lnb_bwd_ref.py, from the references alone (no kernel): every case meets the conditions
tests/test_gpu_lnb_bwd_kernels.py relies on -- finite references, a non-zero scale for every compared tensor,
an ill-conditioned case that is ill-conditioned, an extreme-gate case that is extreme -- and the closed-form
norm reverse in the header of csrc/lnb_bwd.hip is the derivative (float64 autograd, 1e-12)."""
import pytest
import torch

from tests import lnb_bwd_ref as R

NORM_CASES = [(s, False) for s in R.NORM_SHAPES + [R.NORM_LIMIT]] + [(R.NORM_ILL, True)]
GATE_CASES = [(s, False) for s in R.GATE_SHAPES] + [(R.GATE_EXTREME, True)]
FUSED_CASES = [(s, ffn, False) for s in R.HP_SHAPES for ffn in (False, True)] + \
              [(R.GATE_EXTREME, ffn, True) for ffn in (False, True)]


def _usable(ref):
    for name, t in vars(ref).items():
        if not torch.is_tensor(t):
            continue
        assert bool(torch.isfinite(t).all()), name
        assert float(t.abs().max()) > 0.0, name


@pytest.mark.parametrize("shape,ill", NORM_CASES, ids=str)
def test_norm_references_are_usable(shape, ill):
    _usable(R.norm_ref(shape, ill))
    d = R.norm_inputs(shape, ill)
    b, c, h, w = shape
    assert d.x.shape == shape and d.x.dtype == torch.float32 and d.ln_w.shape == (c,)


@pytest.mark.parametrize("shape,extreme", GATE_CASES, ids=str)
def test_gate_references_are_usable(shape, extreme):
    _usable(R.gate_ref(shape, extreme))


@pytest.mark.parametrize("shape,ffn,extreme", FUSED_CASES, ids=str)
def test_fused_gate_references_are_usable(shape, ffn, extreme):
    ref = R.fused_ref(shape, ffn, extreme)
    _usable(ref)
    assert ref.gabs > 0.0
    if extreme:   # centre-only taps: the depthwise output is hh itself under either padding
        d = R.fused_inputs(shape, True)
        assert torch.equal(R.dw3_ref(d.hh, d.wdw), d.hh)
        c2 = d.hh.shape[1]
        assert torch.equal(torch.nn.functional.conv2d(d.hh, d.wdw.view(c2, 1, 3, 3), padding=1, groups=c2), d.hh)


@pytest.mark.parametrize("shape", [(1, 3, 9, 100), (1, 2, 7, 200)], ids=str)
def test_dw3_references_are_usable(shape):
    _usable(R.dw3_case_ref(shape))


def test_case_lists_reach_what_they_name():
    bc = [s[0] * s[1] for s in R.NORM_SHAPES]
    assert max(bc) == 65535 and R.NORM_LIMIT[0] * R.NORM_LIMIT[1] == 65536
    assert any(s[1] == 2 for s in R.NORM_SHAPES) and any(s[1] % 8 for s in R.NORM_SHAPES)
    assert any(s[2] * s[3] == 1 for s in R.NORM_SHAPES)
    # more than one reduction chunk per plane with B > 1 (chunks_for of lnb_bwd.hip)
    chunks = lambda s: max(1, min(-(-4096 // (s[0] * s[1])), -(-s[2] * s[3] // 256)))   # noqa: E731
    assert any(chunks(s) > 1 and s[0] > 1 for s in R.NORM_SHAPES)
    # past the 4096 blocks x 256 threads of gate_bwd_scaled_kernel: its grid-stride loop takes a second turn
    assert max(s[0] * s[1] * s[2] * s[3] for s in R.GATE_SHAPES) > 4096 * 256


def test_ill_conditioned_case_is_ill_conditioned():
    x = R.norm_inputs(R.NORM_ILL, True).x.double()
    ratio = x.mean(dim=1).abs() / x.std(dim=1)
    assert float(ratio.min()) >= 100.0, float(ratio.min())
    # and the benign cases are not
    x = R.norm_inputs(R.NORM_SHAPES[3]).x.double()
    assert float((x.mean(dim=1).abs() / x.std(dim=1)).median()) < 1.0


def test_extreme_gate_case_is_extreme():
    d = R.gate_inputs(R.GATE_EXTREME, True)
    hid = R.GATE_EXTREME[1]
    m = d.hp[:, :hid]
    assert float(m.min()) < -88.0 and float(m.max()) > 88.0
    assert sorted(set(m.flatten().tolist())) == sorted(torch.tensor(R.EXTREME_M).tolist())
    # what fp32 does there: expf(-m) overflows, the sigmoid is 0 and the gate -0, not NaN
    e = torch.exp(-m)
    assert bool(torch.isinf(e).any())
    sg = 1.0 / (1.0 + e)
    assert bool(torch.isfinite(sg * m * d.hp[:, hid:]).all())
    assert torch.equal(R.fused_inputs(R.GATE_EXTREME, True).hh, d.hp)


@pytest.mark.parametrize("shape,ill", NORM_CASES, ids=str)
def test_closed_form_norm_reverse_is_the_derivative(shape, ill):
    d, ref = R.norm_inputs(shape, ill), R.norm_ref(shape, ill)
    x, lw, gn, gout = d.x.double(), d.ln_w.double(), d.gn.double(), d.gout.double()
    n, isd = R.norm_forward_formula(x, lw)
    rel = lambda a, r: float((a - r).abs().max() / r.abs().max())   # noqa: E731
    assert rel(n, ref.n) <= 1e-12 and rel(isd, ref.isd) <= 1e-12
    gx, glw, _ = R.norm_reverse_formula(x, lw, ref.isd, gn)
    tol = 1e-12
    assert rel(gx, ref.gx) <= tol and rel(glw, ref.gln_w) <= 1e-12
    gxs, glw, gs = R.norm_reverse_formula(x, lw, ref.isd, gn, gout, R.SKIP[0])
    assert rel(gxs, ref.gx_skip) <= tol and rel(glw, ref.gln_w) <= 1e-12 and rel(gs, ref.gskip0) <= 1e-12


def test_measures():
    r = torch.tensor([0.0, 2.0, -4.0])
    assert R.elem_err(torch.tensor([0.0, 2.0, -4.0 + 4e-6]).float(), r) == pytest.approx(1e-6, rel=0.1)
    assert R.sum_err(torch.tensor([3.0]), torch.tensor([2.0]), 100) == pytest.approx(0.1)
