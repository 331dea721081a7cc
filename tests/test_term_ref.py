"""CPU checks of the reference helpers the oracle tests of the term reverses stand on (tests/term_ref.py):
term_reference against central finite differences in float64, gap_gamma's rule, and the gap condition
(half-gap >= 1e-4 gamma, both soft-threshold branches >= 1 % of the edges, for every graph) for every prox
case the GPU tests use, with the same seeds."""
import pytest
import torch

from tests import term_ref as R


def test_gap_gamma_picks_the_widest_gap_in_the_window():
    v = torch.arange(100, dtype=torch.float64)
    v[80:] += 5.0                      # the widest gap (79 -> 85) inside [0.7, 0.98]
    v[10:] += 50.0                     # a wider one outside the window
    gm, half = R.gap_gamma(v[torch.randperm(100, generator=torch.Generator().manual_seed(0))])
    assert gm == pytest.approx(50.0 + 79.0 + 3.0) and half == pytest.approx(3.0)
    half2, below, above = R.gap_condition(v, gm)
    assert half2 == pytest.approx(3.0) and below == pytest.approx(0.8) and above == pytest.approx(0.2)
    with pytest.raises(AssertionError):
        R.assert_gap(v, 84.99995 + 50.0)        # an edge within 1e-4 gamma of the threshold
    with pytest.raises(AssertionError):
        R.assert_gap(v, 154.5)                  # no edge above: a branch below 1 % of the edges


def test_taps_kernel_matches_stencil_taps_order():
    from irdu_amd import kernels as K
    from oracle import graph_oracle as O
    g = torch.Generator().manual_seed(3)
    ps = [torch.randn(6, 1, 1, 1, generator=g, dtype=torch.float64) for _ in range(4)]
    p = dict(zip(("stats_kernel_p01", "stats_kernel_p02a", "stats_kernel_p02b", "stats_kernel_p03"), ps))
    assert torch.allclose(R.taps_kernel(K.stencil_taps(*ps)), O.stats_kernel(p, ""), rtol=0, atol=1e-15)


TINY = (1, 2, 2, 3, 4)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_term_reference_matches_finite_differences(mode):
    """Every component of every gradient term_reference returns, against central differences of Phi in
    float64 (step 1e-6; gamma from gap_gamma, so no edge crosses the kink within the step)."""
    d = R.term_inputs(TINY, mode)
    G = TINY[1]
    lg = d["log_gamma"]
    ref = R.term_reference(mode, d["x"], d["g"], d["taps"], d["w"], lg, d["scale"], R.COEF, G)
    args = dict(x=d["x"].double(), taps=d["taps"].double(), w=d["w"].double(), scale=d["scale"].double())
    if mode == 2:
        args["gamma"] = torch.exp(lg.double())
        assert float(d["half_gap"].min()) > 1e-4    # far wider than the step's effect on |t|

    def phi(a):
        return float(R.term_phi(mode, a["x"], d["g"].double(), a["taps"], a["w"], a.get("gamma"), a["scale"],
                                R.COEF, G))
    eps = 1e-6
    for name, key in (("x", "out"), ("w", "gw"), ("taps", "gtaps"), ("scale", "gscale"), ("gamma", "ggam")):
        if name not in args:
            continue
        fd = torch.zeros_like(args[name]).reshape(-1)
        for i in range(fd.numel()):
            vals = []
            for sgn in (1.0, -1.0):
                a = dict(args)
                t = args[name].clone().reshape(-1)
                t[i] += sgn * eps
                a[name] = t.reshape(args[name].shape)
                vals.append(phi(a))
            fd[i] = (vals[0] - vals[1]) / (2 * eps)
        err = float((fd.reshape(ref[key].shape) - ref[key]).abs().max())
        assert float(ref[key].abs().max()) > 1e-3, name
        assert err <= 1e-7 * max(1.0, float(ref[key].abs().max())), (name, err)


@pytest.mark.parametrize("case", [c[:5] for c in R.TERM_CASES], ids=lambda c: "b{}g{}f{}h{}w{}".format(*c))
def test_gap_condition_term_cases(case):
    """The prox inputs of test_gpu_term_oracle.py: graph_gammas asserts the condition for every graph."""
    d = R.term_inputs(case, R.TERM_PROX, R.PROX_SEED_BUMP.get(case, 0))
    gam = torch.exp(d["log_gamma"].double())
    assert (d["half_gap"] >= R.MIN_HALF_GAP * gam).all()
    assert len(set(d["scale"].tolist())) == case[1] and bool(((d["scale"] >= 0.5) & (d["scale"] < 1.5)).all())


@pytest.mark.parametrize("case", R.WIDE_LOWPASS, ids=lambda c: "g{g}f{f}h{h}w{w}".format(**c))
def test_gap_condition_wide_lowpass(case):
    """test_gpu_grad.py::test_lowpass_block_grad_wide: both levels, every graph (asserted in set_gap_gammas)."""
    import irdu_amd
    blk, _, _, ratio = R.wide_lowpass(irdu_amd, case)
    print(f"\nsmallest half-gap / max|t| = {ratio:.3e}, gammas {blk.local_filter.gamma00.exp().flatten().tolist()}")
    assert ratio > 0.0


def test_gap_condition_wide_msgf():
    import irdu_amd
    _, _, _, ratio = R.wide_msgf(irdu_amd)
    print(f"\nsmallest half-gap / max|t| = {ratio:.3e}")
    assert ratio > 0.0
