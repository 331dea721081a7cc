"""The training reverse's operator-term kernels (grr_bwd_term_fused, grr_bwd_term_fused_acc: per-pixel,
register-prefetch row, LDS-ring row, column strips, the one-column tail launch, row segments) and the
edge-weight reverse against float64 autograd through the oracle (tests/term_ref.py), driven through the
solver_grad entry points training uses (glr_term_bwd, gtv_term_bwd, _Level.prox_bwd, edge_weights), across
the dispatch matrix of term_strip_vec / term_ring_shape_ok / launch_term_row (tests/term_ref.TERM_CASES
records the launch of every case).

Bounds (the project's own): element-wise outputs (x-gradient, weight gradient) max-abs error over max-abs
reference <= 2e-5, as test_gpu_subapi_grad.py holds the same operators to; per-graph / per-channel sums
(scale, gamma, taps) error <= 2e-5 max(max|ref|, sqrt(N)), N = B F H W, as test_gpu_term_rows.py holds fp32
sums of O(1) terms to (a missing or doubled column is off by O(H F)).  The prox threshold of every graph
comes from gap_gamma, so no edge lies within 1e-4 gamma of the kink (asserted from the oracle alone in
term_ref.graph_gammas; test_term_ref.py checks every case on the CPU) and no edge is excluded.

Measured on an MI355X, worst over all cases, knob settings and terms, in units of the bound's scale: x-gradient
1.9e-7, weight gradient 3.1e-7, taps 3.7e-7, scale 4.9e-7, gamma 2.1e-7: every path is 40x or more inside
2e-5, and no case needed an explanation from its arithmetic."""
import pytest
import torch

from oracle import graph_oracle as O
from tests import term_ref as R
from tests.test_gpu_parity import DEV, rand

pytestmark = pytest.mark.gpu

ETOL = 2e-5    # element-wise outputs
STOL = 2e-5    # sums, times max(max|ref|, sqrt(N))


@pytest.fixture(scope="module")
def SG():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import irdu_amd
    irdu_amd.load_native()
    from irdu_amd import kernels as K
    from irdu_amd import solver_grad
    try:
        yield solver_grad
    finally:
        K.set_term_rows(2)
        K.set_term_tail(True)
        K.set_term_acc_max_w(128)


def _set_knobs(K, rows=2, tail=1, cap=128):
    K.set_term_rows(rows)
    K.set_term_tail(bool(tail))
    K.set_term_acc_max_w(cap)


def _run_hip(SG, mode, d, G):
    """The term reverse through its solver_grad entry point on pre-filled accumulators; returns what it
    added to each (float64, CPU)."""
    from irdu_amd import kernels as K
    dev = lambda t: t.to(DEV).contiguous()   # noqa: E731
    x, g, taps, w, scale = (dev(d[k]) for k in ("x", "g", "taps", "w", "scale"))
    out, gtaps, gscale, gw = (dev(d[k]) for k in ("pre_out", "pre_gtaps", "pre_gscale", "pre_gw"))
    pre = dict(out=d["pre_out"], gw=d["pre_gw"], gtaps=d["pre_gtaps"], gscale=d["pre_gscale"])
    got = {}
    if mode == R.TERM_GLR:
        SG.glr_term_bwd(x, g, taps, w, scale, R.COEF, G, out, gw, gscale, gtaps)
    elif mode == R.TERM_PAIR:
        # the pair term takes the 2-plane pair weights; its weight gradient returns to the 4 raw planes
        # through bwd_pair_weights (as _mixture_bwd does).  gc is pre-filled too; what the term added to it
        # is what goes on (the fp32 subtraction rounds at 6e-8 of |pre| + |gc|, far below the bound)
        c = K.gtv_pair_weights(w)
        gc = dev(d["pre_gc"])
        SG.gtv_term_bwd(x, g, taps, c, scale, R.COEF, G, out, gc, gscale, gtaps)
        K.bwd_pair_weights(w, gc - dev(d["pre_gc"]), gw)
    else:
        lg = dev(d["log_gamma"])
        st = tuple(taps[:, 0].contiguous() for _ in range(4))
        lvl = SG._Level(w, K.gtv_pair_weights(w), w, st, st, lg, dev(d["log_scale"]), lg, G)
        lvl.tapsG = taps
        lvl.gwG, lvl.gro, lvl.ggam, lvl.gtapG = gw, gscale, dev(d["pre_ggam"]), gtaps
        lvl.prox_bwd(x, g, out)
        pre["ggam"] = d["pre_ggam"]
        got["ggam"] = lvl.ggam
    torch.cuda.synchronize()
    got.update(out=out, gw=gw, gtaps=gtaps, gscale=gscale)
    return {k: v.cpu().double() - pre[k].double() for k, v in got.items()}


PARAMS = [pytest.param(c[:5], kn, id="b{}g{}f{}h{}w{}-{}".format(*c[:5], kn)) for c in R.TERM_CASES for kn in c[5]]


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["glr", "pair", "prox"])
@pytest.mark.parametrize("case,knob", PARAMS)
def test_term_reverse_matches_oracle(SG, case, knob, mode):
    from irdu_amd import kernels as K
    b, G, F, h, wd = case
    assert knob != "rows0" or F <= 4
    d, ref = R.term_case(case, mode)          # computed once per (case, mode), shared by the knob settings
    _set_knobs(K, **R.KNOBS[knob])
    try:
        got = _run_hip(SG, mode, d, G)
    finally:
        _set_knobs(K)
    n = b * F * h * wd
    errs = {}
    for name, r in ref.items():
        a = got[name]
        assert torch.isfinite(a).all(), name
        err = float((a - r).abs().max())
        rmax = float(r.abs().max())
        assert rmax > 0.0, name
        if name in ("out", "gw"):
            errs[name] = (err / rmax, ETOL)
        else:
            errs[name] = (err / max(rmax, n ** 0.5), STOL)
    print("\n" + " ".join(f"{k}={e:.2e}" for k, (e, _) in errs.items()))
    bad = {k: e for k, (e, tol) in errs.items() if e > tol}
    assert not bad, bad


# (b, G, F, H, W): column strips of the edge-weight reverse's row kernel (four-column lanes, 248 owned
# columns: 512 -> 3 strips, 300 -> 2, 744 -> 3 whole, 264 -> 2 with a last strip of 16); F = 12 has no row
# instance (per-pixel at both settings); W = 100, H = 33: two-column lanes, one strip, two row segments
EDGE_CASES = [(1, 2, 6, 7, 512), (2, 1, 3, 5, 300), (1, 2, 4, 6, 744), (1, 2, 12, 9, 264), (1, 3, 1, 33, 100)]


@pytest.fixture(scope="module")
def edge_refs():
    return {}


def _edge_case(case):
    b, G, F, h, wd = case
    f5 = rand(b, G, F, h, wd, seed=11 * F + h)
    f5[:, 0, :, :2, :3] = 0.0                          # some zero-norm pixels (the 1e-12 floor)
    multiM = torch.rand(G, F, generator=torch.Generator().manual_seed(F + wd)) + 0.5
    gw = rand(b, G, 4, h, wd, seed=5)
    gdeg = rand(b, G, h, wd, seed=6)
    fr, mr = f5.double().requires_grad_(True), multiM.double().requires_grad_(True)
    # keep the oracle's unit vectors n = f / |f|: their gradient gn is the un-projected feature gradient
    units, normalize = [], O.Fn.normalize

    def keep(*a, **k):
        units.append(normalize(*a, **k))
        units[-1].retain_grad()
        return units[-1]
    O.Fn.normalize = keep
    try:
        w, deg = O.edge_weights(fr, mr)
    finally:
        O.Fn.normalize = normalize
    ((w * gw.double()).sum() + (deg * gdeg.double()).sum()).backward()
    norm = f5.double().norm(dim=2, keepdim=True)
    unproj = float((units[0].grad.abs() / norm.clamp_min(1e-12))[(norm > 0).expand_as(f5)].max())
    return f5, multiM, gw, gdeg, w.detach(), fr.grad, mr.grad, unproj


@pytest.mark.parametrize("rows", [0, 2])
@pytest.mark.parametrize("case", EDGE_CASES, ids=lambda c: "b{}g{}f{}h{}w{}".format(*c))
def test_edge_weights_reverse_matches_oracle(SG, edge_refs, case, rows):
    """SG.edge_weights (grr_bwd_edge_weights: row kernel in strips / per-pixel) against float64 autograd of
    O.edge_weights, a random cotangent on both outputs; 2e-5 on both gradients as the sub-API tests."""
    from irdu_amd import kernels as K
    if case not in edge_refs:
        edge_refs[case] = _edge_case(case)
    f5, multiM, gw, gdeg, w_ref, gf_ref, gm_ref, unproj = edge_refs[case]
    F = case[2]

    class Mod:
        pass
    mod = Mod()
    mod.multiM = multiM.to(DEV).requires_grad_(True)
    f = f5.to(DEV).requires_grad_(True)
    K.set_term_rows(rows)
    try:
        w, deg = SG.edge_weights(mod, f)
        ((w * gw.to(DEV)).sum() + (deg * gdeg.to(DEV)).sum()).backward()
        torch.cuda.synchronize()
    finally:
        K.set_term_rows(2)
    rel = lambda a, r, scale=None: float((a.cpu().double().reshape(r.shape) - r).abs().max() /   # noqa: E731
                                         (r.abs().max() if scale is None else scale))
    # a zero-norm pixel's feature gradient is gn / 1e-12: held to the bound on its own, so that its size
    # does not become the scale every other pixel is measured against
    zero = (f5.abs().sum(dim=2, keepdim=True) == 0).expand_as(f5)
    assert zero.any() and not zero.all()
    gf = f.grad.cpu().double()
    # F = 1: the feature gradient (gn - n (n . gn)) / |f| is identically zero off the zero-norm pixels (n = +-1;
    # the float64 reference is 0 to ~1e-13), so max|ref| is no scale.  fp32 leaves the cancellation's
    # rounding, eps |gn| / |f|: the error is held to 2e-5 of the un-projected max |gn| / |f| from the oracle
    scale = unproj if F == 1 else None
    assert F > 1 or float(gf_ref[~zero].abs().max()) < 1e-9 * unproj
    e = dict(w=rel(w.detach(), w_ref), gfeat=rel(gf[~zero], gf_ref[~zero], scale),
             gfeat_zero=rel(gf[zero], gf_ref[zero]), gM=rel(mod.multiM.grad, gm_ref))
    print("\n" + " ".join(f"{k}={v:.2e}" for k, v in e.items()))
    assert float(gf_ref[zero].abs().max()) > 1e6 * float(gf_ref[~zero].abs().max())
    assert e["w"] <= 1e-5
    assert e["gfeat"] <= 2e-5 and e["gfeat_zero"] <= 2e-5 and e["gM"] <= 2e-5, e
