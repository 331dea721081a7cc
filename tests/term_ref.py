"""float64 reference of the three operator-term reverses (GLR, pair Laplacian, prox) by autograd through the
oracle, the rule that picks a prox threshold away from every edge (gap_gamma), and the inputs and case
tables the GPU tests (test_gpu_term_oracle.py, test_gpu_grad.py) share with their CPU checks
(test_term_ref.py).  Nothing here needs a GPU."""
import functools
import math

import torch

from oracle import graph_oracle as O

TERM_GLR, TERM_PAIR, TERM_PROX = 0, 1, 2

# ---------------------------------------------------------------------------
# The prox threshold.  phi'(t) jumps at |t| = gamma, so an edge whose |t| lies within fp32 rounding of gamma
# may take the other branch on the GPU, which moves the input gradient at that pixel by O(1).  The prox
# input does not depend on gamma, so gamma is put in the middle of the widest gap of the oracle's own
# sorted |t|.  The tests then assert (from the oracle alone) that the gap is wide against fp32 rounding
# and that both branches are populated; no edge is excluded from any comparison.
Q_LO, Q_HI = 0.7, 0.98
MIN_HALF_GAP = 1e-4     # half-gap >= MIN_HALF_GAP * gamma
MIN_BRANCH = 0.01       # each soft-threshold branch holds >= 1 % of the edges


def gap_gamma(abs_t, q_lo=Q_LO, q_hi=Q_HI):
    """(gamma, half_gap): the midpoint of the widest gap between consecutive sorted values of |t| (one
    graph's edges) inside the quantile window [q_lo, q_hi], and half that gap's width."""
    v = torch.sort(abs_t.detach().double().reshape(-1)).values
    n = v.numel()
    lo = int(math.floor(q_lo * (n - 1)))
    hi = max(int(math.ceil(q_hi * (n - 1))), lo + 1)
    if hi > n - 1:
        raise ValueError(f"gap_gamma: {n} values leave no gap inside [{q_lo}, {q_hi}]")
    d = v[lo + 1:hi + 1] - v[lo:hi]
    i = int(torch.argmax(d))
    return float(v[lo + i] + 0.5 * d[i]), float(0.5 * d[i])


def gap_condition(abs_t, gamma):
    """(half_gap, fraction below, fraction above) of one graph's |t| around gamma."""
    a = abs_t.detach().double().reshape(-1)
    return float((a - gamma).abs().min()), float((a < gamma).double().mean()), float((a > gamma).double().mean())


def assert_gap(abs_t, gamma, what=""):
    half, below, above = gap_condition(abs_t, gamma)
    assert half >= MIN_HALF_GAP * gamma, f"{what}: an edge within {half / gamma:.2e} gamma of the threshold"
    assert min(below, above) >= MIN_BRANCH, f"{what}: branch fractions {below:.3f} / {above:.3f}"
    return half


def graph_gammas(t6):
    """Per-graph (gamma [G], half_gap [G]) from the oracle's prox input t [B,G,F,4,H,W]; asserts the gap
    condition for every graph."""
    gammas, halves = [], []
    for gi in range(t6.shape[1]):
        a = t6[:, gi].abs()
        gm, _ = gap_gamma(a)
        # the threshold the kernels use: exp of log gamma rounded to fp32 (the parameter is log gamma)
        gm = float(torch.exp(torch.log(torch.tensor(gm, dtype=torch.float64)).float().double()))
        halves.append(assert_gap(a, gm, f"graph {gi}"))
        gammas.append(gm)
    return torch.tensor(gammas, dtype=torch.float64), torch.tensor(halves, dtype=torch.float64)


# ---------------------------------------------------------------------------
_TAP_POS = ((1, 1), (0, 1), (1, 0), (1, 2), (2, 1))   # centre, up, left, right, down (kernels.stencil_taps)


def taps_kernel(taps):
    """[C,5] taps -> the [C,1,3,3] depthwise cross-correlation kernel the oracle's stats_conv takes."""
    basis = torch.zeros(5, 3, 3, dtype=taps.dtype)
    for t, (i, j) in enumerate(_TAP_POS):
        basis[t, i, j] = 1.0
    return torch.einsum("ct,tij->cij", taps, basis)[:, None]


def prox_input(x, taps, w, G):
    """The oracle's prox input t = C P x [B,G,F,4,H,W] in float64."""
    b, c, h, wd = x.shape
    return O.gtv_C(x.double().reshape(b, G, c // G, h, wd), w.double(), taps_kernel(taps.double()))


def term_phi(mode, x, g, taps, w, gamma, scale, coef, G):
    """Phi = coef * sum_g scale[g] <g_g, term_g(x)> on tensors of one dtype (float64 in every use here); gamma
    [G] is the threshold itself (mode 2)."""
    b, c, h, wd = x.shape
    f = c // G
    k = taps_kernel(taps)
    x5 = x.reshape(b, G, f, h, wd)
    if mode == TERM_GLR:
        term = O.glr_apply(x5, w, k)
    elif mode == TERM_PAIR:
        term = O.gtv_apply(x5, w, k)
    else:
        t = O.gtv_C(x5, w, k)
        term = O.gtv_Ct(2.0 * O.soft_threshold(t, gamma) - t, w, k)
    return coef * ((term * g.reshape(b, G, f, h, wd)).sum(dim=(0, 2, 3, 4)) * scale).sum()


def term_reference(mode, x, g, taps, w, log_gamma, scale, coef, G):
    """Gradients of  Phi = coef * sum_g scale[g] <g_g, term_g(x)>  in float64 on the CPU by autograd through
    the oracle, with term = glr_apply (mode 0), gtv_apply on the raw 4-plane weights (mode 1) or Ct(phi(C x)),
    phi(t) = 2 soft(t, gamma) - t, gamma = exp(log_gamma) (mode 2).  Returns dict(out = dPhi/dx, gw =
    dPhi/dw, gtaps = dPhi/dtaps [C,5], gscale = dPhi/dscale [G], ggam = dPhi/dgamma [G] (mode 2)): what
    solver_grad's glr_term_bwd / gtv_term_bwd / _Level.prox_bwd add to out / gw / gtaps / gscale (gro) /
    ggam.  ggam is the derivative in gamma itself, not in log gamma: graph_bwd.hip's prox reverse says
    "ggam[g] += scale * d<a,o>/dgamma", and solver_grad._mixture_bwd multiplies it by gamma to reach the
    log gamma parameter."""
    leaf = lambda t: t.detach().cpu().double().clone().requires_grad_(True)   # noqa: E731
    xd, td, wdd, sd = leaf(x), leaf(taps), leaf(w), leaf(scale)
    gam = leaf(torch.exp(log_gamma.detach().cpu().double())) if mode == TERM_PROX else None
    phi = term_phi(mode, xd, g.detach().cpu().double(), td, wdd, gam, sd, coef, G)
    leaves = [xd, wdd, td, sd] + ([gam] if gam is not None else [])
    grads = torch.autograd.grad(phi, leaves)
    out = dict(zip(("out", "gw", "gtaps", "gscale", "ggam"), grads))
    assert all(v.dtype == torch.float64 for v in out.values())
    return out


# ---------------------------------------------------------------------------
# Inputs of the term-reverse tests (issue: x, g ~ N(0,1); taps ~ 0.5 N(0,1); w = softmax over the 4 edges
# of 2 N(0,1); scale in [0.5, 1.5) distinct per graph; accumulators pre-filled)
def term_inputs(case, mode, seed_bump=0):
    """CPU float32 inputs of one (case, mode): dict(x, g, taps, w, scale, log_gamma, pre_*), deterministic."""
    b, G, F, h, wd = case
    gen = torch.Generator().manual_seed(1000 * mode + 7 * h + wd + 31 * F + 3 * b + G + 100003 * seed_bump)
    rn = lambda *s: torch.randn(*s, generator=gen)   # noqa: E731
    C = G * F
    d = dict(x=rn(b, C, h, wd), g=rn(b, C, h, wd), taps=0.5 * rn(C, 5),
             w=torch.softmax(2.0 * rn(b, G, 4, h, wd), dim=2).contiguous())
    d["scale"] = 0.5 + (torch.randperm(G, generator=gen).float() + torch.rand(G, generator=gen)) / G
    d["pre_out"] = 0.5 * rn(b, C, h, wd)
    d["pre_gw"] = 0.5 * rn(b, G, 4, h, wd)
    d["pre_gc"] = 0.5 * rn(b, G, 2, h, wd)
    d["pre_gtaps"] = 0.5 * rn(C, 5)
    d["pre_gscale"] = 0.5 * rn(G)
    d["pre_ggam"] = 0.5 * rn(G)
    d["log_gamma"] = None
    if mode == TERM_PROX:
        gam, half = graph_gammas(prox_input(d["x"], d["taps"], d["w"], G))
        d["log_gamma"] = torch.log(gam).float()
        d["half_gap"] = half
    return d


@functools.lru_cache(maxsize=None)
def term_case(case, mode):
    """(inputs, reference) of one (case, mode), computed once and shared by every knob setting."""
    d = term_inputs(case, mode, PROX_SEED_BUMP.get(case, 0) if mode == TERM_PROX else 0)
    coef = COEF
    if mode == TERM_PROX:
        # _Level.prox_bwd has no coef argument (the solver's rhs carries none) and takes ro = exp(log ro) in
        # fp32 as its scale: coef goes on the cotangent, Phi being linear in g, and the reference takes the
        # same fp32 product and the same fp32 ro
        d["g"] = (COEF * d["g"]).contiguous()
        d["log_scale"] = torch.log(d["scale"])
        d["scale"] = torch.exp(d["log_scale"])
        coef = 1.0
    ref = term_reference(mode, d["x"], d["g"], d["taps"], d["w"], d["log_gamma"], d["scale"], coef, case[1])
    return d, ref


COEF = 0.7

# knob settings: (term rows, tail launch, width cap of the x-gradient pass inside)
KNOBS = {
    "default": dict(rows=2, tail=1, cap=128),
    "notail": dict(rows=2, tail=0, cap=128),
    "rows1": dict(rows=1, tail=1, cap=128),
    "rows0": dict(rows=0, tail=1, cap=128),
    "acc": dict(rows=2, tail=1, cap=1 << 20),
    "acc_notail": dict(rows=2, tail=0, cap=1 << 20),
}
D, NT, R1, R0, ACC, ACCNT = "default", "notail", "rows1", "rows0", "acc", "acc_notail"

# (B, G, F, H, W), knob settings.  The launch of every case was derived from solver_grad (_acc_ok /
# _use_fused), kernels.term_rows_ok and graph_bwd.hip (term_strip_vec, term_ring_shape_ok,
# grr_bwd_term_acc_supported, launch_term_row) and is written GLR | pair | prox where the three differ.
# acc = the x-gradient pass inside (grr_bwd_term_fused_acc, PADJ); ring = LDS-ring kernel; reg =
# register-prefetch row kernel; Vn = n-column lanes; "n+t" = n main strips and the one-column tail launch at
# the given column; per-pixel / five-pass = no row kernel.  Ring strips own 64 V - 8 columns (V4: 248, V2:
# 120), register strips 62 V (V4: 248, V2: 124).  Knobs: notail = set_term_tail(False), rows1 / rows0 =
# set_term_rows(1 / 0), acc = set_term_acc_max_w(1 << 20) (GLR at W > 256 then stays on two-column lanes),
# acc_notail = both.  H <= 32 is one row segment.
TERM_CASES = [
    # --- one strip: lane widths ------------------------------------------------------------------------
    # W = 32: acc reg V1 | acc reg V1 | acc ring V1 (only the prox term takes the ring below W = 64).
    # rows1: acc reg V1.  rows0: per-pixel
    ((1, 2, 3, 5, 32), (D, R1, R0)),
    # F = 16 (W <= 128 only), H = 2: above the ring's 12 channels: acc reg V1
    ((1, 1, 16, 2, 32), (D,)),
    # W = 64, B = 3, H = 2: acc ring V1.  rows1: acc reg V1.  rows0: per-pixel
    ((3, 2, 3, 2, 64), (D, R1, R0)),
    # F = 12, the ring's limit at one- and two-column lanes, H = 3: acc ring V1.  rows1: acc reg V1
    ((1, 2, 12, 3, 64), (D, R1)),
    # F = 5 (no per-pixel instance): acc ring V1.  rows1: acc reg V1
    ((1, 2, 5, 3, 64), (D, R1)),
    # W = 100: acc ring V2.  rows1: acc reg V2.  rows0: per-pixel
    ((1, 2, 2, 17, 100), (D, R1, R0)),
    # F = 16 at two-column lanes: acc reg V2 (above the ring's 12)
    ((1, 1, 16, 3, 100), (D,)),
    # W = 102: W % 4 != 0, no ring: acc reg V2
    ((1, 2, 4, 3, 102), (D,)),
    # W = 101: no row kernel at odd W > 64: per-pixel (F <= 4); F = 5: the five-pass path
    ((1, 2, 3, 4, 101), (D,)),
    ((1, 1, 5, 3, 101), (D,)),
    # W = 200, H = 70 (segments 18 + 18 + 18 + 16, halo rows): ring V4, x-gradient pass outside (W > 128).
    # rows1: reg V4, 4 segments.  rows0: per-pixel.  acc: acc ring V4 PADJ, 4 segments
    ((1, 2, 4, 70, 200), (D, R1, R0, ACC)),
    # F = 7, the ring's limit at four-column lanes: ring V4.  F = 8 leaves it: reg V4
    ((1, 1, 7, 2, 200), (D,)),
    ((1, 1, 8, 2, 200), (D,)),
    # W = 256, H = 1: F = 12: reg V4 (F > 7).  F = 1, B = 2: ring V4; rows0: per-pixel
    ((1, 1, 12, 1, 256), (D,)),
    ((2, 2, 1, 1, 256), (D, R0)),
    # W = 256, H = 33 (segments 17 + 16): ring V4.  rows1: reg V4.  acc: acc ring V4 PADJ
    ((2, 2, 3, 33, 256), (D, R1, ACC)),
    # --- W > 256: column strips, tail and policy -------------------------------------------------------
    # W = 264, the first width above 256: ring V4 1+t@248 (tail owns 16) | same | ring V2 2+t@240 (tail owns
    # 24).  notail: ring V4 2 strips | same | ring V2 3 strips.  rows1: reg V4 2 strips | same | reg V2 3
    # strips (124 + 124 + 16).  rows0: per-pixel.  acc: acc ring V2 PADJ 2+t@240 | acc ring V4 PADJ 1+t@248 |
    # acc ring V2 PADJ 2+t@240 (the PADJ tail launch).  acc_notail: the same without the tail launch
    ((1, 2, 3, 3, 264), (D, NT, R1, R0, ACC, ACCNT)),
    # the same launches at F = 6 with two row segments (17 + 16), so segment and tail slots interleave
    ((1, 1, 6, 33, 264), (D, NT, ACC, ACCNT)),
    # F = 5 in strips: as F = 3 above
    ((1, 1, 5, 2, 264), (D, ACC)),
    # W = 300: ring V4 1+t@248 (tail owns 52) | same | ring V2 3 strips (120 + 120 + 60: no tail).  notail:
    # ring V4 2 strips.  rows1: reg V4 2 strips | same | reg V2 3 strips (last owns 52).  acc: acc ring V2
    # PADJ 3 strips | acc ring V4 PADJ 1+t@248 | acc ring V2 PADJ 3 strips.  acc_notail: pair without the tail
    ((1, 2, 4, 2, 300), (D, NT, R1, R0, ACC, ACCNT)),
    # W = 304: the tail owns exactly 56 columns, the boundary: ring V4 1+t@248 | same | ring V2 3 strips (last
    # owns 64).  acc: acc ring V2 PADJ 3 strips | acc ring V4 PADJ 1+t@248 | acc ring V2 PADJ 3 strips
    ((1, 1, 6, 1, 304), (D, NT, ACC, ACCNT)),
    # W = 308: the last strip owns 60 > 56: ring V4 2 strips, no tail | same | ring V2 3 strips (last owns 68)
    ((1, 1, 6, 2, 308), (D, NT, ACC)),
    # W = 400, F = 7: ring V4 2 strips (248 + 152) | same | ring V2 3+t@360 (tail owns 40).  acc: acc ring V2
    # PADJ 3+t@360 | acc ring V4 PADJ 2 strips | acc ring V2 PADJ 3+t@360
    ((1, 1, 7, 3, 400), (D, ACC)),
    # F = 8 leaves the ring at four-column lanes: GLR on two-column lanes, ring V2 3+t@360 | pair reg V4 2
    # strips | ring V2 3+t@360.  acc: acc ring V2 PADJ 3+t@360 | reg V4 2 strips | acc ring V2 PADJ 3+t@360
    ((1, 1, 8, 2, 400), (D, ACC)),
    # W = 512, B = 2, G = 3 (reduction slots of strips, tail and batch per graph): ring V4 2+t@496 (tail owns
    # 16) | same | ring V2 4+t@480 (tail owns 32).  notail: 3 | 3 | 5 strips.  rows1: reg V4 3 strips | same |
    # reg V2 5 strips.  rows0: per-pixel.  acc: acc ring V2 PADJ 4+t@480 | acc ring V4 PADJ 2+t@496 | acc ring
    # V2 PADJ 4+t@480.  acc_notail: the same in 5 | 3 | 5 strips
    ((2, 3, 2, 3, 512), (D, NT, R1, R0, ACC, ACCNT)),
    # the same launches at F = 6, G = 2 with two row segments (17 + 16)
    ((1, 2, 6, 33, 512), (D, NT, ACC, ACCNT)),
    # F = 12 at W = 512: ring V2 4+t@480 | reg V4 3 strips (F > 7) | ring V2 4+t@480.  acc: acc ring V2 PADJ
    # 4+t@480 | reg V4 3 strips | acc ring V2 PADJ 4+t@480
    ((1, 1, 12, 2, 512), (D, ACC)),
    # W = 744: ring V4 3 whole strips | same | ring V2 6+t@720 (tail owns 24).  rows1: reg V4 3 strips | same |
    # reg V2 6 whole strips of 124.  acc: acc ring V2 PADJ 6+t@720 | acc ring V4 PADJ 3 strips | acc ring V2
    # PADJ 6+t@720
    ((1, 1, 3, 2, 744), (D, NT, R1, ACC)),
    # W = 302, W % 4 != 0: reg V2 in 3 strips (124 + 124 + 54) | per-pixel (the pair term has no two-column
    # strips) | reg V2 in 3 strips.  rows1: the same.  rows0: per-pixel
    ((1, 2, 3, 3, 302), (D, R1, R0)),
]
TERM_CASES = [(*c, k) for c, k in TERM_CASES]

# prox cases whose first seed leaves an edge too near the widest gap's middle (test_term_ref checks all)
PROX_SEED_BUMP = {}

# ---------------------------------------------------------------------------
# End-to-end cases (test_gpu_grad.py): the widths the C4 configuration trains at
WIDE_LOWPASS = [dict(g=2, f=6, b=1, h=16, w=512, s=10), dict(g=2, f=6, b=1, h=40, w=264, s=10),
                dict(g=2, f=3, b=1, h=70, w=300, s=4)]
WIDE_MSGF = dict(g=4, s=3, shape=(1, 3, 16, 264))


def capture_prox_inputs(fn):
    """Run fn() once with O.soft_threshold wrapped; returns the prox inputs t [B,G,F,4,H,W] in call order
    (full level, half level), detached."""
    seen = []
    orig = O.soft_threshold

    def wrapped(d, gamma):
        seen.append(d.detach())
        return orig(d, gamma)
    O.soft_threshold = wrapped
    try:
        with torch.no_grad():
            fn()
    finally:
        O.soft_threshold = orig
    return seen


def set_gap_gammas(module, mixture, fn):
    """Set mixture.gamma00 / gamma01 per graph by gap_gamma from the oracle's |t| at the two levels' prox
    inputs, taken from one float64 oracle forward fn(params) on module's parameters (the prox input does
    not depend on gamma).  Asserts the gap condition for every graph of both levels; returns the smallest
    half-gap over that level's max|t|."""
    torch.set_default_dtype(torch.float64)
    try:
        params = {k: v.detach().cpu().double() for k, v in module.state_dict().items()}
        ts = capture_prox_inputs(lambda: fn(params))
    finally:
        torch.set_default_dtype(torch.float32)
    assert len(ts) == 2, len(ts)
    worst = float("inf")
    for t, p in zip(ts, (mixture.gamma00, mixture.gamma01)):
        gam, half = graph_gammas(t)
        with torch.no_grad():
            p.copy_(torch.log(gam).float().reshape(p.shape))
        worst = min(worst, float(half.min()) / float(t.abs().max()))
    return worst


def wide_lowpass(irdu, case):
    """(block, x, oracle function, smallest half-gap / max|t|) of one WIDE_LOWPASS case: the module and input
    of test_lowpass_block_grad (same seeds) with the thresholds set by the gap rule."""
    from tests.test_gpu_parity import perturb_mixture, rand
    torch.manual_seed(5)
    c = case["g"] * case["f"]
    blk = irdu.LocalLowpassFilteringBlock(dim=c, nsubnets=1, ngraphs=case["g"], n_cgd_iters=case["s"])
    perturb_mixture(blk.local_filter, 51)
    with torch.no_grad():
        blk.skip_weight.copy_(torch.tensor([0.4, 0.9]))
    x = rand(case["b"], c, case["h"], case["w"], seed=19)
    fn = lambda xd, p: O.lowpass_block(xd, p, case["g"])   # noqa: E731
    ratio = set_gap_gammas(blk, blk.local_filter, lambda p: fn(x.double(), p))
    return blk, x, fn, ratio


def wide_msgf(irdu):
    """The same for the MultiScaleGraphFilter case (v13 feature CNN, the LNB reverse at a strip width)."""
    from tests.test_gpu_parity import perturb_mixture
    torch.manual_seed(6)
    g = WIDE_MSGF["g"]
    m = irdu.MultiScaleGraphFilter(3, 3, ngraphs=g, n_cgd_iters=WIDE_MSGF["s"])
    perturb_mixture(m.localfilter, 61)
    x = torch.rand(*WIDE_MSGF["shape"], generator=torch.Generator().manual_seed(62))
    fn = lambda xd, p: O.multiscale_graph_filter(xd, p, g)   # noqa: E731
    ratio = set_gap_gammas(m, m.localfilter, lambda p: fn(x.double(), p))
    return m, x, fn, ratio
