"""References, bounds, the case table and emulated mutants of the window-graph reverse kernels (csrc/window_bwd.hip:
the eight grr_win_bwd_* entry points).  tests/test_window_bwd_ref.py checks all of this on the CPU,
tests/test_gpu_window_bwd_kernels.py runs the kernels against it.  Modelled on tests/window_ref.py, whose windows,
stencil slices, plane measure and fp32-class bound it reuses.  Nothing here imports or touches a kernel.

Unit under test: one entry point each, called the way kernels.win_bwd_* call it.

    term     kernels.win_bwd_glr / win_bwd_gtv (pass 1 + the gather, fused or through the E / PW planes) on fp32
             s, bt, w, sc, log_gamma:  y = l or o,  gs = dL/ds,  gw += dL/dw  with  L = sum sc[g] bt y(s, w),
             gdot[g] += coef <bt, y>,  prox: ggamma[g] += dL/dgamma (the log-gamma gradient divided by gamma)
    stencil  kernels.win_bwd_stencil  mode 0 P (reflect), 1 T* (zero-frame correlation), 2 P* (reflect adjoint);
             out = [out +] scale[g] y
    tapgrad  kernels.win_bwd_tapgrad  gtaps[t] += sum scale[g] u(p) z(reflect(p + d_t)) (mode 0) or z(p - d_t) (1)
    edge     kernels.win_bwd_edge_weights  gfeat slab += dL/dfeat, gmultiM += dL/dM, L = sum w(feat, M) gw
    mix      kernels.win_bwd_mix  gx = gout score, gscore = sum_c gout x

ref64: float64.  Terms and edge weights by autograd through the oracle's blocks (O.glr_apply, O.gtv_C,
O.soft_threshold, O.gtv_Ct with the identity stencil kernel33((1, 0, 0, 0, 0)), so that s is the oracle's input;
O.edge_weights); stencils, tap gradients and the mix in closed form on slices.
ref32: the same function in fp32 from elementwise adds, subtracts and multiplies on shifted slices (edge sums in edge
order, window_ref._evaluate's style), differentiated by autograd: its backward is again elementwise ops and slice
accumulation.  exp, the root, the reciprocal and the softmax's division of the edge weights are each evaluated in
float64 from fp32 inputs and rounded once, their derivatives again elementwise in fp32 (_Exp, _Div, _InvNorm).
Other honest fp32 evaluations, which every case must keep inside its bound on the CPU or be replaced (_RESEED):
the reverse edge order (_term32(reverse=True)), the gather form in both edge orders (gather32), the E-planes path's
running sum in the kernel's order on frames of at most 12 pixels (seq_gather32); the edge weights with every chain
reversed (edge_alt32).

Bounds (none fitted to a kernel's output):
    elementwise outputs (y, gs, gw, gfeat, stencil out, gx, gscore): bound_of(err32) = 4 err32 + 1e-7 per plane,
        err = max |d| / max |ref64| over the plane: (b, g, c) for signals, (b, g) for edge planes and gscore, (b, slab
        channel) for gfeat.  Into a pre-filled buffer: got against pre + ref64 at the scale max |ref64| of the plane,
        plus 2^-23 max |pre + ref64| / max |ref64| for the one rounding of the add (ratio_acc).
    sums (gdot, ggamma, gtaps, gM): |got - (pre + ref)| <= 2e-5 max(|ref|, ||t||_2), t the float64 summands of the
        sum (per pixel and channel for gdot, gtaps and gM, per edge for ggamma), as test_gpu_term_oracle.py /
        test_gpu_term_rows.py hold sums; a missing or doubled pixel moves a sum by about ||t||_2 / sqrt(N).
    F = 1: the feature gradient (gn - n (n . gn)) / |f| is identically zero off the zero-norm pixel, so max |ref64|
        is rounding noise and the plane bound says nothing; there the error is also held to 2e-5 of the un-projected
        max |gn| / |f| (test_gpu_term_oracle.py's rule for the same case).

Kink rule (prox): gamma[g] is the midpoint of the widest gap between consecutive sorted |z| of the graph's edges
inside the quantile window q +- 0.15, q = 0.35 / 0.5 / 0.65 cycling over the graphs (term_ref.gap_gamma's idea), then
exp(fp32(log gamma)) as the kernel sees it; z in float64 from the fp32 s and w.  kink(case) returns the half gap, the
fp32 rounding bound 2^-23 max (|w s(p)| + |w s(n)|) of the kernel's z and the branch fractions per plane; required
(tests/test_window_bwd_ref.py): half gap >= 16 x rounding bound, every branch >= 5 % of every plane's edges, no edge
excluded.  Prox cases are sized for it: about (half gap) ~ 6 / (edges per graph x density), so the big frames take
the small windows and B = 1.

Launch geometry (window_bwd.hip: NTB = 256; plane_grid gives a (b, g) plane min(ceil(HW / 256), max(1, 4096 / (B G)))
blocks; grid_red 4096 blocks; grid_1d 65536 blocks): plane_blocks, sweeps_of, first_sweep.

Mutants (float64 evaluations with one thing wrong, none touching a kernel):
    a  the gather drops the clamp fold: only q - d_e inside counts (gs)
    b  the fold per axis but not at corners: the sources folded on both axes are dropped (gs).  Applies only to
       windows with a diagonal edge (not cross4, plus8: an axis edge folds along one axis only)
    c  GTV reads b(clamp(p + d)) where the edge leaves the frame, instead of 0 (gs, gw, gdot, ggamma).  It does not
       apply to cross4: an axis edge of reach 1 that leaves the frame clamps onto its own pixel, so z = 0, s(p) - s(n)
       = 0 and E_e(p) comes back to p itself: b's difference multiplies nothing that survives
    d  prox: gz = gph inside the threshold too (gs, gw)
    e  prox: ggamma takes -2 on both outer branches
    f  P* (stencil mode 2) lacks the reflected sources at q = 1 and q = n - 2
    g  the T tap gradient reads z(p + d_t) instead of z(p - d_t).  The centre tap (d = 0) cannot show it.
    h  strided cases: the pixels of the second sweep contribute nothing to the sums (gdot, ggamma, gtaps, gM) and
       their gw / gfeat stay at the pre-fill.  Applies only where a second sweep exists.
"""
from collections import namedtuple
from functools import lru_cache
import math

import numpy as np
import torch

from oracle import window_oracle as O
from tests.window_ref import (WINDOWS, _S, _pad, _shift, _slices, _soft, bound_of, delta_of, family, kernel33,
                              plane_err, taps_of)

NTB = 256
TERMS = ("glr", "gtv", "prox")
FAMILIES = ("r1k8", "r1k0", "r2k12", "r2k24", "r2k0")
STOL = 2e-5                      # sums, times max(|ref|, ||t||_2)
KINK_MARGIN, MIN_BRANCH = 16.0, 0.05
EPS32 = 2.0 ** -23
COEF = {"glr": -1.0, "gtv": 0.5, "prox": -0.75}
_SC = (0.45, 0.04, 0.7, 0.9, 0.3, 0.6, 0.2, 0.8)       # graph 1 small
_Q = (0.35, 0.5, 0.65)


# ---- launch geometry -------------------------------------------------------------------------------------------
def plane_blocks(hw, planes):
    return min((hw[0] * hw[1] + NTB - 1) // NTB, max(1, 4096 // max(planes, 1)))


def first_sweep(hw, planes):
    """Pixels of a plane the first grid-stride sweep of a plane_grid kernel covers."""
    return min(plane_blocks(hw, planes) * NTB, hw[0] * hw[1])


def sweeps_of(hw, planes):
    return -(-hw[0] * hw[1] // (plane_blocks(hw, planes) * NTB))


def red_first_sweep(n):
    return min(n, 4096 * NTB)


def grid1d_first_sweep(n):
    return min(n, 65536 * NTB)


def _bc(v):
    return v[None, :, None, None, None]


def _weights(shape, gen):
    return torch.softmax(2.0 * torch.randn(shape, generator=gen, dtype=torch.float64), dim=2).float()


def _scales(g, gen):
    base = torch.tensor([_SC[i % len(_SC)] for i in range(g)])
    return (base + 0.02 * torch.rand(g, generator=gen)).contiguous()


# ---- the term cases --------------------------------------------------------------------------------------------
TermCase = namedtuple("TermCase", "window term fs hw b g seed")
FRAMES = ((2, 2), (3, 2), (2, 5), (4, 3), (2, 700), (17, 65), (33, 130))
# prox stays off frames of fewer than ten pixels (too few edges per plane for each branch to hold 5 %); the kink rule
# sizes the rest: window -> ((frame, B, Fs), (frame, B, Fs))
_PROX = {
    "ring3": (((33, 130), 1, 1), ((2, 5), 2, 2)),
    "cross4": (((33, 130), 1, 2), ((2, 700), 2, 3)),
    "diamond5": (((4, 3), 2, 3), ((17, 65), 1, 1)),
    "full5": (((2, 5), 2, 1), ((4, 3), 2, 2)),
    "plus8": (((2, 700), 1, 1), ((17, 65), 1, 2)),
    "round20": (((4, 3), 2, 3), ((2, 5), 2, 1)),
}


# Seeds replaced because the draw was ill-conditioned: a second honest fp32 evaluation left the bound on a plane of
# gs.  All four are 20- and 24-edge windows on 2 x 2 and 3 x 2, where up to 9 K terms fold onto each of 4 or 6 pixels
# and the plane's err32 is a maximum over as few values: full5 linear GTV on both frames under the reverse edge order
# (alt32), round20 GLR on 2 x 2 under the gather form (gather32, 1.69 x bound) and round20 linear GTV on 3 x 2 under
# the E-planes path's own running sum (seq_gather32, 1.32 x bound; the kernels gave the same two figures to three
# digits).  Decided on the CPU from the references alone; tests/test_window_bwd_ref.py asserts it for every case.
_RESEED = {6310: 7310, 6311: 7311, 6501: 7501, 6510: 8510}


def _term_cases():
    out, j = [], 0
    for wi, window in enumerate(WINDOWS):
        for ti, term in enumerate(TERMS):
            for r in range(2):
                seed = 6000 + 100 * wi + 10 * ti + r
                seed = _RESEED.get(seed, seed)
                if term == "prox":
                    hw, b, fs = _PROX[window][r]
                    out.append(TermCase(window, term, fs, hw, b, 2 + (wi + r) % 2, seed))
                else:
                    out.append(TermCase(window, term, 1 + j % 3, FRAMES[j % len(FRAMES)], 2, 2 + (j // 3) % 2, seed))
                    j += 1
    return out


TERM_CASES = _term_cases()
# B G = 1024 planes of 33 x 33: 4 blocks per plane, a first sweep of 1024 pixels and a second of 65 (one wave and
# one lane of block 0; blocks 1..3 reduce an empty second sweep).  n = 1,115,136 > 1,048,576: grid_red strides too.
STRIDED_HW, STRIDED_B, STRIDED_G = (33, 33), 128, 8
STRIDED_WINDOWS = ("cross4", "ring3")
# The kink rule cannot hold with 128 x 1089 x K edges per graph (557,568 at K = 4: the widest gap near the median
# is about 5 x the rounding bound, 1 x at K = 8), so the prox cases keep the 1024 planes -- the launch is the same --
# and split them as B = 4, G = 256: 32 times fewer edges per gamma.
STRIDED_PROX_B, STRIDED_PROX_G = 4, 256
STRIDED_CASES = [TermCase(wn, term, 1, STRIDED_HW, *((STRIDED_PROX_B, STRIDED_PROX_G) if term == "prox" else
                                                      (STRIDED_B, STRIDED_G)), 6900 + 10 * wi + ti)
                 for wi, wn in enumerate(STRIDED_WINDOWS) for ti, term in enumerate(TERMS)]


def term_id(c):
    return f"{c.window}-{c.term}-Fs{c.fs}-{c.hw[0]}x{c.hw[1]}-B{c.b}G{c.g}"


TERM_IDS = [term_id(c) for c in TERM_CASES]
STRIDED_IDS = [term_id(c) for c in STRIDED_CASES]
TermInputs = namedtuple("TermInputs", "s bt w sc log_gamma coef gw_pre gdot_pre ggam_pre delta")


def _z64(s, w, delta):
    """z_e(p) = w_e s(p) - w_e s(n_e(p)) in float64, [B,G,Fs,K,H,W], and |w s(p)| + |w s(n)|."""
    h, ww = s.shape[-2:]
    s, w = s.double(), w.double()
    sp = _pad(s, 2, "replicate")
    z, mag = [], []
    for e, (dy, dx) in enumerate(delta):
        we, sn = w[:, :, e][:, :, None], _shift(sp, dy, dx, h, ww)
        z.append(we * s - we * sn)
        mag.append((we * s).abs() + (we * sn).abs())
    return torch.stack(z, 3), torch.stack(mag, 3)


def _gap_gamma(abs_z, q):
    v = torch.sort(abs_z.reshape(-1)).values
    n = v.numel()
    lo, hi = int(math.floor((q - 0.15) * (n - 1))), int(math.ceil((q + 0.15) * (n - 1)))
    d = v[lo + 1:hi + 1] - v[lo:hi]
    i = int(torch.argmax(d))
    return float(v[lo + i] + 0.5 * d[i])


@lru_cache(maxsize=None)
def term_inputs(case):
    gen = torch.Generator().manual_seed(case.seed)
    b, g, fs = case.b, case.g, case.fs
    h, w = case.hw
    delta = delta_of(case.window)
    k = len(delta)
    s = torch.randn((b, g, fs, h, w), generator=gen)
    bt = torch.randn((b, g, fs, h, w), generator=gen)
    wt = _weights((b, g, k, h, w), gen)
    sc = _scales(g, gen)
    gw_pre = 0.1 * torch.randn((b, g, k, h, w), generator=gen)
    gdot_pre, ggam_pre = torch.randn(g, generator=gen), torch.randn(g, generator=gen)
    log_gamma = None
    if case.term == "prox":
        z, _ = _z64(s, wt, delta)
        gam = [_gap_gamma(z[:, gi].abs(), _Q[gi % 3]) for gi in range(g)]
        log_gamma = torch.log(torch.tensor(gam, dtype=torch.float64)).float().contiguous()
    return TermInputs(s, bt, wt, sc, log_gamma, COEF[case.term], gw_pre, gdot_pre, ggam_pre, delta)


Kink = namedtuple("Kink", "half_gap rounding fractions")


def kink(case):
    """Per graph: the distance of the nearest |z| to the kernel's gamma, the fp32 rounding bound of z; and the branch
    fractions [planes, 3] (z < -gamma, |z| <= gamma, z > gamma) per (b, g, c) plane.  No edge is excluded."""
    inp = term_inputs(case)
    z, mag = _z64(inp.s, inp.w, inp.delta)
    gm = torch.exp(inp.log_gamma.double())
    half = torch.stack([(z[:, gi].abs() - gm[gi]).abs().min() for gi in range(case.g)])
    rnd = torch.stack([EPS32 * mag[:, gi].max() for gi in range(case.g)])
    g6 = gm[None, :, None, None, None, None]
    fr = torch.stack([(z < -g6), (z.abs() <= g6), (z > g6)], -1).double().mean((3, 4, 5))
    return Kink(half, rnd, fr.reshape(-1, 3))


# ---- ref64 of a term: autograd through the oracle's blocks ------------------------------------------------------
def _term64(case):
    inp = term_inputs(case)
    d = torch.float64
    dl = np.asarray(inp.delta)
    s, w = inp.s.double().requires_grad_(True), inp.w.double().requires_grad_(True)
    kI = kernel33(torch.tensor([1.0, 0.0, 0.0, 0.0, 0.0], dtype=d), case.fs)
    leaves = [s, w]
    if case.term == "glr":
        y = O.glr_apply(s, w, kI, dl)
    else:
        e = O.gtv_C(s, w, kI, dl)
        if case.term == "prox":
            lg = inp.log_gamma.double().requires_grad_(True)
            leaves.append(lg)
            eps = O.soft_threshold(e, torch.exp(lg))
            e = eps - (e - eps)
        y = O.gtv_Ct(e, w, kI, dl)
    bt = inp.bt.double()
    grads = torch.autograd.grad((bt * y * _bc(inp.sc.double())).sum(), leaves)
    out = {"y": y.detach(), "gs": grads[0], "gw": grads[1], "gdot": inp.coef * (bt * y.detach()).sum((0, 2, 3, 4))}
    if case.term == "prox":
        out["ggamma"] = grads[2] / torch.exp(inp.log_gamma.double())
    return out


# ---- ref32 / alt32: the forward from elementwise ops on shifted slices, differentiated by autograd ---------------
def _term_forward(s, w, delta, term, gm, reverse=False):
    h, ww = s.shape[-2:]
    sp = _pad(s, 2, "replicate")
    order = list(enumerate(delta))
    if reverse:
        order.reverse()
    if term == "glr":
        wx = torch.zeros_like(s)
        for e, (dy, dx) in order:
            wx = wx + w[:, :, e][:, :, None] * _shift(sp, dy, dx, h, ww)
        return s - wx
    acc, pws = torch.zeros_like(s), []
    for e, (dy, dx) in order:
        we = w[:, :, e][:, :, None]
        z = we * s - we * _shift(sp, dy, dx, h, ww)
        if term == "prox":
            eps = _soft(z, gm)
            z = eps - (z - eps)
        pw = we * z
        pws.append(((dy, dx), pw))
        acc = acc + pw
    acc = acc.clone()
    for (dy, dx), pw in pws:
        src, dst = _slices(dy, dx, h, ww)
        acc[..., dst[0], dst[1]] = acc[..., dst[0], dst[1]] - pw[..., src[0], src[1]]
    return acc


def _term32(case, reverse=False):
    inp = term_inputs(case)
    s, w = inp.s.clone().requires_grad_(True), inp.w.clone().requires_grad_(True)
    gm = _bc(torch.exp(inp.log_gamma.double()).float()) if case.term == "prox" else None     # expf, rounded once
    y = _term_forward(s, w, inp.delta, case.term, gm, reverse)
    gs, gw = torch.autograd.grad(((_bc(inp.sc) * inp.bt) * y).sum(), [s, w])
    out = {"y": y.detach(), "gs": gs, "gw": gw}
    assert all(v.dtype == torch.float32 for v in out.values())
    return out


# ---- the reverse written out (float64): the summands of the sums, and the mutants ---------------------------------
def _scatter(planes, delta, h, w, fold):
    """out[n(p + d_e)] += E_e[p] summed over the edges.  fold 'clamp': n = clamp; 'none': what leaves the frame is
    dropped; 'axes': folded along one axis only (what leaves the frame on both axes is dropped)."""
    first = planes[0]
    buf = torch.zeros((*first.shape[:-2], h + 4, w + 4), dtype=first.dtype)
    for (dy, dx), e in zip(delta, planes):
        buf[..., 2 + dy:2 + dy + h, 2 + dx:2 + dx + w] += e
    if fold == "axes":
        for rs in (slice(0, 2), slice(h + 2, h + 4)):
            for cs in (slice(0, 2), slice(w + 2, w + 4)):
                buf[..., rs, cs] = 0.0
    if fold != "none":
        buf[..., 2, :] += buf[..., 0, :] + buf[..., 1, :]
        buf[..., h + 1, :] += buf[..., h + 2, :] + buf[..., h + 3, :]
        buf[..., :, 2] += buf[..., :, 0] + buf[..., :, 1]
        buf[..., :, w + 1] += buf[..., :, w + 2] + buf[..., :, w + 3]
    return buf[..., 2:2 + h, 2:2 + w]


def has_diagonal(window):
    return any(dy and dx for dy, dx in delta_of(window))


def term_mutant_applies(case, m):
    strided = sweeps_of(case.hw, case.b * case.g) > 1
    other = any((dy and dx) or max(abs(dy), abs(dx)) > 1 for dy, dx in delta_of(case.window))   # clamps elsewhere
    return {"a": True, "b": has_diagonal(case.window), "c": case.term != "glr" and other, "d": case.term == "prox",
            "e": case.term == "prox", "h": strided}.get(m, False)


def term_explicit(case, mutant=None, dtype=torch.float64, reverse=False):
    """The kernels' reverse written out on slices (pass 1's expressions, then the gather): y, gs, gw (the increment),
    gdot, ggamma, and the summands t_dot [B,G,Fs,H,W] (coef b y per pixel; per pixel the edge terms of the kernel's
    sum for GTV) and t_gam [B,G,Fs,K,H,W].  float64: the reference of the sums' summands, and the mutants.  fp32
    (gather32): a further honest fp32 ordering, the kernels' own formulation; reverse: the edges in reverse order."""
    assert mutant is None or term_mutant_applies(case, mutant)
    inp = term_inputs(case)
    h, ww = case.hw
    delta = inp.delta
    s, bt, w = inp.s.to(dtype), inp.bt.to(dtype), inp.w.to(dtype)
    sc = _bc(inp.sc.to(dtype))
    order = list(enumerate(delta))
    if reverse:
        order.reverse()
    delta = [d for _, d in order]
    sp = _pad(s, 2, "replicate")
    fold = {"a": "none", "b": "axes"}.get(mutant, "clamp")
    gws, es = [], []
    out = {}
    if case.term == "glr":
        gl, wx = sc * bt, torch.zeros_like(s)
        for e, (dy, dx) in order:
            we, sn = w[:, :, e][:, :, None], _shift(sp, dy, dx, h, ww)
            wx = wx + we * sn
            gws.append(-(gl * sn).sum(2))
            es.append(gl * we)
        y = s - wx
        gs = gl - _scatter(es, delta, h, ww, fold)
        t_dot = inp.coef * bt * y
    else:
        prox = case.term == "prox"
        bz = _pad(bt, 2, "replicate" if mutant == "c" else "constant")
        gm = _bc(torch.exp(inp.log_gamma.double()).to(dtype)) if prox else None
        gsd, t_dot, pws, tg = torch.zeros_like(s), torch.zeros_like(s), [], []
        for e, (dy, dx) in order:
            we, sn = w[:, :, e][:, :, None], _shift(sp, dy, dx, h, ww)
            z = we * s - we * sn
            bd = bt - _shift(bz, dy, dx, h, ww)
            da = sc * bd
            gph = we * da
            ph, gz = z, gph
            if prox:
                eps = _soft(z, gm)
                ph = eps - (z - eps)
                beyond = z.abs() > gm
                if mutant != "d":
                    gz = torch.where(beyond, gph, -gph)
                sign = torch.where(z < -gm, 2.0, -2.0) if mutant != "e" else torch.full_like(z, -2.0)
                tg.append(gph * torch.where(beyond, sign, torch.zeros_like(z)))
            gws.append((ph * da + gz * (s - sn)).sum(2))
            gsd = gsd + gz * we
            es.append(gz * we)
            pws.append(we * ph)
            t_dot = t_dot + inp.coef * ph * we * bd
        y = sum(pws) - _scatter(pws, delta, h, ww, "none")
        gs = gsd - _scatter(es, delta, h, ww, fold)
        if prox:
            out["t_gam"] = torch.stack(tg, 3)
    if reverse:
        gws.reverse()
        if "t_gam" in out:
            out["t_gam"] = out["t_gam"].flip(3)
    gw = torch.stack(gws, 2)
    if mutant == "h":
        keep = torch.zeros(h * ww, dtype=dtype)
        keep[:first_sweep(case.hw, case.b * case.g)] = 1.0
        keep = keep.reshape(h, ww)
        gw, t_dot = gw * keep, t_dot * keep
        if "t_gam" in out:
            out["t_gam"] = out["t_gam"] * keep
    out.update(y=y, gs=gs, gw=gw, t_dot=t_dot, gdot=t_dot.sum((0, 2, 3, 4)), E=es, gsd=gl if case.term == "glr" else gsd)
    if "t_gam" in out:
        out["ggamma"] = out["t_gam"].sum((0, 2, 3, 4, 5))
    return out


def sum_bound(ref, t, dims):
    """2e-5 max(|ref|, ||t||_2), ||t||_2 over dims of the float64 summands."""
    return STOL * torch.maximum(ref.abs(), t.double().pow(2).sum(dims).sqrt())


# elementwise outputs of a term -> the dims of a plane
TERM_DIMS = {"y": (-2, -1), "gs": (-2, -1), "gw": (-3, -2, -1)}
TermRefs = namedtuple("TermRefs", "inp out64 err32 bound sum_bound")


@lru_cache(maxsize=None)
def term_refs(case):
    out64 = _term64(case)
    out32 = _term32(case)
    ex = term_explicit(case)
    err32 = {n: plane_err(out32[n], out64[n], TERM_DIMS[n]) for n in TERM_DIMS}
    sb = {"gdot": sum_bound(out64["gdot"], ex["t_dot"], (0, 2, 3, 4))}
    if case.term == "prox":
        sb["ggamma"] = sum_bound(out64["ggamma"], ex["t_gam"], (0, 2, 3, 4, 5))
    return TermRefs(term_inputs(case), out64, err32, {n: bound_of(e) for n, e in err32.items()}, sb)


def ratio(got, ref64, bound, dims):
    """The worst err / bound over the planes of an output written from scratch."""
    return float((plane_err(got, ref64, dims) / bound).max())


def ratio_acc(got, pre, ref64, bound, dims):
    """The same for an output accumulated into ``pre``: got against pre + ref64 at the plane's scale max |ref64|,
    the bound widened by 2^-23 max |pre + ref64| / max |ref64| for the rounding of the add."""
    want = pre.double() + ref64
    scale = ref64.abs().amax(dims).clamp_min(1e-300)
    err = (got.detach().double().cpu() - want).abs().amax(dims) / scale
    return float((err / (bound + EPS32 * want.abs().amax(dims) / scale)).max())


def sum_ratio(got, pre, ref, bound):
    return float(((got.detach().double().cpu() - (pre.double() + ref)).abs() / bound).max())


def term_ratios(case, got):
    """got: y, gs (written), gw, gdot, ggamma (accumulated into the case's pre-fills; the sums may be absent) ->
    worst err / bound each."""
    r = term_refs(case)
    out = {"y": ratio(got["y"], r.out64["y"], r.bound["y"], TERM_DIMS["y"]),
           "gs": ratio(got["gs"], r.out64["gs"], r.bound["gs"], TERM_DIMS["gs"]),
           "gw": ratio_acc(got["gw"], r.inp.gw_pre, r.out64["gw"], r.bound["gw"], TERM_DIMS["gw"])}
    if "gdot" in got:
        out["gdot"] = sum_ratio(got["gdot"], r.inp.gdot_pre, r.out64["gdot"], r.sum_bound["gdot"])
    if "ggamma" in got:
        out["ggamma"] = sum_ratio(got["ggamma"], r.inp.ggam_pre, r.out64["ggamma"], r.sum_bound["ggamma"])
    return out


def gather32(case, reverse=False):
    """y, gs, gw of the gather form in fp32."""
    ev = term_explicit(case, dtype=torch.float32, reverse=reverse)
    assert ev["gs"].dtype == torch.float32
    return {n: ev[n] for n in TERM_DIMS}


def _clamp_sources(q, d, n):
    """The pixels p along one axis with clamp(p + d) = q, in win_gather_bwd_kernel's order."""
    src = [q - d] if 0 <= q - d < n else []
    if d < 0 and q == 0:
        src += [p for p in range(min(-d, n)) if p != q - d]
    if d > 0 and q == n - 1:
        src += [p for p in range(n - 1, max(n - 1 - d, -1), -1) if p != q - d]
    return src


SEQ_PIXELS = 12


def seq_gather32(case):
    """gs of the E-planes path in fp32 in the kernel's own order: pass 1's E_e(p) and gsd(p) rounded to fp32, then per
    pixel one running sum over the edges and the sources of each, subtracted from gsd.  The least accurate honest
    order (a chain of up to 9 K adds); evaluated for frames of at most SEQ_PIXELS pixels, where the folds dominate."""
    assert case.hw[0] * case.hw[1] <= SEQ_PIXELS
    ev = term_explicit(case, dtype=torch.float32)
    h, w = case.hw
    E = torch.stack(ev["E"], 3).numpy()                      # [B,G,Fs,K,H,W]
    gsd = ev["gsd"].numpy()
    delta = term_inputs(case).delta
    gs = np.empty_like(gsd)
    for r in range(h):
        for c in range(w):
            acc = np.zeros(gsd.shape[:3], dtype=np.float32)
            for e, (dy, dx) in enumerate(delta):
                for py in _clamp_sources(r, dy, h):
                    for px in _clamp_sources(c, dx, w):
                        acc = acc + E[:, :, :, e, py, px]
            gs[..., r, c] = gsd[..., r, c] - acc
    return torch.from_numpy(gs)


def as_got(case, ev):
    """An evaluation (increments) as a kernel's outputs: the accumulated ones on top of the case's pre-fills."""
    inp = term_inputs(case)
    got = {"y": ev["y"], "gs": ev["gs"], "gw": inp.gw_pre.double() + ev["gw"]}
    if "gdot" in ev:
        got["gdot"] = inp.gdot_pre.double() + ev["gdot"]
    if "ggamma" in ev:
        got["ggamma"] = inp.ggam_pre.double() + ev["ggamma"]
    return got


# ---- stencils -----------------------------------------------------------------------------------------------------
def stencil_eval(x, t, mode, mutant=None):
    """mode 0 P x (reflect frame), 1 T* x (zero-frame correlation), 2 P* x (the reflect adjoint: x(p) lands on
    reflect(p + d_t)); the taps in the kernel's order, in x's dtype."""
    h, w = x.shape[-2:]
    if mode == 0:
        return _S(x, t)
    if mode == 1:
        xp = _pad(x, 1, "constant")
        v = t[0] * xp[..., 1:-1, 1:-1]
        v = v + t[1] * xp[..., :-2, 1:-1]
        v = v + t[2] * xp[..., 1:-1, :-2]
        v = v + t[3] * xp[..., 1:-1, 2:]
        return v + t[4] * xp[..., 2:, 1:-1]
    y = t[0] * x
    for i, (dy, dx) in ((1, (-1, 0)), (2, (0, -1)), (3, (0, 1)), (4, (1, 0))):
        buf = torch.zeros((*x.shape[:-2], h + 2, w + 2), dtype=x.dtype)
        buf[..., 1 + dy:1 + dy + h, 1 + dx:1 + dx + w] = x
        if mutant != "f":
            buf[..., 2, :] = buf[..., 2, :] + buf[..., 0, :]                  # reflect(-1) = 1
            buf[..., h - 1, :] = buf[..., h - 1, :] + buf[..., h + 1, :]      # reflect(n) = n - 2
            buf[..., :, 2] = buf[..., :, 2] + buf[..., :, 0]
            buf[..., :, w - 1] = buf[..., :, w - 1] + buf[..., :, w + 1]
        y = y + t[i] * buf[..., 1:-1, 1:-1]
    return y


STENCIL_FRAMES = ((2, 2), (2, 3), (3, 4), (17, 65))
STENCIL_MODES = (0, 1, 2)
# B G Fs H W = 16,793,600 > 16,777,216 = 65536 x 256: the last four rows of the last plane belong to grid_1d's
# second sweep
GRID1D_SHAPE = (2, 2, 1, 1025, 4096)
StencilRefs = namedtuple("StencilRefs", "x taps scale pre y64 bound ys64 bound_s")


def _stencil_refs(shape, seed):
    gen = torch.Generator().manual_seed(seed)
    x, pre = torch.randn(shape, generator=gen), torch.randn(shape, generator=gen)
    st = 0.05 * torch.rand(4, generator=gen)
    taps = taps_of(0.9 + st[0], 0.3 + st[1], 0.5 + st[2], 0.2 + st[3])
    scale = _scales(shape[1], gen)
    y64, ys64, bound, bound_s = {}, {}, {}, {}
    for mode in STENCIL_MODES:
        y64[mode] = stencil_eval(x.double(), taps.double(), mode)
        y32 = stencil_eval(x, taps, mode)
        ys64[mode] = y64[mode] * _bc(scale.double())
        bound[mode] = bound_of(plane_err(y32, y64[mode]))
        bound_s[mode] = bound_of(plane_err(y32 * _bc(scale), ys64[mode]))
    return StencilRefs(x, taps, scale, pre, y64, bound, ys64, bound_s)


@lru_cache(maxsize=None)
def stencil_refs(hw):
    return _stencil_refs((2, 3, 2, *hw), 7000 + 10 * hw[0] + hw[1])


@lru_cache(maxsize=1)
def grid1d_refs():
    return _stencil_refs(GRID1D_SHAPE, 7900)


# ---- tap gradients -------------------------------------------------------------------------------------------------
_TAP_D = ((0, 0), (-1, 0), (0, -1), (0, 1), (1, 0))       # centre, up, left, right, down


def tapgrad_summands(u, z, scale, mode, mutant=None):
    """[5, B,G,Fs,H,W] float64: scale[g] u(p) z(reflect(p + d_t)) (mode 0) or u(p) z(p - d_t) [inside] (mode 1)."""
    u, z = u.double(), z.double()
    h, w = u.shape[-2:]
    uv = u * _bc(scale.double()) if scale is not None else u
    zp = _pad(z, 1, "reflect" if mode == 0 else "constant")
    sign = 1 if mode == 0 or mutant == "g" else -1
    return torch.stack([uv * zp[..., 1 + sign * dy:1 + sign * dy + h, 1 + sign * dx:1 + sign * dx + w]
                        for dy, dx in _TAP_D])


TAPGRAD_CASES = [((2, 2), 2, 3, 1), ((3, 4), 2, 2, 3), ((17, 65), 2, 3, 2), (STRIDED_HW, STRIDED_B, STRIDED_G, 1)]
TAPGRAD_IDS = [f"{hw[0]}x{hw[1]}-B{b}G{g}Fs{fs}" for hw, b, g, fs in TAPGRAD_CASES]
TapRefs = namedtuple("TapRefs", "u z scale pre gt bound")


@lru_cache(maxsize=None)
def tapgrad_refs(hw, b, g, fs):
    """gt / bound: {(mode, with_scale): [5]}."""
    gen = torch.Generator().manual_seed(7100 + hw[0] + b)
    u, z = (torch.randn((b, g, fs, *hw), generator=gen) for _ in range(2))
    scale, pre = _scales(g, gen), torch.randn(5, generator=gen)
    gt, bound = {}, {}
    for mode in (0, 1):
        for ws in (True, False):
            t = tapgrad_summands(u, z, scale if ws else None, mode).reshape(5, -1)
            gt[mode, ws] = t.sum(1)
            bound[mode, ws] = sum_bound(gt[mode, ws], t, 1)
    return TapRefs(u, z, scale, pre, gt, bound)


def tapgrad_mutant(hw, b, g, fs, mode, ws, m):
    r = tapgrad_refs(hw, b, g, fs)
    t = tapgrad_summands(r.u, r.z, r.scale if ws else None, mode, "g" if m == "g" else None).reshape(5, -1)
    if m == "h":
        t = t.clone()
        t[:, red_first_sweep(t.shape[1]):] = 0.0
    return t.sum(1)


# ---- edge-weight reverse --------------------------------------------------------------------------------------------
EdgeCase = namedtuple("EdgeCase", "window f hw b g offset extra")
# F on both sides of each FMAX boundary (4, 12) and the maximum; offsets 0 and 3 with channels after the slab; frames
# of 3 and 4 pixels along an axis at reach 2; 17 x 20 = 340 pixels: two blocks, the second ragged
EDGE_CASES = [EdgeCase("cross4", 1, (17, 20), 2, 3, 0, 2), EdgeCase("ring3", 4, (2, 5), 2, 2, 3, 1),
              EdgeCase("plus8", 5, (4, 3), 2, 2, 0, 3), EdgeCase("diamond5", 12, (3, 4), 2, 3, 3, 2),
              EdgeCase("round20", 13, (17, 20), 2, 2, 3, 4), EdgeCase("full5", 24, (5, 7), 2, 2, 0, 1),
              EdgeCase("full5", 4, (2, 130), 2, 3, 3, 2)]
STRIDED_EDGE_CASES = [EdgeCase(wn, 3, STRIDED_HW, STRIDED_B, STRIDED_G, 3, 2) for wn in STRIDED_WINDOWS]


def edge_id(c):
    return f"{c.window}-F{c.f}-{c.hw[0]}x{c.hw[1]}-B{c.b}G{c.g}-off{c.offset}"


class _Exp(torch.autograd.Function):
    """exp in float64 from x, rounded once to x's dtype; the backward g y in that dtype."""
    @staticmethod
    def forward(ctx, x):
        y = torch.exp(x.double()).to(x.dtype)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0]


def _div(a, b):
    return (a.double() / b.double()).to(a.dtype)


class _Div(torch.autograd.Function):
    """a / b in float64, rounded once; the backward from g / b (rounded once) and one product."""
    @staticmethod
    def forward(ctx, a, b):
        q = _div(a, b)
        ctx.save_for_backward(q, b)
        return q

    @staticmethod
    def backward(ctx, g):
        q, b = ctx.saved_tensors
        ga = _div(g, b)
        return ga, -(ga * q)


class _InvNorm(torch.autograd.Function):
    """1 / max(sqrt(nrm), 1e-12): the root and the reciprocal each in float64 from an input of nrm's dtype and each
    rounded once (two correctly rounded operations, not one fused); d / d nrm = -inv^3 / 2 off the clamp, 0 on it."""
    @staticmethod
    def forward(ctx, nrm):
        root = torch.sqrt(nrm.double()).to(nrm.dtype)
        inv = (1.0 / root.double().clamp_min(1e-12)).to(nrm.dtype)
        ctx.save_for_backward(inv, root > 1e-12)
        return inv

    @staticmethod
    def backward(ctx, g):
        inv, free = ctx.saved_tensors
        return torch.where(free, g * (-0.5 * inv) * (inv * inv), torch.zeros_like(g))


def _edge_forward(f5, m, delta, reverse=False):
    """w [B,G,K,H,W] of grr_win_edge_weights from f5 [B,G,F,H,W] in f5's dtype, with fh and n = f / |f| kept:
    |f|^2, the dot products and the softmax's sum as chains; sqrt, the reciprocal, exp and the softmax's division
    in float64 and (for fp32 inputs) rounded once (window_ref._edge32), their derivatives again elementwise in
    f5's dtype (_Exp, _Div, _InvNorm): no float64 stretch and no library reduction in the backward either."""
    b, g, f, h, w = f5.shape
    dt = f5.dtype
    chain = list(range(f))[::-1] if reverse else list(range(f))          # reverse: the chains the other way round
    edges = list(range(len(delta)))[::-1] if reverse else list(range(len(delta)))
    nrm = torch.zeros((b, g, h, w), dtype=dt)
    for i in chain:
        nrm = nrm + f5[:, :, i] * f5[:, :, i]
    inv = _InvNorm.apply(nrm)                           # |f| = 0: 1e12, with no gradient through the clamp
    n = f5 * inv[:, :, None]
    fh = n * m[None, :, :, None, None]
    ap = _pad(fh, 2, "replicate")
    sims = []
    for dy, dx in delta:
        nb = _shift(ap, dy, dx, h, w)
        dot = torch.zeros((b, g, h, w), dtype=dt)
        for i in chain:
            dot = dot + fh[:, :, i] * nb[:, :, i]
        sims.append(dot)
    s = torch.stack(sims, 2)
    ex = _Exp.apply(s - s.amax(2, keepdim=True).detach())
    tot = torch.zeros((b, g, h, w), dtype=dt)
    for e in edges:
        tot = tot + ex[:, :, e]
    return torch.stack([_Div.apply(ex[:, :, e], tot) for e in range(len(delta))], 2), fh, n


EdgeRefs = namedtuple("EdgeRefs", "feat multiM w gw_up gfeat_pre gM_pre zero gf64 gM64 bound bound_zero gM_bound "
                      "unproj t_gM")


def _split_zero(gf, zero):
    """(planes with the zero-norm pixel's vector blanked, that vector [F])."""
    zb, zg, zy, zx = zero
    rest = gf.clone()
    rest[zb, zg, :, zy, zx] = 0.0
    return rest, gf[zb, zg, :, zy, zx]


def edge32(f5, m, gw_up, delta, reverse=False):
    """The feature gradient in fp32 by autograd through _edge_forward."""
    f3, m3 = f5.clone().requires_grad_(True), m.clone().requires_grad_(True)
    w3, _, _ = _edge_forward(f3, m3, delta, reverse)
    gf32, _ = torch.autograd.grad((w3 * gw_up).sum(), [f3, m3])
    assert gf32.dtype == torch.float32
    return gf32


def edge_alt32(case):
    """gfeat [B,Ctot,H,W] as a call would leave it whose arithmetic is edge32 with every chain reversed."""
    e = edge_refs(case)
    lo, n = case.offset, case.g * case.f
    f5 = e.feat[:, lo:lo + n].reshape(case.b, case.g, case.f, *case.hw)
    gfeat = e.gfeat_pre.clone()
    gfeat[:, lo:lo + n] += edge32(f5, e.multiM, e.gw_up, delta_of(case.window), True).reshape(case.b, n, *case.hw)
    return gfeat


@lru_cache(maxsize=None)
def edge_refs(case):
    """feat [B, offset + G F + extra, H, W] with one all-zero feature vector (image 0, graph 0, pixel (H - 1, 0)); w
    the forward's fp32 weights (the float64 oracle's, rounded); gw_up the upstream gradient the call consumes."""
    delta = delta_of(case.window)
    k = len(delta)
    gen = torch.Generator().manual_seed(7300 + case.f + k + case.hw[1])
    h, w = case.hw
    b, g, f = case.b, case.g, case.f
    ctot = case.offset + g * f + case.extra
    feat = torch.randn((b, ctot, h, w), generator=gen)
    zero = (0, 0, h - 1, 0)
    feat[0, case.offset:case.offset + f, h - 1, 0] = 0.0
    m = (0.5 + torch.rand((g, f), generator=gen)).contiguous()
    gw_up = torch.randn((b, g, k, h, w), generator=gen)
    gfeat_pre, gM_pre = torch.randn((b, ctot, h, w), generator=gen), torch.randn((g, f), generator=gen)
    f5 = feat[:, case.offset:case.offset + g * f].reshape(b, g, f, h, w)
    # float64: the oracle under autograd
    fr, mr = f5.double().requires_grad_(True), m.double().requires_grad_(True)
    w64, _ = O.edge_weights(fr, mr, np.asarray(delta))
    gf64, gM64 = torch.autograd.grad((w64 * gw_up.double()).sum(), [fr, mr])
    # float64 again from the slice-wise forward, for the summands of gM and the un-projected scale
    fe, me = f5.double().requires_grad_(True), m.double().requires_grad_(True)
    we, fh, n = _edge_forward(fe, me, delta)
    fh.retain_grad()
    (we * gw_up.double()).sum().backward()
    assert float((fe.grad - gf64).abs().max()) <= 1e-9 * float(gf64.abs().max())
    t_gM = (fh.grad * n.detach())                                       # [B,G,F,H,W]
    norm = f5.double().pow(2).sum(2, keepdim=True).sqrt()
    gn = (fh.grad * me.detach()[None, :, :, None, None]).abs()
    unproj = float((gn / norm.clamp_min(1e-12))[(norm > 0).expand_as(gn)].max())
    gf32 = edge32(f5, m, gw_up, delta)
    r64, z64 = _split_zero(gf64, zero)
    r32, z32 = _split_zero(gf32, zero)
    bound = bound_of(plane_err(r32, r64))
    bound_zero = bound_of((z32.double() - z64).abs().max() / z64.abs().max().clamp_min(1e-300))
    return EdgeRefs(feat, m, w64.detach().float().contiguous(), gw_up, gfeat_pre, gM_pre, zero, gf64, gM64, bound,
                    bound_zero, sum_bound(gM64, t_gM, (0, 3, 4)), unproj, t_gM)


def edge_ratios(case, gfeat, gM):
    """gfeat [B,Ctot,H,W] and gM [G,F] after the call (both pre-filled) -> worst err / bound: the slab's planes off
    the zero-norm pixel, that pixel's vector, gM; 'outside' is 0.0 exactly when every channel outside the slab came
    back bitwise unchanged; 'unproj': the slab's error over 2e-5 of the un-projected scale.  At F = 1 'gfeat' is left
    out: the gradient off the zero-norm pixel is identically zero, max |ref64| and err32 are both rounding noise and
    their quotient decides nothing either way; 'unproj' holds that case."""
    e = edge_refs(case)
    b, g, f = case.b, case.g, case.f
    h, w = case.hw
    lo, hi = case.offset, case.offset + g * f
    got = gfeat.detach().cpu()
    outside = torch.ones(got.shape[1], dtype=torch.bool)
    outside[lo:hi] = False
    same = torch.equal(got[:, outside], e.gfeat_pre[:, outside])
    g5 = got[:, lo:hi].reshape(b, g, f, h, w).double()
    p5 = e.gfeat_pre[:, lo:hi].reshape(b, g, f, h, w).double()
    rest_g, zero_g = _split_zero(g5, e.zero)
    rest_p, zero_p = _split_zero(p5, e.zero)
    rest_r, zero_r = _split_zero(e.gf64, e.zero)
    zs = zero_r.abs().max().clamp_min(1e-300)
    zerr = (zero_g - (zero_p + zero_r)).abs().max() / zs
    out = {} if f == 1 else {"gfeat": ratio_acc(rest_g, rest_p, rest_r, e.bound, (-2, -1))}
    return {**out, "gfeat_zero": float(zerr / (e.bound_zero + EPS32 * (zero_p + zero_r).abs().max() / zs)),
            "gM": sum_ratio(gM, e.gM_pre, e.gM64, e.gM_bound),
            "unproj": float((rest_g - (rest_p + rest_r)).abs().max()) / (STOL * max(e.unproj, 1e-300)),
            "outside": 0.0 if same else float("inf")}


def edge_mutant_h(case):
    """(gfeat, gM) as the call would leave them with the second sweep's pixels lost (mutant h)."""
    e = edge_refs(case)
    h, w = case.hw
    keep = torch.zeros(h * w, dtype=torch.float64)
    keep[:first_sweep(case.hw, case.b * case.g)] = 1.0
    keep = keep.reshape(h, w)
    gfeat = e.gfeat_pre.double().clone()
    lo = case.offset
    gfeat[:, lo:lo + case.g * case.f] += (e.gf64 * keep).reshape(case.b, -1, h, w)
    return gfeat, e.gM_pre.double() + (e.t_gM * keep).sum((0, 3, 4))


# ---- mix ---------------------------------------------------------------------------------------------------------------
MIX_CASES = [(1, (2, 2), 2), (2, (17, 20), 3), (3, (16, 16), 5)]
MixRefs = namedtuple("MixRefs", "gout x score gx64 gscore64 bound_gx bound_gscore")


@lru_cache(maxsize=None)
def mix_refs(fs, hw, g):
    gen = torch.Generator().manual_seed(7500 + fs + hw[0])
    x = torch.randn((2, g, fs, *hw), generator=gen)
    score = torch.softmax(torch.randn((2, g, *hw), generator=gen), dim=1)
    gout = torch.randn((2, fs, *hw), generator=gen)
    gx64 = gout.double()[:, None] * score.double()[:, :, None]
    gscore64 = (gout.double()[:, None] * x.double()).sum(2)
    gx32 = gout[:, None] * score[:, :, None]
    gs32 = torch.zeros_like(score)
    for c in range(fs):
        gs32 = gs32 + gout[:, None, c] * x[:, :, c]
    return MixRefs(gout, x, score, gx64, gscore64, bound_of(plane_err(gx32, gx64)),
                   bound_of(plane_err(gs32, gscore64)))
