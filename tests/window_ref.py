"""References, the fp32-class bound, the case table and emulated mutants of the window-graph forward kernels
(csrc/window_ops.hip: win_solver_kernel, win_pair_weights_kernel, win_edge_weights_kernel, win_mix_kernel).
tests/test_window_ref.py checks all of this on the CPU, tests/test_gpu_window_kernels.py runs the kernels against
it.  Modelled on tests/lnb_ref.py and tests/gemm_ref.py.  Nothing here imports or touches a kernel.

The solver kernel is one template  win_solver_kernel<R, MODE, KT, PAIR>  dispatched on (reach, K):

    family   R  KT   windows here
    r1k8     1   8   ring3
    r1k0     1   0   cross4 (K = 4)                  runtime K
    r2k12    2  12   diamond5
    r2k24    2  24   full5
    r2k0     2   0   plus8 (K = 8: reach 2, so not <1, ., 8>), round20 (K = 20)      runtime K

``ref64(case)`` is the op of the case in float64 from the oracle's blocks (oracle/window_oracle.py: stats_conv,
glr_apply, gtv_C, soft_threshold, gtv_Ct, stats_conv_t), following include/grr.h:

    op     mode  what
    0      0     CG step with u_prev: out = x + alpha u, u = (y - A x) + beta u_prev          (out and u)
    0nou   0     the same, u_prev absent
    1      1     rhs  ro S^T C^T C S x + y, x per graph          1rep   x [B,Fs,H,W] shared by the graphs
    2      2     prox rhs, phi = 2 soft - t                      2rep   the same with the shared x
    3L     3     mu S^T (I - W) S x       3G   ro S^T C^T C S x      3LG   both      3LG1   both, mu and ro absent (= 1)
    4 5 7  4 5 7 ops 0, 1, 3LG on the pair weights of the same w_G: the same references

``ref32(case)`` is the same op in fp32 with the same bits on every host: only elementwise fp32 adds, subtracts and
multiplies on shifted slices (each correctly rounded, none fused), the five taps of S in the kernel's order
(centre, up, left, right, down), the edge sums in edge order, the scatter subtracted edge by edge after them;
exp and the division of the softmax are evaluated in float64 from their fp32 inputs and rounded once.  No library
convolution, einsum or reduction is used (gemm_ref.py records that the library's fp32 convolution differs between
hosts).  ``alt32`` is a second honest fp32 evaluation in another summation order, the pair formulation
c_e (s - s_n) of ops 0, 1 and 3: a case whose alt32 left the bound would be ill-conditioned, not a kernel's fault.

    bound = 4 err32 + 1e-7   (gemm_ref.fp32_class_bound) per output plane (b, g, c), err = max |d| / max |ref64| over
    the plane; per (b, g) for edge and pair weights, per (b, c) for the mix.

No bound is fitted to a kernel's output.

Inputs: x, y, u_prev ~ randn (every pixel of a plane at the plane's scale: the per-plane max-norm sees a localized
error); weights softmax(2 randn) over K; taps from four distinct stencil parameters, different for L and G; mu, ro,
alpha, beta per graph and distinct, graph 1 with a small mu and ro; for mode 2 gamma[g] is a quantile (0.35 / 0.5 /
0.65) of the graph's nonzero |C S x| so that every branch of the soft threshold holds >= 5 % of every plane's
edges (branch_fractions; asserted by tests/test_window_ref.py).  One seed per case.

Shapes (tile 16 x 64, halo R + 2): 2 x 2 (reach exceeds the frame), 3 x 2 and 2 x 5 (the clamp folds), 16 x 64 (one
exact tile), 17 x 65 (2 x 2 tiles, the last row and column one pixel), 33 x 130 (3 x 3 tiles, seams inside the halo).

Mutants (``mutant64``), float64 evaluations with one thing wrong, none touching a kernel:
    a  S reads a replicate frame instead of the reflect frame along the top border only
    b  the C^T scatter folds what lands outside the frame back onto it (clamp) instead of dropping it.  It does
       not apply to cross4: an axis edge of reach 1 that leaves the frame clamps onto its own pixel, its difference
       s(p) - s(p) is exactly 0 in every mode, and nothing lands outside (has_outside_scatter)
    c  edge K // 2 left out of the L / C sums in the tile-seam column x = 63 (W >= 65; K // 2 is the edge (0, 1) or
       (0, 2), whose neighbour lies across the seam)
    d  Fs = 2: the last real channel's s replaced by channel Fs - 2's (min(c, Fs - 1) gone wrong)
    e  mode 2: soft in place of 2 soft - t at edges with gamma < |t| <= 1.1 gamma
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np
import torch
import torch.nn.functional as F

from oracle import window_oracle as O

TILE_H, TILE_W = 16, 64
SEAM_COL = 63          # the last column of the first tile; its right neighbours lie in the next tile at W >= 65

WINDOWS = {
    "ring3": np.array([1, 1, 1, 1, 0, 1, 1, 1, 1]).reshape(3, 3),
    "cross4": np.array([0, 1, 0, 1, 0, 1, 0, 1, 0]).reshape(3, 3),
    "diamond5": np.array([0, 0, 1, 0, 0, 0, 1, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 1, 0, 0, 0, 1, 0, 0]).reshape(5, 5),
    "full5": np.array([1] * 12 + [0] + [1] * 12).reshape(5, 5),
    "plus8": np.array([0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 1, 1, 0, 1, 1, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0]).reshape(5, 5),
    "round20": np.array([0, 1, 1, 1, 0] + [1] * 5 + [1, 1, 0, 1, 1] + [1] * 5 + [0, 1, 1, 1, 0]).reshape(5, 5),
}
FAMILIES = ("r1k8", "r1k0", "r2k12", "r2k24", "r2k0")
SHAPES = ((2, 2), (3, 2), (2, 5), (16, 64), (17, 65), (33, 130))
OPS = ("0", "0nou", "1", "1rep", "2", "2rep", "3L", "3G", "3LG", "3LG1", "4", "5", "7")
REQUIRED_OPS = tuple(o for o in OPS if o != "3LG1")
# op -> (solver mode, pair)
MODE = {"0": (0, False), "0nou": (0, False), "1": (1, False), "1rep": (1, False), "2": (2, False), "2rep": (2, False),
        "3L": (3, False), "3G": (3, False), "3LG": (3, False), "3LG1": (3, False), "4": (0, True), "5": (1, True),
        "7": (3, True)}
MUTANTS = ("a", "b", "c", "d", "e")


def delta_of(window):
    return tuple((int(a), int(b)) for a, b in O.window_edges(WINDOWS[window]))


def family(window):
    """The win_solver_kernel<R, ., KT> instance grr_win_solver dispatches the window to."""
    d = delta_of(window)
    reach = max(max(abs(a), abs(b)) for a, b in d)
    k = len(d)
    kt = (k if k == 8 else 0) if reach <= 1 else (k if k in (12, 24) else 0)
    return f"r{max(reach, 1)}k{kt}"


Case = namedtuple("Case", "window op fs hw g seed")

# op -> shape, two assignments that the windows alternate between.  Not the full product: every family meets every
# op, every shape and every Fs (tests/test_window_ref.py asserts that from CASES).  The mode 2 ops stay off the
# frames of fewer than ten pixels, where a plane has too few edges for each soft-threshold branch to hold 5 %.
_SHAPE_OF = (
    {"0": (17, 65), "0nou": (2, 2), "1": (3, 2), "1rep": (16, 64), "2": (33, 130), "2rep": (2, 5), "3L": (2, 5),
     "3G": (33, 130), "3LG": (17, 65), "3LG1": (3, 2), "4": (2, 2), "5": (33, 130), "7": (16, 64)},
    {"0": (33, 130), "0nou": (3, 2), "1": (2, 2), "1rep": (17, 65), "2": (17, 65), "2rep": (2, 5), "3L": (16, 64),
     "3G": (2, 5), "3LG": (33, 130), "3LG1": (2, 2), "4": (17, 65), "5": (3, 2), "7": (2, 5)},
)


def _cases():
    out = []
    for wi, window in enumerate(WINDOWS):
        for i, op in enumerate(OPS):
            out.append(Case(window, op, 1 + (i + wi) % 3, _SHAPE_OF[wi % 2][op], 2 + (i + wi) % 2, 4000 + 100 * wi + i))
    return out


CASES = _cases()


def case_id(c):
    return f"{c.window}-op{c.op}-Fs{c.fs}-{c.hw[0]}x{c.hw[1]}-G{c.g}"


IDS = [case_id(c) for c in CASES]
# (mutant, case id) -> why the case cannot show the mutant; at most one per mutant, none for a and b
MUTANT_EXEMPT = {}


# ---- inputs ------------------------------------------------------------------------------------------------
def taps_of(p01, p02a, p02b, p03):
    """(centre, up, left, right, down) of the stats stencil, the expression of kernels.win_taps in fp32."""
    return torch.stack([p01 - p02a - p02b + 4.0 * p03, -p03, -p03, p02a - p03, p02b - p03]).float().contiguous()


def kernel33(taps, fs):
    """The oracle's [Fs, 1, 3, 3] stencil of five taps (stats_conv correlates: 'up' multiplies x(p - row))."""
    k = torch.zeros(3, 3, dtype=taps.dtype)
    k[1, 1], k[0, 1], k[1, 0], k[1, 2], k[2, 1] = taps
    return k.expand(fs, 1, 3, 3)


def _softmax_weights(shape, gen):
    return torch.softmax(2.0 * torch.randn(shape, generator=gen, dtype=torch.float64), dim=2).float()


Inputs = namedtuple("Inputs", "x y u_prev wL wG tapsL tapsG mu ro alpha beta log_gamma delta")


@lru_cache(maxsize=None)
def inputs(case):
    """fp32 CPU tensors of the case (None where the op has no such operand)."""
    mode, _ = MODE[case.op]
    gen = torch.Generator().manual_seed(case.seed)
    b, g, fs = 2, case.g, case.fs
    h, w = case.hw
    delta = delta_of(case.window)
    k = len(delta)
    rep = case.op.endswith("rep")
    x = torch.randn((b, fs, h, w) if rep else (b, g, fs, h, w), generator=gen)
    y = torch.randn((b, g, fs, h, w) if mode == 0 else (b, fs, h, w), generator=gen) if mode != 3 else None
    u_prev = torch.randn((b, g, fs, h, w), generator=gen) if case.op in ("0", "4") else None
    wL = _softmax_weights((b, g, k, h, w), gen) if case.op not in ("1", "1rep", "2", "2rep", "3G", "5") else None
    wG = _softmax_weights((b, g, k, h, w), gen) if case.op != "3L" else None
    st = 0.05 * torch.rand(8, generator=gen)
    tapsL = taps_of(0.9 + st[0], 0.3 + st[1], 0.5 + st[2], 0.2 + st[3])
    tapsG = taps_of(1.1 + st[4], 0.6 + st[5], 0.25 + st[6], 0.35 + st[7])
    jit = 0.02 * torch.rand((4, g), generator=gen)
    mu = (torch.tensor([0.45, 0.04, 0.7])[:g] + jit[0]).contiguous()
    ro = (torch.tensor([0.6, 0.05, 0.3])[:g] + jit[1]).contiguous()
    alpha = (torch.tensor([0.5, 0.8, 0.25])[:g] + jit[2]).contiguous()
    beta = (torch.tensor([0.3, 0.1, 0.45])[:g] + jit[3]).contiguous()
    if case.op == "3LG1":
        mu = ro = None
    log_gamma = None
    if mode == 2:
        x5 = (x[:, None].expand(b, g, fs, h, w) if rep else x).double()
        t = O.gtv_C(x5, wG.double(), kernel33(tapsG.double(), fs), np.asarray(delta)).abs()
        gam = []
        for gi in range(g):
            tg = t[:, gi].reshape(-1)
            gam.append(torch.quantile(tg[tg > 0], (0.35, 0.5, 0.65)[gi]))
        log_gamma = torch.log(torch.stack(gam)).float().contiguous()
    return Inputs(x, y, u_prev, wL, wG, tapsL, tapsG, mu, ro, alpha, beta, log_gamma, delta)


def _x5(inp, case, dtype):
    x = inp.x.to(dtype)
    if x.dim() == 4:
        b, fs, h, w = x.shape
        x = x[:, None].expand(b, case.g, fs, h, w)
    return x


# ---- float64 from the oracle's blocks ---------------------------------------------------------------------------
def _bc(v):
    return v[None, :, None, None, None]


def _ref64(case):
    inp = inputs(case)
    mode, _ = MODE[case.op]
    d = torch.float64
    dl = np.asarray(inp.delta)
    x = _x5(inp, case, d)
    kG, kL = kernel33(inp.tapsG.double(), case.fs), kernel33(inp.tapsL.double(), case.fs)
    one = torch.ones(case.g, dtype=d)
    mu = inp.mu.double() if inp.mu is not None else one
    ro = inp.ro.double() if inp.ro is not None else one

    def gtv(phi=None):
        e = O.gtv_C(x, inp.wG.double(), kG, dl)
        if phi:
            eps = O.soft_threshold(e, torch.exp(inp.log_gamma.double()))
            e = eps - (e - eps)
        return O.gtv_Ct(e, inp.wG.double(), kG, dl)

    if mode == 0:
        ax = x + O.glr_apply(x, inp.wL.double(), kL, dl) * _bc(mu) + gtv() * _bc(ro)
        u = inp.y.double() - ax
        if inp.u_prev is not None:
            u = u + _bc(inp.beta.double()) * inp.u_prev.double()
        return {"out": x + _bc(inp.alpha.double()) * u, "u": u}
    if mode in (1, 2):
        return {"out": gtv(mode == 2) * _bc(ro) + inp.y.double()[:, None]}
    out = 0.0
    if inp.wL is not None:
        out = O.glr_apply(x, inp.wL.double(), kL, dl) * _bc(mu)
    if inp.wG is not None:
        out = out + gtv() * _bc(ro)
    return {"out": out}


# ---- the same from elementwise ops on shifted slices (fp32: ref32, alt32; float64: the mutants) ---------------------
def _pad(t, n, mode):
    sh = t.shape
    return F.pad(t.reshape(1, -1, sh[-2], sh[-1]), (n, n, n, n), mode=mode).reshape(*sh[:-2], sh[-2] + 2 * n,
                                                                                    sh[-1] + 2 * n)


def _shift(p2, dy, dx, h, w):
    return p2[..., 2 + dy:2 + dy + h, 2 + dx:2 + dx + w]


def _S(x, t, replicate_top=False):
    xp = _pad(x, 1, "reflect").clone()
    if replicate_top:
        xp[..., 0, :] = xp[..., 1, :]
    v = t[0] * xp[..., 1:-1, 1:-1]
    v = v + t[1] * xp[..., :-2, 1:-1]
    v = v + t[2] * xp[..., 1:-1, :-2]
    v = v + t[3] * xp[..., 1:-1, 2:]
    return v + t[4] * xp[..., 2:, 1:-1]


def _St(v, t):
    vp = _pad(v, 1, "constant")
    o = t[0] * vp[..., 1:-1, 1:-1]
    o = o + t[1] * vp[..., 2:, 1:-1]          # the up tap's contributions come from the row below
    o = o + t[2] * vp[..., 1:-1, 2:]
    o = o + t[3] * vp[..., 1:-1, :-2]
    return o + t[4] * vp[..., :-2, 1:-1]


def _slices(dy, dx, h, w):
    """(source p, destination q = p + d) index pairs of the positions whose neighbour lies inside the frame."""
    src = (slice(max(0, -dy), h - max(0, dy)), slice(max(0, -dx), w - max(0, dx)))
    dst = (slice(max(0, dy), h - max(0, -dy)), slice(max(0, dx), w - max(0, -dx)))
    return src, dst


def pair_weights(w, delta):
    """c_e(q) = w_e(q)^2 + [q + d_e inside] w_e'(q + d_e)^2 in w's dtype (float64: the reference of
    grr_win_pair_weights; fp32: two products and an add)."""
    h, ww = w.shape[-2:]
    c = w * w
    for e, (dy, dx) in enumerate(delta):
        o = delta.index((-dy, -dx))
        src, dst = _slices(dy, dx, h, ww)
        sq = w[:, :, o] * w[:, :, o]
        c[:, :, e][..., src[0], src[1]] = c[:, :, e][..., src[0], src[1]] + sq[..., dst[0], dst[1]]
    return c


def _soft(t, gm):
    z = torch.zeros_like(t)
    return torch.where(t < -gm, t + gm, z) + torch.where(t > gm, t - gm, z)


def _evaluate(case, dtype, mutant=None, pair=False):
    inp = inputs(case)
    mode, _ = MODE[case.op]
    h, w = case.hw
    delta = inp.delta
    k = len(delta)
    x = _x5(inp, case, dtype)
    tG, tL = inp.tapsG.to(dtype), inp.tapsL.to(dtype)
    colmask = None
    if mutant == "c":
        colmask = torch.ones(w, dtype=dtype)
        colmask[SEAM_COL] = 0.0
    gm = None
    if mode == 2:       # expf of the kernel: exp in float64 from the fp32 log_gamma, rounded once
        gm = _bc(torch.exp(inp.log_gamma.double()).to(dtype))

    def phi(t):
        if mode != 2:
            return t
        eps = _soft(t, gm)
        full = eps - (t - eps)
        if mutant == "e":
            near = (t.abs() > gm) & (t.abs() <= 1.1 * gm)
            return torch.where(near, eps, full)
        return full

    def s_of(t):
        s = _S(x, t, replicate_top=mutant == "a")
        if mutant == "d":
            s = s.clone()
            s[:, :, case.fs - 1] = s[:, :, case.fs - 2]
        return s

    tg = tl = None
    if inp.wG is not None:
        s = s_of(tG)
        sp = _pad(s, 2, "replicate")
        wG = inp.wG.to(dtype)
        acc = torch.zeros_like(s)
        if pair:
            c = pair_weights(wG, delta)
            for e, (dy, dx) in enumerate(delta):
                acc = acc + c[:, :, e][:, :, None] * (s - _shift(sp, dy, dx, h, w))
        else:
            zs = []
            for e, (dy, dx) in enumerate(delta):
                we = wG[:, :, e][:, :, None]
                z = phi(we * s - we * _shift(sp, dy, dx, h, w)) * we
                zs.append(z)
                acc = acc + (z * colmask if colmask is not None and e == k // 2 else z)
            if mutant == "b":
                buf = torch.zeros((*s.shape[:-2], h + 4, w + 4), dtype=dtype)
                for (dy, dx), z in zip(delta, zs):
                    buf[..., 2 + dy:2 + dy + h, 2 + dx:2 + dx + w] -= z
                buf[..., 2, :] += buf[..., 0, :] + buf[..., 1, :]
                buf[..., h + 1, :] += buf[..., h + 2, :] + buf[..., h + 3, :]
                buf[..., :, 2] += buf[..., :, 0] + buf[..., :, 1]
                buf[..., :, w + 1] += buf[..., :, w + 2] + buf[..., :, w + 3]
                acc = acc + buf[..., 2:2 + h, 2:2 + w]
            else:
                acc = acc.clone()
                for (dy, dx), z in zip(delta, zs):
                    src, dst = _slices(dy, dx, h, w)
                    acc[..., dst[0], dst[1]] = acc[..., dst[0], dst[1]] - z[..., src[0], src[1]]
        tg = _St(acc, tG)
    if inp.wL is not None:
        s = s_of(tL)
        sp = _pad(s, 2, "replicate")
        wL = inp.wL.to(dtype)
        wx = torch.zeros_like(s)
        for e, (dy, dx) in enumerate(delta):
            term = wL[:, :, e][:, :, None] * _shift(sp, dy, dx, h, w)
            wx = wx + (term * colmask if colmask is not None and e == k // 2 else term)
        tl = _St(s - wx, tL)

    one = torch.ones(case.g, dtype=dtype)
    mu = _bc(inp.mu.to(dtype) if inp.mu is not None else one)
    ro = _bc(inp.ro.to(dtype) if inp.ro is not None else one)
    if mode == 0:
        ax = (x + tl * mu) + tg * ro
        u = inp.y.to(dtype) - ax
        if inp.u_prev is not None:
            u = u + _bc(inp.beta.to(dtype)) * inp.u_prev.to(dtype)
        return {"out": x + _bc(inp.alpha.to(dtype)) * u, "u": u}
    if mode in (1, 2):
        return {"out": tg * ro + inp.y.to(dtype)[:, None]}
    if tl is not None and tg is not None:
        return {"out": tl * mu + tg * ro}
    return {"out": tl * mu if tl is not None else tg * ro}


def has_outside_scatter(window):
    """Whether an edge that leaves the frame can carry a nonzero difference: its clamped neighbour is another pixel
    (a diagonal edge, or one of reach 2 from the second row or column)."""
    return any((dy and dx) or max(abs(dy), abs(dx)) > 1 for dy, dx in delta_of(window))


def mutant_applies(case, m):
    mode, _ = MODE[case.op]
    return {"a": True, "b": case.op != "3L" and has_outside_scatter(case.window), "c": case.hw[1] > SEAM_COL + 1,
            "d": case.fs == 2, "e": mode == 2}[m]


def mutant64(case, m):
    assert mutant_applies(case, m)
    return _evaluate(case, torch.float64, mutant=m)


def branch_fractions(case):
    """[planes, 3]: the share of a (b, g, c) plane's K H W edges with t < -gamma, |t| <= gamma, t > gamma (mode 2)."""
    inp = inputs(case)
    x = _x5(inp, case, torch.float64)
    t = O.gtv_C(x, inp.wG.double(), kernel33(inp.tapsG.double(), case.fs), np.asarray(inp.delta))
    gm = torch.exp(inp.log_gamma.double())[None, :, None, None, None, None]
    fr = torch.stack([(t < -gm), (t.abs() <= gm), (t > gm)], -1).double().mean((3, 4, 5))
    return fr.reshape(-1, 3)


# ---- measures and the bound ---------------------------------------------------------------------------------
def plane_err(got, ref64, dims=(-2, -1)):
    """max |got - ref64| / max |ref64| over dims, one figure per remaining index (a plane of zeros: by 1e-300)."""
    d = (got.detach().double().cpu() - ref64).abs()
    return d.amax(dims) / ref64.abs().amax(dims).clamp_min(1e-300)


def bound_of(err32):
    return 4.0 * err32 + 1e-7          # gemm_ref.fp32_class_bound, per plane


def whole_err(got, ref64):
    """What the older tests measure: max-norm over the whole tensor."""
    return float((got.detach().double().cpu() - ref64).abs().max()) / max(float(ref64.abs().max()), 1e-300)


Refs = namedtuple("Refs", "inp out64 out32 err32 bound")


@lru_cache(maxsize=None)
def refs(case):
    """float64 and fp32 outputs of the case ({"out": ..., "u": ... for mode 0}), err32 and the bound per plane."""
    out64 = _ref64(case)
    out32 = _evaluate(case, torch.float32)
    assert all(v.dtype == torch.float32 for v in out32.values())
    err32 = {n: plane_err(out32[n], out64[n]) for n in out64}
    return Refs(inputs(case), out64, out32, err32, {n: bound_of(e) for n, e in err32.items()})


def ratio(got, r, name="out"):
    """The worst err / bound over the planes of output ``name``."""
    return float((plane_err(got, r.out64[name]) / r.bound[name]).max())


def eval64(case):
    return _evaluate(case, torch.float64)


def alt32(case):
    """The pair formulation in fp32 (ops of modes 0, 1, 3 with a GTV term), else None."""
    mode, _ = MODE[case.op]
    if mode == 2 or inputs(case).wG is None:
        return None
    return _evaluate(case, torch.float32, pair=True)


# ---- pair weights, edge weights, mix ------------------------------------------------------------------------------
PairRefs = namedtuple("PairRefs", "w c64 c32 bound")


@lru_cache(maxsize=None)
def pair_refs(window, hw=(17, 65), g=3, seed=4900):
    delta = delta_of(window)
    gen = torch.Generator().manual_seed(seed + len(delta))
    w = _softmax_weights((2, g, len(delta), *hw), gen)
    c64, c32 = pair_weights(w.double(), delta), pair_weights(w, delta)
    return PairRefs(w, c64, c32, bound_of(plane_err(c32, c64, (-3, -2, -1))))


EdgeCase = namedtuple("EdgeCase", "window f hw g offset extra")
# F on both sides of each FMAX boundary (4, 12) and the maximum; 17 x 20 = 340 pixels: two blocks of 256, the
# second ragged.  One case reads its slab at channel 5 of G F + 9 channels (feat_bstride > G F H W).
EDGE_CASES = [EdgeCase("cross4", 1, (17, 20), 3, 0, 0), EdgeCase("ring3", 4, (2, 5), 2, 0, 0),
              EdgeCase("plus8", 5, (17, 20), 2, 5, 9), EdgeCase("diamond5", 12, (3, 2), 3, 0, 0),
              EdgeCase("round20", 13, (17, 20), 2, 0, 0), EdgeCase("full5", 24, (17, 20), 2, 0, 0),
              EdgeCase("ring3", 24, (2, 2), 3, 0, 0)]
EDGE_IDS = [f"{c.window}-F{c.f}-{c.hw[0]}x{c.hw[1]}" + (f"-off{c.offset}" if c.offset else "") for c in EDGE_CASES]
EdgeRefs = namedtuple("EdgeRefs", "feat multiM zero w64 deg64 w32 deg32 bound_w bound_deg")


def _edge32(f5, m, delta):
    """grr_win_edge_weights in fp32: |f|^2 and the dot products as chains over F, sqrt, the reciprocal, exp and the
    softmax's division in float64 from their fp32 inputs, rounded once."""
    b, g, f, h, w = f5.shape
    nrm = torch.zeros((b, g, h, w))
    for i in range(f):
        nrm = nrm + f5[:, :, i] * f5[:, :, i]
    inv = (1.0 / torch.sqrt(nrm.double()).clamp_min(1e-12)).float()
    a = (f5 * inv[:, :, None]) * m[None, :, :, None, None]
    ap = _pad(a, 2, "replicate")
    sims = []
    for dy, dx in delta:
        nb = _shift(ap, dy, dx, h, w)
        dot = torch.zeros((b, g, h, w))
        for i in range(f):
            dot = dot + a[:, :, i] * nb[:, :, i]
        sims.append(dot)
    s = torch.stack(sims, 2)
    ex = torch.exp((s - s.amax(2, keepdim=True)).double()).float()
    tot = torch.zeros((b, g, h, w))
    for e in range(len(delta)):
        tot = tot + ex[:, :, e]
    wt = (ex.double() / tot.double()[:, :, None]).float()
    deg = torch.zeros((b, g, h, w))
    for e in range(len(delta)):
        deg = deg + wt[:, :, e]
    return wt, deg


@lru_cache(maxsize=None)
def edge_refs(case):
    """feat [2, G F + extra, H, W] with one all-zero feature vector per image and graph slab (the max(|f|, 1e-12)
    branch: f^ = 0 there, every similarity 0, uniform weights 1 / K)."""
    delta = delta_of(case.window)
    gen = torch.Generator().manual_seed(4700 + case.f + len(delta))
    h, w = case.hw
    g, f = case.g, case.f
    feat = torch.randn((2, g * f + case.extra, h, w), generator=gen)
    zero = [(h - 1, 0), (0, w - 1)]
    for b, (zy, zx) in enumerate(zero):
        feat[b, :, zy, zx] = 0.0
    m = (0.5 + torch.rand((g, f), generator=gen)).contiguous()
    f5 = feat[:, case.offset:case.offset + g * f].reshape(2, g, f, h, w)
    w64, deg64 = O.edge_weights(f5.double(), m.double(), np.asarray(delta))
    w32, deg32 = _edge32(f5, m, delta)
    return EdgeRefs(feat, m, zero, w64, deg64, w32, deg32, bound_of(plane_err(w32, w64, (-3, -2, -1))),
                    bound_of(plane_err(deg32, deg64)))


MixRefs = namedtuple("MixRefs", "x score dc out64 bound")


@lru_cache(maxsize=None)
def mix_refs(fs, hw, g, with_dc):
    gen = torch.Generator().manual_seed(4800 + fs + hw[0])
    x = torch.randn((2, g, fs, *hw), generator=gen)
    score = torch.softmax(torch.randn((2, g, *hw), generator=gen), dim=1)
    dc = torch.randn((2, fs, *hw), generator=gen) if with_dc else None
    out64 = torch.einsum("bgchw, bghw -> bchw", x.double(), score.double())
    out32 = torch.zeros((2, fs, *hw))
    for gi in range(g):
        out32 = out32 + x[:, gi] * score[:, gi, None]
    if with_dc:
        out64, out32 = out64 + dc.double(), out32 + dc
    return MixRefs(x, score, dc, out64, bound_of(plane_err(out32, out64)))


MIX_CASES = [(1, (2, 2), 2, False), (2, (17, 20), 3, True), (3, (16, 16), 5, True)]
