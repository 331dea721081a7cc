"""References, the fp32-class bound, emulated split-bf16 mutants and the case tables of the GEMM-class kernels
(tests/test_gemm_ref.py checks them on the CPU, tests/test_gpu_gemm_class.py runs the kernels against them).

Every op here is bilinear in two fp32 operands (a, b).  ``OPS[name].f(a, b)`` evaluates it with the library's
operators (in float64: the reference), ``F32[name](a, b)`` is the CPU's plain fp32 evaluation in a fixed order
(dot32: an fma chain per output, as a CPU GEMM runs it), whose error defines the bound

    fp32_class_bound(ref64, ref32) = 4 rel_err(ref32, ref64) + 1e-7

(test_x3_gemm_is_fp32_accurate's, fp32_class in tests/test_gpu_codec.py).  The hot kernels split each operand
exactly into three bf16 terms v = v0 + v1 + v2 (RNE) and accumulate the six products a_i b_j with i + j <= 2.
``split3`` does the same split on the CPU and ``emulate`` sums a chosen subset of the products in float64, so
the error a kernel would make by dropping products is known from the inputs alone:

    SIX      every product the kernels keep: the split itself, far inside the bound
    DROP11   the smallest kept product (a_1 b_1) left out
    KEEP3    only a_0 b_0, a_0 b_1, a_1 b_0 kept

The structural mutants (``structural``) leave out one pixel, one k row, or the last 16-pixel step of one chunk
of the weight-gradient reduction.  None of this touches the kernels.

Case notes name the dispatch edge a case reaches, in the words of launch_x3 / launch_x3k / launch_gemm
(csrc/feature_ops.hip), wgrad_plan (csrc/wgrad_ops.hip) and cd_grid (csrc/codec_ops.hip):
  x3    K <= 128: gemm_x3_kernel<KS>, KS = ceil(K / 16) k-steps held in registers; nch = ceil(M / 32) row chunks;
        tiles = ceil(P / 256) pixel tiles of 8 waves x 32 pixels
  x3k   K > 128: gemm_x3k_kernel<TM>, TM = min(4, ceil(M / 32)) row groups per workgroup, nmt = ceil(groups / TM)
        M tiles; KS k-steps streamed two per ring chunk (an odd KS ends on a single k-step)
  f32   gemm_f32_kernel: 128 x 128 block tiles, k-chunks of 16; vec = K % 4 == 0 and P % 4 == 0 (and aligned
        pointers), else the scalar staging and epilogue
  wgrad wave tile 128x96 / 192x64 / 64x96, operands swapped or not, CP pixels per chunk, cpi chunks per image;
        a chunk runs ns = len // 16 full steps two per loop trip (an odd ns ends on the single `if (i < ns)` step)
        and a guarded tail of len % 16 pixels
"""
from collections import namedtuple
from functools import lru_cache

import torch
import torch.nn.functional as F

from tests.test_gpu_parity import rand, rel_err

SIX = ((0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0))
DROP11 = tuple(t for t in SIX if t != (1, 1))
KEEP3 = ((0, 0), (0, 1), (1, 0))


def fp32_class_bound(ref64, ref32):
    return 4.0 * rel_err(ref32, ref64) + 1e-7


def split3(v):
    """Exact three-term RNE bf16 split of an fp32 tensor: [3, *v.shape] in float64, v == t0 + t1 + t2 up to
    the third term's rounding (2^-24 |v|), each term a bf16 value."""
    assert v.dtype == torch.float32
    t0 = v.bfloat16().float()
    r1 = v - t0                     # exact in fp32
    t1 = r1.bfloat16().float()
    r2 = r1 - t1                    # exact in fp32
    t2 = r2.bfloat16().float()
    return torch.stack([t0, t1, t2]).double()


def emulate(f, a, b, keep):
    """f evaluated in float64 from the term products (i, j) in keep of the split operands."""
    sa, sb = split3(a), split3(b)
    out = None
    for i, j in keep:
        t = f(sa[i], sb[j])
        out = t if out is None else out + t
    return out


# ---- the ops ---------------------------------------------------------------------------------------------
def _embed(x, w):
    return F.conv2d(F.pad(x, (1, 1, 1, 1), mode="replicate"), w)


def _vjp(fn, at, g):
    """g^T d fn / d at (autograd in the dtype of the arguments; fn is linear in ``at``)."""
    at = torch.zeros_like(at).requires_grad_()
    return torch.autograd.grad(fn(at), at, g)[0]


def f_conv1x1(x, w):                # x [B, K, H, W], w [M, K, 1, 1]
    return F.conv2d(x, w)


def f_conv2x2s2(x, w):              # x [B, K, H, W], w [M, K, 2, 2]; an odd last row / column is dropped
    return F.conv2d(x, w, stride=2)


def f_conv2x2s2_bwd_data(g, w):     # g [B, M, H/2, W/2], w [M, K, 2, 2] -> [B, K, H, W] (H, W even)
    b, _, h, ww = g.shape
    x0 = g.new_zeros(b, w.shape[1], 2 * h, 2 * ww)
    return _vjp(lambda x: F.conv2d(x, w, stride=2), x0, g)


def f_convt2x2s2(x, w):             # x [B, K, H, W], w [K, M, 2, 2]
    return F.conv_transpose2d(x, w, stride=2)


def f_wgrad(a, bop):                # a [B, M, P], bop [B, K, P] -> [M, K]
    return torch.einsum("bmp,bkp->mk", a, bop)


def f_embed_bwd_w(g, x):            # g [B, M, H, W], x [B, Cin, H, W] -> [M, Cin, 3, 3]
    w0 = g.new_zeros(g.shape[1], x.shape[1], 3, 3)
    return _vjp(lambda w: _embed(x, w), w0, g)


def f_embed_bwd_x(g, w):            # g [B, M, H, W], w [M, Cin, 3, 3] -> [B, Cin, H, W]
    x0 = g.new_zeros(g.shape[0], w.shape[1], g.shape[2], g.shape[3])
    return _vjp(lambda x: _embed(x, w), x0, g)


# ---- the fp32 evaluation --------------------------------------------------------------------------------------
# err32 has to be one number on every host.  The CPU library's fp32 convolution is not: it blocks a reduction by
# its instruction set and thread count (the P = 1300 weight gradient below measured err32 2.2e-7 on one host and
# 1.4e-6 on another; a single thread doubles the K = 512 convolution's).  So the fp32 evaluation is spelled out
# in correctly rounded steps, the same bits everywhere, in the order of a CPU GEMM micro-kernel: one fp32
# accumulator per output, a fused multiply-add per reduction step in index order, in blocks of FMA_BLOCK steps
# whose partial sums are added in order.  FMA_BLOCK = 128 is calibrated on the library's own figures, not on any
# kernel: of 16 ... 256 and no blocking it comes closest to the err32 column of the table this work started
# from (conv1x1 K 96 / 384 / 27: 3.9e-7, 3.0e-7, 1.9e-7 against the library's 3.4e-7, 3.8e-7, 1.5e-7; weight
# gradients over 8192 / 1173 / 120 pixels: 3.1e-7, 2.4e-7, 3.3e-7 against 3.6e-7, 3.4e-7, 3.0e-7), and up to
# K = 128 it is this host's library bit for bit.
FMA_BLOCK = 128


def dot32(a, b):
    """[O1, R] x [R, O2] -> [O1, O2] in fp32.  The fma is evaluated in float64 (the product of two floats is
    exact there) and rounded to fp32 once per step."""
    assert a.dtype == torch.float32 and b.dtype == torch.float32
    r = a.shape[1]
    ad, bd = a.double(), b.double()
    total, acc = None, torch.zeros(a.shape[0], b.shape[1])
    for i in range(r):
        acc = (acc.double() + ad[:, i, None] * bd[None, i, :]).float()
        if (i + 1) % FMA_BLOCK == 0 or i == r - 1:
            total = acc if total is None else total + acc
            acc = torch.zeros_like(acc)
    return total


def _conv1x1_32(x, w2):             # x [B, K, ...], w2 [M, K] -> [B, M, ...]
    b, k = x.shape[:2]
    return torch.stack([dot32(w2, x[i].reshape(k, -1)) for i in range(b)]).reshape(b, w2.shape[0], *x.shape[2:])


def _patches2x2(x):                 # [B, K, H, W] -> [B, (k, di, dj), H/2, W/2], an odd last row / column dropped
    b, k, h, w = x.shape
    he, we = h // 2 * 2, w // 2 * 2
    return x[:, :, :he, :we].reshape(b, k, he // 2, 2, we // 2, 2).permute(0, 1, 3, 5, 2, 4).reshape(
        b, 4 * k, he // 2, we // 2)


def _shuffle2x2(t, k):              # [B, (k, di, dj), h, w] -> [B, k, 2h, 2w]
    b, _, h, w = t.shape
    return t.reshape(b, k, 2, 2, h, w).permute(0, 1, 4, 2, 5, 3).reshape(b, k, 2 * h, 2 * w)


def _wgrad_32(a, bop):              # [B, M, P], [B, K, P] -> [M, K], one dot32 over all B P pixels (b-major)
    m, k = a.shape[1], bop.shape[1]
    return dot32(a.permute(1, 0, 2).reshape(m, -1), bop.permute(1, 0, 2).reshape(k, -1).t().contiguous())


def _embed_patches(x):              # [B, Cin, H, W] -> [B, (c, ky, kx), H W], replicate-clamped taps
    b = x.shape[0]
    return F.unfold(F.pad(x, (1, 1, 1, 1), mode="replicate"), 3).reshape(b, -1, x.shape[2] * x.shape[3])


def _embed_bwd_x_32(g, w):
    """Per tap, the dot32 sum over m of w[m, c, ky, kx] g[b, m, p]; then the nine taps' planes are added at
    their clamped positions in (ky, kx) order, row-major over the pixels."""
    b, m, h, ww = g.shape
    cin = w.shape[1]
    t = _conv1x1_32(g, w.permute(1, 2, 3, 0).reshape(cin * 9, m)).reshape(b, cin, 9, h * ww)
    ys, xs = torch.meshgrid(torch.arange(h), torch.arange(ww), indexing="ij")
    out = torch.zeros(b, cin, h * ww)
    for ky in range(3):
        for kx in range(3):
            q = ((ys + ky - 1).clamp(0, h - 1) * ww + (xs + kx - 1).clamp(0, ww - 1)).reshape(-1)
            out.index_add_(2, q, t[:, :, ky * 3 + kx])
    return out.reshape(b, cin, h, ww)


F32 = {
    "conv1x1": lambda x, w: _conv1x1_32(x, w.reshape(w.shape[0], -1)),
    "conv2x2s2": lambda x, w: _conv1x1_32(_patches2x2(x), w.reshape(w.shape[0], -1)),
    "conv2x2s2_bwd_data": lambda g, w: _shuffle2x2(
        _conv1x1_32(g, w.permute(1, 2, 3, 0).reshape(-1, w.shape[0])), w.shape[1]),
    "convt2x2s2": lambda x, w: _shuffle2x2(_conv1x1_32(x, w.permute(1, 2, 3, 0).reshape(-1, w.shape[0])), w.shape[1]),
    "wgrad": _wgrad_32,
    "embed_bwd_w": lambda g, x: _wgrad_32(g.flatten(2), _embed_patches(x)).reshape(g.shape[1], x.shape[1], 3, 3),
    "embed_bwd_x": _embed_bwd_x_32,
    "embed": lambda x, w: _conv1x1_32(_embed_patches(x), w.reshape(w.shape[0], -1)).reshape(
        x.shape[0], w.shape[0], x.shape[2], x.shape[3]),
}
F32["conv1x1_f32"] = F32["conv1x1_cat2"] = F32["conv1x1"]


# shapes(case shape) -> (shape of a, shape of b); kind: "fwd" (a = activations reduced over their channels,
# b = weights) or "wgrad" (a, b = activations reduced over batch and pixels)
Op = namedtuple("Op", "f shapes kind")
OPS = {
    "conv1x1": Op(f_conv1x1, lambda b, k, m, h, w: ((b, k, h, w), (m, k, 1, 1)), "fwd"),
    "conv1x1_f32": Op(f_conv1x1, lambda b, k, m, h, w: ((b, k, h, w), (m, k, 1, 1)), "fwd"),
    # shape (B, Ka, Kb, M, H, W): a is the concatenation, the kernel gets a[:, :Ka] and a[:, Ka:]
    "conv1x1_cat2": Op(f_conv1x1, lambda b, ka, kb, m, h, w: ((b, ka + kb, h, w), (m, ka + kb, 1, 1)), "fwd"),
    "conv2x2s2": Op(f_conv2x2s2, lambda b, k, m, h, w: ((b, k, h, w), (m, k, 2, 2)), "fwd"),
    # shape (B, K, M, H, W) of the forward conv: g [B, M, H/2, W/2]
    "conv2x2s2_bwd_data": Op(f_conv2x2s2_bwd_data, lambda b, k, m, h, w: ((b, m, h // 2, w // 2), (m, k, 2, 2)),
                             "fwd"),
    "convt2x2s2": Op(f_convt2x2s2, lambda b, k, m, h, w: ((b, k, h, w), (k, m, 2, 2)), "fwd"),
    "wgrad": Op(f_wgrad, lambda b, m, k, p: ((b, m, p), (b, k, p)), "wgrad"),
    # shape (B, Cin, M, H, W)
    "embed_bwd_w": Op(f_embed_bwd_w, lambda b, c, m, h, w: ((b, m, h, w), (b, c, h, w)), "wgrad"),
    "embed_bwd_x": Op(f_embed_bwd_x, lambda b, c, m, h, w: ((b, m, h, w), (m, c, 3, 3)), "fwd"),
}

WEIGHT_SCALE = 0.2


class Case(namedtuple("Case", "op shape seed scale offset note opts")):
    @property
    def id(self):
        return self.op + "-" + "x".join(map(str, self.shape)) + ("-" + "-".join(self.opts) if self.opts else "")


def C(op, shape, seed, scale, offset, note, *opts):
    return Case(op, tuple(shape), seed, scale, offset, note, tuple(opts))


def inputs(case):
    """(a, b) in fp32.  Activations are rand(seed) * scale + offset; weights are rand(seed + 1) * 0.2; the
    second half of a concatenated input has the offset's sign flipped (as test_gpu_codec.py's)."""
    sa, sb = OPS[case.op].shapes(*case.shape)
    a = rand(*sa, seed=case.seed, scale=case.scale, offset=case.offset)
    if case.op == "conv1x1_cat2":
        ka = case.shape[1]
        a[:, ka:] = rand(sa[0], sa[1] - ka, *sa[2:], seed=case.seed + 2, scale=case.scale, offset=-case.offset)
    if OPS[case.op].kind == "wgrad":
        b = rand(*sb, seed=case.seed + 1, scale=case.scale, offset=case.offset)
    else:
        b = rand(*sb, seed=case.seed + 1) * WEIGHT_SCALE
    return a, b


Refs = namedtuple("Refs", "a b ref64 ref32 bound")


@lru_cache(maxsize=None)
def refs(case):
    """The case's inputs, float64 and fp32 CPU references and its bound, computed once and shared."""
    a, b = inputs(case)
    f = OPS[case.op].f
    ref64 = f(a.double(), b.double())
    ref32 = F32[case.op](a, b)
    assert ref32.dtype == torch.float32
    return Refs(a, b, ref64, ref32, fp32_class_bound(ref64, ref32))


def mutant_errors(case):
    """rel_err against float64 of the SIX, DROP11 and KEEP3 emulations (one evaluation per product)."""
    r = refs(case)
    f = OPS[case.op].f
    sa, sb = split3(r.a), split3(r.b)
    prod = {t: f(sa[t[0]], sb[t[1]]) for t in SIX}
    return tuple(rel_err(sum(prod[t] for t in keep), r.ref64) for keep in (SIX, DROP11, KEEP3))


# ---- grr_wgrad's plan (csrc/wgrad_ops.hip wgrad_plan), mirrored so the seams can be named and cut ------------
WG_TILES = ((4, 3, 1, 1.0), (6, 2, 1, 1.05), (2, 3, 2, 0.8))     # 128 x 96, 192 x 64, 64 x 96 (two waves / SIMD)
WgPlan = namedtuple("WgPlan", "tile swap CP cpi")


def wgrad_plan(b, m, k, p, tiles=True):
    best = None
    for ta, tb, wps, c in (WG_TILES if tiles else WG_TILES[:1]):
        for sw in (False, True):
            ma, kb = (k, m) if sw else (m, k)
            na, nb = -(-ma // (32 * ta)), -(-kb // (32 * tb))
            cost = na * nb * c
            if best is None or cost < best[0]:
                best = (cost, ta, tb, wps, sw, na * nb)
    _, ta, tb, wps, sw, ntile = best
    target = 3072 * wps
    cp = -(-(b * p * ntile) // target)
    cp = -(-cp // 32) * 32
    pmax = -(-p // 32) * 32
    cp = min(max(cp, 512), pmax)
    while True:
        cpi = -(-p // cp)
        if (b * cpi <= 4096 and b * cpi * m * k * 4 <= (128 << 20)) or cp >= pmax:
            break
        cp = min(pmax, cp * 2)
    return WgPlan(f"{32 * ta}x{32 * tb}", sw, cp, cpi)


def wgrad_dims(case):
    """(B, M, K, P) of the grr_wgrad launch behind a wgrad-kind case."""
    if case.op == "wgrad":
        return case.shape
    b, cin, m, h, w = case.shape
    return b, m, 9 * cin, h * w


def structural(case):
    """{name: mutant reference in float64}: one pixel, one k row, and (weight gradients whose last chunk has
    a full step) the last 16-pixel step of the last chunk of the last image left out."""
    r = refs(case)
    op = OPS[case.op]
    a, b = r.a.double(), r.b.double()
    out = {}
    if op.kind == "fwd":
        px = r.ref64.clone()
        px[-1, :, -1, -1] = 0
        out["pixel"] = px
        ak = a.clone()
        ak[:, -1] = 0
        out["krow"] = op.f(ak, b)
        return out
    bb, m, k, p = wgrad_dims(case)
    af = a.clone().reshape(bb, m, p)
    af[-1, :, -1] = 0
    out["pixel"] = op.f(af.reshape(a.shape), b)
    bk = b.clone()
    bk[:, -1] = 0
    out["krow"] = op.f(a, bk)
    plan = wgrad_plan(bb, m, k, p, "tiles0" not in case.opts)
    begin = (plan.cpi - 1) * plan.CP
    ns = (p - begin) // 16
    if ns > 0:
        af = a.clone().reshape(bb, m, p)
        af[-1, :, begin + 16 * (ns - 1):begin + 16 * ns] = 0
        out["step"] = op.f(af.reshape(a.shape), b)
    return out


# ---- case tables -------------------------------------------------------------------------------------------
# (shape, seed, scale, offset, note).  Shapes: conv ops (B, K, M, H, W); cat2 (B, Ka, Kb, M, H, W); wgrad (B, M, K, P);
# embed (B, Cin, M, H, W).
CONV1X1_X3 = [
    C("conv1x1", (1, 1, 32, 1, 31), 101, 2.0, 0.3, "x3 KS=1, K=1 (15 of 16 rows past num_records); one ragged tile P=31"),
    C("conv1x1", (2, 16, 33, 1, 257), 103, 2.0, 0.3, "x3 KS=1 whole step; nch=2 (M=33, one row in the last chunk); tiles=2, last holds 1 pixel; B=2"),
    C("conv1x1", (1, 17, 3, 1, 1), 105, 3.0, 0.5, "x3 KS=2, one row in the last step; M=3; P=1 (every lane but one clamped to pixel 0)"),
    C("conv1x1", (1, 27, 48, 10, 10), 107, 2.0, 0.3, "x3 KS=2 ragged (the embedding's K=27); nch=2 with 16 rows in the last"),
    C("conv1x1", (2, 48, 192, 1, 257), 109, 2.0, 0.3, "x3 KS=3 whole; nch=6; tiles=2; B=2"),
    C("conv1x1", (1, 64, 32, 40, 36), 111, 1.0, 0.0, "x3 KS=4 whole; nch=1; tiles=6 (P=1440, last tile 160 pixels); zero-mean"),
    C("conv1x1", (1, 72, 33, 1, 31), 113, 2.0, 0.3, "x3 KS=5, 8 rows in the last step; nch=2; P=31"),
    C("conv1x1", (2, 96, 192, 40, 36), 31, 3.0, 0.5, "x3 KS=6 (test_x3_gemm_is_fp32_accurate's shape); nch=6; tiles=6"),
    C("conv1x1", (1, 100, 3, 1, 257), 1117, 2.0, 0.3, "x3 KS=7, 4 rows in the last step; M=3; tiles=2"),
    C("conv1x1", (1, 128, 33, 1, 31), 119, 2.0, 0.3, "x3 KS=8 whole (the last K on gemm_x3); nch=2; P=31"),
    C("conv1x1", (2, 128, 192, 1, 1), 121, 3.0, 0.5, "x3 KS=8; nch=6; P=1; B=2"),
]
CONV1X1_X3K = [
    C("conv1x1", (1, 129, 5, 1, 5), 131, 2.0, 0.3, "x3k KS=9 (first K on gemm_x3k; one row in the last step; odd KS: single k-step tail); TM=1; P=5"),
    C("conv1x1", (2, 144, 40, 10, 33), 7133, 2.0, 0.3, "x3k KS=9 whole last step; TM=2 (8 rows in group 1); tiles=2 (P=330); B=2"),
    C("conv1x1", (1, 200, 96, 10, 33), 28135, 1.0, 0.0, "x3k KS=13 ragged; TM=3; tiles=2; zero-mean"),
    C("conv1x1", (1, 384, 128, 1, 5), 137, 2.0, 0.3, "x3k KS=24 (even: no k-step tail); TM=4, nmt=1; P=5"),
    C("conv1x1", (1, 512, 130, 10, 33), 25139, 3.0, 0.5, "x3k KS=32; groups=5: TM=4, nmt=2, three clamped groups in the last M tile"),
    C("conv1x1", (2, 144, 300, 1, 5), 4141, 2.0, 0.3, "x3k KS=9; groups=10: TM=4, nmt=3, two clamped groups in the last M tile; B=2"),
]
CONV1X1_F32 = [
    C("conv1x1_f32", (2, 20, 130, 11, 12), 151, 2.0, 0.3, "f32 vec (K=20, P=132): second k-chunk partial (scalar fill inside vec); mt=2 (M=130); nt=2, last 4 pixels; B=2"),
    C("conv1x1_f32", (1, 7, 130, 5, 6), 153, 2.0, 0.3, "f32 scalar path (K=7, P=30); one partial k-chunk; mt=2"),
    C("conv1x1_f32", (1, 160, 40, 9, 10), 9155, 1.0, 0.0, "f32 scalar path (P=90 % 4 != 0) at ten k-chunks (test_conv1x1_fp32_kernel's shape); zero-mean"),
]
CONV1X1_CAT2 = [
    C("conv1x1_cat2", (1, 16, 1, 16, 7, 11), 161, 2.0, 0.3, "x3 CAT KS=2: Ka=16 (the smallest), second source one row, 15 past its num_records; P=77"),
    C("conv1x1_cat2", (2, 16, 16, 48, 9, 37), 163, 2.0, 0.3, "x3 CAT KS=2, one whole step per source; nch=2 ragged; tiles=2 (P=333); B=2"),
    C("conv1x1_cat2", (1, 48, 96, 130, 7, 11), 165, 2.0, 0.3, "x3k CAT KS=9, Ka != Kb, source switch at step 3; TM=4, nmt=2 (M=130)"),
    C("conv1x1_cat2", (1, 112, 16, 48, 7, 11), 167, 3.0, 0.5, "x3 CAT KS=8: Ka + Kb = 128, the last shape on gemm_x3"),
    C("conv1x1_cat2", (1, 112, 17, 48, 7, 11), 4169, 3.0, 0.5, "x3k CAT KS=9: Ka + Kb = 129, the first on gemm_x3k; second source's last step one row"),
    C("conv1x1_cat2", (1, 128, 5, 16, 9, 37), 171, 2.0, 0.3, "x3k CAT KS=9; Kb=5 ragged; TM=1 (M=16); tiles=2"),
    C("conv1x1_cat2", (1, 64, 200, 16, 7, 11), 14173, 1.0, 0.0, "x3k CAT KS=17 (odd), Kb % 16 = 8; TM=1; zero-mean"),
    C("conv1x1_cat2", (1, 192, 192, 48, 7, 11), 24175, 2.0, 0.3, "x3k CAT KS=24, Ka = Kb (the model's combine); TM=2"),
]
CONV2X2S2 = [
    C("conv2x2s2", (1, 3, 48, 34, 50), 181, 2.0, 0.3, "f32 IM2COL K=12 (one partial k-chunk); P=425 (% 4 != 0: scalar path); nt=4"),
    C("conv2x2s2", (2, 12, 5, 16, 16), 183, 2.0, 0.3, "f32 IM2COL vec (K=48, P=64); M=5 < 32; B=2"),
    C("conv2x2s2", (1, 48, 96, 9, 13), 8185, 2.0, 0.3, "odd H and W: row 8 and column 12 never read; P=24 vec; K=192"),
    C("conv2x2s2", (1, 96, 130, 8, 6), 12187, 2.0, 0.3, "mt=2 (M=130); P=12 vec; K=384 (24 k-chunks)"),
    C("conv2x2s2", (1, 192, 384, 2, 2), 189, 2.0, 0.3, "2x2 image: P=1 (scalar path); mt=3; K=768"),
    C("conv2x2s2", (2, 48, 24, 16, 16), 191, 1.0, 0.0, "M=24 < 32; vec; the channel roles of convt2x2s2's data gradient (48 <- 24); B=2; zero-mean"),
    C("conv2x2s2", (1, 12, 5, 9, 13), 193, 2.0, 0.3, "odd H and W at M < 32, K=48"),
    C("conv2x2s2", (1, 3, 48, 2, 2), 195, 2.0, 0.3, "2x2 image at K=12: one pixel, one partial k-chunk"),
]
# both = the direct kernel and the GEMM + interleave (W % 4 == 0); direct = grr_conv2x2s2_bwd_data only
CONV2X2S2_BWD = [
    C("conv2x2s2_bwd_data", (2, 12, 24, 12, 16), 201, 2.0, 0.3, "both; GEMM: x3 KS=2 (K=M=24), 48 rows; B=2", "both"),
    C("conv2x2s2_bwd_data", (1, 96, 192, 2, 4), 203, 2.0, 0.3, "both; 2x4 image (P=2); GEMM: x3k KS=12, 384 rows: nmt=3", "both"),
    C("conv2x2s2_bwd_data", (1, 24, 160, 34, 52), 10205, 1.0, 0.0, "both; GEMM: x3k KS=10, 96 rows: TM=3; P=442; zero-mean", "both"),
    C("conv2x2s2_bwd_data", (2, 3, 48, 12, 16), 207, 3.0, 0.5, "both; GEMM: x3 KS=3, 12 rows; B=2", "both"),
    C("conv2x2s2_bwd_data", (1, 12, 24, 34, 14), 209, 2.0, 0.3, "direct only (W=14: W % 4 != 0, the shape training sends it)", "direct"),
    C("conv2x2s2_bwd_data", (1, 3, 48, 12, 50), 211, 2.0, 0.3, "direct only (W=50); 600 pixels: three blocks per plane, last partial", "direct"),
]
CONVT2X2S2 = [
    C("convt2x2s2", (1, 48, 3, 5, 7), 221, 2.0, 0.3, "x3 KS=3; 4M=12 rows; P=35 (% 32 != 0)"),
    C("convt2x2s2", (1, 192, 130, 3, 5), 2223, 3.0, 0.5, "x3k KS=12; 4M=520 rows: groups=17, nmt=5 (three clamped groups); P=15"),
    C("convt2x2s2", (2, 64, 48, 3, 11), 225, 1.0, 0.0, "x3 KS=4; 192 rows; P=33; B=2; zero-mean"),
]
WGRAD = [
    # tiles (test_wgrad_tile_plans_match_float64's shapes, the 64 x 64 images shrunk to 16 x 16)
    C("wgrad", (2, 192, 48, 256), 7231, 2.0, 0.3, "192x64 noswap CP=256 cpi=1; ns=16"),
    C("wgrad", (2, 48, 192, 256), 27233, 2.0, 0.3, "192x64 swap CP=256 cpi=1"),
    C("wgrad", (2, 48, 96, 256), 25235, 2.0, 0.3, "64x96 noswap CP=256 cpi=1 (two waves per SIMD)"),
    C("wgrad", (1, 40, 70, 143), 237, 2.0, 0.3, "64x96 noswap CP=160 cpi=1; rows past the tile; P % 4 != 0 (scalar loads); ns=8, tail 15"),
    C("wgrad", (3, 170, 33, 180), 15239, 3.0, 0.3, "192x64 noswap CP=192 cpi=1; rows past the tile; ns=11 (odd), tail 4"),
    C("wgrad", (1, 12, 7, 9), 241, 1.0, 0.0, "64x96 noswap CP=32 cpi=1; ns=0: tail only (9 pixels, both half-waves); zero-mean"),
    # the knob: the 128 x 96 tile alone
    C("wgrad", (2, 192, 48, 256), 7231, 2.0, 0.3, "tiles off: 128x96 noswap CP=256 cpi=1, two tiles", "tiles0"),
    C("wgrad", (1, 40, 70, 143), 237, 2.0, 0.3, "tiles off: 128x96 noswap CP=160 cpi=1", "tiles0"),
    # seams
    C("wgrad", (1, 33, 20, 5), 243, 2.0, 0.3, "64x96 noswap CP=32 cpi=1; ns=0, tail 5 (first half-wave only)"),
    C("wgrad", (1, 33, 20, 15), 245, 2.0, 0.3, "64x96 noswap CP=32 cpi=1; ns=0, tail 15"),
    C("wgrad", (1, 33, 20, 16), 247, 2.0, 0.3, "64x96 noswap CP=32 cpi=1; ns=1: the single step alone, no tail; vec"),
    C("wgrad", (1, 33, 20, 17), 249, 2.0, 0.3, "64x96 noswap CP=32 cpi=1; ns=1, tail 1"),
    C("wgrad", (1, 33, 20, 32), 251, 2.0, 0.3, "64x96 noswap CP=32 cpi=1; ns=2 (even: one loop trip, no single step); vec"),
    C("wgrad", (2, 33, 20, 48), 253, 2.0, 0.3, "64x96 noswap CP=64 cpi=1; ns=3 (odd: one trip + the single step); vec; B=2"),
    C("wgrad", (2, 48, 27, 60), 255, 2.0, 0.3, "64x96 noswap CP=64 cpi=1; ns=3, tail 12 (both half-waves); K=27"),
    C("wgrad", (3, 130, 97, 391), 22257, 3.0, 0.5, "128x96 swap CP=416 cpi=1, two tiles; ns=24, tail 7; P % 4 != 0"),
    C("wgrad", (3, 33, 20, 1300), 259, 2.0, 0.3, "64x96 noswap CP=512 cpi=3, last chunk 276 pixels: ns=17 (odd), tail 4; vec"),
    C("wgrad", (3, 33, 20, 1301), 261, 1.0, 0.0, "64x96 noswap CP=512 cpi=3, last chunk 277: scalar loads across chunk seams; zero-mean"),
    # the embedding's patch reductions K = 9 Cin
    C("wgrad", (2, 128, 36, 60), 263, 2.0, 0.3, "128x96 noswap CP=64 cpi=1; K=36"),
    C("wgrad", (2, 5, 9, 60), 265, 2.0, 0.3, "64x96 noswap CP=64 cpi=1; M=5, K=9"),
    C("wgrad", (2, 64, 18, 60), 267, 3.0, 0.5, "64x96 noswap CP=64 cpi=1; K=18"),
]
EMBED_SHAPES = [(2, 3, 48, 6, 10), (1, 1, 5, 1, 1), (1, 4, 128, 2, 2), (1, 2, 16, 3, 1), (1, 3, 48, 1, 70),
                (2, 3, 48, 17, 23)]
_EMBED_NOTES = ["P=60, K=27", "one pixel: all nine taps clamp onto it", "2x2 image, Cin=4 (K=36), M=128",
                "one column (W=1), Cin=2", "one row (H=1), W=70", "odd H and W, P=391: ragged wgrad steps; B=2"]
# (seed, scale, offset) per shape; zero-mean at the one-row image
_EMBED_W_IN = [(271, 2.0, 0.3), (1273, 2.0, 0.3), (275, 2.0, 0.3), (277, 2.0, 0.3), (279, 1.0, 0.0), (23281, 3.0, 0.5)]
_EMBED_X_IN = [(291, 2.0, 0.3), (293, 2.0, 0.3), (2295, 2.0, 0.3), (297, 2.0, 0.3), (299, 1.0, 0.0), (301, 2.0, 0.3)]
EMBED_BWD_W = [C("embed_bwd_w", s, *i, "patches + grr_wgrad: " + n + ("; zero-mean" if i[2] == 0.0 else ""))
               for s, n, i in zip(EMBED_SHAPES, _EMBED_NOTES, _EMBED_W_IN)]
# regression: embed_bwd_x_kernel summed its up to 81 M terms in one fp32 accumulator; at (1, 4, 128, 2, 2) (1152
# terms per output) that measured 1.18e-6 against the bound 1.02e-6.  It accumulates in fp64 now.
EMBED_BWD_X = [C("embed_bwd_x", s, *i, "clamped-gather adjoint (one fma chain per output, fp64 accumulator): " + n
                 + ("; zero-mean" if i[2] == 0.0 else "")
                 + ("; regression: 1152-term chain, a single fp32 accumulator missed the bound" if s[2] == 128 else ""))
               for s, n, i in zip(EMBED_SHAPES, _EMBED_NOTES, _EMBED_X_IN)]

TABLES = {
    "conv1x1_x3": CONV1X1_X3, "conv1x1_x3k": CONV1X1_X3K, "conv1x1_f32": CONV1X1_F32, "conv1x1_cat2": CONV1X1_CAT2,
    "conv2x2s2": CONV2X2S2, "conv2x2s2_bwd_data": CONV2X2S2_BWD, "convt2x2s2": CONVT2X2S2, "wgrad": WGRAD,
    "embed_bwd_w": EMBED_BWD_W, "embed_bwd_x": EMBED_BWD_X,
}
ALL_CASES = [c for t in TABLES.values() for c in t]

# cases whose dispatch edge exists only where DROP11 is not 1.5 x bound away (at most one per op): the
# structural conditions alone.  {case id: why}
STRUCTURAL_ONLY = {}
