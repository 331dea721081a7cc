"""Float64 references, case lists and input makers for the pointwise and reduction kernels of the
LocalNonLinearBlock / FeedForward reverse (csrc/lnb_bwd.hip): the per-pixel norm and its two reverses, the
LNB gate and its two reverses, the fused depthwise + gate row kernels of both blocks.

Every reference is a plain PyTorch restatement of the operation differentiated by autograd in float64; the
closed forms the kernels evaluate (the header of lnb_bwd.hip) are restated separately (norm_forward_formula,
norm_reverse_formula) in a chosen dtype: in float64 tests/test_lnb_bwd_ref.py holds them to autograd, in
float32 they are the "same formulas in fp32" whose error against float64 bounds an ill-conditioned case.

tests/test_gpu_lnb_bwd_kernels.py (GPU) and tests/test_lnb_bwd_ref.py (CPU) draw the same tensors from here.
"""
import functools
from types import SimpleNamespace

import torch

EPS = 1e-5            # REF:919-925: 1 / sqrt(var + 1e-5), unbiased variance, x not centred
SKIP = (0.7, 1.3)     # the block's skip weights (s0 scales gout in the fused tail)
SCALE = 0.7           # the skip scale folded into the gate's reverse

# (B, C, H, W)
NORM_SHAPES = [
    (2, 2, 3, 5),        # C - 1 = 1
    (1, 3, 1, 1),        # P = 1
    (3, 7, 9, 31),       # C % 8 != 0 (the unrolled channel loops' remainder), four pixel blocks
    (2, 48, 16, 20),     # shared with test_lnb_norm_bwd_skip_equals_separate_passes
    (1, 96, 33, 7),      # shared with test_lnb_norm_bwd_skip_equals_separate_passes
    (2, 33, 40, 50),     # 8 chunks per plane (chunks_for: 4096 / 66 planes = 63, capped by 2000 / 256), B = 2
    (255, 257, 1, 2),    # B*C = 65535, the last accepted value
]
NORM_LIMIT = (256, 256, 1, 1)    # B*C = 65536: the reverses refuse, the forward has no plane limit
NORM_ILL = (2, 12, 8, 16)        # x = 40 + 0.05 randn: |mean| / std ~ 800 per pixel

# (B, hid, H, W)
GATE_SHAPES = [(2, 1, 1, 1), (1, 3, 7, 9), (2, 5, 16, 20),
               (2, 3, 300, 600)]  # 1.08 M gated elements: past 4096 blocks x 256 of gate_bwd_scaled_kernel
GATE_EXTREME = (1, 2, 4, 16)
EXTREME_M = (-100.0, -30.0, -1e-3, 0.0, 1e-3, 30.0, 100.0)   # expf(-m) overflows fp32 below m = -88.7

# lnb_gate_dw3_bwd with hp given: V = 1, 2, 4 and column strips
HP_SHAPES = [(2, 3, 9, 32), (1, 4, 20, 100), (1, 2, 12, 200), (1, 2, 10, 300)]


def _seed(shape, salt):
    s = salt
    for v in shape:
        s = s * 1009 + v
    return s % (2 ** 31 - 1)


def _randn(gen, *shape):
    return torch.randn(*shape, generator=gen)


# ---- the norm ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def norm_inputs(shape, ill=False):
    """fp32 CPU tensors of one norm case.  pre_*: the random pre-fill of the accumulating outputs."""
    b, c, h, w = shape
    g = torch.Generator().manual_seed(_seed(shape, 11 + int(ill)))
    x = (40.0 + 0.05 * _randn(g, b, c, h, w)) if ill else (_randn(g, b, c, h, w) + 0.3)
    return SimpleNamespace(
        shape=shape, x=x, ln_w=torch.rand(c, generator=g) + 0.5, gn=_randn(g, b, c, h, w),
        gout=_randn(g, b, c, h, w), skip=torch.tensor(SKIP), pre_gx=0.5 * _randn(g, b, c, h, w),
        pre_gln_w=_randn(g, c), pre_gskip0=_randn(g, 1))


@functools.lru_cache(maxsize=None)
def norm_ref(shape, ill=False):
    """float64: n, isd of the forward; gx, gln_w of the cotangent gn; the skip form gx_skip = s0 gout + gx,
    gskip0 = <gout, x>."""
    d = norm_inputs(shape, ill)
    x = d.x.double().requires_grad_(True)
    lw = d.ln_w.double().requires_grad_(True)
    isd = 1.0 / torch.sqrt(x.var(dim=1, keepdim=True, correction=1) + EPS)
    n = lw[None, :, None, None] * x * isd
    n.backward(d.gn.double())
    gout = d.gout.double()
    return SimpleNamespace(n=n.detach(), isd=isd.detach()[:, 0], gx=x.grad, gln_w=lw.grad,
                           gx_skip=SKIP[0] * gout + x.grad, gskip0=(gout * d.x.double()).sum().reshape(1))


def norm_forward_formula(x, ln_w):
    """The forward as ln_fwd_kernel evaluates it, channel by channel in x's dtype: (n, isd)."""
    c = x.shape[1]
    s = torch.zeros_like(x[:, 0])
    for k in range(c):
        s = s + x[:, k]
    mean = s / c
    q = torch.zeros_like(s)
    for k in range(c):
        dlt = x[:, k] - mean
        q = q + dlt * dlt
    isd = 1.0 / torch.sqrt(q / (c - 1) + torch.tensor(EPS, dtype=x.dtype))
    return (ln_w[None, :, None, None] * x) * isd[:, None], isd


def norm_reverse_formula(x, ln_w, isd, gn, gout=None, s0=None):
    """The closed-form reverse in the header of lnb_bwd.hip, in x's dtype:
      gx_k = ln_w_k gn_k isd - (x_k - mean) isd^3 / (C - 1) sum_c ln_w_c gn_c x_c,  gln_w_c = sum gn_c x_c isd
    and with gout the skip form (s0 gout + gx, <gout, x>).  Returns (gx, gln_w, gskip0 or None)."""
    c = x.shape[1]
    s = torch.zeros_like(x[:, 0])
    dot = torch.zeros_like(s)
    for k in range(c):
        s = s + x[:, k]
        dot = dot + ln_w[k] * gn[:, k] * x[:, k]
    mean = s / c
    kk = dot * isd * isd * isd / (c - 1)
    gx = ln_w[None, :, None, None] * gn * isd[:, None] - (x - mean[:, None]) * kk[:, None]
    gln_w = (gn * x * isd[:, None]).sum(dim=(0, 2, 3))
    if gout is None:
        return gx, gln_w, None
    return s0 * gout + gx, gln_w, (gout * x).sum().reshape(1)


# ---- the LNB gate -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gate_inputs(shape, extreme=False):
    """hp = [m; v] [B, 2 hid, H, W], one cotangent g [B, hid, H, W] (ggate of the plain reverse, gq of the
    scaled one).  extreme: m cycles through EXTREME_M in a shuffled order."""
    b, hid, h, w = shape
    g = torch.Generator().manual_seed(_seed(shape, 23 + int(extreme)))
    hp = _randn(g, b, 2 * hid, h, w) * (1.0 if extreme else 2.0)
    if extreme:
        n = b * hid * h * w
        vals = torch.tensor(EXTREME_M).repeat(-(-n // len(EXTREME_M)))[:n]
        hp[:, :hid] = vals[torch.randperm(n, generator=g)].view(b, hid, h, w)
    return SimpleNamespace(shape=shape, hp=hp, g=_randn(g, b, hid, h, w), scale=torch.tensor([SCALE]),
                           pre_gdot=_randn(g, 1))


@functools.lru_cache(maxsize=None)
def gate_ref(shape, extreme=False):
    """float64: gate = sigmoid(m) m v; ghp from the cotangent g; the scaled form ghp_s = SCALE ghp and
    gdot = <g, gate>."""
    d = gate_inputs(shape, extreme)
    hp = d.hp.double().requires_grad_(True)
    m, v = hp.chunk(2, dim=1)
    gate = torch.sigmoid(m) * m * v
    (d.g.double() * gate).sum().backward()
    return SimpleNamespace(gate=gate.detach(), ghp=hp.grad, ghp_s=SCALE * hp.grad,
                           gdot=(d.g.double() * gate.detach()).sum().reshape(1))


# ---- depthwise 3x3 and the fused depthwise + gate ----------------------------------------------------------------
def dw3_ref(h, w):
    """Replicate-padded depthwise 3x3 (REF:946), h [B, C, H, W], w [C, 9]."""
    c = h.shape[1]
    return torch.nn.functional.conv2d(torch.nn.functional.pad(h, (1, 1, 1, 1), mode="replicate"),
                                      w.view(c, 1, 3, 3), groups=c)


def dw3_gate(hh, w, ffn):
    """(LNB) replicate-pad depthwise, sigmoid(m) m v  /  (FFN, REF7:42-46) zero-pad depthwise, gelu(m) v with
    the exact-erf gelu: the gate of tests/test_gpu_dwconv._gate_ref."""
    c2 = hh.shape[1]
    if ffn:
        d = torch.nn.functional.conv2d(hh, w.view(c2, 1, 3, 3), padding=1, groups=c2)
    else:
        d = dw3_ref(hh, w)
    m, v = d.chunk(2, dim=1)
    return (torch.nn.functional.gelu(m) if ffn else torch.sigmoid(m) * m) * v


@functools.lru_cache(maxsize=None)
def fused_inputs(shape, extreme=False):
    """hh [B, 2 hid, H, W], depthwise taps [2 hid, 9], gq [B, hid, H, W].  extreme: the m half of hh cycles
    through EXTREME_M and the taps are 1 at the centre, 0 elsewhere, so the depthwise output is hh itself."""
    b, hid, h, w = shape
    if extreme:
        gi = gate_inputs(shape, True)
        wdw = torch.zeros(2 * hid, 9)
        wdw[:, 4] = 1.0
        return SimpleNamespace(shape=shape, hh=gi.hp, wdw=wdw, gq=gi.g, scale=gi.scale)
    g = torch.Generator().manual_seed(_seed(shape, 37))
    return SimpleNamespace(shape=shape, hh=_randn(g, b, 2 * hid, h, w), wdw=_randn(g, 2 * hid, 9) * 0.5,
                           gq=_randn(g, b, hid, h, w), scale=torch.tensor([SCALE]))


@functools.lru_cache(maxsize=None)
def fused_ref(shape, ffn=False, extreme=False):
    """float64: the gate, gh and gwdw of SCALE <gq, gate>, gdot = <gq, gate> and sum |gq gate| (the scale the
    fused tests hold gdot to)."""
    d = fused_inputs(shape, extreme)
    hh = d.hh.double().requires_grad_(True)
    w = d.wdw.double().requires_grad_(True)
    gate = dw3_gate(hh, w, ffn)
    prod = d.gq.double() * gate
    (SCALE * prod.sum()).backward()
    return SimpleNamespace(gate=gate.detach(), gh=hh.grad, gwdw=w.grad, gdot=prod.detach().sum().reshape(1),
                           gabs=float(prod.detach().abs().sum()))


@functools.lru_cache(maxsize=None)
def dw3_inputs(shape):
    b, c, h, w = shape
    g = torch.Generator().manual_seed(_seed(shape, 41))
    return SimpleNamespace(shape=shape, h=_randn(g, b, c, h, w), wdw=_randn(g, c, 9), g=_randn(g, b, c, h, w),
                           pre_gwdw=_randn(g, c, 9))


@functools.lru_cache(maxsize=None)
def dw3_case_ref(shape):
    d = dw3_inputs(shape)
    h = d.h.double().requires_grad_(True)
    w = d.wdw.double().requires_grad_(True)
    out = dw3_ref(h, w)
    out.backward(d.g.double())
    return SimpleNamespace(out=out.detach(), gh=h.grad, gwdw=w.grad)


# ---- measures ---------------------------------------------------------------------------------------------------
def elem_err(a, r):
    """max-abs error over max-abs reference (element-wise outputs)."""
    a, r = a.detach().double().cpu().reshape(r.shape), r.double()
    return float((a - r).abs().max()) / float(r.abs().max())


def sum_err(a, r, n):
    """Error of a sum of n O(1) terms in units of max(max|ref|, sqrt(n)) (the tests/test_gpu_term_oracle.py rule)."""
    a, r = a.detach().double().cpu().reshape(r.shape), r.double()
    return float((a - r).abs().max()) / max(float(r.abs().max()), n ** 0.5)
