"""Gradients of the GLRFast / GTVFast module methods (the reference differentiates these ATen
compositions with autograd, REF = exploration/GGTV_GGLR_v1.0/deep_multiscale_GGLR_GGTV_v1x0.py
:128-228, :452-516): the HIP reverses (csrc/subapi_bwd.hip through solver_grad's opaque functions)
against float64 autograd through the oracle's restatement of the same methods.

Cases (B, G, F, H, W), every method at every case:
  (2, 3, 4, 9, 13)      odd image sizes, every replicate / zero / frame-drop boundary rule; one block per plane
  (1, 2, 3, 1, 1)       a 1 x 1 image: all four edges clamp to the pixel itself (clamp_adj's self term alone)
  (1, 2, 3, 1, 7), (2, 1, 2, 6, 1)   one side of the image is 1: clamp_adj counts the shifted source and the self-clamp
  (1, 1, 1, 2, 2)       G = F = 1
  (1, 2, 16, 5, 70)     F = 16 = FMAX, two blocks per plane (the per-block partials are combined)
  (2, 3, 4, 40, 300)    47 blocks per plane, B > 1: chunk_slot with gridDim.x > 1 and the B * blocks slot plan
  (520, 8, 2, 3, 90)    B*G = 4160, B*G*F = 8320 planes: grid2's 8192 / rows cap leaves one block per plane of 270
                        pixels, so every kernel takes a second grid-stride turn with a partial block
  (65535, 1, 1, 1, 1)   65535 planes, the last accepted count ((65535, 1, 2, 1, 1) for normalize_features, whose
                        rows are B*G and whose feature gradient is identically zero at F = 1); 65536 is refused

Tolerances: forward 1e-5; input gradients max-abs error over max-abs reference <= 2e-5 (fp32 kernels vs fp64
reference).  Per-channel and per-graph sums (the stencil parameters' and multiM's gradients) are held to
2e-5 max(max|ref|, sqrt(N)), N = B H W, as tests/test_gpu_term_oracle.py holds its sums (a relative bound on a sum
of 140,000 O(1) terms measures its cancellation); the first case keeps the relative 2e-5 as well.  Where a
reference cancels to nothing -- below 1e-6 of the terms it is made of: op_L_norm and op_C on a 1 x 1 image, where
x - sum_e w_e x = x (1 - sum_e w_e) is the fp32 softmax weights' own rounding (their sum is 1 +- 2e-7) and
s - s(clamp) = 0; normalize_features at F = 1, y = +-1 -- the error is held to the same 2e-5 of the un-cancelled
terms' scale from the oracle, as test_edge_weights_reverse_matches_oracle does at F = 1.

Measured on an MI355X, worst over all cases in units of each bound's scale: forward 2.4e-7, input gradients 1.1e-6
(normalize_features at 65535 planes; 1.8e-7 elsewhere), multiM 2.5e-7, stencil parameters 3.7e-7."""
import pytest
import torch

from oracle import graph_oracle as O
from tests.test_gpu_parity import DEV, perturbed_graph_module, rand

pytestmark = pytest.mark.gpu

B, G, F, H, W = 2, 3, 4, 9, 13
FIRST = (B, G, F, H, W)
CASES = [FIRST, (1, 2, 3, 1, 1), (1, 2, 3, 1, 7), (2, 1, 2, 6, 1), (1, 1, 1, 2, 2), (1, 2, 16, 5, 70),
         (2, 3, 4, 40, 300), (520, 8, 2, 3, 90)]
ROWS_BGF = (65535, 1, 1, 1, 1)    # B*G*F = 65535 rows of 1 x 1 images
ROWS_BG = (65535, 1, 2, 1, 1)     # B*G = 65535 rows (normalize_features_bwd)
ids = lambda c: "b{}g{}f{}h{}w{}".format(*c)   # noqa: E731
cases = pytest.mark.parametrize("case", CASES + [ROWS_BGF], ids=ids)


@pytest.fixture(scope="module")
def irdu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import irdu_amd
    irdu_amd.load_native()
    return irdu_amd


def rel(a, b, floor=None):
    """max-abs error over max-abs reference; a reference below 1e-6 of `floor` (the scale of the terms that
    cancel in it) is those terms' rounding and no scale: the error is then measured against the floor."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    scale = float(b.abs().max())
    if floor is not None and scale < 1e-6 * floor:
        scale = floor
    return float((a - b).abs().max()) / max(scale, 1e-30)


def _module(irdu, cls, seed, case=FIRST):
    torch.manual_seed(seed)
    m = getattr(irdu, cls)(case[2], case[1], 1.0)
    perturbed_graph_module(m, seed + 1)
    return m


def _ref_params(m):
    """The module's parameters as float64 leaves keyed like the oracle's parameter dicts."""
    return {k: v.detach().cpu().double().clone().requires_grad_(True) for k, v in m.state_dict().items()}


def _hip_grads(m, fn, inputs, gout):
    ins = [t.to(DEV).requires_grad_(True) for t in inputs]
    m = m.to(DEV)
    for p in m.parameters():
        p.grad = None
    out = fn(m, *ins)
    out.backward(gout.to(DEV))
    torch.cuda.synchronize()
    return out, [t.grad for t in ins], {k: p.grad for k, p in m.named_parameters() if p.grad is not None}


def _check(case, out, ref_out, gin, ref_in, gp, ref_p, tol=2e-5, out_floor=None, gin_floors=None):
    b, _, _, h, w = case
    n = b * h * w
    errs = {"out": (rel(out, ref_out, out_floor), 1e-5)}
    for i, (a, r) in enumerate(zip(gin, ref_in)):
        assert bool(torch.isfinite(a).all())
        errs[f"gin{i}"] = (rel(a, r, gin_floors[i] if gin_floors else None), tol)
    for k, g in gp.items():
        r = ref_p[k].grad
        err = float((g.detach().double().cpu() - r).abs().max())
        errs[k.replace("stats_kernel_", "")] = (err / max(float(r.abs().max()), n ** 0.5), tol)
        if case == FIRST:
            assert rel(g, r) <= tol, k
    print("\n" + " ".join(f"{k}={e:.2e}" for k, (e, _) in errs.items()))
    bad = {k: v for k, v in errs.items() if not v[0] <= v[1]}
    assert not bad, bad


@cases
def test_get_neighbors_pixels_grad(irdu, case):
    b, g, f, h, w = case
    m = _module(irdu, "GLRFast", 1, case)
    x = rand(b, g * f, h, w, seed=2)
    gout = rand(b, g * f, 4, h, w, seed=3)
    out, gin, _ = _hip_grads(m, lambda mm, a: mm.get_neighbors_pixels(a), [x], gout)
    xr = x.double().requires_grad_(True)
    ref = O.gather_neighbors(xr)
    ref.backward(gout.double())
    _check(case, out, ref, gin, [xr.grad], {}, {})


@pytest.mark.parametrize("case", CASES + [ROWS_BG], ids=ids)
def test_normalize_and_transform_features_grad(irdu, case):
    b, g, f, h, w = case
    m = _module(irdu, "GLRFast", 4, case)
    f5 = rand(b, g, f, h, w, seed=5)
    zero = torch.zeros(b, g, 1, h, w, dtype=torch.bool)
    if h * w > 1:                                     # a zero feature vector (|f| below eps)
        zero[(0, 1, 0, 2, 3) if case == FIRST else (0, g - 1, 0, h - 1, w - 1)] = True
    zero = zero.expand_as(f5)
    with torch.no_grad():
        f5[zero] = 0.0
    gout = rand(b, g * f, h, w, seed=6)
    out, gin, gp = _hip_grads(m, lambda mm, a: mm.normalize_and_transform_features(a), [f5], gout)
    p = _ref_params(m)
    fr = f5.double().requires_grad_(True)
    ref = O.normalize_features(fr, p["multiM"])
    ref.backward(gout.double())
    _check(case, out, ref, gin, [fr.grad], gp, p)
    # the zero vector's gradient is gy / 1e-12 and sets the scale above: every other pixel on its own.  F = 1:
    # (gy - y (y . gy)) / |f| is identically zero there (y = +-1), held to 2e-5 of the un-projected max |gy| / |f|
    gf, gr = gin[0].detach().cpu().double(), fr.grad
    floor = None
    if f == 1:
        gy = gout.double().view(b, g, f, h, w) * p["multiM"].detach()[None, :, :, None, None]
        floor = float((gy.abs() / f5.double().abs().clamp_min(1e-12))[~zero].max())
        assert float(gr[~zero].abs().max()) < 1e-9 * floor
    e = rel(gf[~zero], gr[~zero], floor)
    print(f"gfeat(nonzero)={e:.2e}")
    assert e <= 2e-5
    if bool(zero.any()):
        assert rel(gf[zero], gr[zero]) <= 2e-5
        assert f == 1 or float(gr[zero].abs().max()) > 1e6 * float(gr[~zero].abs().max())


@pytest.mark.parametrize("transpose", [False, True])
@cases
def test_stats_conv_grad(irdu, case, transpose):
    b, g, f, h, w = case
    m = _module(irdu, "GTVFast", 7, case)
    x5 = rand(b, g, f, h, w, seed=8)
    gout = rand(b, g, f, h, w, seed=9)
    fn = (lambda mm, a: mm.stats_conv_transpose(a)) if transpose else (lambda mm, a: mm.stats_conv(a))
    out, gin, gp = _hip_grads(m, fn, [x5], gout)
    p = _ref_params(m)
    xr = x5.double().requires_grad_(True)
    k = O.stats_kernel(p, "")
    ref = O.stats_conv_t(xr, k) if transpose else O.stats_conv(xr, k)
    ref.backward(gout.double())
    _check(case, out, ref, gin, [xr.grad], gp, p)


def _weights(seed, case=FIRST):
    b, g, _, h, w = case
    return torch.softmax(rand(b, g, 4, h, w, seed=seed, scale=2.0), dim=2)


@cases
def test_op_L_norm_grad(irdu, case):
    b, g, f, h, w = case
    m = _module(irdu, "GLRFast", 10, case)
    x5, wt = rand(b, g, f, h, w, seed=11), _weights(12, case)
    gout = rand(b, g, f, h, w, seed=13)
    out, gin, _ = _hip_grads(m, lambda mm, a, c: mm.op_L_norm(a, c), [x5, wt], gout)
    xr, wr = x5.double().requires_grad_(True), wt.double().requires_grad_(True)
    nb = O.gather_neighbors(xr.reshape(b, g * f, h, w)).view(b, g, f, 4, h, w)
    ref = xr - torch.einsum("bgfehw,bgehw->bgfhw", nb, wr)    # REF:222-226
    ref.backward(gout.double())
    # 1 x 1 image: out = x (1 - sum_e w_e) and gx = g (1 - sum_e w_e) are identically zero (the terms: x, g)
    _check(case, out, ref, gin, [xr.grad, wr.grad], {}, {}, out_floor=float(x5.abs().max()),
           gin_floors=[float(gout.abs().max()), None])


@cases
def test_op_C_grad(irdu, case):
    b, g, f, h, w = case
    m = _module(irdu, "GTVFast", 14, case)
    x5, wt = rand(b, g, f, h, w, seed=15), _weights(16, case)
    gout = rand(b, g, f, 4, h, w, seed=17)
    out, gin, gp = _hip_grads(m, lambda mm, a, c: mm.op_C(a, c), [x5, wt], gout)
    p = _ref_params(m)
    xr, wr = x5.double().requires_grad_(True), wt.double().requires_grad_(True)
    k = O.stats_kernel(p, "")
    ref = O.gtv_C(xr, wr, k)
    ref.backward(gout.double())
    # 1 x 1 image: E_e = w_e (s - s(clamp)) and all its gradients are identically zero; the terms that cancel are
    # w_e s (out), gE_e s (gw) and S* of w_e gE_e (gx)
    with torch.no_grad():
        smax = float(O.stats_conv(x5.double(), k).abs().max())
        wmax, gmax, kl1 = float(wt.max()), float(gout.abs().max()), float(k.abs().sum(dim=(1, 2, 3)).max())
    _check(case, out, ref, gin, [xr.grad, wr.grad], gp, p, out_floor=wmax * smax,
           gin_floors=[wmax * gmax * kl1, gmax * smax])


@cases
def test_op_C_transpose_grad(irdu, case):
    b, g, f, h, w = case
    m = _module(irdu, "GTVFast", 18, case)
    e6, wt = rand(b, g, f, 4, h, w, seed=19), _weights(20, case)
    gout = rand(b, g, f, h, w, seed=21)
    out, gin, gp = _hip_grads(m, lambda mm, a, c: mm.op_C_transpose(a, c), [e6, wt], gout)
    p = _ref_params(m)
    er, wr = e6.double().requires_grad_(True), wt.double().requires_grad_(True)
    ref = O.gtv_Ct(er, wr, O.stats_kernel(p, ""))
    ref.backward(gout.double())
    _check(case, out, ref, gin, [er.grad, wr.grad], gp, p)


def test_plane_limits(irdu):
    """65536 rows (grid.y) are refused by every reverse entry point, F = 17 by normalize_features_bwd, and its
    message names the limit that was passed."""
    from irdu_amd import kernels as K
    from irdu_amd._native import GrrError
    n = 65536
    e = lambda *s: torch.zeros(*s, device=DEV)   # noqa: E731
    m = _module(irdu, "GTVFast", 30, (n, 1, 1, 1, 1)).to(DEV)
    st = K.stencil(m)
    x5, w4, e6 = e(n, 1, 1, 1, 1), e(n, 1, 4, 1, 1), e(n, 1, 1, 4, 1, 1)
    gtaps = e(1, 5)
    refused = {
        "neighbor_gather_bwd": lambda: K.neighbor_gather_bwd(e(n, 1, 4, 1, 1)),
        "normalize_features_bwd": lambda: K.normalize_features_bwd(x5, e(1, 1), x5.clone(), e(1, 1)),
        "stats_conv_bwd": lambda: K.stats_conv_bwd(x5, st, False, x5.clone(), gtaps),
        "stats_conv_bwd-t": lambda: K.stats_conv_bwd(x5, st, True, x5.clone(), gtaps),
        "glr_op_L_norm_bwd": lambda: K.glr_op_L_norm_bwd(x5, w4, x5.clone()),
        "gtv_op_C_bwd": lambda: K.gtv_op_C_bwd(x5, w4, st, e6, gtaps),
        "gtv_op_C_transpose_bwd": lambda: K.gtv_op_C_transpose_bwd(e6, w4, st, x5, x5.clone(), gtaps),
    }
    for name, fn in refused.items():
        with pytest.raises(GrrError) as info:
            fn()
        assert "F > 16" not in str(info.value), name
    torch.cuda.synchronize()
    assert float(gtaps.abs().max()) == 0.0
    with pytest.raises(GrrError, match="F > 16"):
        K.normalize_features_bwd(e(1, 1, 17, 2, 2), e(1, 17), e(1, 1, 17, 2, 2), e(1, 17))


def test_sub_api_composition_matches_forward_grads(irdu):
    """The reference composes the methods into GTVFast.forward = op_C_transpose(op_C(x)) (REF:518-523):
    differentiating the composition equals differentiating the fused forward."""
    m = _module(irdu, "GTVFast", 22).to(DEV)
    x5, w = rand(B, G, F, H, W, seed=23).to(DEV), _weights(24).to(DEV)
    gout = rand(B, G, F, H, W, seed=25).to(DEV)
    grads = []
    for fn in (lambda a, b: m.op_C_transpose(m.op_C(a, b), b), lambda a, b: m(a, b)):
        xa, wa = x5.clone().requires_grad_(True), w.clone().requires_grad_(True)
        for p in m.parameters():
            p.grad = None
        fn(xa, wa).backward(gout)
        grads.append([xa.grad, wa.grad] + [p.grad for p in m.parameters() if p.grad is not None])
    for a, b in zip(*grads):
        assert rel(a, b) <= 2e-5
