"""The window-graph reverse kernels (csrc/window_bwd.hip), one entry point at a time through the kernels.win_bwd_*
wrappers, held to the float64 references and the bounds of tests/window_bwd_ref.py: the three terms on all six
windows, Fs = 1, 2, 3, frames from 2 x 2 to a long thin 2 x 700, through the fused gather and through the E / PW planes,
each on its own; the same at 1024 planes of 33 x 33, where every plane-grid kernel takes a second, ragged grid-stride
sweep (what training at B = 16, G = 24 on 64 x 64 patches runs) and grid_red strides too; the stencils with
accumulate and scale crossed, and once past grid_1d's 65536 blocks; the tap gradients; the edge-weight reverse at
F on both sides of each FMAX boundary, at a channel offset, into pre-filled gfeat and gM; the mix; and the
validation branches of the entry points on real device tensors.  Every accumulating output starts pre-filled.
Every test prints its worst err / bound.  tests/test_window_bwd_ref.py shows on the CPU what these bounds catch."""
import ctypes

import pytest
import torch

from tests import window_bwd_ref as B

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import irdu_amd
    irdu_amd.load_native()
    from irdu_amd import kernels
    return kernels


def _d(t):
    return None if t is None else t.to(DEV).contiguous()


def _run_term(K, case, fused):
    inp = B.term_inputs(case)
    s, bt, w, sc, lg = _d(inp.s), _d(inp.bt), _d(inp.w), _d(inp.sc), _d(inp.log_gamma)
    gw, gdot, ggam = _d(inp.gw_pre).clone(), _d(inp.gdot_pre).clone(), _d(inp.ggam_pre).clone()
    saved = K.WIN_FUSED_GATHER
    try:
        K.WIN_FUSED_GATHER = fused
        if case.term == "glr":
            y, gs = K.win_bwd_glr(s, bt, w, inp.delta, sc, inp.coef, gw, gdot, case.g)
        else:
            prox = case.term == "prox"
            y, gs = K.win_bwd_gtv(s, bt, w, inp.delta, prox, lg, sc, inp.coef, gw, gdot, ggam if prox else None,
                                  case.g)
        torch.cuda.synchronize()
    finally:
        K.WIN_FUSED_GATHER = saved
    got = {"y": y, "gs": gs, "gw": gw, "gdot": gdot}
    if case.term == "prox":
        got["ggamma"] = ggam
    else:
        assert torch.equal(ggam.cpu(), inp.ggam_pre)
    return got


def _check_term(K, case, fused):
    got = _run_term(K, case, fused)
    r = B.term_ratios(case, got)
    print(f"{B.term_id(case)} {'fused' if fused else 'planes'}: err / bound " + "  ".join(f"{n} {v:.3f}" for n, v in r.items()))
    for n, v in r.items():
        assert torch.isfinite(got[n]).all(), n
        assert v <= 1.0, (n, v)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "planes"])
@pytest.mark.parametrize("case", B.TERM_CASES, ids=B.TERM_IDS)
def test_window_term_reverse_planes_vs_fp64(K, case, fused):
    """Each gather path meets the bound on its own (their equality is test_gpu_window_grad.py's)."""
    _check_term(K, case, fused)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "planes"])
@pytest.mark.parametrize("case", B.STRIDED_CASES, ids=B.STRIDED_IDS)
def test_window_term_reverse_strided_vs_fp64(K, case, fused):
    """1024 planes: 4 blocks per plane, a first sweep of 1024 pixels and a second of 65."""
    _check_term(K, case, fused)


@pytest.mark.parametrize("mode", B.STENCIL_MODES)
@pytest.mark.parametrize("hw", B.STENCIL_FRAMES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_window_stencil_reverse_vs_fp64(K, hw, mode):
    _check_stencil(K, B.stencil_refs(hw), mode, f"stencil {hw} mode {mode}")


def _check_stencil(K, r, mode, what, combos=((False, False), (False, True), (True, False), (True, True))):
    x, taps, g = _d(r.x), _d(r.taps), r.x.shape[1]
    worst = {}
    for acc, ws in combos:
        out = _d(r.pre).clone() if acc else None
        got = K.win_bwd_stencil(x, taps, mode, g, scale=_d(r.scale) if ws else None, out=out)
        torch.cuda.synchronize()
        assert not acc or got is out
        ref, bound = (r.ys64[mode], r.bound_s[mode]) if ws else (r.y64[mode], r.bound[mode])
        v = B.ratio_acc(got, r.pre, ref, bound, (-2, -1)) if acc else B.ratio(got, ref, bound, (-2, -1))
        worst[f"acc{int(acc)}scale{int(ws)}"] = v
        assert torch.isfinite(got).all()
    print(f"{what}: err / bound " + "  ".join(f"{n} {v:.3f}" for n, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


def test_window_stencil_reverse_past_65536_blocks(K):
    """B G Fs H W = 16,793,600: grid_1d stops at 65536 blocks and the last four rows belong to a second sweep."""
    r = B.grid1d_refs()
    for mode in B.STENCIL_MODES:
        _check_stencil(K, r, mode, f"stencil {B.GRID1D_SHAPE} mode {mode}", combos=((True, True),))


@pytest.mark.parametrize("case", B.TAPGRAD_CASES, ids=B.TAPGRAD_IDS)
def test_window_tapgrad_vs_fp64(K, case):
    """The last case has n = 1,115,136 elements: grid_red's 4096 blocks take a second sweep."""
    r = B.tapgrad_refs(*case)
    u, z, g = _d(r.u), _d(r.z), case[2]
    worst = 0.0
    for (mode, ws), gt in r.gt.items():
        got = _d(r.pre).clone()
        K.win_bwd_tapgrad(u, z, mode, g, _d(r.scale) if ws else None, got)
        torch.cuda.synchronize()
        assert torch.isfinite(got).all()
        v = B.sum_ratio(got, r.pre, gt, r.bound[mode, ws])
        print(f"tapgrad {B.TAPGRAD_IDS[B.TAPGRAD_CASES.index(case)]} mode {mode} scale {int(ws)}: err / bound {v:.3f}")
        worst = max(worst, v)
    assert worst <= 1.0


def _check_edge(K, case):
    e = B.edge_refs(case)
    gfeat, gM, gw = _d(e.gfeat_pre).clone(), _d(e.gM_pre).clone(), _d(e.gw_up).clone()
    K.win_bwd_edge_weights(_d(e.feat), case.offset, case.g, case.f, _d(e.multiM), _d(e.w), gw, B.delta_of(case.window),
                           gfeat, gM)
    torch.cuda.synchronize()
    r = B.edge_ratios(case, gfeat, gM)
    print(f"edge {B.edge_id(case)}: err / bound " + "  ".join(f"{n} {v:.3f}" for n, v in r.items()))
    assert torch.isfinite(gfeat).all() and torch.isfinite(gM).all()
    assert r["outside"] == 0.0                   # channels outside the slab: bitwise unchanged
    assert max(r.values()) <= 1.0, r


@pytest.mark.parametrize("case", B.EDGE_CASES, ids=B.edge_id)
def test_window_edge_weight_reverse_vs_fp64(K, case):
    _check_edge(K, case)


@pytest.mark.parametrize("case", B.STRIDED_EDGE_CASES, ids=B.edge_id)
def test_window_edge_weight_reverse_strided_vs_fp64(K, case):
    """win_feat_bwd_kernel<4> on the 1024 planes of the strided term cases: gMa carried across two sweeps."""
    _check_edge(K, case)


@pytest.mark.parametrize("fs,hw,g", B.MIX_CASES)
def test_window_mix_reverse_vs_fp64(K, fs, hw, g):
    m = B.mix_refs(fs, hw, g)
    gx, gscore = K.win_bwd_mix(_d(m.gout), _d(m.x), _d(m.score))
    torch.cuda.synchronize()
    rx = B.ratio(gx, m.gx64, m.bound_gx, (-2, -1))
    rs = B.ratio(gscore, m.gscore64, m.bound_gscore, (-2, -1))
    print(f"mix reverse Fs={fs} {hw} G={g}: err / bound  gx {rx:.3f}  gscore {rs:.3f}")
    assert torch.isfinite(gx).all() and torch.isfinite(gscore).all()
    assert rx <= 1.0 and rs <= 1.0


# ---- validation: rejected before any launch, every output untouched -------------------------------------------------
SENTINEL = -12345.0
RING = B.delta_of("ring3")
CROSS = B.delta_of("cross4")
K25 = tuple((dy, dx) for dy in range(-2, 3) for dx in range(-2, 3))
OFFSET3 = ((0, 1), (0, -1), (3, 0), (-3, 0))
ENTRIES = ("stencil", "tapgrad", "glr", "gtv", "gather", "gather_fused", "edge_weights")


def _raw(entry, b=1, g=2, fs=2, h=4, w=5, delta=RING, mode=0, prox=1, with_gamma=True, f=3):
    """The entry point with every operand present and sized for the call, outputs sentinel-filled:
    (call, outputs, their contents before the call)."""
    from irdu_amd._native import call
    flat = [v for e in delta for v in e]
    arr, k = (ctypes.c_int32 * len(flat))(*flat), len(delta)
    rnd = lambda *s: torch.randn(s, device=DEV)
    sent = lambda *s: torch.full(s, SENTINEL, device=DEV)
    sig = (b, g, fs, h, w)
    x, y, wt = rnd(*sig), rnd(*sig), torch.softmax(rnd(b, g, k, h, w), 2)
    taps, sc, lg = rnd(5), torch.rand(g, device=DEV), torch.log(0.1 + torch.rand(g, device=DEV))
    planes = rnd(b, g, fs, k, h, w)
    P = lambda t: t.data_ptr()
    if entry == "stencil":
        outs = [sent(*sig)]
        args = ("grr_win_bwd_stencil", P(x), P(taps), mode, P(sc), 0, P(outs[0]), *sig, None)
    elif entry == "tapgrad":
        outs = [sent(5)]
        args = ("grr_win_bwd_tapgrad", P(x), P(y), mode, P(sc), P(outs[0]), *sig, None)
    elif entry == "glr":
        outs = [sent(*sig), sent(*sig), sent(b, g, k, h, w), sent(g)]           # l_out, gsd, gw, gdot
        args = ("grr_win_bwd_glr", P(x), P(y), P(wt), arr, k, P(sc), -1.0, P(outs[0]), None, P(outs[1]), P(outs[2]),
                P(outs[3]), *sig, None)
    elif entry == "gtv":
        outs = [sent(*sig), sent(b, g, k, h, w), sent(g), sent(g)]              # gsd, gw, gdot, ggamma
        args = ("grr_win_bwd_gtv", P(x), P(y), P(wt), arr, k, prox, P(lg) if with_gamma else None, P(sc), 1.0, None,
                None, P(outs[0]), P(outs[1]), P(outs[2]), P(outs[3]), *sig, None)
    elif entry == "gather":
        outs = [sent(*sig), sent(*sig)]                                          # gs, o_out
        args = ("grr_win_bwd_gather", P(planes), P(planes), arr, k, P(outs[0]), P(outs[1]), *sig, None)
    elif entry == "gather_fused":
        outs = [sent(*sig), sent(*sig)]
        args = ("grr_win_bwd_gather_fused", P(x), P(y), P(wt), arr, k, 1, prox, P(lg) if with_gamma else None, P(sc),
                P(outs[0]), P(outs[1]), *sig, None)
    else:
        feat, m = rnd(b, g * f, h, w), rnd(g, f)
        outs = [rnd(b, g, k, h, w), sent(b, g * f, h, w), sent(g, f)]           # gw (an input, consumed in place), gfeat, gM
        args = ("grr_win_bwd_edge_weights", P(feat), g * f * h * w, P(m), P(wt), P(outs[0]), arr, k, P(outs[1]),
                g * f * h * w, P(outs[2]), b, g, f, h, w, None)
        x = (x, feat, m)
    keep = (x, y, wt, taps, sc, lg, planes, arr)
    before = [t.clone() for t in outs]

    def run():
        call(*args)
        return keep
    return run, outs, before


def _untouched(outs, before):
    torch.cuda.synchronize()
    return all(torch.equal(t, t0) for t, t0 in zip(outs, before))


def _written(outs, before):
    """Every output finite and changed at a quarter of its elements or more (an accumulating output keeps an
    element whose increment is zero -- gw at an axis edge that leaves a 2 x 2 frame -- or rounds away against the
    sentinel)."""
    torch.cuda.synchronize()
    return all(bool(torch.isfinite(t).all()) and float((t != t0).float().mean()) >= 0.25 for t, t0 in zip(outs, before))


SIGNAL_ENTRIES = ("stencil", "tapgrad", "glr", "gtv", "gather", "gather_fused")     # H, W >= 2 (the reflect frame)
WINDOW_ENTRIES = ("glr", "gtv", "gather", "gather_fused", "edge_weights")           # take a window
BIG = dict(b=16384, g=4, fs=1, h=2, w=2, delta=CROSS, f=1)                          # B G = 65536 blocks along y
BAD = ([(e, "H = 1", dict(h=1)) for e in SIGNAL_ENTRIES] + [(e, "W = 1", dict(w=1)) for e in SIGNAL_ENTRIES]
       + [(e, "K = 25", dict(delta=K25)) for e in WINDOW_ENTRIES]
       + [(e, "offset 3", dict(delta=OFFSET3)) for e in WINDOW_ENTRIES]
       + [("stencil", "mode 3", dict(mode=3)), ("tapgrad", "mode 2", dict(mode=2)),
          ("gtv", "prox without log_gamma", dict(with_gamma=False)),
          ("gather_fused", "prox without log_gamma", dict(with_gamma=False)),
          ("edge_weights", "F = 25", dict(f=25)),
          ("glr", "B G = 65536", BIG), ("gtv", "B G = 65536", BIG), ("edge_weights", "B G = 65536", BIG)])


@pytest.mark.parametrize("entry,what,over", BAD, ids=[f"{e}-{w}" for e, w, _ in BAD])
def test_window_reverse_rejects_before_launch(K, entry, what, over):
    """B G = 65536 on grr_win_bwd_edge_weights used to come back with gw already overwritten by the softmax reverse."""
    from irdu_amd._native import GrrError
    run, outs, before = _raw(entry, **over)
    with pytest.raises(GrrError):
        run()
    assert _untouched(outs, before), what


@pytest.mark.parametrize("entry", ENTRIES)
def test_window_reverse_accepts_the_same_call_when_valid(K, entry):
    """The harness of the rejections above is a valid call once nothing is wrong with it: it writes every output."""
    run, outs, before = _raw(entry)
    run()
    assert _written(outs, before)


@pytest.mark.parametrize("entry", ("glr", "gtv", "edge_weights"))
def test_window_reverse_accepts_the_largest_plane_count(K, entry):
    """B G = 65535 is inside the limit the rejections above sit just past (F = 2: at F = 1 the feature gradient is
    zero and would leave gfeat as it was)."""
    run, outs, before = _raw(entry, **dict(BIG, b=13107, g=5, f=2))
    run()
    assert _written(outs, before)
