"""The window-graph forward kernels (csrc/window_ops.hip), each held on its own to the float64 references and
fp32-class bounds of tests/window_ref.py: every solver family <R, ., KT> in every mode (the runtime-K families
<1, ., 0> and <2, ., 0> and the module apply on pair weights, mode 7, included), Fs = 1, 2, 3, frames from 2 x 2 to
3 x 3 tiles; the pair weights on all six windows; the edge weights on both sides of each FMAX boundary, at a
channel offset and at an all-zero feature vector; the mix; bitwise determinism; and the validation branches of the
entry points on real device tensors.  Every test prints its worst err / bound.
tests/test_window_ref.py shows on the CPU what these bounds catch."""
import ctypes

import pytest
import torch

from tests import window_ref as R

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


def _run(K, case, want_u=True):
    """The case through kernels.win_solver / win_apply -> {"out": ..., "u": ...} on the device."""
    inp = R.inputs(case)
    mode, pair = R.MODE[case.op]
    g, fs = case.g, case.fs
    wG = _d(inp.wG)
    if pair:
        wG = K.win_pair_weights(wG, inp.delta)
    if mode == 3:
        out = K.win_apply(_d(inp.x), inp.delta, g, fs, wL=_d(inp.wL), tapsL=_d(inp.tapsL) if inp.wL is not None else None,
                          mu=_d(inp.mu) if inp.wL is not None else None, wG=wG,
                          tapsG=_d(inp.tapsG) if wG is not None else None, ro=_d(inp.ro) if wG is not None else None,
                          pair=pair)
        return {"out": out}
    if mode == 0:
        out, u = K.win_solver(0, _d(inp.x), _d(inp.y), wG, _d(inp.tapsG), _d(inp.ro), inp.delta, g, fs, wL=_d(inp.wL),
                              tapsL=_d(inp.tapsL), mu=_d(inp.mu), alpha=_d(inp.alpha), beta=_d(inp.beta),
                              u_prev=_d(inp.u_prev), want_u=want_u, pair=pair)
        return {"out": out, "u": u} if want_u else {"out": out}
    out, _ = K.win_solver(mode, _d(inp.x), _d(inp.y), wG, _d(inp.tapsG), _d(inp.ro), inp.delta, g, fs,
                          log_gamma=_d(inp.log_gamma), pair=pair)
    return {"out": out}


@pytest.mark.parametrize("case", R.CASES, ids=R.IDS)
def test_window_solver_planes_vs_fp64(K, case):
    r = R.refs(case)
    got = _run(K, case)
    torch.cuda.synchronize()
    assert set(got) == set(r.out64)
    worst = {n: R.ratio(got[n], r, n) for n in r.out64}
    print(f"{R.family(case.window)} {R.case_id(case)}: err / bound " + "  ".join(f"{n} {v:.3f}" for n, v in worst.items())
          + f"   (bound <= {max(float(b.max()) for b in r.bound.values()):.2e})")
    for n, v in worst.items():
        assert torch.isfinite(got[n]).all(), n
        assert v <= 1.0, (n, v)


@pytest.mark.parametrize("window", list(R.WINDOWS))
def test_window_pair_weights_vs_fp64(K, window):
    p = R.pair_refs(window)
    c = K.win_pair_weights(_d(p.w), R.delta_of(window))
    ratio = float((R.plane_err(c, p.c64, (-3, -2, -1)) / p.bound).max())
    print(f"{window}: pair weights err / bound {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("case", R.EDGE_CASES, ids=R.EDGE_IDS)
def test_window_edge_weights_vs_fp64(K, case):
    e = R.edge_refs(case)
    w, deg = K.win_edge_weights(_d(e.feat), case.offset, case.g, case.f, _d(e.multiM), R.delta_of(case.window),
                                with_degree=True)
    rw = float((R.plane_err(w, e.w64, (-3, -2, -1)) / e.bound_w).max())
    rd = float((R.plane_err(deg, e.deg64) / e.bound_deg).max())
    print(f"{R.EDGE_IDS[R.EDGE_CASES.index(case)]}: err / bound  w {rw:.3f}  deg {rd:.3f}")
    assert rw <= 1.0 and rd <= 1.0
    k = w.shape[2]
    for b, (zy, zx) in enumerate(e.zero):                       # |f| = 0: the 1e-12 clamp, uniform weights
        assert float((w[b, :, :, zy, zx].cpu().double() - 1.0 / k).abs().max()) <= 2.0 ** -24
    w2, none = K.win_edge_weights(_d(e.feat), case.offset, case.g, case.f, _d(e.multiM), R.delta_of(case.window))
    assert none is None and torch.equal(w2, w)


def test_window_edge_weights_reject_25_features(K):
    from irdu_amd._native import GrrError
    feat = torch.randn((1, 25, 4, 4), device=DEV)
    with pytest.raises(GrrError):
        K.win_edge_weights(feat, 0, 1, 25, torch.ones(25, device=DEV), R.delta_of("ring3"))
    torch.cuda.synchronize()


@pytest.mark.parametrize("fs,hw,g,with_dc", R.MIX_CASES)
def test_window_mix_vs_fp64(K, fs, hw, g, with_dc):
    m = R.mix_refs(fs, hw, g, with_dc)
    out = K.win_mix(_d(m.x), _d(m.score), _d(m.dc))
    ratio = float((R.plane_err(out, m.out64) / m.bound).max())
    print(f"mix Fs={fs} {hw} G={g}: err / bound {ratio:.3f}")
    assert ratio <= 1.0
    assert torch.equal(K.win_mix(_d(m.x), _d(m.score), _d(m.dc)), out)


def _first(fam, op):
    return next(c for c in R.CASES if R.family(c.window) == fam and c.op == op)


def test_window_solver_without_u_is_bitwise_the_same(K):
    case = _first("r2k0", "0")
    a, b = _run(K, case, want_u=True), _run(K, case, want_u=False)
    torch.cuda.synchronize()
    assert set(b) == {"out"} and torch.equal(a["out"], b["out"])


@pytest.mark.parametrize("fam,op", [("r1k8", "2"), ("r1k0", "0"), ("r2k12", "7"), ("r2k24", "1rep"), ("r2k0", "4")])
def test_window_solver_is_deterministic(K, fam, op):
    """No atomics in the forward window kernels: two runs are bitwise equal."""
    case = _first(fam, op)
    a, b = _run(K, case), _run(K, case)
    torch.cuda.synchronize()
    for n in a:
        assert torch.equal(a[n], b[n]), n


# ---- validation: rejected before any launch, out untouched ---------------------------------------------------------
SENTINEL = -12345.0


def _delta_array(delta):
    flat = [v for e in delta for v in e]
    return (ctypes.c_int32 * len(flat))(*flat), len(delta)


def _raw_solver(K, mode, delta, b=1, g=2, fs=2, h=4, w=5):
    """grr_win_solver with every operand present and sized for the call; returns (call, out)."""
    from irdu_amd._native import call
    arr, k = _delta_array(delta)
    t = lambda *s: torch.randn(s, device=DEV)
    x, y5, y4, up = t(b, g, fs, h, w), t(b, g, fs, h, w), t(b, fs, h, w), t(b, g, fs, h, w)
    wL, wG = (torch.softmax(t(b, g, k, h, w), 2) for _ in range(2))
    taps, sc = t(5), torch.rand(g, device=DEV)
    out = torch.full((b, g, fs, h, w), SENTINEL, device=DEV)
    u = torch.full_like(out, SENTINEL)
    y = y5 if mode in (0, 4) else y4
    keep = (x, y5, y4, up, wL, wG, taps, sc, arr)

    def run():
        call("grr_win_solver", mode, x.data_ptr(), 0, y.data_ptr(), up.data_ptr(), wL.data_ptr(), wG.data_ptr(),
             taps.data_ptr(), taps.data_ptr(), sc.data_ptr(), sc.data_ptr(), sc.data_ptr(), sc.data_ptr(), sc.data_ptr(),
             arr, k, out.data_ptr(), u.data_ptr(), b, g, fs, h, w, None)
        return keep
    return run, out, u


def _untouched(*ts):
    torch.cuda.synchronize()
    return all(bool((t == SENTINEL).all()) for t in ts)


RING = R.delta_of("ring3")
BAD = {
    "mode 6": dict(mode=6, delta=RING),
    "mode 8": dict(mode=8, delta=RING),
    "Fs = 4": dict(mode=1, delta=RING, fs=4),
    "H = 1": dict(mode=1, delta=RING, h=1),
    "W = 1": dict(mode=0, delta=RING, w=1),
    "K = 25": dict(mode=1, delta=tuple((dy, dx) for dy in range(-2, 3) for dx in range(-2, 3))),
    "offset 3": dict(mode=3, delta=((0, 1), (0, -1), (3, 0), (-3, 0))),
}


@pytest.mark.parametrize("what", list(BAD))
def test_window_solver_rejects_before_launch(K, what):
    from irdu_amd._native import GrrError
    run, out, u = _raw_solver(K, **BAD[what])
    with pytest.raises(GrrError):
        run()
    assert _untouched(out, u)


def test_window_solver_accepts_the_same_call_when_valid(K):
    """The harness of the rejections above is a valid call once nothing is wrong with it."""
    run, out, u = _raw_solver(K, mode=0, delta=RING)
    run()
    torch.cuda.synchronize()
    assert bool((out != SENTINEL).all()) and bool((u != SENTINEL).all()) and torch.isfinite(out).all()


def test_window_pair_weights_reject_one_sided_window(K):
    from irdu_amd._native import GrrError, call
    delta = ((0, 1), (1, 0), (1, 1))
    w = torch.softmax(torch.randn((1, 2, 3, 4, 5), device=DEV), 2)
    with pytest.raises(GrrError):
        K.win_pair_weights(w, delta)
    arr, k = _delta_array(delta)
    c = torch.full_like(w, SENTINEL)
    with pytest.raises(GrrError):
        call("grr_win_pair_weights", w.data_ptr(), arr, k, c.data_ptr(), 1, 2, 4, 5, None)
    assert _untouched(c)


def test_window_wrappers_reject_prox_on_pair_weights_and_four_channels(K):
    g, fs, h, w = 2, 2, 4, 5
    x = torch.randn((1, g, fs, h, w), device=DEV)
    y = torch.randn((1, fs, h, w), device=DEV)
    wt = torch.softmax(torch.randn((1, g, 8, h, w), device=DEV), 2)
    taps, sc = torch.randn(5, device=DEV), torch.rand(g, device=DEV)
    with pytest.raises(ValueError):
        K.win_solver(2, x, y, K.win_pair_weights(wt, RING), taps, sc, RING, g, fs, log_gamma=sc, pair=True)
    with pytest.raises(ValueError):
        K.win_apply(torch.randn((1, g, 4, h, w), device=DEV), RING, g, 4, wG=wt, tapsG=taps, ro=sc)
    with pytest.raises(ValueError):
        K.win_apply(x, RING, g, fs, wL=wt, tapsL=taps, mu=sc, pair=True)
    torch.cuda.synchronize()
