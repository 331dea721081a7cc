"""The pointwise and reduction kernels of the LocalNonLinearBlock / FeedForward reverse (csrc/lnb_bwd.hip), each
entry point through irdu_amd.kernels against the float64 references of tests/lnb_bwd_ref.py
(tests/test_lnb_bwd_ref.py checks on the CPU what the cases reach):

  grr_lnb_norm, grr_lnb_norm_bwd, grr_lnb_norm_bwd_skip   C = 2, C % 8 != 0, P = 1, several reduction chunks per
                                                          plane with B > 1 (chunk_slot, the B * chunks slot plan),
                                                          B*C = 65535 accepted and 65536 refused, accumulating
                                                          outputs pre-filled, a channel mean 800 x the spread
  grr_lnb_gate, grr_lnb_gate_bwd_scaled                   1 element ... 1.08 M (a second turn of the 4096-block
                                                          grid-stride loop), m = +-100 (expf overflows)
  grr_lnb_dw3_gate, grr_lnb_gate_dw3_bwd,                 the same extreme values through the fused row kernels;
  grr_ffn_dw3_gate, grr_ffn_gate_dw3_bwd                  grr_lnb_gate_dw3_bwd with hp given (dw3_gate_row_bwd_kernel
                                                          <V, false>) at V = 1, 2, 4 and in strips
  misaligned contiguous operands                          the table in test_misaligned_* below

Bounds (the project's own): element-wise outputs max-abs error over max-abs reference <= 2e-6 (n, isd, gate, gx,
the depthwise outputs) and <= 2e-5 (ghp, gh, gwdw), the pair of test_gpu_dwconv.py; sums (gln_w, gskip0, gdot)
error <= 2e-5 max(max|ref|, sqrt(N)), N the number of summed terms, the rule of test_gpu_term_oracle.py; the fused
row kernels' gdot <= 2e-5 sum |gq gate| as test_gate_dw3_rows_vs_autograd.  The ill-conditioned norm case is held
to 4 x the error of the same formulas in fp32 on the CPU + 1e-7 (test_ffblock_matches_float64's rule).

Measured on an MI355X, worst over all benign cases, in units of each bound's scale: n 2.3e-7, isd 2.8e-7, gx 2.3e-7,
gate 1.2e-7, depthwise out 1.4e-7 (bound 2e-6); ghp 2.6e-7, gh 2.1e-7, gwdw 2.6e-7 (2e-5); gln_w 1.4e-7, gskip0 3.2e-7,
gdot 7.9e-7 (2e-5); gh with hp given against the recomputing call 1.7e-7 (2e-6): every output is 7x or more inside
its bound, and no benign case needed the fp32-evaluation rule.  The ill-conditioned case: gx 7.2e-5 against
4 x 7.2e-5 + 1e-7 (the kernel's error is the fp32 formula's), n 1.2e-7, isd 8.7e-8, gln_w 8.5e-8, gskip0 1.4e-9, each
below a tenth of its bound.

Left out: the grid-stride loops of ln_fwd_kernel, ln_bwd_kernel and gate_kernel start above 65536 x 256 = 16.7 M
pixels or elements, too large for a test of a few seconds.  Which of two kernels served a misaligned operand
cannot be read from the result (both compute the same sums); the tests hold the result to float64 either way.
"""
import pytest
import torch

from tests import lnb_bwd_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
ETOL = 2e-6       # n, isd, gate, gx, depthwise outputs
GTOL = 2e-5       # ghp, gh, gwdw
STOL = 2e-5       # sums, times max(max|ref|, sqrt(N))
SENTINEL = -777.25


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import irdu_amd
    irdu_amd.load_native()
    from irdu_amd import kernels
    return kernels


def dv(t):
    return t.to(DEV).contiguous()


def added(t, pre):
    """What a kernel added to a pre-filled fp32 accumulator (float64, CPU)."""
    return t.detach().cpu().double() - pre.double().reshape(t.shape)


def _hold(errs):
    """errs: name -> (error, bound).  Print every figure, then assert."""
    print("\n" + " ".join(f"{k}={e:.2e}/{b:.1e}" for k, (e, b) in errs.items()))
    bad = {k: v for k, v in errs.items() if not v[0] <= v[1]}
    assert not bad, bad


def _mis(t, off=1):
    """t as a contiguous device view `off` floats past a 32-byte boundary."""
    whole = torch.full((t.numel() + off + 8,), SENTINEL, dtype=torch.float32, device=DEV)
    v = whole[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 32 == 4 * off
    return v


def _call(name, *args):
    from irdu_amd._native import call
    call(name, *[a.data_ptr() if torch.is_tensor(a) else a for a in args], torch.cuda.current_stream().cuda_stream)


def _ids(fmt):
    return lambda s: fmt.format(*s)


# ---- the norm ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.NORM_SHAPES + [R.NORM_LIMIT], ids=_ids("b{}c{}h{}w{}"))
def test_lnb_norm_forward(K, shape):
    d, ref = R.norm_inputs(shape), R.norm_ref(shape)
    n, isd = K.lnb_norm(dv(d.x), dv(d.ln_w))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(n).all()) and bool(torch.isfinite(isd).all())
    _hold(dict(n=(R.elem_err(n, ref.n), ETOL), isd=(R.elem_err(isd, ref.isd), ETOL)))


@pytest.mark.parametrize("shape", R.NORM_SHAPES, ids=_ids("b{}c{}h{}w{}"))
def test_lnb_norm_bwd(K, shape):
    """gx and gln_w accumulate: both pre-filled with random values, what was added is compared.  isd is the
    reference's, rounded to fp32, so the reverse is measured on its own."""
    b, c, h, w = shape
    d, ref = R.norm_inputs(shape), R.norm_ref(shape)
    gx, glw = dv(d.pre_gx), dv(d.pre_gln_w)
    K.lnb_norm_bwd(dv(d.x), dv(d.ln_w), dv(ref.isd.float()), dv(d.gn), gx, glw)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(gx).all()) and bool(torch.isfinite(glw).all())
    _hold(dict(gx=(R.elem_err(added(gx, d.pre_gx), ref.gx), ETOL),
               gln_w=(R.sum_err(added(glw, d.pre_gln_w), ref.gln_w, b * h * w), STOL)))


@pytest.mark.parametrize("shape", R.NORM_SHAPES, ids=_ids("b{}c{}h{}w{}"))
def test_lnb_norm_bwd_skip(K, shape):
    """The fused tail: gx = s0 gout + (the norm's data gradient) is written; gln_w and gskip0 = <gout, x>
    accumulate and are pre-filled."""
    b, c, h, w = shape
    d, ref = R.norm_inputs(shape), R.norm_ref(shape)
    glw, gs = dv(d.pre_gln_w), dv(d.pre_gskip0)
    gx = K.lnb_norm_bwd_skip(dv(d.x), dv(d.ln_w), dv(ref.isd.float()), dv(d.gn), dv(d.gout), dv(d.skip), glw, gs)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(gx).all())
    _hold(dict(gx=(R.elem_err(gx, ref.gx_skip), ETOL),
               gln_w=(R.sum_err(added(glw, d.pre_gln_w), ref.gln_w, b * h * w), STOL),
               gskip0=(R.sum_err(added(gs, d.pre_gskip0), ref.gskip0, b * c * h * w), STOL)))


def test_norm_reverses_refuse_65536_planes(K):
    """B*C = 65536 (grid.y of ln_wgrad_kernel): both reverses raise and leave their outputs untouched."""
    from irdu_amd._native import GrrError
    b, c, h, w = R.NORM_LIMIT
    d, ref = R.norm_inputs(R.NORM_LIMIT), R.norm_ref(R.NORM_LIMIT)
    x, lw, isd, gn, gout, skip = (dv(t) for t in (d.x, d.ln_w, ref.isd.float(), d.gn, d.gout, d.skip))
    gx, glw, gs = (torch.full(s, SENTINEL, device=DEV) for s in (R.NORM_LIMIT, (c,), (1,)))
    with pytest.raises(GrrError):
        _call("grr_lnb_norm_bwd", x, lw, isd, gn, gx, glw, b, c, h * w)
    with pytest.raises(GrrError):
        _call("grr_lnb_norm_bwd_skip", x, lw, isd, gn, gout, skip, gx, glw, gs, b, c, h * w)
    torch.cuda.synchronize()
    for t in (gx, glw, gs):
        assert bool((t == SENTINEL).all())


def test_lnb_norm_with_a_mean_800_times_the_spread(K):
    """x = 40 + 0.05 randn.  The norm is not centred: dot = sum w gn x is 800 x what survives the subtraction of
    (x - mean) k from ln_w gn isd, and x - mean keeps 1e-4 of fp32's digits.  Bound: 4 x the error of
    lnb_bwd_ref.norm_*_formula in fp32 on the CPU against float64, + 1e-7, per output in its own measure."""
    shape = R.NORM_ILL
    b, c, h, w = shape
    d, ref = R.norm_inputs(shape, True), R.norm_ref(shape, True)
    isd32 = ref.isd.float()
    n_c, isd_c = R.norm_forward_formula(d.x, d.ln_w)
    gx_c, glw_c, _ = R.norm_reverse_formula(d.x, d.ln_w, isd32, d.gn)
    gxs_c, _, gs_c = R.norm_reverse_formula(d.x, d.ln_w, isd32, d.gn, d.gout, R.SKIP[0])
    x, lw, isd, gn = dv(d.x), dv(d.ln_w), dv(isd32), dv(d.gn)
    n, isd_k = K.lnb_norm(x, lw)
    gx, glw = dv(d.pre_gx), dv(d.pre_gln_w)
    K.lnb_norm_bwd(x, lw, isd, gn, gx, glw)
    glw2, gs = dv(d.pre_gln_w), dv(d.pre_gskip0)
    gxs = K.lnb_norm_bwd_skip(x, lw, isd, gn, dv(d.gout), dv(d.skip), glw2, gs)
    torch.cuda.synchronize()
    np_, nt = b * h * w, b * c * h * w
    b4 = lambda e: 4.0 * e + 1e-7   # noqa: E731
    _hold(dict(
        n=(R.elem_err(n, ref.n), b4(R.elem_err(n_c, ref.n))),
        isd=(R.elem_err(isd_k, ref.isd), b4(R.elem_err(isd_c, ref.isd))),
        gx=(R.elem_err(added(gx, d.pre_gx), ref.gx), b4(R.elem_err(gx_c, ref.gx))),
        gln_w=(R.sum_err(added(glw, d.pre_gln_w), ref.gln_w, np_), b4(R.sum_err(glw_c, ref.gln_w, np_))),
        gx_skip=(R.elem_err(gxs, ref.gx_skip), b4(R.elem_err(gxs_c, ref.gx_skip))),
        gln_w_skip=(R.sum_err(added(glw2, d.pre_gln_w), ref.gln_w, np_), b4(R.sum_err(glw_c, ref.gln_w, np_))),
        gskip0=(R.sum_err(added(gs, d.pre_gskip0), ref.gskip0, nt), b4(R.sum_err(gs_c, ref.gskip0, nt)))))


# ---- the LNB gate -----------------------------------------------------------------------------------------------
def _gate_all(K, shape, extreme):
    b, hid, h, w = shape
    d, ref = R.gate_inputs(shape, extreme), R.gate_ref(shape, extreme)
    hp, g, sc = dv(d.hp), dv(d.g), dv(d.scale)
    gate_f, none = K.lnb_gate(hp)                                 # forward only
    gate_b, ghp_b = K.lnb_gate(hp, g)                             # forward with the reverse
    none2, ghp_r = K.lnb_gate(hp, g, want_gate=False)             # reverse only
    gdot = dv(d.pre_gdot)
    ghp_s = K.lnb_gate_bwd_scaled(hp, g, sc, gdot)
    torch.cuda.synchronize()
    assert none is None and none2 is None
    for t in (gate_f, gate_b, ghp_b, ghp_r, ghp_s, gdot):
        assert bool(torch.isfinite(t).all())
    _hold(dict(gate=(R.elem_err(gate_f, ref.gate), ETOL), gate_with_rev=(R.elem_err(gate_b, ref.gate), ETOL),
               ghp_with_gate=(R.elem_err(ghp_b, ref.ghp), GTOL), ghp=(R.elem_err(ghp_r, ref.ghp), GTOL),
               ghp_scaled=(R.elem_err(ghp_s, ref.ghp_s), GTOL),
               gdot=(R.sum_err(added(gdot, d.pre_gdot), ref.gdot, b * hid * h * w), STOL)))


@pytest.mark.parametrize("shape", R.GATE_SHAPES, ids=_ids("b{}hid{}h{}w{}"))
def test_lnb_gate_and_reverses(K, shape):
    _gate_all(K, shape, False)


def test_lnb_gate_at_extreme_values(K):
    """m in {-100, -30, -1e-3, 0, 1e-3, 30, 100}: expf(-m) is inf at -100, the sigmoid 0 and every product
    finite.  The measure is max-abs over max-abs, so a denormal flushed to zero passes."""
    _gate_all(K, R.GATE_EXTREME, True)


def _fused_bwd(K, ffn, hp, gq, sc, hh, wdw, gw, gdot):
    if ffn:
        return K.ffn_gate_dw3_bwd(gq, sc, hh, wdw, gw, gdot)
    return K.lnb_gate_dw3_bwd(hp, gq, sc, hh, wdw, gw, gdot)


def _fused_errs(ref, gh, gw, gdot):
    return dict(gh=(R.elem_err(gh, ref.gh), GTOL), gwdw=(R.elem_err(gw, ref.gwdw), GTOL),
                gdot=(abs(float(gdot) - float(ref.gdot)) / ref.gabs, STOL))


@pytest.mark.parametrize("kind", ["lnb-ring", "lnb-register", "ffn"])
def test_fused_gate_rows_at_extreme_values(K, kind):
    """The same values through the fused depthwise + gate row kernels of both blocks (W = 16), the depthwise
    taps 1 at the centre and 0 elsewhere so that the depthwise output is hh itself."""
    ffn = kind == "ffn"
    d, ref = R.fused_inputs(R.GATE_EXTREME, True), R.fused_ref(R.GATE_EXTREME, ffn, True)
    hh, wdw, gq, sc = dv(d.hh), dv(d.wdw), dv(d.gq), dv(d.scale)
    gw, gdot = torch.zeros_like(wdw), torch.zeros(1, device=DEV)
    K.set_lnb_bwd_ring(kind != "lnb-register")
    try:
        gate = (K.ffn_dw3_gate if ffn else K.lnb_dw3_gate)(hh, wdw)
        gh = _fused_bwd(K, ffn, None, gq, sc, hh, wdw, gw, gdot)
        torch.cuda.synchronize()
    finally:
        K.set_lnb_bwd_ring(True)
    for t in (gate, gh, gw, gdot):
        assert bool(torch.isfinite(t).all())
    _hold(dict(gate=(R.elem_err(gate, ref.gate), ETOL), **_fused_errs(ref, gh, gw, gdot)))


@pytest.mark.parametrize("shape", R.HP_SHAPES, ids=_ids("b{}hid{}h{}w{}"))
def test_gate_dw3_bwd_with_hp_given(K, shape):
    """grr_lnb_gate_dw3_bwd with the stored depthwise output (dw3_gate_row_bwd_kernel<V, false>; V = 1, 2, 4 and
    strips): the bounds of test_gate_dw3_rows_vs_autograd, and gh within 2e-6 of the call that recomputes hp."""
    d, ref = R.fused_inputs(shape), R.fused_ref(shape)
    hh, wdw, gq, sc = dv(d.hh), dv(d.wdw), dv(d.gq), dv(d.scale)
    hp = K.dwconv3(hh, wdw)
    gw, gdot = torch.zeros_like(wdw), torch.zeros(1, device=DEV)
    gh = K.lnb_gate_dw3_bwd(hp, gq, sc, hh, wdw, gw, gdot)
    gw0, gdot0 = torch.zeros_like(wdw), torch.zeros(1, device=DEV)
    gh0 = K.lnb_gate_dw3_bwd(None, gq, sc, hh, wdw, gw0, gdot0)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(gh).all())
    _hold(dict(vs_recomputed=(R.elem_err(gh, gh0.cpu().double()), 2e-6), **_fused_errs(ref, gh, gw, gdot)))


# ---- misaligned, contiguous operands ----------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["g", "h"])
@pytest.mark.parametrize("shape", [(1, 3, 9, 100), (1, 2, 7, 200)], ids=_ids("b{}c{}h{}w{}"))
def test_misaligned_dwconv3_falls_back_to_the_per_pixel_kernels(K, shape, which):
    """Contiguous operands at a storage offset, read from the entry points of csrc/lnb_bwd.hip (V = the row
    kernels' columns per lane: 1 for W <= 64, 2 for even W <= 128, else 4 for W % 4 == 0):

    entry point                vector accesses on a caller's pointer              misaligned operand
    grr_dwconv3 /              4 V-byte row loads of g, h, row stores of out /     dw3_row_ok declines: the
    grr_dwconv3_bwd              gh (dw3_row_*_kernel)                             per-pixel kernels (scalar)
    grr_lnb_gate_dw3_bwd       4 V-byte row loads of hp, gq, hh, stores of gh;     below 4 V bytes: GrrError;
      (hp NULL)                  ring kernel: 16-byte LDS-DMA of gq, hh rows;      gq, hh below 16: the register
                                 V = 8 instance (256 < W <= 512, W % 8 == 0):      kernel<V>; gq, hh, gh below 32:
                                 32-byte rows of gq, hh, gh                        the V = 4 strips
    grr_lnb_dw3_gate /         4 V-byte row loads of hh, stores of gate            GrrError, outputs untouched
    grr_ffn_dw3_gate
    grr_ffn_gate_dw3_bwd       4 V-byte row loads of gq, hh, stores of gh          GrrError, outputs untouched

    Here: g or h one float off at W = 100 (V = 2) and W = 200 (V = 4); the results are held to float64 within the
    bounds of test_dwconv3_forward_and_reverse_vs_autograd, gwdw pre-filled."""
    d, ref = R.dw3_inputs(shape), R.dw3_case_ref(shape)
    h = _mis(d.h) if which == "h" else dv(d.h)
    g = _mis(d.g) if which == "g" else dv(d.g)
    wdw, gw = dv(d.wdw), dv(d.pre_gwdw)
    out = K.dwconv3(h, wdw)
    gh = K.dwconv3_bwd(g, h, wdw, gw)
    torch.cuda.synchronize()
    _hold(dict(out=(R.elem_err(out, ref.out), ETOL), gh=(R.elem_err(gh, ref.gh), ETOL),
               gwdw=(R.elem_err(added(gw, d.pre_gwdw), ref.gwdw), GTOL)))


RING_DECLINES = [((1, 2, 9, 32), 1, "gq"), ((1, 2, 9, 32), 1, "hh"),        # ring -> register kernel, V = 1
                 ((1, 2, 6, 100), 2, "gq"), ((1, 2, 6, 100), 2, "hh"),      # ring -> register kernel, V = 2
                 ((1, 1, 5, 512), 4, "gq"), ((1, 1, 5, 512), 4, "hh"), ((1, 1, 5, 512), 4, "gh")]   # V = 8 -> V = 4


@pytest.mark.parametrize("shape,off,which", RING_DECLINES, ids=lambda v: str(v).replace(" ", ""))
def test_misaligned_gate_dw3_bwd_declines_to_the_narrower_kernel(K, shape, off, which):
    """grr_lnb_gate_dw3_bwd(NULL hp, ...) with one operand aligned for its row accesses but not for the wider
    kernel's (the table above): float64 within the bounds of test_gate_dw3_rows_vs_autograd.  gh is an output the
    wrapper allocates, so the entry point is called directly."""
    b, hid, h, w = shape
    d, ref = R.fused_inputs(shape), R.fused_ref(shape)
    t = dict(gq=dv(d.gq), hh=dv(d.hh), gh=torch.full(d.hh.shape, SENTINEL, device=DEV))
    t[which] = _mis(t[which], off)
    wdw, sc = dv(d.wdw), dv(d.scale)
    gw, gdot = torch.zeros_like(wdw), torch.zeros(1, device=DEV)
    _call("grr_lnb_gate_dw3_bwd", None, t["gq"], sc, t["hh"], wdw, t["gh"], gw, gdot, b, hid, h, w)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(t["gh"]).all())
    _hold(_fused_errs(ref, t["gh"], gw, gdot))


REFUSALS = [("grr_lnb_dw3_gate", "hh"), ("grr_lnb_dw3_gate", "gate"), ("grr_ffn_dw3_gate", "hh"),
            ("grr_ffn_dw3_gate", "gate"), ("grr_lnb_gate_dw3_bwd", "hp"), ("grr_lnb_gate_dw3_bwd", "gq"),
            ("grr_lnb_gate_dw3_bwd", "hh"), ("grr_lnb_gate_dw3_bwd", "gh"), ("grr_ffn_gate_dw3_bwd", "gq"),
            ("grr_ffn_gate_dw3_bwd", "hh"), ("grr_ffn_gate_dw3_bwd", "gh")]


@pytest.mark.parametrize("name,which", REFUSALS, ids=lambda v: str(v))
def test_fused_gate_entry_points_refuse_a_misaligned_plane(K, name, which):
    """W = 100 (V = 2: 8-byte row accesses), one operand one float off: GrrError, and the output buffers, filled
    with a sentinel, are unchanged after a synchronize."""
    from irdu_amd._native import GrrError
    shape = (1, 2, 6, 100)
    b, hid, h, w = shape
    d = R.fused_inputs(shape)
    t = dict(hh=dv(d.hh), gq=dv(d.gq), hp=dv(R.dw3_ref(d.hh, d.wdw)),
             gate=torch.full(d.gq.shape, SENTINEL, device=DEV), gh=torch.full(d.hh.shape, SENTINEL, device=DEV))
    t[which] = _mis(t[which])
    wdw, sc = dv(d.wdw), dv(d.scale)
    gw, gdot = torch.full_like(wdw, SENTINEL), torch.full((1,), SENTINEL, device=DEV)
    args = {"grr_lnb_dw3_gate": (t["hh"], wdw, t["gate"]), "grr_ffn_dw3_gate": (t["hh"], wdw, t["gate"]),
            "grr_lnb_gate_dw3_bwd": (t["hp"], t["gq"], sc, t["hh"], wdw, t["gh"], gw, gdot),
            "grr_ffn_gate_dw3_bwd": (t["gq"], sc, t["hh"], wdw, t["gh"], gw, gdot)}[name]
    with pytest.raises(GrrError):
        _call(name, *args, b, hid, h, w)
    torch.cuda.synchronize()
    for out in (t["gate"], t["gh"], gw, gdot):
        assert bool((out == SENTINEL).all())
