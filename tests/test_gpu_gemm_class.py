"""Every GEMM-class kernel at its shape and dispatch edges against float64, held to the fp32-class bound
4 err32 + 1e-7 (tests/gemm_ref.py: references, bound, case tables; tests/test_gemm_ref.py proves on the CPU that
the bound rejects a kernel that drops one of its six split-bf16 products, keeps only three, or loses a pixel,
a k row or a 16-pixel step, for every case used here).

(a) test_fp32_class: every case of every table; run-to-run bitwise; a batch item equals its single-item run.
(b) test_guarded_*: operands and output inside larger tensors with NaN / sentinel guards: nothing leaks in,
    nothing is written outside; a NaN image next to a clean one does not reach it.
(c) test_misaligned_*: contiguous operands at a 1-float storage offset (the table is in that test's docstring).
(d) test_grid_stride_*: the grid-stride loops of csrc/codec_ops.hip on their second trip.
(e) test_conv2x2s2_fn_odd_sizes: Conv2x2s2Fn's forward and reverse at odd H / W.

Measured on an MI355X: the worst err / bound over each table's cases, with that case's err and bound (both sides
are deterministic, so these are the figures of every run; no case needed a bound of its own):
  table               cases  worst err / bound   at                                   err        bound
  conv1x1_x3            11        0.364          conv1x1-1x17x3x1x1                   8.29e-08   2.28e-07
  conv1x1_x3k            6        0.715          conv1x1-1x512x130x10x33              8.92e-07   1.25e-06
  conv1x1_f32            3        0.242          conv1x1_f32-1x160x40x9x10            2.69e-07   1.11e-06
  conv1x1_cat2           8        0.491          conv1x1_cat2-1x192x192x48x7x11       6.05e-07   1.23e-06
  conv2x2s2              8        0.852          conv2x2s2-1x192x384x2x2 (K = 768)    7.77e-07   9.12e-07
  conv2x2s2_bwd_data    10        0.313          conv2x2s2_bwd_data-1x96x192x2x4      4.23e-07   1.35e-06
  convt2x2s2             3        0.281          convt2x2s2-1x192x130x3x5             4.39e-07   1.56e-06
  wgrad                 21        0.405          wgrad-3x130x97x391                   4.60e-07   1.14e-06
  embed_bwd_w            6        0.396          embed_bwd_w-2x3x48x17x23             4.25e-07   1.08e-06
  embed_bwd_x            6        0.051          embed_bwd_x-1x1x5x1x1                2.30e-08   4.52e-07
  grid-stride (d)        4        0.335          convt2x2s2 1x1x1x2050x4100           7.31e-08   2.18e-07
  odd Conv2x2s2Fn (e)    9        0.228          y at (8, 13)                         2.60e-07   1.14e-06
embed_bwd_x is that low because the kernel now accumulates in fp64: with its single fp32 accumulator the
(1, 4, 128, 2, 2) case measured err 1.18e-06 against its bound 1.02e-06 (1152 terms in one chain), which this test found.
"""
import math
import time

import pytest
import torch
import torch.nn.functional as F

from tests import gemm_ref as R
from tests.gemm_ref import rand, rel_err

pytestmark = pytest.mark.gpu

DEV = "cuda"
TABLE_OF = {c.id: name for name, t in R.TABLES.items() for c in t}

# A correct kernel outside 4 err32 + 1e-7 for an accumulation-order reason: {case id: (bound, why)}.  The bound is
# at least twice the measured error and at most the case's DROP11 emulation error / 1.5 (checked below from the
# references, never from the kernel).
CASE_BOUND = {}


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import irdu_amd
    irdu_amd.load_native()
    from irdu_amd import kernels
    return kernels


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _call(name, *args):
    from irdu_amd._native import call
    call(name, *[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args], _stream())


def _lib():
    from irdu_amd import _native
    return _native.load()


def _ws(nbytes):
    return torch.empty((max(int(nbytes), 4) + 3) // 4, dtype=torch.float32, device=DEV)


def conv1x1_f32(x, w):
    """grr_conv1x1, the ABI's plain fp32 MFMA entry point (gemm_f32_kernel<LD_PLAIN>)."""
    b, k, h, ww = x.shape
    out = torch.empty(b, w.shape[0], h, ww, device=DEV)
    _call("grr_conv1x1", x, w, out, b, k, w.shape[0], h * ww)
    return out


def run(K, case, a, b):
    """{variant: result} of the case's kernel(s) on device operands (the batch is a's)."""
    op = case.op
    if op == "conv1x1":
        return {"x3": K.conv1x1(a, b)}
    if op == "conv1x1_f32":
        return {"f32": conv1x1_f32(a, b)}
    if op == "conv1x1_cat2":
        ka = case.shape[1]
        return {"cat2": K.conv1x1_cat2(a[:, :ka].contiguous(), a[:, ka:].contiguous(), b)}
    if op == "conv2x2s2":
        return {"f32": K.conv2x2s2(a, b)}
    if op == "conv2x2s2_bwd_data":
        h, w = case.shape[3:]
        out = {"direct": K.conv2x2s2_bwd_data(a, b, h, w)}
        if "both" in case.opts:
            out["gemm"] = K.conv2x2s2_bwd_data_gemm(a, b, h, w)
        return out
    if op == "convt2x2s2":
        return {"x3": K.convt2x2s2(a, b)}
    if op == "wgrad":
        return {"wgrad": K.wgrad(a, b)}
    if op == "embed_bwd_w":
        return {"wgrad": K.conv3x3_embed_bwd_w(a, b)}
    assert op == "embed_bwd_x"
    return {"direct": K.conv3x3_embed_bwd_x(a, b)}


def case_bound(case, r):
    if case.id not in CASE_BOUND:
        return r.bound
    bound, _why = CASE_BOUND[case.id]
    assert r.bound < bound <= R.mutant_errors(case)[1] / 1.5, case.id
    return bound


# ---- (a) accuracy ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.ALL_CASES, ids=[c.id for c in R.ALL_CASES])
def test_fp32_class(K, case):
    r = R.refs(case)
    a, b = r.a.to(DEV), r.b.to(DEV)
    bound = case_bound(case, r)
    tiles = "tiles0" not in case.opts
    try:
        K.set_wgrad_tiles(tiles)
        outs = run(K, case, a, b)
        again = run(K, case, a, b)
        if OPS_KIND(case) == "wgrad":
            # the mirrored plan (the table's notes) is the library's: its workspace is nchunk M K floats
            bb, m, k, p = R.wgrad_dims(case)
            plan = R.wgrad_plan(bb, m, k, p, tiles)
            assert _lib().grr_wgrad_workspace_bytes(bb, m, k, p) == bb * plan.cpi * m * k * 4, plan
        torch.cuda.synchronize()
    finally:
        K.set_wgrad_tiles(True)
    for name, got in outs.items():
        err = rel_err(got, r.ref64)
        print(f"GEMMCLASS {TABLE_OF[case.id]} {case.id} {name}: err {err:.3e}  err32 {(r.bound - 1e-7) / 4:.3e}  "
              f"bound {bound:.3e}  err/bound {err / bound:.3f}")
        assert bool(torch.isfinite(got).all())
        assert err <= bound, (name, err, bound)
        assert torch.equal(again[name], got), f"{name}: not bitwise repeatable"
    if "gemm" in outs:                       # two routes to one float64 value: within both bounds of each other
        assert rel_err(outs["direct"], outs["gemm"].double().cpu()) <= 2 * bound
    if case.op == "conv1x1_cat2":            # the stated contract: bitwise conv1x1 on the concatenation
        bb, ka, kb, m, h, w = case.shape
        assert K.conv1x1_cat2_ok(ka, kb, m, h * w)
        assert torch.equal(outs["cat2"], K.conv1x1(a, b))
    if OPS_KIND(case) == "fwd" and a.shape[0] > 1:   # an image does not see its batch
        for i in range(a.shape[0]):
            for name, got in run(K, case, a[i:i + 1].contiguous(), b).items():
                assert torch.equal(got[0], outs[name][i]), (name, i)


def OPS_KIND(case):
    return R.OPS[case.op].kind


# ---- (b) guards ----------------------------------------------------------------------------------------------
GUARD = 4096            # floats on each side; a multiple of 64, so the view stays 256-byte aligned
SENTINEL = -12345.625


def _placed(t, fill):
    """t copied into the middle of a larger tensor filled with ``fill``: (view, whole)."""
    n = t.numel()
    whole = torch.full((2 * GUARD + (n + 63) // 64 * 64,), fill, dtype=torch.float32, device=DEV)
    view = whole[GUARD:GUARD + n].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 256 == 0 and view.is_contiguous()
    return view, whole


def _guards_intact(whole, n):
    return bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[GUARD + n:] == SENTINEL).all())


# ragged everywhere: K = 27 or 200 (K % 16 != 0), M = 33 (M % 32 != 0), P = 77 or 35 (P % 32 != 0)
def _g_conv1x1_ws(k):
    def make(b):
        return [(rand(b, k, 7, 11, seed=301, scale=2.0, offset=0.3), True), (rand(33, k, seed=302) * 0.2, False)]

    def launch(ins, out, b):
        _call("grr_conv1x1_ws", ins[0], ins[1], out, _ws(_lib().grr_conv1x1_workspace_bytes(k, 33)), b, k, 33, 77)
    return make, (lambda b: (b, 33, 7, 11)), launch, True


def _g_cat2(ka, kb):
    def make(b):
        return [(rand(b, ka, 7, 11, seed=303, scale=2.0, offset=0.3), True),
                (rand(b, kb, 7, 11, seed=304, scale=2.0, offset=-0.3), True), (rand(33, ka + kb, seed=305) * 0.2, False)]

    def launch(ins, out, b):
        _call("grr_conv1x1_cat2", ins[0], ins[1], ins[2], out, _ws(_lib().grr_conv1x1_cat2_workspace_bytes(ka, kb, 33)),
              b, ka, kb, 33, 77)
    return make, (lambda b: (b, 33, 7, 11)), launch, True


def _g_conv2x2s2():
    def make(b):
        return [(rand(b, 3, 10, 14, seed=306, scale=2.0, offset=0.3), True), (rand(33, 3, 2, 2, seed=307) * 0.2, False)]

    def launch(ins, out, b):
        _call("grr_conv2x2s2", ins[0], ins[1], out, b, 3, 33, 10, 14)
    return make, (lambda b: (b, 33, 5, 7)), launch, True


def _g_convt2x2s2():
    def make(b):
        return [(rand(b, 27, 5, 7, seed=308, scale=2.0, offset=0.3), True), (rand(27, 5, 2, 2, seed=309) * 0.2, False)]

    def launch(ins, out, b):
        _call("grr_convt2x2s2", ins[0], ins[1], out, _ws(_lib().grr_convt2x2s2_workspace_bytes(b, 27, 5, 5, 7)),
              b, 27, 5, 5, 7)
    return make, (lambda b: (b, 5, 10, 14)), launch, True


def _g_wgrad():
    def make(b):
        return [(rand(b, 33, 77, seed=310, scale=2.0, offset=0.3), True), (rand(b, 27, 77, seed=311, scale=2.0, offset=0.3), True)]

    def launch(ins, out, b):
        _call("grr_wgrad", ins[0], ins[1], out, _ws(_lib().grr_wgrad_workspace_bytes(b, 33, 27, 77)), b, 33, 27, 77)
    return make, (lambda b: (33, 27)), launch, False


def _g_embed():
    def make(b):
        return [(rand(b, 3, 5, 7, seed=312, scale=2.0, offset=0.3), True), (rand(33, 3, 3, 3, seed=313) * 0.3, False)]

    def launch(ins, out, b):
        _call("grr_conv3x3_embed", ins[0], ins[1], out, b, 3, 33, 5, 7)
    return make, (lambda b: (b, 33, 5, 7)), launch, True


def _g_embed_bwd_w():
    def make(b):
        return [(rand(b, 33, 5, 7, seed=314, scale=2.0, offset=0.3), True), (rand(b, 3, 5, 7, seed=315, scale=2.0, offset=0.3), True)]

    def launch(ins, out, b):
        _call("grr_conv3x3_embed_bwd_w", ins[0], ins[1], out,
              _ws(_lib().grr_conv3x3_embed_bwd_w_workspace_bytes(b, 3, 33, 5, 7)), b, 3, 33, 5, 7)
    return make, (lambda b: (33, 3, 3, 3)), launch, False


def _g_embed_bwd_x():
    def make(b):
        return [(rand(b, 33, 5, 7, seed=316, scale=2.0, offset=0.3), True), (rand(33, 3, 3, 3, seed=317) * 0.3, False)]

    def launch(ins, out, b):
        _call("grr_conv3x3_embed_bwd_x", ins[0], ins[1], out, b, 3, 33, 5, 7)
    return make, (lambda b: (b, 3, 5, 7)), launch, True


def _g_interleave():
    def make(b):
        return [(rand(b, 12, 3, 4, seed=318, scale=2.0, offset=0.3), True)]

    def launch(ins, out, b):
        _call("grr_interleave2x2", ins[0], out, b, 3, 6, 8)
    return make, (lambda b: (b, 3, 6, 8)), launch, True


def _g_bwd_data():
    def make(b):
        return [(rand(b, 33, 5, 7, seed=319, scale=2.0, offset=0.3), True), (rand(33, 3, 2, 2, seed=320) * 0.2, False)]

    def launch(ins, out, b):
        _call("grr_conv2x2s2_bwd_data", ins[0], ins[1], out, b, 3, 33, 10, 14)
    return make, (lambda b: (b, 3, 10, 14)), launch, True


GUARDED = {
    "conv1x1_ws-x3-K27": _g_conv1x1_ws(27), "conv1x1_ws-x3k-K200": _g_conv1x1_ws(200),
    "conv1x1_cat2-x3-16+5": _g_cat2(16, 5), "conv1x1_cat2-x3k-128+5": _g_cat2(128, 5),
    "conv2x2s2": _g_conv2x2s2(), "convt2x2s2": _g_convt2x2s2(), "wgrad": _g_wgrad(), "conv3x3_embed": _g_embed(),
    "conv3x3_embed_bwd_w": _g_embed_bwd_w(), "conv3x3_embed_bwd_x": _g_embed_bwd_x(), "interleave2x2": _g_interleave(),
    "conv2x2s2_bwd_data": _g_bwd_data(),
}


def _plain_run(spec, b, nan_image=None, first_of=None):
    """One unguarded launch at batch b (first_of: the first b images of that larger batch's inputs)."""
    make, oshape, launch, _ = spec
    ins = []
    for t, batched in make(first_of or b):
        t = t.clone()
        if batched and nan_image is not None:
            t[nan_image] = float("nan")
        ins.append((t[:b].contiguous() if batched else t).to(DEV))
    out = torch.full(oshape(b), SENTINEL, device=DEV)
    launch(ins, out, b)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", list(GUARDED))
def test_guarded_operands_and_output(K, name):
    """Operands inside NaN guards, the output inside sentinel guards (4096 floats on each side, one allocation
    each, 256-byte aligned views): the result is finite and bitwise the unguarded run's, the guards unchanged."""
    spec = GUARDED[name]
    make, oshape, launch, _ = spec
    b = 2
    want = _plain_run(spec, b)
    assert bool(torch.isfinite(want).all()) and not bool((want == SENTINEL).any())
    ins = [_placed(t, float("nan"))[0] for t, _ in make(b)]
    out, whole = _placed(torch.full(oshape(b), SENTINEL), SENTINEL)
    launch(ins, out, b)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    assert torch.equal(out, want)
    assert _guards_intact(whole, out.numel())


@pytest.mark.parametrize("name", [n for n, s in GUARDED.items() if s[3]])
def test_nan_image_does_not_reach_its_neighbour(K, name):
    """B = 2 with image 1 all NaN: image 0 is bitwise the B = 1 run (rows past K, pixels past P and rows past
    M of image 0 border on image 1's memory)."""
    spec = GUARDED[name]
    one = _plain_run(spec, 1, first_of=2)
    two = _plain_run(spec, 2, nan_image=1)
    assert bool(torch.isfinite(two[0]).all())
    assert torch.equal(two[0], one[0])
    assert bool(torch.isnan(two[1]).all())


# ---- (c) misaligned, contiguous operands ---------------------------------------------------------------------
def _mis(t):
    """t as a contiguous device view one float past a 16-byte boundary."""
    whole = torch.empty(t.numel() + 1, dtype=torch.float32, device=DEV)
    v = whole[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def _mis_cases(K):
    x27 = rand(2, 27, 6, 8, seed=331, scale=2.0, offset=0.3)          # P = 48, P % 4 == 0
    x200 = rand(1, 200, 6, 8, seed=332, scale=2.0, offset=0.3)
    g33 = rand(2, 33, 6, 8, seed=333, scale=2.0, offset=0.3)
    img = rand(2, 3, 6, 8, seed=334, scale=2.0, offset=0.3)
    return {
        "conv1x1-x3": (K.conv1x1, [x27, rand(33, 27, 1, 1, seed=335) * 0.2]),
        "conv1x1-x3k": (K.conv1x1, [x200, rand(33, 200, 1, 1, seed=336) * 0.2]),
        "conv1x1_f32": (conv1x1_f32, [rand(2, 28, 6, 8, seed=337), rand(33, 28, 1, 1, seed=338) * 0.2]),
        "conv1x1_cat2": (K.conv1x1_cat2, [x27[:, :16].contiguous(), x27[:, 16:].contiguous(),
                                          rand(33, 27, 1, 1, seed=339) * 0.2]),
        "conv2x2s2": (K.conv2x2s2, [img, rand(33, 3, 2, 2, seed=340) * 0.2]),
        "convt2x2s2": (K.convt2x2s2, [x27, rand(27, 5, 2, 2, seed=341) * 0.2]),
        "wgrad": (K.wgrad, [g33, x27]),
        "conv3x3_embed": (K.conv3x3_embed, [img, rand(33, 3, 3, 3, seed=342) * 0.3]),
        "conv3x3_embed_bwd_w": (K.conv3x3_embed_bwd_w, [g33, img]),
        "conv3x3_embed_bwd_x": (K.conv3x3_embed_bwd_x, [g33, rand(33, 3, 3, 3, seed=343) * 0.3]),
        "conv2x2s2_bwd_data": (lambda g, w: K.conv2x2s2_bwd_data(g, w, 12, 16), [g33, rand(33, 3, 2, 2, seed=344) * 0.2]),
        "conv2x2s2_bwd_data_gemm": (lambda g, w: K.conv2x2s2_bwd_data_gemm(g, w, 12, 16),
                                    [g33, rand(33, 3, 2, 2, seed=345) * 0.2]),
        "repeat_graphs": (lambda x: K.repeat_graphs(x, 4), [img]),
    }


MIS_NAMES = ["conv1x1-x3", "conv1x1-x3k", "conv1x1_f32", "conv1x1_cat2", "conv2x2s2", "convt2x2s2", "wgrad",
             "conv3x3_embed", "conv3x3_embed_bwd_w", "conv3x3_embed_bwd_x", "conv2x2s2_bwd_data",
             "conv2x2s2_bwd_data_gemm", "repeat_graphs"]


@pytest.mark.parametrize("name", MIS_NAMES)
def test_misaligned_operands(K, name):
    """Contiguous operands at a 1-float storage offset (all of them, then each alone), through the wrappers.
    Read from the entry points (csrc/feature_ops.hip, codec_ops.hip, wgrad_ops.hip, graph_bwd.hip):

    entry point               16-byte accesses on a caller's pointer             misaligned operand
    grr_conv1x1_ws            none (x, out: 4-byte buffer loads / stores; wt:    bitwise the aligned run
    grr_conv1x1_cat2            scalar pack); workspace checked (& 255)
    grr_conv1x1 /             float4 loads of x, wt, float4 stores of out: the   scalar path, same MFMA order:
    grr_conv2x2s2 (launch_gemm) `vec` flag needs all three aligned (out was        bitwise the aligned run
                                missing from the flag: fixed with this test)
    grr_convt2x2s2            x, wt as grr_conv1x1_ws; out: 8-byte stores,       operands: bitwise; out: GrrError
                                checked (& 7)
    grr_wgrad                 float4 row loads of a, bop when P % 4 == 0;        GrrError from the entry point;
                                both checked (& 15) at every P                     K.wgrad copies: bitwise
    grr_conv3x3_embed         float4 loads of x, stores of out: `vec` flag       scalar path, same fmaf chain: bitwise
    grr_conv3x3_embed_bwd_w   g through grr_wgrad, checked (& 15); x scalar      GrrError on g; the wrapper copies g:
                                                                                   bitwise
    grr_conv3x3_embed_bwd_x   none (scalar)                                      bitwise
    grr_conv2x2s2_bwd_data    none (scalar)                                      bitwise
    grr_interleave2x2         float2 loads of t (& 7), float4 stores of gx       GrrError; K.conv2x2s2_bwd_data_gemm
                                (& 15), both checked                               hands it fresh tensors: bitwise
    grr_repeat_graphs         float4 copies: flag needs img and out aligned      scalar kernel: bitwise
    """
    fn, ts = _mis_cases(K)[name]
    aligned = [t.to(DEV) for t in ts]
    want = fn(*aligned)
    torch.cuda.synchronize()
    for which in [None] + list(range(len(ts))):
        args = [_mis(t) if which is None or which == i else aligned[i] for i, t in enumerate(ts)]
        got = fn(*args)
        torch.cuda.synchronize()
        assert torch.equal(got, want), (name, which)


def test_misaligned_output_of_the_fp32_gemm_takes_the_scalar_path(K):
    """Regression: launch_gemm's `vec` flag looked at x and wt only, so a misaligned `out` (or skip-epilogue
    residual) at K % 4 == 0 and P % 4 == 0 got 16-byte stores.  The flag now covers out and res."""
    x = rand(2, 28, 6, 8, seed=337).to(DEV)
    w = (rand(33, 28, 1, 1, seed=338) * 0.2).to(DEV)
    want = conv1x1_f32(x, w)
    whole = torch.full((want.numel() + 8,), SENTINEL, device=DEV)
    out = whole[1:1 + want.numel()].view(want.shape)
    _call("grr_conv1x1", x, w, out, 2, 28, 33, 48)
    img = rand(2, 3, 6, 8, seed=334, scale=2.0, offset=0.3).to(DEV)
    w2 = (rand(33, 3, 2, 2, seed=340) * 0.2).to(DEV)
    want2 = K.conv2x2s2(img, w2)
    whole2 = torch.full((want2.numel() + 8,), SENTINEL, device=DEV)
    out2 = whole2[1:1 + want2.numel()].view(want2.shape)
    _call("grr_conv2x2s2", img, w2, out2, 2, 3, 33, 6, 8)
    torch.cuda.synchronize()
    assert torch.equal(out, want) and torch.equal(out2, want2)
    for wh, n in ((whole, want.numel()), (whole2, want2.numel())):
        assert float(wh[0]) == SENTINEL and bool((wh[1 + n:] == SENTINEL).all())


def test_entry_points_reject_what_they_cannot_take(K):
    """The checked pointers: grr_wgrad's operands, grr_conv3x3_embed_bwd_w's g, grr_interleave2x2's t and gx,
    grr_convt2x2s2's out raise instead of running."""
    from irdu_amd._native import GrrError
    a, bop = _mis(rand(2, 33, 48, seed=351)), rand(2, 27, 48, seed=352).to(DEV)
    out = torch.empty(33, 27, device=DEV)
    with pytest.raises(GrrError):
        _call("grr_wgrad", a, bop, out, _ws(_lib().grr_wgrad_workspace_bytes(2, 33, 27, 48)), 2, 33, 27, 48)
    g, x = _mis(rand(2, 33, 6, 8, seed=353)), rand(2, 3, 6, 8, seed=354).to(DEV)
    gw = torch.empty(33, 3, 3, 3, device=DEV)
    with pytest.raises(GrrError):
        _call("grr_conv3x3_embed_bwd_w", g, x, gw, _ws(_lib().grr_conv3x3_embed_bwd_w_workspace_bytes(2, 3, 33, 6, 8)),
              2, 3, 33, 6, 8)
    t, gx = rand(2, 12, 3, 4, seed=355).to(DEV), torch.empty(2, 3, 6, 8, device=DEV)
    with pytest.raises(GrrError):
        _call("grr_interleave2x2", _mis(t.cpu()), gx, 2, 3, 6, 8)
    with pytest.raises(GrrError):
        _call("grr_interleave2x2", t, _mis(gx.cpu()), 2, 3, 6, 8)
    xt, wt = rand(2, 27, 5, 7, seed=356).to(DEV), (rand(27, 5, 2, 2, seed=357) * 0.2).to(DEV)
    with pytest.raises(GrrError):
        _call("grr_convt2x2s2", xt, wt, _mis(torch.zeros(2, 5, 10, 14)),
              _ws(_lib().grr_convt2x2s2_workspace_bytes(2, 27, 5, 5, 7)), 2, 27, 5, 5, 7)
    torch.cuda.synchronize()


def test_autograd_batch_slice_reaches_wgrad_aligned(K):
    """A contiguous batch slice whose offset is no multiple of 4 floats (M P odd) is what autograd can hand the
    weight-gradient wrappers: they copy it to an aligned buffer, bitwise the aligned run."""
    from irdu_amd import solver_grad as SG
    x = rand(3, 3, 5, 7, seed=361, scale=2.0, offset=0.3).to(DEV)       # 105 floats per image
    w = (rand(33, 3, 3, 3, seed=362) * 0.3).to(DEV).requires_grad_()
    lw = rand(3, 33, 5, 7, seed=363).to(DEV)
    sl = x[1:2]
    assert sl.is_contiguous() and sl.data_ptr() % 16 != 0
    (SG.Conv3x3EmbedFn.apply(sl, w) * lw[1:2]).sum().backward()
    got = w.grad.clone()
    w.grad = None
    (SG.Conv3x3EmbedFn.apply(sl.clone(), w) * lw[1:2].clone()).sum().backward()
    assert torch.equal(got, w.grad)
    g = lw[1:2]
    assert g.is_contiguous() and g.data_ptr() % 16 != 0
    assert torch.equal(K.conv3x3_embed_bwd_w(g, sl), K.conv3x3_embed_bwd_w(g.clone(), sl.clone()))
    assert torch.equal(K.wgrad(g, sl), K.wgrad(g.clone(), sl.clone()))


# ---- (d) grid-stride second trips ----------------------------------------------------------------------------
def _timed(label, t0):
    torch.cuda.synchronize()
    print(f"GEMMCLASS time {label}: {time.time() - t0:.2f} s")


def test_grid_stride_embed_forward(K):
    """embed_fwd_kernel's grid is capped at 2^12 blocks of 256 items: B H ceil(W / 4) = 1100 * 1000 > 2^20 items
    sends every thread round its loop a second time.  (0.7 s, most of it the CPU references.)"""
    t0 = time.time()
    b, cin, m, h, w = 1, 1, 2, 1100, 4000
    assert b * h * math.ceil(w / 4) > (1 << 12) * 256
    x = rand(b, cin, h, w, seed=371, scale=2.0, offset=0.3)
    wt = rand(m, cin, 3, 3, seed=372) * 0.3
    got = K.conv3x3_embed(x.to(DEV), wt.to(DEV))
    ref64, ref32 = R._embed(x.double(), wt.double()), R.F32["embed"](x, wt)
    err, bound = rel_err(got, ref64), R.fp32_class_bound(ref64, ref32)
    print(f"GEMMCLASS large embed_fwd: err {err:.3e}  bound {bound:.3e}  err/bound {err / bound:.3f}")
    assert err <= bound
    _timed("embed_fwd", t0)


def test_grid_stride_embed_reverses(K):
    """embed_patches_kernel and embed_bwd_x_kernel are capped at 2^14 blocks: B H W = 2050 * 2048 > 2^22 at
    Cin = M = 1.  (1.3 s, most of it the CPU references.)"""
    t0 = time.time()
    shape = (1, 1, 1, 2050, 2048)
    assert shape[0] * shape[3] * shape[4] > (1 << 14) * 256
    for op, fn in (("embed_bwd_x", K.conv3x3_embed_bwd_x), ("embed_bwd_w", K.conv3x3_embed_bwd_w)):
        case = R.C(op, shape, 373, 2.0, 0.3, "grid-stride second trip")
        a, b = R.inputs(case)
        f = R.OPS[op].f
        # the 2^22-pixel reduction of the weight gradient is out of dot32's reach: the library's fp32 there
        # (measured err / bound 0.013: the bound's host dependence is far inside the margin)
        ref64, ref32 = f(a.double(), b.double()), (f(a, b) if op == "embed_bwd_w" else R.F32[op](a, b))
        got = fn(a.to(DEV), b.to(DEV))
        err, bound = rel_err(got, ref64), R.fp32_class_bound(ref64, ref32)
        print(f"GEMMCLASS large {op}: err {err:.3e}  bound {bound:.3e}  err/bound {err / bound:.3f}")
        assert err <= bound, op
    _timed("embed reverses", t0)


def test_grid_stride_convt_interleave(K):
    """convt_interleave_kernel is capped at 2^16 blocks: 2 B M H W = 2 * 2050 * 4100 > 2^24 at K = M = 1.  Every
    output is one product x[y, x] w[di, dj], so the references are that product in float64 and fp32.  (0.5 s.)"""
    t0 = time.time()
    h, w = 2050, 4100
    assert 2 * h * w > (1 << 16) * 256
    x = rand(1, 1, h, w, seed=375, scale=2.0, offset=0.3)
    wt = rand(1, 1, 2, 2, seed=376) * 0.2
    got = K.convt2x2s2(x.to(DEV), wt.to(DEV))

    def ref(x, wt):
        return (x[0, 0, :, None, :, None] * wt[0, 0, None, :, None, :]).reshape(1, 1, 2 * h, 2 * w)

    ref64, ref32 = ref(x.double(), wt.double()), ref(x, wt)
    small = (1, 1, 3, 5)                                           # the product form is conv_transpose2d
    xs = rand(*small, seed=377)
    assert torch.equal((xs[0, 0, :, None, :, None] * wt[0, 0, None, :, None, :]).reshape(1, 1, 6, 10),
                       F.conv_transpose2d(xs, wt, stride=2))
    err, bound = rel_err(got, ref64), R.fp32_class_bound(ref64, ref32)
    print(f"GEMMCLASS large convt2x2s2: err {err:.3e}  bound {bound:.3e}  err/bound {err / bound:.3f}")
    assert err <= bound
    _timed("convt interleave", t0)


# ---- (e) Conv2x2s2Fn at odd sizes ----------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(9, 12), (8, 13), (9, 13)])
def test_conv2x2s2_fn_odd_sizes(K, hw):
    """The forward drops an odd last row / column as F.conv2d(stride=2) does; the reverse (cropped to the even
    size around the existing kernels, the data gradient zero-padded) matches float64 autograd, with an exactly
    zero data gradient in the dropped row and column.  W = 12: the GEMM + interleave route; 13: W // 2 * 2 = 12 too."""
    from irdu_amd import solver_grad as SG
    h, w = hw
    b, k, m = 2, 12, 24
    x = rand(b, k, h, w, seed=381, scale=2.0, offset=0.3)
    wt = rand(m, k, 2, 2, seed=382) * 0.2
    lw = rand(b, m, h // 2, w // 2, seed=383, scale=2.0, offset=0.3)

    xx, ww = x.double().requires_grad_(), wt.double().requires_grad_()
    y64 = F.conv2d(xx, ww, stride=2)
    y64.backward(lw.double())
    r64 = (y64.detach(), xx.grad, ww.grad)
    he, we = h // 2 * 2, w // 2 * 2
    gx32 = torch.zeros(b, k, h, w)
    gx32[:, :, :he, :we] = R.F32["conv2x2s2_bwd_data"](lw, wt)
    r32 = (R.F32["conv2x2s2"](x, wt), gx32, R.F32["wgrad"](lw.flatten(2), R._patches2x2(x).flatten(2)).view_as(wt))

    def gpu():
        xd, wd = x.to(DEV).requires_grad_(), wt.to(DEV).requires_grad_()
        y = SG.Conv2x2s2Fn.apply(xd, wd)
        y.backward(lw.to(DEV))
        return y.detach(), xd.grad, wd.grad

    got, again = gpu(), gpu()
    for name, g, g2, a64, a32 in zip(("y", "gx", "gw"), got, again, r64, r32):
        assert g.shape == a64.shape, name
        err, bound = rel_err(g, a64), R.fp32_class_bound(a64, a32)
        print(f"GEMMCLASS odd {hw} {name}: err {err:.3e}  bound {bound:.3e}  err/bound {err / bound:.3f}")
        assert err <= bound, name
        assert torch.equal(g, g2), name
    gx = got[1]
    assert not bool(gx[:, :, he:, :].any()) and not bool(gx[:, :, :, we:].any())
    assert not bool(r64[1][:, :, he:, :].any()) and not bool(r64[1][:, :, :, we:].any())
