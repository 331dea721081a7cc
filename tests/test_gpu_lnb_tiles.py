"""The persistent fused LocalNonLinearBlock (lnb_fused16_kernel) with workgroups that walk two and three tiles,
against float64 on the per-pixel, per-row and max-norm measures of tests/lnb_ref.py (bounds 4 x the fixed-order
fp32 evaluation's error + 1e-7 per measure; tests/test_lnb_ref.py proves on the CPU what they reject).

The kernel carries state across a workgroup's tile boundary: the 3-slot DMA ring and the h-buffer parity, the
producers' x / sigma registers and exponent correction, the consumers' W2 accumulators and running exponent.
The batch B = ceil((2 CUs + 5) / 9) of 20 x 70 images (9 tiles each, partial right and bottom tiles) gives some
workgroups three tiles and the rest two, at every template instance (KS 1 ... 6, MT 1 ... 3), a partial last
chunk, nch = 1, 2, 3 (the ring period), the kept gate and the c8 layouts.  Per case:
  branch        skip = (0, 1): err_max, err_pix, err_row <= their bounds
  skip          skip = (0.7, 1.4): out - 0.7 x per pixel inside 1.4 x the err_pix bound + the skip product's rounding
  keep          grr_lnb_forward_keep: out bitwise the plain pass, gate_pix <= its bound
  walk          the same images in batches of CUs // 9 (one tile per workgroup): bitwise the big batch
  NaN / Inf     image 1 overwritten: every other image bitwise the clean run (its tiles are followed in their
                workgroups by tiles of images about CUs / 9 later)
  c8            layouts 1 ... 3 bitwise layout 0, pads written 0 (C = 20, 96)
x sits between NaN guards (an over-read would show in the result), out and the workspace between sentinel
guards, all checked after every launch.  The non-persistent kernels (head16 + mix, the C = 128 head + mix,
lnb_rep_kernel) are held to the same measures at B = 2.
"""
import math

import pytest
import torch

from tests import lnb_ref as L
from tests.test_gpu_gemm_class import GUARD, SENTINEL, _guards_intact, _placed

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import irdu_amd
    irdu_amd.load_native()
    from irdu_amd import kernels
    return kernels


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def batch():
    """Some workgroups walk three tiles, the rest two (grid = min(tiles, CUs) = CUs)."""
    n = cus()
    b = math.ceil((2 * n + 5) / L.TILES)
    assert L.TILES * b > 2 * n and (L.TILES * b) % n != 0, (b, n)
    return b


def _lib():
    from irdu_amd import _native
    return _native.load()


def _dev(p):
    return L.Params(*[t.to(DEV).contiguous() for t in p])


def launch(x, p, skip, keep=False, io=0):
    """One guarded launch of grr_lnb_forward / _keep / _c8 on device x ([B, C, H, W], or blocked when io & 1).
    Returns (out, gate or None)."""
    from irdu_amd._native import call
    c, hid = p.ln_w.numel(), p.w2.shape[1]
    b, (h, w) = x.shape[0], ((x.shape[2], x.shape[3]) if io & 1 else x.shape[2:])
    lib = _lib()
    nbytes = lib.grr_lnb_workspace_bytes(b, c, hid, h, w) if keep else lib.grr_lnb_fused_workspace_bytes(c, hid)
    xv, xw = _placed(x, NAN)
    oshape = (b, (c + 7) // 8, h, w, 8) if io & 2 else (b, c, h, w)
    ov, ow = _placed(torch.full(oshape, SENTINEL, device=DEV), SENTINEL)
    wv, ww = _placed(torch.full(((nbytes + 3) // 4,), SENTINEL, device=DEV), SENTINEL)
    sk = torch.tensor(skip, dtype=torch.float32, device=DEV)
    args = [xv.data_ptr(), p.ln_w.data_ptr(), p.w1.data_ptr(), p.wdw.data_ptr(), p.w2.data_ptr(), sk.data_ptr(),
            ov.data_ptr(), wv.data_ptr(), b, c, hid, h, w]
    stream = torch.cuda.current_stream().cuda_stream
    if io:
        assert not keep
        call("grr_lnb_forward_c8", *args, io, stream)
    else:
        call("grr_lnb_forward_keep" if keep else "grr_lnb_forward", *args, stream)
    torch.cuda.synchronize()
    n = x.numel()
    assert bool(torch.isnan(xw[:GUARD]).all()) and bool(torch.isnan(xw[GUARD + n:]).all()), "x guards"
    assert torch.equal(xv.view(torch.int32), x.view(torch.int32)), "x written"
    assert _guards_intact(ow, ov.numel()), "out guards"
    assert _guards_intact(ww, wv.numel()), "workspace guards"
    assert not bool((ov == SENTINEL).any()), "out not fully written"
    gate = wv[:b * hid * h * w].view(b, hid, h, w).clone() if keep else None
    return ov.clone(), gate


_CLEAN = {}


def clean(case):
    """(big references, device x, device params, branch output of the big batch), once per case."""
    if case not in _CLEAN:
        ref = L.big(case, batch())
        assert _lib().grr_lnb_fused(case.c, case.hid) == 1
        x, p = ref.x.to(DEV), _dev(ref.p)
        _CLEAN[case] = (ref, x, p, launch(x, p, (0.0, 1.0))[0])
    return _CLEAN[case]


def _report(tag, e, bound):
    msg = f"{tag}: " + "  ".join(f"{k} {v:.3e} / {bound[k]:.3e} = {v / bound[k]:.3f}" for k, v in e.items())
    print(msg)
    return msg


@pytest.mark.parametrize("case", L.CASES, ids=L.IDS)
def test_branch_is_fp32_class_on_every_measure(K, case):
    ref, x, p, out = clean(case)
    print(f"CUs {cus()}  B {batch()}  tiles {L.TILES * batch()}")
    e = L.errors(out, ref.o64, ref.sc)
    bound = L.refs(case).bound
    msg = _report(f"{L.IDS[L.CASES.index(case)]} branch", e, bound)
    for k in L.MEASURES:
        assert e[k] <= bound[k], msg


@pytest.mark.parametrize("case", L.CASES, ids=L.IDS)
def test_skip_output_holds_the_branch_bound_per_pixel(K, case):
    ref, x, p, _ = clean(case)
    out, _ = launch(x, p, L.SKIP)
    ratio = L.skip_branch_ratio(out, ref.x, ref.o64, ref.sc, L.refs(case).bound["err_pix"])
    print(f"{L.IDS[L.CASES.index(case)]} skip {L.SKIP}: worst |out - s0 x - s1 o64| / allowance = {ratio:.3f}")
    assert ratio <= 1.0, ratio


@pytest.mark.parametrize("case", L.CASES, ids=L.IDS)
def test_kept_gate(K, case):
    ref, x, p, out = clean(case)
    out_k, gate = launch(x, p, (0.0, 1.0), keep=True)
    assert torch.equal(out_k, out)
    e, bound = L.gate_pix(gate, ref.g64), L.refs(case).gate_bound
    print(f"{L.IDS[L.CASES.index(case)]} gate_pix {e:.3e} / {bound:.3e} = {e / bound:.3f}")
    assert e <= bound, (e, bound)


@pytest.mark.parametrize("case", L.CASES, ids=L.IDS)
def test_walk_independence(K, case):
    """A workgroup's second and third tile equal the same tile computed as a workgroup's only one."""
    if cus() < L.TILES:
        pytest.skip(f"{cus()} CUs < {L.TILES}: no batch has one tile per workgroup (walk sub-check only)")
    ref, x, p, out = clean(case)
    nb = max(1, cus() // L.TILES)
    assert L.TILES * nb <= cus()
    for i in range(0, x.shape[0], nb):
        part, _ = launch(x[i:i + nb].contiguous(), p, (0.0, 1.0))
        assert torch.equal(part, out[i:i + nb]), (i, (part - out[i:i + nb]).abs().max().item())


@pytest.mark.parametrize("fill", [NAN, float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("case", L.CASES, ids=L.IDS)
def test_bad_image_does_not_reach_the_tiles_walked_after_it(K, case, fill):
    ref, x, p, out = clean(case)
    bad = x.clone()
    bad[1] = fill
    got, _ = launch(bad, p, (0.0, 1.0))
    keep = [i for i in range(x.shape[0]) if i != 1]
    assert torch.equal(got[keep], out[keep])
    assert not bool(torch.isfinite(got[1]).any())


@pytest.mark.parametrize("case", [L.CASES[1], L.CASES[5]], ids=[L.IDS[1], L.IDS[5]])
def test_c8_layouts_bitwise_at_this_tile_count(K, case):
    ref, x, p, out = clean(case)
    c = case.c
    x8 = K.to_c8(x)
    for io in (1, 2, 3):
        got, _ = launch(x8 if io & 1 else x, p, (0.0, 1.0), io=io)
        if io & 2:
            if c % 8:
                assert torch.count_nonzero(got[:, -1, :, :, c % 8:]) == 0      # pads written 0
            got = K.from_c8(got, c)
        assert torch.equal(got, out), (io, (got - out).abs().max().item())


# ---- the non-persistent siblings on the same measures (B = 2) ------------------------------------------------
def _sibling(tag, case, out, gate=None):
    r = L.refs(case)
    e = L.errors(out, r.s64.o, r.sc)
    msg = _report(tag, e, r.bound)
    for k in L.MEASURES:
        assert e[k] <= r.bound[k], msg
    if gate is not None:
        eg = L.gate_pix(gate, r.s64.g)
        print(f"{tag} gate_pix {eg:.3e} / {r.gate_bound:.3e} = {eg / r.gate_bound:.3f}")
        assert eg <= r.gate_bound, (eg, r.gate_bound)


@pytest.mark.parametrize("case", L.TWO_KERNEL, ids=[f"C{c.c}-hid{c.hid}" for c in L.TWO_KERNEL])
def test_two_kernel_path(K, case):
    r = L.refs(case)
    p = _dev(r.p)
    sk = torch.tensor([0.0, 1.0], device=DEV)
    try:
        K.set_lnb_fused(False)
        assert _lib().grr_lnb_fused(case.c, case.hid) == 0
        out, gate = K.lnb_forward_keep(r.x.to(DEV), p.ln_w, p.w1, p.wdw, p.w2, sk)
        plain = K.lnb_forward(r.x.to(DEV), p.ln_w, p.w1, p.wdw, p.w2, sk)
        torch.cuda.synchronize()
    finally:
        K.set_lnb_fused(True)
    assert torch.equal(plain, out)
    _sibling(f"head16 + mix C{case.c}-hid{case.hid}", case, out, gate)


def test_never_fused_width(K):
    case = L.NEVER_FUSED
    assert _lib().grr_lnb_fused(case.c, case.hid) == 0
    r = L.refs(case)
    p = _dev(r.p)
    out, gate = K.lnb_forward_keep(r.x.to(DEV), p.ln_w, p.w1, p.wdw, p.w2, torch.tensor([0.0, 1.0], device=DEV))
    _sibling("head + mix C128-hid24", case, out, gate)


@pytest.mark.parametrize("case", L.REPLICATED, ids=[f"Cs{c.rep}-R{c.c // c.rep}-hid{c.hid}" for c in L.REPLICATED])
def test_replicated_block(K, case):
    assert _lib().grr_lnb_rep_fused(case.rep, case.c // case.rep, case.c, case.hid) == 1
    r = L.refs(case)
    p = _dev(r.p)
    xd = r.x.to(DEV)
    src = xd[:, :case.rep].contiguous()
    sk = torch.tensor([0.0, 1.0], device=DEV)
    for xin in (None, xd):
        out = K.lnb_forward_rep(src, xin, p.ln_w, p.w1, p.wdw, p.w2, sk)
        tag = f"rep Cs{case.rep} R{case.c // case.rep} hid{case.hid} x={'src' if xin is None else 'replicas'}"
        _sibling(tag, case, out)
