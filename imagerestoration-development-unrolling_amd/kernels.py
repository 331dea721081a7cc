"""Torch-tensor front end of the HIP kernels (one function per C-ABI entry point).

Every function checks that its tensors are fp32, contiguous and on the GPU,
allocates its outputs with ``torch.empty`` (the C ABI never allocates), and
launches on the current torch stream of that device.  There is no fallback: a CPU
tensor or a missing libgrr.so raises.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import ctypes
import os

import numpy as np
import torch

from . import _native
from ._native import Stencil, call

Tensor = torch.Tensor


def _ptr(t: Optional[Tensor]):
    return None if t is None else t.data_ptr()


def _aligned16(t: Tensor) -> Tensor:
    """t, or a copy of it in a fresh allocation where its data pointer is not 16-byte aligned (torch's
    allocations are; a contiguous view at a storage offset that is no multiple of 4 floats is not)."""
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _check(name: str, *ts: Optional[Tensor]) -> torch.device:
    dev = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(f"{name}: tensors must be on the GPU (got {t.device}); "
                               "the HIP engine has no CPU path")
        if t.dtype != torch.float32:
            raise TypeError(f"{name}: expected float32, got {t.dtype}")
        if not t.is_contiguous():
            raise ValueError(f"{name}: expected a contiguous tensor")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError(f"{name}: tensors on different devices ({dev} vs {t.device})")
    return dev


def _stream(dev: torch.device):
    return torch.cuda.current_stream(dev).cuda_stream


class LaunchTimer:
    """Brackets each launch with HIP events on the stream it is queued on.

    ``records[kind]`` collects (start, end, algorithmic_bytes) per launch; ``summary()``
    synchronises and returns per-kind launch count, mean duration and achieved GB/s.
    """
    split_lnb = False   # True: C <= 128 LocalNonLinearBlocks timed as "lnb_head" + "lnb_mix"

    def __init__(self):
        self.records = {}

    def run(self, kind: str, nbytes: int, fn, flops: int = 0):
        s = torch.cuda.Event(enable_timing=True)
        e = torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        self.records.setdefault(kind, []).append((s, e, nbytes, flops))

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for kind, recs in self.records.items():
            ms = [s.elapsed_time(e) for s, e, _, _ in recs]
            nb = sum(r[2] for r in recs)
            fl = sum(r[3] for r in recs)
            tot = sum(ms)
            out[kind] = {"launches": len(recs), "total_ms": tot, "mean_ms": tot / len(recs),
                         "bytes_per_launch": nb / len(recs), "gbps": nb / (tot * 1e-3) / 1e9 if tot > 0 else 0.0,
                         "flops_per_launch": fl / len(recs),
                         "tflops": fl / (tot * 1e-3) / 1e12 if tot > 0 else 0.0}
        return out


_TIMER = None


def set_timer(timer):
    """Install (or clear, with None) a LaunchTimer for subsequent launches."""
    global _TIMER
    _TIMER = timer


# GRR_TIMER_SHAPES=1: the instrumented loops time the GEMM-like launches per operand shape
TIMER_SHAPES = os.environ.get("GRR_TIMER_SHAPES", "0") == "1"


def _launch(kind: str, nbytes: int, name: str, *args, flops: int = 0):
    if _TIMER is None:
        call(name, *args)
    else:
        _TIMER.run(kind, int(nbytes), lambda: call(name, *args), int(flops))


def lnb_flops(px: int, c_head: int, c: int, hid: int) -> int:
    """Algorithmic fp32 flops of one LocalNonLinearBlock (REF:911-964) over px pixels: LN (4 per
    input channel), W1 (2 c_head 2hid), depthwise 3x3 (18 per hidden channel), gate (4 per
    gated channel), W2 (2 hid c), skip (3 per output channel)."""
    return px * (4 * c_head + 2 * c_head * 2 * hid + 18 * 2 * hid + 4 * hid + 2 * hid * c + 3 * c)


def stencil(module) -> Stencil:
    """grr_stencil of a GLRFast/GTVFast module (its stats_kernel_p* parameters)."""
    ps = [module.stats_kernel_p01, module.stats_kernel_p02a, module.stats_kernel_p02b, module.stats_kernel_p03]
    _check("stencil", *[p.data for p in ps])
    return Stencil(*[p.data_ptr() for p in ps])


NO_STENCIL = Stencil(None, None, None, None)


# ---------------------------------------------------------------------------
TERM_ROWS = True


def set_term_rows(enable) -> None:
    """Row-streaming (True / 2, default: the LDS-ring row kernel where the shape allows, else the
    register-prefetch one; 1: always the register-prefetch row kernel) or per-pixel (False / 0) term
    reverses (grr_bwd_term_fused)."""
    global TERM_ROWS
    level = 2 if enable is True else int(enable)
    _native.call("grr_bwd_set_term_rows", level)
    TERM_ROWS = level > 0


def set_term_tail(enable: bool) -> None:
    """The wide ring-kernel term reverse's last column strip as a one-column-lane launch (default on)."""
    _native.call("grr_bwd_set_term_tail", int(bool(enable)))


def set_term_acc_max_w(w: int) -> None:
    """Widest image where the LDS-ring term reverse takes the x-gradient pass inside (default 128)."""
    _native.call("grr_bwd_set_term_acc_max_w", int(w))


def term_rows_ok(w: int, f: int) -> bool:
    """Widths / channel counts the row-streaming term reverse takes (16-byte aligned planes assumed)."""
    if w <= 64:
        return f <= 16
    if w <= 128 and w % 2 == 0:
        return f <= 16
    return w % 4 == 0 and f <= 12   # W > 256: column strips


def set_kernel_variant(variant: str) -> None:
    """Select the graph-operator kernels: "auto" (row waves for W <= 256, the channel waves
    of a graph in lockstep), "strips" (column strips at every width) or "independent" (row
    waves, channel waves unsynchronised).  Test / benchmark knob; process-wide."""
    _native.call("grr_set_kernel_variant", {"auto": 0, "strips": 1, "independent": 2}[variant])


def stream_copy(src: Tensor, dst: Tensor) -> None:
    """float4 streaming copy (bench's measured HBM ceiling)."""
    assert src.is_contiguous() and dst.is_contiguous() and src.numel() == dst.numel()
    call("grr_stream_copy", src.data_ptr(), dst.data_ptr(), src.numel(), _stream(src.device))


def neighbor_table(h: int, w: int, device) -> Tensor:
    out = torch.empty((4, h, w), dtype=torch.int32, device=device)
    call("grr_neighbor_table", out.data_ptr(), h, w, _stream(out.device))
    return out


def edge_weights(feat: Tensor, channel_offset: int, n_graphs: int, n_fts: int, multiM: Tensor,
                 with_degree: bool = False) -> Tuple[Tensor, Optional[Tensor]]:
    """Edge weights of the [n_graphs*n_fts] channel slab starting at ``channel_offset`` of feat [B,Ctot,H,W]."""
    dev = _check("edge_weights", feat, multiM)
    b, ctot, h, w = feat.shape
    if channel_offset + n_graphs * n_fts > ctot:
        raise ValueError("edge_weights: channel slab out of range")
    wt = torch.empty((b, n_graphs, 4, h, w), dtype=torch.float32, device=dev)
    deg = torch.empty((b, n_graphs, h, w), dtype=torch.float32, device=dev) if with_degree else None
    base = feat.data_ptr() + channel_offset * h * w * feat.element_size()
    nbytes = 4 * b * h * w * (n_graphs * n_fts + 4 * n_graphs + (n_graphs if with_degree else 0))
    _launch("edge_weights", nbytes, "grr_edge_weights", base, ctot * h * w, multiM.data_ptr(), wt.data_ptr(),
            _ptr(deg), b, n_graphs, n_fts, h, w, _stream(dev))
    return wt, deg


def edge_weights_block(feat: Tensor, n_graphs: int, n_fts: int, multiM_gtv: Tensor,
                       multiM_glr: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """Both graph modules of a level from one [B, 2C, H, W] feature map (GTV half first, REF:714):
    returns (wG raw [B,G,4,H,W], cG pair [B,G,2,H,W], wL [B,G,4,H,W])."""
    dev = _check("edge_weights_block", feat, multiM_gtv, multiM_glr)
    b, ctot, h, w = feat.shape
    c = n_graphs * n_fts
    if ctot != 2 * c:
        raise ValueError(f"edge_weights_block: expected {2 * c} feature channels, got {ctot}")
    wG = torch.empty((b, n_graphs, 4, h, w), dtype=torch.float32, device=dev)
    wL = torch.empty_like(wG)
    cG = torch.empty((b, n_graphs, 2, h, w), dtype=torch.float32, device=dev)
    nbytes = 4 * b * h * w * (2 * c + 10 * n_graphs)
    _launch("edge_weights", nbytes, "grr_edge_weights_block", feat.data_ptr(), ctot * h * w, 0,
            multiM_gtv.data_ptr(), c, multiM_glr.data_ptr(), wG.data_ptr(), cG.data_ptr(), wL.data_ptr(),
            b, n_graphs, n_fts, h, w, _stream(dev))
    return wG, cG, wL


def feature_edges_ok(c: int, n_graphs: int, n_fts: int, h: int, w: int) -> bool:
    """Where feature_edges applies: grr_feature_edges_supported's conditions (F = 3, G <= 32, C = G F) in plain
    Python (traceable; tests/test_abi.py checks the two agree)."""
    return (n_fts == 3 and 1 <= n_graphs <= 32 and c == n_graphs * n_fts and c <= 96 and h >= 1 and w >= 1
            and n_graphs * 4 * h * w * 4 < (1 << 31) and ((c + 7) // 8) * 8 * h * w * 4 < (1 << 31))


def feature_edges(x: Tensor, x_blocked: bool, weight: Tensor, n_graphs: int, n_fts: int, multiM_gtv: Tensor,
                  multiM_glr: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """edge_weights_block(conv1x1(x, weight), ...) in one pass (grr_feature_edges): the [B, 2C, H, W]
    features stay on chip.  x: [B, C, H, W], or the channel-blocked layout (x_blocked, lnb_forward_c8's).
    Returns (wG raw [B,G,4,H,W], cG pair [B,G,2,H,W], wL [B,G,4,H,W])."""
    dev = _check("feature_edges", x, weight, multiM_gtv, multiM_glr)
    if x_blocked:
        b, _, h, w, _ = x.shape
        c = n_graphs * n_fts
    else:
        b, c, h, w = x.shape
    if tuple(weight.shape[:2]) != (2 * n_graphs * n_fts, c):
        raise ValueError(f"feature_edges: weight {tuple(weight.shape)} for {c} -> {2 * n_graphs * n_fts} channels")
    wG = torch.empty((b, n_graphs, 4, h, w), dtype=torch.float32, device=dev)
    wL = torch.empty_like(wG)
    cG = torch.empty((b, n_graphs, 2, h, w), dtype=torch.float32, device=dev)
    lib = _native.load()
    ws = torch.empty((lib.grr_feature_edges_workspace_bytes(n_graphs) + 3) // 4, dtype=torch.float32, device=dev)
    nbytes = 4 * b * h * w * (c + 10 * n_graphs)   # x in; wG, wL, cG out
    _launch("feature_edges", nbytes, "grr_feature_edges", x.contiguous().data_ptr(), int(x_blocked),
            weight.contiguous().data_ptr(), multiM_gtv.contiguous().data_ptr(), multiM_glr.contiguous().data_ptr(),
            wG.data_ptr(), cG.data_ptr(), wL.data_ptr(), ws.data_ptr(), b, c, n_graphs, n_fts, h, w, _stream(dev),
            flops=2 * b * h * w * c * 2 * c)
    return wG, cG, wL


def gtv_pair_weights(w: Tensor) -> Tensor:
    dev = _check("gtv_pair_weights", w)
    b, g, four, h, ww = w.shape
    assert four == 4
    c = torch.empty((b, g, 2, h, ww), dtype=torch.float32, device=dev)
    _launch("gtv_pair_weights", 4 * b * g * h * ww * 6, "grr_gtv_pair_weights", w.data_ptr(), c.data_ptr(),
            b, g, h, ww, _stream(dev))
    return c


def pool2(x: Tensor) -> Tensor:
    dev = _check("pool2", x)
    b, c, h, w = x.shape
    out = torch.empty((b, c, h // 2, w // 2), dtype=torch.float32, device=dev)
    _launch("pool2", 4 * b * c * h * w * 5 // 4, "grr_pool2", x.data_ptr(), out.data_ptr(), b, c, h, w, _stream(dev))
    return out


def system_half(xd: Tensor, wL: Optional[Tensor], cG: Optional[Tensor], sL: Stencil, sG: Stencil,
                log_mu: Optional[Tensor], log_ro: Optional[Tensor], n_graphs: int) -> Tensor:
    dev = _check("system_half", xd, wL, cG, log_mu, log_ro)
    b, c, h, w = xd.shape
    t = torch.empty_like(xd)
    nbytes = 4 * b * h * w * (2 * c + (4 * n_graphs if wL is not None else 0) + (2 * n_graphs if cG is not None else 0))
    _launch("system_half", nbytes, "grr_system_half", xd.data_ptr(), _ptr(wL), _ptr(cG), sL, sG, _ptr(log_mu),
            _ptr(log_ro), t.data_ptr(), b, n_graphs, c // n_graphs, h, w, _stream(dev))
    return t


def gtv_rhs_half(xd: Tensor, wG: Tensor, sG: Stencil, prox: bool, log_gamma: Optional[Tensor],
                 n_graphs: int) -> Tensor:
    dev = _check("gtv_rhs_half", xd, wG, log_gamma)
    b, c, h, w = xd.shape
    t = torch.empty_like(xd)
    nbytes = 4 * b * h * w * (2 * c + (4 if prox else 2) * n_graphs)
    _launch("gtv_rhs_half", nbytes, "grr_gtv_rhs_half", xd.data_ptr(), wG.data_ptr(), sG, int(prox),
            _ptr(log_gamma), t.data_ptr(), b, n_graphs, c // n_graphs, h, w, _stream(dev))
    return t


def gtv_rhs_full(x: Tensor, y: Tensor, wG: Tensor, sG: Stencil, prox: bool, log_gamma: Optional[Tensor],
                 log_ro0: Tensor, t_half: Optional[Tensor], log_ro1: Optional[Tensor], n_graphs: int,
                 want_pool: bool = False) -> Tuple[Tensor, Optional[Tensor]]:
    dev = _check("gtv_rhs_full", x, y, wG, log_gamma, log_ro0, t_half, log_ro1)
    b, c, h, w = x.shape
    out = torch.empty_like(x)
    xd = torch.empty((b, c, h // 2, w // 2), dtype=torch.float32, device=dev) if want_pool else None
    px = b * h * w
    nbytes = 4 * (px * (3 * c if x.data_ptr() != y.data_ptr() else 2 * c) + px * (4 if prox else 2) * n_graphs
                  + (px * c // 4 if t_half is not None else 0) + (px * c // 4 if want_pool else 0))
    _launch("gtv_rhs_full", nbytes, "grr_gtv_rhs_full", x.data_ptr(), y.data_ptr(), wG.data_ptr(), sG, int(prox),
            _ptr(log_gamma), log_ro0.data_ptr(), _ptr(t_half), _ptr(log_ro1), out.data_ptr(), _ptr(xd),
            b, n_graphs, c // n_graphs, h, w, _stream(dev))
    return out, xd


def gtv_rhs_full_rep(x: Tensor, x_rep: bool, y: Tensor, y_rep: bool, wG: Tensor, sG: Stencil, prox: bool,
                     log_gamma: Optional[Tensor], log_ro0: Tensor, t_half: Optional[Tensor],
                     log_ro1: Optional[Tensor], n_graphs: int, want_pool: bool = False) -> Tuple[Tensor, Optional[Tensor]]:
    """grr_gtv_rhs_full with x and/or y given as the [B, F, H, W] image they replicate over the graphs."""
    dev = _check("gtv_rhs_full", x, y, wG, log_gamma, log_ro0, t_half, log_ro1)
    full = y if not y_rep else (x if not x_rep else None)
    b, f, h, w = (x if x_rep else y).shape if full is None else (full.shape[0], full.shape[1] // n_graphs,
                                                                  full.shape[2], full.shape[3])
    c = n_graphs * f
    out = torch.empty((b, c, h, w), dtype=torch.float32, device=dev)
    xd = torch.empty((b, c, h // 2, w // 2), dtype=torch.float32, device=dev) if want_pool else None
    px = b * h * w
    nbytes = 4 * (px * (f if x_rep else c) + px * (f if y_rep else c) + px * c + px * (4 if prox else 2) * n_graphs
                  + (px * c // 4 if t_half is not None else 0) + (px * c // 4 if want_pool else 0))
    _launch("gtv_rhs_full", nbytes, "grr_gtv_rhs_full_rep", x.data_ptr(), int(x_rep), y.data_ptr(), int(y_rep),
            wG.data_ptr(), sG, int(prox), _ptr(log_gamma), log_ro0.data_ptr(), _ptr(t_half), _ptr(log_ro1),
            out.data_ptr(), _ptr(xd), b, n_graphs, f, h, w, _stream(dev))
    return out, xd


def system_step(x: Tensor, rhs: Tensor, u_prev: Optional[Tensor], t_half: Optional[Tensor],
                wL: Optional[Tensor], cG: Optional[Tensor], sL: Stencil, sG: Stencil,
                log_mu0: Optional[Tensor], log_ro0: Optional[Tensor], alpha: Tensor, beta: Optional[Tensor],
                n_graphs: int, want_u: bool, want_pool: bool, skip: Optional[Tensor] = None,
                y_skip: Optional[Tensor] = None, u_out: Optional[Tensor] = None) -> Tuple[Tensor, Optional[Tensor], Optional[Tensor]]:
    dev = _check("system_step", x, rhs, u_prev, t_half, wL, cG, log_mu0, log_ro0, alpha, beta, skip, y_skip)
    b, c, h, w = x.shape
    out = torch.empty_like(x)
    if want_u and u_out is None:
        u_out = torch.empty_like(x)
    if not want_u:
        u_out = None
    xd = torch.empty((b, c, h // 2, w // 2), dtype=torch.float32, device=dev) if want_pool else None
    _launch("system_step", step_bytes(b, c, n_graphs, h, w, rhs is not x, u_prev is not None, t_half is not None,
                                      wL is not None, cG is not None, u_out is not None, want_pool, skip is not None),
            "grr_system_step", x.data_ptr(), rhs.data_ptr(), _ptr(u_prev), _ptr(t_half), _ptr(wL), _ptr(cG), sL, sG,
            _ptr(log_mu0), _ptr(log_ro0), alpha.data_ptr(), _ptr(beta), _ptr(skip), _ptr(y_skip),
            out.data_ptr(), _ptr(u_out), _ptr(xd), b, n_graphs, c // n_graphs, h, w, _stream(dev))
    return out, u_out, xd


def system_step2(x: Tensor, rhs: Tensor, u_prev: Optional[Tensor], xd_in: Tensor,
                 wL0: Tensor, cG0: Tensor, sL0: Stencil, sG0: Stencil, log_mu0: Tensor, log_ro0: Tensor,
                 wL1: Tensor, cG1: Tensor, sL1: Stencil, sG1: Stencil, log_mu1: Tensor, log_ro1: Tensor,
                 alpha_a: Tensor, beta_a: Optional[Tensor], alpha_b: Tensor, beta_b: Optional[Tensor],
                 n_graphs: int, want_u: bool, want_pool: bool, skip: Optional[Tensor] = None,
                 y_skip: Optional[Tensor] = None, u_out: Optional[Tensor] = None
                 ) -> Tuple[Tensor, Optional[Tensor], Optional[Tensor]]:
    """Stages k and k+1 in one pass (grr_system_step2), the half level of both inside it; xd_in = D x_k
    (the previous pass's pooled output).  Returns (x_{k+2}, u_{k+2}, D x_{k+2})."""
    dev = _check("system_step2", x, rhs, u_prev, xd_in, wL0, cG0, log_mu0, log_ro0, wL1, cG1, log_mu1, log_ro1,
                 alpha_a, beta_a, alpha_b, beta_b, skip, y_skip)
    b, c, h, w = x.shape
    out = torch.empty_like(x)
    if want_u and (u_out is None or (u_prev is not None and u_out.data_ptr() == u_prev.data_ptr())):
        u_out = torch.empty_like(x)
    if not want_u:
        u_out = None
    xd = torch.empty((b, c, h // 2, w // 2), dtype=torch.float32, device=dev) if want_pool else None
    _launch("system_step2", step2_bytes(b, c, n_graphs, h, w, u_prev is not None, u_out is not None, want_pool,
                                        skip is not None),
            "grr_system_step2", x.data_ptr(), rhs.data_ptr(), _ptr(u_prev), xd_in.data_ptr(), wL0.data_ptr(),
            cG0.data_ptr(), sL0, sG0, log_mu0.data_ptr(), log_ro0.data_ptr(), wL1.data_ptr(), cG1.data_ptr(), sL1, sG1,
            log_mu1.data_ptr(), log_ro1.data_ptr(), alpha_a.data_ptr(), _ptr(beta_a), alpha_b.data_ptr(),
            _ptr(beta_b), _ptr(skip), _ptr(y_skip), out.data_ptr(), _ptr(u_out), _ptr(xd), b, n_graphs,
            c // n_graphs, h, w, _stream(dev))
    return out, u_out, xd


def system_first_pair(b_a: Tensor, xd_a: Tensor, y: Tensor, y_rep: bool,
                      wL0: Tensor, cG0: Tensor, wG0: Tensor, sL0: Stencil, sG0: Stencil, log_mu0: Tensor,
                      log_ro0: Tensor, log_gamma0: Tensor, wL1: Tensor, cG1: Tensor, wG1: Tensor, sL1: Stencil,
                      sG1: Stencil, log_mu1: Tensor, log_ro1: Tensor, log_gamma1: Tensor, alpha0: Tensor,
                      alpha1: Tensor, n_graphs: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """Stage 0, the prox right-hand side B and stage 1 in one pass (grr_system_first_pair); xd_a = D b_A.
    y: [B, C, H, W], or the [B, F, H, W] image it replicates (y_rep).  Returns (b_B, x_2, u_2, D x_2)."""
    dev = _check("system_first_pair", b_a, xd_a, y, wL0, cG0, wG0, log_mu0, log_ro0, log_gamma0, wL1, cG1, wG1,
                 log_mu1, log_ro1, log_gamma1, alpha0, alpha1)
    b, c, h, w = b_a.shape
    b_out, x_out, u_out = (torch.empty_like(b_a) for _ in range(3))
    xd = torch.empty((b, c, h // 2, w // 2), dtype=torch.float32, device=dev)
    _launch("system_first_pair", first_pair_bytes(b, c, n_graphs, h, w, y_rep),
            "grr_system_first_pair", b_a.data_ptr(), xd_a.data_ptr(), y.data_ptr(), int(y_rep), wL0.data_ptr(),
            cG0.data_ptr(), wG0.data_ptr(), sL0, sG0, log_mu0.data_ptr(), log_ro0.data_ptr(), log_gamma0.data_ptr(),
            wL1.data_ptr(), cG1.data_ptr(), wG1.data_ptr(), sL1, sG1, log_mu1.data_ptr(), log_ro1.data_ptr(),
            log_gamma1.data_ptr(), alpha0.data_ptr(), alpha1.data_ptr(), b_out.data_ptr(), x_out.data_ptr(),
            u_out.data_ptr(), xd.data_ptr(), b, n_graphs, c // n_graphs, h, w, _stream(dev))
    return b_out, x_out, u_out, xd


def first_pair_bytes(b, c, g, h, w, y_rep):
    """Compulsory HBM bytes of one grr_system_first_pair launch: b_A, D b_A, y read once, the full- and
    half-level GLR + pair weights and the prox raw weights read once per channel group; b_B, x_2, u_2, D x_2
    written once (t_0, x_1, D x_1, the prox terms and t_1 stay on chip)."""
    f = c * (1 + 3) + (c // g if y_rep else c)                         # b_A in; b_B, x_2, u_2 out; y in
    f += (c // 4) * 2                                                  # D b_A in, D x_2 out
    ngrp = -(-(c // g) // 3)
    f += (6 * g + 4 * g + (6 * g + 4 * g) // 4) * ngrp                 # wL0, cG0, wG0; wL1, cG1, wG1
    return 4 * b * h * w * f


# stage 0, right-hand side B and stage 1 in one pass where the shape allows (tests set False for the
# per-stage sequence)
FIRST_PAIR = True


def first_pair_supported(x: Tensor, n_graphs: int) -> bool:
    b, c, h, w = x.shape
    return FIRST_PAIR and w == 256 and h % 2 == 0 and c % n_graphs == 0


# two CG stages per launch where the shape allows (tests set False to run one launch per stage)
STEP2 = True


def system_step2_train(x: Tensor, rhs: Tensor, u_prev: Optional[Tensor], xd_in: Tensor,
                       wL0: Tensor, cG0: Tensor, sL0: Stencil, sG0: Stencil, log_mu0: Tensor, log_ro0: Tensor,
                       wL1: Tensor, cG1: Tensor, sL1: Stencil, sG1: Stencil, log_mu1: Tensor, log_ro1: Tensor,
                       alpha_a: Tensor, beta_a: Optional[Tensor], alpha_b: Tensor, beta_b: Optional[Tensor],
                       n_graphs: int, want_pool: bool, want_mid_pool: bool = False
                       ) -> Tuple[Tensor, Tensor, Tensor, Tensor, Optional[Tensor], Optional[Tensor]]:
    """Stages k, k+1 in one pass keeping the middle iterate (grr_system_step2_train, the training
    forward).  Returns (x_{k+1}, u_{k+1}, x_{k+2}, u_{k+2}, D x_{k+2}, D x_{k+1}); the pooled
    outputs are None unless asked for."""
    dev = _check("system_step2_train", x, rhs, u_prev, xd_in, wL0, cG0, log_mu0, log_ro0, wL1, cG1, log_mu1,
                 log_ro1, alpha_a, beta_a, alpha_b, beta_b)
    b, c, h, w = x.shape
    x_mid, u_mid, out, u_out = (torch.empty_like(x) for _ in range(4))
    xd = torch.empty((b, c, h // 2, w // 2), dtype=torch.float32, device=dev) if want_pool else None
    xdm = torch.empty((b, c, h // 2, w // 2), dtype=torch.float32, device=dev) if want_mid_pool else None
    _launch("system_step2", step2_bytes(b, c, n_graphs, h, w, u_prev is not None, True, want_pool, False)
            + 8 * x.numel() + (x.numel() if want_mid_pool else 0),
            "grr_system_step2_train", x.data_ptr(), rhs.data_ptr(), _ptr(u_prev), xd_in.data_ptr(), wL0.data_ptr(),
            cG0.data_ptr(), sL0, sG0, log_mu0.data_ptr(), log_ro0.data_ptr(), wL1.data_ptr(), cG1.data_ptr(), sL1, sG1,
            log_mu1.data_ptr(), log_ro1.data_ptr(), alpha_a.data_ptr(), _ptr(beta_a), alpha_b.data_ptr(),
            _ptr(beta_b), out.data_ptr(), u_out.data_ptr(), _ptr(xd), x_mid.data_ptr(), u_mid.data_ptr(),
            _ptr(xdm), b, n_graphs, c // n_graphs, h, w, _stream(dev))
    return x_mid, u_mid, out, u_out, xd, xdm


# W != 256 (W % 8 == 0) runs the two-stage pass in column strips of 256 lanes with a 16-column halo
# (STEP2_STRIPS = False: one launch per stage there; bench_wide.py's per-stage comparison).  Narrower images are one strip with idle lanes:
# at W = 128 (the v1.0 model's second level) that still beats one launch per stage (v1.0 forward
# 25.15-25.22 -> 24.75 ms at 16 x 256^2), at W = 64 it does not (25.48 ms; profiles/r03/s2strips/narrow.txt)
STEP2_STRIPS = True
STEP2_MIN_W = 128   # narrowest strip-pass width the loops use


def step2_supported(x: Tensor, n_graphs: int) -> bool:
    """Where the model loops use grr_system_step2: W = 256, or W >= STEP2_MIN_W with W % 8 == 0
    (column strips); even H (F > 3: channel groups of <= 3)."""
    b, c, h, w = x.shape
    wide = STEP2_STRIPS and w >= STEP2_MIN_W and w % 8 == 0
    return (w == 256 or wide) and h % 2 == 0 and c % n_graphs == 0


def step2_bytes(b, c, g, h, w, has_u_prev, has_u_out, has_pool, has_skip):
    """Compulsory HBM bytes of one grr_system_step2 launch: x, b, u_prev, D x_k, the full- and
    half-level GLR + pair weights read once; x_out, u_out, D x_out written once (t_k, x_{k+1},
    u_{k+1}, t_{k+1} stay on chip; the second reads of b rows and of half-level weight rows are
    L2 hits by construction)."""
    f = c * (2 + int(has_u_prev) + 1 + int(has_u_out) + int(has_skip))    # x, b, u_prev, x_out, u_out, y
    f += (c // 4) * (1 + int(has_pool))                                   # D x_k in, D x_out
    ngrp = -(-(c // g) // 3)                                              # workgroups per graph (F > 3)
    f += (6 * g + (6 * g) // 4) * ngrp                                    # full + half-level weights, per group
    return 4 * b * h * w * f


def step_bytes(b, c, g, h, w, has_rhs, has_u_prev, has_half, has_glr, has_gtv, has_u_out, has_pool, has_skip):
    """Compulsory HBM bytes of one grr_system_step launch (each input read once, each output written once)."""
    f = c * (1 + int(has_rhs) + int(has_u_prev) + int(has_u_out) + 1 + int(has_skip))  # x, b, u_prev, u, x_out, y
    f += (c // 4) * (int(has_half) + int(has_pool))                                     # half-level in / out
    f += g * (4 * int(has_glr) + 2 * int(has_gtv))                                      # edge / pair weights
    return 4 * b * h * w * f


# ---- GLRFast / GTVFast sub-API (REF:128-228, :452-516) ---------------------------------
def neighbor_gather(x: Tensor) -> Tensor:
    """get_neighbors_pixels: [B,C,H,W] -> [B,C,4,H,W] replicate-clamped neighbours (REF:128-144)."""
    dev = _check("neighbor_gather", x)
    b, c, h, w = x.shape
    out = torch.empty((b, c, 4, h, w), dtype=torch.float32, device=dev)
    _launch("subapi", 4 * x.numel() * 5, "grr_neighbor_gather", x.data_ptr(), out.data_ptr(), b, c, h, w, _stream(dev))
    return out


def normalize_features(f5: Tensor, multiM: Tensor) -> Tensor:
    """normalize_and_transform_features: [B,G,F,H,W] -> [B,G*F,H,W] (REF:146-157)."""
    dev = _check("normalize_features", f5, multiM)
    b, g, f, h, w = f5.shape
    if tuple(multiM.shape) != (g, f):
        raise ValueError(f"normalize_features: multiM {tuple(multiM.shape)} vs ({g}, {f})")
    out = torch.empty((b, g * f, h, w), dtype=torch.float32, device=dev)
    _launch("subapi", 8 * f5.numel(), "grr_normalize_features", f5.data_ptr(), multiM.data_ptr(), out.data_ptr(),
            b, g, f, h, w, _stream(dev))
    return out


def stats_conv(x5: Tensor, st: Stencil, transpose: bool) -> Tensor:
    """stats_conv (replicate) / stats_conv_transpose (zero frame) of [B,G,F,H,W] (REF:177-215)."""
    dev = _check("stats_conv", x5)
    b, g, f, h, w = x5.shape
    out = torch.empty_like(x5)
    _launch("subapi", 8 * x5.numel(), "grr_stats_conv", x5.data_ptr(), st, int(transpose), out.data_ptr(),
            b, g, f, h, w, _stream(dev))
    return out


def glr_op_L_norm(x5: Tensor, w: Tensor) -> Tensor:
    """GLRFast.op_L_norm: x - sum_e w_e x(clamp(p + delta_e)) (REF:218-228)."""
    dev = _check("glr_op_L_norm", x5, w)
    b, g, f, h, ww = x5.shape
    if tuple(w.shape) != (b, g, 4, h, ww):
        raise ValueError(f"glr_op_L_norm: edge weights {tuple(w.shape)} vs {(b, g, 4, h, ww)}")
    out = torch.empty_like(x5)
    _launch("subapi", 4 * (2 * x5.numel() + w.numel()), "grr_glr_op_l_norm", x5.data_ptr(), w.data_ptr(),
            out.data_ptr(), b, g, f, h, ww, _stream(dev))
    return out


def gtv_op_C(x5: Tensor, w: Tensor, st: Stencil) -> Tensor:
    """GTVFast.op_C: [B,G,F,H,W] -> edge signals [B,G,F,4,H,W] (REF:452-467)."""
    dev = _check("gtv_op_C", x5, w)
    b, g, f, h, ww = x5.shape
    if tuple(w.shape) != (b, g, 4, h, ww):
        raise ValueError(f"gtv_op_C: edge weights {tuple(w.shape)} vs {(b, g, 4, h, ww)}")
    out = torch.empty((b, g, f, 4, h, ww), dtype=torch.float32, device=dev)
    _launch("subapi", 4 * (5 * x5.numel() + w.numel()), "grr_gtv_op_c", x5.data_ptr(), w.data_ptr(), st,
            out.data_ptr(), b, g, f, h, ww, _stream(dev))
    return out


def gtv_op_C_transpose(e6: Tensor, w: Tensor, st: Stencil, want_work: bool = False):
    """GTVFast.op_C_transpose: edge signals [B,G,F,4,H,W] -> [B,G,F,H,W] (REF:469-516)."""
    dev = _check("gtv_op_C_transpose", e6, w)
    b, g, f, four, h, ww = e6.shape
    if four != 4 or tuple(w.shape) != (b, g, 4, h, ww):
        raise ValueError(f"gtv_op_C_transpose: edges {tuple(e6.shape)} / weights {tuple(w.shape)}")
    work = torch.empty((b, g, f, h, ww), dtype=torch.float32, device=dev)
    out = torch.empty_like(work)
    _launch("subapi", 4 * (e6.numel() + w.numel() + 3 * work.numel()), "grr_gtv_op_c_transpose", e6.data_ptr(),
            w.data_ptr(), st, work.data_ptr(), out.data_ptr(), b, g, f, h, ww, _stream(dev))
    return (out, work) if want_work else out


# reverses of the sub-API (csrc/subapi_bwd.hip); gM / gtaps accumulate, gtaps is [G*F, 5]
def neighbor_gather_bwd(g: Tensor) -> Tensor:
    dev = _check("neighbor_gather_bwd", g)
    b, c, four, h, w = g.shape
    gx = torch.empty((b, c, h, w), dtype=torch.float32, device=dev)
    _launch("subapi_bwd", 4 * g.numel() * 5 // 4, "grr_neighbor_gather_bwd", g.data_ptr(), gx.data_ptr(), b, c, h, w,
            _stream(dev))
    return gx


def normalize_features_bwd(f5: Tensor, multiM: Tensor, gout: Tensor, gM: Tensor) -> Tensor:
    dev = _check("normalize_features_bwd", f5, multiM, gout, gM)
    b, g, f, h, w = f5.shape
    gf = torch.empty_like(f5)
    _launch("subapi_bwd", 12 * f5.numel(), "grr_normalize_features_bwd", f5.data_ptr(), multiM.data_ptr(),
            gout.data_ptr(), gf.data_ptr(), gM.data_ptr(), b, g, f, h, w, _stream(dev))
    return gf


def stats_conv_bwd(x5: Tensor, st: Stencil, transpose: bool, g: Tensor, gtaps: Optional[Tensor]) -> Tensor:
    dev = _check("stats_conv_bwd", x5, g, gtaps)
    b, gg, f, h, w = x5.shape
    gx = torch.empty_like(x5)
    _launch("subapi_bwd", 12 * x5.numel(), "grr_stats_conv_bwd", x5.data_ptr(), st, int(transpose), g.data_ptr(),
            gx.data_ptr(), _ptr(gtaps), b, gg, f, h, w, _stream(dev))
    return gx


def glr_op_L_norm_bwd(x5: Tensor, w: Tensor, g: Tensor) -> Tuple[Tensor, Tensor]:
    dev = _check("glr_op_L_norm_bwd", x5, w, g)
    b, gg, f, h, ww = x5.shape
    gx, gw = torch.empty_like(x5), torch.empty_like(w)
    _launch("subapi_bwd", 4 * (3 * x5.numel() + 3 * w.numel()), "grr_glr_op_l_norm_bwd", x5.data_ptr(), w.data_ptr(),
            g.data_ptr(), gx.data_ptr(), gw.data_ptr(), b, gg, f, h, ww, _stream(dev))
    return gx, gw


def gtv_op_C_bwd(x5: Tensor, w: Tensor, st: Stencil, gE: Tensor, gtaps: Tensor) -> Tuple[Tensor, Tensor]:
    dev = _check("gtv_op_C_bwd", x5, w, gE, gtaps)
    b, gg, f, h, ww = x5.shape
    work, gx, gw = torch.empty_like(x5), torch.empty_like(x5), torch.empty_like(w)
    _launch("subapi_bwd", 4 * (gE.numel() + 6 * x5.numel() + 2 * w.numel()), "grr_gtv_op_c_bwd", x5.data_ptr(),
            w.data_ptr(), st, gE.data_ptr(), work.data_ptr(), gx.data_ptr(), gw.data_ptr(), gtaps.data_ptr(),
            b, gg, f, h, ww, _stream(dev))
    return gx, gw


def gtv_op_C_transpose_bwd(e6: Tensor, w: Tensor, st: Stencil, z: Tensor, g: Tensor,
                           gtaps: Tensor) -> Tuple[Tensor, Tensor]:
    dev = _check("gtv_op_C_transpose_bwd", e6, w, z, g, gtaps)
    b, gg, f, four, h, ww = e6.shape
    work2, gE, gw = torch.empty_like(z), torch.empty_like(e6), torch.empty_like(w)
    _launch("subapi_bwd", 4 * (2 * e6.numel() + 4 * z.numel() + 2 * w.numel()), "grr_gtv_op_c_transpose_bwd",
            e6.data_ptr(), w.data_ptr(), st, z.data_ptr(), g.data_ptr(), work2.data_ptr(), gE.data_ptr(),
            gw.data_ptr(), gtaps.data_ptr(), b, gg, f, h, ww, _stream(dev))
    return gE, gw


# ---- feature CNN -----------------------------------------------------------
def conv1x1(x: Tensor, weight: Tensor) -> Tensor:
    """nn.Conv2d(K, M, 1, bias=False) with weight [M,K,1,1]."""
    dev = _check("conv1x1", x, weight)
    b, k, h, w = x.shape
    m = weight.shape[0]
    if weight.shape[1] != k:
        raise ValueError(f"conv1x1: weight {tuple(weight.shape)} vs input channels {k}")
    out = torch.empty((b, m, h, w), dtype=torch.float32, device=dev)
    kind = f"conv1x1[{k}->{m},{b}x{h}x{w}]" if TIMER_SHAPES else "conv1x1"
    ws_bytes = _native.load().grr_conv1x1_workspace_bytes(k, m)
    if ws_bytes > 0:   # split-bf16 MFMA path (fp32-accurate); K > 128 streams K (gemm_x3k_kernel)
        ws = torch.empty((ws_bytes + 3) // 4, dtype=torch.float32, device=dev)  # allocator: 512-B aligned
        _launch(kind, 4 * b * h * w * (k + m), "grr_conv1x1_ws", x.data_ptr(), weight.data_ptr(),
                out.data_ptr(), ws.data_ptr(), b, k, m, h * w, _stream(dev), flops=2 * b * h * w * k * m)
    else:
        _launch(kind, 4 * b * h * w * (k + m), "grr_conv1x1", x.data_ptr(), weight.data_ptr(),
                out.data_ptr(), b, k, m, h * w, _stream(dev), flops=2 * b * h * w * k * m)
    return out


def conv2x2s2(x: Tensor, weight: Tensor) -> Tensor:
    """nn.Conv2d(K, M, 2, stride=2, bias=False) with weight [M,K,2,2]."""
    dev = _check("conv2x2s2", x, weight)
    b, k, h, w = x.shape
    m = weight.shape[0]
    if tuple(weight.shape[1:]) != (k, 2, 2):
        raise ValueError(f"conv2x2s2: weight {tuple(weight.shape)} vs input channels {k}")
    out = torch.empty((b, m, h // 2, w // 2), dtype=torch.float32, device=dev)
    _launch("conv2x2s2", 4 * b * (h * w * k + (h // 2) * (w // 2) * m), "grr_conv2x2s2", x.data_ptr(),
            weight.data_ptr(), out.data_ptr(), b, k, m, h, w, _stream(dev))
    return out


# ---- v1.0 encoder / decoder convolutions (csrc/codec_ops.hip) -----------------
def _ws(nbytes: int, dev) -> Tensor:
    return torch.empty((max(int(nbytes), 4) + 3) // 4, dtype=torch.float32, device=dev)  # allocator: 512-B aligned


def conv3x3_embed_ok(cin: int, m: int) -> bool:
    """grr_conv3x3_embed_supported in plain Python (traceable; tests/test_codec_abi.py checks the two agree)."""
    return 1 <= cin <= 4 and 1 <= m <= 128


def convt2x2s2_ok(k: int, m: int, h: int, w: int) -> bool:
    """Where grr_convt2x2s2 applies (grr_convt2x2s2_workspace_bytes > 0 and its H*W limit), in plain Python."""
    return 1 <= k <= 4096 and 1 <= m <= (1 << 20) and h >= 1 and w >= 1 and h * w * 16 < (1 << 31)


def conv1x1_cat2_ok(ka: int, kb: int, m: int, p: int) -> bool:
    """grr_conv1x1_cat2_supported in plain Python: a k-step of 16 rows must lie in one source."""
    k = ka + kb
    return (ka >= 16 and ka % 16 == 0 and kb >= 1 and k <= 4096 and 1 <= m <= (1 << 20) and p >= 1
            and (k + 16) * p < (1 << 30) and (m + 128) * p < (1 << 30))


def _embed_shapes(name: str, x: Tensor, weight: Tensor) -> Tuple[int, int, int, int, int]:
    if x.dim() != 4 or weight.dim() != 4:
        raise ValueError(f"{name}: expected x [B,Cin,H,W] and weight [M,Cin,3,3]")
    b, cin, h, w = x.shape
    m = weight.shape[0]
    if tuple(weight.shape[1:]) != (cin, 3, 3):
        raise ValueError(f"{name}: weight {tuple(weight.shape)} vs input channels {cin}")
    if not conv3x3_embed_ok(cin, m) or min(b, h, w) < 1:
        raise ValueError(f"{name}: Cin={cin}, M={m} outside the kernel's range (Cin <= 4, M <= 128)")
    return b, cin, m, h, w


def conv3x3_embed(x: Tensor, weight: Tensor) -> Tensor:
    """nn.Conv2d(Cin, M, 3, padding=1, padding_mode="replicate", bias=False) with weight [M,Cin,3,3]."""
    dev = _check("conv3x3_embed", x, weight)
    b, cin, m, h, w = _embed_shapes("conv3x3_embed", x, weight)
    out = torch.empty((b, m, h, w), dtype=torch.float32, device=dev)
    _launch("conv3x3_embed", 4 * b * h * w * (cin + m), "grr_conv3x3_embed", x.data_ptr(), weight.data_ptr(),
            out.data_ptr(), b, cin, m, h, w, _stream(dev), flops=2 * b * h * w * 9 * cin * m)
    return out


def conv3x3_embed_bwd_w(g: Tensor, x: Tensor) -> Tensor:
    """Weight gradient of conv3x3_embed: g [B,M,H,W], x [B,Cin,H,W] -> [M,Cin,3,3] (fixed summation order)."""
    dev = _check("conv3x3_embed_bwd_w", g, x)
    if x.dim() != 4 or g.dim() != 4 or g.shape[0] != x.shape[0] or g.shape[2:] != x.shape[2:]:
        raise ValueError(f"conv3x3_embed_bwd_w: g {tuple(g.shape)} vs x {tuple(x.shape)}")
    b, cin, h, w = x.shape
    m = g.shape[1]
    if not conv3x3_embed_ok(cin, m) or min(b, h, w) < 1:
        raise ValueError(f"conv3x3_embed_bwd_w: Cin={cin}, M={m} outside the kernel's range (Cin <= 4, M <= 128)")
    g = _aligned16(g)   # grr_wgrad's 16-byte row loads; x is read by the scalar patch gather
    gw = torch.empty((m, cin, 3, 3), dtype=torch.float32, device=dev)
    ws = _ws(_native.load().grr_conv3x3_embed_bwd_w_workspace_bytes(b, cin, m, h, w), dev)
    _launch("conv3x3_embed_bwd_w", 4 * b * h * w * (m + cin + 18 * cin), "grr_conv3x3_embed_bwd_w", g.data_ptr(),
            x.data_ptr(), gw.data_ptr(), ws.data_ptr(), b, cin, m, h, w, _stream(dev),
            flops=2 * b * h * w * 9 * cin * m)
    return gw


def conv3x3_embed_bwd_x(g: Tensor, weight: Tensor) -> Tensor:
    """Data gradient of conv3x3_embed: g [B,M,H,W], weight [M,Cin,3,3] -> [B,Cin,H,W]."""
    dev = _check("conv3x3_embed_bwd_x", g, weight)
    if g.dim() != 4 or weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3) or weight.shape[0] != g.shape[1]:
        raise ValueError(f"conv3x3_embed_bwd_x: g {tuple(g.shape)} vs weight {tuple(weight.shape)}")
    b, m, h, w = g.shape
    cin = weight.shape[1]
    if not conv3x3_embed_ok(cin, m) or min(b, h, w) < 1:
        raise ValueError(f"conv3x3_embed_bwd_x: Cin={cin}, M={m} outside the kernel's range (Cin <= 4, M <= 128)")
    gx = torch.empty((b, cin, h, w), dtype=torch.float32, device=dev)
    _launch("conv3x3_embed_bwd_x", 4 * b * h * w * (m + cin), "grr_conv3x3_embed_bwd_x", g.data_ptr(),
            weight.data_ptr(), gx.data_ptr(), b, cin, m, h, w, _stream(dev), flops=2 * b * h * w * 9 * cin * m)
    return gx


def convt2x2s2(x: Tensor, weight: Tensor) -> Tensor:
    """nn.ConvTranspose2d(K, M, 2, stride=2, bias=False) with weight [K,M,2,2]: x [B,K,H,W] -> [B,M,2H,2W]."""
    dev = _check("convt2x2s2", x, weight)
    if x.dim() != 4 or weight.dim() != 4:
        raise ValueError("convt2x2s2: expected x [B,K,H,W] and weight [K,M,2,2]")
    b, k, h, w = x.shape
    m = weight.shape[1]
    if tuple(weight.shape) != (k, m, 2, 2):
        raise ValueError(f"convt2x2s2: weight {tuple(weight.shape)} vs input channels {k}")
    if not convt2x2s2_ok(k, m, h, w) or b < 1:
        raise ValueError(f"convt2x2s2: shape {tuple(x.shape)} -> {m} channels outside the kernel's range")
    out = torch.empty((b, m, 2 * h, 2 * w), dtype=torch.float32, device=dev)
    ws = _ws(_native.load().grr_convt2x2s2_workspace_bytes(b, k, m, h, w), dev)
    kind = f"convt2x2s2[{k}->{m},{b}x{h}x{w}]" if TIMER_SHAPES else "convt2x2s2"
    _launch(kind, 4 * b * h * w * (k + 4 * m), "grr_convt2x2s2", x.data_ptr(), weight.data_ptr(), out.data_ptr(),
            ws.data_ptr(), b, k, m, h, w, _stream(dev), flops=2 * b * h * w * k * 4 * m)
    return out


def conv1x1_cat2(xa: Tensor, xb: Tensor, weight: Tensor) -> Tensor:
    """nn.Conv2d(Ka + Kb, M, 1, bias=False) on cat([xa, xb], 1), weight [M,Ka+Kb,1,1].  Where grr_conv1x1_cat2
    applies (conv1x1_cat2_ok) the concatenation is never written and the result is bitwise conv1x1's on it;
    elsewhere this concatenates and calls conv1x1."""
    dev = _check("conv1x1_cat2", xa, xb, weight)
    if xa.dim() != 4 or xb.dim() != 4 or xa.shape[0] != xb.shape[0] or xa.shape[2:] != xb.shape[2:]:
        raise ValueError(f"conv1x1_cat2: inputs {tuple(xa.shape)} and {tuple(xb.shape)} disagree")
    b, ka, h, w = xa.shape
    kb = xb.shape[1]
    m = weight.shape[0]
    if weight.numel() != m * (ka + kb) or weight.shape[1] != ka + kb:
        raise ValueError(f"conv1x1_cat2: weight {tuple(weight.shape)} vs input channels {ka} + {kb}")
    if not conv1x1_cat2_ok(ka, kb, m, h * w):
        return conv1x1(torch.cat([xa, xb], 1), weight)
    out = torch.empty((b, m, h, w), dtype=torch.float32, device=dev)
    ws = _ws(_native.load().grr_conv1x1_cat2_workspace_bytes(ka, kb, m), dev)
    kind = f"conv1x1_cat2[{ka}+{kb}->{m},{b}x{h}x{w}]" if TIMER_SHAPES else "conv1x1_cat2"
    _launch(kind, 4 * b * h * w * (ka + kb + m), "grr_conv1x1_cat2", xa.data_ptr(), xb.data_ptr(), weight.data_ptr(),
            out.data_ptr(), ws.data_ptr(), b, ka, kb, m, h * w, _stream(dev), flops=2 * b * h * w * (ka + kb) * m)
    return out


def ffn_forward(x: Tensor, ln_w: Tensor, w_in: Tensor, w_dw: Tensor, w_out: Tensor, skip: Tensor) -> Tensor:
    """FFBlock of the window models' feature CNN (grr_ffn_forward, REF7:13-67): x [B,C,H,W]; ln_w [C];
    w_in [2 hid, C]; w_dw [2 hid, 9]; w_out [C, hid]; skip [2]."""
    dev = _check("ffn_forward", x, ln_w, w_in, w_dw, w_out, skip)
    b, c, h, w = x.shape
    hid = w_out.shape[1]
    if tuple(w_in.shape) != (2 * hid, c) or tuple(w_dw.shape) != (2 * hid, 9) or tuple(w_out.shape) != (c, hid) \
            or ln_w.numel() != c or skip.numel() != 2:
        raise ValueError("ffn_forward: weight shapes disagree with x / hid")
    out = torch.empty_like(x)
    ws = torch.empty((_native.load().grr_ffn_workspace_bytes(b, c, hid, h, w) + 3) // 4, dtype=torch.float32,
                     device=dev)
    p = b * h * w
    _launch("ffn", 4 * p * (2 * c + 3 * hid + 2 * hid), "grr_ffn_forward", x.data_ptr(), ln_w.data_ptr(),
            w_in.data_ptr(), w_dw.data_ptr(), w_out.data_ptr(), skip.data_ptr(), out.data_ptr(), ws.data_ptr(),
            b, c, hid, h, w, _stream(dev), flops=p * (2 * c * 2 * hid + 18 * 2 * hid + 2 * hid * c))
    return out


def wgrad(a: Tensor, bop: Tensor) -> Tensor:
    """Weight gradient out[m, k] = sum_b sum_p a[b, m, p] bop[b, k, p] (grr_wgrad): a [B, M, ...],
    bop [B, K, ...] with the same trailing pixel extent.  The reverse of a 1x1 conv / LNB GEMM's
    weight (REF:556-612 under autograd) without a library GEMM: split-bf16 MFMA (three exact bf16 terms per
    operand, six products accumulated in fp32: fp32-accurate), fixed summation order.  grr_wgrad wants 16-byte
    aligned operands; a contiguous view that is not (a batch slice at an odd offset) is copied first."""
    dev = _check("wgrad", a, bop)
    a, bop = _aligned16(a), _aligned16(bop)
    b, m = a.shape[:2]
    k = bop.shape[1]
    p = a.numel() // (b * m)
    if bop.shape[0] != b or bop.numel() != b * k * p:
        raise ValueError(f"wgrad: operands {tuple(a.shape)} and {tuple(bop.shape)} disagree")
    out = torch.empty((m, k), dtype=torch.float32, device=dev)
    ws = torch.empty((_native.load().grr_wgrad_workspace_bytes(b, m, k, p) + 3) // 4, dtype=torch.float32,
                     device=dev)
    _launch(f"wgrad[{m}x{k},{b}x{p}]" if TIMER_SHAPES else "wgrad", 4 * b * p * (m + k), "grr_wgrad", a.data_ptr(), bop.data_ptr(), out.data_ptr(), ws.data_ptr(),
            b, m, k, p, _stream(dev), flops=2 * b * p * m * k)
    return out


def set_wgrad_tiles(enable: bool) -> None:
    """grr_wgrad's per-shape wave tile (True, default) or the 128 x 96 tile only (grr_wgrad_set_tiles)."""
    _native.call("grr_wgrad_set_tiles", int(bool(enable)))


_WS_CACHE = {}


# the LNB kernels address one image's [max(hid, C), H, W] planes with 32-bit byte offsets
_LNB_MAX_BYTES = 1 << 31


def _lnb_band_rows(c: int, hid: int, h: int, w: int) -> int:
    """Rows per band so one band (+ its two halo rows) fits the kernels' 32-bit image offsets."""
    per_row = max(hid, c) * w * 4
    return h if per_row * h < _LNB_MAX_BYTES else max(1, (_LNB_MAX_BYTES - 1) // per_row - 2)


def _lnb_banded(run, xs, h: int, rows: int) -> Tensor:
    """Run an LNB forward on row bands of a tall image: the block's only spatial op is the
    depthwise 3x3 (replicate pad), so output rows [r0, r1) need input rows [r0-1, r1+1), and the
    band's own edge padding only reaches the halo rows, which are dropped."""
    outs = []
    for r0 in range(0, h, rows):
        r1 = min(r0 + rows, h)
        a, e = max(r0 - 1, 0), min(r1 + 1, h)
        y = run(*[None if t is None else t[:, :, a:e].contiguous() for t in xs])
        outs.append(y[:, :, r0 - a:r1 - a])
    return torch.cat(outs, 2)


def lnb_forward(x: Tensor, ln_w: Tensor, w1: Tensor, wdw: Tensor, w2: Tensor, skip: Tensor) -> Tensor:
    """LocalNonLinearBlock (nsubnets = 1) forward."""
    dev = _check("lnb_forward", x, ln_w, w1, wdw, w2, skip)
    b, c, h, w = x.shape
    hid = w2.shape[1]
    rows = _lnb_band_rows(c, hid, h, w)
    if rows < h:
        return _lnb_banded(lambda xb: lnb_forward(xb, ln_w, w1, wdw, w2, skip), [x], h, rows)
    lib = _native.load()
    fused = bool(lib.grr_lnb_fused(c, hid))
    # the fused pass needs only its chunk images (g stays on chip); the two-kernel path g + images
    nbytes = lib.grr_lnb_fused_workspace_bytes(c, hid) if fused else lib.grr_lnb_workspace_bytes(b, c, hid, h, w)
    ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=dev)
    out = torch.empty_like(x)
    args = (x.data_ptr(), ln_w.data_ptr(), w1.data_ptr(), wdw.data_ptr(), w2.data_ptr(), skip.data_ptr(),
            out.data_ptr(), ws.data_ptr(), b, c, hid, h, w, _stream(dev))
    if fused:
        # one fused pass (lnb_fused16_kernel): x in (its halo and the skip read once), out written; the
        # gated activation stays on chip
        _launch("lnb_fused", 4 * b * h * w * 2 * c, "grr_lnb_forward", *args, flops=lnb_flops(b * h * w, c, c, hid))
        return out
    if _lnb_split(c):
        _lnb_timed_parts("grr_lnb_forward", args, b * h * w, c, c, hid, c)
        return out
    # C <= 128: x (head), gated g (hid) written and read back once, residual x, out
    nbytes_algo = 4 * b * h * w * (3 * c + 2 * hid) if c <= 128 else 4 * b * h * w * (3 * c + 2 * (2 * hid) + 2 * hid)
    _launch("lnb", nbytes_algo, "grr_lnb_forward", *args, flops=lnb_flops(b * h * w, c, c, hid))
    return out


def c8_shape(b: int, c: int, h: int, w: int) -> Tuple[int, int, int, int, int]:
    """Shape of the channel-blocked layout of a [B, C, H, W] tensor: [B, ceil(C / 8), H, W, 8]."""
    return (b, (c + 7) // 8, h, w, 8)


def to_c8(x: Tensor) -> Tensor:
    """[B, C, H, W] -> the channel-blocked layout (grr_c8_convert; pad channels 0)."""
    dev = _check("to_c8", x)
    b, c, h, w = x.shape
    y = torch.empty(c8_shape(b, c, h, w), dtype=torch.float32, device=dev)
    _launch("c8_convert", 8 * y.numel(), "grr_c8_convert", x.contiguous().data_ptr(), y.data_ptr(), b, c, h, w, 1,
            _stream(dev))
    return y


def from_c8(y: Tensor, c: int) -> Tensor:
    """The channel-blocked layout -> [B, C, H, W]."""
    dev = _check("from_c8", y)
    b, nb, h, w, _ = y.shape
    x = torch.empty((b, c, h, w), dtype=torch.float32, device=dev)
    _launch("c8_convert", 8 * x.numel(), "grr_c8_convert", y.data_ptr(), x.data_ptr(), b, c, h, w, 0, _stream(dev))
    return x


# Python mirror of grr_lnb_set_fused (set_lnb_fused keeps both): the layout decisions below are plain Python so
# that Dynamo traces them (a ctypes query would break the graph); a stale mirror fails loudly in the C entry
# point (GRR_ERR_UNSUPPORTED), never silently
LNB_FUSED = True


def set_lnb_fused(enable: bool) -> None:
    """C <= 96 blocks as one fused pass (default) or on the head + mix kernels (grr_lnb_set_fused)."""
    global LNB_FUSED
    _native.call("grr_lnb_set_fused", int(bool(enable)))
    LNB_FUSED = bool(enable)


def lnb_c8_ok(c: int, hid: int, h: int, w: int) -> bool:
    """Where lnb_forward_c8 applies: the fused C <= 96 pass (grr_lnb_fused), one band."""
    return LNB_FUSED and 2 <= c <= 96 and hid >= 1 and _lnb_band_rows(c, hid, h, w) >= h and \
        ((c + 7) // 8) * 8 * h * w * 4 < (1 << 31)


def lnb_forward_c8(x: Tensor, c: int, ln_w: Tensor, w1: Tensor, wdw: Tensor, w2: Tensor, skip: Tensor,
                   in_c8: bool, out_c8: bool) -> Tensor:
    """lnb_forward with x and / or out in the channel-blocked layout (grr_lnb_forward_c8): a chain of fused
    blocks hands the blocked tensor on, the kernel then loads and stores 16 / 32 bytes per lane instead of
    dwords.  Bitwise equal to lnb_forward.  lnb_c8_ok must hold."""
    dev = _check("lnb_forward_c8", x, ln_w, w1, wdw, w2, skip)
    if in_c8:
        b, _, h, w, _ = x.shape
    else:
        b, c_in, h, w = x.shape
        if c_in != c:
            raise ValueError("lnb_forward_c8: channels")
    hid = w2.shape[1]
    lib = _native.load()
    ws = torch.empty((lib.grr_lnb_fused_workspace_bytes(c, hid) + 3) // 4, dtype=torch.float32, device=dev)
    out = torch.empty(c8_shape(b, c, h, w) if out_c8 else (b, c, h, w), dtype=torch.float32, device=dev)
    xc = x.contiguous()
    _launch("lnb_fused", 4 * b * h * w * 2 * c, "grr_lnb_forward_c8", xc.data_ptr(), ln_w.data_ptr(), w1.data_ptr(),
            wdw.data_ptr(), w2.data_ptr(), skip.data_ptr(), out.data_ptr(), ws.data_ptr(), b, c, hid, h, w,
            int(in_c8) | 2 * int(out_c8), _stream(dev), flops=lnb_flops(b * h * w, c, c, hid))
    return out


def lnb_gate_keepable(c: int, hid: int, h: int, w: int) -> bool:
    """lnb_forward_keep's shapes: the C <= 128 head + mix pipeline in one band (its workspace starts
    with the gated activation g [B, hid, H, W])."""
    return 2 <= c <= 128 and _lnb_band_rows(c, hid, h, w) >= h


def lnb_forward_keep(x: Tensor, ln_w: Tensor, w1: Tensor, wdw: Tensor, w2: Tensor,
                     skip: Tensor) -> Tuple[Tensor, Tensor]:
    """lnb_forward that also returns the head's gated activation g = sigmoid(m) m v,
    [B, hid, H, W] (a view of the launch's workspace), for the training reverse's W2 weight gradient."""
    dev = _check("lnb_forward_keep", x, ln_w, w1, wdw, w2, skip)
    b, c, h, w = x.shape
    hid = w2.shape[1]
    if not lnb_gate_keepable(c, hid, h, w):
        raise ValueError("lnb_forward_keep: needs C <= 128 and one band")
    nbytes = _native.load().grr_lnb_workspace_bytes(b, c, hid, h, w)
    ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=dev)
    out = torch.empty_like(x)
    args = (x.data_ptr(), ln_w.data_ptr(), w1.data_ptr(), wdw.data_ptr(), w2.data_ptr(), skip.data_ptr(),
            out.data_ptr(), ws.data_ptr(), b, c, hid, h, w, _stream(dev))
    if _native.load().grr_lnb_fused(c, hid):
        # the fused pass also stores g (fp32) at the workspace's start: x in, out and g written
        _launch("lnb_fused", 4 * b * h * w * (2 * c + hid), "grr_lnb_forward_keep", *args,
                flops=lnb_flops(b * h * w, c, c, hid))
    elif _lnb_split(c):
        _lnb_timed_parts("grr_lnb_forward_keep", args, b * h * w, c, c, hid, c)
    else:
        _launch("lnb", 4 * b * h * w * (3 * c + 2 * hid), "grr_lnb_forward_keep", *args,
                flops=lnb_flops(b * h * w, c, c, hid))
    return out, ws[:b * hid * h * w].view(b, hid, h, w)


def lnb_forward_rep(src: Tensor, x: Optional[Tensor], ln_w: Tensor, w1: Tensor, wdw: Tensor, w2: Tensor,
                    skip: Tensor) -> Tensor:
    """LocalNonLinearBlock forward when its input [B, R*Cs, H, W] is R copies of src [B, Cs, H, W];
    x is that replicated input (read by the skip) or None (the skip reads src)."""
    dev = _check("lnb_forward_rep", src, x, ln_w, w1, wdw, w2, skip)
    b, cs, h, w = src.shape
    c = ln_w.numel()
    if c % cs or (x is not None and tuple(x.shape) != (b, c, h, w)):
        raise ValueError("lnb_forward_rep: the block input must be copies of src")
    hid = w2.shape[1]
    rows = _lnb_band_rows(c, hid, h, w)
    if rows < h:
        return _lnb_banded(lambda sb, xb: lnb_forward_rep(sb, xb, ln_w, w1, wdw, w2, skip), [src, x], h, rows)
    nbytes = _native.load().grr_lnb_workspace_bytes(b, c, hid, h, w)
    ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=dev)
    out = torch.empty((b, c, h, w), dtype=torch.float32, device=dev)
    args = (src.data_ptr(), cs, c // cs, _ptr(x), ln_w.data_ptr(), w1.data_ptr(), wdw.data_ptr(), w2.data_ptr(),
            skip.data_ptr(), out.data_ptr(), ws.data_ptr(), b, hid, h, w, _stream(dev))
    if _native.load().grr_lnb_rep_fused(cs, c // cs, c, hid):
        # one fused pass (lnb_rep_kernel): src with its 3x3 halo in, out written; no gated tensor in memory
        _launch("lnb_rep_fused", 4 * b * h * w * (cs + 2 * c if x is not None else cs + c), "grr_lnb_forward_rep",
                *args, flops=lnb_flops(b * h * w, cs, c, hid))
        return out
    if _lnb_split(c):
        _lnb_timed_parts("grr_lnb_forward_rep", args, b * h * w, cs, c, hid, c if x is not None else cs)
        return out
    _launch("lnb", 4 * b * h * w * (cs + 2 * c + 2 * hid), "grr_lnb_forward_rep", *args,
            flops=lnb_flops(b * h * w, cs, c, hid))
    return out


# LaunchTimer with split_lnb: the head (LN + W1 + depthwise + gate) and the mix (W2 + skip) of a C <= 128
# block are launched and timed apart on one workspace (grr_lnb_set_phases), as kinds "lnb_head" / "lnb_mix"
def _lnb_split(c: int) -> bool:
    return _TIMER is not None and getattr(_TIMER, "split_lnb", False) and c <= 128


def lnb_head_flops(px: int, c_head: int, hid: int) -> int:
    """Algorithmic fp32 flops of the head: LN (4 per input channel), W1 (2 c_head 2hid), depthwise 3x3
    (18 per hidden channel), gate (4 per gated channel)."""
    return px * (4 * c_head + 2 * c_head * 2 * hid + 18 * 2 * hid + 4 * hid)


def _lnb_timed_parts(name: str, args, px: int, c_head: int, c: int, hid: int, c_skip: int) -> None:
    try:
        call("grr_lnb_set_phases", 3)
        _launch("lnb_head", 4 * px * (c_head + hid), name, *args, flops=lnb_head_flops(px, c_head, hid))
        call("grr_lnb_set_phases", 4)
        _launch("lnb_mix", 4 * px * (hid + c_skip + c), name, *args, flops=px * (2 * hid * c + 3 * c))
    finally:
        call("grr_lnb_set_phases", 7)


def repeat_graphs(img: Tensor, n_graphs: int) -> Tensor:
    dev = _check("repeat_graphs", img)
    b, cin, h, w = img.shape
    out = torch.empty((b, n_graphs * cin, h, w), dtype=torch.float32, device=dev)
    _launch("repeat_graphs", 4 * b * h * w * cin * (1 + n_graphs), "grr_repeat_graphs", img.data_ptr(),
            out.data_ptr(), b, cin, n_graphs, h * w, _stream(dev))
    return out


# ---- reverse pass (training) ------------------------------------------------
# Modes of grr_bwd_stencil / grr_bwd_tapgrad
ST_P, ST_T, ST_T_ADJ, ST_P_ADJ = 0, 1, 2, 3


def stencil_taps(p01: Tensor, p02a: Tensor, p02b: Tensor, p03: Tensor) -> Tensor:
    """[C,5] taps (centre, up, left, right, down) of the 3x3 cross stencil
    p01*k01 + p02a*k02a + p02b*k02b + p03*k03 (REF:56-118, :178-183)."""
    a, b, c, d = (t.reshape(-1) for t in (p01, p02a, p02b, p03))
    return torch.stack([a - b - c + 4 * d, -d, -d, b - d, c - d], dim=1).contiguous()


def stencil_taps_backward(gt: Tensor):
    """Chain [C,5] tap gradients back to (p01, p02a, p02b, p03) gradients, each [C,1,1,1]."""
    dc, du, dl, dr, dd = gt.unbind(1)
    out = (dc, dr - dc, dd - dc, 4 * dc - du - dl - dr - dd)
    return tuple(t.reshape(-1, 1, 1, 1) for t in out)


def _bgfhw(x: Tensor, n_graphs: int):
    b, c, h, w = x.shape
    if c % n_graphs:
        raise ValueError(f"{c} channels not divisible by {n_graphs} graphs")
    return b, n_graphs, c // n_graphs, h, w


def bwd_stencil(x: Tensor, taps: Tensor, mode: int, n_graphs: int, scale: Optional[Tensor] = None,
                out: Optional[Tensor] = None) -> Tensor:
    """out = [out +] scale[g] * mode(x)  (out given -> accumulate)."""
    dev = _check("bwd_stencil", x, taps, scale, out)
    acc = out is not None
    if out is None:
        out = torch.empty_like(x)
    _launch("bwd_stencil", 4 * x.numel() * (3 if acc else 2), "grr_bwd_stencil", x.data_ptr(), taps.data_ptr(), mode,
            _ptr(scale), int(acc), out.data_ptr(), *_bgfhw(x, n_graphs), _stream(dev))
    return out


def padj2_ok(x: Tensor) -> bool:
    return x.shape[3] % 4 == 0


def bwd_padj2(v1: Tensor, taps1: Tensor, scale1: Tensor, v2: Tensor, taps2: Tensor, scale2: Tensor, out: Tensor,
              n_graphs: int) -> None:
    """out += scale1[g] P1*(v1) + scale2[g] P2*(v2) in one pass (the two x-gradient passes of a level's terms)."""
    dev = _check("bwd_padj2", v1, taps1, scale1, v2, taps2, scale2, out)
    _launch("bwd_stencil", 4 * v1.numel() * 4, "grr_bwd_padj2", v1.data_ptr(), taps1.data_ptr(), scale1.data_ptr(),
            v2.data_ptr(), taps2.data_ptr(), scale2.data_ptr(), out.data_ptr(), *_bgfhw(v1, n_graphs), _stream(dev))


def bwd_tapgrad(u: Tensor, z: Tensor, mode: int, n_graphs: int, scale: Optional[Tensor], gtaps: Tensor) -> None:
    dev = _check("bwd_tapgrad", u, z, scale, gtaps)
    _launch("bwd_tapgrad", 8 * u.numel(), "grr_bwd_tapgrad", u.data_ptr(), z.data_ptr(), mode, _ptr(scale),
            gtaps.data_ptr(), *_bgfhw(u, n_graphs), _stream(dev))


def bwd_glr(s: Tensor, a: Tensor, w: Tensor, scale: Tensor, coef: float, gw: Tensor, gdot: Tensor, n_graphs: int):
    dev = _check("bwd_glr", s, a, w, scale, gw, gdot)
    z, ap = torch.empty_like(s), torch.empty_like(s)
    _launch("bwd_glr", 4 * (4 * s.numel() + 3 * w.numel()), "grr_bwd_glr", s.data_ptr(), a.data_ptr(), w.data_ptr(),
            scale.data_ptr(), float(coef), z.data_ptr(), ap.data_ptr(), gw.data_ptr(), _ptr(gdot),
            *_bgfhw(s, n_graphs), _stream(dev))
    return z, ap


def bwd_pair(s: Tensor, a: Tensor, c: Tensor, scale: Tensor, coef: float, gc: Tensor, gdot: Tensor, n_graphs: int):
    dev = _check("bwd_pair", s, a, c, scale, gc, gdot)
    z, ap = torch.empty_like(s), torch.empty_like(s)
    _launch("bwd_pair", 4 * (4 * s.numel() + 3 * c.numel()), "grr_bwd_pair", s.data_ptr(), a.data_ptr(), c.data_ptr(),
            scale.data_ptr(), float(coef), z.data_ptr(), ap.data_ptr(), gc.data_ptr(), _ptr(gdot),
            *_bgfhw(s, n_graphs), _stream(dev))
    return z, ap


def bwd_prox(s: Tensor, a: Tensor, w: Tensor, log_gamma: Tensor, scale: Tensor, coef: float, gw: Tensor,
             ggamma: Tensor, gdot: Tensor, n_graphs: int):
    dev = _check("bwd_prox", s, a, w, log_gamma, scale, gw, ggamma, gdot)
    o, gs = torch.empty_like(s), torch.empty_like(s)
    _launch("bwd_prox", 4 * (4 * s.numel() + 3 * w.numel()), "grr_bwd_prox", s.data_ptr(), a.data_ptr(),
            w.data_ptr(), log_gamma.data_ptr(), scale.data_ptr(), float(coef), o.data_ptr(), gs.data_ptr(),
            gw.data_ptr(), ggamma.data_ptr(), gdot.data_ptr(), *_bgfhw(s, n_graphs), _stream(dev))
    return o, gs


# node-feature counts with a fused reverse instance (measured slower than the multi-pass path
# for F = 6 and 12: 49.6 vs 46.5 ms of term reverses per v1.0 training step at 8 x 256^2)
FUSED_TERM_FTS = (1, 2, 3, 4)
TERM_GLR, TERM_PAIR, TERM_PROX = 0, 1, 2


def bwd_term_fused(mode: int, x: Tensor, g: Tensor, taps: Tensor, w: Tensor, log_gamma: Optional[Tensor],
                   scale: Tensor, coef: float, gw: Tensor, ggamma: Optional[Tensor], gdot: Optional[Tensor],
                   gtaps: Tensor, n_graphs: int) -> Tensor:
    """One-pass reverse of an operator term (grr_bwd_term_fused); returns v for the P* pass."""
    dev = _check("bwd_term_fused", x, g, taps, w, log_gamma, scale, gw, ggamma, gdot, gtaps)
    v = torch.empty_like(x)
    _launch("bwd_term_fused", 4 * (3 * x.numel() + 3 * w.numel()), "grr_bwd_term_fused", mode, x.data_ptr(),
            g.data_ptr(), taps.data_ptr(), w.data_ptr(), _ptr(log_gamma), scale.data_ptr(), float(coef),
            v.data_ptr(), gw.data_ptr(), _ptr(ggamma), _ptr(gdot), gtaps.data_ptr(), *_bgfhw(x, n_graphs),
            _stream(dev))
    return v


def term_acc_ok(mode: int, x: Tensor, n_graphs: int, *planes: Tensor) -> bool:
    """Whether grr_bwd_term_fused_acc takes this term reverse (row kernel with the P* pass inside)."""
    b, c, h, w = x.shape
    if not TERM_ROWS or c % n_graphs or any(t.data_ptr() % 16 for t in (x, *planes)):
        return False
    return bool(_native.load().grr_bwd_term_acc_supported(mode, c // n_graphs, h, w))


def bwd_term_fused_acc(mode: int, x: Tensor, g: Tensor, taps: Tensor, w: Tensor, log_gamma: Optional[Tensor],
                       scale: Tensor, coef: float, gx: Tensor, gw: Tensor, ggamma: Optional[Tensor],
                       gdot: Optional[Tensor], gtaps: Tensor, n_graphs: int) -> None:
    """bwd_term_fused + bwd_stencil(v, taps, ST_P_ADJ, scale, out=gx) in one pass (grr_bwd_term_fused_acc):
    gx += scale[g] P*(v), v never written (term_acc_ok must hold)."""
    dev = _check("bwd_term_fused", x, g, taps, w, log_gamma, scale, gx, gw, ggamma, gdot, gtaps)
    if gx.shape != x.shape:
        raise ValueError(f"bwd_term_fused_acc: gx {tuple(gx.shape)} vs x {tuple(x.shape)}")
    _launch("bwd_term_fused", 4 * (4 * x.numel() + 3 * w.numel()), "grr_bwd_term_fused_acc", mode, x.data_ptr(),
            g.data_ptr(), taps.data_ptr(), w.data_ptr(), _ptr(log_gamma), scale.data_ptr(), float(coef),
            gx.data_ptr(), gw.data_ptr(), _ptr(ggamma), _ptr(gdot), gtaps.data_ptr(), *_bgfhw(x, n_graphs),
            _stream(dev))


def bwd_pair_weights(w: Tensor, gc: Tensor, gw: Tensor) -> None:
    dev = _check("bwd_pair_weights", w, gc, gw)
    b, g, _, h, ww = w.shape
    _launch("bwd_pair_weights", 4 * (3 * w.numel() + gc.numel()), "grr_bwd_pair_weights", w.data_ptr(),
            gc.data_ptr(), gw.data_ptr(), b, g, h, ww, _stream(dev))


def bwd_edge_weights(feat: Tensor, channel_offset: int, n_graphs: int, n_fts: int, multiM: Tensor, w: Tensor,
                     gw: Tensor, gfeat: Tensor, gmultiM: Tensor) -> None:
    """Writes the gradient of the [G*F] slab at channel_offset of gfeat (same shape as feat)."""
    dev = _check("bwd_edge_weights", feat, multiM, w, gw, gfeat, gmultiM)
    b, ctot, h, ww = feat.shape
    if gfeat.shape != feat.shape or channel_offset + n_graphs * n_fts > ctot:
        raise ValueError("bwd_edge_weights: bad slab")
    off = channel_offset * h * ww * 4
    _launch("bwd_edge_weights", 4 * b * h * ww * (2 * n_graphs * n_fts + 8 * n_graphs), "grr_bwd_edge_weights",
            feat.data_ptr() + off, ctot * h * ww, multiM.data_ptr(), w.data_ptr(), gw.data_ptr(),
            gfeat.data_ptr() + off, ctot * h * ww, gmultiM.data_ptr(), b, n_graphs, n_fts, h, ww, _stream(dev))


def bwd_graph_dot(u: Tensor, v: Tensor, out: Tensor, n_graphs: int, coef: float = 1.0) -> None:
    """out[g] += coef * sum over (b, f, pixels) of u * v."""
    dev = _check("bwd_graph_dot", u, v, out)
    _launch("bwd_graph_dot", 8 * u.numel(), "grr_bwd_graph_dot", u.data_ptr(), v.data_ptr(), float(coef),
            out.data_ptr(), *_bgfhw(u, n_graphs), _stream(dev))


def bwd_lincomb(x: Tensor, sa: Optional[Tensor], y: Optional[Tensor], sb: Optional[Tensor], n_graphs: int,
                out: Optional[Tensor] = None, accumulate: bool = False) -> Tensor:
    """out = [out +] sa[g] x + sb[g] y (per-graph coefficient vectors; None = 1)."""
    dev = _check("bwd_lincomb", x, sa, y, sb, out)
    if out is None:
        out = torch.empty_like(x)
        accumulate = False
    _launch("bwd_lincomb", 4 * x.numel() * (2 + int(y is not None) + int(accumulate)), "grr_bwd_lincomb",
            x.data_ptr(), _ptr(sa), _ptr(y), _ptr(sb), out.data_ptr(), int(accumulate), *_bgfhw(x, n_graphs),
            _stream(dev))
    return out


def bwd_cg_glue(gx: Tensor, u: Tensor, gu_next: Optional[Tensor], u_prev: Optional[Tensor], alpha: Tensor,
                beta_next: Optional[Tensor], gbb: Optional[Tensor], galpha: Tensor, gbeta: Optional[Tensor],
                n_graphs: int, inplace: bool = False, gx_half: Optional[Tensor] = None,
                padj: Optional[tuple] = None, want_pool: bool = False):
    """One reverse step of the stage recurrence glue (grr_bwd_cg_glue): returns (gu, gx - gu), and
    D gu third when want_pool (grr_bwd_cg_glue_pool; glue_pool_ok must hold);
    galpha / gbeta accumulate <gx, u> / <gu, u_prev>, gbb += gu.  inplace: gx - gu overwrites gx.
    Passes of the previous stage folded in (gx taken as ((gx + s1 P1*(v1)) + s2 P2*(v2)) + U gx_half):
    padj = (v1, taps1, s1, v2, taps2, s2), bwd_padj2's operands (padj2_ok); gx_half, bwd_unpool2_acc's."""
    v1, t1, s1, v2, t2, s2 = padj if padj is not None else (None,) * 6
    dev = _check("bwd_cg_glue", gx, gx_half, v1, t1, s1, v2, t2, s2, u, gu_next, u_prev, alpha, beta_next, gbb,
                 galpha, gbeta)
    for t in (v1, v2):
        if t is not None and t.shape != gx.shape:
            raise ValueError("bwd_cg_glue: padj shapes")
    for t in (u, gu_next, u_prev, gbb):
        if t is not None and t.shape != gx.shape:
            raise ValueError("bwd_cg_glue: shapes")
    b, c, h, w = gx.shape
    if gx_half is not None and tuple(gx_half.shape) != (b, c, h // 2, w // 2):
        raise ValueError("bwd_cg_glue: gx_half shape")
    gu = torch.empty_like(gx)
    gx_out = gx if inplace else torch.empty_like(gx)
    n_rw = 2 + int(gu_next is not None) + int(u_prev is not None) + 2 * int(gbb is not None) + 2
    n_rw += 2 * int(v1 is not None)
    nbytes = 4 * (gx.numel() * n_rw + (0 if gx_half is None else gx_half.numel()))
    ptrs = (gx.data_ptr(), _ptr(gx_half), _ptr(v1), _ptr(t1), _ptr(s1), _ptr(v2), _ptr(t2), _ptr(s2),
            u.data_ptr(), _ptr(gu_next), _ptr(u_prev), alpha.data_ptr(), _ptr(beta_next), gu.data_ptr(), _ptr(gbb),
            gx_out.data_ptr())
    if want_pool:
        gud = torch.empty((b, c, h // 2, w // 2), dtype=torch.float32, device=dev)
        _launch("bwd_cg_glue", nbytes + gx.numel(), "grr_bwd_cg_glue_pool", *ptrs, gud.data_ptr(),
                galpha.data_ptr(), _ptr(gbeta), *_bgfhw(gx, n_graphs), _stream(dev))
        return gu, gx_out, gud
    _launch("bwd_cg_glue", nbytes, "grr_bwd_cg_glue", *ptrs, galpha.data_ptr(), _ptr(gbeta),
            *_bgfhw(gx, n_graphs), _stream(dev))
    return gu, gx_out


def glue_pool_ok(x: Tensor, *planes: Optional[Tensor], gx_half: Optional[Tensor] = None) -> bool:
    """Where grr_bwd_cg_glue_pool takes the glue: W % 4 == 0, even H, and every operand plane the pass
    reads on its float4 path (x = gx, then u, gu_next, u_prev, gbb, the padj v planes: None = absent)
    16-byte aligned, gx_half 8-byte aligned (the outputs are fresh torch allocations)."""
    b, c, h, w = x.shape
    if w % 4 or h % 2 or any(t is not None and t.data_ptr() % 16 for t in (x, *planes)):
        return False
    return gx_half is None or gx_half.data_ptr() % 8 == 0


def bwd_unpool2_acc(xd: Tensor, out: Tensor) -> None:
    dev = _check("bwd_unpool2_acc", xd, out)
    b, c, h, w = out.shape
    _launch("bwd_unpool2_acc", 4 * (2 * out.numel() + xd.numel()), "grr_bwd_unpool2_acc", xd.data_ptr(),
            out.data_ptr(), b, c, h, w, _stream(dev))


def conv2x2s2_bwd_data_gemm(g: Tensor, weight: Tensor, h: int, w: int) -> Tensor:
    """Data gradient of nn.Conv2d(K, M, 2, stride=2): one split-bf16 1x1 GEMM with the 4K tap rows
    W[m, k, di, dj] -> row (2 di + dj) K + k, then grr_interleave2x2 to full resolution."""
    dev = _check("conv2x2s2_bwd_data", g, weight)
    b, m = g.shape[:2]
    k = weight.shape[1]
    w4 = weight.permute(2, 3, 1, 0).reshape(4 * k, m, 1, 1).contiguous()
    t = conv1x1(g, w4)
    gx = torch.empty((b, k, h, w), dtype=torch.float32, device=dev)
    _launch("interleave2x2", 8 * gx.numel(), "grr_interleave2x2", t.data_ptr(), gx.data_ptr(), b, k, h, w,
            _stream(dev))
    return gx


def conv2x2s2_bwd_data(g: Tensor, weight: Tensor, h: int, w: int) -> Tensor:
    dev = _check("conv2x2s2_bwd_data", g, weight)
    b, m = g.shape[:2]
    k = weight.shape[1]
    gx = torch.empty((b, k, h, w), dtype=torch.float32, device=dev)
    _launch("conv2x2s2_bwd", 4 * (g.numel() + gx.numel()), "grr_conv2x2s2_bwd_data", g.data_ptr(),
            weight.data_ptr(), gx.data_ptr(), b, k, m, h, w, _stream(dev))
    return gx


def glr_stage(x: Tensor, b: Tensor, u_prev: Optional[Tensor], wL: Tensor, sL: Stencil, mu: Tensor, alpha: Tensor,
              beta: Optional[Tensor], n_graphs: int, want_u: bool = True,
              u_out: Optional[Tensor] = None) -> Tuple[Tensor, Optional[Tensor]]:
    """One v10 MixtureGLR stage (grr_glr_stage): returns (x_out, u)."""
    dev = _check("glr_stage", x, b, u_prev, wL, mu, alpha, beta, u_out)
    bb, c, h, w = x.shape
    out = torch.empty_like(x)
    if want_u and u_out is None:
        u_out = torch.empty_like(x)
    if not want_u:
        u_out = None
    nbytes = 4 * bb * h * w * (c * (2 + int(b is not x) + int(u_prev is not None) + int(u_out is not None))
                               + 4 * n_graphs)
    _launch("glr_stage", nbytes, "grr_glr_stage", x.data_ptr(), b.data_ptr(), _ptr(u_prev), wL.data_ptr(), sL,
            mu.data_ptr(), alpha.data_ptr(), _ptr(beta), out.data_ptr(), _ptr(u_out), bb, n_graphs, c // n_graphs,
            h, w, _stream(dev))
    return out, u_out


# ---- LocalNonLinearBlock reverse pieces ---------------------------------------
def lnb_norm(x: Tensor, ln_w: Tensor) -> Tuple[Tensor, Tensor]:
    dev = _check("lnb_norm", x, ln_w)
    b, c, h, w = x.shape
    n = torch.empty_like(x)
    isd = torch.empty((b, h, w), dtype=torch.float32, device=dev)
    _launch("lnb_norm", 8 * x.numel(), "grr_lnb_norm", x.data_ptr(), ln_w.data_ptr(), n.data_ptr(), isd.data_ptr(),
            b, c, h * w, _stream(dev))
    return n, isd


def lnb_norm_bwd(x: Tensor, ln_w: Tensor, isd: Tensor, gn: Tensor, gx: Tensor, gln_w: Tensor) -> None:
    dev = _check("lnb_norm_bwd", x, ln_w, isd, gn, gx, gln_w)
    b, c, h, w = x.shape
    _launch("lnb_norm_bwd", 20 * x.numel(), "grr_lnb_norm_bwd", x.data_ptr(), ln_w.data_ptr(), isd.data_ptr(),
            gn.data_ptr(), gx.data_ptr(), gln_w.data_ptr(), b, c, h * w, _stream(dev))


def lnb_norm_bwd_skip(x: Tensor, ln_w: Tensor, isd: Tensor, gn: Tensor, gout: Tensor, skip: Tensor,
                      gln_w: Tensor, gskip0: Tensor) -> Tensor:
    """The LNB reverse's tail in one pass (grr_lnb_norm_bwd_skip): returns gx = skip[0] gout + d<gn, n>/dx;
    gskip0 += <gout, x>, gln_w += sum gn x isd."""
    dev = _check("lnb_norm_bwd", x, ln_w, isd, gn, gout, skip, gln_w, gskip0)
    b, c, h, w = x.shape
    if gout.shape != x.shape or gn.shape != x.shape:
        raise ValueError("lnb_norm_bwd_skip: shapes")
    gx = torch.empty_like(x)
    _launch("lnb_norm_bwd", 24 * x.numel(), "grr_lnb_norm_bwd_skip", x.data_ptr(), ln_w.data_ptr(), isd.data_ptr(),
            gn.data_ptr(), gout.data_ptr(), skip.data_ptr(), gx.data_ptr(), gln_w.data_ptr(), gskip0.data_ptr(), b, c,
            h * w, _stream(dev))
    return gx


def dwconv3(h: Tensor, wdw: Tensor) -> Tensor:
    dev = _check("dwconv3", h, wdw)
    b, c, hh, ww = h.shape
    out = torch.empty_like(h)
    _launch("dwconv3", 8 * h.numel(), "grr_dwconv3", h.data_ptr(), wdw.data_ptr(), out.data_ptr(), b, c, hh, ww,
            _stream(dev))
    return out


def dwconv3_bwd(g: Tensor, h: Tensor, wdw: Tensor, gwdw: Tensor) -> Tensor:
    dev = _check("dwconv3_bwd", g, h, wdw, gwdw)
    b, c, hh, ww = h.shape
    gh = torch.empty_like(h)
    # compulsory bytes: g and h read once, gh written once (one fused pass for W <= 256)
    _launch("dwconv3_bwd", 12 * h.numel(), "grr_dwconv3_bwd", g.data_ptr(), h.data_ptr(), wdw.data_ptr(), gh.data_ptr(),
            gwdw.data_ptr(), b, c, hh, ww, _stream(dev))
    return gh


def lnb_gate_bwd_scaled(hp: Tensor, gq: Tensor, scale: Tensor, gdot: Tensor) -> Tensor:
    """ghp = scale * (d gate / d hp) . gq;  gdot += <gq, gate>   (grr_lnb_gate_bwd_scaled)."""
    dev = _check("lnb_gate_bwd_scaled", hp, gq, scale, gdot)
    b, c2, h, w = hp.shape
    hid = c2 // 2
    if tuple(gq.shape) != (b, hid, h, w):
        raise ValueError("lnb_gate_bwd_scaled: gq shape")
    ghp = torch.empty_like(hp)
    _launch("lnb_gate", 4 * hp.numel() * 2 + 4 * gq.numel(), "grr_lnb_gate_bwd_scaled", hp.data_ptr(), gq.data_ptr(),
            scale.data_ptr(), ghp.data_ptr(), gdot.data_ptr(), b, hid, h * w, _stream(dev))
    return ghp


def lnb_gate_dw3_ok(h: int, w: int) -> bool:
    """The depthwise / gate row kernels' widths (W > 256: column strips of 4-wide lanes)."""
    return (w <= 64) or (w <= 128 and w % 2 == 0) or (w % 4 == 0)


def set_lnb_bwd_ring(enable: bool) -> None:
    """The LDS-ring gate + depthwise reverse (True, default) or the register row kernel (grr_lnb_set_bwd_ring)."""
    _native.call("grr_lnb_set_bwd_ring", int(bool(enable)))


def lnb_gate_dw3_bwd(hp: Optional[Tensor], gq: Tensor, scale: Tensor, hh: Tensor, wdw: Tensor, gwdw: Tensor,
                     gdot: Tensor) -> Tensor:
    """Gate reverse + depthwise reverse in one row pass (grr_lnb_gate_dw3_bwd): returns gh.
    hp None: the depthwise output is recomputed from hh in-kernel."""
    dev = _check("lnb_gate_dw3_bwd", hp, gq, scale, hh, wdw, gwdw, gdot)
    b, c2, h, w = hh.shape
    if (hp is not None and hp.shape != hh.shape) or tuple(gq.shape) != (b, c2 // 2, h, w):
        raise ValueError("lnb_gate_dw3_bwd: shapes")
    gh = torch.empty_like(hh)
    nbytes = 4 * ((hp.numel() if hp is not None else 0) + gq.numel() + hh.numel() + gh.numel())
    _launch("lnb_gate_dw3_bwd", nbytes, "grr_lnb_gate_dw3_bwd", _ptr(hp), gq.data_ptr(), scale.data_ptr(),
            hh.data_ptr(), wdw.data_ptr(), gh.data_ptr(), gwdw.data_ptr(), gdot.data_ptr(), b, c2 // 2, h, w,
            _stream(dev))
    return gh


def lnb_dw3_gate(hh: Tensor, wdw: Tensor) -> Tensor:
    """gate = sigmoid(m) m v of (m, v) = dwconv3(hh), the depthwise output not stored (grr_lnb_dw3_gate)."""
    dev = _check("lnb_dw3_gate", hh, wdw)
    b, c2, h, w = hh.shape
    gate = torch.empty((b, c2 // 2, h, w), dtype=torch.float32, device=dev)
    _launch("lnb_dw3_gate", 4 * (hh.numel() + gate.numel()), "grr_lnb_dw3_gate", hh.data_ptr(), wdw.data_ptr(),
            gate.data_ptr(), b, c2 // 2, h, w, _stream(dev))
    return gate


def ffn_dw3_gate(hh: Tensor, wdw: Tensor) -> Tensor:
    """gate = gelu(d1) d2 of [d1; d2] = zero-padded dwconv3(hh) (the window FeedForward, REF7:29-48;
    grr_ffn_dw3_gate, the depthwise output not stored)."""
    dev = _check("ffn_dw3_gate", hh, wdw)
    b, c2, h, w = hh.shape
    gate = torch.empty((b, c2 // 2, h, w), dtype=torch.float32, device=dev)
    _launch("ffn_dw3_gate", 4 * (hh.numel() + gate.numel()), "grr_ffn_dw3_gate", hh.data_ptr(), wdw.data_ptr(),
            gate.data_ptr(), b, c2 // 2, h, w, _stream(dev))
    return gate


def ffn_gate_dw3_bwd(gq: Tensor, scale: Tensor, hh: Tensor, wdw: Tensor, gwdw: Tensor, gdot: Tensor) -> Tensor:
    """Reverse of ffn_dw3_gate with the skip scale (grr_ffn_gate_dw3_bwd): returns gh; gwdw += ;
    gdot[0] += <gq, gate>."""
    dev = _check("ffn_gate_dw3_bwd", gq, scale, hh, wdw, gwdw, gdot)
    b, c2, h, w = hh.shape
    if tuple(gq.shape) != (b, c2 // 2, h, w):
        raise ValueError("ffn_gate_dw3_bwd: shapes")
    gh = torch.empty_like(hh)
    _launch("ffn_gate_dw3_bwd", 4 * (gq.numel() + hh.numel() + gh.numel()), "grr_ffn_gate_dw3_bwd", gq.data_ptr(),
            scale.data_ptr(), hh.data_ptr(), wdw.data_ptr(), gh.data_ptr(), gwdw.data_ptr(), gdot.data_ptr(), b,
            c2 // 2, h, w, _stream(dev))
    return gh


def lnb_gate(hp: Tensor, ggate: Optional[Tensor] = None, want_gate: bool = True):
    """gate = sigmoid(m) m v of hp = [m; v]; with ggate also the reverse ghp.  Returns (gate, ghp)."""
    dev = _check("lnb_gate", hp, ggate)
    b, c2, h, w = hp.shape
    hid = c2 // 2
    gate = torch.empty((b, hid, h, w), dtype=torch.float32, device=dev) if want_gate else None
    ghp = torch.empty_like(hp) if ggate is not None else None
    _launch("lnb_gate", 4 * hp.numel() * 2, "grr_lnb_gate", hp.data_ptr(), _ptr(ggate), _ptr(gate), _ptr(ghp), b, hid,
            h * w, _stream(dev))
    return gate, ghp


# ---- window graphs (REF7 = lib/model_GLR_GTV_deep_v7.py, REF1 = lib/model_GLR_GTV_deep_v1.py) ----
_DELTA_CACHE = {}


def _delta_arg(edge_delta) -> Tuple[object, int]:
    """Host int32 [K,2] (dy, dx) array for the window entry points (cached per window)."""
    key = tuple((int(a), int(b)) for a, b in edge_delta)
    arr = _DELTA_CACHE.get(key)
    if arr is None:
        import ctypes
        flat = [v for e in key for v in e]
        arr = (ctypes.c_int32 * len(flat))(*flat)
        _DELTA_CACHE[key] = arr
    return arr, len(key)


def win_edge_weights(feat: Tensor, channel_offset: int, n_graphs: int, n_fts: int, multiM: Tensor, edge_delta,
                     with_degree: bool = False) -> Tuple[Tensor, Optional[Tensor]]:
    """Window-graph edge weights (grr_win_edge_weights, REF7:418-446) of the [n_graphs*n_fts] channel
    slab at ``channel_offset`` of feat [B,Ctot,H,W] -> (w [B,G,K,H,W], degree or None)."""
    dev = _check("win_edge_weights", feat, multiM)
    b, ctot, h, w = feat.shape
    if channel_offset + n_graphs * n_fts > ctot:
        raise ValueError("win_edge_weights: channel slab out of range")
    delta, k = _delta_arg(edge_delta)
    if multiM.numel() != n_graphs * n_fts:
        raise ValueError(f"win_edge_weights: multiM has {multiM.numel()} entries, expected {n_graphs * n_fts}")
    wt = torch.empty((b, n_graphs, k, h, w), dtype=torch.float32, device=dev)
    deg = torch.empty((b, n_graphs, h, w), dtype=torch.float32, device=dev) if with_degree else None
    base = feat.data_ptr() + channel_offset * h * w * feat.element_size()
    nbytes = 4 * b * h * w * (n_graphs * n_fts + k * n_graphs + (n_graphs if with_degree else 0))
    _launch("win_edge_weights", nbytes, "grr_win_edge_weights", base, ctot * h * w, multiM.data_ptr(), delta, k,
            wt.data_ptr(), _ptr(deg), b, n_graphs, n_fts, h, w, _stream(dev))
    return wt, deg


def win_taps(p01: Tensor, p02a: Tensor, p02b: Tensor, p03: Tensor) -> Tensor:
    """(centre, up, left, right, down) of the stats stencil p01 k01 + p02a k02a + p02b k02b + p03 k03
    (REF7:300-358, scalar parameters): centre p01 - p02a - p02b + 4 p03, right p02a - p03,
    down p02b - p03, up = left = -p03."""
    p01, p02a, p02b, p03 = (t.reshape(()) for t in (p01, p02a, p02b, p03))
    return torch.stack([p01 - p02a - p02b + 4.0 * p03, -p03, -p03, p02a - p03, p02b - p03]).float().contiguous()


IDENTITY_TAPS = (1.0, 0.0, 0.0, 0.0, 0.0)


def _check_win_scalars(n_graphs: int, **ts) -> None:
    """Host-side size checks of the per-graph scalars / stencil taps the window kernels index."""
    for name, t in ts.items():
        if t is None:
            continue
        need = 5 if name.startswith("taps") else n_graphs
        if t.numel() < need:
            raise ValueError(f"window graph: {name} has {t.numel()} entries, needs {need}")


def win_solver(mode: int, x: Tensor, y: Tensor, wG: Tensor, tapsG: Tensor, ro: Tensor, edge_delta, n_graphs: int,
               n_sig: int, *, wL: Optional[Tensor] = None, tapsL: Optional[Tensor] = None, mu: Optional[Tensor] = None,
               log_gamma: Optional[Tensor] = None, alpha: Optional[Tensor] = None, beta: Optional[Tensor] = None,
               u_prev: Optional[Tensor] = None, want_u: bool = True,
               pair: bool = False) -> Tuple[Tensor, Optional[Tensor]]:
    """One fused pass of the window-graph MixtureGTV solver (grr_win_solver, REF7:892-1004).
    pair: wG holds win_pair_weights(w_G) (modes 0 and 1: the same linear GTV term from K weights
    per position instead of K plus K gathered reverse-edge weights).

    mode 0: CG step, x [B,G,Fs,H,W], y = rhs [B,G,Fs,H,W] -> (x_next, u);
    mode 1/2: (prox) right-hand side, y [B,Fs,H,W] shared by the graphs, x per graph or
    [B,Fs,H,W] (shared) -> (rhs [B,G,Fs,H,W], None)."""
    dev = _check("win_solver", x, y, wG, tapsG, ro, wL, tapsL, mu, log_gamma, alpha, beta, u_prev)
    delta, k = _delta_arg(edge_delta)
    b, h, w = x.shape[0], x.shape[-2], x.shape[-1]
    x_rep = int(x.dim() == 4)
    if x_rep and x.shape[1] != n_sig or not x_rep and tuple(x.shape[1:3]) != (n_graphs, n_sig):
        raise ValueError(f"win_solver: x has shape {tuple(x.shape)}")
    if tuple(wG.shape) != (b, n_graphs, k, h, w):
        raise ValueError(f"win_solver: wG has shape {tuple(wG.shape)}, expected {(b, n_graphs, k, h, w)}")
    _check_win_scalars(n_graphs, tapsG=tapsG, tapsL=tapsL, ro=ro, mu=mu, log_gamma=log_gamma, alpha=alpha, beta=beta)
    out = torch.empty((b, n_graphs, n_sig, h, w), dtype=torch.float32, device=dev)
    if u_prev is not None and tuple(u_prev.shape) != tuple(out.shape):
        raise ValueError(f"win_solver: u_prev has shape {tuple(u_prev.shape)}, expected {tuple(out.shape)}")
    u_out = torch.empty_like(out) if (mode == 0 and want_u) else None
    planes = b * n_graphs * n_sig
    if mode == 0:
        if tuple(wL.shape) != tuple(wG.shape) or tuple(y.shape) != tuple(out.shape):
            raise ValueError("win_solver: wL / rhs shapes do not match")
        nbytes = 4 * h * w * (planes * (2 + int(u_prev is not None) + 1 + int(u_out is not None))
                              + 2 * k * b * n_graphs)
    else:
        if tuple(y.shape) != (b, n_sig, h, w):
            raise ValueError(f"win_solver: y has shape {tuple(y.shape)}, expected {(b, n_sig, h, w)}")
        nbytes = 4 * h * w * (planes * (1 + int(not x_rep)) + b * n_sig * (1 + x_rep) + k * b * n_graphs)
    if pair and mode == 2:
        raise ValueError("win_solver: the prox rhs (mode 2) needs the raw GTV weights")
    _launch("win_solver", nbytes, "grr_win_solver", mode + (4 if pair else 0), x.data_ptr(), x_rep, y.data_ptr(),
            _ptr(u_prev), _ptr(wL),
            wG.data_ptr(), _ptr(tapsL), tapsG.data_ptr(), _ptr(mu), ro.data_ptr(), _ptr(log_gamma), _ptr(alpha),
            _ptr(beta), delta, k, out.data_ptr(), _ptr(u_out), b, n_graphs, n_sig, h, w, _stream(dev))
    return out, u_out


def win_pair_weights(w: Tensor, edge_delta) -> Tensor:
    """Pair weights c_e(q) = w_e(q)^2 + [q + d_e inside] w_e'(q + d_e)^2 of the linear window GTV
    term (grr_win_pair_weights), w [B,G,K,H,W] -> c of the same shape."""
    dev = _check("win_pair_weights", w)
    delta, k = _delta_arg(edge_delta)
    b, g, kk, h, ww = w.shape
    if kk != k:
        raise ValueError(f"win_pair_weights: w has {kk} edge planes, the window {k}")
    c = torch.empty_like(w)
    _launch("win_pair_weights", 4 * w.numel() * 3, "grr_win_pair_weights", w.data_ptr(), delta, k, c.data_ptr(), b, g,
            h, ww, _stream(dev))
    return c


def win_mix(x: Tensor, score: Tensor, dc: Optional[Tensor] = None) -> Tensor:
    """sum_g x[b,g,c] score[b,g] (+ dc[b,c]) (grr_win_mix, REF7:1006-1009)."""
    dev = _check("win_mix", x, score, dc)
    b, g, c, h, w = x.shape
    if tuple(score.shape) != (b, g, h, w) or (dc is not None and tuple(dc.shape) != (b, c, h, w)):
        raise ValueError("win_mix: score / dc shapes do not match")
    out = torch.empty((b, c, h, w), dtype=torch.float32, device=dev)
    nbytes = 4 * h * w * (x[0].numel() // (h * w) * b + b * g + b * c * (1 + int(dc is not None)))
    _launch("win_mix", nbytes, "grr_win_mix", x.data_ptr(), score.data_ptr(), _ptr(dc), out.data_ptr(), b, g, c, h, w,
            _stream(dev))
    return out


def win_apply(x: Tensor, edge_delta, n_graphs: int, n_sig: int, *, wL: Optional[Tensor] = None,
              tapsL: Optional[Tensor] = None, mu: Optional[Tensor] = None, wG: Optional[Tensor] = None,
              tapsG: Optional[Tensor] = None, ro: Optional[Tensor] = None, pair: bool = False) -> Tensor:
    """mu S_L^T (I - W_L) S_L x [wL] + ro S_G^T C^T C S_G x [wG] (grr_win_solver mode 3; the
    GLRFast / GTVFast.forward of REF7:503-511, :776-782).  x [B,G,Fs,H,W].
    pair: wG holds win_pair_weights(w_G) (mode 7: the same GTV term from K weights per position)."""
    dev = _check("win_apply", x, wL, tapsL, mu, wG, tapsG, ro)
    delta, k = _delta_arg(edge_delta)
    b, g, c, h, w = x.shape
    for t in (wL, wG):
        if t is not None and tuple(t.shape) != (b, n_graphs, k, h, w):
            raise ValueError(f"win_apply: edge weights of shape {tuple(t.shape)}, expected {(b, n_graphs, k, h, w)}")
    if g != n_graphs or c > 3:
        raise ValueError(f"win_apply: x has shape {tuple(x.shape)} (graphs {n_graphs}, at most 3 signal channels)")
    _check_win_scalars(n_graphs, tapsG=tapsG, tapsL=tapsL, ro=ro, mu=mu)
    out = torch.empty_like(x)
    nbytes = 4 * h * w * (2 * x.numel() // (h * w) + k * b * n_graphs * (int(wL is not None) + int(wG is not None)))
    if pair and wG is None:
        raise ValueError("win_apply: pair needs the pair weights in wG")
    _launch("win_solver", nbytes, "grr_win_solver", 7 if pair else 3, x.data_ptr(), 0, None, None, _ptr(wL), _ptr(wG),
            _ptr(tapsL), _ptr(tapsG), _ptr(mu), _ptr(ro), None, None, None, delta, k, out.data_ptr(), None, b, n_graphs,
            n_sig, h, w, _stream(dev))
    return out


# ---- window-graph reverse (window_bwd.hip; training through MixtureGTV of REF7 / REF1) ----
WST_P, WST_T_ADJ, WST_P_ADJ = 0, 1, 2      # S x (reflect) / S^T* g (zero-frame correlation) / S* g
WTAP_P, WTAP_T = 0, 1


def _win5(x: Tensor, n_graphs: int):
    """(B, G, Fs, H, W) of a [B,G,Fs,H,W] window signal."""
    if x.dim() != 5 or x.shape[1] != n_graphs:
        raise ValueError(f"window reverse: expected [B,{n_graphs},Fs,H,W], got {tuple(x.shape)}")
    b, g, fs, h, w = x.shape
    if h < 2 or w < 2:
        raise ValueError("window reverse: the reflect frame needs H, W >= 2")
    return b, g, fs, h, w


def win_bwd_stencil(x: Tensor, taps: Tensor, mode: int, n_graphs: int, scale: Optional[Tensor] = None,
                    out: Optional[Tensor] = None) -> Tensor:
    """out = [out +] scale[g] * mode(x)  (out given -> accumulate)."""
    dev = _check("win_bwd_stencil", x, taps, scale, out)
    dims = _win5(x, n_graphs)
    acc = out is not None
    if out is None:
        out = torch.empty_like(x)
    elif out.shape != x.shape:
        raise ValueError("win_bwd_stencil: out shape")
    _check_win_scalars(n_graphs, taps=taps, scale=scale)
    _launch("win_bwd_stencil", 4 * x.numel() * (2 + int(acc)), "grr_win_bwd_stencil", x.data_ptr(), taps.data_ptr(),
            mode, _ptr(scale), int(acc), out.data_ptr(), *dims, _stream(dev))
    return out


def win_bwd_tapgrad(u: Tensor, z: Tensor, mode: int, n_graphs: int, scale: Optional[Tensor], gtaps: Tensor) -> None:
    dev = _check("win_bwd_tapgrad", u, z, scale, gtaps)
    dims = _win5(u, n_graphs)
    if z.shape != u.shape or gtaps.numel() < 5:
        raise ValueError("win_bwd_tapgrad: shapes")
    _launch("win_bwd_tapgrad", 8 * u.numel(), "grr_win_bwd_tapgrad", u.data_ptr(), z.data_ptr(), mode, _ptr(scale),
            gtaps.data_ptr(), *dims, _stream(dev))


def _edge_shape_ok(w: Tensor, dims, k: int) -> None:
    b, g, _, h, ww = dims
    if tuple(w.shape) != (b, g, k, h, ww):
        raise ValueError(f"window reverse: edge weights of shape {tuple(w.shape)}, expected {(b, g, k, h, ww)}")


# The window term reverses' second pass recomputes the E / PW planes where they are gathered
# (grr_win_bwd_gather_fused) instead of pass 1 writing 2 Fs K floats per pixel for it to read back;
# False: the planes (the A/B and parity reference)
WIN_FUSED_GATHER = True


def win_bwd_glr(s: Tensor, bt: Tensor, w: Tensor, edge_delta, sc: Tensor, coef: float, gw: Tensor,
                gdot: Optional[Tensor], n_graphs: int) -> Tuple[Tensor, Tensor]:
    """GLR term reverse, both passes: returns (l = (I - W) s, gs = (I - W)^T (sc * bt))."""
    dev = _check("win_bwd_glr", s, bt, w, sc, gw, gdot)
    dims = _win5(s, n_graphs)
    delta, k = _delta_arg(edge_delta)
    _edge_shape_ok(w, dims, k)
    if bt.shape != s.shape or gw.shape != w.shape:
        raise ValueError("win_bwd_glr: shapes")
    _check_win_scalars(n_graphs, sc=sc, gdot=gdot)
    b, g, fs, h, ww = dims
    l_out, gs = torch.empty_like(s), torch.empty_like(s)
    if WIN_FUSED_GATHER:   # no E planes: the gather recomputes them (grr_win_bwd_gather_fused)
        _launch("win_bwd_glr", 4 * (4 * s.numel() + 3 * w.numel()), "grr_win_bwd_glr",
                s.data_ptr(), bt.data_ptr(), w.data_ptr(), delta, k, sc.data_ptr(), float(coef), l_out.data_ptr(),
                None, gs.data_ptr(), gw.data_ptr(), _ptr(gdot), *dims, _stream(dev))
        _launch("win_bwd_gather", 4 * (4 * s.numel() + w.numel()), "grr_win_bwd_gather_fused", s.data_ptr(),
                bt.data_ptr(), w.data_ptr(), delta, k, 0, 0, None, sc.data_ptr(), gs.data_ptr(), None, *dims,
                _stream(dev))
        return l_out, gs
    E = torch.empty((b, g, fs, k, h, ww), dtype=torch.float32, device=dev)
    _launch("win_bwd_glr", 4 * (3 * s.numel() + 3 * w.numel() + (k + 2) * s.numel()), "grr_win_bwd_glr",
            s.data_ptr(), bt.data_ptr(), w.data_ptr(), delta, k, sc.data_ptr(), float(coef), l_out.data_ptr(),
            E.data_ptr(), gs.data_ptr(), gw.data_ptr(), _ptr(gdot), *dims, _stream(dev))
    _launch("win_bwd_gather", 4 * (k + 2) * s.numel(), "grr_win_bwd_gather", E.data_ptr(), None, delta, k,
            gs.data_ptr(), None, *dims, _stream(dev))
    return l_out, gs


def win_bwd_gtv(s: Tensor, bt: Tensor, w: Tensor, edge_delta, prox: bool, log_gamma: Optional[Tensor], sc: Tensor,
                coef: float, gw: Tensor, gdot: Optional[Tensor], ggamma: Optional[Tensor],
                n_graphs: int) -> Tuple[Tensor, Tensor]:
    """GTV term (C^T C or C^T phi(C .)) reverse, both passes: returns (o, gs)."""
    dev = _check("win_bwd_gtv", s, bt, w, log_gamma, sc, gw, gdot, ggamma)
    dims = _win5(s, n_graphs)
    delta, k = _delta_arg(edge_delta)
    _edge_shape_ok(w, dims, k)
    if bt.shape != s.shape or gw.shape != w.shape or (prox and log_gamma is None):
        raise ValueError("win_bwd_gtv: shapes / log_gamma")
    _check_win_scalars(n_graphs, sc=sc, gdot=gdot, log_gamma=log_gamma, ggamma=ggamma)
    b, g, fs, h, ww = dims
    o, gs = torch.empty_like(s), torch.empty_like(s)
    if WIN_FUSED_GATHER:   # no E / PW planes: the gather recomputes them (grr_win_bwd_gather_fused)
        _launch("win_bwd_gtv", 4 * (3 * s.numel() + 3 * w.numel()), "grr_win_bwd_gtv",
                s.data_ptr(), bt.data_ptr(), w.data_ptr(), delta, k, int(prox), _ptr(log_gamma), sc.data_ptr(),
                float(coef), None, None, gs.data_ptr(), gw.data_ptr(), _ptr(gdot), _ptr(ggamma), *dims,
                _stream(dev))
        _launch("win_bwd_gather", 4 * (5 * s.numel() + w.numel()), "grr_win_bwd_gather_fused", s.data_ptr(),
                bt.data_ptr(), w.data_ptr(), delta, k, 1, int(prox), _ptr(log_gamma), sc.data_ptr(), gs.data_ptr(),
                o.data_ptr(), *dims, _stream(dev))
        return o, gs
    E = torch.empty((b, g, fs, k, h, ww), dtype=torch.float32, device=dev)
    PW = torch.empty_like(E)
    _launch("win_bwd_gtv", 4 * (3 * s.numel() + 3 * w.numel() + (2 * k + 1) * s.numel()), "grr_win_bwd_gtv",
            s.data_ptr(), bt.data_ptr(), w.data_ptr(), delta, k, int(prox), _ptr(log_gamma), sc.data_ptr(),
            float(coef), PW.data_ptr(), E.data_ptr(), gs.data_ptr(), gw.data_ptr(), _ptr(gdot), _ptr(ggamma), *dims,
            _stream(dev))
    _launch("win_bwd_gather", 4 * (2 * k + 3) * s.numel(), "grr_win_bwd_gather", E.data_ptr(), PW.data_ptr(), delta,
            k, gs.data_ptr(), o.data_ptr(), *dims, _stream(dev))
    return o, gs


def win_bwd_edge_weights(feat: Tensor, channel_offset: int, n_graphs: int, n_fts: int, multiM: Tensor, w: Tensor,
                         gw: Tensor, edge_delta, gfeat: Tensor, gmultiM: Tensor) -> None:
    """Accumulates into the [G*F] slab at channel_offset of gfeat (same shape as feat) and gmultiM;
    gw is consumed (overwritten by the softmax reverse)."""
    dev = _check("win_bwd_edge_weights", feat, multiM, w, gw, gfeat, gmultiM)
    b, ctot, h, ww = feat.shape
    delta, k = _delta_arg(edge_delta)
    if gfeat.shape != feat.shape or channel_offset + n_graphs * n_fts > ctot:
        raise ValueError("win_bwd_edge_weights: bad slab")
    if tuple(w.shape) != (b, n_graphs, k, h, ww) or gw.shape != w.shape or multiM.numel() != n_graphs * n_fts \
            or gmultiM.numel() != n_graphs * n_fts:
        raise ValueError("win_bwd_edge_weights: shapes")
    off = channel_offset * h * ww * 4
    _launch("win_bwd_edge_weights", 4 * b * h * ww * n_graphs * (3 * n_fts + 3 * k), "grr_win_bwd_edge_weights",
            feat.data_ptr() + off, ctot * h * ww, multiM.data_ptr(), w.data_ptr(), gw.data_ptr(), delta, k,
            gfeat.data_ptr() + off, ctot * h * ww, gmultiM.data_ptr(), b, n_graphs, n_fts, h, ww, _stream(dev))


def win_bwd_mix(gout: Tensor, x: Tensor, score: Tensor) -> Tuple[Tensor, Tensor]:
    """Reverse of win_mix: (gx [B,G,Fs,H,W], gscore [B,G,H,W]); gdc = gout."""
    dev = _check("win_bwd_mix", gout, x, score)
    b, g, c, h, w = x.shape
    if tuple(score.shape) != (b, g, h, w) or tuple(gout.shape) != (b, c, h, w):
        raise ValueError("win_bwd_mix: shapes")
    gx, gscore = torch.empty_like(x), torch.empty_like(score)
    _launch("win_bwd_mix", 4 * (2 * x.numel() + 2 * score.numel() + gout.numel()), "grr_win_bwd_mix",
            gout.data_ptr(), x.data_ptr(), score.data_ptr(), gx.data_ptr(), gscore.data_ptr(), b, g, c, h, w,
            _stream(dev))
    return gx, gscore


# ---------------------------------------------------------------------------
# whole-image restoration I/O (image_ops.hip; restore.py is the caller)
IMAGE_DTYPES = (torch.uint8, torch.float32)


def image_io_ok(c: int, h: int, w: int) -> bool:
    """grr_image_io_supported in plain Python (tests/test_restore_abi.py checks the two agree): an H x W x C
    image, or a window batch as (C, n th, tw), the image entry points take."""
    return 1 <= c <= 4 and h >= 1 and w >= 1 and h * w * c < (1 << 31)


def _check_image(name: str, img: Tensor) -> Tuple[int, int, int]:
    """(H, W, C) of an HWC uint8 / float32 device image; ValueError before any launch otherwise."""
    if not isinstance(img, Tensor) or img.dim() != 3:
        raise ValueError(f"{name}: expected an H x W x C tensor, got {tuple(getattr(img, 'shape', ()))}")
    if img.dtype not in IMAGE_DTYPES:
        raise ValueError(f"{name}: image dtype must be uint8 or float32, got {img.dtype}")
    h, w, c = img.shape
    if not image_io_ok(c, h, w):
        raise ValueError(f"{name}: needs an H x W x C image with C <= 4 and below 2^31 elements, got {tuple(img.shape)}")
    if not img.is_cuda:
        raise RuntimeError(f"{name}: tensors must be on the GPU (got {img.device}); the HIP engine has no CPU path")
    return h, w, c


_TABLE_ROWS = {6: "(wr, wc, r0, r1, c0, c1)", 7: "(img, wr, wc, r0, r1, c0, c1)"}


def _check_table(name: str, table: Tensor, dev, cols: int, owner: str) -> int:
    if not isinstance(table, Tensor) or table.dtype != torch.int32 or table.dim() != 2 or table.shape[1] != cols \
            or table.shape[0] < 1:
        raise ValueError(f"{name}: the window table is int32 [n, {cols}] {_TABLE_ROWS[cols]}")
    if table.device != dev or not table.is_contiguous():
        raise ValueError(f"{name}: the window table must be contiguous and on the {owner}'s device")
    return table.shape[0]


def _check_batch(name: str, n: int, c: int, th: int, tw: int) -> None:
    """The window-batch bound of the four gather / scatter entry points: 1 <= n th tw C < 2^31."""
    if th < 1 or tw < 1 or not image_io_ok(c, n * th, tw):
        raise ValueError(f"{name}: window batch {n} x {c} x {th} x {tw} must have 1..2^31-1 elements")


def _gather(kind: str, buf: Tensor, src_args: tuple, c: int, table: Tensor, th: int, tw: int) -> Tensor:
    """tile_gather / tiles_gather after their own checks: ``buf`` is the image or the arena, ``src_args`` what
    grr_<kind> takes in front of (table, n, th, tw, out, stream)."""
    n = table.shape[0]
    _check_batch(kind, n, c, th, tw)
    out = torch.empty((n, c, th, tw), dtype=torch.float32, device=buf.device)
    _launch(kind, out.numel() * (buf.element_size() + 4), "grr_" + kind, *src_args, table.data_ptr(), n, th, tw,
            out.data_ptr(), _stream(buf.device))
    return out


def _scatter(kind: str, y: Tensor, table: Tensor, buf: Tensor, src_args: tuple, core_px: Optional[int]) -> None:
    """tile_scatter / tiles_scatter after their own checks: ``src_args`` is what grr_<kind> takes between
    (y, table, n, th, tw) and the stream."""
    n, c, th, tw = y.shape
    _check_batch(kind, n, c, th, tw)
    px = n * th * tw if core_px is None else core_px
    _launch(kind, px * c * (4 + buf.element_size()), "grr_" + kind, y.data_ptr(), table.data_ptr(), n, th, tw,
            *src_args, _stream(buf.device))


def tile_gather(img: Tensor, table: Tensor, th: int, tw: int) -> Tensor:
    """Windows [n, C, th, tw] (float32, the model's input) of the HWC uint8 / float32 image reflect-padded at
    the bottom and right; table: int32 [n, 6] device rows (wr, wc, r0, r1, c0, c1) of tiling.Window.  uint8
    becomes float(v) / 255; float32 is copied bit for bit.  A non-contiguous image is copied first."""
    h, w, c = _check_image("tile_gather", img)
    _check_table("tile_gather", table, img.device, 6, "image")
    img = img.contiguous()
    return _gather("tile_gather", img, (img.data_ptr(), int(img.dtype == torch.float32), h, w, c), c, table, th, tw)


def tile_scatter(y: Tensor, table: Tensor, img: Tensor, core_px: Optional[int] = None) -> None:
    """Write each window's core box of y [n, C, th, tw], cut to the image, into the contiguous HWC image
    (uint8: img_as_ubyte(clip(y, 0, 1)), NaN -> 0; float32: copy).  core_px: pixels written, for the timer's
    byte count (default: all n th tw)."""
    h, w, c = _check_image("tile_scatter", img)
    if not img.is_contiguous():
        raise ValueError("tile_scatter: the output image must be contiguous")
    n = _check_table("tile_scatter", table, img.device, 6, "image")
    _check("tile_scatter", y)
    if y.dim() != 4 or y.shape[0] != n or y.shape[1] != c or y.device != img.device:
        raise ValueError(f"tile_scatter: y {tuple(y.shape)} does not match {n} windows of {c} channels")
    _scatter("tile_scatter", y, table, img, (img.data_ptr(), int(img.dtype == torch.float32), h, w, c), core_px)


def u8_sse(a: Tensor, b: Tensor) -> int:
    """sum (a - b)^2 over two uint8 device tensors of one shape, exact (a Python int; synchronises)."""
    for t in (a, b):
        if not isinstance(t, Tensor) or t.dtype != torch.uint8:
            raise ValueError(f"u8_sse: expected uint8 tensors, got {getattr(t, 'dtype', type(t))}")
    if a.shape != b.shape or a.numel() < 1 or not image_io_ok(1, 1, a.numel()):
        raise ValueError(f"u8_sse: shapes {tuple(a.shape)} / {tuple(b.shape)} must match, 1..2^31-1 elements")
    if not (a.is_cuda and b.is_cuda and a.device == b.device):
        raise RuntimeError("u8_sse: tensors must be on one GPU; the HIP engine has no CPU path")
    a, b = a.contiguous(), b.contiguous()
    out = torch.empty(1, dtype=torch.int64, device=a.device)
    _launch("u8_sse", 2 * a.numel(), "grr_u8_sse", a.data_ptr(), b.data_ptr(), a.numel(), out.data_ptr(),
            _stream(a.device))
    return int(out.item())


# ---------------------------------------------------------------------------
# ... for a list of images in one arena (restore.restore_images).  ``pack`` is restore.ImagePack or anything
# with its fields: ``arena`` (1-D uint8 / float32 device tensor, the HWC images back to back), ``table``
# (device int64 [n_img, 3], rows (element offset, H, W)), ``host_table`` (the same rows as Python ints) and
# ``c`` (channels, shared).  The kernels cannot trust device tables and clamp; the host copy is checked here.
MAX_SSE_SEGMENTS = 65535      # grr_u8_sse_segments: one grid row per segment


def image_arena_ok(c: int, n_img: int, arena_elems: int) -> bool:
    """grr_image_arena_supported in plain Python (tests/test_restore_images_abi.py checks the two agree):
    1 <= C <= 4, 1 <= n_img <= arena_elems < 2^62.  The arena may exceed 2^31 elements; each image may not
    (image_io_ok, checked on the host table)."""
    return 1 <= c <= 4 and 1 <= n_img <= arena_elems < (1 << 62)


def _check_pack(name: str, pack, placed: bool = True) -> Tuple[int, int]:
    """(n_img, C) of an image pack whose host table describes its arena; ValueError before any launch
    otherwise, RuntimeError for CPU tensors (placed=False leaves where the tensors are to _check_placed)."""
    arena, table, host, c = (getattr(pack, f, None) for f in ("arena", "table", "host_table", "c"))
    if not isinstance(arena, Tensor) or arena.dim() != 1 or arena.dtype not in IMAGE_DTYPES:
        raise ValueError(f"{name}: the arena is a 1-D uint8 or float32 tensor, got "
                         f"{tuple(getattr(arena, 'shape', ()))} {getattr(arena, 'dtype', type(arena).__name__)}")
    if not isinstance(c, int) or host is None or not image_arena_ok(c, len(host), arena.numel()):
        raise ValueError(f"{name}: needs C <= 4 and 1 <= images <= arena elements (got C {c}, "
                         f"{0 if host is None else len(host)} images, {arena.numel()} elements)")
    n_img = len(host)
    if not isinstance(table, Tensor) or table.dtype != torch.int64 or tuple(table.shape) != (n_img, 3):
        raise ValueError(f"{name}: the image table is int64 [{n_img}, 3] (element offset, H, W)")
    end = 0
    for i, row in enumerate(host):
        off, h, w = (int(v) for v in row)
        if not image_io_ok(c, h, w):
            raise ValueError(f"{name}: image {i} needs H W C < 2^31 (got {h} x {w} x {c})")
        if off < end:
            raise ValueError(f"{name}: image {i} starts at element {off}, before image {i - 1} ends ({end}): offsets "
                             "must be non-negative and increasing")
        end = off + h * w * c
        if end > arena.numel():
            raise ValueError(f"{name}: image {i} ends at element {end} of an arena of {arena.numel()}")
    if placed:
        _check_placed(name, pack)
    return n_img, c


def _check_placed(name: str, pack) -> None:
    arena, table = pack.arena, pack.table
    if not arena.is_cuda:
        raise RuntimeError(f"{name}: tensors must be on the GPU (got {arena.device}); the HIP engine has no CPU path")
    if table.device != arena.device or not table.is_contiguous() or not arena.is_contiguous():
        raise ValueError(f"{name}: the arena and the image table must be contiguous and on one device")


def _arena_args(pack, n_img: int, c: int) -> tuple:
    arena = pack.arena
    return (arena.data_ptr(), arena.numel(), int(arena.dtype == torch.float32), c, pack.table.data_ptr(), n_img)


def tiles_gather(pack, table: Tensor, th: int, tw: int) -> Tensor:
    """Windows [n, C, th, tw] (float32) of the images of ``pack``: row i of the int32 [n, 7] device table
    (img, wr, wc, r0, r1, c0, c1) is read from image img with that image's own H and W in the reflect rule.
    Element conversion as tile_gather."""
    n_img, c = _check_pack("tiles_gather", pack)
    _check_table("tiles_gather", table, pack.arena.device, 7, "arena")
    return _gather("tiles_gather", pack.arena, _arena_args(pack, n_img, c), c, table, th, tw)


def tiles_scatter(y: Tensor, table: Tensor, pack_out, core_px: Optional[int] = None) -> None:
    """Write each window's core box of y [n, C, th, tw], cut to its own image, into that image's span of
    ``pack_out.arena`` (quantisation as tile_scatter).  core_px: pixels written, for the timer's byte count."""
    n_img, c = _check_pack("tiles_scatter", pack_out)
    arena = pack_out.arena
    n = _check_table("tiles_scatter", table, arena.device, 7, "arena")
    if not isinstance(y, Tensor) or y.dim() != 4 or y.shape[0] != n or y.shape[1] != c:
        raise ValueError(f"tiles_scatter: y {tuple(getattr(y, 'shape', ()))} does not match {n} windows of {c} channels")
    _check("tiles_scatter", y)
    if y.device != arena.device:
        raise ValueError("tiles_scatter: y must be on the arena's device")
    _scatter("tiles_scatter", y, table, arena, _arena_args(pack_out, n_img, c), core_px)


# ---------------------------------------------------------------------------
# ... under the 8 flips and quarter turns of a window (restore_image(ensemble=...)).  Mode m = 2k + f:
# np.rot90(a, k), then np.flipud if f -- the numbering of the reference's data_augmentation.
def dihedral_index(m: int, th: int, tw: int, i: int, j: int) -> Tuple[int, int]:
    """Where pixel (i, j) of a th x tw window lands in T_m, in plain Python: k = m // 2 quarter turns
    counter-clockwise, (i, j, th, tw) <- (tw - 1 - j, i, tw, th) each, then i <- th - 1 - i if m is odd.  T_m is
    th x tw for even k and tw x th for odd k."""
    if not 0 <= m <= 7:
        raise ValueError(f"dihedral_index: mode {m} is outside 0..7")
    for _ in range(m // 2):
        i, j, th, tw = tw - 1 - j, i, tw, th
    return (th - 1 - i if m % 2 else i), j


def _check_modes(name: str, modes) -> Tuple[int, ...]:
    try:
        ms = tuple(int(m) for m in modes)
    except TypeError:
        ms = ()
    if not 1 <= len(ms) <= 8 or any(not 0 <= m <= 7 for m in ms) or any(b <= a for a, b in zip(ms, ms[1:])):
        raise ValueError(f"{name}: modes are 1..8 strictly ascending ints of 0..7, got {modes!r}")
    return ms


def _mode_array(ms: Tuple[int, ...]):
    return (ctypes.c_int32 * len(ms))(*ms)


def _check_gather_modes(name: str, modes) -> Tuple[int, ...]:
    ms = _check_modes(name, modes)
    if len({m // 2 % 2 for m in ms}) != 1:
        raise ValueError(f"{name}: the modes of one call share an orientation (0, 1, 4, 5 or 2, 3, 6, 7), got {ms}")
    return ms


def _gather_d8(kind: str, buf: Tensor, src_args: tuple, c: int, table: Tensor, ms: Tuple[int, ...], bh: int,
               bw: int) -> Tensor:
    """tile_gather_d8 / tiles_gather_d8 after their own checks (as _gather); ms: the checked modes."""
    n = table.shape[0]
    _check_batch(kind, n * len(ms), c, bh, bw)
    out = torch.empty((n * len(ms), c, bh, bw), dtype=torch.float32, device=buf.device)
    _launch(kind, n * c * bh * bw * (buf.element_size() + 4 * len(ms)), "grr_" + kind, *src_args, table.data_ptr(), n,
            _mode_array(ms), len(ms), bh, bw, out.data_ptr(), _stream(buf.device))
    return out


def _scatter_mean(kind: str, y0: Optional[Tensor], y1: Optional[Tensor], table: Tensor, ms: Tuple[int, ...], th: int,
                  tw: int, c: int, buf: Tensor, src_args: tuple, core_px: Optional[int]) -> None:
    """tile_scatter_mean / tiles_scatter_mean after their own checks (as _scatter): y0 [n M0, C, th, tw] holds
    the even-k members, y1 [n M1, C, tw, th] the odd-k ones; ms: the checked modes."""
    n = table.shape[0]
    m1 = sum(m // 2 % 2 for m in ms)
    counts = (len(ms) - m1, m1)
    for y, cnt, shape in ((y0, counts[0], (th, tw)), (y1, counts[1], (tw, th))):
        if cnt == 0:
            if y is not None:
                raise ValueError(f"{kind}: a batch was given for an orientation that has no mode in {ms}")
            continue
        if not isinstance(y, Tensor) or y.dim() != 4 or tuple(y.shape) != (n * cnt, c) + shape:
            raise ValueError(f"{kind}: expected a batch {(n * cnt, c) + shape} for {n} windows and modes {ms}, got "
                             f"{tuple(getattr(y, 'shape', ()))}")
        _check(kind, y)
        if y.device != buf.device:
            raise ValueError(f"{kind}: the batches must be on the output's device")
    _check_batch(kind, n * max(counts), c, th, tw)
    px = n * th * tw if core_px is None else core_px
    _launch(kind, px * c * (4 * len(ms) + buf.element_size()), "grr_" + kind, y0.data_ptr() if counts[0] else None,
            y1.data_ptr() if counts[1] else None, table.data_ptr(), n, _mode_array(ms), len(ms), counts[0], counts[1],
            th, tw, *src_args, _stream(buf.device))


def tile_gather_d8(img: Tensor, table: Tensor, modes, bh: int, bw: int) -> Tensor:
    """tile_gather under the modes of one orientation (all of 0, 1, 4, 5 or all of 2, 3, 6, 7, ascending): out
    [n M, C, bh, bw], row w M + j = T_modes[j] of window w, which is bh x bw in the picture for even k and
    bw x bh for odd k.  Element conversion as tile_gather."""
    ms = _check_gather_modes("tile_gather_d8", modes)
    h, w, c = _check_image("tile_gather_d8", img)
    _check_table("tile_gather_d8", table, img.device, 6, "image")
    img = img.contiguous()
    return _gather_d8("tile_gather_d8", img, (img.data_ptr(), int(img.dtype == torch.float32), h, w, c), c, table,
                      ms, bh, bw)


def tile_scatter_mean(y0: Optional[Tensor], y1: Optional[Tensor], table: Tensor, modes, th: int, tw: int, img: Tensor,
                      core_px: Optional[int] = None) -> None:
    """The float32 pairwise-tree mean, in the listed (ascending) order, of the members T_m^-1(y) of each th x tw
    window -- y0 [n M0, C, th, tw] the even-k members, y1 [n M1, C, tw, th] the odd-k ones, window-major as
    tile_gather_d8 lays them out, None where an orientation has no mode -- then tile_scatter's steps into the
    contiguous HWC image."""
    ms = _check_modes("tile_scatter_mean", modes)
    h, w, c = _check_image("tile_scatter_mean", img)
    if not img.is_contiguous():
        raise ValueError("tile_scatter_mean: the output image must be contiguous")
    _check_table("tile_scatter_mean", table, img.device, 6, "image")
    _scatter_mean("tile_scatter_mean", y0, y1, table, ms, th, tw, c, img,
                  (img.data_ptr(), int(img.dtype == torch.float32), h, w, c), core_px)


def tiles_gather_d8(pack, table: Tensor, modes, bh: int, bw: int) -> Tensor:
    """tile_gather_d8 for the images of ``pack`` (table rows [n, 7], as tiles_gather)."""
    ms = _check_gather_modes("tiles_gather_d8", modes)
    n_img, c = _check_pack("tiles_gather_d8", pack)
    _check_table("tiles_gather_d8", table, pack.arena.device, 7, "arena")
    return _gather_d8("tiles_gather_d8", pack.arena, _arena_args(pack, n_img, c), c, table, ms, bh, bw)


def tiles_scatter_mean(y0: Optional[Tensor], y1: Optional[Tensor], table: Tensor, modes, th: int, tw: int, pack_out,
                       core_px: Optional[int] = None) -> None:
    """tile_scatter_mean into each window's own image of ``pack_out.arena``."""
    ms = _check_modes("tiles_scatter_mean", modes)
    n_img, c = _check_pack("tiles_scatter_mean", pack_out)
    _check_table("tiles_scatter_mean", table, pack_out.arena.device, 7, "arena")
    _scatter_mean("tiles_scatter_mean", y0, y1, table, ms, th, tw, c, pack_out.arena,
                  _arena_args(pack_out, n_img, c), core_px)


# ---------------------------------------------------------------------------
# ... and training batches cut from a uint8 arena (training.DevicePatchLoader)
def patch_batch_ok(c: int, n_img: int, arena_elems: int, n: int, ph: int, pw: int) -> bool:
    """grr_patch_batch_supported in plain Python (tests/test_patch_abi.py checks the two agree): an arena the
    arena entry points take, n, ph, pw >= 1 and n C ph pw < 2^31."""
    return image_arena_ok(c, n_img, arena_elems) and n >= 1 and ph >= 1 and pw >= 1 and n * c * ph * pw < (1 << 31)


class PatchSource:
    """A uint8 image pack that patch_batch's checks have passed (patch_source): the pack, its image count and
    channels, and the images' (H, W) as an int64 array.  A caller that makes many batches from one pack checks it
    once; the checks walk every image of the pack on the host."""
    __slots__ = ("pack", "n_img", "c", "hw")

    def __init__(self, pack, n_img: int, c: int, hw):
        self.pack, self.n_img, self.c, self.hw = pack, n_img, c, hw


def patch_source(pack) -> PatchSource:
    """Check ``pack`` for patch_batch (as the arena wrappers check theirs, and uint8) and return its PatchSource.
    The pack's tensors and host table must not change afterwards."""
    import numpy as np
    n_img, c = _check_pack("patch_batch", pack)
    if pack.arena.dtype != torch.uint8:
        raise ValueError(f"patch_batch: the arena must be uint8, got {pack.arena.dtype}")
    hw = np.asarray(pack.host_table, dtype=np.int64).reshape(n_img, 3)[:, 1:3].copy()
    return PatchSource(pack, n_img, c, hw)


def patch_batch(pack, rows, sample_ids, sigma, seed: int, ph: int, pw: int) -> Tuple[Tensor, Tensor]:
    """(clean, noisy), float32 [n, C, ph, pw] each: sample s is the ph x pw patch of image rows[s][0] of the
    uint8 ``pack`` at (rows[s][1], rows[s][2]), the bottom / right filled by the edge-repeating mirror
    (np.pad "symmetric"), moved by T_mode (rows[s][3], numbered as tiles_gather_d8's), as float(v) / 255; noisy
    adds sigma[s] times a normal that is a function of (seed, sample_ids[s], element) alone (include/grr.h).
    ``pack``: an image pack, checked on every call (host time in proportion to its images), or the PatchSource
    that patch_source made of it once.
    rows [n, 4], sample_ids [n] and sigma [n] are host data (anything np.asarray takes): they are checked here --
    indices inside the pack, modes 0..7, the odd quarter turns only with ph == pw -- and uploaded.  Three device
    tensors (int32 [n, 4], int64 [n], float32 [n], contiguous, on the arena's device) are taken as they are: the
    kernel clamps what it reads from them."""
    src = pack if isinstance(pack, PatchSource) else patch_source(pack)
    table, ids, sg = _patch_tables("patch_batch", src.pack.arena, src.n_img, src.c, src.hw, rows, sample_ids, sigma,
                                   seed, ph, pw)
    return _patch_batch(src.pack, src.n_img, src.c, table, ids, sg, seed, ph, pw)


def _patch_tables(name: str, arena: Tensor, n_img: int, c: int, hw, rows, sample_ids, sigma, seed: int, ph: int,
                  pw: int, no_sigma: bool = False) -> Tuple[Tensor, Tensor, Optional[Tensor]]:
    """The host checks patch_batch and patch_pair_batch share, and the three device tables (int32 [n, 4],
    int64 [n], float32 [n]); no_sigma: ``sigma`` may be None, and stays None."""
    import numpy as np
    if not 0 <= int(seed) < (1 << 64):
        raise ValueError(f"{name}: seed must fit 64 bits, got {seed}")
    absent = no_sigma and sigma is None
    if isinstance(rows, Tensor) and rows.is_cuda:
        n = rows.shape[0] if rows.dim() == 2 else 0
        for t, dtype, shape in ((rows, torch.int32, (n, 4)), (sample_ids, torch.int64, (n,)), (sigma, torch.float32, (n,))):
            if absent and dtype == torch.float32:
                continue
            if not isinstance(t, Tensor) or t.dtype != dtype or tuple(t.shape) != shape or t.device != arena.device \
                    or not t.is_contiguous():
                raise ValueError(f"{name}: device tables are int32 [n, 4], int64 [n] and float32 [n], contiguous "
                                 "and on the arena's device")
        if not isinstance(ph, int) or not isinstance(pw, int) or not patch_batch_ok(c, n_img, arena.numel(), n, ph, pw):
            raise ValueError(f"{name}: patch batch {n} x {c} x {ph} x {pw} must have 1..2^31-1 elements")
        return rows, sample_ids, sigma
    rows = np.asarray(rows)
    if rows.ndim != 2 or rows.shape[1] != 4 or rows.shape[0] < 1 or rows.dtype.kind not in "iu":
        raise ValueError(f"{name}: rows are integers [n, 4] (img, row, col, mode)")
    n = rows.shape[0]
    rows = rows.astype(np.int64)
    ids = np.asarray(sample_ids)
    sg = np.zeros(n, np.float32) if absent else np.asarray(sigma, dtype=np.float32)
    if ids.shape != (n,) or ids.dtype.kind not in "iu" or sg.shape != (n,):
        raise ValueError(f"{name}: sample_ids (integers) and sigma must have one entry per row ({n})")
    if not (np.isfinite(sg).all() and (sg >= 0).all()):
        raise ValueError(f"{name}: sigma must be finite and non-negative")
    if not isinstance(ph, int) or not isinstance(pw, int) or not patch_batch_ok(c, n_img, arena.numel(), n, ph, pw):
        raise ValueError(f"{name}: patch batch {n} x {c} x {ph} x {pw} must have 1..2^31-1 elements")
    if ((rows[:, 0] < 0) | (rows[:, 0] >= n_img)).any():
        raise ValueError(f"{name}: image indices must lie in [0, {n_img})")
    if ((rows[:, 1:3] < 0) | (rows[:, 1:3] >= hw[rows[:, 0]])).any():
        raise ValueError(f"{name}: (row, col) must lie inside the row's image")
    if ((rows[:, 3] < 0) | (rows[:, 3] > 7)).any():
        raise ValueError(f"{name}: modes must lie in 0..7")
    if ph != pw and (rows[:, 3] & 2).any():
        raise ValueError(f"{name}: the odd quarter turns (modes 2, 3, 6, 7) need a square patch, got {ph} x {pw}")
    dev = arena.device
    return (torch.from_numpy(rows.astype(np.int32)).to(dev), torch.from_numpy(ids.astype(np.int64)).to(dev),
            None if absent else torch.from_numpy(np.ascontiguousarray(sg)).to(dev))


def _patch_batch(pack, n_img: int, c: int, table: Tensor, ids: Tensor, sigma: Tensor, seed: int, ph: int,
                 pw: int) -> Tuple[Tensor, Tensor]:
    """patch_batch after its checks, on device tables."""
    arena, n = pack.arena, table.shape[0]
    clean = torch.empty((n, c, ph, pw), dtype=torch.float32, device=arena.device)
    noisy = torch.empty_like(clean)
    _launch("patch_batch", clean.numel() * 9, "grr_patch_batch", arena.data_ptr(), arena.numel(), c,
            pack.table.data_ptr(), n_img, table.data_ptr(), ids.data_ptr(), sigma.data_ptr(), n, int(seed), ph, pw,
            clean.data_ptr(), noisy.data_ptr(), _stream(arena.device))
    return clean, noisy


# ... and from a degraded and a clean arena under one image table (training.PairedImageRestoration)
def patch_pair_batch_ok(c: int, n_img: int, arena_elems: int, n: int, ph: int, pw: int) -> bool:
    """grr_patch_pair_batch_supported in plain Python (tests/test_pair_abi.py checks the two agree): patch_batch_ok's
    bounds; each of the two outputs has n C ph pw < 2^31 elements."""
    return patch_batch_ok(c, n_img, arena_elems, n, ph, pw)


class PatchPairSource:
    """Two uint8 image packs that patch_pair_batch's checks have passed (patch_pair_source): ``input`` the
    degraded pictures, ``target`` their ground truth, one host table and one C; the image count, the channels
    and the images' (H, W) as an int64 array."""
    __slots__ = ("input", "target", "n_img", "c", "hw")

    def __init__(self, input_pack, target_pack, n_img: int, c: int, hw):
        self.input, self.target, self.n_img, self.c, self.hw = input_pack, target_pack, n_img, c, hw


def patch_pair_source(input_pack, target_pack) -> PatchPairSource:
    """Check the two packs for patch_pair_batch -- each as patch_source checks its pack, then: one device, one C,
    one host table (image i of ``input_pack`` is the degraded image i of ``target_pack``; a ValueError names the
    first image that differs) -- and return their PatchPairSource.  The same pack twice is legal.  The packs'
    tensors and host tables must not change afterwards."""
    import numpy as np
    name = "patch_pair_batch"
    checked = []
    for pack in (input_pack, target_pack):
        n_img, c = _check_pack(name, pack)
        if pack.arena.dtype != torch.uint8:
            raise ValueError(f"{name}: the arenas must be uint8, got {pack.arena.dtype}")
        checked.append((n_img, c, tuple(tuple(int(v) for v in row) for row in pack.host_table)))
    (n_img, c, host_in), (n_tgt, c_tgt, host_tgt) = checked
    if input_pack.arena.device != target_pack.arena.device:
        raise ValueError(f"{name}: the two arenas must be on one device (got {input_pack.arena.device} and "
                         f"{target_pack.arena.device})")
    if c != c_tgt:
        raise ValueError(f"{name}: image 0 has {c} channel(s) in the input pack and {c_tgt} in the target pack")
    for i, (a, b) in enumerate(zip(host_in, host_tgt)):
        if a != b:
            raise ValueError(f"{name}: image {i} is (offset, H, W) = {a} in the input pack and {b} in the target "
                             "pack: the packs must share one image table")
    if n_img != n_tgt:
        raise ValueError(f"{name}: image {min(n_img, n_tgt)} exists in one pack only ({n_img} input images, {n_tgt} "
                         "target images)")
    if input_pack.arena.numel() != target_pack.arena.numel():
        raise ValueError(f"{name}: the arenas hold {input_pack.arena.numel()} and {target_pack.arena.numel()} "
                         f"elements after image {n_img - 1}: one length")
    hw = np.asarray(host_in, dtype=np.int64).reshape(n_img, 3)[:, 1:3].copy()
    return PatchPairSource(input_pack, target_pack, n_img, c, hw)


def patch_pair_batch(source: PatchPairSource, rows, sample_ids, sigma, seed: int, ph: int,
                     pw: int) -> Tuple[Tensor, Tensor]:
    """(target, input), float32 [n, C, ph, pw] each, of a patch_pair_source: target is patch_batch's clean patch
    of the target pack, input the same patch (same origin, mirror fill and T_mode) of the input pack, plus
    patch_batch's noise where ``sigma`` is given.  sigma None, or a zero entry, leaves the degraded pixels bit for
    bit.  rows, sample_ids, sigma, seed: as patch_batch takes and checks them."""
    if not isinstance(source, PatchPairSource):
        raise ValueError("patch_pair_batch: source is what patch_pair_source returns")
    table, ids, sg = _patch_tables("patch_pair_batch", source.target.arena, source.n_img, source.c, source.hw, rows,
                                   sample_ids, sigma, seed, ph, pw, no_sigma=True)
    return _patch_pair_batch(source, table, ids, sg, seed, ph, pw)


def _patch_pair_batch(source: PatchPairSource, table: Tensor, ids: Tensor, sigma: Optional[Tensor], seed: int, ph: int,
                      pw: int) -> Tuple[Tensor, Tensor]:
    """patch_pair_batch after its checks, on device tables."""
    arena, n = source.target.arena, table.shape[0]
    target = torch.empty((n, source.c, ph, pw), dtype=torch.float32, device=arena.device)
    inp = torch.empty_like(target)
    _launch("patch_pair_batch", target.numel() * 10, "grr_patch_pair_batch", source.input.arena.data_ptr(),
            arena.data_ptr(), arena.numel(), source.c, source.target.table.data_ptr(), source.n_img, table.data_ptr(),
            ids.data_ptr(), None if sigma is None else sigma.data_ptr(), n, int(seed), ph, pw, target.data_ptr(),
            inp.data_ptr(), _stream(arena.device))
    return target, inp


def u8_sse_segments(a: Tensor, b: Tensor, offsets) -> List[int]:
    """[sum (a - b)^2 over [offsets[i], offsets[i + 1]) for each i]: two 1-D uint8 device tensors of one
    length, all segments in one launch, exact Python ints; one device-to-host copy of the sums (synchronises).
    offsets: n_seg + 1 non-decreasing ints in [0, len(a)] (checked here and uploaded), or a device int64
    tensor (which the kernel clamps)."""
    for t in (a, b):
        if not isinstance(t, Tensor) or t.dtype != torch.uint8 or t.dim() != 1:
            raise ValueError(f"u8_sse_segments: expected 1-D uint8 tensors, got {getattr(t, 'dtype', type(t))}")
    if a.shape != b.shape or a.numel() < 1:
        raise ValueError(f"u8_sse_segments: lengths {tuple(a.shape)} / {tuple(b.shape)} must match and not be 0")
    on_device = isinstance(offsets, Tensor) and offsets.is_cuda
    if on_device:
        if offsets.dtype != torch.int64 or offsets.dim() != 1 or not offsets.is_contiguous():
            raise ValueError("u8_sse_segments: device offsets are a contiguous 1-D int64 tensor")
        n_seg = offsets.numel() - 1
    else:
        host = [int(v) for v in (offsets.tolist() if isinstance(offsets, Tensor) else offsets)]
        n_seg = len(host) - 1
        if any(y < x for x, y in zip([0] + host, host + [a.numel()])):
            raise ValueError(f"u8_sse_segments: offsets must be non-decreasing within [0, {a.numel()}]")
    if not 1 <= n_seg <= MAX_SSE_SEGMENTS:
        raise ValueError(f"u8_sse_segments: 1..{MAX_SSE_SEGMENTS} segments per call (got {n_seg})")
    if not (a.is_cuda and b.is_cuda and a.device == b.device):
        raise RuntimeError("u8_sse_segments: tensors must be on one GPU; the HIP engine has no CPU path")
    if on_device and offsets.device != a.device:
        raise ValueError("u8_sse_segments: the offsets must be on the arrays' device")
    a, b = a.contiguous(), b.contiguous()
    offs = offsets if on_device else torch.tensor(host, dtype=torch.int64).to(a.device)
    out = torch.empty(n_seg, dtype=torch.int64, device=a.device)
    _launch("u8_sse_segments", 2 * a.numel(), "grr_u8_sse_segments", a.data_ptr(), b.data_ptr(), a.numel(),
            offs.data_ptr(), n_seg, out.data_ptr(), _stream(a.device))
    return [int(v) for v in out.tolist()]


# ---------------------------------------------------------------------------
# SSIM of uint8 images (csrc/metric_ops.hip; include/grr.h has the definition).  Both calls return sum q, the exact
# integer sum of q = rint(2^32 s) over the N = (H - 10)(W - 10) C valid values; SSIM = sum q / (2^32 N)
# (restore.ssim_u8 divides).
SSIM_WINDOW = 11              # the Gaussian window's side: an image side below it has no SSIM
SSIM_TILE = (32, 256)         # a workgroup's output rows and interleaved output byte columns ((W - 10) C per row)
SSIM_ONE = 1 << 32            # q of s = 1
MAX_SSIM_IMAGES = 65535       # grr_u8_ssim_images: one grid row per image


def ssim_ok(c: int, h: int, w: int) -> bool:
    """grr_u8_ssim_supported in plain Python (tests/test_ssim_abi.py checks the two agree): 1 <= C <= 4, both
    sides at least 11, H W C < 2^31."""
    return 1 <= c <= 4 and h >= SSIM_WINDOW and w >= SSIM_WINDOW and h * w * c < (1 << 31)


def ssim_count(c: int, h: int, w: int) -> int:
    """N: the values the SSIM of an H x W x C image is the mean of."""
    return (h - SSIM_WINDOW + 1) * (w - SSIM_WINDOW + 1) * c


def _ssim_flops(n: int) -> int:
    return 2 * 110 * n      # 55 horizontal and 55 vertical float64 FMAs per value


def u8_ssim(a: Tensor, b: Tensor) -> int:
    """sum of rint(2^32 s) over the valid pixels and channels of two H x W x C uint8 device images, exact (a
    Python int; synchronises).  Equal images give ssim_count(C, H, W) << 32."""
    for t in (a, b):
        if not isinstance(t, Tensor) or t.dtype != torch.uint8 or t.dim() != 3:
            raise ValueError("u8_ssim: expected H x W x C uint8 tensors, got "
                             f"{tuple(getattr(t, 'shape', ()))} {getattr(t, 'dtype', type(t))}")
    h, w, c = a.shape
    if a.shape != b.shape or not ssim_ok(c, h, w):
        raise ValueError(f"u8_ssim: shapes {tuple(a.shape)} / {tuple(b.shape)} must match, with C <= 4, both sides at "
                         f"least {SSIM_WINDOW} and below 2^31 elements")
    if not (a.is_cuda and b.is_cuda and a.device == b.device):
        raise RuntimeError("u8_ssim: tensors must be on one GPU; the HIP engine has no CPU path")
    a, b = a.contiguous(), b.contiguous()
    out = torch.empty(1, dtype=torch.int64, device=a.device)
    _launch("u8_ssim", 2 * a.numel(), "grr_u8_ssim", a.data_ptr(), b.data_ptr(), h, w, c, out.data_ptr(),
            _stream(a.device), flops=_ssim_flops(ssim_count(c, h, w)))
    return int(out.item())


def _check_pack_pair(name: str, a_pack, b_pack, ok, channels: Optional[int] = None) -> Tuple[int, int, tuple]:
    """(n_img, C, host table) of two uint8 packs that describe the same images on one device, every image passing
    ok(C, H, W) (and C == channels where given); errors before any launch otherwise."""
    n_img, c = _check_pack(name, a_pack, placed=False)
    _check_pack(name, b_pack, placed=False)
    a, b = a_pack.arena, b_pack.arena
    if a.dtype != torch.uint8 or b.dtype != torch.uint8:
        raise ValueError(f"{name}: expected uint8 arenas, got {a.dtype} and {b.dtype}")
    host = tuple(tuple(int(v) for v in row) for row in a_pack.host_table)
    if host != tuple(tuple(int(v) for v in row) for row in b_pack.host_table) or b_pack.c != c or a.numel() != b.numel():
        raise ValueError(f"{name}: the two packs must hold the same images (equal host tables, C and arena "
                         "lengths)")
    if channels is not None and c != channels:
        raise ValueError(f"{name}: the luma is defined for H x W x {channels} images (R, G, B), got C {c}")
    for i, (_, h, w) in enumerate(host):
        if not ok(c, h, w):
            raise ValueError(f"{name}: image {i} needs both sides at least {SSIM_WINDOW} (got {h} x {w} x {c})")
    if n_img > MAX_SSIM_IMAGES:
        raise ValueError(f"{name}: 1..{MAX_SSIM_IMAGES} images per call (got {n_img})")
    _check_placed(name, a_pack)
    _check_placed(name, b_pack)
    if a.device != b.device:
        raise ValueError(f"{name}: the two packs must be on one device")
    return n_img, c, host


def u8_ssim_images(a_pack, b_pack) -> List[int]:
    """[u8_ssim of image i of the two packs for each i] in one launch: exact Python ints, one device-to-host copy
    of the sums (synchronises).  The packs (restore.ImagePack: uint8 arenas) describe the same images: equal host
    tables, one device; every image has both sides at least 11."""
    n_img, c, host = _check_pack_pair("u8_ssim_images", a_pack, b_pack, ssim_ok)
    a, b = a_pack.arena, b_pack.arena
    out = torch.empty(n_img, dtype=torch.int64, device=a.device)
    _launch("u8_ssim_images", 2 * a.numel(), "grr_u8_ssim_images", a.data_ptr(), b.data_ptr(), a.numel(), c,
            a_pack.table.data_ptr(), n_img, max(h for _, h, _ in host), max(w for _, _, w in host), out.data_ptr(),
            _stream(a.device), flops=_ssim_flops(sum(ssim_count(c, h, w) for _, h, w in host)))
    return [int(v) for v in out.tolist()]


# ---------------------------------------------------------------------------
# PSNR and SSIM on the luma of uint8 H x W x 3 images, channels R, G, B (csrc/metric_ops.hip; include/grr.h has the
# definition): Y = Ny / LUMA_SCALE, Ny = 4080000 + 65481 R + 128553 G + 24966 B, the Y of ITU-R BT.601 "studio
# range" YCbCr, not rounded.  u8_luma_sse returns S = sum (Ny(a) - Ny(b))^2, an exact Python int that can exceed 64
# bits (the kernel returns it in two words); PSNR_Y = 10 log10(255^2 LUMA_SCALE^2 N / S) (restore.psnr_y_u8).
# u8_luma_ssim returns sum q of the single plane Y over the luma_ssim_count(H, W) valid positions, as u8_ssim does
# per channel.
LUMA_SCALE = 255000
LUMA_WEIGHTS = (65481, 128553, 24966)     # of R, G, B in Ny; their sum is 219000
LUMA_SSIM_TILE = (32, 256)    # a workgroup's output rows and output pixel columns
LUMA_SSE_BLOCK = (2048, 8)    # the pixels a workgroup and a lane take per step
LUMA_SSE_MAX_BLOCKS = 1024    # workgroups of a single-image call: beyond them each strides over the image


def luma_ok(h: int, w: int, need_window: bool = False) -> bool:
    """grr_u8_luma_supported in plain Python (tests/test_luma_abi.py checks the two agree): both sides at least 1,
    at least 11 where the SSIM window is needed, H W 3 < 2^31."""
    least = SSIM_WINDOW if need_window else 1
    return h >= least and w >= least and h * w * 3 < (1 << 31)


def luma_ssim_count(h: int, w: int) -> int:
    """N: the values the luma SSIM of an H x W x 3 image is the mean of."""
    return (h - SSIM_WINDOW + 1) * (w - SSIM_WINDOW + 1)


def _check_luma_pair(name: str, a, b, need_window: bool) -> Tuple[int, int]:
    """(H, W) of two H x W x 3 uint8 device images of one shape; errors before any launch otherwise."""
    for t in (a, b):
        if not isinstance(t, Tensor) or t.dtype != torch.uint8 or t.dim() != 3:
            raise ValueError(f"{name}: expected H x W x 3 uint8 tensors, got "
                             f"{tuple(getattr(t, 'shape', ()))} {getattr(t, 'dtype', type(t))}")
    h, w, c = a.shape
    if c != 3:
        raise ValueError(f"{name}: the luma is defined for H x W x 3 images (R, G, B), got {tuple(a.shape)}")
    if a.shape != b.shape or not luma_ok(h, w, need_window):
        raise ValueError(f"{name}: shapes {tuple(a.shape)} / {tuple(b.shape)} must match, with both sides at "
                         f"least {SSIM_WINDOW if need_window else 1} and below 2^31 elements")
    if not (a.is_cuda and b.is_cuda and a.device == b.device):
        raise RuntimeError(f"{name}: tensors must be on one GPU; the HIP engine has no CPU path")
    return h, w


def _luma_sse_of(words) -> int:
    """sum (D^2 mod 2^32) + (sum (D^2 >> 32) << 32)."""
    return int(words[0]) + (int(words[1]) << 32)


def u8_luma_sse(a: Tensor, b: Tensor) -> int:
    """S = sum over the pixels of (Ny(a) - Ny(b))^2 of two H x W x 3 uint8 device images, exact (a Python int, up
    to 82 bits; synchronises)."""
    h, w = _check_luma_pair("u8_luma_sse", a, b, False)
    a, b = a.contiguous(), b.contiguous()
    out = torch.empty(2, dtype=torch.int64, device=a.device)
    _launch("u8_luma_sse", 2 * a.numel(), "grr_u8_luma_sse", a.data_ptr(), b.data_ptr(), h, w, out.data_ptr(),
            _stream(a.device))
    return _luma_sse_of(out.tolist())


def u8_luma_sse_images(a_pack, b_pack) -> List[int]:
    """[u8_luma_sse of image i of the two packs for each i] in one launch: exact Python ints, one device-to-host
    copy of the sums (synchronises).  The packs (restore.ImagePack: uint8 arenas, C = 3) describe the same images:
    equal host tables, one device."""
    n_img, _, host = _check_pack_pair("u8_luma_sse_images", a_pack, b_pack, lambda c, h, w: luma_ok(h, w), 3)
    a, b = a_pack.arena, b_pack.arena
    out = torch.empty((n_img, 2), dtype=torch.int64, device=a.device)
    _launch("u8_luma_sse_images", 2 * a.numel(), "grr_u8_luma_sse_images", a.data_ptr(), b.data_ptr(), a.numel(),
            a_pack.table.data_ptr(), n_img, out.data_ptr(), _stream(a.device))
    return [_luma_sse_of(row) for row in out.tolist()]


def u8_luma_ssim(a: Tensor, b: Tensor) -> int:
    """sum of rint(2^32 s) over the valid pixels of the luma planes of two H x W x 3 uint8 device images, exact (a
    Python int; synchronises).  Equal images give luma_ssim_count(H, W) << 32."""
    h, w = _check_luma_pair("u8_luma_ssim", a, b, True)
    a, b = a.contiguous(), b.contiguous()
    out = torch.empty(1, dtype=torch.int64, device=a.device)
    _launch("u8_luma_ssim", 2 * a.numel(), "grr_u8_luma_ssim", a.data_ptr(), b.data_ptr(), h, w, out.data_ptr(),
            _stream(a.device), flops=_ssim_flops(luma_ssim_count(h, w)))
    return int(out.item())


def u8_luma_ssim_images(a_pack, b_pack) -> List[int]:
    """[u8_luma_ssim of image i of the two packs for each i] in one launch: exact Python ints, one device-to-host
    copy of the sums (synchronises).  Packs as for u8_luma_sse_images; every image has both sides at least 11."""
    n_img, _, host = _check_pack_pair("u8_luma_ssim_images", a_pack, b_pack, lambda c, h, w: luma_ok(h, w, True), 3)
    a, b = a_pack.arena, b_pack.arena
    out = torch.empty(n_img, dtype=torch.int64, device=a.device)
    _launch("u8_luma_ssim_images", 2 * a.numel(), "grr_u8_luma_ssim_images", a.data_ptr(), b.data_ptr(), a.numel(),
            a_pack.table.data_ptr(), n_img, max(h for _, h, _ in host), max(w for _, _, w in host), out.data_ptr(),
            _stream(a.device), flops=_ssim_flops(sum(luma_ssim_count(h, w) for _, h, w in host)))
    return [int(v) for v in out.tolist()]


# ---------------------------------------------------------------------------
# The SSIM training loss on float32 planar batches (csrc/ssim_loss_ops.hip; include/grr.h has the definition): the
# index above on [B, C, H, W] planes of data range 1, x the prediction and y the target.  The forward returns the
# exact integer sum q per batch item and, on request, the float64 coefficient planes [3, B, C, H - 10, W - 10] the
# reverse gathers the gradient from (losses.py wraps the two for autograd).
SSIM_LOSS_TILE = (32, 256)        # a workgroup's rows and columns: valid positions (forward), pixels (reverse)
MAX_SSIM_LOSS_PLANES = 65535      # B C: one grid row per plane


def ssim_loss_ok(b: int, c: int, h: int, w: int) -> bool:
    """grr_ssim_loss_supported in plain Python (tests/test_ssim_loss_abi.py checks the two agree): B, C >= 1, both
    sides at least 11, B C <= 65535, B C H W < 2^31."""
    return (b >= 1 and c >= 1 and h >= SSIM_WINDOW and w >= SSIM_WINDOW and b * c <= MAX_SSIM_LOSS_PLANES
            and b * c * h * w < (1 << 31))


def ssim_loss_count(b: int, c: int, h: int, w: int) -> int:
    """N: the values the loss is one minus the mean of."""
    return b * c * (h - SSIM_WINDOW + 1) * (w - SSIM_WINDOW + 1)


def _check_ssim_loss(name: str, x: Tensor, y: Tensor, placed: bool = True) -> Tuple[int, int, int, int]:
    """(B, C, H, W) of a prediction / target pair the loss takes; placed: they must also be on one GPU."""
    for t in (x, y):
        if not isinstance(t, Tensor) or t.dim() != 4:
            raise ValueError(f"{name}: expected [B, C, H, W] tensors, got {tuple(getattr(t, 'shape', ()))}")
        if t.dtype != torch.float32:
            raise ValueError(f"{name}: expected float32, got {t.dtype}")
    if x.shape != y.shape:
        raise ValueError(f"{name}: shapes {tuple(x.shape)} / {tuple(y.shape)} must match")
    b, c, h, w = x.shape
    if min(h, w) < SSIM_WINDOW:
        raise ValueError(f"{name}: both sides must be at least {SSIM_WINDOW}, the window's (got {h} x {w})")
    if not ssim_loss_ok(b, c, h, w):
        raise ValueError(f"{name}: needs B C <= {MAX_SSIM_LOSS_PLANES} and below 2^31 elements (got {tuple(x.shape)})")
    if not (x.is_contiguous() and y.is_contiguous()):
        raise ValueError(f"{name}: expected contiguous tensors")
    if placed and not (x.is_cuda and y.is_cuda and x.device == y.device):
        raise RuntimeError(f"{name}: tensors must be on one GPU; the HIP engine has no CPU path")
    return b, c, h, w


def ssim_loss_forward(x: Tensor, y: Tensor, want_coef: bool) -> Tuple[Tensor, Optional[Tensor]]:
    """(qsum, coef): qsum int64 [B] on the device, the exact sum of rint(2^32 s) over each item's positions (no
    synchronisation); coef the float64 planes [3, B, C, H - 10, W - 10] of ds/dmx, ds/dE[x^2], ds/dE[xy], or None
    (nothing allocated or written) unless want_coef."""
    b, c, h, w = _check_ssim_loss("ssim_loss_forward", x, y)
    n = ssim_loss_count(b, c, h, w)
    qsum = torch.empty(b, dtype=torch.int64, device=x.device)
    coef = torch.empty((3, b, c, h - SSIM_WINDOW + 1, w - SSIM_WINDOW + 1), dtype=torch.float64,
                       device=x.device) if want_coef else None
    _launch("ssim_loss_forward", 8 * x.numel() + 8 * b + (24 * n if want_coef else 0), "grr_ssim_loss_forward",
            x.data_ptr(), y.data_ptr(), b, c, h, w, qsum.data_ptr(), _ptr(coef), _stream(x.device),
            flops=_ssim_flops(n) + (30 + (20 if want_coef else 0)) * n)
    return qsum, coef


def ssim_loss_backward(x: Tensor, y: Tensor, coef: Tensor, gout: Tensor) -> Tensor:
    """gx = gout dloss/dx, float32 like x, from the forward's coefficient planes; gout: one float32 on the device,
    read by the kernel."""
    b, c, h, w = _check_ssim_loss("ssim_loss_backward", x, y, placed=False)
    shape = (3, b, c, h - SSIM_WINDOW + 1, w - SSIM_WINDOW + 1)
    if not isinstance(coef, Tensor) or coef.dtype != torch.float64 or tuple(coef.shape) != shape or not coef.is_contiguous():
        raise ValueError(f"ssim_loss_backward: coef must be the forward's contiguous float64 {shape} planes, got "
                         f"{tuple(getattr(coef, 'shape', ()))} {getattr(coef, 'dtype', type(coef))}")
    if not isinstance(gout, Tensor) or gout.dtype != torch.float32 or gout.numel() != 1:
        raise ValueError("ssim_loss_backward: gout must be one float32 value, got "
                         f"{tuple(getattr(gout, 'shape', ()))} {getattr(gout, 'dtype', type(gout))}")
    if not (x.is_cuda and all(t.device == x.device for t in (y, coef, gout))):
        raise RuntimeError("ssim_loss_backward: tensors must be on one GPU; the HIP engine has no CPU path")
    gx = torch.empty_like(x)
    _launch("ssim_loss_backward", 12 * x.numel() + 8 * coef.numel() + 4, "grr_ssim_loss_backward", x.data_ptr(),
            y.data_ptr(), coef.data_ptr(), gout.data_ptr(), gx.data_ptr(), b, c, h, w, _stream(x.device),
            flops=(2 * 66 + 8) * x.numel())
    return gx


# ---------------------------------------------------------------------------
# Exact bicubic resize of uint8 images by an integer scale (csrc/resize_ops.hip; include/grr.h has the definition):
# MATLAB imresize's convention with fixed-point weights, every tap set summing to 2^30.  The tap sets are computed
# here from exact rationals and handed to the library as host arrays, as the mode lists above are.
RESIZE_SCALES = (2, 8)        # the smallest and the largest scale
RESIZE_ONE = 1 << 30          # the sum of a tap set
RESIZE_TILE = 32              # a workgroup's output rows and columns
MAX_RESIZE_IMAGES = 65535     # grr_u8_resize_images: one grid row per image


def _cubic(x):
    from fractions import Fraction
    x = abs(x)
    if x <= 1:
        return Fraction(3, 2) * x ** 3 - Fraction(5, 2) * x ** 2 + 1
    if x < 2:
        return Fraction(-1, 2) * x ** 3 + Fraction(5, 2) * x ** 2 - 4 * x + 2
    return Fraction(0)


_RESIZE_TAPS = {}


def resize_taps(s: int, up: bool) -> tuple:
    """The quantised tap sets of scale ``s``: a tuple of phases -- one for down, whose offsets count from i s; s for
    up, phase p = y mod s, whose offsets count from y // s -- each a tuple of (offset, q) pairs with
    sum q = 2^30 and the zero taps dropped (8 / 9 / 16 / 32 taps down for s = 2 / 3 / 4 / 8, at most 4 up).
    Exact: the raw weights are Fractions, normalised by their sum, rounded half to even at 2^-30, and the remainder
    goes to the largest tap (the lowest index among equals).  Cached."""
    from fractions import Fraction
    key = (int(s), bool(up))
    if key not in _RESIZE_TAPS:
        s = key[0]
        if not RESIZE_SCALES[0] <= s <= RESIZE_SCALES[1]:
            raise ValueError(f"resize_taps: the scale is an integer of {RESIZE_SCALES[0]}..{RESIZE_SCALES[1]}, got {s}")
        sets = []
        for p in range(s if key[1] else 1):
            if key[1]:
                u, reach, width = Fraction(2 * p + 1, 2 * s) - Fraction(1, 2), 2, 1
            else:
                u, reach, width = Fraction(s - 1, 2), 2 * s, s
            offsets = [j for j in range(-3 * width, 4 * width) if abs(u - j) < reach]
            raw = [_cubic((u - j) / width) for j in offsets]
            total = sum(raw)
            q = [round(w / total * RESIZE_ONE) for w in raw]         # Fraction.__round__: half to even
            q[q.index(max(q))] += RESIZE_ONE - sum(q)
            sets.append(tuple((o, v) for o, v in zip(offsets, q) if v))
        _RESIZE_TAPS[key] = tuple(sets)
    return _RESIZE_TAPS[key]


_RESIZE_TAP_ARGS = {}


def _resize_tap_args(s: int, up: bool) -> tuple:
    """(n_phase, first, count, taps) as the entry points take them: per phase a run of consecutive offsets from its
    first tap to its last, a dropped zero in between passed as 0.  The ctypes arrays are cached (and so alive)."""
    key = (int(s), bool(up))
    if key not in _RESIZE_TAP_ARGS:
        first, count, flat = [], [], []
        for phase in resize_taps(*key):
            by_offset = dict(phase)
            lo, hi = min(by_offset), max(by_offset)
            first.append(lo)
            count.append(hi - lo + 1)
            flat.extend(by_offset.get(o, 0) for o in range(lo, hi + 1))
        arr = lambda v: (ctypes.c_int32 * len(v))(*v)
        _RESIZE_TAP_ARGS[key] = (len(first), arr(first), arr(count), arr(flat))
    return _RESIZE_TAP_ARGS[key]


def resize_ok(c: int, h: int, w: int, s: int, up) -> bool:
    """grr_u8_resize_supported in plain Python (tests/test_resize_abi.py checks the two agree): 1 <= C <= 4,
    2 <= s <= 8, sides >= 1, and the input's and the output's element counts (down: ceil(H / s) ceil(W / s) C, up:
    s H s W C) below 2^31."""
    if not (1 <= c <= 4 and RESIZE_SCALES[0] <= s <= RESIZE_SCALES[1] and h >= 1 and w >= 1):
        return False
    out = s * h * s * w if up else -(-h // s) * -(-w // s)
    return h * w * c < (1 << 31) and out * c < (1 << 31)


def resize_out_hw(name: str, h: int, w: int, s: int, up, out_hw=None) -> Tuple[int, int]:
    """The output sides of an h x w image: down ceil(h / s) x ceil(w / s); up s h x s w, or ``out_hw`` where each
    side n of it has s (n_in - 1) < n <= s n_in.  ValueError otherwise."""
    if not up:
        want = (-(-h // s), -(-w // s))
        if out_hw is not None and tuple(int(v) for v in out_hw) != want:
            raise ValueError(f"{name}: {h} x {w} at scale {s} shrinks to {want[0]} x {want[1]}, got {tuple(out_hw)}")
        return want
    if out_hw is None:
        return s * h, s * w
    ho, wo = (int(v) for v in out_hw)
    if not (s * (h - 1) < ho <= s * h and s * (w - 1) < wo <= s * w):
        raise ValueError(f"{name}: {h} x {w} at scale {s} grows to sides in (s (n - 1), s n], got {ho} x {wo}")
    return ho, wo


def _check_scale(name: str, s) -> int:
    if isinstance(s, bool) or not isinstance(s, int) or not RESIZE_SCALES[0] <= s <= RESIZE_SCALES[1]:
        raise ValueError(f"{name}: the scale is an integer of {RESIZE_SCALES[0]}..{RESIZE_SCALES[1]}, got {s!r}")
    return s


def _resize_bytes(shapes, out_shapes, c: int) -> int:
    """Algorithmic bytes of a resize: every input byte read once and every output byte written once."""
    return sum(h * w * c for h, w in shapes) + sum(h * w * c for h, w in out_shapes)


def u8_resize(img: Tensor, s: int, up, out_hw=None) -> Tensor:
    """The exact bicubic resize of an H x W x C uint8 device image (include/grr.h): ``up`` false shrinks it to
    ceil(H / s) x ceil(W / s) with the antialiased kernel, ``up`` true grows it to s H x s W, or to ``out_hw`` with
    s (n - 1) < side <= s n (the size a down pass came from).  Rows first, then columns, rounded to uint8 after
    each; both in one launch.  A non-contiguous image is copied first."""
    name = "u8_resize"
    s, up = _check_scale(name, s), bool(up)
    if isinstance(img, Tensor) and img.dtype != torch.uint8:
        raise ValueError(f"{name}: the image must be uint8, got {img.dtype}")
    h, w, c = _check_image(name, img)
    ho, wo = resize_out_hw(name, h, w, s, up, out_hw)
    if not resize_ok(c, h, w, s, up):
        raise ValueError(f"{name}: needs fewer than 2^31 input and output elements, got {tuple(img.shape)} at scale {s}")
    img = img.contiguous()
    out = torch.empty((ho, wo, c), dtype=torch.uint8, device=img.device)
    _launch("u8_resize", _resize_bytes([(h, w)], [(ho, wo)], c), "grr_u8_resize", img.data_ptr(), h, w, c,
            out.data_ptr(), ho, wo, s, int(up), *_resize_tap_args(s, up), _stream(img.device))
    return out


def u8_resize_images(pack, s: int, up, out_shapes=None):
    """u8_resize of every image of a uint8 image pack into a new pack (a restore.ImagePack of the resized sizes,
    the images back to back), one launch per 65535 images.  ``out_shapes``: with ``up``, the (h, w) each image
    grows to (default: s H x s W)."""
    from .restore import ImagePack, _host_table
    name = "u8_resize_images"
    s, up = _check_scale(name, s), bool(up)
    n_img, c = _check_pack(name, pack)
    if pack.arena.dtype != torch.uint8:
        raise ValueError(f"{name}: the arena must be uint8, got {pack.arena.dtype}")
    shapes = [(int(h), int(w)) for _, h, w in pack.host_table]
    if out_shapes is not None and len(out_shapes) != n_img:
        raise ValueError(f"{name}: {len(out_shapes)} output shapes for {n_img} images")
    outs = []
    for i, (h, w) in enumerate(shapes):
        try:
            outs.append(resize_out_hw(name, h, w, s, up, None if out_shapes is None else out_shapes[i]))
        except ValueError as e:
            raise ValueError(f"{e} (image {i})") from None
        if not resize_ok(c, h, w, s, up):
            raise ValueError(f"{name}: image {i} needs fewer than 2^31 input and output elements, got {h} x {w} x {c} "
                             f"at scale {s}")
    host_table, total = _host_table(outs, c)
    dev = pack.arena.device
    arena = torch.empty(total, dtype=torch.uint8, device=dev)
    table = torch.tensor(host_table, dtype=torch.int64).to(dev)
    taps = _resize_tap_args(s, up)
    for at in range(0, n_img, MAX_RESIZE_IMAGES):
        n = min(MAX_RESIZE_IMAGES, n_img - at)
        part = outs[at:at + n]
        _launch("u8_resize_images", _resize_bytes(shapes[at:at + n], part, c), "grr_u8_resize_images",
                pack.arena.data_ptr(), pack.arena.numel(), pack.table.data_ptr() + at * 24, arena.data_ptr(), total,
                table.data_ptr() + at * 24, c, n, max(h for h, _ in part), max(w for _, w in part), s, int(up), *taps,
                _stream(dev))
    return ImagePack(arena, table, host_table, c, tuple(getattr(pack, "kinds", ())))


def u8_bicubic_degrade(img: Tensor, s: int) -> Tensor:
    """The bicubic super-resolution input of an H x W x C uint8 device image, at its size: u8_resize down by ``s``,
    then up to H x W.  Two launches; the low-resolution image between them is the only other buffer."""
    h, w = int(img.shape[0]), int(img.shape[1])
    return u8_resize(u8_resize(img, s, False), s, True, (h, w))


def u8_bicubic_degrade_images(pack, s: int):
    """u8_bicubic_degrade of every image of a uint8 pack, the results back to back.  Where ``pack``'s images lie back
    to back as well (as pack_images lays them) the result has its host table and shares its device image table, so
    the two can form a patch_pair_source.  Two launches per 65535 images."""
    low = u8_resize_images(pack, s, False)
    out = u8_resize_images(low, s, True, [(h, w) for _, h, w in pack.host_table])
    same = out.host_table == tuple(tuple(int(v) for v in row) for row in pack.host_table)
    return type(out)(out.arena, pack.table, out.host_table, out.c, out.kinds) if same else out


# ---------------------------------------------------------------------------
# The JPEG round trip decode(encode(x)) of uint8 images in libjpeg's integer arithmetic (csrc/jpeg_ops.hip;
# include/grr.h has the definition) and the blocking sums of PSNR-B (csrc/metric_ops.hip).  The quantisation tables
# are made from the quality on the device: the library takes the quality itself.
JPEG_TILE = 32                # a workgroup's rows and columns of the picture
JPEG_QUALITIES = (1, 100)     # the smallest and the largest quality
JPEG_SUBSAMPLINGS = (0, 2)    # 4:4:4 and 4:2:0, Pillow's numbering
MAX_JPEG_IMAGES = 65535       # grr_u8_jpeg_images: one grid row per image
BLOCKING_BLOCK = 2048         # the bytes a workgroup of the blocking kernel takes per step
BLOCKING_MAX_BLOCKS = 1024    # workgroups of a single-image call: beyond them each strides over the image
PSNRB_MIN_SIDE = 16           # PSNR-B is defined for pictures with both sides at least 16


def jpeg_ok(c: int, h: int, w: int, sub: int = 0) -> bool:
    """grr_u8_jpeg_supported in plain Python (tests/test_jpeg_abi.py checks the two agree): C of 1 or 3, a
    subsampling of 0 or 2, sides >= 1, H W C < 2^31."""
    return c in (1, 3) and sub in JPEG_SUBSAMPLINGS and h >= 1 and w >= 1 and h * w * c < (1 << 31)


def _check_quality(name: str, q) -> int:
    if isinstance(q, (bool, np.bool_)) or not isinstance(q, (int, np.integer)) \
            or not JPEG_QUALITIES[0] <= q <= JPEG_QUALITIES[1]:
        raise ValueError(f"{name}: the quality is an integer of {JPEG_QUALITIES[0]}..{JPEG_QUALITIES[1]}, got {q!r}")
    return int(q)


def _check_subsampling(name: str, sub) -> int:
    if isinstance(sub, (bool, np.bool_)) or not isinstance(sub, (int, np.integer)) or sub not in JPEG_SUBSAMPLINGS:
        raise ValueError(f"{name}: the subsampling is 0 (4:4:4) or 2 (4:2:0), got {sub!r}")
    return int(sub)


def u8_jpeg(img: Tensor, quality: int, subsampling: int = 0) -> Tensor:
    """The JPEG round trip of an H x W x C uint8 device image, C of 1 or 3, at ``quality`` (1..100): what decoding
    its baseline JPEG gives, byte for byte as libjpeg-turbo (Pillow) computes it, without a bitstream
    (include/grr.h).  ``subsampling``: 0 for 4:4:4, 2 for 4:2:0 (Pillow's numbering; a gray image has no chroma
    and ignores it).  One launch.  A non-contiguous image is copied first."""
    name = "u8_jpeg"
    quality, sub = _check_quality(name, quality), _check_subsampling(name, subsampling)
    if isinstance(img, Tensor) and img.dtype != torch.uint8:
        raise ValueError(f"{name}: the image must be uint8, got {img.dtype}")
    if isinstance(img, Tensor) and img.dim() == 3 and img.shape[2] not in (1, 3):
        raise ValueError(f"{name}: needs 1 or 3 channels (gray or R, G, B), got {tuple(img.shape)}")
    h, w, c = _check_image(name, img)
    img = img.contiguous()
    out = torch.empty_like(img)
    _launch("u8_jpeg", 2 * img.numel(), "grr_u8_jpeg", img.data_ptr(), h, w, c, out.data_ptr(), quality, sub,
            _stream(img.device))
    return out


def u8_jpeg_images(pack, qualities, subsampling: int = 0):
    """u8_jpeg of every image of a uint8 image pack into a new pack that shares its image table (so the two can
    form a patch_pair_source), one launch per 65535 images.  ``qualities``: one integer for all images, a sequence
    of one integer per image (checked here), or an int32 device tensor of one value per image (which the kernel
    clamps into 1..100, as it does every device table)."""
    from .restore import ImagePack
    name = "u8_jpeg_images"
    sub = _check_subsampling(name, subsampling)
    n_img, c = _check_pack(name, pack, placed=False)
    if pack.arena.dtype != torch.uint8:
        raise ValueError(f"{name}: the arena must be uint8, got {pack.arena.dtype}")
    shapes = [(int(h), int(w)) for _, h, w in pack.host_table]
    for i, (h, w) in enumerate(shapes):
        if not jpeg_ok(c, h, w, sub):
            raise ValueError(f"{name}: image {i} needs 1 or 3 channels (gray or R, G, B), got {h} x {w} x {c}")
    dev = pack.arena.device
    if not isinstance(qualities, Tensor):       # the host list is checked before anything is asked of the device
        if isinstance(qualities, (int, np.integer)) and not isinstance(qualities, (bool, np.bool_)):
            qualities = [qualities] * n_img
        if len(qualities) != n_img:
            raise ValueError(f"{name}: {len(qualities)} qualities for {n_img} images")
        qualities = [_check_quality(name, v) for v in qualities]
    _check_placed(name, pack)
    if isinstance(qualities, Tensor):
        if qualities.dtype != torch.int32 or tuple(qualities.shape) != (n_img,) or qualities.device != dev \
                or not qualities.is_contiguous():
            raise ValueError(f"{name}: a quality tensor is int32 [{n_img}], contiguous and on the arena's device")
        q = qualities
    else:
        q = torch.tensor(qualities, dtype=torch.int32).to(dev)
    covered = sum(h * w * c for h, w in shapes) == pack.arena.numel()
    arena = (torch.empty_like if covered else torch.zeros_like)(pack.arena)      # bytes between images stay 0
    for at in range(0, n_img, MAX_JPEG_IMAGES):
        n = min(MAX_JPEG_IMAGES, n_img - at)
        part = shapes[at:at + n]
        _launch("u8_jpeg_images", 2 * sum(h * w * c for h, w in part), "grr_u8_jpeg_images", pack.arena.data_ptr(),
                pack.arena.numel(), c, pack.table.data_ptr() + at * 24, n, max(h for h, _ in part),
                max(w for _, w in part), arena.data_ptr(), q.data_ptr() + at * 4, sub, _stream(dev))
    return ImagePack(arena, pack.table, tuple(tuple(int(v) for v in row) for row in pack.host_table), c,
                     tuple(getattr(pack, "kinds", ())))


def u8_blocking(est: Tensor) -> Tuple[int, int, int, int]:
    """(S_b, N_b, S_n, N_n) of an H x W x C uint8 device image (include/grr.h, PSNR-B): the sums of squared
    differences and the counts of the adjacent same-channel pairs that straddle a multiple-of-8 line and of those
    that do not, exact Python ints (synchronises)."""
    name = "u8_blocking"
    if isinstance(est, Tensor) and est.dtype != torch.uint8:
        raise ValueError(f"{name}: the image must be uint8, got {est.dtype}")
    h, w, c = _check_image(name, est)
    est = est.contiguous()
    out = torch.empty(4, dtype=torch.int64, device=est.device)
    _launch("u8_blocking", est.numel(), "grr_u8_blocking", est.data_ptr(), h, w, c, out.data_ptr(), _stream(est.device))
    return tuple(int(v) for v in out.tolist())


def u8_blocking_images(pack) -> List[Tuple[int, int, int, int]]:
    """[u8_blocking of image i of a uint8 pack for each i] in one launch (synchronises)."""
    name = "u8_blocking_images"
    n_img, c = _check_pack(name, pack)
    if pack.arena.dtype != torch.uint8:
        raise ValueError(f"{name}: the arena must be uint8, got {pack.arena.dtype}")
    if n_img > MAX_SSIM_IMAGES:
        raise ValueError(f"{name}: 1..{MAX_SSIM_IMAGES} images per call (got {n_img})")
    a = pack.arena
    out = torch.empty((n_img, 4), dtype=torch.int64, device=a.device)
    _launch("u8_blocking_images", a.numel(), "grr_u8_blocking_images", a.data_ptr(), a.numel(), c,
            pack.table.data_ptr(), n_img, max(int(h) for _, h, _ in pack.host_table),
            max(int(w) for _, _, w in pack.host_table), out.data_ptr(), _stream(a.device))
    return [tuple(int(v) for v in row) for row in out.tolist()]


# ---------------------------------------------------------------------------
# Bayer mosaicking and the initial fill of demosaicking (csrc/demosaic_ops.hip; include/grr.h has the definition):
# an RGB picture sampled through a colour filter array, its missing channels filled by a fixed integer filter.
DEMOSAIC_TILE = (16, 64)      # a workgroup's rows and columns of the picture
DEMOSAIC_PATTERNS = ("rggb", "grbg", "gbrg", "bggr")      # the top-left 2 x 2 cell in reading order; the index is the code
DEMOSAIC_FILLS = ("zero", "bilinear", "malvar")           # the index is the code
MAX_DEMOSAIC_IMAGES = 65535   # grr_u8_demosaic_images: one grid row per image


def demosaic_ok(src_c: int, h: int, w: int) -> bool:
    """grr_u8_demosaic_supported in plain Python (tests/test_demosaic_abi.py checks the two agree): a source of 1 or
    3 channels, sides >= 1, 3 H W < 2^31."""
    return src_c in (1, 3) and h >= 1 and w >= 1 and 3 * h * w < (1 << 31)


def _check_code(name: str, what: str, names, v) -> int:
    if isinstance(v, str) and v in names:
        return names.index(v)
    if isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)) and 0 <= v < len(names):
        return int(v)
    raise ValueError(f"{name}: the {what} is one of {names} or its code 0..{len(names) - 1}, got {v!r}")


def _check_pattern(name: str, pattern) -> int:
    """The code of a Bayer pattern given by name or code; ValueError otherwise."""
    return _check_code(name, "pattern", DEMOSAIC_PATTERNS, pattern)


def _check_fill(name: str, fill) -> int:
    """The code of a fill given by name or code; ValueError otherwise."""
    return _check_code(name, "fill", DEMOSAIC_FILLS, fill)


def u8_demosaic(img: Tensor, pattern, fill="malvar") -> Tensor:
    """The Bayer mosaic of a uint8 device image with its missing channels filled, H x W x 3 (include/grr.h).
    ``img``: H x W x 3 (R, G, B: the mosaic keeps the site's channel of each pixel), or H x W x 1 or H x W (already
    the mosaic plane).  ``pattern``: "rggb", "grbg", "gbrg", "bggr" or the code 0..3; ``fill``: "zero", "bilinear",
    "malvar" (Malvar-He-Cutler, the default) or the code 0..2.  One launch.  A non-contiguous image is copied first."""
    name = "u8_demosaic"
    pattern, fill = _check_pattern(name, pattern), _check_fill(name, fill)
    if isinstance(img, Tensor) and img.dtype != torch.uint8:
        raise ValueError(f"{name}: the image must be uint8, got {img.dtype}")
    if isinstance(img, Tensor) and img.dim() == 2:
        img = img[:, :, None]
    if isinstance(img, Tensor) and img.dim() == 3 and img.shape[2] not in (1, 3):
        raise ValueError(f"{name}: needs 1 channel (the mosaic) or 3 (R, G, B), got {tuple(img.shape)}")
    h, w, c = _check_image(name, img)
    if not demosaic_ok(c, h, w):
        raise ValueError(f"{name}: needs 3 H W < 2^31, got {tuple(img.shape)}")
    img = img.contiguous()
    out = torch.empty((h, w, 3), dtype=torch.uint8, device=img.device)
    _launch("u8_demosaic", img.numel() + out.numel(), "grr_u8_demosaic", img.data_ptr(), h, w, c, out.data_ptr(),
            pattern, fill, _stream(img.device))
    return out


def u8_demosaic_images(pack, patterns, fill="malvar"):
    """u8_demosaic of every image of a uint8 RGB image pack into a new pack that shares its image table (so the two
    can form a patch_pair_source), one launch per 65535 images.  ``patterns``: one name or code for all images, a
    sequence of one per image (checked here), or an int32 device tensor of one code per image (which the kernel
    clamps into 0..3, as it does every device table)."""
    from .restore import ImagePack
    name = "u8_demosaic_images"
    fill = _check_fill(name, fill)
    n_img, c = _check_pack(name, pack, placed=False)
    if pack.arena.dtype != torch.uint8:
        raise ValueError(f"{name}: the arena must be uint8, got {pack.arena.dtype}")
    if c != 3:
        raise ValueError(f"{name}: the arena form takes R, G, B pictures, got {c} channel(s)")
    shapes = [(int(h), int(w)) for _, h, w in pack.host_table]
    dev = pack.arena.device
    if not isinstance(patterns, Tensor):        # the host list is checked before anything is asked of the device
        if isinstance(patterns, (str, int, np.integer)):
            patterns = [patterns] * n_img
        if len(patterns) != n_img:
            raise ValueError(f"{name}: {len(patterns)} patterns for {n_img} images")
        patterns = [_check_pattern(name, v) for v in patterns]
    _check_placed(name, pack)
    if isinstance(patterns, Tensor):
        if patterns.dtype != torch.int32 or tuple(patterns.shape) != (n_img,) or patterns.device != dev \
                or not patterns.is_contiguous():
            raise ValueError(f"{name}: a pattern tensor is int32 [{n_img}], contiguous and on the arena's device")
        p = patterns
    else:
        p = torch.tensor(patterns, dtype=torch.int32).to(dev)
    covered = sum(h * w * 3 for h, w in shapes) == pack.arena.numel()
    arena = (torch.empty_like if covered else torch.zeros_like)(pack.arena)      # bytes between images stay 0
    for at in range(0, n_img, MAX_DEMOSAIC_IMAGES):
        n = min(MAX_DEMOSAIC_IMAGES, n_img - at)
        part = shapes[at:at + n]
        _launch("u8_demosaic_images", 2 * sum(h * w * 3 for h, w in part), "grr_u8_demosaic_images",
                pack.arena.data_ptr(), pack.arena.numel(), pack.table.data_ptr() + at * 24, n,
                max(h for h, _ in part), max(w for _, w in part), arena.data_ptr(), p.data_ptr() + at * 4, fill,
                _stream(dev))
    return ImagePack(arena, pack.table, tuple(tuple(int(v) for v in row) for row in pack.host_table), 3,
                     tuple(getattr(pack, "kinds", ())))


# ---------------------------------------------------------------------------
# Joint denoising and demosaicking (csrc/rawnoise_ops.hip; include/grr.h has the definition): sensor noise of variance
# a x + b on the Bayer mosaic, quantised to ``bits`` bits, before the fill -- made per batch, inside the patch kernel.
RAW_NOISE_TILE = (16, 64)     # a workgroup's rows and columns of the patch, in source orientation
RAW_NOISE_BITS = (8, 16)      # the smallest and the largest depth of the raw samples


def patch_raw_batch_ok(n_img: int, arena_elems: int, n: int, ph: int, pw: int) -> bool:
    """grr_patch_raw_batch_supported in plain Python (tests/test_raw_noise_abi.py checks the two agree): an RGB arena
    the arena entry points take, n, ph, pw >= 1, 3 n ph pw < 2^31 and a window (ph + 4)(pw + 4) < 2^31."""
    return image_arena_ok(3, n_img, arena_elems) and arena_elems >= 3 and n >= 1 and ph >= 1 and pw >= 1 \
        and 3 * n * ph * pw < (1 << 31) and (ph + 4) * (pw + 4) < (1 << 31)


def raw_noise_demosaic_ok(h: int, w: int) -> bool:
    """grr_u8_raw_noise_demosaic_supported in plain Python: sides >= 1, 3 H W < 2^31 and (H + 4)(W + 4) < 2^31."""
    return h >= 1 and w >= 1 and 3 * h * w < (1 << 31) and (h + 4) * (w + 4) < (1 << 31)


def _check_bits(name: str, bits) -> int:
    if isinstance(bits, (bool, np.bool_)) or not isinstance(bits, (int, np.integer)) \
            or not RAW_NOISE_BITS[0] <= bits <= RAW_NOISE_BITS[1]:
        raise ValueError(f"{name}: bits is an integer of {RAW_NOISE_BITS[0]}..{RAW_NOISE_BITS[1]}, got {bits!r}")
    return int(bits)


def _check_level(name: str, what: str, v, top: float) -> float:
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) \
            or not (np.isfinite(v) and 0 <= v <= top):
        raise ValueError(f"{name}: {what} is a number of 0..{top:g}, got {v!r}")
    return float(v)


def raw_noise_pair(name: str, shot, read) -> Tuple[float, float]:
    """The kernel's float32 noise pair (a, b) of a shot-noise gain ``shot`` (0..1) and a read-noise standard deviation
    ``read`` in 8-bit levels (0..255, as lambda_noise is): a = float32(shot), b = float32((read / 255)^2)."""
    shot, read = _check_level(name, "shot", shot, 1.0), _check_level(name, "read", read, 255.0)
    return float(np.float32(shot)), float(np.float32((read / 255.0) ** 2))


class PatchRawSource:
    """A uint8 RGB image pack that patch_raw_batch's checks have passed (patch_raw_source), with the Bayer code of
    every image as an int32 device tensor: the pack, its image count, the images' (H, W) as an int64 array, the
    device pattern list and its host copy."""
    __slots__ = ("pack", "n_img", "hw", "patterns", "host_patterns")

    def __init__(self, pack, n_img: int, hw, patterns: Tensor, host_patterns: tuple):
        self.pack, self.n_img, self.hw, self.patterns, self.host_patterns = pack, n_img, hw, patterns, host_patterns


def patch_raw_source(pack, patterns) -> PatchRawSource:
    """Check ``pack`` for patch_raw_batch (as patch_source checks its pack; 3 channels) and ``patterns`` -- one name
    or code for all images, or a sequence of one per image -- and return their PatchRawSource; the pattern list is
    uploaded once.  The pack's tensors and host table must not change afterwards."""
    name = "patch_raw_batch"
    n_img, c = _check_pack(name, pack, placed=False)
    if pack.arena.dtype != torch.uint8:
        raise ValueError(f"{name}: the arena must be uint8, got {pack.arena.dtype}")
    if c != 3:
        raise ValueError(f"{name}: a Bayer mosaic is made from R, G, B pictures, got {c} channel(s)")
    if isinstance(patterns, (str, int, np.integer)):
        patterns = [patterns] * n_img
    if len(patterns) != n_img:
        raise ValueError(f"{name}: {len(patterns)} patterns for {n_img} images")
    codes = tuple(_check_pattern(name, v) for v in patterns)
    _check_placed(name, pack)
    hw = np.asarray(pack.host_table, dtype=np.int64).reshape(n_img, 3)[:, 1:3].copy()
    return PatchRawSource(pack, n_img, hw, torch.tensor(codes, dtype=torch.int32).to(pack.arena.device), codes)


def patch_raw_batch(source: PatchRawSource, rows, sample_ids, noise, seed: int, ph: int, pw: int, fill="malvar",
                    bits: int = 16, clip: bool = True) -> Tuple[Tensor, Tensor]:
    """(target, input), float32 [n, 3, ph, pw] each, of a patch_raw_source: sample s is the ph x pw patch of image
    rows[s][0] at (rows[s][1], rows[s][2]) with a 2-pixel frame, continued outside the picture by the reflection that
    keeps the colour filter array's parity, sampled through the image's Bayer pattern, given noise of variance
    a x + b (``noise[s]`` = (a, b), float32 in [0, 1]; the normals are patch_batch's function of (seed,
    sample_ids[s], window element)), clipped to [0, 1] if ``clip``, quantised to ``bits`` bits, filled by ``fill`` and
    moved by T_mode (include/grr.h).  input is the filled picture, neither clamped nor rounded again; target the clean
    patch as float(v) / 255.  ``noise`` None: no noise, and no random number is computed.
    rows [n, 4], sample_ids [n] and noise [n, 2] are host data, checked here as patch_batch checks its own and
    uploaded; device tensors (int32 [n, 4], int64 [n], float32 [n, 2], contiguous, on the arena's device) are taken as
    they are: the kernel clamps what it reads from them."""
    name = "patch_raw_batch"
    if not isinstance(source, PatchRawSource):
        raise ValueError(f"{name}: source is what patch_raw_source returns")
    fill, bits = _check_fill(name, fill), _check_bits(name, bits)
    if not isinstance(clip, (bool, np.bool_)):
        raise ValueError(f"{name}: clip is True or False, got {clip!r}")
    arena = source.pack.arena
    on_device = isinstance(rows, Tensor) and rows.is_cuda
    n = int(rows.shape[0]) if on_device and rows.dim() == 2 else (len(rows) if hasattr(rows, "__len__") else 0)
    if isinstance(ph, int) and isinstance(pw, int) and min(ph, pw) >= 1 and (ph + 4) * (pw + 4) >= (1 << 31):
        raise ValueError(f"{name}: the window ({ph} + 4) x ({pw} + 4) must have fewer than 2^31 elements")
    if noise is not None:
        if on_device:
            if not isinstance(noise, Tensor) or noise.dtype != torch.float32 or tuple(noise.shape) != (n, 2) \
                    or noise.device != arena.device or not noise.is_contiguous():
                raise ValueError(f"{name}: a device noise table is float32 [n, 2] (a, b), contiguous and on the arena's "
                                 "device")
        else:
            noise = np.asarray(noise, dtype=np.float32)
            if noise.shape != (n, 2) or not (np.isfinite(noise).all() and (noise >= 0).all() and (noise <= 1).all()):
                raise ValueError(f"{name}: noise is [n, 2] rows (a, b) of [0, 1], one per row ({n})")
    table, ids, _ = _patch_tables(name, arena, source.n_img, 3, source.hw, rows, sample_ids, None, seed, ph, pw,
                                  no_sigma=True)
    if noise is not None and not on_device:
        noise = torch.from_numpy(np.ascontiguousarray(noise)).to(arena.device)
    return _patch_raw_batch(source, table, ids, noise, seed, ph, pw, fill, bits, bool(clip))


def _patch_raw_batch(source: PatchRawSource, table: Tensor, ids: Tensor, noise: Optional[Tensor], seed: int, ph: int,
                     pw: int, fill: int, bits: int, clip: bool) -> Tuple[Tensor, Tensor]:
    """patch_raw_batch after its checks, on device tables."""
    arena, n = source.pack.arena, table.shape[0]
    target = torch.empty((n, 3, ph, pw), dtype=torch.float32, device=arena.device)
    inp = torch.empty_like(target)
    _launch("patch_raw_batch", target.numel() * 8 + n * (ph + 4) * (pw + 4), "grr_patch_raw_batch", arena.data_ptr(),
            arena.numel(), source.pack.table.data_ptr(), source.n_img, source.patterns.data_ptr(), table.data_ptr(),
            ids.data_ptr(), None if noise is None else noise.data_ptr(), n, int(seed), ph, pw, fill, bits, int(clip),
            target.data_ptr(), inp.data_ptr(), _stream(arena.device))
    return target, inp


def u8_raw_noise_demosaic(img: Tensor, pattern, fill="malvar", a: float = 0.0, b: float = 0.0, bits: int = 16,
                          clip: bool = True, seed: int = 2204, sample_id: int = 0) -> Tensor:
    """The noisy Bayer mosaic of a uint8 H x W x 3 device picture, filled: float32 H x W x 3 (HWC), patch_raw_batch's
    input of the whole picture (row = col = 0, ph = H, pw = W, mode 0) up to layout.  ``a``, ``b``: the noise pair in
    [0, 1] (raw_noise_pair makes it from a shot gain and a read level); ``sample_id``: a 64-bit integer.  One launch.
    A non-contiguous image is copied first."""
    name = "u8_raw_noise_demosaic"
    pattern, fill, bits = _check_pattern(name, pattern), _check_fill(name, fill), _check_bits(name, bits)
    a, b = _check_level(name, "a", a, 1.0), _check_level(name, "b", b, 1.0)
    if not isinstance(clip, (bool, np.bool_)):
        raise ValueError(f"{name}: clip is True or False, got {clip!r}")
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed < (1 << 64):
        raise ValueError(f"{name}: seed must fit 64 bits, got {seed!r}")
    if isinstance(sample_id, bool) or not isinstance(sample_id, (int, np.integer)) or not -(1 << 63) <= sample_id < (1 << 63):
        raise ValueError(f"{name}: sample_id is a 64-bit integer, got {sample_id!r}")
    if isinstance(img, Tensor) and img.dtype != torch.uint8:
        raise ValueError(f"{name}: the image must be uint8, got {img.dtype}")
    if isinstance(img, Tensor) and img.dim() == 3 and img.shape[2] != 3:
        raise ValueError(f"{name}: needs 3 channels (R, G, B), got {tuple(img.shape)}")
    h, w, _ = _check_image(name, img)
    if not raw_noise_demosaic_ok(h, w):
        raise ValueError(f"{name}: needs 3 H W < 2^31 and (H + 4)(W + 4) < 2^31, got {tuple(img.shape)}")
    img = img.contiguous()
    out = torch.empty((h, w, 3), dtype=torch.float32, device=img.device)
    _launch("u8_raw_noise_demosaic", img.numel() + out.numel() * 4, "grr_u8_raw_noise_demosaic", img.data_ptr(), h, w,
            out.data_ptr(), pattern, fill, a, b, bits, int(clip), int(seed), int(sample_id), _stream(img.device))
    return out


# ---------------------------------------------------------------------------
# 2-D blur by an integer point-spread function (csrc/blur_ops.hip; include/grr.h has the definition): the degradation
# of deblurring.  A kernel is an int32 table of odd sides up to 31, non-negative, of sum 65536.
BLUR_TILE = (16, 64)          # a workgroup's rows and columns of the picture
BLUR_BOUNDARIES = ("wrap", "replicate", "reflect")        # the index is the code
MAX_BLUR_SIDE = 31            # GRR_BLUR_MAX_SIDE
BLUR_ONE = 65536              # GRR_BLUR_ONE
MAX_BLUR_KERNELS = 16         # grr_u8_blur_images: kernels per call
MAX_BLUR_IMAGES = 65535       # grr_u8_blur_images: one grid row per image


def blur_ok(c: int, h: int, w: int) -> bool:
    """grr_u8_blur_supported in plain Python (tests/test_blur_abi.py checks the two agree): 1..4 channels, sides
    >= 1, C H W < 2^31."""
    return 1 <= c <= 4 and h >= 1 and w >= 1 and c * h * w < (1 << 31)


def _check_boundary(name: str, boundary) -> int:
    """The code of a blur boundary given by name or code; ValueError otherwise."""
    return _check_code(name, "boundary", BLUR_BOUNDARIES, boundary)


def _check_blur_table(name: str, weights) -> np.ndarray:
    """A blur kernel's weight table as a contiguous int32 [kh, kw] array, the definition's conditions checked on the
    host: ``weights`` is that table (a 2-D integer array or host tensor) or a record with one as its ``table``
    (training.BlurKernel).  ValueError otherwise."""
    w = getattr(weights, "table", weights)
    if isinstance(w, Tensor):
        if w.is_cuda:
            raise ValueError(f"{name}: a blur kernel is a host table; it is checked before it is sent to the device")
        w = w.numpy()
    w = np.asarray(w)
    if w.ndim != 2 or w.dtype.kind not in "iu" or w.size == 0:
        raise ValueError(f"{name}: a blur kernel is a 2-D integer table, got {w.dtype} {w.shape}")
    if any(s % 2 == 0 or s > MAX_BLUR_SIDE for s in w.shape):
        raise ValueError(f"{name}: a blur kernel's sides are odd and at most {MAX_BLUR_SIDE}, got {w.shape}")
    w = w.astype(np.int64)
    if w.min() < 0 or int(w.sum()) != BLUR_ONE:
        raise ValueError(f"{name}: a blur kernel's weights are non-negative and sum to {BLUR_ONE} "
                         f"(got a minimum of {int(w.min())} and a sum of {int(w.sum())})")
    return np.ascontiguousarray(w, dtype=np.int32)


def u8_blur(img: Tensor, weights, boundary="wrap") -> Tensor:
    """The uint8 device image H x W x C (or H x W) convolved with a blur kernel in exact integers (include/grr.h).
    ``weights``: the int32 table (a 2-D host array of odd sides up to 31, non-negative, of sum 65536) or a
    training.BlurKernel; ``boundary``: "wrap" (circular), "replicate" or "reflect", or the code 0..2.  One launch.  A
    non-contiguous image is copied first."""
    name = "u8_blur"
    table, boundary = _check_blur_table(name, weights), _check_boundary(name, boundary)
    if isinstance(img, Tensor) and img.dtype != torch.uint8:
        raise ValueError(f"{name}: the image must be uint8, got {img.dtype}")
    flat = isinstance(img, Tensor) and img.dim() == 2
    if flat:
        img = img[:, :, None]
    h, w, c = _check_image(name, img)
    if not blur_ok(c, h, w):
        raise ValueError(f"{name}: needs 1..4 channels and H W C < 2^31, got {tuple(img.shape)}")
    img = img.contiguous()
    out = torch.empty_like(img)
    wd = torch.from_numpy(table).to(img.device)
    _launch("u8_blur", img.numel() + out.numel(), "grr_u8_blur", img.data_ptr(), h, w, c, out.data_ptr(),
            wd.data_ptr(), table.shape[0], table.shape[1], boundary, _stream(img.device))
    return out[:, :, 0] if flat else out


def u8_blur_images(pack, kernels, kernel_of, boundary="wrap"):
    """u8_blur of every image of a uint8 image pack into a new pack that shares its image table (so the two can form
    a patch_pair_source), one launch per 65535 images.  ``kernels``: one kernel or a sequence of at most 16 (tables or
    training.BlurKernel records, checked here); ``kernel_of``: the index into ``kernels`` of every image, one int for
    all, a sequence of one per image (checked here), or an int32 device tensor of one per image (which the kernel
    clamps into range, as it does every device table)."""
    from .restore import ImagePack
    name = "u8_blur_images"
    boundary = _check_boundary(name, boundary)
    if hasattr(kernels, "table") or isinstance(kernels, (np.ndarray, Tensor)):
        kernels = [kernels]
    if not 1 <= len(kernels) <= MAX_BLUR_KERNELS:
        raise ValueError(f"{name}: takes 1..{MAX_BLUR_KERNELS} kernels, got {len(kernels)}")
    tables = [_check_blur_table(name, k) for k in kernels]
    n_img, c = _check_pack(name, pack, placed=False)
    if pack.arena.dtype != torch.uint8:
        raise ValueError(f"{name}: the arena must be uint8, got {pack.arena.dtype}")
    shapes = [(int(h), int(w)) for _, h, w in pack.host_table]
    dev = pack.arena.device
    if not isinstance(kernel_of, Tensor):       # the host list is checked before anything is asked of the device
        if isinstance(kernel_of, (int, np.integer)):
            kernel_of = [kernel_of] * n_img
        if len(kernel_of) != n_img:
            raise ValueError(f"{name}: {len(kernel_of)} kernel indices for {n_img} images")
        for v in kernel_of:
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not 0 <= v < len(tables):
                raise ValueError(f"{name}: a kernel index is an integer of 0..{len(tables) - 1}, got {v!r}")
    _check_placed(name, pack)
    if isinstance(kernel_of, Tensor):
        if kernel_of.dtype != torch.int32 or tuple(kernel_of.shape) != (n_img,) or kernel_of.device != dev \
                or not kernel_of.is_contiguous():
            raise ValueError(f"{name}: a kernel-index tensor is int32 [{n_img}], contiguous and on the arena's device")
        of = kernel_of
    else:
        of = torch.tensor([int(v) for v in kernel_of], dtype=torch.int32).to(dev)
    slots = np.zeros((len(tables), MAX_BLUR_SIDE, MAX_BLUR_SIDE), np.int32)
    for slot, t in zip(slots, tables):
        slot[:t.shape[0], :t.shape[1]] = t
    weights = torch.from_numpy(slots).to(dev)
    sizes = torch.tensor([t.shape for t in tables], dtype=torch.int32).to(dev)
    covered = sum(h * w * c for h, w in shapes) == pack.arena.numel()
    arena = (torch.empty_like if covered else torch.zeros_like)(pack.arena)      # bytes between images stay 0
    for at in range(0, n_img, MAX_BLUR_IMAGES):
        n = min(MAX_BLUR_IMAGES, n_img - at)
        part = shapes[at:at + n]
        _launch("u8_blur_images", 2 * sum(h * w * c for h, w in part), "grr_u8_blur_images", pack.arena.data_ptr(),
                pack.arena.numel(), pack.table.data_ptr() + at * 24, n, max(h for h, _ in part),
                max(w for _, w in part), c, arena.data_ptr(), weights.data_ptr(), sizes.data_ptr(), len(tables),
                of.data_ptr() + at * 4, boundary, _stream(dev))
    return ImagePack(arena, pack.table, tuple(tuple(int(v) for v in row) for row in pack.host_table), c,
                     tuple(getattr(pack, "kinds", ())))


# ---------------------------------------------------------------------------
# Inpainting (csrc/inpaint_ops.hip; include/grr.h has the definition): a Bernoulli mask that is a function of (seed,
# sample id, window element), or a given one, and the initial fill of the missing pixels -- zero, or a normalised
# convolution of the known ones under a uint8 weight table -- made per batch, inside the patch kernel.
MASK_TILE = (16, 64)          # a workgroup's rows and columns of the patch, in source orientation
MASK_FILLS = ("zero", "conv")                             # the index is the code
MASK_HALO = 7                 # GRR_MASK_HALO
MAX_MASK_SIDE = 15            # GRR_MASK_MAX_SIDE
MASK_ONE = 1 << 24            # GRR_MASK_ONE


def patch_mask_batch_ok(c: int, n_img: int, arena_elems: int, n: int, ph: int, pw: int) -> bool:
    """grr_patch_mask_batch_supported in plain Python (tests/test_inpaint_abi.py checks the two agree): what
    patch_batch takes, and a window (ph + 14)(pw + 14) < 2^31."""
    return patch_batch_ok(c, n_img, arena_elems, n, ph, pw) and (ph + 14) * (pw + 14) < (1 << 31)


def mask_fill_ok(c: int, h: int, w: int) -> bool:
    """grr_u8_mask_fill_supported in plain Python: 1..4 channels, sides >= 1, C H W < 2^31 and (H + 14)(W + 14) < 2^31."""
    return image_io_ok(c, h, w) and (h + 14) * (w + 14) < (1 << 31)


def keep_units(fraction) -> int:
    """The known share ``fraction`` of [0, 1] in the kernel's units of 2^-24: round(fraction 2^24)."""
    if isinstance(fraction, (bool, np.bool_)) or not isinstance(fraction, (int, float, np.integer, np.floating)) \
            or not (np.isfinite(fraction) and 0 <= fraction <= 1):
        raise ValueError(f"keep_units: the known share is a number of 0..1, got {fraction!r}")
    return int(round(float(fraction) * MASK_ONE))


def mask_weights(side, sigma=None) -> np.ndarray:
    """The uint8 weight table of the conv fill, ``side`` x ``side`` (or (kh, kw)), odd and at most 15:
    round(255 exp(-d^2 / (2 sigma^2))) with d the distance to the centre, made in float64 on the host; ``sigma`` None
    gives a flat table of 255.  The table is data handed to the kernel: the fill itself is exact integers."""
    sides = tuple(side) if isinstance(side, (list, tuple)) else (side, side)
    if len(sides) != 2 or any(isinstance(s, (bool, np.bool_)) or not isinstance(s, (int, np.integer)) or s < 1
                              or s > MAX_MASK_SIDE or s % 2 == 0 for s in sides):
        raise ValueError(f"mask_weights: a weight table's sides are odd and lie in 1..{MAX_MASK_SIDE}, got {side!r}")
    kh, kw = int(sides[0]), int(sides[1])
    if sigma is None:
        return np.full((kh, kw), 255, np.uint8)
    if isinstance(sigma, (bool, np.bool_)) or not isinstance(sigma, (int, float, np.integer, np.floating)) \
            or not (np.isfinite(sigma) and sigma > 0):
        raise ValueError(f"mask_weights: sigma is a positive number or None, got {sigma!r}")
    y, x = np.meshgrid(np.arange(kh, dtype=np.float64) - kh // 2, np.arange(kw, dtype=np.float64) - kw // 2, indexing="ij")
    return np.round(255.0 * np.exp(-(y * y + x * x) / (2.0 * float(sigma) ** 2))).astype(np.uint8)


def _check_mask_fill(name: str, fill) -> int:
    """The code of a mask fill given by name or code; ValueError otherwise."""
    return _check_code(name, "fill", MASK_FILLS, fill)


def _check_mask_table(name: str, weights) -> np.ndarray:
    """A conv fill's weight table as a contiguous uint8 [kh, kw] host array; ValueError otherwise."""
    w = weights
    if isinstance(w, Tensor):
        if w.is_cuda:
            raise ValueError(f"{name}: a weight table is a host table; it is checked before it is sent to the device")
        w = w.numpy()
    w = np.asarray(w)
    if w.ndim != 2 or w.dtype != np.uint8 or w.size == 0:
        raise ValueError(f"{name}: a weight table is a 2-D uint8 table, got {w.dtype} {w.shape}")
    if any(s % 2 == 0 or s > MAX_MASK_SIDE for s in w.shape):
        raise ValueError(f"{name}: a weight table's sides are odd and at most {MAX_MASK_SIDE}, got {w.shape}")
    return np.ascontiguousarray(w)


def _check_hole(name: str, hole) -> int:
    if isinstance(hole, (bool, np.bool_)) or not isinstance(hole, (int, np.integer)) or not 0 <= hole <= 255:
        raise ValueError(f"{name}: the hole is an integer of 0..255, got {hole!r}")
    return int(hole)


def _mask_call_args(name: str, weights, fill, hole) -> Tuple[np.ndarray, int, int]:
    """(table, fill code, hole) of a call, checked; ``weights`` None: the flat 7 x 7 table (the zero fill reads none)."""
    fill, hole = _check_mask_fill(name, fill), _check_hole(name, hole)
    table = _check_mask_table(name, mask_weights(7) if weights is None else weights)
    return table, fill, hole


def patch_mask_batch(pack, rows, sample_ids, keep, seed: int, ph: int, pw: int, weights=None, fill="conv",
                     hole: int = 128, with_mask: bool = True):
    """(target, input, mask) of a uint8 ``pack`` (or the PatchSource that patch_source made of it): sample s is
    patch_batch's clean patch of rows[s] as target; input is the same patch with a pixel known with probability
    keep[s] / 2^24 -- a bit that is a function of (seed, sample_ids[s], window element) alone -- and the missing ones
    filled by ``fill``: "zero", or "conv", the normalised convolution of the known pixels under the uint8 table
    ``weights`` (odd sides up to 15; None: flat 7 x 7), ``hole`` where no known pixel lies under the table
    (include/grr.h).  target and input are float32 [n, C, ph, pw]; mask is float32 [n, 1, ph, pw], 1 known and 0
    missing, or None without ``with_mask``.
    rows [n, 4], sample_ids [n] and keep [n] (integers, units of 2^-24; keep_units makes one from a fraction) are host
    data, checked here as patch_batch checks its own and uploaded; device tensors (int32 [n, 4], int64 [n], int32 [n],
    contiguous, on the arena's device) are taken as they are: the kernel clamps what it reads from them."""
    name = "patch_mask_batch"
    table, fill, hole = _mask_call_args(name, weights, fill, hole)
    src = pack if isinstance(pack, PatchSource) else patch_source(pack)
    arena = src.pack.arena
    on_device = isinstance(rows, Tensor) and rows.is_cuda
    n = int(rows.shape[0]) if on_device and rows.dim() == 2 else (len(rows) if hasattr(rows, "__len__") else 0)
    if isinstance(ph, int) and isinstance(pw, int) and min(ph, pw) >= 1 and (ph + 14) * (pw + 14) >= (1 << 31):
        raise ValueError(f"{name}: the window ({ph} + 14) x ({pw} + 14) must have fewer than 2^31 elements")
    if on_device:
        if not isinstance(keep, Tensor) or keep.dtype != torch.int32 or tuple(keep.shape) != (n,) \
                or keep.device != arena.device or not keep.is_contiguous():
            raise ValueError(f"{name}: a device keep list is int32 [n], contiguous and on the arena's device")
    else:
        keep = np.asarray(keep)
        if keep.shape != (n,) or keep.dtype.kind not in "iu" or (keep.astype(np.int64) < 0).any() \
                or (keep.astype(np.int64) > MASK_ONE).any():
            raise ValueError(f"{name}: keep is integers of 0..2^24, one per row ({n})")
    tab, ids, _ = _patch_tables(name, arena, src.n_img, src.c, src.hw, rows, sample_ids, None, seed, ph, pw, no_sigma=True)
    if not on_device:
        keep = torch.from_numpy(np.ascontiguousarray(keep.astype(np.int32))).to(arena.device)
    wd = torch.from_numpy(table).to(arena.device)
    return _patch_mask_batch(src, tab, ids, keep, seed, ph, pw, wd, table.shape, fill, hole, bool(with_mask))


def _patch_mask_batch(src: PatchSource, table: Tensor, ids: Tensor, keep: Tensor, seed: int, ph: int, pw: int,
                      weights: Tensor, sides, fill: int, hole: int, with_mask: bool):
    """patch_mask_batch after its checks, on device tables; ``weights``: the uint8 device table of ``sides``."""
    arena, n, c = src.pack.arena, table.shape[0], src.c
    target = torch.empty((n, c, ph, pw), dtype=torch.float32, device=arena.device)
    inp = torch.empty_like(target)
    mask = torch.empty((n, 1, ph, pw), dtype=torch.float32, device=arena.device) if with_mask else None
    _launch("patch_mask_batch", target.numel() * 8 + (mask.numel() * 4 if with_mask else 0) + n * c * (ph + 14) * (pw + 14),
            "grr_patch_mask_batch", arena.data_ptr(), arena.numel(), c, src.pack.table.data_ptr(), src.n_img,
            table.data_ptr(), ids.data_ptr(), keep.data_ptr(), n, int(seed), ph, pw, weights.data_ptr(), int(sides[0]),
            int(sides[1]), fill, hole, target.data_ptr(), inp.data_ptr(), mask.data_ptr() if with_mask else None,
            _stream(arena.device))
    return target, inp, mask


def u8_mask_fill(img: Tensor, mask: Optional[Tensor] = None, keep: int = MASK_ONE, weights=None, fill="conv",
                 hole: int = 128, seed: int = 2204, sample_id: int = 0) -> Tuple[Tensor, Tensor]:
    """(filled, mask_out) of a uint8 H x W x C device picture: the missing pixels filled as patch_mask_batch fills
    them, one launch.  ``mask``: a uint8 H x W device tensor, nonzero known (read by the mirror outside the picture),
    or None: the mask of (seed, sample_id) is drawn with the share ``keep`` (units of 2^-24), patch_mask_batch's mask
    of the whole picture for the same id.  mask_out (uint8 H x W) carries ``mask``'s nonzero values through (1 for a
    drawn known pixel), is 2 where this call filled a pixel from at least one known one and 0 where a hole is left:
    feeding both results back in is a second pass, which grows the filled region by one table radius.  A
    non-contiguous picture or mask is copied first."""
    name = "u8_mask_fill"
    table, fill, hole = _mask_call_args(name, weights, fill, hole)
    if isinstance(keep, (bool, np.bool_)) or not isinstance(keep, (int, np.integer)) or not 0 <= keep <= MASK_ONE:
        raise ValueError(f"{name}: keep is an integer of 0..2^24, got {keep!r}")
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed < (1 << 64):
        raise ValueError(f"{name}: seed must fit 64 bits, got {seed!r}")
    if isinstance(sample_id, bool) or not isinstance(sample_id, (int, np.integer)) or not -(1 << 63) <= sample_id < (1 << 63):
        raise ValueError(f"{name}: sample_id is a 64-bit integer, got {sample_id!r}")
    if isinstance(img, Tensor) and img.dtype != torch.uint8:
        raise ValueError(f"{name}: the image must be uint8, got {img.dtype}")
    if mask is not None and (not isinstance(mask, Tensor) or mask.dtype != torch.uint8 or mask.dim() != 2
                             or not isinstance(img, Tensor) or tuple(mask.shape) != tuple(img.shape[:2])):
        raise ValueError(f"{name}: a mask is a uint8 H x W tensor of the picture's sides, got "
                         f"{getattr(mask, 'dtype', None)} {tuple(getattr(mask, 'shape', ()))}")
    h, w, c = _check_image(name, img)
    if mask is not None and mask.device != img.device:
        raise ValueError(f"{name}: the mask must be on the picture's device")
    if not mask_fill_ok(c, h, w):
        raise ValueError(f"{name}: needs H W C < 2^31 and (H + 14)(W + 14) < 2^31, got {tuple(img.shape)}")
    img = img.contiguous()
    mask = None if mask is None else mask.contiguous()
    out = torch.empty_like(img)
    mask_out = torch.empty((h, w), dtype=torch.uint8, device=img.device)
    wd = torch.from_numpy(table).to(img.device)
    _launch("u8_mask_fill", 2 * img.numel() + 2 * h * w, "grr_u8_mask_fill", img.data_ptr(),
            None if mask is None else mask.data_ptr(), h, w, c, int(keep), int(seed), int(sample_id), wd.data_ptr(),
            table.shape[0], table.shape[1], fill, hole, out.data_ptr(), mask_out.data_ptr(), _stream(img.device))
    return out, mask_out
