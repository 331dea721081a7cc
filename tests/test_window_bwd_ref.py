"""CPU checks that the case table, references and bounds of tests/window_bwd_ref.py have teeth, from the inputs alone
(no kernel): the table reaches every window and family with every term, signal-channel count and frame, and the
strided cases reach a second grid-stride sweep in every launch geometry of csrc/window_bwd.hip; every prox case
meets the kink rule with no edge excluded; the reverse written out on slices is the oracle's autograd in float64;
ref32 is inside bound / 4 and every other honest fp32 order tried (the reverse edge order, the gather form both
ways, the E-planes path's running sum on the tiny frames) inside the bound; every emulated mutant is >= 2 x bound
outside on every case it applies to."""
import pytest
import torch

from tests import window_bwd_ref as B
from tests.window_ref import _S, _St


def test_term_table_covers_every_window_term_fs_and_frame():
    cs = B.TERM_CASES
    assert len(set(B.TERM_IDS)) == len(cs) and len({c.seed for c in cs + B.STRIDED_CASES}) == len(cs) + 6
    assert {(c.window, c.term) for c in cs} == {(w, t) for w in B.WINDOWS for t in B.TERMS}
    assert {(B.family(c.window), c.term) for c in cs} == {(f, t) for f in B.FAMILIES for t in B.TERMS}
    assert {c.fs for c in cs} == {1, 2, 3} and {c.g for c in cs} == {2, 3}
    assert {c.hw for c in cs} == set(B.FRAMES)
    assert B.FRAMES == ((2, 2), (3, 2), (2, 5), (4, 3), (2, 700), (17, 65), (33, 130))
    for t in B.TERMS:
        assert {c.fs for c in cs if c.term == t} == {1, 2, 3}, t
    prox = [c for c in cs if c.term == "prox"]
    assert all(c.hw[0] * c.hw[1] >= 10 for c in prox)
    assert {c.hw for c in prox} == {f for f in B.FRAMES if f[0] * f[1] >= 10}
    # reach 2 on axes of 3 and 4 pixels (clamp_sources mixes an inside source with folded ones), and a long thin frame
    assert any(c.hw == (4, 3) and B.family(c.window).startswith("r2") for c in cs)
    assert any(c.hw == (2, 700) and B.plane_blocks(c.hw, c.b * c.g) > 1 for c in cs)
    assert all(B.sweeps_of(c.hw, c.b * c.g) == 1 for c in cs)       # the second sweep is the strided cases' business


def test_strided_cases_reach_a_second_sweep_in_every_launch_geometry():
    # what training runs (multiblocks_v7.yaml: B = 16, G = 24, 64 x 64): 10 blocks per plane, two sweeps
    assert B.plane_blocks((64, 64), 384) == 10 and B.sweeps_of((64, 64), 384) == 2
    assert {(c.window, c.term) for c in B.STRIDED_CASES} == {(w, t) for w in ("cross4", "ring3") for t in B.TERMS}
    for c in B.STRIDED_CASES:
        planes = c.b * c.g
        assert planes == 1024 and c.hw == (33, 33) and c.fs == 1
        assert (c.b, c.g) == ((4, 256) if c.term == "prox" else (128, 8))
        assert B.plane_blocks(c.hw, planes) == 4 and B.first_sweep(c.hw, planes) == 1024
        assert B.sweeps_of(c.hw, planes) == 2 and 33 * 33 - 1024 == 65          # one wave and one lane
    n = 128 * 8 * 33 * 33
    assert n == 1115136 and B.red_first_sweep(n) == 1048576 < n                 # grid_red strides as well
    assert B.TAPGRAD_CASES[-1] == ((33, 33), 128, 8, 1)
    assert [(c.b, c.g, c.f, c.hw) for c in B.STRIDED_EDGE_CASES] == [(128, 8, 3, (33, 33))] * 2
    nn = 1
    for v in B.GRID1D_SHAPE:
        nn *= v
    assert B.grid1d_first_sweep(nn) == 16777216 < nn <= 16777216 + B.GRID1D_SHAPE[-1] * B.GRID1D_SHAPE[-2]


def test_edge_stencil_and_tapgrad_tables():
    assert {c.f for c in B.EDGE_CASES} == {1, 4, 5, 12, 13, 24}
    assert {c.offset for c in B.EDGE_CASES} == {0, 3} and all(c.extra > 0 for c in B.EDGE_CASES)
    assert {c.window for c in B.EDGE_CASES} == set(B.WINDOWS)
    assert {c.offset for c in B.EDGE_CASES if c.f in (4, 12, 13)} == {3}
    assert B.STENCIL_FRAMES == ((2, 2), (2, 3), (3, 4), (17, 65))
    assert any(B.plane_blocks(c.hw, c.b * c.g) > 1 for c in B.EDGE_CASES)


@pytest.mark.parametrize("case", [c for c in B.TERM_CASES + B.STRIDED_CASES if c.term == "prox"],
                         ids=lambda c: B.term_id(c))
def test_prox_cases_meet_the_kink_rule(case):
    k = B.kink(case)
    margin = float((k.half_gap / k.rounding).min())
    print(f"{B.term_id(case)}: half gap / rounding bound {margin:.1f}, smallest branch {float(k.fractions.min()):.3f}")
    assert margin >= B.KINK_MARGIN
    assert k.fractions.shape == (case.b * case.g * case.fs, 3)
    assert float(k.fractions.min()) >= B.MIN_BRANCH, k.fractions
    assert len(set(B.term_inputs(case).log_gamma.tolist())) == case.g          # the graphs differ


@pytest.mark.parametrize("case", B.TERM_CASES + B.STRIDED_CASES, ids=B.TERM_IDS + B.STRIDED_IDS)
def test_term_references_agree_and_ref32_is_fp32_accurate(case):
    """The reverse written out on slices (what the mutants alter) is the oracle's autograd to rounding; ref32 is
    within fp32 rounding on every plane; the reverse edge order in fp32 stays inside the bound."""
    r = B.term_refs(case)
    ex = B.term_explicit(case)
    assert set(r.out64) == {"y", "gs", "gw", "gdot"} | ({"ggamma"} if case.term == "prox" else set())
    for n, v in r.out64.items():
        assert float((ex[n] - v).abs().max()) <= 1e-12 * float(v.abs().max()), n
    inp = r.inp
    assert tuple(r.out64["gw"].shape) == tuple(inp.w.shape) and tuple(r.out64["gdot"].shape) == (case.g,)
    assert len(set(inp.sc[:8].tolist())) == min(case.g, 8) and float(inp.sc[1]) < 0.1      # cycling beyond 8 graphs
    for n in B.TERM_DIMS:
        assert float(r.err32[n].max()) <= 2e-6, (n, r.err32[n].max())
    own = B.term_ratios(case, B.as_got(case, B._term32(case)))
    assert max(own.values()) <= 0.25
    # further honest fp32 evaluations stay inside the bound, or the draw is ill-conditioned and is replaced: the
    # reverse edge order, the gather form (the kernels' own formulation) in both edge orders, and on the tiny frames
    # the E-planes path's running sum in the kernel's order
    alts = {"reverse": B._term32(case, reverse=True), "gather": B.gather32(case),
            "gather reverse": B.gather32(case, reverse=True)}
    if case.hw[0] * case.hw[1] <= B.SEQ_PIXELS:
        alts["running sum"] = {"y": r.out64["y"], "gw": r.out64["gw"], "gs": B.seq_gather32(case)}
    worst = {k: max(B.term_ratios(case, B.as_got(case, ev)).values()) for k, ev in alts.items()}
    print(f"{B.term_id(case)}: other fp32 orders, worst err / bound " + "  ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst
    exr = B.term_explicit(case, reverse=True)
    for n, v in r.out64.items():
        assert float((exr[n] - v).abs().max()) <= 1e-12 * float(v.abs().max()), n
    # the exact sums are inside their own bound by a wide margin, pre-fill included
    sums = B.term_ratios(case, B.as_got(case, ex))
    assert sums["gdot"] <= 1e-6 and sums.get("ggamma", 0.0) <= 1e-6


@pytest.mark.parametrize("m", ["a", "b", "c", "d", "e"])
def test_term_mutants_are_outside_the_bound(m):
    cases = [c for c in B.TERM_CASES if B.term_mutant_applies(c, m)]
    assert {B.family(c.window) for c in cases} == set(B.FAMILIES) - ({"r1k0"} if m in "bc" else set())
    # where a mutant cannot apply is recorded (window_bwd_ref's docstring), as window_ref records its mutant b on cross4
    missing = {c.window for c in B.TERM_CASES} - {c.window for c in cases}
    assert missing == {"b": {"cross4", "plus8"}, "c": {"cross4"}}.get(m, set())
    worst = []
    for c in cases:
        r = B.term_ratios(c, B.as_got(c, B.term_explicit(c, m)))
        seen = {"a": ("gs",), "b": ("gs",), "c": ("gs", "gw", "gdot", "ggamma"), "d": ("gs", "gw"), "e": ("ggamma",)}[m]
        worst.append(max(r[n] for n in seen if n in r))
        assert worst[-1] >= 2.0, (B.term_id(c), r)
        assert all(v <= 1e-6 for n, v in r.items() if n not in seen), (B.term_id(c), r)
    print(f"mutant {m}: {len(cases)} cases, smallest worst err / bound {min(worst):.3g}")


@pytest.mark.parametrize("case", B.STRIDED_CASES, ids=B.STRIDED_IDS)
def test_mutant_h_a_lost_second_sweep_is_outside_the_bound(case):
    assert not any(B.term_mutant_applies(c, "h") for c in B.TERM_CASES)        # one sweep: nothing to lose
    r = B.term_ratios(case, B.as_got(case, B.term_explicit(case, "h")))
    print(f"{B.term_id(case)}: " + "  ".join(f"{n} {v:.3g}" for n, v in r.items()))
    assert r["gw"] >= 2.0 and r["gdot"] >= 2.0 and r.get("ggamma", 2.0) >= 2.0, r
    assert r["y"] <= 1e-6 and r["gs"] <= 1e-6


@pytest.mark.parametrize("hw", B.STENCIL_FRAMES)
def test_stencil_adjoints_and_mutant_f(hw):
    r = B.stencil_refs(hw)
    x = r.x.double().requires_grad_(True)
    g = torch.randn(x.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    t = r.taps.double()
    (adj_p,) = torch.autograd.grad((g * _S(x, t)).sum(), x)
    (adj_t,) = torch.autograd.grad((g * _St(x, t)).sum(), x)
    assert float((B.stencil_eval(g, t, 2) - adj_p).abs().max()) <= 1e-13
    assert float((B.stencil_eval(g, t, 1) - adj_t).abs().max()) <= 1e-13
    for mode in B.STENCIL_MODES:
        assert float(r.bound[mode].max()) <= 2e-6 and float(r.bound_s[mode].max()) <= 2e-6
    mut = B.stencil_eval(r.x.double(), t, 2, mutant="f")
    worst = B.ratio(mut, r.y64[2], r.bound[2], (-2, -1))
    per_plane = B.plane_err(mut, r.y64[2]) / r.bound[2]
    print(f"mutant f on {hw}: err / bound {worst:.3g}")
    assert float(per_plane.min()) >= 2.0


@pytest.mark.parametrize("case", B.TAPGRAD_CASES, ids=B.TAPGRAD_IDS)
def test_tapgrad_mutants_g_and_h(case):
    r = B.tapgrad_refs(*case)
    for ws in (True, False):
        d = (B.tapgrad_mutant(*case, 1, ws, "g") - r.gt[1, ws]).abs() / r.bound[1, ws]
        assert float(d[0]) == 0.0 and float(d[1:].min()) >= 2.0, d          # the centre tap has d = 0
        if case[0] == B.STRIDED_HW:
            for mode in (0, 1):
                dh = (B.tapgrad_mutant(*case, mode, ws, "h") - r.gt[mode, ws]).abs() / r.bound[mode, ws]
                assert float(dh.min()) >= 2.0, dh


@pytest.mark.parametrize("case", B.EDGE_CASES, ids=B.edge_id)
def test_edge_references(case):
    e = B.edge_refs(case)             # asserts the slice-wise float64 forward against the oracle's autograd itself
    zb, zg, zy, zx = e.zero
    assert float(e.feat[zb, case.offset:case.offset + case.f, zy, zx].abs().max()) == 0.0
    if case.f > 1:
        assert float(e.bound.max()) <= 2e-5, e.bound.max()
    assert float(e.bound_zero) <= 2e-5
    assert float(e.gf64[zb, zg, :, zy, zx].abs().max()) >= 1e6         # gn / 1e-12: the zero vector is held on its own
    # the float64 reference as a call's result is inside every bound; the pre-fill alone is not
    gfeat = e.gfeat_pre.double().clone()
    lo = case.offset
    gfeat[:, lo:lo + case.g * case.f] += e.gf64.reshape(case.b, -1, *case.hw)
    r = B.edge_ratios(case, gfeat.float(), (e.gM_pre.double() + e.gM64).float())
    assert max(r.values()) <= 1.0, r
    assert ("gfeat" in r) == (case.f > 1) and "unproj" in r
    # a second honest fp32 evaluation (every chain reversed) stays inside the bound
    alt = B.edge_ratios(case, B.edge_alt32(case), (e.gM_pre.double() + e.gM64).float())
    print(f"{B.edge_id(case)}: reversed chains in fp32 " + "  ".join(f"{n} {v:.2f}" for n, v in alt.items()))
    assert max(alt.values()) <= 1.0, alt
    r0 = B.edge_ratios(case, e.gfeat_pre, e.gM_pre)
    assert r0["gM"] >= 2.0 and r0["gfeat_zero"] >= 2.0 and r0["outside"] == 0.0
    assert r0.get("gfeat", 2.0) >= 2.0, r0
    touched = e.gfeat_pre.clone()
    touched[0, -1, 0, 0] += 1e-6
    assert B.edge_ratios(case, touched, e.gM_pre)["outside"] == float("inf")


@pytest.mark.parametrize("case", B.STRIDED_EDGE_CASES, ids=B.edge_id)
def test_edge_mutant_h(case):
    e = B.edge_refs(case)
    alt = B.edge_ratios(case, B.edge_alt32(case), (e.gM_pre.double() + e.gM64).float())
    print(f"{B.edge_id(case)}: reversed chains in fp32 " + "  ".join(f"{n} {v:.2f}" for n, v in alt.items()))
    assert max(alt.values()) <= 1.0, alt
    gfeat, gM = B.edge_mutant_h(case)
    r = B.edge_ratios(case, gfeat, gM)
    print(f"{B.edge_id(case)}: mutant h " + "  ".join(f"{n} {v:.3g}" for n, v in r.items()))
    assert r["gfeat"] >= 2.0 and r["gM"] >= 2.0 and r["outside"] == 0.0


def test_mix_references():
    for m in B.MIX_CASES:
        r = B.mix_refs(*m)
        assert float(r.bound_gx.max()) <= 5e-7 and float(r.bound_gscore.max()) <= 2e-6
