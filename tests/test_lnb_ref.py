"""CPU checks that the measures and bounds of tests/lnb_ref.py have teeth, from the inputs alone (two images per
case, no kernel): the fixed-order fp32 evaluation is the block; what the two-term fp16 split of either GEMM
loses sits inside bound / 4 on every measure; a whole dropped product is >= 2 x bound on err_max; a product
dropped in one chunk of one tile, a whole chunk of one tile, a product dropped in the smallest W2 row or at
the pixels that do not dominate the max-norm is >= 2 x bound on the measure meant to see it -- and below the
bound of the older tests' measure (err_max of the output with skip = (0.7, 1.4)), which is the hole closed."""
import pytest
import torch

from tests import lnb_ref as L
from tests.gemm_ref import dot32


def _fmt(e, bound):
    return "  ".join(f"{k} {v:.2e} ({v / bound[k]:.2f} x bound)" for k, v in e.items())


def test_cases_reach_every_instance_and_the_image_has_partial_tiles():
    assert [-(-c.c // 16) for c in L.CASES] == [1, 2, 3, 4, 5, 6]                 # KS
    assert [-(-c.c // 32) for c in L.CASES] == [1, 1, 2, 2, 3, 3]                 # MT
    assert [-(-c.hid // 16) for c in L.CASES] == [1, 2, 3, 4, 3, 16]              # nch
    assert (L.TILES_Y, L.TILES_X, L.TILES) == (3, 3, 9)
    assert L.W - (L.TILES_X - 1) * L.TILE_W == 6 and L.H - (L.TILES_Y - 1) * L.TILE_H == 4


@pytest.mark.parametrize("case", L.CASES, ids=L.IDS)
def test_inputs_are_per_image_and_carry_their_edges(case):
    x2, gray2, p = L.inputs(case, 2)
    x3, gray3, _ = L.inputs(case, 3)
    assert torch.equal(x3[:2], x2) and torch.equal(gray3[:2], gray2)
    frac = float(gray2.float().mean())
    assert 0.015 <= frac <= 0.04, frac
    for b in range(2):
        g = x2[b][:, gray2[b]]
        assert bool((g == g[:1]).all()) and float(g.abs().max()) <= 4.0 * (64.0 if b else 1.0)
        assert bool((g * 8 == (g * 8).round()).all()) and bool((g != 0).all())     # exact fp32 statistics
        xs = L.xs32(x2[b:b + 1])[0][:, gray2[b]]
        assert torch.equal(xs, (g.double() / torch.tensor(L.EPS, dtype=torch.float64).sqrt().float().double()).float())
        assert not bool(gray2[b, 16:, 64:].any())                                # the mutants' tile
        assert not bool((gray2[b, :, 1:] & gray2[b, :, :-1]).any()) and not bool((gray2[b, 1:] & gray2[b, :-1]).any())
    ratio = p.w2.abs().amax(1)
    assert float(ratio.max() / ratio.min()) >= 2.0 ** 12                         # W2 rows span 2^15 (C = 6) ... 2^18
    # both exponent paths fire: pixels off the common 2^10 of GEMM1's x operand, and a spread of GEMM2 exponents
    r = L.refs(case)
    em = L.emulation(case)
    assert int((em.e1p != 10).sum()) >= int(r.gray.sum()) // 2
    assert int(em.e2p.max() - em.e2p.min()) >= 24


def test_split2_is_exact_and_its_terms_are_fp16():
    v = torch.randn(4096, generator=torch.Generator().manual_seed(1)) * 3.0
    e = L.scale_exp(v.abs().max().reshape(1))
    t = L.split2(v, e)
    assert torch.equal(t.float().half().double(), t)
    vs = torch.ldexp(v, e.expand_as(v)).double()
    assert 2.0 ** 13 <= float(vs.abs().max()) < 2.0 ** 14
    assert torch.equal(t[0], vs.float().half().double())
    big = vs.abs() >= 1.0                                    # lo stays a normal fp16 number
    assert float(((vs - t.sum(0)).abs() / vs.abs())[big].max()) <= 2.0 ** -22
    assert float((t[1].abs() / vs.abs())[big].max()) <= 2.0 ** -11


@pytest.mark.parametrize("case", L.CASES[:2], ids=L.IDS[:2])
def test_all_four_products_are_the_product_of_the_fp32_operands(case):
    em, r = L.emulation(case), L.refs(case)
    """With lo.lo added only the terms' own rounding is left: <= 2^-22 |v| per operand (an fp16 term rounds to
    2^-11 of itself), doubled by the quadratic gate."""
    four = tuple((i, j) for i in range(2) for j in range(2))
    for stage in ("gemm1", "gemm2"):
        e = L.errors(em.o(stage, four), em.full(stage), r.sc)
        assert max(e.values()) <= 2.0 ** -20, (stage, e)


@pytest.mark.parametrize("case", L.CASES, ids=L.IDS)
def test_fp32_evaluation_is_the_block_at_fp32_accuracy(case):
    """A wrong fp32 evaluation would only loosen the bounds: it is within fp32 rounding of float64 on every
    measure, its GEMMs are dot32's, and float64 is the oracle's local_nonlinear_block."""
    from oracle import graph_oracle as O
    r = L.refs(case)
    assert all(t.dtype == torch.float32 for t in r.s32)
    assert max(r.err32.values()) <= 3e-6 and r.gate32 <= 6e-6, (r.err32, r.gate32)
    n = r.s32.n[0].reshape(case.c, -1)
    assert torch.equal(dot32(r.p.w1, n).reshape(r.s32.h[0].shape), r.s32.h[0])
    hid = case.hid
    sd = {"norm.weighted_transform.weight": r.p.ln_w.double().reshape(-1, 1, 1, 1),
          "local_linear.channels_linear_op.weight": r.p.w1.double().reshape(2 * hid, case.c, 1, 1),
          "local_linear.channels_local_linear_op.weight": r.p.wdw.double().reshape(2 * hid, 1, 3, 3),
          "local_linear.project_out.weight": r.p.w2.double().reshape(case.c, hid, 1, 1),
          "skip_weight": torch.tensor([0.0, 1.0], dtype=torch.float64)}
    ref = O.local_nonlinear_block(r.x.double(), sd, "")
    assert L.rel_err(r.s64.o, ref) <= 1e-13


@pytest.mark.parametrize("stage", ["gemm1", "gemm2"])
@pytest.mark.parametrize("case", L.CASES, ids=L.IDS)
def test_split_is_inside_a_quarter_of_every_bound(case, stage):
    """What the kept products hi.hi + hi.lo + lo.hi lose against the product of the same fp32 operands: each
    operand's lo term rounds to 2^-22 of the operand at worst and the dropped lo.lo product is up to 2^-22 of
    |a| |x| per term.  Measured: <= 0.19 x bound at every case and measure; at C = 6, where a six-term dot
    product averages nothing out, the figure depends on the seed (lnb_ref.CASES)."""
    r = L.refs(case)
    e = L.split_errors(case, stage)
    msg = f"{L.IDS[L.CASES.index(case)]} {stage} split: {_fmt(e, r.bound)}"
    print(msg)
    for k in L.MEASURES:
        assert e[k] <= r.bound[k] / 4, msg


@pytest.mark.parametrize("case", L.CASES, ids=L.IDS)
def test_whole_product_mutants_are_outside_the_bound(case):
    r = L.refs(case)
    for stage in ("gemm1", "gemm2"):
        kept = L.errors(L.emulate16(case, stage, L.KEEP3), r.s64.o, r.sc)
        for name, keep in (("DROP_LOHI", L.DROP_LOHI), ("DROP_HILO", L.DROP_HILO)):
            e = L.errors(L.emulate16(case, stage, keep), r.s64.o, r.sc)
            msg = f"{stage} {name}: {_fmt(e, r.bound)}   kept: {_fmt(kept, r.bound)}"
            print(msg)
            assert e["err_max"] >= 2 * r.bound["err_max"], msg
            assert kept["err_max"] <= r.bound["err_max"] / 2, msg


@pytest.mark.parametrize("case", L.CASES, ids=L.IDS)
def test_localized_mutants_show_on_their_measure_and_hide_in_the_old_one(case):
    r = L.refs(case)
    muts = L.localized(case)
    assert set(muts) == {"tile_lo", "tile_chunk", "small_row", "nondominant"}
    base = L.errors(L.emulate16(case, "gemm2", L.KEEP3), r.s64.o, r.sc)
    out64 = L.skip_out64(r.x, r.s64.o)
    for name, (o, measure) in muts.items():
        e = L.errors(o, r.s64.o, r.sc)
        old = L.rel_err(L.skip_out64(r.x, o), out64)
        msg = (f"{name} on {measure}: {_fmt(e, r.bound)}   err_max with skip {SKIP_TXT} {old:.2e} "
               f"({old / r.out_bound:.2f} x its bound {r.out_bound:.2e})")
        print(msg)
        assert e[measure] >= 2 * r.bound[measure], msg
        assert old < r.out_bound, msg
        if name == "small_row":                 # only that row moves: the other two measures do not see it
            assert e["err_max"] == base["err_max"] and e["err_pix"] <= max(base["err_pix"], r.bound["err_pix"] / 4), msg


SKIP_TXT = "(%.1f, %.1f)" % L.SKIP
