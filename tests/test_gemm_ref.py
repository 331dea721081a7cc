"""CPU checks that the fp32-class bound of the GEMM-class kernel tests has teeth (tests/gemm_ref.py): for every
case of every table, from the references alone, the six-product split-bf16 arithmetic sits far inside the bound
while a dropped product, a three-product kernel, a missing pixel, k row or 16-pixel step all land far outside it.
Also pins the table's notes to the mirrored grr_wgrad plan and the split to its definition."""
import re

import pytest
import torch

from tests import gemm_ref as R

IDS = [c.id for c in R.ALL_CASES]


def test_case_ids_are_unique_and_every_op_has_a_zero_mean_case():
    assert len(set(IDS)) == len(IDS)
    for name, table in R.TABLES.items():
        assert any(c.offset == 0.0 for c in table), name
        assert all(c.offset == 0.0 or (2.0 <= c.scale <= 3.0 and 0.3 <= c.offset <= 0.5) for c in table), name
        assert all(c.note for c in table), name
    assert len(R.STRUCTURAL_ONLY) <= len({R.OPS[c.op] for c in R.ALL_CASES})
    ops = [next(c.op for c in R.ALL_CASES if c.id == i) for i in R.STRUCTURAL_ONLY]
    assert len(set(ops)) == len(ops)                      # at most one per op


def test_split3_is_exact_and_its_terms_are_bf16():
    v = R.rand(4096, seed=1, scale=3.0, offset=0.5)
    v[:4] = torch.tensor([0.0, 1.0, -2.5, 3.0e-20])
    t = R.split3(v)
    assert torch.equal(t.float().bfloat16().double(), t)              # each term is a bf16 value
    resid = (v.double() - t.sum(0)).abs()
    assert float((resid / v.double().abs().clamp_min(1e-300)).max()) <= 2.0 ** -24
    assert torch.equal(t[0], v.bfloat16().double())
    # the kernels' term magnitudes: |t1| <= 2^-8 |v|, |t2| <= 2^-16 |v|
    assert float((t[1].abs() / v.double().abs().clamp_min(1e-300)).max()) <= 2.0 ** -8
    assert float((t[2].abs() / v.double().abs().clamp_min(1e-300)).max()) <= 2.0 ** -16


def test_emulate_with_all_nine_products_is_the_float64_reference():
    c = R.CONV1X1_X3[3]
    r = R.refs(c)
    nine = tuple((i, j) for i in range(3) for j in range(3))
    assert R.rel_err(R.emulate(R.OPS[c.op].f, r.a, r.b, nine), r.ref64) <= 2.0 ** -22
    assert R.SIX == tuple(sorted(R.SIX, key=R.SIX.index)) and len(R.DROP11) == 5 and (1, 1) not in R.DROP11


def test_dot32_is_an_fma_chain_in_blocks():
    """One fp32 accumulator per output, an fma per step, blocks of FMA_BLOCK steps added in order."""
    a = R.rand(3, 2 * R.FMA_BLOCK + 5, seed=2, scale=2.0, offset=0.3)
    b = R.rand(2 * R.FMA_BLOCK + 5, 4, seed=3)
    want = torch.zeros(3, 4)
    for i in range(3):
        for j in range(4):
            total = None
            for lo in range(0, a.shape[1], R.FMA_BLOCK):
                acc = torch.zeros((), dtype=torch.float32)
                for r in range(lo, min(lo + R.FMA_BLOCK, a.shape[1])):
                    acc = (acc.double() + a[i, r].double() * b[r, j].double()).float()
                total = acc if total is None else total + acc
            want[i, j] = total
    assert torch.equal(R.dot32(a, b), want)


@pytest.mark.parametrize("case", R.ALL_CASES, ids=IDS)
def test_fp32_evaluation_is_the_op_at_fp32_accuracy(case):
    """The fixed-order fp32 evaluation computes the op (a wrong one would only loosen the bound): within fp32
    rounding of float64 and of the library's own fp32 operators."""
    r = R.refs(case)
    assert r.ref32.dtype == torch.float32 and r.ref32.shape == r.ref64.shape
    assert R.rel_err(r.ref32, r.ref64) <= 6e-7
    assert R.rel_err(R.OPS[case.op].f(r.a, r.b), r.ref32.double()) <= 3e-6


@pytest.mark.parametrize("case", R.ALL_CASES, ids=IDS)
def test_bound_separates_the_split_from_the_term_mutants(case):
    six, drop11, keep3 = R.mutant_errors(case)
    bound = R.refs(case).bound
    print(f"{case.id}: bound {bound:.3e}  six {six:.3e} ({six / bound:.3f})  drop11 {drop11:.3e} "
          f"({drop11 / bound:.2f})  keep3 {keep3:.3e} ({keep3 / bound:.2f})")
    assert six <= bound / 10, (six, bound)
    if case.id in R.STRUCTURAL_ONLY:
        return
    assert drop11 >= 1.5 * bound, (drop11, bound)
    assert keep3 >= 2.0 * bound, (keep3, bound)


@pytest.mark.parametrize("case", R.ALL_CASES, ids=IDS)
def test_bound_catches_the_structural_mutants(case):
    r = R.refs(case)
    muts = R.structural(case)
    assert {"pixel", "krow"} <= set(muts)
    for name, m in muts.items():
        e = R.rel_err(m, r.ref64)
        print(f"{case.id}: {name} {e:.3e} = {e / r.bound:.0f} x bound")
        assert e >= 100 * r.bound, (name, e, r.bound)


WG_CASES = [c for c in R.ALL_CASES if c.op == "wgrad"]


@pytest.mark.parametrize("case", WG_CASES, ids=[c.id for c in WG_CASES])
def test_wgrad_notes_match_the_plan(case):
    """The note's tile, operand order, CP and cpi are the mirrored wgrad_plan's (the GPU test pins the mirror to
    grr_wgrad_workspace_bytes), and its step count / tail are the last chunk's."""
    b, m, k, p = case.shape
    plan = R.wgrad_plan(b, m, k, p, "tiles0" not in case.opts)
    want = f"{plan.tile} {'swap' if plan.swap else 'noswap'} CP={plan.CP} cpi={plan.cpi}"
    assert want in case.note, (want, case.note)
    last = p - (plan.cpi - 1) * plan.CP
    for key, val in (("ns", last // 16), ("tail", last % 16)):
        got = re.search(rf"{key}[= ](\d+)", case.note)
        if got:
            assert int(got.group(1)) == val, (key, val, case.note)


def test_wgrad_plan_reaches_every_tile_both_orders_and_a_multi_chunk_image():
    plans = [R.wgrad_plan(*c.shape, "tiles0" not in c.opts) for c in WG_CASES]
    assert {(pl.tile, pl.swap) for pl in plans} >= {("128x96", False), ("128x96", True), ("192x64", False),
                                                    ("192x64", True), ("64x96", False)}
    assert any(pl.cpi == 3 and c.shape[3] - 2 * pl.CP == 276 for pl, c in zip(plans, WG_CASES))


def test_structural_step_mutant_exists_where_the_last_chunk_has_a_full_step():
    for c in WG_CASES:
        b, m, k, p = c.shape
        plan = R.wgrad_plan(b, m, k, p, "tiles0" not in c.opts)
        assert ("step" in R.structural(c)) == ((p - (plan.cpi - 1) * plan.CP) >= 16), c.id
