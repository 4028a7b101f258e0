"""The GQA dK/dV bound of tests/fa_gqa_ref.py and the plan function, on the CPU.

On every shape of test_fa_gqa_gpu.py and every valid G (q heads per block):
  * the fp32 torch evaluation of the group-summed reference formulas stays
    within the bound (so the bound is not tighter than fp32 arithmetic), dQ
    included;
  * a torch emulation of the design (one tile stream across the G heads of a
    block, fp32 accumulators over the whole stream, fp32 partials summed in
    head order for G < rep, one bf16 rounding) stays within it;
  * the same emulation with one planted mistake (fa_gqa_ref.MISTAKES) is
    rejected, for dV and for dK, wherever the mistake can act at all; where
    it cannot (one head per block, one kv head, no reduce) the emulation must
    return exactly the design's result.
_fa_bwd_gqa_plan, the one place that chooses G, is checked for its
properties on shapes alone.
"""
import pytest
import torch

from fa_gqa_ref import MISTAKES, SHAPES, can_act, case, divisors, emulate, shape_id, worst
from paddle_amd.ops.functional import _FA_GQA_MIN_BLOCKS, _fa_bwd_gqa_plan

CASES = [(s, g) for s in SHAPES for g in divisors(s[1] // s[2])]


def _id(c):
    return "%s_G%d" % (shape_id(c[0]), c[1])


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_fp32_reference_within_bound(shape):
    c = case(shape)
    for n in ("dv", "dk", "dq"):
        w = worst(c, n, c["r32"][n])
        print(f"[fa_gqa] {shape_id(shape)} fp32 formulas {n}: E={c['E'][n]:.3e} err/bound={w:.4f}")
        assert w <= 1.0


@pytest.mark.parametrize("shape,G", CASES, ids=[_id(c) for c in CASES])
def test_design_within_bound(shape, G):
    c = case(shape)
    dv, dk, _ = emulate(shape, G)
    assert dv.dtype == torch.bfloat16 and dv.shape == c["k"].shape
    for n, out in (("dv", dv), ("dk", dk)):
        w = worst(c, n, out)
        print(f"[fa_gqa] {_id((shape, G))} design {n}: err/bound={w:.4f}")
        assert w <= 1.0


def test_every_mistake_acts_on_two_shapes():
    for m in MISTAKES:
        shapes = {s for s, g in CASES if can_act(s, g, m)}
        assert len(shapes) >= 2, m


@pytest.mark.parametrize("mistake", MISTAKES)
@pytest.mark.parametrize("shape,G", CASES, ids=[_id(c) for c in CASES])
def test_mistake_rejected(shape, G, mistake):
    c = case(shape)
    dv, dk, applied = emulate(shape, G, mistake)
    assert applied == can_act(shape, G, mistake)
    if not applied:
        dv0, dk0, _ = emulate(shape, G)
        assert torch.equal(dv, dv0) and torch.equal(dk, dk0)
        return
    for n, out in (("dv", dv), ("dk", dk)):
        w = worst(c, n, out)
        print(f"[fa_gqa] {_id((shape, G))} {mistake} {n}: err/bound={w:.2f}")
        assert w > 1.0, f"{mistake} passes the {n} bound (err/bound {w:.3f})"


# ---------------------------------------------------------------------------
# _fa_bwd_gqa_plan
# ---------------------------------------------------------------------------
PLAN_HEADS = [(8, 1), (8, 2), (32, 8), (64, 8), (6, 2), (12, 1), (4, 4), (7, 1)]


@pytest.mark.parametrize("h,hkv", PLAN_HEADS)
def test_plan_properties(h, hkv):
    rep = h // hkv
    prev = None
    for blocks in (1 << 20, 4096, 512, 300, 128, 64, 17, 4, 1):   # B * n_kv_blocks, shrinking
        for b, nkv in ((blocks, 1), (1, blocks)):
            g = _fa_bwd_gqa_plan(b, h, hkv, nkv)
            assert 1 <= g <= rep and rep % g == 0
            assert g == _fa_bwd_gqa_plan(nkv, h, hkv, b)          # the grid's size alone
        if prev is not None:
            assert g <= prev, "G grows as the grid shrinks"
        prev = g
    assert _fa_bwd_gqa_plan(1 << 20, h, hkv, 1) == rep            # large grid: the whole group
    if rep > 1:
        assert _fa_bwd_gqa_plan(1, h, hkv, 1) == 1                # tiny grid: one head per block
    # the largest divisor that still fills the machine
    for blocks in (512, 300, 64, 3):
        g = _fa_bwd_gqa_plan(1, h, hkv, blocks)
        assert g == 1 or (h // g) * blocks >= _FA_GQA_MIN_BLOCKS
        for g2 in divisors(rep):
            if g2 > g:
                assert (h // g2) * blocks < _FA_GQA_MIN_BLOCKS


def test_plan_mha_is_one():
    for b, h, n in ((1, 1, 1), (4, 32, 16), (12, 32, 16), (1, 8, 1024)):
        assert _fa_bwd_gqa_plan(b, h, h, n) == 1


def test_plan_tp8_70b_rank():
    """H 8, HKV 1 at B 2, S 4096: a whole-group grid is 64 blocks, so the plan
    splits the group."""
    assert _fa_bwd_gqa_plan(2, 8, 1, 32) < 8
    assert _fa_bwd_gqa_plan(4, 32, 8, 16) == 4     # 512 blocks with the whole group
