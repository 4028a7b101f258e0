"""The dK/dV bound of tests/fa_dkv_ref.py, checked on the CPU.

On every shape of test_fa_dkv_gpu.py:
  * the fp32 torch evaluation of the reference formulas stays within the
    bound (so the bound is not tighter than fp32 arithmetic);
  * a torch emulation of the kernel's design (bf16-rounded P and dS, 64-row
    q tiles, 128-row kv blocks, fp32 accumulation, bf16 outputs) stays
    within it;
  * the same emulation with one planted mistake is rejected, for dV and for
    dK, wherever the mistake can act at all:
      b_halves_swapped   B-fragment rows 8g+4..7 delivered before 8g+0..3
                         while the A fragment stays in natural k order
      chunks_swapped     the two 16-byte chunks of a row's 32 bytes swapped
                         on rows with (row>>2)&1 (address from base + 8p +
                         stride*q instead of the image's offset function)
      stale_buffer       the second tile's dV/dK products read the first
                         tile's Q/dO (needs two tiles in a kv block)
      last_tile_dropped  the last q tile of every kv block is not computed
      q_start_late       the causal q_start one tile late (causal only)
    Where a mistake cannot act (one tile per kv block, non-causal) the
    emulation must return exactly the design's result.
"""
import pytest
import torch

from fa_dkv_ref import MISTAKES, SHAPES, case, emulate, shape_id, worst


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_fp32_reference_within_bound(shape):
    c = case(shape)
    for n in ("dv", "dk"):
        w = worst(c, n, c["r32"][n])
        print(f"[fa_dkv] {shape_id(shape)} fp32 formulas {n}: E={c['E'][n]:.3e} err/bound={w:.4f}")
        assert w <= 1.0


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_design_within_bound(shape):
    c = case(shape)
    dv, dk, _ = emulate(c)
    for n, out in (("dv", dv), ("dk", dk)):
        w = worst(c, n, out)
        print(f"[fa_dkv] {shape_id(shape)} design {n}: err/bound={w:.4f}")
        assert w <= 1.0


def _can_act(shape, mistake):
    b, h, sq, skv, d, causal = shape
    if mistake == "q_start_late":
        return causal
    if mistake == "stale_buffer":     # some kv block with at least two q tiles
        return any(len(range((kv0 // 64) * 64 if causal else 0, sq, 64)) >= 2
                   for kv0 in range(0, skv, 128))
    return True


@pytest.mark.parametrize("mistake", MISTAKES)
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_mistake_rejected(shape, mistake):
    c = case(shape)
    dv, dk, applied = emulate(c, mistake)
    assert applied == _can_act(shape, mistake)
    if not applied:
        dv0, dk0, _ = emulate(c)
        assert torch.equal(dv, dv0) and torch.equal(dk, dk0)
        return
    for n, out in (("dv", dv), ("dk", dk)):
        w = worst(c, n, out)
        print(f"[fa_dkv] {shape_id(shape)} {mistake} {n}: err/bound={w:.2f}")
        assert w > 1.0, f"{mistake} passes the {n} bound (err/bound {w:.3f})"
