"""The O / LSE / dQ bounds of tests/fa_fwd_dq_ref.py, checked on the CPU.

On every shape of test_fa_fwd_dq_gpu.py:
  * the fp32 torch evaluation of the reference formulas stays within the
    bounds (so they are not tighter than fp32 arithmetic);
  * a torch emulation of the design of fa_fwd32_kernel and
    fa_bwd_dq32_kernel (64-row kv tiles, online softmax with the threshold-8
    deferred maximum, P and dS rounded to bf16, fp32 accumulation, bf16
    outputs) stays within them;
  * the same emulation with one planted mistake is rejected, for O and for
    dQ, wherever the mistake can act at all:
      b_halves_swapped   B-fragment rows 8g+4..7 delivered before 8g+0..3
                         while the A fragment stays in natural k order
      chunks_swapped     the two 16-byte chunks of a row's 32 bytes swapped
                         on rows with (row>>2)&1 (address from base + 8p +
                         stride*q instead of the image's offset function)
      stale_buffer       tile t's second product reads tile t-1's V (O) or K
                         (dQ) image (needs two tiles in a q block)
      last_tile_dropped  the last kv tile of every q block is not computed
      causal_end_early   the causal end one tile early (causal only)
    Where a mistake cannot act (one tile per q block, non-causal) the
    emulation must return exactly the design's result.  The mistakes that
    touch only the second product's B operand must leave LSE bit-equal.
"""
import pytest
import torch

from fa_fwd_dq_ref import MISTAKES, OUTPUTS, SHAPES, can_act, case, emulate, shape_id, worst


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_fp32_reference_within_bound(shape):
    c = case(shape)
    for n in OUTPUTS:
        w = worst(c, n, c["r32"][n])
        print(f"[fa_fwd_dq] {shape_id(shape)} fp32 formulas {n}: E={c['E'][n]:.3e} err/bound={w:.4f}")
        assert w <= 1.0


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_design_within_bound(shape):
    c = case(shape)
    out, _ = emulate(shape)
    for n in OUTPUTS:
        w = worst(c, n, out[n])
        print(f"[fa_fwd_dq] {shape_id(shape)} design {n}: err/bound={w:.4f}")
        assert w <= 1.0


@pytest.mark.parametrize("mistake", MISTAKES)
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_mistake_rejected(shape, mistake):
    c = case(shape)
    out, applied = emulate(shape, mistake)
    out0, _ = emulate(shape)
    assert applied == can_act(shape, mistake)
    if not applied:
        assert all(torch.equal(out[n], out0[n]) for n in OUTPUTS)
        return
    if mistake in ("b_halves_swapped", "chunks_swapped", "stale_buffer"):
        assert torch.equal(out["lse"], out0["lse"])
    for n in ("o", "dq"):
        w = worst(c, n, out[n])
        print(f"[fa_fwd_dq] {shape_id(shape)} {mistake} {n}: err/bound={w:.2f}")
        assert w > 1.0, f"{mistake} passes the {n} bound (err/bound {w:.3f})"
