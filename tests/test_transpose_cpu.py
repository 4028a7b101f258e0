"""CPU side of the K-contiguous wgrad: the gate stays closed off the GPU, and
the column-sum bound used on the GPU catches the mistakes a chunked sum can
make (tests/transpose_ref.py emulates transpose.hip's summation)."""
import pytest
import torch

import paddle_amd.nn.functional as F
from paddle_amd.ops import functional as hot
from paddle_amd.ops import gemm_dispatch as gd

from transpose_ref import SHAPES, chunked_colsum, colsum_bound, plan


def _x(r, c, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(r, c, generator=g).to(torch.bfloat16)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("bias", [True, False])
def test_cpu_gate_closed_grads_equal_autograd(dtype, bias):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 24, 16, generator=g).to(dtype).requires_grad_()
    w = torch.randn(16, 40, generator=g).to(dtype).requires_grad_()
    b = torch.randn(40, generator=g).to(dtype).requires_grad_() if bias else None
    dy = torch.randn(2, 24, 40, generator=g).to(dtype)
    assert not hot._lt_linear_ok(x, w, b)
    assert not gd.transpose_ok(x.reshape(-1, 16))
    assert hot._wgrad_form(x.reshape(-1, 16), dy.reshape(-1, 40)) == "tn"
    F.linear(x, w, b).backward(dy)
    got = [t.grad.clone() for t in (x, w) + ((b,) if bias else ())]
    for t in (x, w, b):
        if t is not None:
            t.grad = None
    x2 = x.reshape(-1, 16)
    y = torch.addmm(b, x2, w).reshape(2, 24, 40) if bias else torch.matmul(x, w)
    y.backward(dy)
    ref = [t.grad for t in (x, w) + ((b,) if bias else ())]
    for a, r in zip(got, ref):
        assert torch.equal(a, r)


def test_cpu_gate_closed_at_flagship_size():
    # the size gate alone would open: the device keeps it shut
    x = torch.empty(16384, 4096, dtype=torch.bfloat16, device="meta")
    w = torch.empty(4096, 4096, dtype=torch.bfloat16, device="meta").requires_grad_()
    assert hot._wgrad_kc_size(16384, 4096, 4096)
    assert not hot._lt_linear_ok(x, w, None)


@pytest.mark.parametrize("r,c", SHAPES)
def test_chunked_colsum_within_bound(r, c):
    x = _x(r, c)
    ref, bound = colsum_bound(x)
    err = (chunked_colsum(x).double() - ref).abs()
    assert (err <= bound).all(), float((err / bound).max())


def test_plan_covers_rows():
    for r, c in SHAPES + [(24576, 4096), (24576, 16384)]:
        tpc, chunks = plan(r, c)
        nrt = -(-r // 128)
        assert chunks >= 1 and (chunks - 1) * tpc < nrt <= chunks * tpc


def _fails(x, got):
    ref, bound = colsum_bound(x)
    return got.shape != ref.shape or not ((got.double() - ref).abs() <= bound).all()


def test_planted_last_partial_tile_dropped_fails():
    x = _x(200, 264)
    assert _fails(x, chunked_colsum(x, drop_last_partial_tile=True))


def test_planted_chunk_dropped_fails():
    x = _x(1032, 4096)
    assert plan(1032, 4096)[1] >= 2
    assert _fails(x, chunked_colsum(x, drop_chunk=1))


def test_planted_sum_over_output_columns_fails():
    x = _x(64, 64)
    assert _fails(x, chunked_colsum(x, over_output_columns=True))
