"""flash_attn_fwd's O / LSE and flash_attn_bwd's dQ against the fp64
reference of fa_fwd_dq_ref.py.

Both are called through paddle_amd._C with inputs built on the CPU; the
backward gets the fp32 lse and the bf16 O of the fp64 forward, so dQ is
tested on its own.  Bounds, with no free constant (fa_fwd_dq_ref.py):
    |out - ref| <= 2^-7*|ref| + 2^-7*A + 4*E            (O, dQ)
    |lse - ref| <= 4*E + 2^-22*(1 + |ref|)
test_fa_fwd_dq_cpu.py shows on the CPU that these bounds accept the kernels'
design and reject the mistakes their tile pipeline and transposed LDS reads
could make.

Shapes are the smallest at which the pipeline takes another path
(fa_fwd_dq_ref.SHAPES); the 2x3x200x200x128 cases also run on the strides of
the packed [B, S, 3, H, D] layout that the model uses, with dQ written into
the packed gradient.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from paddle_amd import _ext  # noqa: E402
from fa_fwd_dq_ref import OUTPUTS, SHAPES, case, shape_id, worst  # noqa: E402

DEV = "cuda:0"
CASES = [(s, False) for s in SHAPES] + [(s, True) for s in SHAPES if s[:5] == (2, 3, 200, 200, 128)]


def _case_id(c):
    return shape_id(c[0]) + ("_packed" if c[1] else "")


@pytest.mark.parametrize("shape,packed", CASES, ids=[_case_id(c) for c in CASES])
def test_fa_fwd_dq(shape, packed):
    C = _ext.get_ext(required=True)
    c = case(shape)
    b, h, sq, skv, d, causal = shape
    q, k, v, do, o_ref = (c[n].to(DEV) for n in ("q", "k", "v", "do", "o"))
    lse_ref = c["lse"].to(DEV)
    if packed:
        qkv = torch.stack([q, k, v], 0).permute(1, 3, 0, 2, 4).contiguous()   # [B, S, 3, H, D]
        q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
        o_ref = o_ref.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)    # [B, S, H, D] memory
        do = do.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
        o_buf = torch.full_like(o_ref, float("nan"))
        o, lse = C.flash_attn_fwd(q, k, v, o_buf, c["scale"], causal)
        dqkv = torch.full_like(qkv, float("nan"))
        dq, dk, dv = (dqkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
        C.flash_attn_bwd(do, q, k, v, o_ref, lse_ref, dq, dk, dv, c["scale"], causal)
    else:
        o, lse = C.flash_attn_fwd(q, k, v, None, c["scale"], causal)
        dq, _, _ = C.flash_attn_bwd(do, q, k, v, o_ref, lse_ref, None, None, None,
                                    c["scale"], causal)
    torch.cuda.synchronize()
    assert o.dtype == torch.bfloat16 and dq.dtype == torch.bfloat16 and lse.dtype == torch.float32
    assert tuple(o.shape) == (b, h, sq, d) and tuple(dq.shape) == (b, h, sq, d)
    assert tuple(lse.shape) == (b, h, sq)
    w = {n: worst(c, n, out) for n, out in (("o", o), ("lse", lse), ("dq", dq))}
    print(f"[fa_fwd_dq] {_case_id((shape, packed))}: err/bound o={w['o']:.4f} lse={w['lse']:.4f} "
          f"dq={w['dq']:.4f} (E " + " ".join(f"{n}={c['E'][n]:.2e}" for n in OUTPUTS) + ")")
    for n in OUTPUTS:
        assert w[n] <= 1.0, f"{n} err/bound {w[n]:.3f}"
