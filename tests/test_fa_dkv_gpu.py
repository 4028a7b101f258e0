"""flash_attn_bwd's dK / dV against the fp64 reference of fa_dkv_ref.py.

The backward is called through paddle_amd._C.flash_attn_bwd with inputs
built on the CPU: bf16 Q, K, V, dO, the fp32 lse and the bf16 O of an fp64
forward.  Bound, with no free constant (fa_dkv_ref.py):
    |out - ref| <= 2^-7*|ref| + 2^-7*A + 4*E
test_fa_dkv_cpu.py shows on the CPU that this bound accepts the kernel's
design and rejects the mistakes its pipeline could make.

Shapes are the smallest at which the kernel's tile pipeline takes another
path (fa_dkv_ref.SHAPES); every shape with Sq == Skv also runs on the
strides of the packed [B, S, 3, H, D] layout that the model uses, with dK /
dV written into the packed gradient.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from paddle_amd import _ext  # noqa: E402
from fa_dkv_ref import SHAPES, case, shape_id, worst  # noqa: E402

DEV = "cuda:0"
CASES = [(s, False) for s in SHAPES] + [(s, True) for s in SHAPES if s[2] == s[3]]


def _case_id(c):
    return shape_id(c[0]) + ("_packed" if c[1] else "")


@pytest.mark.parametrize("shape,packed", CASES, ids=[_case_id(c) for c in CASES])
def test_fa_bwd_dkv(shape, packed):
    C = _ext.get_ext(required=True)
    c = case(shape)
    b, h, sq, skv, d, causal = shape
    q, k, v, do, o = (c[n].to(DEV) for n in ("q", "k", "v", "do", "o"))
    lse = c["lse"].to(DEV)
    if packed:
        qkv = torch.stack([q, k, v], 0).permute(1, 3, 0, 2, 4).contiguous()   # [B, S, 3, H, D]
        q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
        o = o.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)            # [B, S, H, D] memory
        do = do.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
        dqkv = torch.full_like(qkv, float("nan"))
        dq, dk, dv = (dqkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
        C.flash_attn_bwd(do, q, k, v, o, lse, dq, dk, dv, c["scale"], causal)
    else:
        dq, dk, dv = C.flash_attn_bwd(do, q, k, v, o, lse, None, None, None, c["scale"], causal)
    torch.cuda.synchronize()
    assert dk.dtype == torch.bfloat16 and dv.dtype == torch.bfloat16
    assert tuple(dk.shape) == (b, h, skv, d) and tuple(dv.shape) == (b, h, skv, d)
    w = {n: worst(c, n, out) for n, out in (("dv", dv), ("dk", dk))}
    print(f"[fa_dkv] {_case_id((shape, packed))}: err/bound dv={w['dv']:.4f} dk={w['dk']:.4f} "
          f"(E dv={c['E']['dv']:.2e} dk={c['E']['dk']:.2e})")
    assert w["dv"] <= 1.0, f"dv err/bound {w['dv']:.3f}"
    assert w["dk"] <= 1.0, f"dk err/bound {w['dk']:.3f}"
