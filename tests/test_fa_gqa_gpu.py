"""The native GQA flash-attention backward (hkv != h) on the GPU.

paddle_amd._C.flash_attn_bwd / flash_attn_varlen_bwd with K / V of HKV heads:
dK / dV come back per kv head, summed over the group inside the kernel.
Inputs and the fp64 reference come from fa_gqa_ref.py; the bound has no free
constant:
    dK, dV:  |out - ref| <= 2^-7*|ref| + 2^-7*sum_g A_g + 4*E
    dQ:      the same with the A term of fa_fwd_dq_ref.py, on K / V repeated
test_fa_gqa_cpu.py shows on the CPU that this bound accepts the design and
rejects the mistakes the tile stream across heads could make.

Every shape runs with G (q heads per dK/dV block, gqa_heads_per_block) = rep
(bf16 straight from the kernel) and 1 (fp32 partials and the reduce kernel),
and 2 where rep is 4 or 8.  Shapes with Sq == Skv also run on the strides of a
packed [B, S, H + 2*HKV, D] qkv buffer with the gradients written into a
NaN-filled packed buffer.  Dropout and varlen go through the 32x32 kernels
and are checked at the tolerances of test_fa_launch_gpu.py (5e-2 backward,
6e-2 with dropout); dropout cases keep skv a multiple of 4 as there.
"""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from paddle_amd import _ext  # noqa: E402
from paddle_amd.ops.functional import (  # noqa: E402
    _FlashAttn, _fa_bwd_gqa_plan, _sdpa_ref, _sdpa_ref_bwd, flash_attn_varlen_func)
from fa_gqa_ref import SHAPES, case, shape_id, worst, worst_pair  # noqa: E402

DEV = "cuda:0"
P_DROP, SEED, OFFSET = 0.1, 4321, 77


def _gs(shape):
    rep = shape[1] // shape[2]
    return [rep, 1] + ([2] if rep in (4, 8) else [])


CASES = [(s, g) for s in SHAPES for g in _gs(s)]
PACKED = [(s, g) for s, g in CASES if s[3] == s[4]]


def _id(c):
    return "%s_G%d" % (shape_id(c[0]), c[1])


def _close(ours, ref, tol):
    torch.testing.assert_close(ours.float(), ref.float(), atol=tol, rtol=tol)


@functools.lru_cache(maxsize=None)
def _randn(seed, *shape):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(torch.bfloat16).to(DEV)


@functools.lru_cache(maxsize=None)
def _run(shape, G):
    """(dq, dk, dv) of the contiguous call; shared, never written to"""
    C = _ext.get_ext(required=True)
    c = case(shape)
    q, k, v, do, o = (c[n].to(DEV) for n in ("q", "k", "v", "do", "o"))
    out = C.flash_attn_bwd(do, q, k, v, o, c["lse"].to(DEV), None, None, None, c["scale"],
                           c["causal"], gqa_heads_per_block=G)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("shape,G", CASES, ids=[_id(c) for c in CASES])
def test_fa_gqa_bwd(shape, G):
    c = case(shape)
    b, h, hkv, sq, skv, d, causal = shape
    dq, dk, dv = _run(shape, G)
    assert dk.dtype == torch.bfloat16 and dv.dtype == torch.bfloat16
    assert tuple(dk.shape) == (b, hkv, skv, d) and tuple(dv.shape) == (b, hkv, skv, d)
    assert tuple(dq.shape) == (b, h, sq, d)
    w = {n: worst(c, n, out) for n, out in (("dv", dv), ("dk", dk), ("dq", dq))}
    print(f"[fa_gqa] {_id((shape, G))}: err/bound dv={w['dv']:.4f} dk={w['dk']:.4f} "
          f"dq={w['dq']:.4f} (E dv={c['E']['dv']:.2e} dk={c['E']['dk']:.2e} dq={c['E']['dq']:.2e})")
    for n in ("dv", "dk", "dq"):
        assert w[n] <= 1.0, f"{n} err/bound {w[n]:.3f}"


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_fa_gqa_heads_per_block_agree(shape):
    """Whole group per block and one head per block split the fp32 sum at
    different places and round once each: they agree within the bound, and dQ
    does not depend on G at all."""
    c = case(shape)
    rep = shape[1] // shape[2]
    dq_a, dk_a, dv_a = _run(shape, rep)
    dq_b, dk_b, dv_b = _run(shape, 1)
    assert torch.equal(dq_a, dq_b)
    for n, x, y in (("dv", dv_a, dv_b), ("dk", dk_a, dk_b)):
        w = worst_pair(c, n, x, y)
        print(f"[fa_gqa] {shape_id(shape)} G={rep} vs G=1 {n}: diff/bound={w:.4f}")
        assert w <= 1.0
    # G = 0 is the whole group
    C = _ext.get_ext(required=True)
    q, k, v, do, o = (c[n].to(DEV) for n in ("q", "k", "v", "do", "o"))
    out = C.flash_attn_bwd(do, q, k, v, o, c["lse"].to(DEV), None, None, None, c["scale"],
                           c["causal"])
    torch.cuda.synchronize()
    for x, y in zip(out, (dq_a, dk_a, dv_a)):
        assert torch.equal(x, y)


@pytest.mark.parametrize("shape,G", PACKED, ids=[_id(c) for c in PACKED])
def test_fa_gqa_bwd_packed(shape, G):
    """q, k, v are views of one [B, S, H + 2*HKV, D] buffer, dq / dk / dv views
    of a NaN-filled buffer of that layout: bit-equal to the contiguous call,
    and every element of the gradient buffer is written."""
    C = _ext.get_ext(required=True)
    c = case(shape)
    b, h, hkv, sq, skv, d, causal = shape
    bshd = lambda t: t.permute(0, 2, 1, 3)
    qkv = torch.cat([bshd(c[n]) for n in ("q", "k", "v")], 2).contiguous().to(DEV)
    assert tuple(qkv.shape) == (b, sq, h + 2 * hkv, d)
    split = lambda t: (bshd(t[:, :, :h]), bshd(t[:, :, h:h + hkv]), bshd(t[:, :, h + hkv:]))
    q, k, v = split(qkv)
    o = bshd(bshd(c["o"]).contiguous().to(DEV))
    do = bshd(bshd(c["do"]).contiguous().to(DEV))
    dqkv = torch.full_like(qkv, float("nan"))
    dq, dk, dv = split(dqkv)
    C.flash_attn_bwd(do, q, k, v, o, c["lse"].to(DEV), dq, dk, dv, c["scale"], causal,
                     gqa_heads_per_block=G)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(dqkv).any())
    for n, x, y in zip(("dq", "dk", "dv"), (dq, dk, dv), _run(shape, G)):
        assert torch.equal(x, y), f"{n}: packed and contiguous calls differ"


# ---------------------------------------------------------------------------
# dropout, dense: the 32x32 dK/dV kernels, dropout index by q head
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("G", [2, 1])
def test_fa_gqa_dropout(G):
    C = _ext.get_ext(required=True)
    B, H, HKV, S, d = 1, 4, 2, 136, 128
    scale = 1.0 / math.sqrt(d)
    q, do = _randn(600, B, H, S, d), _randn(603, B, H, S, d)
    k, v = _randn(601, B, HKV, S, d), _randn(602, B, HKV, S, d)
    o, lse = C.flash_attn_fwd(q, k, v, None, scale, True, None, P_DROP, SEED, OFFSET)
    dq, dk, dv = C.flash_attn_bwd(do, q, k, v, o, lse, None, None, None, scale, True, None,
                                  P_DROP, SEED, OFFSET, gqa_heads_per_block=G)
    keep = C.fa_dropout_mask(B, H, S, S, P_DROP, SEED, OFFSET)
    torch.cuda.synchronize()
    assert tuple(dk.shape) == (B, HKV, S, d) and tuple(dv.shape) == (B, HKV, S, d)
    ref_o, ref_lse = _sdpa_ref(q.float(), k.float(), v.float(), scale, True, None, keep, P_DROP)
    rdq, rdk, rdv = _sdpa_ref_bwd(do.float(), q.float(), k.float(), v.float(), ref_lse,
                                  scale, True, None, keep, P_DROP)
    _close(o, ref_o, 4e-2)
    _close(dq, rdq, 6e-2)
    _close(dk, rdk, 6e-2)
    _close(dv, rdv, 6e-2)


# ---------------------------------------------------------------------------
# varlen
# ---------------------------------------------------------------------------
LENS = [1, 37, 128, 130]
TOTAL = sum(LENS)
assert TOTAL % 4 == 0
VH, VHKV = 4, 2


def _cu():
    return torch.tensor([0] + list(torch.cumsum(torch.tensor(LENS), 0)),
                        dtype=torch.int32, device=DEV)


def _varlen_oracle(q, k, v, g, scale, causal, keep, p):
    """Per-sequence fp32 oracle; keep is fa_dropout_mask(1, H, total, total)
    with the column local to the sequence."""
    dq = torch.empty(q.shape, device=DEV)
    dk, dv = torch.empty(k.shape, device=DEV), torch.empty(k.shape, device=DEV)
    o = torch.empty(q.shape, device=DEV)
    s0 = 0
    for L in LENS:
        sl = slice(s0, s0 + L)
        s0 += L
        qs, ks, vs, gs = (t[sl].transpose(0, 1).unsqueeze(0).float() for t in (q, k, v, g))
        km = keep[:, :, sl, :L] if keep is not None else None
        oo, ll = _sdpa_ref(qs, ks, vs, scale, causal, None, km, p)
        a, b, c = _sdpa_ref_bwd(gs, qs, ks, vs, ll, scale, causal, None, km, p)
        o[sl] = oo[0].transpose(0, 1)
        dq[sl], dk[sl], dv[sl] = (t[0].transpose(0, 1) for t in (a, b, c))
    return o, dq, dk, dv


@pytest.mark.parametrize("p", [0.0, P_DROP], ids=["nodrop", "drop"])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("d", [64, 128])
def test_fa_gqa_varlen(d, causal, p):
    C = _ext.get_ext(required=True)
    scale = 1.0 / math.sqrt(d)
    cu = _cu()
    q, g = _randn(700, TOTAL, VH, d), _randn(703, TOTAL, VH, d)
    k, v = _randn(701, TOTAL, VHKV, d), _randn(702, TOTAL, VHKV, d)
    o, lse = C.flash_attn_varlen_fwd(q, k, v, cu, cu, scale, causal, p, SEED, OFFSET)
    res = {G: C.flash_attn_varlen_bwd(g, q, k, v, o, lse, cu, cu, scale, causal, p, SEED,
                                      OFFSET, gqa_heads_per_block=G) for G in (2, 1)}
    keep = C.fa_dropout_mask(1, VH, TOTAL, TOTAL, p, SEED, OFFSET) if p > 0 else None
    if p == 0:   # the public wrapper takes the native path with the plan's G
        G = _fa_bwd_gqa_plan(1, VH, VHKV, -(-TOTAL // 128))
        qg, kg, vg = (t.clone().requires_grad_(True) for t in (q, k, v))
        out = flash_attn_varlen_func(qg, kg, vg, cu, cu, max(LENS), max(LENS),
                                     scale=scale, causal=causal)
        out.backward(g)
        for a, b in zip((out, qg.grad, kg.grad, vg.grad), (o,) + tuple(res[G])):
            assert a.shape == b.shape and torch.equal(a, b)
    torch.cuda.synchronize()
    ro, rdq, rdk, rdv = _varlen_oracle(q, k, v, g, scale, causal, keep, p)
    ftol, btol = (4e-2, 6e-2) if p > 0 else (3e-2, 5e-2)
    _close(o, ro, ftol)
    assert torch.equal(res[1][0], res[2][0])    # dQ does not depend on G
    for G, (dq, dk, dv) in res.items():
        assert tuple(dk.shape) == (TOTAL, VHKV, d) and tuple(dv.shape) == (TOTAL, VHKV, d)
        _close(dq, rdq, btol)
        _close(dk, rdk, btol)
        _close(dv, rdv, btol)


# ---------------------------------------------------------------------------
# autograd path
# ---------------------------------------------------------------------------
# (shape, the plan's block threshold for the test, the G it must then choose):
# the threshold of the build gives one head per block on grids this small, so
# smaller ones bring the whole group (no workspace) and an intermediate G
# through the same autograd path
AUTOGRAD = [(SHAPES[1], None, 1), (SHAPES[1], 1, 2),
            (SHAPES[5], None, 1), (SHAPES[5], 8, 2), (SHAPES[5], 4, 4), (SHAPES[5], 1, 8)]


@pytest.mark.parametrize("shape,min_blocks,G", AUTOGRAD,
                         ids=["%s_G%d" % (shape_id(a[0]), a[2]) for a in AUTOGRAD])
def test_fa_gqa_autograd(shape, min_blocks, G, monkeypatch):
    """_FlashAttn with GQA calls the kernel directly: grads of k's shape,
    bit-equal to the direct call with the plan's G."""
    from paddle_amd.ops import functional
    C = _ext.get_ext(required=True)
    c = case(shape)
    b, h, hkv, sq, skv, d, causal = shape
    if min_blocks is not None:
        monkeypatch.setattr(functional, "_FA_GQA_MIN_BLOCKS", min_blocks)
    assert _fa_bwd_gqa_plan(b, h, hkv, -(-skv // 128)) == G
    q, k, v, do = (c[n].to(DEV) for n in ("q", "k", "v", "do"))
    qg, kg, vg = (t.clone().requires_grad_(True) for t in (q, k, v))
    o, lse = _FlashAttn.apply(qg, kg, vg, c["scale"], causal)
    o.backward(do)
    o2, lse2 = C.flash_attn_fwd(q, k, v, None, c["scale"], causal)
    want = C.flash_attn_bwd(do, q, k, v, o2, lse2, None, None, None, c["scale"], causal,
                            gqa_heads_per_block=G)
    torch.cuda.synchronize()
    assert kg.grad.shape == k.shape and vg.grad.shape == v.shape
    for x, y in zip((qg.grad, kg.grad, vg.grad), want):
        assert torch.equal(x, y)


# ---------------------------------------------------------------------------
# contract: off-contract calls raise before any launch
# ---------------------------------------------------------------------------
# Every bad argument is chosen so that even an unchecked launch would stay
# inside its buffers.
@pytest.mark.parametrize("bad", ["heads_per_block_3", "h_not_multiple", "gqa_mask", "dk_of_q_shape"])
def test_fa_gqa_bwd_contract(bad):
    C = _ext.get_ext(required=True)
    B, H, HKV, S, d = 1, 4, 1, 160, 64
    scale = 1.0 / math.sqrt(d)
    q, do = _randn(800, B, H, S, d), _randn(803, B, H, S, d)
    k, v = _randn(801, B, HKV, S, d), _randn(802, B, HKV, S, d)
    o, lse = C.flash_attn_fwd(q, k, v, None, scale, True)

    def call(q=q, k=k, v=v, o=o, lse=lse, do=do, dk=None, dv=None, mask=None, G=2):
        return C.flash_attn_bwd(do, q, k, v, o, lse, None, dk, dv, scale, True, mask,
                                gqa_heads_per_block=G)

    want = call()
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError):
        if bad == "heads_per_block_3":
            call(G=3)
        elif bad == "h_not_multiple":      # 3 q heads on 2 kv heads (K / V repeated)
            k2, v2 = k.expand(B, 2, S, d).contiguous(), v.expand(B, 2, S, d).contiguous()
            call(q=q[:, :3], k=k2, v=v2, o=o[:, :3], lse=lse[:, :3].contiguous(), do=do[:, :3], G=0)
        elif bad == "gqa_mask":
            call(mask=torch.zeros(1, 1, S, S, dtype=torch.bfloat16, device=DEV))
        else:
            call(dk=torch.empty_like(q), dv=torch.empty_like(q))
    torch.cuda.synchronize()
    got = call()
    torch.cuda.synchronize()
    for x, y in zip(got, want):
        assert torch.equal(x, y)
