"""Flash-attention launch path: strides, mask + dropout, varlen, contract.

The numerics of the kernels are covered by test_kernels_gpu.py and
test_fa_dkv_gpu.py on contiguous or equal-stride tensors.  These tests are
about what sits between the binding and the kernel: which stride triple goes
with which tensor, the mask strides, the dropout element index, the varlen
block geometry, and the checks a call has to pass before anything is
launched.  They go through paddle_amd._C and paddle_amd.ops.functional only.

Shapes are the smallest that cross a 128-row block edge and leave a tail
(160 = 128 + 32, varlen lengths 1 / 37 / 128 / 130).  Tolerances are those of
test_kernels_gpu.py: 3e-2 forward and 5e-2 backward, 4e-2 / 6e-2 with
dropout, 2e-2 on lse.

Every dropout case keeps skv (varlen: the packed total) a multiple of 4: the
forward / dQ kernels and the dK/dV kernel / fa_dropout_mask index the Philox
lanes differently otherwise (docs/KERNELS.md, flash attention, known
limitation).
"""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from paddle_amd import _ext  # noqa: E402
from paddle_amd.ops.functional import (  # noqa: E402
    _FlashAttn, _sdpa_ref, _sdpa_ref_bwd, flash_attn_varlen_func)

DEV = "cuda:0"
SENTINEL = -768.0   # exact in bf16
P_DROP, SEED, OFFSET = 0.3, 4321, 77


def _close(ours, ref, tol):
    torch.testing.assert_close(ours.float(), ref.float(), atol=tol, rtol=tol)


@functools.lru_cache(maxsize=None)
def _randn(seed, *shape):
    """bf16 normal data generated on the CPU from a fixed seed; shared and
    never written to."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(torch.bfloat16).to(DEV)


def _into(buf, view, src):
    """Copy src into view(buf) and return that view."""
    t = view(buf)
    t.copy_(src)
    return t


def _assert_padding_untouched(buf, *views):
    written = torch.zeros_like(buf, dtype=torch.bool)
    for view in views:
        view(written).fill_(True)
    assert (~written).any(), "buffer has no padding"
    assert bool((buf[~written] == SENTINEL).all()), "padding was written"


def _triple(t):
    return (t.stride(0), t.stride(1), t.stride(2))


# ---------------------------------------------------------------------------
# every stride triple distinct
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("d", [64, 128])
def test_fa_distinct_strides(d, causal):
    """q, {k, v}, dout, o, dq_out and {dk_out, dv_out} are views of buffers in
    six different layouts.  The results are bit-equal to the same calls on
    contiguous clones (no atomics, no address-dependent arithmetic), agree
    with the fp32 oracle, and leave the padding of the output buffers alone."""
    C = _ext.get_ext(required=True)
    B, H, S = 2, 2, 160
    scale = 1.0 / math.sqrt(d)
    qc, kc, vc, doc = (_randn(100 + i, B, H, S, d) for i in range(4))

    def bf(*shape):
        return torch.full(shape, SENTINEL, dtype=torch.bfloat16, device=DEV)

    v_q = lambda t: t.permute(0, 2, 1, 3)                         # [B,S,H,D]
    v_k = lambda t: t[:, :, 0].permute(0, 2, 1, 3)                # [B,S,2,H,D]
    v_v = lambda t: t[:, :, 1].permute(0, 2, 1, 3)
    v_do = lambda t: t[:, :, :S]                                  # [B,H,S+8,D]
    v_o = lambda t: t[:, :, :S].permute(1, 0, 2, 3)               # [H,B,S+24,D]
    v_dq = lambda t: t[:, :S, :, :d].permute(0, 2, 1, 3)          # [B,S+8,H,2D]
    v_dk = lambda t: t[:, :, 0, :S]                               # [B,H,2,S+8,D]
    v_dv = lambda t: t[:, :, 1, :S]

    q = _into(bf(B, S, H, d), v_q, qc)
    kv_buf = bf(B, S, 2, H, d)
    k, v = _into(kv_buf, v_k, kc), _into(kv_buf, v_v, vc)
    do = _into(bf(B, H, S + 8, d), v_do, doc)
    o_buf, dq_buf, dkv_buf = bf(H, B, S + 24, d), bf(B, S + 8, H, 2 * d), bf(B, H, 2, S + 8, d)
    o, dq, dk, dv = v_o(o_buf), v_dq(dq_buf), v_dk(dkv_buf), v_dv(dkv_buf)

    triples = [_triple(t) for t in (q, k, do, o, dq, dk)]
    assert len(set(triples)) == 6, triples
    assert _triple(k) == _triple(v) and _triple(dk) == _triple(dv)
    for t in (q, k, v, do, o, dq, dk, dv):
        assert t.stride(3) == 1 and t.stride(2) % 8 == 0 and tuple(t.shape) == (B, H, S, d)

    o_ret, lse = C.flash_attn_fwd(q, k, v, o, scale, causal)
    assert o_ret.data_ptr() == o.data_ptr()
    C.flash_attn_bwd(do, q, k, v, o, lse, dq, dk, dv, scale, causal)

    o_c, lse_c = C.flash_attn_fwd(qc, kc, vc, None, scale, causal)
    dq_c, dk_c, dv_c = C.flash_attn_bwd(doc, qc, kc, vc, o_c, lse_c, None, None, None,
                                        scale, causal)
    torch.cuda.synchronize()
    for name, a, b in (("o", o, o_c), ("lse", lse, lse_c), ("dq", dq, dq_c),
                       ("dk", dk, dk_c), ("dv", dv, dv_c)):
        assert torch.equal(a, b), f"{name}: strided and contiguous calls differ"

    _assert_padding_untouched(o_buf, v_o)
    _assert_padding_untouched(dq_buf, v_dq)
    _assert_padding_untouched(dkv_buf, v_dk, v_dv)

    ref_o, ref_lse = _sdpa_ref(qc.float(), kc.float(), vc.float(), scale, causal)
    rdq, rdk, rdv = _sdpa_ref_bwd(doc.float(), qc.float(), kc.float(), vc.float(),
                                  ref_lse, scale, causal)
    _close(o, ref_o, 3e-2)
    _close(lse, ref_lse, 2e-2)
    _close(dq, rdq, 5e-2)
    _close(dk, rdk, 5e-2)
    _close(dv, rdv, 5e-2)


# ---------------------------------------------------------------------------
# mask and dropout together
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mask_kind", ["1H", "B1"])
@pytest.mark.parametrize("sq,skv,causal", [(96, 160, False), (160, 160, True)],
                         ids=["96x160", "160x160_causal"])
@pytest.mark.parametrize("d", [64, 128])
def test_fa_mask_dropout(d, sq, skv, causal, mask_kind):
    """Additive mask broadcast over batch or over heads, a view of a buffer
    with row length skv + 8, together with dropout: forward and the three
    gradients against the oracle fed with fa_dropout_mask."""
    C = _ext.get_ext(required=True)
    B, H = 2, 2
    scale = 1.0 / math.sqrt(d)
    q, do = _randn(200, B, H, sq, d), _randn(203, B, H, sq, d)
    k, v = _randn(201, B, H, skv, d), _randn(202, B, H, skv, d)
    mb, mh = (1, H) if mask_kind == "1H" else (B, 1)
    mvals = _randn(204, mb, mh, sq, skv).float() * 0.5
    mvals[..., ::7] = -10000.0
    mask = torch.zeros(mb, mh, sq, skv + 8, dtype=torch.bfloat16, device=DEV)[..., :skv]
    mask.copy_(mvals)
    assert mask.stride(2) == skv + 8

    qg, kg, vg = (t.clone().requires_grad_(True) for t in (q, k, v))
    o, lse = _FlashAttn.apply(qg, kg, vg, scale, causal, mask, P_DROP, SEED, OFFSET)
    o.backward(do)
    keep = C.fa_dropout_mask(B, H, sq, skv, P_DROP, SEED, OFFSET)
    torch.cuda.synchronize()
    assert abs(keep.float().mean().item() - (1 - P_DROP)) < 0.02

    ref_o, ref_lse = _sdpa_ref(q.float(), k.float(), v.float(), scale, causal,
                               mask.float(), keep, P_DROP)
    rdq, rdk, rdv = _sdpa_ref_bwd(do.float(), q.float(), k.float(), v.float(), ref_lse,
                                  scale, causal, mask.float(), keep, P_DROP)
    _close(o, ref_o, 4e-2)
    _close(lse, ref_lse, 2e-2)
    _close(qg.grad, rdq, 6e-2)
    _close(kg.grad, rdk, 6e-2)
    _close(vg.grad, rdv, 6e-2)


# ---------------------------------------------------------------------------
# varlen
# ---------------------------------------------------------------------------
LENS = [1, 37, 128, 130]
TOTAL = sum(LENS)
assert TOTAL % 4 == 0


def _cu():
    return torch.tensor([0] + list(torch.cumsum(torch.tensor(LENS), 0)),
                        dtype=torch.int32, device=DEV)


def _varlen_oracle(q, k, v, g, scale, causal, keep, p):
    """Per-sequence fp32 oracle.  keep is fa_dropout_mask(1, H, total_q,
    total_k): the element of sequence i, head h, row r, column c is
    keep[0, h, cu_q[i] + r, c] -- the column is local to the sequence."""
    h, hkv = q.shape[1], k.shape[1]
    o = torch.empty(q.shape, device=DEV)
    lse = torch.empty(h, q.shape[0], device=DEV)
    dq = torch.empty(q.shape, device=DEV)
    dk, dv = torch.empty(k.shape, device=DEV), torch.empty(k.shape, device=DEV)
    s0 = 0
    for L in LENS:
        sl = slice(s0, s0 + L)
        s0 += L
        qs, ks, vs = (t[sl].transpose(0, 1).unsqueeze(0).float() for t in (q, k, v))
        km = keep[:, :, sl, :L] if keep is not None else None
        oo, ll = _sdpa_ref(qs, ks, vs, scale, causal, None, km, p)
        o[sl], lse[:, sl] = oo[0].transpose(0, 1), ll[0]
        if g is not None and hkv == h:
            gs = g[sl].transpose(0, 1).unsqueeze(0).float()
            a, b, c = _sdpa_ref_bwd(gs, qs, ks, vs, ll, scale, causal, None, km, p)
            dq[sl], dk[sl], dv[sl] = (t[0].transpose(0, 1) for t in (a, b, c))
    return o, lse, dq, dk, dv


@pytest.mark.parametrize("p", [0.0, P_DROP], ids=["nodrop", "drop"])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("d", [64, 128])
def test_fa_varlen(d, causal, p):
    C = _ext.get_ext(required=True)
    H = 4
    scale = 1.0 / math.sqrt(d)
    cu = _cu()
    q, k, v, g = (_randn(300 + i, TOTAL, H, d) for i in range(4))
    o, lse = C.flash_attn_varlen_fwd(q, k, v, cu, cu, scale, causal, p, SEED, OFFSET)
    dq, dk, dv = C.flash_attn_varlen_bwd(g, q, k, v, o, lse, cu, cu, scale, causal,
                                         p, SEED, OFFSET)
    keep = C.fa_dropout_mask(1, H, TOTAL, TOTAL, p, SEED, OFFSET) if p > 0 else None
    if p == 0:   # the public wrapper takes the same path
        qg, kg, vg = (t.clone().requires_grad_(True) for t in (q, k, v))
        out = flash_attn_varlen_func(qg, kg, vg, cu, cu, max(LENS), max(LENS),
                                     scale=scale, causal=causal)
        out.backward(g)
        for a, b in ((out, o), (qg.grad, dq), (kg.grad, dk), (vg.grad, dv)):
            assert torch.equal(a, b)
    torch.cuda.synchronize()
    ro, rlse, rdq, rdk, rdv = _varlen_oracle(q, k, v, g, scale, causal, keep, p)
    ftol, btol = (4e-2, 6e-2) if p > 0 else (3e-2, 5e-2)
    _close(o, ro, ftol)
    _close(lse, rlse, 2e-2)
    _close(dq, rdq, btol)
    _close(dk, rdk, btol)
    _close(dv, rdv, btol)


def test_fa_varlen_gqa_fwd():
    C = _ext.get_ext(required=True)
    H, HKV, d = 4, 2, 128
    scale = 1.0 / math.sqrt(d)
    cu = _cu()
    q = _randn(310, TOTAL, H, d)
    k, v = _randn(311, TOTAL, HKV, d), _randn(312, TOTAL, HKV, d)
    with torch.no_grad():
        o, lse = C.flash_attn_varlen_fwd(q, k, v, cu, cu, scale, True)
    torch.cuda.synchronize()
    ro, rlse, *_ = _varlen_oracle(q, k, v, None, scale, True, None, 0.0)
    _close(o, ro, 3e-2)
    _close(lse, rlse, 2e-2)


# ---------------------------------------------------------------------------
# contract: off-contract calls raise before any launch
# ---------------------------------------------------------------------------
# Every bad argument is chosen so that even an unchecked launch would stay
# inside its buffers.
def _dense_args():
    B, H, S, d = 1, 2, 160, 64
    q, k, v, do = (_randn(400 + i, B, H, S, d) for i in range(4))
    return dict(q=q, k=k, v=v, do=do, scale=1.0 / math.sqrt(d), dq=None, dk=None, dv=None)


def _dense_bwd(C, a, o, lse):
    return C.flash_attn_bwd(a["do"], a["q"], a["k"], a["v"], o, lse, a["dq"], a["dk"],
                            a["dv"], a["scale"], True)


def _bad_fp16_q(a, o, lse):
    a["q"] = a["q"].to(torch.float16)
    return o, lse


def _bad_rank3_q(a, o, lse):
    a["q"] = a["q"][0]
    return o, lse


def _bad_head_dim_96(a, o, lse):
    for n in ("q", "k", "v", "do"):
        a[n] = torch.cat([a[n], a[n]], -1)[..., :96]
    return torch.cat([o, o], -1)[..., :96], lse


def _bad_lse_shape(a, o, lse):
    return o, torch.cat([lse, lse[..., :1]], -1)


def _bad_dout_shape(a, o, lse):
    a["do"] = torch.cat([a["do"], a["do"][:, :, :8]], 2)
    return o, lse


def _bad_kv_strides(a, o, lse):
    a["v"] = a["v"].permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
    return o, lse


def _bad_dkdv_strides(a, o, lse):
    a["dk"] = torch.empty_like(a["k"])
    B, H, S, d = a["v"].shape
    a["dv"] = torch.empty(B, S, H, d, dtype=torch.bfloat16, device=DEV).permute(0, 2, 1, 3)
    assert _triple(a["dk"]) != _triple(a["dv"])
    return o, lse


def _bad_seq_stride_132(a, o, lse):
    B, H, S, d = a["q"].shape
    buf = torch.zeros(B, H, S, 132, dtype=torch.bfloat16, device=DEV)
    buf[..., :d] = a["q"]
    a["q"] = buf[..., :d]
    assert a["q"].stride(2) == 132
    return o, lse


DENSE_BAD = [_bad_fp16_q, _bad_rank3_q, _bad_head_dim_96, _bad_lse_shape, _bad_dout_shape,
             _bad_kv_strides, _bad_dkdv_strides, _bad_seq_stride_132]


@pytest.mark.parametrize("bad", DENSE_BAD, ids=[f.__name__[5:] for f in DENSE_BAD])
def test_fa_bwd_contract(bad):
    C = _ext.get_ext(required=True)
    good = _dense_args()
    o, lse = C.flash_attn_fwd(good["q"], good["k"], good["v"], None, good["scale"], True)
    want = _dense_bwd(C, good, o, lse)
    torch.cuda.synchronize()
    a = dict(good)
    bad_o, bad_lse = bad(a, o, lse)
    with pytest.raises(RuntimeError):
        _dense_bwd(C, a, bad_o, bad_lse)
    torch.cuda.synchronize()
    got = _dense_bwd(C, good, o, lse)
    torch.cuda.synchronize()
    for x, y in zip(got, want):
        assert torch.equal(x, y)


@pytest.mark.parametrize("bad", ["noncontiguous_k", "cu_q_last"])
def test_fa_varlen_bwd_contract(bad):
    C = _ext.get_ext(required=True)
    H, d = 2, 64
    scale = 1.0 / math.sqrt(d)
    cu = _cu()
    q, k, v, g = (_randn(500 + i, TOTAL, H, d) for i in range(4))
    o, lse = C.flash_attn_varlen_fwd(q, k, v, cu, cu, scale, False)
    want = C.flash_attn_varlen_bwd(g, q, k, v, o, lse, cu, cu, scale, False, 0.0, 0, 0)
    torch.cuda.synchronize()
    bk, bcu = k, cu
    if bad == "noncontiguous_k":
        bk = torch.cat([k, k], -1)[..., :d]
        assert not bk.is_contiguous()
    else:
        bcu = cu.clone()
        bcu[-1] -= 4
    with pytest.raises(RuntimeError):
        C.flash_attn_varlen_bwd(g, q, bk, v, o, lse, bcu, cu, scale, False, 0.0, 0, 0)
    torch.cuda.synchronize()
    got = C.flash_attn_varlen_bwd(g, q, k, v, o, lse, cu, cu, scale, False, 0.0, 0, 0)
    torch.cuda.synchronize()
    for x, y in zip(got, want):
        assert torch.equal(x, y)
