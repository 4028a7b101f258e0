"""Unsplit paged decode attention on the GPU: C.decode_attention and
C.decode_attention_int8 (one block per q-head of the decode_attn_kernel
that C.decode_attention_split also launches), the dense [2, B, H, MS, D]
layout of masked_multihead_attention, and the contract of decode_attention.

Cases, reference and bound are those of test_decode_attn_split_gpu.py /
test_kv_int8_gpu.py: softmax(scale q k^T) v in fp64 from the stored values,

    |out - ref| <= 2^-7 |ref| + 4 E + 2^-22 A

compared with <=.  The unsplit launch walks [0, S) with the scale folded
into q and merges its position slots in slot order, which the CPU emulation
of test_kv_int8_cpu.py / test_decode_attn_split_cpu.py (n = 1) covers.
"""
import functools
import math

import pytest
import torch

from test_decode_attn_split_gpu import (EDGE_LENS, SHAPES, edge_case,
                                        needle_head_case, ref_attn_bf16,
                                        ref_of, run_unsplit)
from test_kv_int8_gpu import BF16, DEV, check, to_dev


def _C():
    from paddle_amd import _ext
    return _ext.get_ext(required=True)


@pytest.mark.gpu
@pytest.mark.parametrize("D,H,HKV,bs", SHAPES)
def test_decode_attention_edges_gpu(D, H, HKV, bs):
    """The bf16 unsplit kernel at the derived bound: lengths around the
    block step and the 64-position granule, S = 0 exactly zero."""
    c, ref, bound = edge_case("bf16", D, H, HKV, bs)
    out = run_unsplit(_C(), c)
    assert out.dtype == BF16 and tuple(out.shape) == (len(EDGE_LENS), H, D)
    assert bool((out[0] == 0).all()), "S = 0 must give zeros"
    check(f"bf16 D{D} H{H} HKV{HKV} bs{bs} unsplit", out, ref, bound)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["int8_token", "bf16"])
def test_decode_attention_unsplit_needle_gpu(kind):
    """S = 513: the needle at the first position, either side of the first
    block edge and the last position, for each q-head of the group."""
    D, H, HKV, bs, S = 128, 8, 2, 16, 513
    C = _C()
    for n in (0, 15, 16, 512):
        for j in range(H // HKV):
            c = needle_head_case(kind, D, H, HKV, bs, S, n, j, 900 + 7 * n + j)
            ref, bound = ref_of(c)
            assert float((ref[0, j] - 3.0).abs().max()) < 1.5
            check(f"{kind} needle n={n} head {j}",
                  run_unsplit(C, to_dev(c, DEV)), ref, bound)


# ---------------------------------------------------------------------------
# dense layout: cache_kv [2, B, H, MS, D], one "block" of MS positions per
# sequence, addressed by the strides masked_multihead_attention passes
# ---------------------------------------------------------------------------
DENSE_B, DENSE_H, DENSE_MS = 3, 4, 40
DENSE_LENS = [0, 17, 40]


@functools.lru_cache(maxsize=None)
def dense_case(D):
    """(q, cache_kv, table, lens on the device; ref, bound).  Rows >= len
    hold large finite values, so reading one is a wrong number."""
    B, H, MS = DENSE_B, DENSE_H, DENSE_MS
    g = torch.Generator().manual_seed(300 + D)
    cache = torch.randn(2, B, H, MS, D, generator=g)
    cache = (cache * torch.randn(2, B, H, MS, 1, generator=g).exp()).to(BF16)
    for b, S in enumerate(DENSE_LENS):
        cache[0, b, :, S:] = 3.0e4
        cache[1, b, :, S:] = -3.0e4
    q = torch.randn(B, H, D, generator=g).to(BF16)
    table = torch.arange(B, dtype=torch.int32).reshape(B, 1)
    lens = torch.tensor(DENSE_LENS, dtype=torch.int32)
    # the same cache as a paged pool [nblocks = B, bs = MS, HKV = H, D]
    kp, vp = (cache[i].permute(0, 2, 1, 3).contiguous() for i in (0, 1))
    ref, bound = ref_attn_bf16(q, kp, vp, table, lens)
    return tuple(t.to(DEV) for t in (q, cache, table, lens)) + (ref, bound)


def dense_strides(H, MS, D):
    return H * MS * D, D, MS * D, MS


@pytest.mark.gpu
@pytest.mark.parametrize("D", [64, 128])
def test_decode_attention_dense_layout_gpu(D):
    q, cache, table, lens, ref, bound = dense_case(D)
    out = _C().decode_attention(q, cache[0], cache[1], table, lens,
                                1.0 / math.sqrt(D),
                                *dense_strides(DENSE_H, DENSE_MS, D))
    assert bool((out[0] == 0).all()), "S = 0 must give zeros"
    check(f"dense D{D}", out, ref, bound)


@pytest.mark.gpu
def test_masked_multihead_attention_native_matches_torch_gpu(monkeypatch):
    """End to end through the dense strides, against the op's torch path at
    the bf16 tolerance of test_paged_decode_attention_gpu (3e-2)."""
    import paddle_amd as paddle
    from paddle_amd.incubate.nn import functional as inf
    B, H, MS, D = DENSE_B, DENSE_H, DENSE_MS, 128
    g = torch.Generator().manual_seed(17)
    cache = torch.randn(2, B, H, MS, D, generator=g).to(BF16).to(DEV)
    x = torch.randn(B, 3 * H * D, generator=g).to(BF16).to(DEV)
    lens = torch.tensor([0, 16, MS - 1], dtype=torch.int32, device=DEV)
    C = _C()
    calls = []
    real = C.decode_attention
    monkeypatch.setattr(C, "decode_attention",
                        lambda *a, **k: calls.append(1) or real(*a, **k))
    out, c1 = inf.masked_multihead_attention(x, cache.clone(),
                                             sequence_lengths=lens)
    assert calls == [1]
    paddle.set_flags({"FLAGS_use_native_kernels": False})
    try:
        ref, c2 = inf.masked_multihead_attention(x, cache.clone(),
                                                 sequence_lengths=lens)
    finally:
        paddle.set_flags({"FLAGS_use_native_kernels": True})
    assert calls == [1] and torch.equal(c1, c2)
    assert out.dtype == BF16 and tuple(out.shape) == (B, H * D)
    torch.testing.assert_close(out.float(), ref.float(), atol=3e-2, rtol=3e-2)


# ---------------------------------------------------------------------------
# contract: every check raises before any launch
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_decode_attention_contract_gpu():
    C = _C()
    c, _, _ = edge_case("bf16", 128, 8, 2, 16)
    q, kc, vc, tb, ln = (c[n] for n in ("q", "kc", "vc", "table", "lens"))
    HKV, D = kc.shape[2], kc.shape[3]
    sc = 1.0 / math.sqrt(D)
    f = C.decode_attention
    q32 = torch.zeros(q.shape[0], q.shape[1], 32, dtype=BF16, device=DEV)
    k32 = torch.zeros(kc.shape[0], kc.shape[1], HKV, 32, dtype=BF16, device=DEV)
    dq, dcache, dtb, dln, _, _ = dense_case(D)
    dk, dv = dcache[0], dcache[1]
    blk, pos, head, ms = dense_strides(DENSE_H, DENSE_MS, D)
    bad = {
        "q on cpu": lambda: f(q.cpu(), kc, vc, tb, ln, sc),
        "q fp32": lambda: f(q.float(), kc, vc, tb, ln, sc),
        "q strided": lambda: f(q.transpose(0, 1).contiguous().transpose(0, 1),
                               kc, vc, tb, ln, sc),
        "q 2-D": lambda: f(q[0], kc, vc, tb, ln, sc),
        "D 32": lambda: f(q32, k32, k32.clone(), tb, ln, sc),
        "cache fp32": lambda: f(q, kc.float(), vc.float(), tb, ln, sc),
        "cache int8": lambda: f(q, kc.to(torch.int8), vc.to(torch.int8), tb,
                                ln, sc),
        "cache on cpu": lambda: f(q, kc.cpu(), vc, tb, ln, sc),
        "cache strided": lambda: f(
            q, kc.transpose(1, 2).contiguous().transpose(1, 2), vc, tb, ln, sc),
        "cache shapes differ": lambda: f(q, kc, vc[:-1], tb, ln, sc),
        "cache D != q D": lambda: f(q[..., :64].contiguous(), kc, vc, tb, ln, sc),
        "H % HKV": lambda: f(q[:, :7].contiguous(), kc, vc, tb, ln, sc),
        "table int64": lambda: f(q, kc, vc, tb.long(), ln, sc),
        "table rows": lambda: f(q, kc, vc, tb[:-1], ln, sc),
        "table strided": lambda: f(q, kc, vc, tb[:, ::2], ln, sc),
        "lens int64": lambda: f(q, kc, vc, tb, ln.long(), sc),
        "lens length": lambda: f(q, kc, vc, tb, ln[:-1], sc),
        "lens on cpu": lambda: f(q, kc, vc, tb, ln.cpu(), sc),
        "dense blk stride 0": lambda: f(dq, dk, dv, dtb, dln, sc, 0, pos, head, ms),
        "dense pos stride 0": lambda: f(dq, dk, dv, dtb, dln, sc, blk, 0, head, ms),
        "dense bs 0": lambda: f(dq, dk, dv, dtb, dln, sc, blk, pos, head, 0),
        "dense negative": lambda: f(dq, dk, dv, dtb, dln, sc, -blk, pos, head, ms),
        "dense misaligned": lambda: f(dq, dk, dv, dtb, dln, sc, blk, pos + 4,
                                      head, ms),
        "dense bs past numel": lambda: f(dq, dk, dv, dtb, dln, sc, blk, pos,
                                         head, ms + 1),
        "dense stride past numel": lambda: f(dq, dk, dv, dtb, dln, sc, blk,
                                             2 * pos, head, ms),
        "paged with bs": lambda: f(q, kc, vc, tb, ln, sc, 0, 0, 0, 16),
    }
    good = f(q, kc, vc, tb, ln, sc)
    dgood = f(dq, dk, dv, dtb, dln, sc, blk, pos, head, ms)
    for name, fn in bad.items():
        with pytest.raises(RuntimeError, match="decode_attention"):
            fn()
            pytest.fail(f"{name}: no error")
        assert torch.equal(f(q, kc, vc, tb, ln, sc), good), name
    assert torch.equal(f(dq, dk, dv, dtb, dln, sc, blk, pos, head, ms), dgood)
    torch.cuda.synchronize()
