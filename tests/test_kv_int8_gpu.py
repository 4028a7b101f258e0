"""int8 paged KV cache on the GPU: the kv_quant_append kernel, the
decode_attention_int8 binding, the paged_decode_attention dispatch, the
bindings' contract, hipGraph capture and the serving runners.

Reference (independent of the code under test): this file packs and unpacks
the documented storage format itself --

    codes  int8 [nblocks, bs, HKV, D] in [-127, 127]
    per token: scale fp32 [nblocks, bs, HKV], d = absmax(row) * fp32(1/127),
               code = clamp(rint(x / d), +-127); a zero row has d = 0, codes 0
    per head:  code = clamp(rint(x * qs[h]), +-127), dequant step ds[h]
    x^ = code * scale

-- and ref_attn computes softmax(scale * q k^^T) v^ in fp64 from the bf16 q and
the STORED codes and scales, so quantisation error is not part of the
kernel's tolerance.

Attention bound (the row-kernel convention of docs/KERNELS.md):

    |out - ref| <= 2^-7 |ref| + 4 E + 2^-22 A

  2^-7   one bf16 ulp for the output cast,
  E      max over the (b, h) output row of |the same formula evaluated by
         torch in fp32 - fp64| on the same inputs: the error any fp32
         evaluation makes; 4x admits a different summation order, the scale
         folded into q and the approximate exp,
  A      sum_pos p |v^|: fp32 rounding of the PV products and of the slot
         merge.

Quantiser bound, in fp64: |code - x/d| <= 0.5 + 127 * 2^-22 (one hardware
reciprocal ulp plus two fp32 roundings on a value <= 127; admits either tie
direction), |code| <= 127, the absmax element has |code| = 127.

Compared with <=, never by ratio.  The helpers are shared with
test_kv_int8_cpu.py, which shows on a CPU emulation of the kernel's design
that the bound accepts it and rejects the mistakes such a kernel can make.
"""
import functools
import math

import pytest
import torch

DEV = "cuda:0"
BF16, F32, F64, I8 = torch.bfloat16, torch.float32, torch.float64, torch.int8
U_BF16 = 2.0 ** -7
Q_MARGIN = 0.5 + 127 * 2.0 ** -22
LENS = [1, 7, 8, 9, 31, 32, 33, 250]
POISON_CODE, POISON_SCALE = 127, 3.0e4


# ---------------------------------------------------------------------------
# the documented format, written out independently of paddle_amd
# ---------------------------------------------------------------------------
def ref_quant(x, qs=None):
    """x bf16 [..., HKV, D] -> (codes int8, d fp32 [..., HKV] | None)."""
    xf = x.to(F32)
    if qs is None:
        d = xf.abs().amax(-1) * torch.tensor(1.0 / 127.0, dtype=F32)
        safe = torch.where(d == 0, torch.ones_like(d), d)
        y = xf / safe.unsqueeze(-1)
    else:
        d = None
        y = xf * qs.to(F32).reshape(*([1] * (x.dim() - 2)), -1, 1)
    return torch.round(y).clamp(-127, 127).to(I8), d


def quant_violations(codes, x, d=None, qs=None):
    """Number of elements outside the quantiser bound (fp64)."""
    c = codes.to(F64)
    xd = x.to(F64)
    bad = int((c.abs() > 127).sum())
    if qs is None:
        dd = d.to(F64).unsqueeze(-1)
        y = torch.where(dd > 0, xd / torch.where(dd > 0, dd, torch.ones_like(dd)),
                        torch.zeros_like(xd))
        am = xd.abs().amax(-1, keepdim=True)
        at_max = (xd.abs() == am) & (am > 0)
        bad += int((at_max & (c.abs() != 127)).sum())
        bad += int(((dd == 0) & (c != 0)).sum())
    else:
        y = (xd * qs.to(F64).reshape(*([1] * (x.dim() - 2)), -1, 1)
             ).clamp(-127, 127)
    return bad + int(((c - y).abs() > Q_MARGIN).sum())


def _scale_rows(sc, blocks, S, hkv):
    if sc.dim() == 3:
        return sc[blocks].reshape(-1, hkv)[:S]
    return sc.reshape(1, hkv).expand(S, hkv)


def _attn_one(q, kc, vc, ks, vs, table, lens, scale, dt):
    """softmax(scale q k^^T) v^ per (b, h) in dtype dt -> (out, A)."""
    B, H, D = q.shape
    bs, HKV = kc.shape[1], kc.shape[2]
    rep = H // HKV
    out = torch.zeros(B, H, D, dtype=dt)
    A = torch.zeros(B, H, D, dtype=dt)
    for b in range(B):
        S = int(lens[b])
        if S == 0:
            continue
        blocks = table[b, :(S + bs - 1) // bs].long()
        kh = (kc[blocks].reshape(-1, HKV, D)[:S].to(dt)
              * _scale_rows(ks, blocks, S, HKV).to(dt).unsqueeze(-1))
        vh = (vc[blocks].reshape(-1, HKV, D)[:S].to(dt)
              * _scale_rows(vs, blocks, S, HKV).to(dt).unsqueeze(-1))
        kh = kh.repeat_interleave(rep, dim=1)          # [S, H, D]
        vh = vh.repeat_interleave(rep, dim=1)
        s = torch.einsum("hd,shd->hs", q[b].to(dt), kh) * scale
        p = torch.softmax(s, dim=-1)
        out[b] = torch.einsum("hs,shd->hd", p, vh)
        A[b] = torch.einsum("hs,shd->hd", p, vh.abs())
    return out, A


def ref_attn(q, kc, vc, ks, vs, table, lens, scale=None):
    """(ref fp64 [B, H, D], bound fp64 [B, H, D]) on CPU copies."""
    q, kc, vc, ks, vs, table, lens = (t.cpu() for t in
                                      (q, kc, vc, ks, vs, table, lens))
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    ref, A = _attn_one(q, kc, vc, ks, vs, table, lens, scale, F64)
    r32, _ = _attn_one(q, kc, vc, ks, vs, table, lens, scale, F32)
    E = (r32.to(F64) - ref).abs().amax(-1, keepdim=True)
    return ref, U_BF16 * ref.abs() + 4 * E + 2.0 ** -22 * A


def violations(out, ref, bound):
    return int(((out.detach().cpu().to(F64) - ref).abs() > bound).sum())


def check(name, out, ref, bound):
    err = (out.detach().cpu().to(F64) - ref).abs()
    n = int((err > bound).sum())
    worst = float((err / bound.clamp_min(1e-300)).max()) if n else 0.0
    assert n == 0, f"{name}: {n}/{err.numel()} outside the bound (worst {worst:.3g}x)"
    assert bool(torch.isfinite(out.float()).all()), f"{name}: non-finite output"


# ---------------------------------------------------------------------------
# cases: a paged pool where every wrong read is a wrong number, not a fault
# ---------------------------------------------------------------------------
def make_rows(S, HKV, D, g):
    """K/V rows [S, HKV, D] bf16 whose row magnitudes span exp(randn)."""
    def rows():
        x = torch.randn(S, HKV, D, generator=g)
        return (x * torch.randn(S, HKV, 1, generator=g).exp()).to(BF16)
    return rows(), rows()


def make_case(D, H, HKV, bs, lens, seed, static=False, rows=None):
    """CPU tensors of one batch.  Blocks in randperm order; the last block
    (index nblocks - 1) is poison: unused table entries point at it, and so
    do the positions >= S of each sequence's last block (large finite codes
    and scales).  rows: optional {b: (k, v)} bf16 [S, HKV, D] overrides."""
    g = torch.Generator().manual_seed(seed)
    B = len(lens)
    nb = [(S + bs - 1) // bs for S in lens]
    max_blocks = max(nb + [1]) + 1
    nblocks = sum(nb) + 1
    perm = torch.randperm(nblocks - 1, generator=g)
    table = torch.full((B, max_blocks), nblocks - 1, dtype=torch.int32)
    kc = torch.full((nblocks, bs, HKV, D), POISON_CODE, dtype=I8)
    vc = torch.full((nblocks, bs, HKV, D), -POISON_CODE, dtype=I8)
    if static:
        kq = 127.0 / (4.0 + torch.arange(HKV, dtype=F32))
        vq = 127.0 / (6.0 - 0.5 * torch.arange(HKV, dtype=F32))
        ks, vs = 1.0 / kq, 1.0 / vq
    else:
        kq = vq = None
        ks = torch.full((nblocks, bs, HKV), POISON_SCALE, dtype=F32)
        vs = torch.full((nblocks, bs, HKV), POISON_SCALE, dtype=F32)
    used = 0
    for b, S in enumerate(lens):
        blocks = perm[used:used + nb[b]]
        used += nb[b]
        table[b, :nb[b]] = blocks.int()
        if S == 0:
            continue
        k, v = rows[b] if rows and b in rows else make_rows(S, HKV, D, g)
        pos = torch.arange(S)
        pb, po = blocks[pos // bs], pos % bs
        kcode, kd = ref_quant(k, kq)
        vcode, vd = ref_quant(v, vq)
        kc[pb, po], vc[pb, po] = kcode, vcode
        if not static:
            ks[pb, po], vs[pb, po] = kd, vd
    q = torch.randn(B, H, D, generator=g).to(BF16)
    return dict(q=q, kc=kc, vc=vc, ks=ks, vs=vs, table=table,
                lens=torch.tensor(lens, dtype=torch.int32), kq=kq, vq=vq)


def needle_case(D, H, HKV, bs, S, n, seed):
    """One sequence where K at position n is 8 q (of kv head's first q head)
    so it takes nearly all the weight, and V there is a distinct row."""
    g = torch.Generator().manual_seed(seed)
    k, v = (torch.randn(S, HKV, D, generator=g).to(BF16) for _ in range(2))
    q = torch.randn(1, H, D, generator=g).to(BF16)
    rep = H // HKV
    k[n] = (8.0 * q[0, ::rep].float()).to(BF16)
    v[n] = (3.0 + torch.arange(D).float() / D).to(BF16).expand(HKV, D)
    c = make_case(D, H, HKV, bs, [S], seed, rows={0: (k, v)})
    c["q"] = q
    return c


def case_ref(c, scale=None):
    return ref_attn(c["q"], c["kc"], c["vc"], c["ks"], c["vs"], c["table"],
                    c["lens"], scale)


def to_dev(c, dev):
    return {k: (v.to(dev) if isinstance(v, torch.Tensor) else v)
            for k, v in c.items()}


@functools.lru_cache(maxsize=None)
def gpu_case(D, H, HKV, bs, static=False):
    """(device tensors, ref, bound): computed once, shared, never modified."""
    c = make_case(D, H, HKV, bs, LENS, 1000 + D + 8 * HKV + bs, static)
    return (to_dev(c, DEV),) + case_ref(c)


def _C():
    from paddle_amd import _ext
    return _ext.get_ext(required=True)


def _run(C, c, scale=None):
    if scale is None:
        scale = 1.0 / math.sqrt(c["q"].shape[-1])
    return C.decode_attention_int8(c["q"], c["kc"], c["vc"], c["ks"], c["vs"],
                                   c["table"], c["lens"], scale)


# ---------------------------------------------------------------------------
# kv_quant_append
# ---------------------------------------------------------------------------
def append_inputs(T, HKV, D, bs, nblocks, seed, dev):
    """k/v as strided views of a fused qkv buffer; scattered unique slots
    that include offset bs - 1; row (0, 0) of k is all zero."""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(T, 3, HKV, D, generator=g)
    qkv = (qkv * torch.randn(T, 3, HKV, 1, generator=g).exp()).to(BF16)
    qkv[0, 1, 0] = 0
    slots = torch.randperm(nblocks * bs, generator=g)[:T]
    slots[T - 1] = (nblocks - 1) * bs + bs - 1 if T > 1 else bs - 1
    assert slots.unique().numel() == T
    qkv = qkv.to(dev)
    return (qkv[:, 1], qkv[:, 2], (slots // bs).to(dev), (slots % bs).to(dev))


APPEND_CASES = [(1, 1, 64), (5, 2, 128), (67, 2, 128), (67, 8, 64)]


@pytest.mark.gpu
@pytest.mark.parametrize("T,HKV,D", APPEND_CASES)
def test_kv_quant_append_dynamic_gpu(T, HKV, D):
    bs, nblocks = 16, 9
    k, v, blk, off = append_inputs(T, HKV, D, bs, nblocks, 7 * T + D, DEV)
    assert T == 1 or not k.is_contiguous()
    assert k.storage_offset() == HKV * D and k.stride(0) == 3 * HKV * D
    kc = torch.full((nblocks, bs, HKV, D), 0x55, dtype=I8, device=DEV)
    vc = kc.clone()
    ks = torch.full((nblocks, bs, HKV), -1.0, dtype=F32, device=DEV)
    vs = ks.clone()
    _C().kv_quant_append(k, v, kc, vc, ks, vs, blk, off)
    torch.cuda.synchronize()
    third = torch.tensor(1.0 / 127.0, dtype=F32, device=DEV)
    for x, cache, sc in ((k, kc, ks), (v, vc, vs)):
        d = sc[blk, off]
        assert torch.equal(d, x.float().abs().amax(-1) * third)
        assert quant_violations(cache[blk, off].cpu(), x.cpu(), d.cpu()) == 0
        written = torch.zeros(nblocks, bs, dtype=torch.bool, device=DEV)
        written[blk, off] = True
        assert bool((cache[~written] == 0x55).all())
        assert bool((sc[~written] == -1.0).all())
    # zero row: d = 0, codes 0, nothing non-finite
    assert float(ks[blk[0], off[0], 0]) == 0.0
    assert bool((kc[blk[0], off[0], 0] == 0).all())
    assert bool(torch.isfinite(ks).all() and torch.isfinite(vs).all())


@pytest.mark.gpu
@pytest.mark.parametrize("T,HKV,D", APPEND_CASES)
def test_kv_quant_append_fixed_gpu(T, HKV, D):
    bs, nblocks = 16, 9
    k, v, blk, off = append_inputs(T, HKV, D, bs, nblocks, 11 * T + D, DEV)
    kc = torch.full((nblocks, bs, HKV, D), 0x55, dtype=I8, device=DEV)
    vc = kc.clone()
    kq = (127.0 / (2.0 + torch.arange(HKV, dtype=F32))).to(DEV)   # clamps some
    vq = (127.0 / (9.0 - torch.arange(HKV, dtype=F32))).to(DEV)
    ks, vs = (1.0 / kq).contiguous(), (1.0 / vq).contiguous()
    ks0, vs0 = ks.clone(), vs.clone()
    _C().kv_quant_append(k, v, kc, vc, ks, vs, blk, off, kq, vq)
    torch.cuda.synchronize()
    assert torch.equal(ks, ks0) and torch.equal(vs, vs0)
    for x, cache, qs in ((k, kc, kq), (v, vc, vq)):
        assert quant_violations(cache[blk, off].cpu(), x.cpu(), qs=qs.cpu()) == 0
        written = torch.zeros(nblocks, bs, dtype=torch.bool, device=DEV)
        written[blk, off] = True
        assert bool((cache[~written] == 0x55).all())


# ---------------------------------------------------------------------------
# decode_attention_int8
# ---------------------------------------------------------------------------
ATTN_CASES = [(D, H, HKV, bs) for D in (64, 128)
              for (H, HKV) in ((8, 8), (8, 2), (8, 1)) for bs in (16, 24)]


@pytest.mark.gpu
@pytest.mark.parametrize("D,H,HKV,bs", ATTN_CASES)
def test_decode_attention_int8_gpu(D, H, HKV, bs):
    c, ref, bound = gpu_case(D, H, HKV, bs)
    out = _run(_C(), c)
    assert out.dtype == BF16 and tuple(out.shape) == (len(LENS), H, D)
    check(f"D{D} H{H} HKV{HKV} bs{bs}", out, ref, bound)


@pytest.mark.gpu
@pytest.mark.parametrize("D,H,HKV,bs", [(64, 8, 2, 16), (128, 8, 2, 24),
                                        (128, 8, 8, 16)])
def test_decode_attention_int8_static_scales_gpu(D, H, HKV, bs):
    c, ref, bound = gpu_case(D, H, HKV, bs, True)
    assert tuple(c["ks"].shape) == (HKV,)
    check(f"static D{D}", _run(_C(), c), ref, bound)


@pytest.mark.gpu
@pytest.mark.parametrize("D", [64, 128])
def test_decode_attention_int8_empty_and_zero_rows_gpu(D):
    """S = 0 gives zeros; all-zero K/V rows (d = 0, codes 0) stay finite."""
    H, HKV, bs = 8, 2, 16
    lens = [0, 5, 40, 0]
    z = {1: tuple(torch.zeros(5, HKV, D, dtype=BF16) for _ in range(2))}
    g = torch.Generator().manual_seed(5)
    k, v = make_rows(40, HKV, D, g)
    k[3] = 0
    v[3] = 0
    k[39] = 0
    z[2] = (k, v)
    c = make_case(D, H, HKV, bs, lens, 77 + D, rows=z)
    ref, bound = case_ref(c)
    out = _run(_C(), to_dev(c, DEV))
    assert bool((out[0] == 0).all() and (out[3] == 0).all())
    assert bool((out[1] == 0).all())          # V rows all zero
    check(f"zero rows D{D}", out, ref, bound)


NEEDLE_S = 70


@pytest.mark.gpu
@pytest.mark.parametrize("D,bs", [(128, 16), (64, 24)])
def test_decode_attention_int8_needle_gpu(D, bs):
    """The needle position takes nearly all the weight, so a position that
    is dropped, doubled or read from the wrong slot changes the output."""
    H, HKV, S = 8, 2, NEEDLE_S
    C = _C()
    for n in (0, 1, 7, 8, 31, 32, 33, S - 2, S - 1):
        c = needle_case(D, H, HKV, bs, S, n, 300 + n)
        ref, bound = case_ref(c)
        # the needle's V row dominates the reference
        assert float((ref[0, 0] - 3.0).abs().max()) < 1.5
        check(f"needle n={n} D{D}", _run(C, to_dev(c, DEV)), ref, bound)


# ---------------------------------------------------------------------------
# dispatch
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_paged_decode_attention_int8_dispatch_gpu(monkeypatch):
    import paddle_amd as paddle
    from paddle_amd.ops import functional as hot
    c, ref, bound = gpu_case(128, 8, 2, 16)
    C = _C()
    calls = []
    real = C.decode_attention_int8
    monkeypatch.setattr(C, "decode_attention_int8",
                        lambda *a: calls.append(1) or real(*a))
    args = (c["q"], c["kc"], c["vc"], c["table"], c["lens"])
    on = hot.paged_decode_attention(*args, k_scale=c["ks"], v_scale=c["vs"])
    assert calls == [1]
    paddle.set_flags({"FLAGS_use_native_kernels": False})
    try:
        off = hot.paged_decode_attention(*args, k_scale=c["ks"], v_scale=c["vs"])
    finally:
        paddle.set_flags({"FLAGS_use_native_kernels": True})
    assert calls == [1]
    check("native", on, ref, bound)
    check("torch path", off, ref, bound)
    # fp32 q is outside the kernel's contract: torch path
    f32 = hot.paged_decode_attention(c["q"].float(), *args[1:],
                                     k_scale=c["ks"], v_scale=c["vs"])
    assert calls == [1] and f32.dtype == F32


@pytest.mark.gpu
def test_paged_decode_attention_bf16_unchanged_gpu():
    """Without scales on a bf16 cache the call is today's kernel, bit for bit."""
    from paddle_amd.ops import functional as hot
    g = torch.Generator().manual_seed(3)
    B, H, HKV, D, bs = 3, 8, 2, 128, 16
    kc = torch.randn(12, bs, HKV, D, generator=g).to(BF16).to(DEV)
    vc = torch.randn(12, bs, HKV, D, generator=g).to(BF16).to(DEV)
    q = torch.randn(B, H, D, generator=g).to(BF16).to(DEV)
    table = torch.randperm(12, generator=g).int().reshape(B, 4).to(DEV)
    lens = torch.tensor([1, 33, 64], dtype=torch.int32, device=DEV)
    out = hot.paged_decode_attention(q, kc, vc, table, lens)
    assert torch.equal(out, _C().decode_attention(q, kc, vc, table, lens,
                                                  1.0 / math.sqrt(D)))
    with pytest.raises(ValueError):
        hot.paged_decode_attention(q, kc, vc, table, lens,
                                   k_scale=torch.ones(HKV, device=DEV))


# ---------------------------------------------------------------------------
# contract: every check raises before any launch
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_kv_int8_contract_gpu():
    C = _C()
    c, _, _ = gpu_case(128, 8, 2, 16)
    q, kc, vc, ks, vs, tb, ln = (c[n] for n in
                                 ("q", "kc", "vc", "ks", "vs", "table", "lens"))
    nblocks, bs, HKV, D = kc.shape
    sc = 1.0 / math.sqrt(D)
    hks = torch.ones(HKV, device=DEV)
    att = {
        "q on cpu": lambda: C.decode_attention_int8(q.cpu(), kc, vc, ks, vs, tb, ln, sc),
        "cache on cpu": lambda: C.decode_attention_int8(q, kc.cpu(), vc, ks, vs, tb, ln, sc),
        "lens on cpu": lambda: C.decode_attention_int8(q, kc, vc, ks, vs, tb, ln.cpu(), sc),
        "q fp32": lambda: C.decode_attention_int8(q.float(), kc, vc, ks, vs, tb, ln, sc),
        "q strided": lambda: C.decode_attention_int8(
            q.transpose(0, 1).contiguous().transpose(0, 1), kc, vc, ks, vs, tb, ln, sc),
        "q 2-D": lambda: C.decode_attention_int8(q[0], kc, vc, ks, vs, tb, ln, sc),
        "D 32": lambda: C.decode_attention_int8(
            q[..., :32].contiguous(), kc[..., :32].contiguous(),
            vc[..., :32].contiguous(), ks, vs, tb, ln, sc),
        "cache bf16": lambda: C.decode_attention_int8(
            q, kc.to(BF16), vc.to(BF16), ks, vs, tb, ln, sc),
        "cache strided": lambda: C.decode_attention_int8(
            q, kc.transpose(1, 2).contiguous().transpose(1, 2), vc, ks, vs, tb, ln, sc),
        "cache shapes differ": lambda: C.decode_attention_int8(
            q, kc, vc[:-1], ks, vs, tb, ln, sc),
        "cache D != q D": lambda: C.decode_attention_int8(
            q[..., :64].contiguous(), kc, vc, ks, vs, tb, ln, sc),
        "H % HKV": lambda: C.decode_attention_int8(
            q[:, :7].contiguous(), kc, vc, ks, vs, tb, ln, sc),
        "scale fp64": lambda: C.decode_attention_int8(
            q, kc, vc, ks.double(), vs.double(), tb, ln, sc),
        "scale shape": lambda: C.decode_attention_int8(
            q, kc, vc, ks[:, :-1].contiguous(), vs[:, :-1].contiguous(), tb, ln, sc),
        "scale kinds differ": lambda: C.decode_attention_int8(
            q, kc, vc, ks, hks, tb, ln, sc),
        "scale [HKV+1]": lambda: C.decode_attention_int8(
            q, kc, vc, torch.ones(HKV + 1, device=DEV),
            torch.ones(HKV + 1, device=DEV), tb, ln, sc),
        "table int64": lambda: C.decode_attention_int8(q, kc, vc, ks, vs, tb.long(), ln, sc),
        "table rows": lambda: C.decode_attention_int8(q, kc, vc, ks, vs, tb[:-1], ln, sc),
        "table strided": lambda: C.decode_attention_int8(
            q, kc, vc, ks, vs, tb[:, ::2], ln, sc),
        "lens int64": lambda: C.decode_attention_int8(q, kc, vc, ks, vs, tb, ln.long(), sc),
        "lens length": lambda: C.decode_attention_int8(q, kc, vc, ks, vs, tb, ln[:-1], sc),
    }
    T = 4
    qkv = torch.randn(T, 3, HKV, D, device=DEV).to(BF16)
    k, v = qkv[:, 1], qkv[:, 2]
    blk = torch.arange(T, device=DEV)
    off = torch.arange(T, device=DEV)
    kc2, vc2, ks2, vs2 = kc.clone(), vc.clone(), ks.clone(), vs.clone()
    odd = torch.randn(T, HKV * D + 4, device=DEV).to(BF16)
    app = {
        "k fp32": lambda: C.kv_quant_append(k.float(), v.float(), kc2, vc2, ks2, vs2, blk, off),
        "k on cpu": lambda: C.kv_quant_append(k.cpu(), v.cpu(), kc2, vc2, ks2, vs2, blk, off),
        "k 2-D": lambda: C.kv_quant_append(k[0], v[0], kc2, vc2, ks2, vs2, blk, off),
        "k HKV": lambda: C.kv_quant_append(k[:, :1], v[:, :1], kc2, vc2, ks2, vs2, blk, off),
        "k D": lambda: C.kv_quant_append(k[..., :64], v[..., :64], kc2, vc2, ks2, vs2, blk, off),
        "v T": lambda: C.kv_quant_append(k, v[:-1], kc2, vc2, ks2, vs2, blk, off),
        "k D strided": lambda: C.kv_quant_append(
            k.transpose(1, 2).contiguous().transpose(1, 2), v, kc2, vc2, ks2, vs2, blk, off),
        "k token stride % 8": lambda: C.kv_quant_append(
            odd[:, :HKV * D].reshape(T, HKV, D), v, kc2, vc2, ks2, vs2, blk, off),
        "k misaligned": lambda: C.kv_quant_append(
            odd.reshape(-1)[4:4 + T * HKV * D].reshape(T, HKV, D), v, kc2, vc2,
            ks2, vs2, blk, off),
        "cache bf16": lambda: C.kv_quant_append(
            k, v, kc2.to(BF16), vc2.to(BF16), ks2, vs2, blk, off),
        "scale shape": lambda: C.kv_quant_append(
            k, v, kc2, vc2, ks2[:-1], vs2[:-1], blk, off),
        "blk int32": lambda: C.kv_quant_append(k, v, kc2, vc2, ks2, vs2, blk.int(), off),
        "off length": lambda: C.kv_quant_append(k, v, kc2, vc2, ks2, vs2, blk, off[:-1]),
        "blk on cpu": lambda: C.kv_quant_append(k, v, kc2, vc2, ks2, vs2, blk.cpu(), off),
        "one quant scale": lambda: C.kv_quant_append(
            k, v, kc2, vc2, hks, hks.clone(), blk, off, hks),
        "quant scales with per-token pools": lambda: C.kv_quant_append(
            k, v, kc2, vc2, ks2, vs2, blk, off, hks, hks),
        "per-head pools without quant scales": lambda: C.kv_quant_append(
            k, v, kc2, vc2, hks, hks.clone(), blk, off),
        "quant scale shape": lambda: C.kv_quant_append(
            k, v, kc2, vc2, hks, hks.clone(), blk, off,
            torch.ones(HKV + 1, device=DEV), torch.ones(HKV + 1, device=DEV)),
    }
    for name, fn in {**att, **app}.items():
        with pytest.raises(RuntimeError):
            fn()
            pytest.fail(f"{name}: no error")
    torch.cuda.synchronize()
    # nothing was launched: the pools are untouched
    assert torch.equal(kc2, kc) and torch.equal(ks2, ks)


# ---------------------------------------------------------------------------
# hipGraph: append + attention captured on one stream, inputs changed in place
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_kv_int8_graph_gpu():
    C = _C()
    D, H, HKV, bs = 128, 8, 2, 16
    c = to_dev(make_case(D, H, HKV, bs, [20, 45, 3], 21), DEV)
    B = 3
    sc = 1.0 / math.sqrt(D)
    g = torch.Generator().manual_seed(9)

    def fresh():
        qkv = torch.randn(B, H + 2 * HKV, D, generator=g).to(BF16).to(DEV)
        lens = c["lens"].clone()
        table = c["table"].clone()
        return qkv, lens, table

    def step(qkv, lens, table, blk, off, pools):
        kc, vc, ks, vs = pools
        C.kv_quant_append(qkv[:, H:H + HKV], qkv[:, H + HKV:], kc, vc, ks, vs,
                          blk, off)
        return C.decode_attention_int8(qkv[:, :H].contiguous(), kc, vc, ks, vs,
                                       table, lens, sc)

    def write_slots(lens, table):
        pos = (lens - 1).long()
        return (table.long().gather(1, (pos // bs).unsqueeze(1)).squeeze(1),
                pos % bs)

    pools = tuple(c[n].clone() for n in ("kc", "vc", "ks", "vs"))
    qkv, lens, table = fresh()
    lens += 1
    blk, off = write_slots(lens, table)
    st = dict(qkv=qkv.clone(), lens=lens.clone(), table=table.clone(),
              blk=blk.clone(), off=off.clone())
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        step(st["qkv"], st["lens"], st["table"], st["blk"], st["off"], pools)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_g = step(st["qkv"], st["lens"], st["table"], st["blk"], st["off"],
                     pools)
    # new inputs, longer sequences, another write slot, a permuted table row
    qkv2, lens2, table2 = fresh()
    lens2 += 2
    table2[0, :2] = table2[0, :2].flip(0)
    blk2, off2 = write_slots(lens2, table2)
    for k_, v_ in (("qkv", qkv2), ("lens", lens2), ("table", table2),
                   ("blk", blk2), ("off", off2)):
        st[k_].copy_(v_)
    for p, n in zip(pools, ("kc", "vc", "ks", "vs")):
        p.copy_(c[n])
    graph.replay()
    torch.cuda.synchronize()
    eager_pools = tuple(c[n].clone() for n in ("kc", "vc", "ks", "vs"))
    eager = step(qkv2, lens2, table2, blk2, off2, eager_pools)
    assert torch.equal(out_g, eager)
    assert all(torch.equal(a, b) for a, b in zip(pools, eager_pools))
    ref, bound = ref_attn(qkv2[:, :H].contiguous(), *eager_pools, table2, lens2)
    check("graph replay", out_g, ref, bound)


# ---------------------------------------------------------------------------
# runners: D = 64 variants of the tiny presets so the kernels run
# ---------------------------------------------------------------------------
def _serve(runner_cls, model, use_graphs, prompts):
    from paddle_amd.serving import Engine, Request
    runner = runner_cls(model, num_blocks=64, block_size=16, max_seq=128,
                        use_graphs=use_graphs, kv_cache="int8")
    assert runner.use_graphs == use_graphs
    assert all(p.dtype == I8 for p in runner.k + runner.v)
    assert all(tuple(s.shape) == (65, 16, runner.HKV) and s.dtype == F32
               for s in runner.k_scale + runner.v_scale)
    eng = Engine(runner, num_blocks=64, block_size=16, max_batch=4)
    reqs = [Request(prompt_ids=p, max_new_tokens=8) for p in prompts]
    for r in reqs:
        eng.add_request(r)
    eng.run_until_done()
    assert all(r.done and len(r.out_ids) == 8 for r in reqs)
    assert len(eng.alloc.free) == 64
    assert any(bool((p != 0).any()) for p in runner.k)
    return [r.out_ids for r in reqs]


PROMPTS = [[3, 7, 11, 2], [5, 9, 4, 8, 15, 16, 23], list(range(20, 53)),
           [3, 7, 11, 2]]


@pytest.mark.gpu
def test_gpt_runner_int8_kv_gpu():
    import paddle_amd as paddle
    from paddle_amd.models import build_gpt
    from paddle_amd.serving import GPTModelRunner
    paddle.seed(0)
    m = build_gpt("gpt3-tiny", num_heads=2, max_seq_len=128).to("cuda", BF16)
    a = _serve(GPTModelRunner, m, True, PROMPTS)
    b = _serve(GPTModelRunner, m, False, PROMPTS)
    assert a == b


@pytest.mark.gpu
def test_llama_runner_int8_kv_gpu():
    import paddle_amd as paddle
    from paddle_amd.models.llama import build_llama
    from paddle_amd.serving import LlamaModelRunner
    paddle.seed(0)
    m = build_llama("llama-tiny", num_heads=2, num_kv_heads=1,
                    max_seq_len=128).to("cuda", BF16).eval()
    a = _serve(LlamaModelRunner, m, True, PROMPTS)
    b = _serve(LlamaModelRunner, m, False, PROMPTS)
    assert a == b
