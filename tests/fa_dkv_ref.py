"""Shared by test_fa_dkv_cpu.py and test_fa_dkv_gpu.py: inputs, the fp64
reference of the flash-attention dK/dV backward, its bound, and a torch
emulation of the kernel's design (csrc/kernels/fa_bwd.hip,
fa_bwd_dkv_kernel).  Everything here runs on the CPU.

Reference, from the bf16 inputs (upcast, so exactly what the kernel reads):
    S = scale * Q K^T          P = exp(S - lse)   (lse: the fp32 one passed in)
    delta = rowsum(dO * O)     (O: the bf16 one passed in)
    dS = P * (dO V^T - delta) * scale
    dV = P^T dO                dK = dS^T Q
Bound (docs/KERNELS.md, "kernel contract and tolerances"):
    |out - ref| <= 2^-7*|ref| + 2^-7*A + 4*E
    A_dV = sum_q P*|dO|, A_dK = sum_q |dS|*|Q|: one bf16 ulp on every P / dS
        element, which the kernel rounds to bf16 before the second product
    E = max |formulas in fp32 torch - formulas in fp64| on the same inputs
"""
import functools
import math

import torch

BF16 = torch.bfloat16
U = 2.0 ** -7
QB, KVB = 64, 128   # q tile rows, kv rows per block: the kernel's tiling

# (B, H, Sq, Skv, D, causal)
SHAPES = [
    (1, 1, 40, 40, 128, True),      # only a guarded tile
    (1, 1, 64, 64, 128, True),      # prologue only
    (1, 2, 192, 192, 128, True),    # odd tile count; 2nd kv block starts at its own q_start
    (1, 2, 256, 256, 128, True),    # even tile count
    (1, 2, 256, 256, 128, False),
    (2, 3, 200, 200, 128, True),    # DMA tiles, then a guarded tail; partial kv block
    (2, 3, 200, 200, 128, False),
    (1, 1, 320, 136, 128, False),   # Sq != Skv, 8-row kv tail
    (1, 2, 192, 192, 64, True),
    (1, 2, 200, 264, 64, False),
]


def shape_id(s):
    return "b%d_h%d_sq%d_skv%d_d%d_%s" % (s[0], s[1], s[2], s[3], s[4], "causal" if s[5] else "full")


def _mask(sq, skv, causal):
    if not causal:
        return None
    return torch.arange(skv)[None, :] > torch.arange(sq)[:, None]   # True = masked out


def formulas(q, k, v, do, o, lse, scale, causal):
    """dV, dK and the A terms in the dtype of the inputs ([B, H, S, D])."""
    s = torch.matmul(q, k.transpose(-1, -2)) * scale
    p = torch.exp(s - lse.to(s.dtype)[..., None])
    m = _mask(q.shape[2], k.shape[2], causal)
    if m is not None:
        p = p.masked_fill(m, 0.0)
    delta = (do * o).sum(-1, keepdim=True)
    ds = p * (torch.matmul(do, v.transpose(-1, -2)) - delta) * scale
    pt, dst = p.transpose(-1, -2), ds.transpose(-1, -2)
    return {"dv": torch.matmul(pt, do), "dk": torch.matmul(dst, q),
            "A_dv": torch.matmul(pt, do.abs()), "A_dk": torch.matmul(dst.abs(), q.abs())}


@functools.lru_cache(maxsize=None)
def case(shape):
    """Inputs (bf16 / fp32 lse, CPU), fp64 reference, E and the bounds.
    Computed once per shape and shared; callers must not modify it."""
    b, h, sq, skv, d, causal = shape
    g = torch.Generator().manual_seed(1000 + sq * 7 + skv * 3 + d + int(causal))
    q = torch.randn((b, h, sq, d), generator=g).to(BF16)
    k = torch.randn((b, h, skv, d), generator=g).to(BF16)
    v = torch.randn((b, h, skv, d), generator=g).to(BF16)
    do = torch.randn((b, h, sq, d), generator=g).to(BF16)
    scale = 1.0 / math.sqrt(d)
    # forward in fp64: lse to fp32, O to bf16, as the forward kernel stores them
    s = torch.matmul(q.double(), k.double().transpose(-1, -2)) * scale
    m = _mask(sq, skv, causal)
    if m is not None:
        s = s.masked_fill(m, float("-inf"))
    lse = torch.logsumexp(s, -1).float()
    o = torch.matmul(torch.softmax(s, -1), v.double()).to(BF16)
    args = (q, k, v, do, o)
    r64 = formulas(*[t.double() for t in args], lse, scale, causal)
    r32 = formulas(*[t.float() for t in args], lse, scale, causal)
    E = {n: float((r32[n].double() - r64[n]).abs().max()) for n in ("dv", "dk")}
    bound = {n: U * r64[n].abs() + U * r64["A_" + n] + 4 * E[n] for n in ("dv", "dk")}
    return {"q": q, "k": k, "v": v, "do": do, "o": o, "lse": lse, "scale": scale,
            "causal": causal, "r64": r64, "r32": r32, "E": E, "bound": bound}


def worst(c, name, out):
    """largest err/bound of `out` ([B, H, Skv, D]) against the case's reference"""
    err = (out.detach().double().cpu() - c["r64"][name]).abs()
    ratio = err / c["bound"][name]
    return float(ratio.nan_to_num(nan=float("inf")).max())


# the mistakes test_fa_dkv_cpu.py plants in the emulation
MISTAKES = ("b_halves_swapped", "chunks_swapped", "stale_buffer", "last_tile_dropped",
            "q_start_late")


def emulate(c, mistake=None):
    """fp32 torch emulation of the kernel: 128-row kv blocks, 64-row q tiles
    from the causal q_start, P and dS rounded to bf16 before the dV / dK
    products, fp32 accumulation, bf16 outputs.  `mistake` plants one of
    MISTAKES; returns (dv, dk, applied) with applied = the mistake changed
    which data some product saw."""
    assert mistake is None or mistake in MISTAKES
    q, k, v, do, o = (c[n].float() for n in ("q", "k", "v", "do", "o"))
    lse, scale, causal = c["lse"], c["scale"], c["causal"]
    b, h, sq, d = q.shape
    skv = k.shape[2]
    delta = (do * o).sum(-1)
    dv, dk = torch.zeros_like(v), torch.zeros_like(k)
    applied = False

    def b_operand(t):
        """the [64][D] tile as the transposed reads deliver it to dV / dK"""
        if mistake == "b_halves_swapped":     # rows 8g+4..7 before 8g+0..3
            return t[..., torch.arange(QB) ^ 4, :]
        if mistake == "chunks_swapped":       # 16-byte chunks of a 32-byte pair, rows with (row>>2)&1
            sw = t[..., torch.arange(d) ^ 8]
            odd = ((torch.arange(QB) >> 2) & 1).bool()[:, None]
            return torch.where(odd, sw, t)
        return t

    def tile(t, q0):
        out = torch.zeros((b, h, QB) + t.shape[3:], dtype=t.dtype)
        n = max(0, min(QB, sq - q0))
        out[:, :, :n] = t[:, :, q0:q0 + n]
        return out

    for kv0 in range(0, skv, KVB):
        nkv = min(KVB, skv - kv0)
        kb, vb = k[:, :, kv0:kv0 + nkv], v[:, :, kv0:kv0 + nkv]
        q_start = (kv0 // QB) * QB if causal else 0
        if mistake == "q_start_late" and causal:
            q_start += QB
            applied = True
        starts = list(range(q_start, sq, QB))
        if mistake == "last_tile_dropped" and starts:
            starts.pop()
            applied = True
        for i, q0 in enumerate(starts):
            qt, dot = tile(q, q0), tile(do, q0)
            rows = q0 + torch.arange(QB)
            lse_t = tile(lse[..., None], q0)[..., 0]
            lse_t[..., rows >= sq] = float("inf")
            dl_t = tile(delta[..., None], q0)[..., 0]
            st = torch.matmul(kb, qt.transpose(-1, -2))            # [nkv, 64]
            p = torch.exp(st * scale - lse_t[:, :, None, :])
            kv_abs = kv0 + torch.arange(nkv)
            dead = (rows >= sq)[None, :].expand(nkv, QB).clone()
            if causal:
                dead |= kv_abs[:, None] > rows[None, :]
            p = p.masked_fill(dead, 0.0)
            qb_, dob_ = qt, dot
            if mistake == "stale_buffer" and i == 1:
                qb_, dob_ = tile(q, starts[0]), tile(do, starts[0])
                applied = True
            if mistake in ("b_halves_swapped", "chunks_swapped"):
                applied = True
            dv[:, :, kv0:kv0 + nkv] += torch.matmul(p.to(BF16).float(), b_operand(dob_))
            dp = torch.matmul(vb, dot.transpose(-1, -2))
            ds = p * (dp - dl_t[:, :, None, :]) * scale
            dk[:, :, kv0:kv0 + nkv] += torch.matmul(ds.to(BF16).float(), b_operand(qb_))
    return dv.to(BF16), dk.to(BF16), applied
