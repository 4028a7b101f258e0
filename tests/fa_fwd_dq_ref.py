"""Shared by test_fa_fwd_dq_cpu.py and test_fa_fwd_dq_gpu.py: inputs, the fp64
reference of the flash-attention forward (O, LSE) and of dQ, their bounds,
and a torch emulation of the design of the two kernels
(csrc/kernels/fa_fwd32.hip fa_fwd32_kernel, csrc/kernels/fa_bwd.hip
fa_bwd_dq32_kernel).  Everything here runs on the CPU.

Reference, from the values the kernels read and the rounding their design
documents (Q pre-scaled once, in fp32, and rounded to bf16; exact at D = 64):
    q~ = bf16(q * scale)       S = q~ K^T         (causal: kv <= q)
    lse = logsumexp(S)         O = softmax(S) V
    P = exp(S - lse)           delta = rowsum(dO * O)
    dS = P * (dO V^T - delta) * scale             dQ = dS K
For dQ, lse (fp32) and O (bf16) are the ones passed in: those of the fp64
forward, so dQ is tested on its own.
Bound (docs/KERNELS.md, "kernel contract and tolerances"):
    |out - ref| <= 2^-7*|ref| + 2^-7*A + 4*E           (O, dQ: bf16)
    A_o = sum_kv P*|V|, A_dq = sum_kv |dS|*|K|: one bf16 ulp on every P / dS
        element, which the kernels round to bf16 before the second product
    |lse - ref| <= 4*E + 2^-22*(1 + |ref|)             (fp32, as the lse of
        softmax_cross_entropy: v_log and the final add)
    E = max |formulas in fp32 torch - formulas in fp64| on the same inputs
"""
import functools
import math

import torch

BF16 = torch.bfloat16
U = 2.0 ** -7
EPS = 2.0 ** -22
QB, KB, WQ = 128, 64, 32   # q rows per block, kv tile rows, q rows per wave
THR = 8.0                  # deferred-maximum threshold of the forward

# (B, H, Sq, Skv, D, causal)
SHAPES = [
    (1, 1, 40, 40, 128, True),      # only a guarded tile
    (1, 1, 64, 64, 128, True),      # one DMA tile, no prefetch
    (1, 2, 128, 128, 128, True),    # both buffers
    (1, 2, 192, 192, 128, True),    # buffer 0 reused; 2nd q block half empty
    (2, 3, 200, 200, 128, True),    # DMA tiles, then a guarded tail in the other buffer
    (2, 3, 200, 200, 128, False),
    (1, 1, 320, 136, 128, False),   # Sq != Skv, 8-row kv tail
    (1, 2, 192, 192, 64, True),     # D = 64 image
    (1, 2, 200, 264, 64, False),
]
OUTPUTS = ("o", "lse", "dq")


def shape_id(s):
    return "b%d_h%d_sq%d_skv%d_d%d_%s" % (s[0], s[1], s[2], s[3], s[4], "causal" if s[5] else "full")


def _mask(sq, skv, causal):
    if not causal:
        return None
    return torch.arange(skv)[None, :] > torch.arange(sq)[:, None]   # True = masked out


def prescale(q, scale):
    """q~ as the kernels build it: fp32 product, rounded to bf16"""
    return (q.float() * scale).to(BF16)


def fwd_formulas(qt, k, v, causal):
    """lse, O and A_o in the dtype of the inputs ([B, H, S, D]); qt = q~"""
    s = torch.matmul(qt, k.transpose(-1, -2))
    m = _mask(qt.shape[2], k.shape[2], causal)
    if m is not None:
        s = s.masked_fill(m, float("-inf"))
    p = torch.softmax(s, -1)
    return {"lse": torch.logsumexp(s, -1), "o": torch.matmul(p, v),
            "A_o": torch.matmul(p, v.abs())}


def dq_formulas(qt, k, v, do, o, lse, scale, causal):
    s = torch.matmul(qt, k.transpose(-1, -2))
    p = torch.exp(s - lse.to(s.dtype)[..., None])
    m = _mask(qt.shape[2], k.shape[2], causal)
    if m is not None:
        p = p.masked_fill(m, 0.0)
    delta = (do * o).sum(-1, keepdim=True)
    ds = p * (torch.matmul(do, v.transpose(-1, -2)) - delta) * scale
    return {"dq": torch.matmul(ds, k), "A_dq": torch.matmul(ds.abs(), k.abs())}


@functools.lru_cache(maxsize=None)
def case(shape):
    """Inputs (bf16, CPU), the fp64 reference with its lse (fp32) and O (bf16)
    for the backward, E and the bounds.  Computed once per shape and shared;
    callers must not modify it."""
    b, h, sq, skv, d, causal = shape
    g = torch.Generator().manual_seed(2000 + sq * 7 + skv * 3 + d + int(causal))
    q = torch.randn((b, h, sq, d), generator=g).to(BF16)
    k = torch.randn((b, h, skv, d), generator=g).to(BF16)
    v = torch.randn((b, h, skv, d), generator=g).to(BF16)
    do = torch.randn((b, h, sq, d), generator=g).to(BF16)
    scale = 1.0 / math.sqrt(d)
    qt = prescale(q, scale)
    r64 = fwd_formulas(qt.double(), k.double(), v.double(), causal)
    r32 = fwd_formulas(qt.float(), k.float(), v.float(), causal)
    lse, o = r64["lse"].float(), r64["o"].to(BF16)   # as the forward kernel stores them
    args = (qt, k, v, do, o)
    r64.update(dq_formulas(*[t.double() for t in args], lse, scale, causal))
    r32.update(dq_formulas(*[t.float() for t in args], lse, scale, causal))
    E = {n: float((r32[n].double() - r64[n]).abs().max()) for n in OUTPUTS}
    bound = {n: U * r64[n].abs() + U * r64["A_" + n] + 4 * E[n] for n in ("o", "dq")}
    bound["lse"] = 4 * E["lse"] + EPS * (1 + r64["lse"].abs())
    return {"q": q, "k": k, "v": v, "do": do, "o": o, "lse": lse, "scale": scale,
            "causal": causal, "r64": r64, "r32": r32, "E": E, "bound": bound}


def worst(c, name, out):
    """largest err/bound of `out` against the case's reference"""
    err = (out.detach().double().cpu() - c["r64"][name]).abs()
    ratio = err / c["bound"][name]
    return float(ratio.nan_to_num(nan=float("inf")).max())


# the mistakes test_fa_fwd_dq_cpu.py plants in the emulation
MISTAKES = ("b_halves_swapped", "chunks_swapped", "stale_buffer", "last_tile_dropped",
            "causal_end_early")


def tile_starts(shape, q0, mistake=None):
    """kv0 of the tiles the block of q rows q0.. walks"""
    b, h, sq, skv, d, causal = shape
    kv_end = min(skv, q0 + QB) if causal else skv
    if mistake == "causal_end_early" and causal:
        kv_end -= KB
    starts = list(range(0, kv_end, KB))
    if mistake == "last_tile_dropped" and starts:
        starts.pop()
    return starts


def can_act(shape, mistake):
    b, h, sq, skv, d, causal = shape
    if mistake == "causal_end_early":
        return causal
    if mistake == "stale_buffer":     # some q block with at least two kv tiles
        return any(len(tile_starts(shape, q0)) >= 2 for q0 in range(0, sq, QB))
    return True


def _b_operand(t, mistake):
    """the [64][D] tile as the transposed reads deliver it to the second product"""
    if mistake == "b_halves_swapped":     # rows 8g+4..7 before 8g+0..3
        return t[..., torch.arange(KB) ^ 4, :]
    if mistake == "chunks_swapped":       # 16-byte chunks of a 32-byte pair, rows with (row>>2)&1
        sw = t[..., torch.arange(t.shape[-1]) ^ 8]
        odd = ((torch.arange(KB) >> 2) & 1).bool()[:, None]
        return torch.where(odd, sw, t)
    return t


def _kv_tile(t, kv0):
    """64 rows from kv0, zero-filled past the end (the guarded tail tile)"""
    out = torch.zeros(t.shape[:2] + (KB, t.shape[3]), dtype=t.dtype)
    n = max(0, min(KB, t.shape[2] - kv0))
    out[:, :, :n] = t[:, :, kv0:kv0 + n]
    return out


def emulate(shape, mistake=None):
    """fp32 torch emulation of the two kernels: 128-row q blocks, 64-row kv
    tiles up to the causal end, online softmax with the threshold-8 deferred
    maximum, P and dS rounded to bf16 before the second product, fp32
    accumulation, bf16 O / dQ, fp32 lse.  dQ takes the case's lse and O.
    `mistake` plants one of MISTAKES; returns ({o, lse, dq}, applied) with
    applied = the mistake changed which data some product saw."""
    assert mistake is None or mistake in MISTAKES
    c = case(shape)
    b, h, sq, skv, d, causal = shape
    scale = c["scale"]
    qt = prescale(c["q"], scale).float()
    k, v, do, o_in = (c[n].float() for n in ("k", "v", "do", "o"))
    lse_in = c["lse"]
    delta = (do * o_in).sum(-1)
    o = torch.zeros((b, h, sq, d))
    lse = torch.zeros((b, h, sq))
    dq = torch.zeros((b, h, sq, d))
    applied = mistake in ("b_halves_swapped", "chunks_swapped", "last_tile_dropped") or \
        (mistake == "causal_end_early" and causal)
    kv_off = torch.arange(KB)
    for q0 in range(0, sq, QB):
        n = min(QB, sq - q0)
        rows = q0 + torch.arange(n)
        qb, dob = qt[:, :, q0:q0 + n], do[:, :, q0:q0 + n]
        lse_b, dl_b = lse_in[:, :, q0:q0 + n], delta[:, :, q0:q0 + n]
        m_run = torch.full((b, h, n), float("-inf"))
        l_run = torch.zeros((b, h, n))
        oacc = torch.zeros((b, h, n, d))
        dacc = torch.zeros((b, h, n, d))
        starts = tile_starts(shape, q0, mistake)
        for i, kv0 in enumerate(starts):
            kt, vt = _kv_tile(k, kv0), _kv_tile(v, kv0)
            kb_, vb_ = kt, vt
            if mistake == "stale_buffer" and i >= 1:
                kb_, vb_ = _kv_tile(k, starts[i - 1]), _kv_tile(v, starts[i - 1])
                applied = True
            kv_abs = kv0 + kv_off
            dead = (kv_abs >= skv)[None, :].expand(n, KB).clone()
            if causal:
                dead |= kv_abs[None, :] > rows[:, None]
            st = torch.matmul(qb, kt.transpose(-1, -2))            # [n, 64]
            # forward: online softmax, deferred maximum
            s = st.masked_fill(dead, float("-inf"))
            mx = s.amax(-1)
            first = torch.isinf(m_run)
            grow = (mx > m_run + THR) | first
            m_new = torch.where(grow, torch.maximum(m_run, mx), m_run)
            corr = torch.where(first, torch.zeros_like(m_run), torch.exp(m_run - m_new))
            l_run = l_run * corr
            oacc = oacc * corr[..., None]
            m_run = m_new
            p = torch.where(torch.isinf(s), torch.zeros_like(s), torch.exp(s - m_run[..., None]))
            l_run = l_run + p.sum(-1)
            oacc = oacc + torch.matmul(p.to(BF16).float(), _b_operand(vb_, mistake))
            # dQ
            pb = torch.exp(st - lse_b[..., None]).masked_fill(dead, 0.0)
            dp = torch.matmul(dob, vt.transpose(-1, -2))
            ds = pb * (dp - dl_b[..., None]) * scale
            dacc = dacc + torch.matmul(ds.to(BF16).float(), _b_operand(kb_, mistake))
        inv_l = torch.where(l_run > 0, 1.0 / l_run, torch.zeros_like(l_run))
        o[:, :, q0:q0 + n] = oacc * inv_l[..., None]
        lse[:, :, q0:q0 + n] = torch.where(l_run > 0, m_run + torch.log(l_run),
                                           torch.full_like(l_run, float("-inf")))
        dq[:, :, q0:q0 + n] = dacc
    return {"o": o.to(BF16), "lse": lse, "dq": dq.to(BF16)}, applied
