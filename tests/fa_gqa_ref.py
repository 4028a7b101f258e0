"""Shared by test_fa_gqa_cpu.py and test_fa_gqa_gpu.py: inputs, the fp64
reference of the GQA flash-attention backward, its bounds, and a torch
emulation of the design of the GQA dK/dV kernels (csrc/kernels/fa_bwd.hip,
the GQA = true instantiations).  Everything here runs on the CPU.

GQA: q / dO / O have H heads, K / V have HKV; q head h reads K/V head
h // rep, rep = H // HKV.  Reference, from the bf16 inputs (upcast, so what
the kernels read), with the per-head formulas of fa_dkv_ref.py on k[h // rep]:
    dV[hk] = sum over the group of P_h^T dO_h      dK[hk] = sum of dS_h^T Q_h
Bound (docs/KERNELS.md, "kernel contract and tolerances"; no new constant):
    |out - ref| <= 2^-7*|ref| + 2^-7*sum_g A_g + 4*E
    A_g: the A term of fa_dkv_ref.py for head g of the group (one bf16 ulp on
        every P / dS element), E = max |group-summed formulas in fp32 torch -
        the same in fp64| on the same inputs
dQ is per q head: the formulas and the bound of fa_fwd_dq_ref.py on K / V
repeated per head (Q pre-scaled and rounded to bf16, as the dQ kernel does).

The emulation follows the design: a block owns a 128-row kv block of one kv
head and G consecutive q heads; it streams the 64-row q tiles q_start..Sq of
head h0, then of h0 + 1, ... through two buffers whose parity runs across
head boundaries; P and dS are rounded to bf16 before the second product; the
accumulators are fp32 over the whole stream.  G == rep rounds them to bf16;
G < rep keeps fp32 partials, which are summed in the order of the q heads and
rounded once.
"""
import functools
import math

import torch

from fa_dkv_ref import formulas
from fa_fwd_dq_ref import dq_formulas, prescale

BF16 = torch.bfloat16
U = 2.0 ** -7
QB, KVB = 64, 128   # q tile rows, kv rows per block: the kernel's tiling

# (B, H, HKV, Sq, Skv, D, causal): the smallest shapes at which the GQA tile
# stream takes another path
SHAPES = [
    (1, 2, 1, 40, 40, 128, True),     # guarded tile only; head boundary right after the prologue
    (1, 4, 2, 64, 64, 128, True),     # one tile per head: every tile is a head boundary; two kv heads
    (1, 4, 1, 192, 192, 128, True),   # odd tile count: parity differs at each boundary; 2nd kv block has its own q_start
    (2, 6, 2, 200, 200, 128, True),   # rep 3, batch, DMA tiles then a tail, partial kv block
    (2, 6, 2, 200, 200, 128, False),
    (1, 8, 1, 320, 136, 128, False),  # rep 8, Sq != Skv
    (1, 4, 2, 192, 192, 64, True),    # D = 64
    (1, 4, 2, 200, 264, 64, False),
]


def shape_id(s):
    return "b%d_h%d_hkv%d_sq%d_skv%d_d%d_%s" % (s[0], s[1], s[2], s[3], s[4], s[5],
                                                 "causal" if s[6] else "full")


def divisors(rep):
    return [g for g in range(1, rep + 1) if rep % g == 0]


def _mask(sq, skv, causal):
    if not causal:
        return None
    return torch.arange(skv)[None, :] > torch.arange(sq)[:, None]   # True = masked out


def _group_sum(t, hkv):
    b, h, skv, d = t.shape
    return t.view(b, hkv, h // hkv, skv, d).sum(2)


def gqa_formulas(q, k, v, do, o, lse, scale, causal):
    """group-summed dV, dK and A terms in the dtype of the inputs"""
    hkv, rep = k.shape[1], q.shape[1] // k.shape[1]
    ke, ve = k.repeat_interleave(rep, dim=1), v.repeat_interleave(rep, dim=1)
    r = formulas(q, ke, ve, do, o, lse, scale, causal)
    return {n: _group_sum(t, hkv) for n, t in r.items()}


@functools.lru_cache(maxsize=None)
def case(shape):
    """Inputs (bf16 / fp32 lse, CPU), fp64 references, E and the bounds.
    Computed once per shape and shared; callers must not modify it."""
    b, h, hkv, sq, skv, d, causal = shape
    rep = h // hkv
    g = torch.Generator().manual_seed(3000 + h * 11 + hkv * 5 + sq * 7 + skv * 3 + d + int(causal))
    q = torch.randn((b, h, sq, d), generator=g).to(BF16)
    k = torch.randn((b, hkv, skv, d), generator=g).to(BF16)
    v = torch.randn((b, hkv, skv, d), generator=g).to(BF16)
    do = torch.randn((b, h, sq, d), generator=g).to(BF16)
    scale = 1.0 / math.sqrt(d)
    # forward in fp64: lse to fp32, O to bf16, as the forward kernel stores them
    ke, ve = k.repeat_interleave(rep, dim=1), v.repeat_interleave(rep, dim=1)
    s = torch.matmul(q.double(), ke.double().transpose(-1, -2)) * scale
    m = _mask(sq, skv, causal)
    if m is not None:
        s = s.masked_fill(m, float("-inf"))
    lse = torch.logsumexp(s, -1).float()
    o = torch.matmul(torch.softmax(s, -1), ve.double()).to(BF16)
    args = (q, k, v, do, o)
    r64 = gqa_formulas(*[t.double() for t in args], lse, scale, causal)
    r32 = gqa_formulas(*[t.float() for t in args], lse, scale, causal)
    # dQ: the dQ kernel's own rounding of Q
    qt = prescale(q, scale)
    dargs = (qt, ke, ve, do, o)
    r64.update(dq_formulas(*[t.double() for t in dargs], lse, scale, causal))
    r32.update(dq_formulas(*[t.float() for t in dargs], lse, scale, causal))
    names = ("dv", "dk", "dq")
    E = {n: float((r32[n].double() - r64[n]).abs().max()) for n in names}
    bound = {n: U * r64[n].abs() + U * r64["A_" + n] + 4 * E[n] for n in names}
    return {"q": q, "k": k, "v": v, "do": do, "o": o, "lse": lse, "scale": scale,
            "causal": causal, "r64": r64, "r32": r32, "E": E, "bound": bound}


def worst(c, name, out):
    """largest err/bound of `out` against the case's reference"""
    err = (out.detach().double().cpu() - c["r64"][name]).abs()
    ratio = err / c["bound"][name]
    return float(ratio.nan_to_num(nan=float("inf")).max())


def worst_pair(c, name, x, y):
    """largest |x - y| / bound: two results that both meet the bound differ
    by at most twice it"""
    err = (x.detach().double().cpu() - y.detach().double().cpu()).abs()
    return float((err / c["bound"][name]).nan_to_num(nan=float("inf")).max())


# the mistakes test_fa_gqa_cpu.py plants in the emulation
MISTAKES = ("head_map_mod", "last_head_dropped", "stats_not_advanced", "stale_buffer",
            "q0_not_wrapped", "last_partial_dropped")


def can_act(shape, G, mistake):
    b, h, hkv, sq, skv, d, causal = shape
    rep = h // hkv
    if mistake == "head_map_mod":           # h % hkv == h // rep for every h when hkv == 1
        return hkv > 1
    if mistake == "last_partial_dropped":   # no partials without a reduce
        return G < rep
    return G > 1                            # the others need a head boundary in a block


def emulate(shape, G, mistake=None):
    """fp32 torch emulation of the GQA dK/dV design with G q heads per block.
    `mistake` plants one of MISTAKES:
      head_map_mod          q head h paired with kv head h % hkv, not h // rep
      last_head_dropped     the stream ends one head early
      stats_not_advanced    lse / delta of every head read at the first head's base
      stale_buffer          the first tile of head g+1 reads the buffer the
                            stream's previous tile left (not restaged)
      q0_not_wrapped        q0 keeps running past Sq at a head boundary, so the
                            predicates see the tiles of later heads out of range
      last_partial_dropped  the reduce sums one partial too few
    Returns (dv, dk, applied)."""
    assert mistake is None or mistake in MISTAKES
    c = case(shape)
    b, h, hkv, sq, skv, d, causal = shape
    rep = h // hkv
    assert rep % G == 0
    q, k, v, do, o = (c[n].float() for n in ("q", "k", "v", "do", "o"))
    lse, scale = c["lse"], c["scale"]
    delta = (do * o).sum(-1)
    parts = rep // G
    pdv = torch.zeros((b, hkv, parts, skv, d))
    pdk = torch.zeros((b, hkv, parts, skv, d))
    applied = False

    def tile(t, q0):
        out = torch.zeros((b, QB) + t.shape[2:], dtype=t.dtype)
        n = max(0, min(QB, sq - q0))
        out[:, :n] = t[:, q0:q0 + n]
        return out

    for hk in range(hkv):
        if mistake == "head_map_mod":
            group = [x for x in range(h) if x % hkv == hk]
            applied = applied or group != list(range(hk * rep, hk * rep + rep))
        else:
            group = list(range(hk * rep, hk * rep + rep))
        for part in range(parts):
            heads = group[part * G:(part + 1) * G]
            if mistake == "last_head_dropped" and len(heads) > 1:
                heads = heads[:-1]
                applied = True
            for kv0 in range(0, skv, KVB):
                nkv = min(KVB, skv - kv0)
                kb, vb = k[:, hk, kv0:kv0 + nkv], v[:, hk, kv0:kv0 + nkv]
                q_start = (kv0 // QB) * QB if causal else 0
                starts = list(range(q_start, sq, QB))
                stream = [(hd, q0) for hd in heads for q0 in starts]
                dv_acc = torch.zeros((b, nkv, d))
                dk_acc = torch.zeros((b, nkv, d))
                bufs = [None, None]          # the two {Q, dO} buffers
                q_run = q_start              # q0 as a loop that never wraps sees it
                for t, (hd, q0) in enumerate(stream):
                    first_of_head = q0 == starts[0] and hd != heads[0]
                    if mistake == "stale_buffer" and first_of_head:
                        bufs[t & 1] = bufs[(t - 1) & 1]   # what the previous tile left
                        applied = True
                    else:
                        bufs[t & 1] = (tile(q[:, hd], q0), tile(do[:, hd], q0))
                    qt, dot = bufs[t & 1]
                    q_pred = q0              # the tile's own q0, for the predicates
                    if mistake == "q0_not_wrapped" and hd != heads[0]:
                        q_pred = q_run
                        applied = True
                    q_run += QB
                    hs = hd
                    if mistake == "stats_not_advanced" and hd != heads[0]:
                        hs = heads[0]
                        applied = True
                    rows = q_pred + torch.arange(QB)
                    lse_t = tile(lse[:, hs, :, None], q0)[..., 0]
                    lse_t[:, (q0 + torch.arange(QB)) >= sq] = float("inf")
                    dl_t = tile(delta[:, hs, :, None], q0)[..., 0]
                    st = torch.matmul(kb, qt.transpose(-1, -2))            # [b, nkv, 64]
                    p = torch.exp(st * scale - lse_t[:, None, :])
                    kv_abs = kv0 + torch.arange(nkv)
                    dead = (rows >= sq)[None, :].expand(nkv, QB).clone()
                    if causal:
                        dead |= kv_abs[:, None] > rows[None, :]
                    p = p.masked_fill(dead, 0.0)
                    dv_acc += torch.matmul(p.to(BF16).float(), dot)
                    dp = torch.matmul(vb, dot.transpose(-1, -2))
                    ds = p * (dp - dl_t[:, None, :]) * scale
                    dk_acc += torch.matmul(ds.to(BF16).float(), qt)
                pdv[:, hk, part, kv0:kv0 + nkv] = dv_acc
                pdk[:, hk, part, kv0:kv0 + nkv] = dk_acc

    def reduce(pt):
        if parts == 1:
            return pt[:, :, 0].to(BF16)
        n = parts
        if mistake == "last_partial_dropped":
            n -= 1
        acc = pt[:, :, 0].clone()
        for p_ in range(1, n):               # fixed order: the order of the q heads
            acc += pt[:, :, p_]
        return acc.to(BF16)

    if mistake == "last_partial_dropped" and parts > 1:
        applied = True
    return reduce(pdv), reduce(pdk), applied
