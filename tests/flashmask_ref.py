"""Shared by test_flashmask_cpu.py and test_flashmask_gpu.py: the FlashMask
cases, the fp64 reference of O, LSE, dQ, dK, dV under a boolean mask, their
bounds, and a torch emulation of the tile walk of csrc/kernels/flashmask.hip.
Everything here runs on the CPU.

Reference: the formulas in the header of fa_fwd_dq_ref.py with the mask
applied (q~ = bf16(q * scale); a removed score is -inf in S and 0 in P); dV =
P^T dO, dK = dS^T Q.  The backward gets the reference's own bf16 O and fp32
LSE.  Bounds, unchanged from fa_fwd_dq_ref.py / fa_dkv_ref.py:
    |out - ref| <= 2^-7*|ref| + 2^-7*A + 4*E            (O, dQ, dK, dV)
    |lse - ref| <= 4*E + 2^-22*(1 + |ref|)              (finite entries)
A row with no visible column is compared exactly: O = dQ = 0, LSE = -inf.
"""
import functools
import math

import torch

BF16 = torch.bfloat16
U = 2.0 ** -7
EPS = 2.0 ** -22
S = 328
OUTPUTS = ("o", "lse", "dq", "dk", "dv")
DOCS = (0, 70, 200)       # document starts at S = 328


def _doc_bounds(n, starts, limit):
    """per position its document's (start, end), ends clamped to `limit`"""
    j = torch.arange(n)
    st = torch.tensor(starts)
    which = (j[:, None] >= st[None, :]).sum(-1) - 1
    ends = torch.tensor(list(starts[1:]) + [max(n, limit)])
    return st[which], ends[which].clamp(max=limit)


def indices(name, sq=S, skv=S, hm=1, docs=DOCS):
    """(startend_row_indices int32 [1, hm, skv, C], causal) of a case; head i
    of hm > 1 has its bounds shifted by 32 * i rows"""
    j = torch.arange(skv)
    start, end = _doc_bounds(skv, docs, sq)
    if name == "docs":
        cols, causal = [end], True
    elif name == "prefix_window":
        cols, causal = [torch.where(j < 64, sq, (j + 64).clamp(max=sq))], True
    elif name == "window":                   # what window_size = (63, 0) lowers to
        cols, causal = [j + 64], True
    elif name == "hole":
        cols = [torch.where(j < 128, 128, sq), torch.where(j < 128, 224, sq)]
        causal = True
    elif name == "bidir_docs":
        cols, causal = [end, start], False
    elif name == "dead":
        cols = [torch.full_like(j, 250), torch.full_like(j, sq), torch.zeros_like(j),
                (j - 96).clamp(min=0)]
        causal = False
    else:
        raise KeyError(name)
    one = torch.stack(cols, -1)
    idx = torch.stack([torch.where(one < sq, one + 32 * i, one) if name == "hole" else one
                       for i in range(hm)])
    return idx[None].to(torch.int32), causal


def dense_mask(idx, sq, causal):
    """bool [B, Hm, sq, skv], True = removed: the ranges by two arange
    comparisons each, plus the causal mask"""
    c = idx.shape[-1]
    col = [idx[..., i].long()[:, :, None, :] for i in range(c)]
    row = torch.arange(sq)[:, None]
    if causal:
        gone = (row >= col[0]) & ((row < col[1]) if c == 2 else True)
        gone = gone | (torch.arange(idx.shape[2])[None, :] > row)
    elif c == 2:
        gone = (row >= col[0]) | (row < col[1])
    else:
        gone = ((row >= col[0]) & (row < col[1])) | ((row >= col[2]) & (row < col[3]))
    return gone


def formulas(qt, q, k, v, do, gone, scale, o=None, lse=None):
    """forward (o / lse None) or backward formulas in the dtype of the inputs;
    k, v already expanded to q's heads"""
    s = torch.matmul(qt, k.transpose(-1, -2)).masked_fill(gone, float("-inf"))
    if o is None:
        p = torch.softmax(s, -1).nan_to_num(0.0)
        return {"lse": torch.logsumexp(s, -1), "o": torch.matmul(p, v),
                "A_o": torch.matmul(p, v.abs())}
    lse = lse.to(s.dtype).masked_fill(torch.isinf(lse), 0.0)
    p = torch.exp(s - lse[..., None]).masked_fill(gone, 0.0)
    delta = (do * o).sum(-1, keepdim=True)
    ds = p * (torch.matmul(do, v.transpose(-1, -2)) - delta) * scale
    pt, dst = p.transpose(-1, -2), ds.transpose(-1, -2)
    return {"dq": torch.matmul(ds, k), "A_dq": torch.matmul(ds.abs(), k.abs()),
            "dk": torch.matmul(dst, q), "A_dk": torch.matmul(dst.abs(), q.abs()),
            "dv": torch.matmul(pt, do), "A_dv": torch.matmul(pt, do.abs())}


@functools.lru_cache(maxsize=None)
def case(name, d=128, h=2, hm=1, sq=S, skv=S, hkv=None, docs=DOCS):
    """Inputs (bf16, CPU), indices, the fp64 reference with its lse (fp32) and
    O (bf16), E and the bounds.  Computed once and shared; callers must not
    modify it."""
    hkv = hkv or h
    rep = h // hkv
    idx, causal = indices(name, sq, skv, hm, docs)
    g = torch.Generator().manual_seed(3000 + sq * 7 + skv * 3 + d + h + sum(map(ord, name)))
    q = torch.randn((1, h, sq, d), generator=g).to(BF16)
    k = torch.randn((1, hkv, skv, d), generator=g).to(BF16)
    v = torch.randn((1, hkv, skv, d), generator=g).to(BF16)
    do = torch.randn((1, h, sq, d), generator=g).to(BF16)
    scale = 1.0 / math.sqrt(d)
    qt = (q.float() * scale).to(BF16)
    gone = dense_mask(idx, sq, causal)
    if hm > 1:
        gone = gone.repeat_interleave(h // hm, dim=1)
    ke, ve = k.repeat_interleave(rep, dim=1), v.repeat_interleave(rep, dim=1)

    c = {"q": q, "k": k, "v": v, "do": do, "idx": idx, "causal": causal, "scale": scale,
         "gone": gone, "_in": (qt, q, ke, ve, do), "_gqa": (hkv, rep)}
    r64, r32 = _run(c, torch.float64), _run(c, torch.float32)
    c.update(lse=r64["lse"].float(), o=r64["o"].to(BF16), dead=torch.isinf(r64["lse"]),
             r64=r64, E={}, bound={})
    live = ~c["dead"]
    c["E"] = {n: float((r32[n].double() - r64[n]).abs().max()) for n in ("o",)}
    c["E"]["lse"] = float((r32["lse"].double() - r64["lse"])[live].abs().max())
    c["bound"]["o"] = U * r64["o"].abs() + U * r64["A_o"] + 4 * c["E"]["o"]
    c["bound"]["lse"] = 4 * c["E"]["lse"] + EPS * (1 + r64["lse"].abs())
    return with_forward(c, c["o"], c["lse"])


def _run(c, dt, o=None, lse=None):
    args = [t.to(dt) for t in c["_in"]]
    r = formulas(*args, c["gone"], c["scale"], None if o is None else o.to(dt), lse)
    if o is not None:                        # GQA: dK / dV summed per kv head
        hkv, rep = c["_gqa"]
        for n in ("dk", "dv", "A_dk", "A_dv"):
            r[n] = r[n].view(1, hkv, rep, *r[n].shape[2:]).sum(2)
    return r


def with_forward(c, o, lse):
    """the case with the reference, E and bounds of dQ, dK, dV for a backward
    that reads this O (bf16) and LSE (fp32); a new dict"""
    o, lse = o.detach().cpu(), lse.detach().cpu()
    r64, r32 = _run(c, torch.float64, o, lse), _run(c, torch.float32, o, lse)
    c = dict(c, r64=dict(c["r64"], **r64), E=dict(c["E"]), bound=dict(c["bound"]))
    for n in ("dq", "dk", "dv"):
        c["E"][n] = float((r32[n].double() - r64[n]).abs().max())
        c["bound"][n] = U * r64[n].abs() + U * r64["A_" + n] + 4 * c["E"][n]
    return c


def worst(c, name, out):
    """largest err / bound of `out` against the case's reference; inf if a row
    with no visible column is not exactly O = dQ = 0, LSE = -inf"""
    out = out.detach().double().cpu()
    dead = c["dead"]
    if name in ("o", "dq") and bool((out[dead] != 0).any()):
        return float("inf")
    if name == "lse":
        if not bool((out[dead] == float("-inf")).all()):
            return float("inf")
        out, ref, bound = out[~dead], c["r64"]["lse"][~dead], c["bound"]["lse"][~dead]
    else:
        ref, bound = c["r64"][name], c["bound"][name]
    ratio = (out - ref).abs() / bound
    return float(ratio.nan_to_num(nan=float("inf")).max()) if ratio.numel() else 0.0


# ---------------------------------------------------------------------------
# emulation of the walk: prep summary, skip rule, parity by live tile,
# predicate mask, dK/dV by predicate
# ---------------------------------------------------------------------------
MISTAKES = ("stale_buffer", "skip_min_lo", "hi_inclusive", "second_range_ignored",
            "dead_row_p")
QB, KB = 128, 64


def canonical(idx, sq, causal):
    """(lo0, hi0, lo1, hi1) int64 [skv] of head 0, as flashmask_prep writes them"""
    from paddle_amd.ops.functional import _flashmask_ranges
    return [t[0, 0] for t in _flashmask_ranges(idx, sq, causal)]


def emulate(c, mistake=None):
    """fp32 torch emulation (mask head 0 for every head; P and dS rounded to
    bf16 before the second product) -> ({o, lse, dq, dk, dv}, applied)"""
    assert mistake is None or mistake in MISTAKES
    q, k, v, do, o_in = (c[n].float() for n in ("q", "k", "v", "do", "o"))
    scale, causal = c["scale"], c["causal"]
    sq, skv, d = q.shape[2], k.shape[2], q.shape[3]
    qt = (c["q"].float() * scale).to(BF16).float()
    lo0, hi0, lo1, hi1 = canonical(c["idx"], sq, causal)
    if mistake == "second_range_ignored":
        lo1, hi1 = torch.full_like(lo1, sq), torch.full_like(hi1, sq)
    applied = mistake == "second_range_ignored"
    row_all = torch.arange(sq)

    def removed(rows, cols):                 # [len(rows), len(cols)]
        r = rows[:, None]
        inc = 1 if mistake == "hi_inclusive" else 0
        g = ((r >= lo0[cols]) & (r < hi0[cols] + inc)) | ((r >= lo1[cols]) & (r < hi1[cols] + inc))
        if causal:
            g = g | (cols[None, :] > r)
        return g

    lse_in = c["lse"]
    delta = (do * o_in).sum(-1)
    o, lse, dq = torch.zeros_like(q), torch.zeros(q.shape[:3]), torch.zeros_like(q)
    for q0 in range(0, sq, QB):
        qe = min(q0 + QB, sq)
        rows = torch.arange(q0, qe)
        kv_end = min(skv, q0 + QB) if causal else skv
        live = []
        for kv0 in range(0, kv_end, KB):
            cols = torch.arange(kv0, min(kv0 + KB, skv))
            dead_tile = False
            for lo, hi in ((lo0, hi0), (lo1, hi1)):
                edge = lo[cols].min() if mistake == "skip_min_lo" else lo[cols].max()
                dead_tile |= bool(q0 >= edge and qe <= hi[cols].min())
            if not dead_tile:
                live.append(kv0)
        cols, src = [], []                   # columns walked, columns read
        for i, kv0 in enumerate(live):
            n = min(kv0 + KB, skv) - kv0
            prev = live[i - 1] if i else -KB
            stale = mistake == "stale_buffer" and kv0 - prev > KB
            # stale: the read pointer moves by live tiles, the staging by tile
            # index, so the first skipped tile is read as this one
            applied |= stale or mistake in ("hi_inclusive", "skip_min_lo")
            cols.append(torch.arange(kv0, kv0 + n))
            src.append(torch.arange(prev + KB, prev + KB + n) if stale else cols[-1])
        cols, src = torch.cat(cols or [row_all[:0]]), torch.cat(src or [row_all[:0]])
        gone = removed(rows, cols)
        qb, kr, vr = qt[:, :, q0:qe], k[:, :, src], v[:, :, src]
        s = torch.matmul(qb, kr.transpose(-1, -2)).masked_fill(gone, float("-inf"))
        p = torch.softmax(s, -1).nan_to_num(0.0)
        o[:, :, q0:qe] = torch.matmul(p.to(BF16).float(), vr)
        lse[:, :, q0:qe] = torch.logsumexp(s, -1)
        lse_b = lse_in[:, :, q0:qe].masked_fill(torch.isinf(lse_in[:, :, q0:qe]), 1e30)
        st = torch.matmul(qb, k[:, :, cols].transpose(-1, -2))
        pb = torch.exp(st - lse_b[..., None]).masked_fill(gone, 0.0)
        dp = torch.matmul(do[:, :, q0:qe], v[:, :, cols].transpose(-1, -2))
        ds = pb * (dp - delta[:, :, q0:qe, None]) * scale
        dq[:, :, q0:qe] = torch.matmul(ds.to(BF16).float(), kr)
    # dK / dV: P and dS zeroed by predicate, lse = -inf read as +1e30
    gone = removed(row_all, torch.arange(skv))
    lse_f = lse_in.masked_fill(torch.isinf(lse_in), 1e30)
    if mistake == "dead_row_p":              # lse = -inf taken as 0, no predicate on the row
        dead = torch.isinf(lse_in)
        lse_f = lse_in.masked_fill(dead, 0.0)
        gone = gone[None, None] & ~dead[..., None]
        applied = bool(dead.any())
    st = torch.matmul(q, k.transpose(-1, -2)) * scale
    p = torch.exp(st - lse_f[..., None]).masked_fill(gone, 0.0)
    ds = p * (torch.matmul(do, v.transpose(-1, -2)) - delta[..., None]) * scale
    dv = torch.matmul(p.to(BF16).float().transpose(-1, -2), do)
    dk = torch.matmul(ds.to(BF16).float().transpose(-1, -2), q)
    return {"o": o.to(BF16), "lse": lse, "dq": dq.to(BF16), "dk": dk.to(BF16),
            "dv": dv.to(BF16)}, applied
