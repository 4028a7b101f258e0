#!/usr/bin/env python3
"""Flash-attention bit-parity fingerprint.

Prints a SHA-256 of each of o, lse, dq, dk, dv for a fixed list of
flash_attn_fwd / flash_attn_bwd / varlen calls on inputs generated on the CPU
from fixed seeds.  Run it in two builds (separate processes) and diff the
output: a change that only moves code must leave every line identical.
"""
import hashlib
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import paddle_amd  # noqa: F401,E402
from paddle_amd import _ext  # noqa: E402

DEV = "cuda:0"
P, SEED, OFFSET = 0.3, 4321, 77
LENS = [1, 37, 128, 130]


def randn(seed, *shape):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(torch.bfloat16).to(DEV)


def sha(t):
    t = t.detach().contiguous().cpu()
    return hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()


def report(name, tensors):
    torch.cuda.synchronize()
    for n, t in zip(("o", "lse", "dq", "dk", "dv"), tensors):
        print(f"{name:34s} {n:3s} {sha(t)}")


def dense(C, name, b, h, sq, skv, d, causal, mask=False, p=0.0, packed=False):
    scale = 1.0 / math.sqrt(d)
    if packed:   # the model's [B, S, 3, H, D] layout, gradients written in place
        qkv = randn(1, b, sq, 3, h, d)
        q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
        do = randn(2, b, sq, h, d).permute(0, 2, 1, 3)
        o = torch.empty(b, sq, h, d, dtype=torch.bfloat16, device=DEV).permute(0, 2, 1, 3)
        dqkv = torch.zeros_like(qkv)
        dq, dk, dv = (dqkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    else:
        q, do = randn(1, b, h, sq, d), randn(2, b, h, sq, d)
        k, v = randn(3, b, h, skv, d), randn(4, b, h, skv, d)
        o = dq = dk = dv = None
    m = None
    if mask:
        m = torch.zeros(b, 1, sq, skv + 8, dtype=torch.bfloat16, device=DEV)[..., :skv]
        m.copy_(randn(5, b, 1, sq, skv).float() * 0.5)
        m[..., ::7] = -10000.0
    o, lse = C.flash_attn_fwd(q, k, v, o, scale, causal, m, p, SEED, OFFSET)
    dq, dk, dv = C.flash_attn_bwd(do, q, k, v, o, lse, dq, dk, dv, scale, causal, m,
                                  p, SEED, OFFSET)
    report(name, (o, lse, dq, dk, dv))


def varlen(C, name, h, d, causal, p):
    scale = 1.0 / math.sqrt(d)
    total = sum(LENS)
    cu = torch.tensor([0] + list(torch.cumsum(torch.tensor(LENS), 0)),
                      dtype=torch.int32, device=DEV)
    q, k, v, g = (randn(10 + i, total, h, d) for i in range(4))
    o, lse = C.flash_attn_varlen_fwd(q, k, v, cu, cu, scale, causal, p, SEED, OFFSET)
    dq, dk, dv = C.flash_attn_varlen_bwd(g, q, k, v, o, lse, cu, cu, scale, causal,
                                         p, SEED, OFFSET)
    report(name, (o, lse, dq, dk, dv))


def main():
    C = _ext.get_ext(required=True)
    for d in (64, 128):
        for causal in (False, True):
            c = "causal" if causal else "full"
            dense(C, f"dense_d{d}_{c}", 2, 2, 160, 160, d, causal)
            dense(C, f"packed_d{d}_{c}", 2, 2, 160, 160, d, causal, packed=True)
            dense(C, f"mask_d{d}_{c}", 2, 2, 160, 160, d, causal, mask=True)
            dense(C, f"drop_d{d}_{c}", 2, 2, 160, 160, d, causal, p=P)
            dense(C, f"mask_drop_d{d}_{c}", 2, 2, 160, 160, d, causal, mask=True, p=P)
            varlen(C, f"varlen_d{d}_{c}", 4, d, causal, 0.0)
            varlen(C, f"varlen_drop_d{d}_{c}", 4, d, causal, P)
        dense(C, f"cross_mask_drop_d{d}", 2, 2, 96, 160, d, False, mask=True, p=P)
    dense(C, "dense_b4h32s2048d128_causal", 4, 32, 2048, 2048, 128, True)
    dense(C, "packed_b4h32s2048d128_causal", 4, 32, 2048, 2048, 128, True, packed=True)
    dense(C, "dense_b4h32s2048d128_full", 4, 32, 2048, 2048, 128, False)


if __name__ == "__main__":
    main()
