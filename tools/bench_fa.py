#!/usr/bin/env python3
"""Flash-attention kernel microbenchmark on MI355X.

Reports achieved TFLOP/s for fwd and bwd at GPT-3-6.7B shapes.
attn FLOPs (causal): fwd = 2 * 2 * B*H*S^2*D * 0.5 ; bwd = 2.5x fwd.

--hkv N (N != --h) times grouped-query attention through _FlashAttn, forward
and backward, as a model runs it: whatever the backward does around its
kernels (a tree without the native GQA backward expands K/V and sums the
groups in torch) is inside the figure.  --gqa-heads G times the backward as
the direct flash_attn_bwd call with gqa_heads_per_block = G in place of
_fa_bwd_gqa_plan's choice (dense only; the varlen path is not timed here).
"""
import argparse
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import paddle_amd  # noqa: F401,E402  (patches + ext)
from paddle_amd import _ext
from paddle_amd.ops import functional as F


def bench(fn, iters=20, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--b", type=int, default=4)
    ap.add_argument("--h", type=int, default=32)
    ap.add_argument("--hkv", type=int, default=0, help="kv heads (0 = --h)")
    ap.add_argument("--gqa-heads", type=int, default=0,
                    help="q heads per dK/dV block of the GQA backward (0 = the plan's choice)")
    ap.add_argument("--s", type=int, default=2048)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--causal", type=int, default=1)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    C = _ext.get_ext()
    B, H, S, D = args.b, args.h, args.s, args.d
    HKV = args.hkv or H
    causal = bool(args.causal)
    scale = 1.0 / math.sqrt(D)
    fwd_flops = 4 * B * H * S * S * D * (0.5 if causal else 1.0)
    print(f"shape B{B} H{H} HKV{HKV} S{S} D{D} causal={causal}")

    if HKV == H:
        q = torch.randn(B, H, S, D, device="cuda", dtype=torch.bfloat16)
        k = torch.randn_like(q)
        v = torch.randn_like(q)
        o, lse = C.flash_attn_fwd(q, k, v, None, scale, causal)
        do = torch.randn_like(o)
        t_fwd = bench(lambda: C.flash_attn_fwd(q, k, v, None, scale, causal), args.iters)
        t_bwd = bench(lambda: C.flash_attn_bwd(do, q, k, v, o, lse, None, None, None,
                                               scale, causal), args.iters)
    else:
        q = torch.randn(B, H, S, D, device="cuda", dtype=torch.bfloat16)
        k = torch.randn(B, HKV, S, D, device="cuda", dtype=torch.bfloat16)
        v = torch.randn_like(k)
        do = torch.randn_like(q)
        qg, kg, vg = (t.requires_grad_(True) for t in (q, k, v))
        o, lse = F._FlashAttn.apply(qg, kg, vg, scale, causal)
        if args.gqa_heads:
            # the binding with G pinned: what _FlashAttn.backward launches, with
            # this G in place of _fa_bwd_gqa_plan's
            plan = "G=%d (pinned)" % args.gqa_heads
            od, qd, kd, vd = (t.detach() for t in (o, q, k, v))
            bwd = lambda: C.flash_attn_bwd(do, qd, kd, vd, od, lse, None, None, None, scale,
                                           causal, gqa_heads_per_block=args.gqa_heads)
        else:
            plan = ("G=%d" % F._fa_bwd_gqa_plan(B, H, HKV, -(-S // 128))
                    if hasattr(F, "_fa_bwd_gqa_plan") else "expand")
            bwd = lambda: torch.autograd.grad(o, (qg, kg, vg), do, retain_graph=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t_bwd = bench(bwd, args.iters)
        peak = torch.cuda.max_memory_allocated() - base
        with torch.no_grad():
            t_fwd = bench(lambda: F._FlashAttn.apply(q, k, v, scale, causal), args.iters)
        dq, dk, dv = bwd()
        torch.cuda.synchronize()
        print(f"gqa bwd: {plan}  peak extra memory {peak / 2**20:.1f} MiB  "
              f"|dk| {dk.float().abs().mean().item():.6f} |dv| {dv.float().abs().mean().item():.6f}")
    print(f"fwd: {t_fwd*1e3:8.3f} ms  {fwd_flops/t_fwd/1e12:7.1f} TF")
    print(f"bwd: {t_bwd*1e3:8.3f} ms  {2.5*fwd_flops/t_bwd/1e12:7.1f} TF")


if __name__ == "__main__":
    main()
