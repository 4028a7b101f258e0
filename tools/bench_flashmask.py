"""FlashMask against what a user writes without it (docs/KERNELS.md, "FlashMask").

Per mask and sequence length, forward and forward+backward of
  flashmask : flashmask_attention(startend_row_indices)
  additive  : flash_attention(attn_mask = the same mask as bf16 [B, 1, S, S]),
              mask construction excluded -- the bar to beat
  causal    : plain causal flash_attention, informational: the work FlashMask
              cannot skip is this scaled by the live-tile fraction printed
in two alternating rounds; the rule: flashmask's mean below additive's minimum
in both rounds is a win.  Also flashmask_prep's time and the peak-memory
difference.  One JSON line per (mask, S).  Needs the GPU.

    python tools/bench_flashmask.py --s 8192 32768
"""
import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from paddle_amd import _ext  # noqa: E402
from paddle_amd.ops import functional as hot  # noqa: E402


def masks(s, dev):
    j = torch.arange(s, dtype=torch.int32, device=dev)
    start = j // 2048 * 2048
    return {"causal_docs2048": ((start + 2048)[None, None, :, None], True),
            "causal_window4096": ((j + 4096)[None, None, :, None], True),
            "bidir_docs2048": (torch.stack([start + 2048, start], -1)[None, None], False)}


def live_fraction(idx, s, causal):
    """live 128 x 64 tiles of the forward walk over those of the causal / full problem"""
    lo0, hi0, lo1, hi1 = (t[0, 0].view(-1, 64) for t in hot._flashmask_ranges(idx, s, causal))
    q0 = torch.arange(0, s, 128, device=idx.device)[:, None]
    dead = ((q0 >= lo0.amax(1)) & (q0 + 128 <= hi0.amin(1))) | \
           ((q0 >= lo1.amax(1)) & (q0 + 128 <= hi1.amin(1)))
    inside = (torch.arange(0, s, 64, device=idx.device)[None, :] < q0 + 128) if causal \
        else torch.ones_like(dead)
    return float((inside & ~dead).sum()) / float(inside.sum())


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return {"mean_ms": sum(times) / len(times), "min_ms": min(times), "max_ms": max(times)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--b", type=int, default=4)
    ap.add_argument("--h", type=int, default=32)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--s", type=int, nargs="+", default=[8192, 32768])
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    C = _ext.get_ext(required=True)
    dev = "cuda:0"
    for s in a.s:
        q, k, v = (torch.randn(a.b, s, a.h, a.d, device=dev, dtype=torch.bfloat16,
                               requires_grad=True) for _ in range(3))
        do = torch.randn_like(q)
        for name, (idx, causal) in masks(s, dev).items():
            idx = idx.expand(a.b, -1, -1, -1).contiguous()
            add = torch.zeros(a.b, 1, s, s, device=dev, dtype=torch.bfloat16).masked_fill(
                hot._flashmask_dense(idx, s, causal), float("-inf"))
            calls = {
                "flashmask": lambda: hot.flashmask_attention(q, k, v, idx, causal=causal),
                "additive": lambda: hot.flash_attention(q, k, v, causal=causal, attn_mask=add)[0],
                "causal": lambda: hot.flash_attention(q, k, v, causal=True)[0]}
            res = {"mask": name, "b": a.b, "h": a.h, "s": s, "d": a.d,
                   "live_fraction": live_fraction(idx, s, causal),
                   "prep": timed(lambda: C.flashmask_prep(idx, s, causal), a.iters),
                   "additive_mask_bytes": add.numel() * 2, "rounds": []}
            for _ in range(2):
                r = {}
                for n, f in calls.items():
                    with torch.no_grad():
                        r[n + "_fwd"] = timed(f, a.iters)
                    r[n + "_fwd_bwd"] = timed(lambda: f().backward(do), a.iters)
                res["rounds"].append(r)
            res["win_fwd_bwd"] = all(r["flashmask_fwd_bwd"]["mean_ms"] < r["additive_fwd_bwd"]["min_ms"]
                                     for r in res["rounds"])
            for n, f in calls.items():
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                f().backward(do)
                res[n + "_peak_extra_bytes"] = torch.cuda.max_memory_allocated() - base
            print(json.dumps(res), flush=True)
            del add


if __name__ == "__main__":
    main()
