"""Paged decode attention timing: the bf16 cache kernel vs the int8 cache
kernel (decode_attn.hip) on the same shapes, and against both the split-KV
kernels (decode_attn_split.hip): the heuristic's choice ("auto") and a forced
sweep of num_splits.  "old" is num_splits=0, the one-block-per-q-head kernel:
the yardstick of every other variant of the same cache in the same process.

HBM-cold discipline (as bench_wonly.py): every variant cycles through
`layers` pools (one per model layer) whose bytes exceed --pool-gb, several
times the 256 MB L3, so no call finds its cache in a cache.  The pools are
sized from real block tables (randperm block order, ceil(S/bs) blocks per
sequence).  One pass over the layers is a hipGraph timed with device events;
all variants alternate in one process and the median of --repeats passes is
reported as us per call (with mean, min and max) and TB/s of cache bytes
read (K and V codes of the S valid positions, int8 scales included; q, the
table and the output are not counted).  A variant wins when its mean is
below the yardstick's minimum; it loses when its mean is above the
yardstick's mean plus the yardstick's spread (max - min).
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from paddle_amd.ops import functional as hot  # noqa: E402

SHAPES = [(32, 32, hkv, 128, s) for hkv in (32, 8)
          for s in (128, 512, 2048, 4096)] + \
    [(b, 32, hkv, 128, s) for b in (1, 4, 8) for hkv in (32, 8)
     for s in (2048, 4096, 16384)]
SWEEP = (1, 2, 4, 8, 16, 32)
BS = 16


def variants(s):
    """(name, num_splits): the yardstick, the heuristic, the forced sweep
    (a forced count is kept while each split holds >= 128 positions)."""
    return [("old", 0), ("auto", None)] + [
        (f"n{n}", n) for n in SWEEP if n == 1 or s // n >= 128]


def capture_pass(calls):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for c in calls[:2]:                  # code objects, allocator
            c()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for c in calls:
            c()
    return g, len(calls)


def time_pass(captured):
    g, ncalls = captured
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    g.replay()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e-3 / ncalls


def bench_shape(b, h, hkv, d, s, pool_bytes, repeats):
    dev = "cuda"
    nb = -(-s // BS)
    nblocks = b * nb
    table = torch.randperm(nblocks, device=dev).int().reshape(b, nb)
    lens = torch.full((b,), s, dtype=torch.int32, device=dev)
    q = torch.randn(b, h, d, device=dev, dtype=torch.bfloat16)
    bytes_bf16 = 2 * b * s * hkv * d * 2
    bytes_int8 = 2 * b * s * hkv * (d + 4)
    layers = max(2, -(-pool_bytes // (2 * nblocks * BS * hkv * d)))
    var = variants(s)
    pools = []
    calls = {f"{c}/{name}": [] for c in ("bf16", "int8") for name, _ in var}
    err = None
    for _ in range(layers):
        k = torch.randn(nblocks, BS, hkv, d, device=dev, dtype=torch.bfloat16)
        v = torch.randn(nblocks, BS, hkv, d, device=dev, dtype=torch.bfloat16)
        kc, vc = torch.empty_like(k, dtype=torch.int8), torch.empty_like(v, dtype=torch.int8)
        ks = torch.empty(nblocks, BS, hkv, device=dev, dtype=torch.float32)
        vs = torch.empty_like(ks)
        blk = torch.arange(nblocks, device=dev).repeat_interleave(BS)
        off = torch.arange(BS, device=dev).repeat(nblocks)
        hot.kv_cache_quant_append(k.reshape(-1, hkv, d), v.reshape(-1, hkv, d),
                                  kc, vc, ks, vs, blk, off)
        pools.append((k, v, kc, vc, ks, vs))     # the graphs hold raw pointers
        for name, n in var:
            calls[f"bf16/{name}"].append(
                lambda k=k, v=v, n=n: hot.paged_decode_attention(
                    q, k, v, table, lens, num_splits=n))
            calls[f"int8/{name}"].append(
                lambda kc=kc, vc=vc, ks=ks, vs=vs, n=n:
                hot.paged_decode_attention(q, kc, vc, table, lens, k_scale=ks,
                                           v_scale=vs, num_splits=n))
        if err is None:
            o16 = calls["bf16/old"][0]().float()
            o8 = calls["int8/old"][0]().float()
            err = float((o8 - o16).abs().max() / o16.abs().max())
            # every variant against its own yardstick, relative to max |out|
            split_err = {c: max(float((calls[f"{c}/{name}"][0]().float() - o)
                                      .abs().max() / o.abs().max())
                                for name, _ in var[1:])
                         for c, o in (("bf16", o16), ("int8", o8))}
        del blk, off
    passes = {name: capture_pass(c) for name, c in calls.items()}
    times = {name: [] for name in passes}
    for name in passes:                      # warm-up replay
        time_pass(passes[name])
    for _ in range(repeats):
        for name in passes:                  # alternate the variants
            times[name].append(time_pass(passes[name]))
    row = {"b": b, "h": h, "hkv": hkv, "d": d, "s": s, "layers": layers,
           "int8_vs_bf16_relerr": err, "split_vs_old_relerr": split_err,
           "auto_splits": {c: hot._decode_attn_split_plan(b, h, hkv, d, nb * BS,
                                                          c == "int8")
                           for c in ("bf16", "int8")}}
    for c, nbytes in (("bf16", bytes_bf16), ("int8", bytes_int8)):
        for name, _ in var:
            ts = times[f"{c}/{name}"]
            t = statistics.median(ts)
            row[c if name == "old" else f"{c}/{name}"] = {
                "us": t * 1e6, "mean_us": statistics.mean(ts) * 1e6,
                "min_us": min(ts) * 1e6, "max_us": max(ts) * 1e6,
                "tbps": nbytes / t * 1e-12, "bytes": nbytes,
                "us_all": [x * 1e6 for x in ts]}
    return row


def verdict(row, c, name):
    """win / lose / tie of a variant against its yardstick (module doc)."""
    old, x = row[c], row[f"{c}/{name}"]
    if x["mean_us"] < old["min_us"]:
        return "win"
    if x["mean_us"] > old["mean_us"] + (old["max_us"] - old["min_us"]):
        return "LOSE"
    return "tie"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pool-gb", type=float, default=1.0,
                    help="int8 code bytes cycled per variant (bf16 is twice that)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="write the raw results as JSON")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_decode_attn needs a GPU"
    torch.manual_seed(0)
    results = []
    for b, h, hkv, d, s in SHAPES:
        r = bench_shape(b, h, hkv, d, s, int(args.pool_gb * 1e9), args.repeats)
        results.append(r)
        print(f"B{b} H{h} HKV{hkv} D{d} S{s} x{r['layers']}: "
              f"bf16 {r['bf16']['us']:7.1f}us {r['bf16']['tbps']:5.2f}TB/s  "
              f"int8 {r['int8']['us']:7.1f}us {r['int8']['tbps']:5.2f}TB/s  "
              f"int8/bf16 time {r['int8']['us'] / r['bf16']['us']:.3f}  "
              f"relerr {r['int8_vs_bf16_relerr']:.4f}", flush=True)
        for c in ("bf16", "int8"):
            o = r[c]
            line = (f"    {c} old {o['mean_us']:7.1f} [{o['min_us']:.1f}, "
                    f"{o['max_us']:.1f}] | auto n={r['auto_splits'][c]}")
            for name, _ in variants(s)[1:]:
                x = r[f"{c}/{name}"]
                # a plan of 1 is the yardstick's own kernel, measured twice
                v = ("same kernel" if name == "auto" and r["auto_splits"][c] == 1
                     else verdict(r, c, name))
                line += f" | {name} {x['mean_us']:.1f} {x['tbps']:.2f}TB/s {v}"
            print(line + f" | split relerr {r['split_vs_old_relerr'][c]:.4f}",
                  flush=True)
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
