"""Paged decode attention timing: the bf16 cache kernel vs the int8 cache
kernel (decode_attn.hip) on the same shapes.

HBM-cold discipline (as bench_wonly.py): every variant cycles through
`layers` pools (one per model layer) whose bytes exceed --pool-gb, several
times the 256 MB L3, so no call finds its cache in a cache.  The pools are
sized from real block tables (randperm block order, ceil(S/bs) blocks per
sequence).  One pass over the layers is a hipGraph timed with device events;
bf16 and int8 passes alternate in one process and the median of --repeats
passes is reported as us per call and TB/s of cache bytes read (K and V codes
of the S valid positions, int8 scales included; q, the table and the output
are not counted).
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
          for s in (128, 512, 2048, 4096)] + [(1, 32, 32, 128, 4096),
                                              (1, 32, 8, 128, 4096)]
BS = 16


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
    pools, calls = [], {"bf16": [], "int8": []}
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
        calls["bf16"].append(lambda k=k, v=v: hot.paged_decode_attention(
            q, k, v, table, lens))
        calls["int8"].append(lambda kc=kc, vc=vc, ks=ks, vs=vs:
                             hot.paged_decode_attention(q, kc, vc, table, lens,
                                                        k_scale=ks, v_scale=vs))
        if err is None:
            o16, o8 = calls["bf16"][0]().float(), calls["int8"][0]().float()
            err = float((o8 - o16).abs().max() / o16.abs().max())
        del blk, off
    passes = {name: capture_pass(c) for name, c in calls.items()}
    times = {name: [] for name in passes}
    for name in passes:                      # warm-up replay
        time_pass(passes[name])
    for _ in range(repeats):
        for name in passes:                  # alternate the variants
            times[name].append(time_pass(passes[name]))
    row = {"b": b, "h": h, "hkv": hkv, "d": d, "s": s, "layers": layers,
           "int8_vs_bf16_relerr": err}
    for name, nbytes in (("bf16", bytes_bf16), ("int8", bytes_int8)):
        t = statistics.median(times[name])
        row[name] = {"us": t * 1e6, "tbps": nbytes / t * 1e-12, "bytes": nbytes,
                     "us_all": [x * 1e6 for x in times[name]]}
    return row


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
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
