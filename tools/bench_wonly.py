"""Weight-only decode GEMM timing: int8 vs int4 (per-channel, gs 64, gs 128).

HBM-cold discipline: every variant cycles through a pool of weight copies
whose packed bytes exceed --pool-gb (default 1.6 GB, several times the
256 MB L3), so no call finds its weights in a cache.  Device events time one
pass over the pool; passes of int8 and the int4 variants alternate in one
process and the median of --repeats passes is reported, as us per call and
effective TB/s of packed weight bytes (scales and activations not counted).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from paddle_amd import quantization as Q  # noqa: E402

SHAPES = [(32, 4096, 12288), (32, 4096, 4096), (32, 4096, 16384),
          (32, 16384, 4096), (1, 4096, 16384), (16, 4096, 16384)]
VARIANTS = [("int8", "weight_only_int8", -1), ("int4-pc", "weight_only_int4", -1),
            ("int4-gs64", "weight_only_int4", 64),
            ("int4-gs128", "weight_only_int4", 128)]


def capture_pass(calls):
    """One pass over the pool as a hipGraph: the calls are 10-40 us kernels,
    so eager Python dispatch would time the host, not the device."""
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


def bench_shape(m, k, n, pool_bytes, repeats):
    x = torch.randn(m, k, device="cuda", dtype=torch.bfloat16)
    w = torch.randn(k, n, device="cuda") * 0.02
    ref = x.float() @ w
    copies = max(4, -(-pool_bytes // (k * n // 2)))
    rows, passes, pools = {}, {}, []
    for name, algo, gs in VARIANTS:
        qw, sc = Q.weight_quantize(w, algo=algo, group_size=gs)
        wd = algo.rsplit("_", 1)[1]
        got = Q.weight_only_linear(x, qw, sc, weight_dtype=wd, group_size=gs).float()
        rows[name] = {"packed_bytes": qw.numel(),
                      "relerr": float((got - ref).abs().max() / ref.abs().max())}
        pool = [(qw.clone(), sc.clone()) for _ in range(copies)]
        pools.append(pool)                   # the graph holds raw pointers
        passes[name] = capture_pass([
            (lambda q=q, s=s, wd=wd, gs=gs: Q.weight_only_linear(
                x, q, s, weight_dtype=wd, group_size=gs)) for q, s in pool])
    del w
    times = {name: [] for name in passes}
    for name in passes:                      # warm-up replay
        time_pass(passes[name])
    for _ in range(repeats):
        for name in passes:                  # alternate the variants
            times[name].append(time_pass(passes[name]))
    for name in passes:
        t = statistics.median(times[name])
        rows[name].update(us=t * 1e6, tbps=rows[name]["packed_bytes"] / t * 1e-12,
                          us_all=[v * 1e6 for v in times[name]])
    return {"m": m, "k": k, "n": n, "copies": copies, "variants": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pool-gb", type=float, default=1.6,
                    help="pool size in int4 packed bytes (int8 pool is twice that)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="write the raw results as JSON")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_wonly needs a GPU"
    results = []
    for m, k, n in SHAPES:
        r = bench_shape(m, k, n, int(args.pool_gb * 1e9), args.repeats)
        results.append(r)
        cols = "  ".join(f"{name} {v['us']:7.1f}us {v['tbps']:5.2f}TB/s err {v['relerr']:.3f}"
                         for name, v in r["variants"].items())
        print(f"M{m} K{k} N{n} x{r['copies']}: {cols}", flush=True)
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
