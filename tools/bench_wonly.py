"""Weight-only decode GEMM timing: int8 vs int4 (per-channel, gs 64, gs 128).

HBM-cold discipline: every variant cycles through a pool of weight copies
whose packed bytes exceed --pool-gb (default 1.6 GB, several times the
256 MB L3), so no call finds its weights in a cache.  Device events time one
pass over the pool; passes of int8 and the int4 variants alternate in one
process and the median of --repeats passes is reported, as us per call and
effective TB/s of packed weight bytes (scales and activations not counted).

--mxfp4: the MXFP4 decode streamer (W4A16) against int4 (per-channel, gs 128)
and against the fp4 x fp4 path (mx_quant_fp4 + gemm_mxfp4_nt per call) on the
serving shapes at M 8 and 32; mxfp4 bytes count codes and e8m0 scales,
N K (1/2 + 1/32).  Mean and minimum over the passes are printed for the
win rule (a mean below the other side's minimum).
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
MX_SHAPES = [(m, k, n) for k, n in [(4096, 12288), (4096, 4096), (11008, 4096)]
             for m in (8, 32)]
MX_VARIANTS = [("mxfp4-w4a16", "weight_only_mxfp4", -1),
               ("int4-gs128", "weight_only_int4", 128),
               ("int4-pc", "weight_only_int4", -1),
               ("mxfp4-w4a4", "weight_only_mxfp4", -1)]


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


def make_call(name, x, q, s, wd, gs):
    if name == "mxfp4-w4a4":                 # quantize x per call + fp4 GEMM
        from paddle_amd.incubate.mx import MXFP4Linear
        return lambda layer=MXFP4Linear(q, s): layer(x)
    return lambda: Q.weight_only_linear(x, q, s, weight_dtype=wd, group_size=gs)


def bench_shape(m, k, n, pool_bytes, repeats, variants=VARIANTS):
    x = torch.randn(m, k, device="cuda", dtype=torch.bfloat16)
    w = torch.randn(k, n, device="cuda") * 0.02
    ref = x.float() @ w
    copies = max(4, -(-pool_bytes // (k * n // 2)))
    rows, passes, pools = {}, {}, []
    for name, algo, gs in variants:
        qw, sc = Q.weight_quantize(w.to(torch.bfloat16) if "mxfp4" in algo else w,
                                   algo=algo, group_size=gs)
        wd = algo.rsplit("_", 1)[1]
        got = make_call(name, x, qw, sc, wd, gs)().float()
        rows[name] = {"packed_bytes": qw.numel() + (sc.numel() if wd == "mxfp4" else 0),
                      "relerr": float((got - ref).abs().max() / ref.abs().max())}
        pool = [(qw.clone(), sc.clone()) for _ in range(copies)]
        pools.append(pool)                   # the graph holds raw pointers
        passes[name] = capture_pass([make_call(name, x, q, s, wd, gs)
                                     for q, s in pool])
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
                          us_mean=statistics.mean(times[name]) * 1e6,
                          us_min=min(times[name]) * 1e6,
                          us_all=[v * 1e6 for v in times[name]])
    return {"m": m, "k": k, "n": n, "copies": copies, "variants": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pool-gb", type=float, default=1.6,
                    help="pool size in int4 packed bytes (int8 pool is twice that)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--mxfp4", action="store_true",
                    help="MXFP4 decode streamer vs int4 and the fp4 x fp4 path")
    ap.add_argument("--out", default=None, help="write the raw results as JSON")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_wonly needs a GPU"
    results = []
    for m, k, n in (MX_SHAPES if args.mxfp4 else SHAPES):
        r = bench_shape(m, k, n, int(args.pool_gb * 1e9), args.repeats,
                        MX_VARIANTS if args.mxfp4 else VARIANTS)
        results.append(r)
        cols = "  ".join(f"{name} {v['us']:7.1f}us (mean {v['us_mean']:.1f} min "
                         f"{v['us_min']:.1f}) {v['tbps']:5.2f}TB/s err {v['relerr']:.3f}"
                         for name, v in r["variants"].items())
        print(f"M{m} K{k} N{n} x{r['copies']}: {cols}", flush=True)
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
