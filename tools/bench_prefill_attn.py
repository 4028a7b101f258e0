"""Paged prefill attention timing (prefill_attn.hip): `chunk` new tokens per
sequence attend to `prefix + chunk` cached positions.

Variants, alternating in one process:
  new     paged_prefill_attention on the paged cache.
  gather  yardstick (a), what a user had to write before the op existed:
          gather each sequence's cached rows through the block table into
          contiguous K/V (dequantising an int8 cache to bf16, repeating kv
          heads for GQA, which the varlen kernel needs) and call
          flash_attn_varlen_func, bottom-right causal.
  decode  yardstick (b), q_len = 1 rows only: paged_decode_attention with its
          default dispatch on the same cache.

HBM-cold discipline (as bench_decode_attn.py): every variant cycles through
`layers` pools whose bytes exceed --pool-gb, several times the 256 MB L3.
One pass over the layers is timed with device events (eager launches: the
varlen binding reads cu_seqlens on the host, so no variant is captured); the
variants alternate and the mean, min and max of --repeats passes are
reported as us per call.  `new` wins when its mean is below the yardstick's
minimum; it loses when its mean is above the yardstick's mean plus the
yardstick's spread (max - min).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from paddle_amd.ops import functional as hot  # noqa: E402

BS = 16
# (B, H, HKV, D, chunk, prefix)
PREFILL = [(4, 32, hkv, 128, chunk, prefix) for hkv in (32, 8)
           for chunk in (512, 2048) for prefix in (0, 2048, 16384)]
DECODE = [(b, 32, 8, 128, 1, s - 1) for b in (4, 32) for s in (2048, 16384)]


def time_pass(calls):
    start, stop = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    torch.cuda.synchronize()
    start.record()
    for c in calls:
        c()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e-3 / len(calls)


def gather_call(q, k, v, ks, vs, table, cu_q, cu_k, S, rep, chunk):
    """Yardstick (a) for one pool."""
    B, nb = table.shape
    hkv, d = k.shape[2], k.shape[3]
    idx = table.long().reshape(-1)

    def call():
        kk = k[idx].reshape(B, nb * BS, hkv, d)[:, :S]
        vv = v[idx].reshape(B, nb * BS, hkv, d)[:, :S]
        if ks is not None:
            kk = (kk.float() * ks[idx].reshape(B, nb * BS, hkv, 1)[:, :S]
                  ).to(torch.bfloat16)
            vv = (vv.float() * vs[idx].reshape(B, nb * BS, hkv, 1)[:, :S]
                  ).to(torch.bfloat16)
        kk = kk.reshape(B * S, hkv, d)
        vv = vv.reshape(B * S, hkv, d)
        if rep > 1:
            kk = kk.repeat_interleave(rep, dim=1)
            vv = vv.repeat_interleave(rep, dim=1)
        return hot.flash_attn_varlen_func(q, kk, vv, cu_q, cu_k, chunk, S,
                                          causal=True)
    return call


def bench_shape(b, h, hkv, d, chunk, prefix, pool_bytes, repeats, decode):
    dev = "cuda"
    S = prefix + chunk
    nb = -(-S // BS)
    nblocks = b * nb
    table = torch.randperm(nblocks, device=dev).int().reshape(b, nb)
    lens = torch.full((b,), S, dtype=torch.int32, device=dev)
    cu_q = torch.arange(b + 1, dtype=torch.int32, device=dev) * chunk
    cu_k = torch.arange(b + 1, dtype=torch.int32, device=dev) * S
    q = torch.randn(b * chunk, h, d, device=dev, dtype=torch.bfloat16)
    layers = max(2, min(64, -(-pool_bytes // (2 * nblocks * BS * hkv * d))))
    names = ["new", "decode" if decode else "gather"]
    calls = {f"{c}/{n}": [] for c in ("bf16", "int8") for n in names}
    pools, err = [], {}
    for _ in range(layers):
        k = torch.randn(nblocks, BS, hkv, d, device=dev, dtype=torch.bfloat16)
        v = torch.randn(nblocks, BS, hkv, d, device=dev, dtype=torch.bfloat16)
        kc, vc = (torch.empty_like(k, dtype=torch.int8) for _ in range(2))
        ks = torch.empty(nblocks, BS, hkv, device=dev, dtype=torch.float32)
        vs = torch.empty_like(ks)
        blk = torch.arange(nblocks, device=dev).repeat_interleave(BS)
        off = torch.arange(BS, device=dev).repeat(nblocks)
        hot.kv_cache_quant_append(k.reshape(-1, hkv, d), v.reshape(-1, hkv, d),
                                  kc, vc, ks, vs, blk, off)
        del blk, off
        pools.append((k, v, kc, vc, ks, vs))
        for c, (pk, pv, sk, sv) in (("bf16", (k, v, None, None)),
                                    ("int8", (kc, vc, ks, vs))):
            calls[f"{c}/new"].append(
                lambda pk=pk, pv=pv, sk=sk, sv=sv: hot.paged_prefill_attention(
                    q, pk, pv, table, lens, cu_q, chunk, k_scale=sk, v_scale=sv))
            if decode:
                calls[f"{c}/decode"].append(
                    lambda pk=pk, pv=pv, sk=sk, sv=sv: hot.paged_decode_attention(
                        q, pk, pv, table, lens, k_scale=sk, v_scale=sv))
            else:
                calls[f"{c}/gather"].append(gather_call(
                    q, pk, pv, sk, sv, table, cu_q, cu_k, S, h // hkv, chunk))
        if not err:
            for c in ("bf16", "int8"):
                new = calls[f"{c}/new"][0]().float()
                old = calls[f"{c}/{names[1]}"][0]().float()
                err[c] = float((new - old).abs().max() / old.abs().max())
    times = {n: [] for n in calls}
    for n in calls:                          # warm-up pass
        time_pass(calls[n])
    for _ in range(repeats):
        for n in calls:                      # alternate the variants
            times[n].append(time_pass(calls[n]))
    row = {"b": b, "h": h, "hkv": hkv, "d": d, "chunk": chunk, "prefix": prefix,
           "layers": layers, "yardstick": names[1], "new_vs_yardstick_relerr": err}
    for n, ts in times.items():
        row[n] = {"mean_us": statistics.mean(ts) * 1e6, "min_us": min(ts) * 1e6,
                  "max_us": max(ts) * 1e6, "us_all": [x * 1e6 for x in ts]}
    return row


def verdict(row, c):
    """win / lose / tie of `new` against the row's yardstick (module doc)."""
    old, x = row[f"{c}/{row['yardstick']}"], row[f"{c}/new"]
    if x["mean_us"] < old["min_us"]:
        return "win"
    if x["mean_us"] > old["mean_us"] + (old["max_us"] - old["min_us"]):
        return "LOSE"
    return "tie"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pool-gb", type=float, default=1.0,
                    help="bf16 K bytes cycled per variant")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="write the raw results as JSON")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_prefill_attn needs a GPU"
    torch.manual_seed(0)
    results = []
    for decode, shapes in ((False, PREFILL), (True, DECODE)):
        for b, h, hkv, d, chunk, prefix in shapes:
            r = bench_shape(b, h, hkv, d, chunk, prefix,
                            int(args.pool_gb * 1e9), args.repeats, decode)
            results.append(r)
            line = (f"B{b} H{h} HKV{hkv} D{d} chunk{chunk} prefix{prefix} "
                    f"x{r['layers']}:")
            for c in ("bf16", "int8"):
                n, o = r[f"{c}/new"], r[f"{c}/{r['yardstick']}"]
                line += (f" | {c} new {n['mean_us']:.1f} [{n['min_us']:.1f}, "
                         f"{n['max_us']:.1f}] {r['yardstick']} {o['mean_us']:.1f} "
                         f"[{o['min_us']:.1f}, {o['max_us']:.1f}] "
                         f"{verdict(r, c)} relerr "
                         f"{r['new_vs_yardstick_relerr'][c]:.4f}")
            print(line, flush=True)
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
