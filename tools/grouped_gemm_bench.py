"""Ragged grouped GEMM against what the capacity path runs for the same
matmul (T 8192, k 2, E 64, h 1024, I 4096; cap 513).
  NN  x . w1 (+ b1)        vs torch.baddbmm over [E, cap, h]
  NT  dy . w2^T            vs gemm_bf16_nt_batched over [E, cap, h]
  TN  x^T . dz per expert  vs torch.bmm(x^T, dz) over [E, cap, .]
TF/s counts the occupied rows only (T * k = 16384) on both sides.
--side grouped | capacity | both: which path this process runs, so that the
two can alternate in separate processes (under rocprofv3 --kernel-trace
--stats the kernel names tell the calls apart); --routing uniform | skewed
(one expert at 8x the mean) shapes the grouped side.  Times printed here are
device events."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import paddle_amd as paddle  # noqa: E402

T, K, E, H, I, CAP = 8192, 2, 64, 1024, 4096, 513


def timed(fn, iters=20):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--routing", choices=("uniform", "skewed"), default="uniform")
    ap.add_argument("--side", choices=("grouped", "capacity", "both"), default="both")
    args = ap.parse_args()
    C = paddle._ext.get_ext()
    torch.manual_seed(0)
    R = T * K
    bf = dict(device="cuda", dtype=torch.bfloat16)
    w1, b1, w2 = torch.randn(E, H, I, **bf), torch.randn(E, I, **bf), torch.randn(E, I, H, **bf)
    flops = 2.0 * R * H * I
    rows = []
    if args.side != "capacity":
        sizes = torch.full((E,), R // E)
        if args.routing == "skewed":
            sizes[0] = 8 * (R // E)
            sizes[1:] = (R - int(sizes[0])) // (E - 1)
            sizes[1] += R - int(sizes.sum())
        offsets = torch.cat([sizes.new_zeros(1), sizes.cumsum(0)]).int().cuda()
        topi = torch.rand(T, E, device="cuda").argsort(1)[:, :K].int().contiguous()
        x, dz, dy = torch.randn(R, H, **bf), torch.randn(R, I, **bf), torch.randn(R, H, **bf)
        plan = C.grouped_gemm_plan(offsets, R)
        rows += [
            ("grouped_gemm_plan", lambda: C.grouped_gemm_plan(offsets, R), None),
            ("moe_route_ragged", lambda: C.moe_route_ragged(topi, E), None),
            ("NN grouped x.w1+b1", lambda: C.grouped_gemm_bf16(x, w1, offsets, plan, 0, b1), flops),
            ("NT grouped dy.w2^T", lambda: C.grouped_gemm_bf16(dy, w2, offsets, plan, 1, None), flops),
            ("TN grouped x^T.dz", lambda: C.grouped_gemm_bf16(x, dz, offsets, None, 2, None), flops),
        ]
    if args.side != "grouped":
        xc, dzc, dyc = (torch.randn(E, CAP, H, **bf), torch.randn(E, CAP, I, **bf),
                        torch.randn(E, CAP, H, **bf))
        rows += [
            ("NN baddbmm cap 513", lambda: torch.baddbmm(b1.unsqueeze(1), xc, w1), flops),
            ("NT gemm_bf16_nt_batched cap 513", lambda: C.gemm_bf16_nt_batched(dyc, w2), flops),
            ("TN bmm cap 513", lambda: torch.bmm(xc.transpose(1, 2), dzc), flops),
        ]
    for name, fn, fl in rows:
        ms = timed(fn)
        rate = f"  {fl / ms * 1e-9:7.1f} TF/s on occupied rows" if fl else ""
        print(f"grouped_gemm_bench routing={args.routing} {name}: {ms * 1e3:9.1f} us{rate}", flush=True)


if __name__ == "__main__":
    main()
