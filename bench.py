#!/usr/bin/env python3
"""Flagship benchmark: GPT-3-6.7B, Fleet sharding stage-3, bf16.

Driver contract (BASELINE.json): tokens/sec whole-node on N GPUs of one
node, weak scaling (fixed per-GPU batch), synthetic data, random-init
weights.  Launched directly (N=1) or via torch.distributed.run with one
rank per GPU over RCCL.

  python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times K steps and prints one JSON line.
--dump-outputs DIR also writes what the last timed step computed (loss,
logits, updated parameters) as DIR/<name>.npy so two builds can be
compared output for output; the seed fixes weights and data, so the
same arguments give the same inputs on every run.
"""
from __future__ import annotations

import argparse
import json
import os
import time

import torch

# --dump-outputs caps: elements per sampled array / per parameter tensor
# (float32, so the three files together stay far below 64 MB)
_DUMP_MAX_ELEMS = 1 << 22
_DUMP_PER_PARAM = 4096
_DUMP_SEED = 20240917


def _sample(t, max_elems, gen):
    """Whole tensor as flat float32 numpy, or a fixed seeded sample of it."""
    flat = t.detach().reshape(-1)
    if flat.numel() > max_elems:
        idx = torch.randint(0, flat.numel(), (max_elems,), generator=gen)
        flat = flat[idx.to(flat.device)]
    return flat.float().cpu().numpy()


def dump_outputs(out_dir, loss, logits, state, write):
    """Write the last timed step's results as float32 .npy files.  The
    sample indices depend only on the shapes, so they match across runs."""
    import numpy as np
    gen = torch.Generator().manual_seed(_DUMP_SEED)
    arrays = {
        "loss": loss.detach().float().reshape(1).cpu().numpy(),
        "logits": _sample(logits, _DUMP_MAX_ELEMS, gen),
        "params": np.concatenate([_sample(state[k], _DUMP_PER_PARAM, gen)
                                  for k in sorted(state)]),
    }
    if not write:
        return
    os.makedirs(out_dir, exist_ok=True)
    for name, arr in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), arr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--model", type=str, default="gpt3-6.7b")
    # b12 measured fastest-safe on 288 GB: 21.1k tok/s @ 229 GB peak vs
    # 20.6k @ 195 GB (b8) and 21.3k @ 263 GB (b16, too tight with RCCL buffers)
    ap.add_argument("--batch", type=int, default=12, help="per-GPU micro batch")
    ap.add_argument("--seq", type=int, default=2048)
    ap.add_argument("--sharding-stage", type=int, default=3)
    ap.add_argument("--recompute", action="store_true")
    ap.add_argument("--cpu-smoke", action="store_true",
                    help="tiny CPU run for plumbing checks")
    ap.add_argument("--tunableop", action="store_true",
                    help="autotune hipBLASLt GEMM algo selection during warmup")
    ap.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                    help="after the timed steps write the last step's loss, "
                         "logits and updated parameters (seeded samples of "
                         "the large ones) to DIR/<name>.npy")
    ap.add_argument("--full", action="store_true",
                    help="also run every secondary measurement; bench.py has "
                         "none beyond the headline figure today, so this "
                         "changes nothing yet")
    args = ap.parse_args()

    if args.tunableop:
        import torch.cuda.tunable as tunable
        tunable.enable(True)
        tunable.tuning_enable(True)
        tunable.set_max_tuning_duration(20)

    import paddle_amd as paddle
    from paddle_amd.distributed import fleet
    from paddle_amd.distributed.fleet.sharding import (GroupShardedStage3,
                                                       ShardedAdamW)
    from paddle_amd.models import GPTPretrainingCriterion, build_gpt

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    on_gpu = torch.cuda.is_available() and not args.cpu_smoke

    if world > 1:
        paddle.distributed.init_parallel_env()
    if on_gpu:
        local = int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(local)
        paddle.set_device(f"gpu:{local}")

    model_name = args.model
    if args.cpu_smoke:
        model_name = "gpt3-tiny"
        args.seq = min(args.seq, 128)

    paddle.seed(1234 + rank)
    model = build_gpt(model_name, max_seq_len=args.seq,
                      use_recompute=args.recompute)
    loss_fn = GPTPretrainingCriterion()
    dtype = torch.bfloat16 if on_gpu else torch.float32
    dev = torch.device("cuda", torch.cuda.current_device()) if on_gpu else torch.device("cpu")
    model = model.to(device=dev, dtype=dtype)

    if args.sharding_stage == 3 or world == 1:
        # stage-3 flat-shard path (degenerates cleanly at world == 1)
        wrapped = GroupShardedStage3(model, device=dev)
        opt = ShardedAdamW(wrapped, learning_rate=1e-4, beta1=0.9, beta2=0.95,
                           epsilon=1e-8, weight_decay=0.1,
                           grad_clip=paddle.nn.ClipGradByGlobalNorm(1.0))
    else:
        from paddle_amd.distributed.fleet.sharding import group_sharded_parallel
        inner = paddle.optimizer.AdamW(
            learning_rate=1e-4, beta1=0.9, beta2=0.95, weight_decay=0.1,
            parameters=model.parameters(),
            grad_clip=paddle.nn.ClipGradByGlobalNorm(1.0))
        level = {1: "os", 2: "os_g"}[args.sharding_stage]
        wrapped, opt, _ = group_sharded_parallel(model, inner, level)

    vocab = model.cfg.vocab_size
    ids = torch.randint(0, vocab, (args.batch, args.seq), device=dev)
    labels = torch.randint(0, vocab, (args.batch, args.seq), device=dev)

    kept = {}

    def step(keep=False):
        logits = wrapped(ids)
        loss = loss_fn(logits, labels)
        if keep:
            kept["logits"] = logits.detach()
        del logits
        loss.backward()
        opt.step()
        opt.clear_grad()
        return loss

    for _ in range(args.warmup):
        step()

    if args.tunableop:
        import torch.cuda.tunable as tunable
        tunable.tuning_enable(False)
        step()  # one settled step after tuning

    if world > 1:
        paddle.distributed.barrier()
    if on_gpu:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        loss = step(keep=args.dump_outputs is not None and i == args.steps - 1)
    if on_gpu:
        torch.cuda.synchronize()
    if world > 1:
        paddle.distributed.barrier()
    elapsed = time.perf_counter() - t0

    # max over ranks
    if world > 1:
        t = torch.tensor([elapsed], device=dev if on_gpu else "cpu")
        paddle.distributed.all_reduce(t, op=paddle.distributed.ReduceOp.MAX)
        elapsed = float(t.item())

    if args.dump_outputs is not None:
        # state_dict() gathers sharded parameters, so every rank takes part
        dump_outputs(args.dump_outputs, loss, kept.pop("logits"),
                     wrapped.state_dict(), write=rank == 0)

    n_gpus = world if world > 1 else (1 if on_gpu else 0) or 1
    total_tokens = args.batch * args.seq * args.steps * n_gpus
    tps = total_tokens / elapsed
    ms_per_step = elapsed / args.steps * 1000.0

    if rank == 0:
        out = {
            "metric": "tokens/sec (whole node) GPT-3-6.7B Fleet sharding-3",
            "value": round(tps, 1),
            "unit": "tokens/s",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 2),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "bf16" if on_gpu else "float32",
            "data": "synthetic",
            "config": {
                "model": model_name,
                "global_batch": args.batch * n_gpus,
                "seq_len": args.seq,
                "parallelism": f"sharding{args.sharding_stage}_dp{n_gpus}",
                "loss": round(float(loss.detach().float().cpu()), 4),
                "peak_mem_gb": (round(torch.cuda.max_memory_allocated() / 2**30, 2)
                                if on_gpu else None),
            },
        }
        print(json.dumps(out))


if __name__ == "__main__":
    main()
