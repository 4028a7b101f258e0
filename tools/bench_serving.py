"""Serving throughput: continuous batching on GPT-350M-ish config, 1 GPU.

Measures decode tokens/s and mean TTFT with staggered arrivals through
the paged-KV engine.
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import paddle_amd as paddle  # noqa: E402
from paddle_amd.models import build_gpt  # noqa: E402
from paddle_amd.models.gpt import GPTConfig, GPTForPretraining  # noqa: E402
from paddle_amd.serving import Engine, GPTModelRunner, Request  # noqa: E402


def run_one(tag, model, n_req=64, prompt_len=128, gen_len=128, max_batch=32,
            num_blocks=4096, weight_only=False, runner_cls="gpt",
            group_size=-1, kv_cache="bf16", decode_splits=None,
            prefill_chunk=None):
    cls = GPTModelRunner
    if runner_cls == "llama":
        from paddle_amd.serving import LlamaModelRunner
        cls = LlamaModelRunner
    runner = cls(model, num_blocks=num_blocks, block_size=16,
                 max_seq=max(2048, prompt_len + gen_len),
                 weight_only=weight_only, weight_only_group_size=group_size,
                 kv_cache=kv_cache, decode_splits=decode_splits,
                 prefill_chunk=prefill_chunk)
    pools = runner.k + runner.v + [s for s in runner.k_scale + runner.v_scale
                                   if s is not None]
    pool_gb = sum(t.numel() * t.element_size() for t in pools) / 2**30
    runner.precapture((max_batch,))    # decode graph capture out of ttft
    eng = Engine(runner, num_blocks=num_blocks, block_size=16,
                 max_batch=max_batch)
    import random
    random.seed(0)
    V = model.cfg.vocab_size
    for _ in range(n_req):
        eng.add_request(Request(
            prompt_ids=[random.randrange(V) for _ in range(prompt_len)],
            max_new_tokens=gen_len))
    t0 = time.perf_counter()
    # prefill wave (all same-length prompts); with --prefill-chunk only the
    # first chunk, and the steps counted below interleave prefill and decode
    eng.step()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    tok0 = sum(len(r.out_ids) for r in (eng.active + eng.completed + eng.waiting))
    n_steps = 0
    while eng.active or eng.waiting:
        eng.step()
        n_steps += 1
        if n_steps > 200000:
            break
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    dt_dec = time.perf_counter() - t1
    s = eng.stats()
    dec_toks = s["output_tokens"] - tok0
    print(f"serving {tag}: {n_req} reqs x (p{prompt_len}+g{gen_len}) in {dt:.1f}s"
          f"  decode {s['output_tokens'] / dt:.0f} tok/s (incl prefill)"
          f"  steady-decode {dec_toks / dt_dec:.0f} tok/s"
          f" ({dt_dec / max(n_steps,1) * 1e3:.2f} ms/step)"
          f"  ttft {s['mean_ttft_s'] * 1e3:.0f} ms"
          f"  kv pools {pool_gb:.2f} GB"
          f"  peak {torch.cuda.max_memory_allocated() / 2**30:.1f} GB")


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="gpt-350m",
                    choices=["gpt-350m", "gpt3-6.7b", "llama2-7b"])
    ap.add_argument("--weight-only", action="store_true",
                    help="weight-only decode (MFMA W-streamer); int8 unless "
                         "--weight-only-dtype says otherwise")
    ap.add_argument("--weight-only-dtype", choices=["int8", "int4"],
                    default=None, help="implies --weight-only")
    ap.add_argument("--group-size", type=int, default=-1,
                    choices=[-1, 64, 128], help="int4 scale group size")
    ap.add_argument("--kv-cache", choices=["bf16", "int8"], default="bf16",
                    help="paged KV pool format (int8: codes + per-token scales)")
    ap.add_argument("--prompt-len", type=int, default=128)
    ap.add_argument("--gen-len", type=int, default=128)
    ap.add_argument("--n-req", type=int, default=64)
    ap.add_argument("--max-batch", type=int, default=32,
                    help="engine batch limit (and the pre-captured bucket)")
    ap.add_argument("--decode-splits", type=int, default=None,
                    help="runner decode_splits: unset = heuristic, 0 = "
                         "one-block-per-q-head kernels, n = split-KV kernels")
    ap.add_argument("--prefill-chunk", type=int, default=None,
                    help="runner prefill_chunk: unset = whole-prompt prefill, "
                         "n = at most n prompt tokens per engine step")
    args = ap.parse_args()
    paddle.seed(0)
    wo = args.weight_only_dtype or ("int8" if args.weight_only else False)
    tag_sfx = ""
    if wo:
        tag_sfx = f" {wo}-wo" + (f"-gs{args.group_size}" if args.group_size > 0 else "")
    if args.kv_cache != "bf16":
        tag_sfx += f" {args.kv_cache}-kv"
    if args.decode_splits is not None:
        tag_sfx += f" splits={args.decode_splits}"
    if args.prefill_chunk is not None:
        tag_sfx += f" chunk={args.prefill_chunk}"
    if args.max_batch != 32:
        tag_sfx += f" b{args.max_batch}"
    kw = dict(weight_only=wo, group_size=args.group_size,
              kv_cache=args.kv_cache, prompt_len=args.prompt_len,
              gen_len=args.gen_len, n_req=args.n_req,
              max_batch=args.max_batch, decode_splits=args.decode_splits,
              prefill_chunk=args.prefill_chunk)
    seq = max(2048, args.prompt_len + args.gen_len)
    # blocks for max_batch sequences of prompt+gen tokens, with headroom
    nblk = max(8192, 2 * 32 * (-(-seq // 16)))
    if args.model == "gpt-350m":
        cfg = GPTConfig(vocab_size=50304, hidden_size=1024, num_layers=24,
                        num_heads=16, intermediate_size=4096, max_seq_len=seq)
        m = GPTForPretraining(cfg).to("cuda", torch.bfloat16)
        run_one("gpt-350M" + tag_sfx, m, **kw)
    elif args.model == "gpt3-6.7b":
        m = build_gpt("gpt3-6.7b", max_seq_len=seq).to("cuda", torch.bfloat16)
        run_one("gpt3-6.7B" + tag_sfx, m, num_blocks=nblk, **kw)
    else:
        from paddle_amd.models.llama import build_llama
        m = build_llama("llama2-7b", max_seq_len=seq).to("cuda", torch.bfloat16)
        run_one("llama2-7B" + tag_sfx, m, num_blocks=nblk, runner_cls="llama",
                **kw)


if __name__ == "__main__":
    main()
