"""Continuous-batching serving engine over the paged-KV decode path.

The reference ships the kernel side of serving (fused_multi_transformer +
block_multihead_attention's paged "block" KV cache,
paddle/phi/kernels/fusion/gpu/block_multi_head_attention_kernel.cu); the
engine loop itself lives out-of-tree (FastDeploy).  This module provides
the MI355X-native equivalent end to end:

  * a block allocator over the paged cache (free-list, per-request block
    tables) sized for 288 GB HBM3E,
  * a continuous-batching scheduler: requests join the running batch as
    soon as blocks are free, finished requests release their blocks
    immediately (no head-of-line blocking on the longest sequence),
  * decode steps batched across active requests through
    `paged_decode_attention` (one wavefront-parallel kernel per layer).

`GenerationServer.serve_http` exposes an OpenAI-style /v1/completions on
FastAPI when uvicorn is wanted; the engine itself is framework-free.
"""
from __future__ import annotations

import time
from dataclasses import dataclass, field
from typing import Callable, Optional

import torch


@dataclass
class Request:
    prompt_ids: list
    max_new_tokens: int = 32
    temperature: float = 0.0      # 0 => greedy
    top_p: float = 1.0
    eos_token_id: Optional[int] = None
    # engine state
    rid: int = -1
    out_ids: list = field(default_factory=list)
    done: bool = False
    enqueue_t: float = 0.0
    first_token_t: float = 0.0
    finish_t: float = 0.0


class BlockAllocator:
    """Free-list allocator over the paged KV pool (block granularity)."""

    def __init__(self, num_blocks):
        self.free = list(range(num_blocks - 1, -1, -1))

    def alloc(self, n):
        if len(self.free) < n:
            return None
        return [self.free.pop() for _ in range(n)]

    def release(self, blocks):
        self.free.extend(blocks)


class Engine:
    """Continuous-batching loop around a decode-capable model.

    The model contract (satisfied by models.generation helpers):
      prefill(ids [1, S]) -> (logits [1, S, V], per_layer_kv)  and
      decode_step(token [B, 1], cache_state) -> logits [B, V]
    For round 1 the engine drives `models.generation.generate_gpt`-style
    callables; scheduling (admission, block accounting, eviction on
    completion) is engine-owned and unit-tested on CPU.
    """

    def __init__(self, step_fn: Callable, num_blocks=1024, block_size=16,
                 max_batch=64):
        self.step_fn = step_fn            # (active requests) -> {rid: token}
        self.alloc = BlockAllocator(num_blocks)
        self.block_size = block_size
        self.max_batch = max_batch
        self.waiting: list[Request] = []
        self.active: list[Request] = []
        self.blocks: dict[int, list] = {}
        self._next_rid = 0
        self.completed: list[Request] = []

    # -- API -----------------------------------------------------------------
    def add_request(self, req: Request):
        req.rid = self._next_rid
        self._next_rid += 1
        req.enqueue_t = time.perf_counter()
        self.waiting.append(req)
        return req.rid

    def _blocks_needed(self, req):
        total = len(req.prompt_ids) + req.max_new_tokens
        return (total + self.block_size - 1) // self.block_size

    def _admit(self):
        admitted = []
        while self.waiting and len(self.active) < self.max_batch:
            req = self.waiting[0]
            blks = self.alloc.alloc(self._blocks_needed(req))
            if blks is None:
                break                     # not enough KV blocks yet
            self.blocks[req.rid] = blks
            self.active.append(self.waiting.pop(0))
            admitted.append(req)
        return admitted

    def _retire(self, req):
        req.done = True
        req.finish_t = time.perf_counter()
        self.alloc.release(self.blocks.pop(req.rid))
        self.active.remove(req)
        self.completed.append(req)

    def step(self):
        """One engine iteration: admit, run one decode step, retire."""
        self._admit()
        if not self.active:
            return 0
        new_tokens = self.step_fn(self.active, self.blocks)
        for req in list(self.active):
            tok = new_tokens.get(req.rid)
            if tok is None:
                continue
            if not req.out_ids:
                req.first_token_t = time.perf_counter()
            req.out_ids.append(tok)
            if (len(req.out_ids) >= req.max_new_tokens or
                    (req.eos_token_id is not None and tok == req.eos_token_id)):
                self._retire(req)
        return len(new_tokens)

    def run_until_done(self, max_steps=100000):
        steps = 0
        while (self.waiting or self.active) and steps < max_steps:
            self.step()
            steps += 1
        return steps

    # -- metrics ---------------------------------------------------------------
    def stats(self):
        done = self.completed
        if not done:
            return {}
        ttft = [r.first_token_t - r.enqueue_t for r in done if r.first_token_t]
        lat = [r.finish_t - r.enqueue_t for r in done]
        toks = sum(len(r.out_ids) for r in done)
        span = max(r.finish_t for r in done) - min(r.enqueue_t for r in done)
        return {"requests": len(done), "output_tokens": toks,
                "tokens_per_s": toks / max(span, 1e-9),
                "mean_ttft_s": sum(ttft) / max(len(ttft), 1),
                "mean_latency_s": sum(lat) / len(lat)}


def sample_token(logits, temperature=0.0, top_p=1.0):
    """Greedy / temperature / nucleus sampling over [V] logits."""
    if temperature <= 0.0:
        return int(logits.argmax(-1))
    probs = torch.softmax(logits.float() / temperature, dim=-1)
    if top_p < 1.0:
        sp, si = probs.sort(descending=True)
        keep = sp.cumsum(-1) - sp < top_p
        sp = sp * keep
        sp = sp / sp.sum()
        return int(si[torch.multinomial(sp, 1)])
    return int(torch.multinomial(probs, 1))


class GenerationServer:
    """OpenAI-style /v1/completions over the engine (FastAPI)."""

    def __init__(self, engine: Engine, tokenizer=None):
        self.engine = engine
        self.tokenizer = tokenizer

    def app(self):
        from fastapi import FastAPI
        from pydantic import BaseModel

        class CompletionIn(BaseModel):
            prompt: list
            max_tokens: int = 32
            temperature: float = 0.0
            top_p: float = 1.0

        api = FastAPI(title="paddle_amd serving")

        @api.post("/v1/completions")
        def complete(body: CompletionIn):
            req = Request(prompt_ids=list(body.prompt),
                          max_new_tokens=body.max_tokens,
                          temperature=body.temperature, top_p=body.top_p)
            self.engine.add_request(req)
            self.engine.run_until_done()
            return {"choices": [{"token_ids": req.out_ids}],
                    "usage": {"completion_tokens": len(req.out_ids)}}

        @api.post("/v1/completions/stream")
        def complete_stream(body: CompletionIn):
            """Server-sent events: one `data:` line per generated token."""
            from fastapi.responses import StreamingResponse

            req = Request(prompt_ids=list(body.prompt),
                          max_new_tokens=body.max_tokens,
                          temperature=body.temperature, top_p=body.top_p)
            self.engine.add_request(req)

            def gen():
                import json
                sent = 0
                while not req.done:
                    self.engine.step()
                    while sent < len(req.out_ids):
                        yield f"data: {json.dumps({'token_id': req.out_ids[sent]})}\n\n"
                        sent += 1
                yield "data: [DONE]\n\n"
            return StreamingResponse(gen(), media_type="text/event-stream")

        @api.get("/stats")
        def stats():
            return self.engine.stats()

        return api

    def serve(self, host="127.0.0.1", port=8000):
        import uvicorn
        uvicorn.run(self.app(), host=host, port=port)


# ---------------------------------------------------------------------------
# GPT model runner: dynamic-batch decode over a shared paged pool
# ---------------------------------------------------------------------------
class GPTModelRunner:
    """Engine step_fn for GPTForPretraining: per-request block tables from
    the engine's allocator, one batched paged-decode step per call.
    Admission prefills the new request through the flash-attention path, or
    with prefill_chunk=N at most N prompt tokens per call through
    `paged_prefill_attention` over the cache; decode runs every active
    request through `paged_decode_attention`."""

    def __init__(self, model, num_blocks=1024, block_size=16,
                 device=None, dtype=None, max_seq=2048, use_graphs=True,
                 weight_only=False, weight_only_group_size=-1,
                 kv_cache="bf16", decode_splits=None, prefill_chunk=None):
        import math
        from .ops import functional as hot
        self.hot = hot
        self.model = model.eval()
        # prefill_chunk=None: a prompt is prefilled whole, in one
        # flash-attention pass, when its request is admitted.  N >= 1:
        # chunked prefill -- each call gives the prefilling requests, in
        # admission order, at most N prompt tokens in all and runs them as one
        # packed pass through paged_prefill_attention over the cache
        # (docs/SERVING.md "chunked prefill")
        if prefill_chunk is not None and (
                isinstance(prefill_chunk, bool)
                or not isinstance(prefill_chunk, int) or prefill_chunk < 1):
            raise ValueError("prefill_chunk must be None or an integer >= 1, "
                             f"got {prefill_chunk!r}")
        self.prefill_chunk = prefill_chunk
        self._prefilled = {}         # rid -> prompt tokens cached so far
        # decode_splits -> paged_decode_attention(num_splits=): None lets the
        # shape heuristic choose (bucket B and max_seq only, so each bucket's
        # graph is fixed), 0 pins the one-block-per-q-head kernels, n >= 1
        # forces the split-KV kernels with n splits (docs/KERNELS.md
        # "split-KV decode attention")
        if decode_splits is not None and (
                int(decode_splits) != decode_splits
                or not 0 <= decode_splits <= 64):
            raise ValueError("decode_splits must be None or an integer in "
                             f"[0, 64], got {decode_splits!r}")
        self.decode_splits = decode_splits
        # kv_cache="int8": int8 code pools + per-token fp32 scale pools
        # (about half the KV bytes; docs/KERNELS.md "int8 KV cache")
        if kv_cache not in ("bf16", "int8"):
            raise ValueError(f"kv_cache must be 'bf16' or 'int8', got {kv_cache!r}")
        self.kv_int8 = kv_cache == "int8"
        if weight_only:
            # weight-only decode: True | "int8" (~2x less weight memory) or
            # "int4" (~4x less, weight_only_group_size -1 | 64 | 128);
            # decode linears run the MFMA W-streaming int8 / int4 kernel
            if weight_only is not True and weight_only not in ("int8", "int4"):
                raise ValueError("weight_only must be False, True, 'int8' or "
                                 f"'int4', got {weight_only!r}")
            wdt = "int8" if weight_only is True else weight_only
            from .quantization import quantize_linears_
            quantize_linears_(self.model, skip=("lm_head", "embeddings"),
                              algo=f"weight_only_{wdt}",
                              group_size=weight_only_group_size)
        cfg = model.cfg
        self.H = cfg.num_heads
        self.HKV = getattr(cfg, "num_kv_heads", cfg.num_heads)   # GQA-aware
        self.D = cfg.hidden_size // self.H
        self.scale = 1.0 / math.sqrt(self.D)
        self.bs = block_size
        dev = device or next(iter(model.state_dict().values())).device
        dt = dtype or model.lm_head.weight.dtype
        self.dev = dev
        # +1 scratch block: hipGraph-padded rows write their (discarded) KV
        # into it so every captured bucket replays with fixed shapes
        self.scratch_blk = num_blocks
        self.k = [torch.zeros(num_blocks + 1, block_size, self.HKV, self.D,
                              device=dev,
                              dtype=torch.int8 if self.kv_int8 else dt)
                  for _ in range(cfg.num_layers)]
        self.v = [torch.zeros_like(self.k[0]) for _ in range(cfg.num_layers)]
        # the scratch block has scale rows too; None for the bf16 cache
        self.k_scale = [torch.zeros(num_blocks + 1, block_size, self.HKV,
                                    device=dev, dtype=torch.float32)
                        if self.kv_int8 else None
                        for _ in range(cfg.num_layers)]
        self.v_scale = [torch.zeros_like(s) if self.kv_int8 else None
                        for s in self.k_scale]
        self.seq_len = {}            # rid -> tokens currently cached
        self.last_token = {}         # rid -> next input token
        self.max_blk = (max_seq + block_size - 1) // block_size
        # graphs need the native decode kernel (the python fallback syncs
        # on seq_lens, which is illegal during stream capture)
        from . import _ext
        native_ok = (dev.type == "cuda" and dt == torch.bfloat16 and
                     self.D in (64, 128) and _ext.has_ext())
        self.use_graphs = use_graphs and native_ok
        self._graphs = {}            # bucket B -> (graph, static tensors)

    def _kv_write(self, li, blk, off, k, v):
        """Store k/v rows [..., HKV, D] at (blk, off) [...] of layer li."""
        if not self.kv_int8:
            self.k[li][blk, off] = k
            self.v[li][blk, off] = v
            return
        self.hot.kv_cache_quant_append(
            k.reshape(-1, self.HKV, self.D), v.reshape(-1, self.HKV, self.D),
            self.k[li], self.v[li], self.k_scale[li], self.v_scale[li],
            blk.reshape(-1).contiguous(), off.reshape(-1).contiguous())

    def _qkv(self, layer, x):
        b, s, _ = x.shape
        return (layer.attn.qkv_proj(x)
                .reshape(b, s, 3, self.H, self.D).unbind(2))

    @torch.no_grad()
    def _prefill(self, reqs, blocks):
        """Batched prefill for same-prompt-length requests (one flash-
        attention pass for the whole group)."""
        m = self.model
        N = len(reqs)
        S0 = len(reqs[0].prompt_ids)
        ids = torch.tensor([r.prompt_ids for r in reqs], dtype=torch.long).to(
            self.dev, non_blocking=True)
        pos = torch.arange(S0, device=self.dev)
        blk_t = torch.tensor([blocks[r.rid] for r in reqs],
                             dtype=torch.long).to(self.dev, non_blocking=True)
        blks = blk_t[:, pos // self.bs]          # [N, S0]
        offs = (pos % self.bs).unsqueeze(0).expand(N, S0)
        x = m.gpt.embeddings(ids)
        for li, layer in enumerate(m.gpt.layers):
            h = layer.ln1(x)
            q, k, v = self._qkv(layer, h)
            self._kv_write(li, blks, offs, k, v)
            att, _ = self.hot.flash_attention(q, k, v, causal=True)
            x = x + layer.attn.out_proj(att.reshape(N, S0, -1))
            x = x + layer.mlp(layer.ln2(x))
        logits = m.lm_head(m.gpt.final_norm(x[:, -1]))
        for i, r in enumerate(reqs):
            self.seq_len[r.rid] = S0
            self.last_token[r.rid] = sample_token(logits[i], r.temperature,
                                                  r.top_p)

    @torch.no_grad()
    def _prefill_chunked(self, reqs, blocks):
        """One chunked-prefill pass: the prefilling requests `reqs`, in
        admission order, take prompt tokens until prefill_chunk tokens are
        used up; those T <= prefill_chunk tokens run as one packed pass.
        Returns {rid: first generated token} of the requests whose prompt
        completed; the others stay prefilling."""
        N = self.prefill_chunk
        budget, take = N, []
        for r in reqs:
            if budget == 0:
                break
            done = self._prefilled.get(r.rid, 0)
            n = min(budget, len(r.prompt_ids) - done)
            take.append((r, done, n))
            budget -= n
        ids, pos, blk, off, rows, lens, cu, last, fin = [], [], [], [], [], [], [0], [], []
        for r, done, n in take:
            bl = blocks[r.rid]
            ids += r.prompt_ids[done:done + n]
            pos += range(done, done + n)
            blk += [bl[p // self.bs] for p in range(done, done + n)]
            off += [p % self.bs for p in range(done, done + n)]
            rows.append(bl + [0] * (self.max_blk - len(bl)))
            lens.append(done + n)            # cached so far + this chunk
            cu.append(cu[-1] + n)
            if done + n == len(r.prompt_ids):
                last.append(cu[-1] - 1)
                fin.append(r)

        def dev(x, dt):
            return torch.tensor(x, dtype=dt).to(self.dev, non_blocking=True)
        x = self._chunk_forward(dev(ids, torch.long), dev(pos, torch.long),
                                dev(blk, torch.long), dev(off, torch.long),
                                dev(rows, torch.int32), dev(lens, torch.int32),
                                dev(cu, torch.int32))
        for r, done, n in take:
            self._prefilled[r.rid] = done + n
        out = {}
        if fin:
            logits = self._chunk_logits(x[dev(last, torch.long)])
            for i, r in enumerate(fin):
                del self._prefilled[r.rid]
                self.seq_len[r.rid] = len(r.prompt_ids)
                self.last_token[r.rid] = sample_token(logits[i], r.temperature,
                                                      r.top_p)
                out[r.rid] = self.last_token[r.rid]
        return out

    def _chunk_forward(self, ids, pos, blk, off, table, lens, cu_q):
        """Hidden states [T, hidden] of T packed prompt tokens at their own
        positions `pos`; their K/V go to (blk, off) of every layer before the
        layer's attention reads the cache."""
        m = self.model
        T = ids.shape[0]
        x = m.gpt.embeddings(ids[None], pos[None])
        for li, layer in enumerate(m.gpt.layers):
            h = layer.ln1(x)
            q, k, v = self._qkv(layer, h)
            self._kv_write(li, blk, off, k[0], v[0])
            att = self.hot.paged_prefill_attention(
                q[0], self.k[li], self.v[li], table, lens, cu_q,
                self.prefill_chunk, self.scale,
                k_scale=self.k_scale[li], v_scale=self.v_scale[li])
            x = x + layer.attn.out_proj(att.reshape(1, T, -1))
            x = x + layer.mlp(layer.ln2(x))
        return x[0]

    def _chunk_logits(self, x):
        return self.model.lm_head(self.model.gpt.final_norm(x))

    @torch.no_grad()
    def __call__(self, active, blocks):
        m = self.model
        out = {}
        new = [r for r in active if r.rid not in self.seq_len]
        if new and self.prefill_chunk is not None:
            out.update(self._prefill_chunked(new, blocks))
        elif new:
            by_len = {}
            for r in new:
                by_len.setdefault(len(r.prompt_ids), []).append(r)
            for group in by_len.values():
                self._prefill(group, blocks)
            for r in new:
                out[r.rid] = self.last_token[r.rid]  # first generated token
        rest = [r for r in active if r not in new]
        if not rest:
            return out
        B = len(rest)
        Bp = B if not self.use_graphs else self._bucket(B)
        comp = tuple(r.rid for r in rest)
        all_greedy = all(r.temperature <= 0.0 for r in rest)
        # steady-state fast path: same composition as last step, graph
        # captured, greedy -- advance lens / rotate tokens entirely on
        # device (zero H2D per step)
        if (self.use_graphs and all_greedy and
                comp == getattr(self, "_last_comp", None) and
                Bp in self._graphs and
                getattr(self, "_picked_dev", None) is not None):
            g, st = self._graphs[Bp]
            st["toks"][:B, 0] = self._picked_dev[:B]
            st["lens"][:B] += 1
            st["pos"].copy_(st["lens"].long().unsqueeze(1))
            st["wblk"].copy_(st["table"].long().gather(
                1, st["pos"] // self.bs).squeeze(1))
            st["wblk"][B:] = self.scratch_blk
            st["woff"].copy_((st["pos"] % self.bs).squeeze(1))
            g.replay()
            self._picked_dev = st["logits"][:B].argmax(-1)
            picked = self._picked_dev.tolist()
            for i, r in enumerate(rest):
                t = int(picked[i])
                self.seq_len[r.rid] += 1
                self.last_token[r.rid] = t
                out[r.rid] = t
            return out
        # build once on host, ship with ONE copy (per-row H2D was per-step
        # launch overhead)
        rows = []
        lens_l = []
        for r in rest:
            bl = blocks[r.rid]
            rows.append(bl + [0] * (self.max_blk - len(bl)))
            lens_l.append(self.seq_len[r.rid])
        for _ in range(Bp - B):
            rows.append([self.scratch_blk] + [0] * (self.max_blk - 1))
            lens_l.append(0)
        table = torch.tensor(rows, dtype=torch.int32).to(self.dev,
                                                         non_blocking=True)
        lens = torch.tensor(lens_l, dtype=torch.int32).to(self.dev,
                                                          non_blocking=True)
        toks = torch.tensor([[self.last_token[r.rid]] for r in rest] +
                            [[0]] * (Bp - B), dtype=torch.long).to(
                                self.dev, non_blocking=True)
        pos_ids = lens.long().unsqueeze(1)
        write_blk = table.long().gather(1, (pos_ids // self.bs)).squeeze(1)
        write_off = (pos_ids % self.bs).squeeze(1)
        write_blk[B:] = self.scratch_blk
        logits = self._decode(Bp, toks, pos_ids, table, lens, write_blk,
                              write_off)
        if all_greedy:
            # greedy for the whole batch: ONE argmax + ONE device sync
            self._picked_dev = logits[:B].argmax(-1)
            self._last_comp = comp
            picked = self._picked_dev.tolist()
        else:
            self._last_comp = None
            picked = [sample_token(logits[i], r.temperature, r.top_p)
                      for i, r in enumerate(rest)]
        for i, r in enumerate(rest):
            t = int(picked[i])
            self.seq_len[r.rid] += 1
            self.last_token[r.rid] = t
            out[r.rid] = t
        return out

    @staticmethod
    def _bucket(b):
        n = 1
        while n < b:
            n *= 2
        return n

    def _decode_forward(self, B, toks, pos_ids, table, lens, write_blk,
                        write_off):
        m = self.model
        x = m.gpt.embeddings(toks, pos_ids)
        for li, layer in enumerate(m.gpt.layers):
            h = layer.ln1(x)
            q, k, v = self._qkv(layer, h)
            self._kv_write(li, write_blk, write_off, k[:, 0], v[:, 0])
            att = self.hot.paged_decode_attention(
                q.reshape(B, self.H, self.D), self.k[li], self.v[li],
                table, lens + 1, self.scale,
                k_scale=self.k_scale[li], v_scale=self.v_scale[li],
                num_splits=self.decode_splits)
            x = x + layer.attn.out_proj(att.reshape(B, 1, -1))
            x = x + layer.mlp(layer.ln2(x))
        return m.lm_head(m.gpt.final_norm(x[:, 0]))

    def precapture(self, buckets=(1, 2, 4, 8, 16, 32)):
        """Capture the decode hipGraphs for the given batch buckets ahead
        of serving (otherwise the first request of each bucket pays
        2 warmup steps + capture, which lands in its ttft)."""
        if not self.use_graphs:
            return
        dev = self.dev
        for B in buckets:
            if B in self._graphs:
                continue
            toks = torch.zeros(B, 1, dtype=torch.long, device=dev)
            pos = torch.zeros(B, 1, dtype=torch.long, device=dev)
            rows = torch.full((B, self.max_blk), 0, dtype=torch.int32, device=dev)
            rows[:, 0] = self.scratch_blk
            lens = torch.zeros(B, dtype=torch.int32, device=dev)
            wblk = torch.full((B,), self.scratch_blk, dtype=torch.long, device=dev)
            woff = torch.zeros(B, dtype=torch.long, device=dev)
            self._decode(B, toks, pos, rows, lens, wblk, woff)
        torch.cuda.synchronize()

    def _decode(self, B, toks, pos_ids, table, lens, write_blk, write_off):
        if not self.use_graphs:
            return self._decode_forward(B, toks, pos_ids, table, lens,
                                        write_blk, write_off)
        # hipGraph per batch bucket: decode is launch-bound (~200 small
        # kernels/step); one graph replay replaces them all
        entry = self._graphs.get(B)
        if entry is None:
            st = {"toks": toks.clone(), "pos": pos_ids.clone(),
                  "table": table.clone(), "lens": lens.clone(),
                  "wblk": write_blk.clone(), "woff": write_off.clone()}
            stream = torch.cuda.Stream()
            stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(stream):
                for _ in range(2):   # warmup outside capture
                    self._decode_forward(B, st["toks"], st["pos"], st["table"],
                                         st["lens"], st["wblk"], st["woff"])
            torch.cuda.current_stream().wait_stream(stream)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                st["logits"] = self._decode_forward(
                    B, st["toks"], st["pos"], st["table"], st["lens"],
                    st["wblk"], st["woff"])
            entry = (g, st)
            self._graphs[B] = entry
        g, st = entry
        st["toks"].copy_(toks)
        st["pos"].copy_(pos_ids)
        st["table"].copy_(table)
        st["lens"].copy_(lens)
        st["wblk"].copy_(write_blk)
        st["woff"].copy_(write_off)
        g.replay()
        return st["logits"]


class LlamaModelRunner(GPTModelRunner):
    """Engine step_fn for LlamaForCausalLM: GQA paged KV (num_kv_heads
    cache planes), rope applied at each request's OWN position via a
    gathered cos/sin table (graph-capture-safe: the gather reads a
    static pos tensor updated before replay), RMSNorm + swiglu layers."""

    def __init__(self, model, *args, **kwargs):
        super().__init__(model, *args, **kwargs)
        cfg = model.cfg
        from .ops.functional import build_rope_cache
        cos, sin = build_rope_cache(self.max_blk * self.bs, self.D,
                                    cfg.rope_base, self.dev)
        self._rope_cos = cos.to(torch.float32)        # [S, D/2]
        self._rope_sin = sin.to(torch.float32)
        # fuse q/k/v into ONE decode GEMM per layer (3 separate skinny
        # GEMMs read the same activations 3x and hit hipBLASLt's weak
        # small-N tiles); bf16 weights become views into the fused matrix
        self._qkv_fused = []
        for layer in model.llama.layers:
            a = layer.self_attn
            projs = (a.q_proj, a.k_proj, a.v_proj)
            if all(hasattr(p, "qweight") for p in projs):   # weight-only
                # entry: (weight dtype, qweight, scale, group size).  int8
                # [K, N] and packed int4 [K/2, N] both concatenate along n;
                # per-channel scales are [N], group scales [K/gs, N]
                wdt, gs = a.q_proj.weight_dtype, a.q_proj.group_size
                qw = torch.cat([p.qweight for p in projs], dim=1).contiguous()
                sc = torch.cat([p.scale for p in projs],
                               dim=a.q_proj.scale.dim() - 1).contiguous()
                self._qkv_fused.append((wdt, qw, sc, gs))
            elif all(getattr(p, "weight", None) is not None for p in projs):
                w = torch.cat([p.weight for p in projs], dim=1).contiguous()
                qo = a.q_proj.weight.shape[1]
                ko = a.k_proj.weight.shape[1]
                a.q_proj.weight.data = w[:, :qo]
                a.k_proj.weight.data = w[:, qo:qo + ko]
                a.v_proj.weight.data = w[:, qo + ko:]
                self._qkv_fused.append(("bf16", w, None, -1))
            else:
                # mixed (e.g. GQA k/v under quantize_linears_' min_features
                # cutoff while q was converted): run the module calls
                self._qkv_fused.append(("none", None, None, -1))

    def _rope_rows(self, x, pos):
        """x [B, 1, H, D] at per-row absolute positions pos [B] (long)."""
        c = self._rope_cos[pos].view(-1, 1, 1, self.D // 2).to(x.dtype)
        s = self._rope_sin[pos].view(-1, 1, 1, self.D // 2).to(x.dtype)
        x1, x2 = x[..., : self.D // 2], x[..., self.D // 2:]
        return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)

    def _qkv(self, layer, x):           # prefill path (positions 0..S0)
        b, s, _ = x.shape
        a = layer.self_attn
        q = a.q_proj(x).reshape(b, s, self.H, self.D)
        k = a.k_proj(x).reshape(b, s, self.HKV, self.D)
        v = a.v_proj(x).reshape(b, s, self.HKV, self.D)
        q, k = self.hot.fused_rotary_position_embedding(
            q, k, base=self.model.cfg.rope_base)
        return q, k, v

    @torch.no_grad()
    def _prefill(self, reqs, blocks):
        m = self.model
        N = len(reqs)
        S0 = len(reqs[0].prompt_ids)
        ids = torch.tensor([r.prompt_ids for r in reqs], dtype=torch.long).to(
            self.dev, non_blocking=True)
        pos = torch.arange(S0, device=self.dev)
        blk_t = torch.tensor([blocks[r.rid] for r in reqs],
                             dtype=torch.long).to(self.dev, non_blocking=True)
        blks = blk_t[:, pos // self.bs]
        offs = (pos % self.bs).unsqueeze(0).expand(N, S0)
        x = m.llama.embed_tokens(ids)
        for li, layer in enumerate(m.llama.layers):
            h = layer.input_layernorm(x)
            q, k, v = self._qkv(layer, h)
            self._kv_write(li, blks, offs, k, v)
            att, _ = self.hot.flash_attention(q, k, v, causal=True)
            x = x + layer.self_attn.o_proj(att.reshape(N, S0, -1))
            x = x + layer.mlp(layer.post_attention_layernorm(x))
        logits = m.lm_head(m.llama.norm(x[:, -1]))
        for i, r in enumerate(reqs):
            self.seq_len[r.rid] = S0
            self.last_token[r.rid] = sample_token(logits[i], r.temperature,
                                                  r.top_p)

    def _chunk_forward(self, ids, pos, blk, off, table, lens, cu_q):
        m = self.model
        T = ids.shape[0]
        x = m.llama.embed_tokens(ids[None])
        for li, layer in enumerate(m.llama.layers):
            h = layer.input_layernorm(x).reshape(T, -1)
            a = layer.self_attn
            # rope at each token's own position (the decode path's gather)
            q = self._rope_rows(a.q_proj(h).reshape(T, 1, self.H, self.D), pos)
            k = self._rope_rows(a.k_proj(h).reshape(T, 1, self.HKV, self.D), pos)
            v = a.v_proj(h).reshape(T, self.HKV, self.D)
            self._kv_write(li, blk, off, k[:, 0], v)
            att = self.hot.paged_prefill_attention(
                q[:, 0], self.k[li], self.v[li], table, lens, cu_q,
                self.prefill_chunk, self.scale,
                k_scale=self.k_scale[li], v_scale=self.v_scale[li])
            x = x + a.o_proj(att.reshape(1, T, -1))
            x = x + layer.mlp(layer.post_attention_layernorm(x))
        return x[0]

    def _chunk_logits(self, x):
        return self.model.lm_head(self.model.llama.norm(x))

    def _decode_forward(self, B, toks, pos_ids, table, lens, write_blk,
                        write_off):
        m = self.model
        a_pos = lens.long()                 # absolute position of new token
        x = m.llama.embed_tokens(toks)
        qo = self.H * self.D
        ko = self.HKV * self.D
        for li, layer in enumerate(m.llama.layers):
            h = layer.input_layernorm(x)
            kind, w, sc, gs = self._qkv_fused[li]
            h2 = h.reshape(B, -1)
            at = layer.self_attn
            if kind in ("int8", "int4"):
                from .quantization import weight_only_linear
                qkv = weight_only_linear(h2, w, sc, weight_dtype=kind,
                                         group_size=gs)
            elif kind == "bf16":
                qkv = torch.matmul(h2, w)
            else:
                qkv = torch.cat([at.q_proj(h2), at.k_proj(h2), at.v_proj(h2)],
                                dim=-1)
            q = qkv[:, :qo].reshape(B, 1, self.H, self.D)
            k = qkv[:, qo:qo + ko].reshape(B, 1, self.HKV, self.D)
            v = qkv[:, qo + ko:].reshape(B, 1, self.HKV, self.D)
            q = self._rope_rows(q, a_pos)
            k = self._rope_rows(k, a_pos)
            self._kv_write(li, write_blk, write_off, k[:, 0], v[:, 0])
            att = self.hot.paged_decode_attention(
                q.reshape(B, self.H, self.D), self.k[li], self.v[li],
                table, lens + 1, self.scale,
                k_scale=self.k_scale[li], v_scale=self.v_scale[li],
                num_splits=self.decode_splits)
            x = x + layer.self_attn.o_proj(att.reshape(B, 1, -1))
            x = x + layer.mlp(layer.post_attention_layernorm(x))
        return m.lm_head(m.llama.norm(x[:, 0]))
