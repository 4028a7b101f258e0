"""Paged prefill attention without a GPU: the reference and the cases shared
with test_prefill_attn_gpu.py, a fp32 emulation of paged_prefill_kernel's
design showing that the bound accepts it and rejects the mistakes such a
kernel can make, the torch path of paged_prefill_attention, its q_len = 1
agreement with paged_decode_attention, the dispatch predicate, and chunked
prefill scheduling in the runners.

Reference: a packed token (b, i) with q_len_b new tokens and S_b cached
positions is a decode query of length S_b - q_len_b + i + 1 over sequence
b's table row, so the fp64 reference is the decode reference of
test_kv_int8_gpu.py / test_decode_attn_split_gpu.py (softmax(scale q k^^T) v^
from the bf16 q and the STORED cache values) on the expanded batch.  Bound

    |out - ref| <= 2^-7 |ref| + 2^-7 A + 4 E        (compared with <=)

  2^-7 |ref|  one bf16 ulp for the output cast,
  2^-7 A      A = sum_pos p |v^|: one bf16 ulp on every staged P element (P
              crosses an MFMA in bf16; the convention of test_fa_dkv_gpu.py),
  E           max over the output row of |fp32 torch evaluation - fp64|.

No absolute term: a row that sees nothing must be exactly zero.
"""
import itertools
import math

import pytest
import torch

import paddle_amd as paddle
from paddle_amd.ops import functional as hot

from test_decode_attn_split_gpu import _attn_bf16_one, case_of_kind
from test_kv_int8_gpu import (BF16, F32, F64, U_BF16, _attn_one, check,
                              violations)

# (q_len, S): prefix 0 and 1, the 16-row wave tile, the 64-row block tile
# (from q_len * G), the 64-position K tile, page boundaries
PAIRS = [(0, 0), (0, 40), (1, 1), (5, 5), (16, 16), (17, 17), (3, 4), (7, 64),
         (40, 65), (17, 81), (64, 64), (65, 129), (33, 250), (1, 200)]
KINDS = ["int8_token", "int8_head", "bf16"]
SEED_BASE = 3201


# ---------------------------------------------------------------------------
# cases and reference
# ---------------------------------------------------------------------------
def prefill_case(kind, D, H, HKV, bs, pairs, seed, rows=None):
    """A make_case batch (poisoned last block, poisoned unused table entries,
    every table entry in range) with S_b cached positions per sequence, a
    packed q [T, H, D] and cu_q."""
    c = case_of_kind(kind, D, H, HKV, bs, [s for _, s in pairs], seed,
                     rows=rows)
    g = torch.Generator().manual_seed(seed + 1)
    qls = [q for q, _ in pairs]
    c["q"] = torch.randn(sum(qls), H, D, generator=g).to(BF16)
    c["cu_q"] = torch.tensor([0] + list(itertools.accumulate(qls)),
                             dtype=torch.int32)
    return c


def seq_geometry(c):
    """[(b, first packed token, q_len_b, S_b)] with S_b clamped to the table."""
    cu = c["cu_q"].tolist()
    cap = c["table"].shape[1] * c["kc"].shape[1]
    return [(b, cu[b], cu[b + 1] - cu[b], max(0, min(int(c["lens"][b]), cap)))
            for b in range(len(cu) - 1)]


def expand(c):
    """The batch of decode problems, one per packed token."""
    rows, lens = [], []
    for b, _, ql, S in seq_geometry(c):
        for i in range(ql):
            rows.append(b)
            lens.append(max(0, S - ql + i + 1))
    return dict(c, table=c["table"][rows],
                lens=torch.tensor(lens, dtype=torch.int32))


def ref_prefill(c, scale=None):
    """(ref fp64 [T, H, D], bound fp64 [T, H, D]) on CPU tensors."""
    e = {k: (v.cpu() if isinstance(v, torch.Tensor) else v)
         for k, v in expand(c).items()}
    if scale is None:
        scale = 1.0 / math.sqrt(e["q"].shape[-1])

    def run(dt):
        if e["ks"] is None:
            return _attn_bf16_one(e["q"], e["kc"], e["vc"], e["table"],
                                  e["lens"], scale, dt)
        return _attn_one(e["q"], e["kc"], e["vc"], e["ks"], e["vs"],
                         e["table"], e["lens"], scale, dt)
    ref, A = run(F64)
    r32, _ = run(F32)
    E = (r32.to(F64) - ref).abs().amax(-1, keepdim=True)
    bound = U_BF16 * ref.abs() + U_BF16 * A + 4 * E
    assert violations(ref.to(BF16), ref, bound) == 0, \
        "the correctly rounded reference must lie within the bound"
    return ref, bound


def zero_rows(c):
    """Packed tokens that see no position."""
    e = expand(c)
    return e["lens"] == 0


def worst(out, ref, bound):
    """max |out - ref| / bound over elements with a positive bound."""
    err = (out.detach().cpu().to(F64) - ref).abs()
    ok = bound > 0
    return float((err[ok] / bound[ok]).max()) if bool(ok.any()) else 0.0


# ---------------------------------------------------------------------------
# fp32 emulation of paged_prefill_kernel.  `mutant` plants one mistake.
# ---------------------------------------------------------------------------
def emulate(c, mutant=None):
    q, kc, vc, ks, vs, table = (c[k] for k in
                                ("q", "kc", "vc", "ks", "vs", "table"))
    int8 = ks is not None
    T, H, D = q.shape
    bs, HKV = kc.shape[1], kc.shape[2]
    G = H // HKV
    scale = torch.tensor(1.0 / math.sqrt(D), dtype=F32)
    hmap = torch.arange(H) // G
    if mutant == "kv_neighbour":
        hmap = (hmap + 1) % HKV
    out = torch.zeros(T, H, D, dtype=F32)
    for b, t0, ql, S in seq_geometry(c):
        if ql <= 0:
            continue
        i = torch.arange(ql)
        lim = S - ql + i                                   # [ql]
        if mutant == "diag_far":
            lim = torch.clamp(lim + 1, max=S - 1)
        elif mutant == "diag_short":
            lim = lim - 1
        elif mutant == "top_left":
            lim = torch.clamp(i, max=S - 1)
        lim = lim[:, None].expand(ql, H).clone()           # per (token, head)
        if mutant == "row_swap":
            # the limit of row r = i G + g taken from r % G instead of r / G
            r = i[:, None] * G + (torch.arange(H) % G)[None, :]
            lim = S - ql + torch.clamp(r % G, max=ql - 1)
        m = torch.full((ql, H), -1e30, dtype=F32)
        l = torch.zeros(ql, H, dtype=F32)
        o = torch.zeros(ql, H, D, dtype=F32)
        qf = q[t0:t0 + ql].to(F32)
        n_pos = int(lim.max()) + 1 if S > 0 else 0
        for p0 in range(0, n_pos, 64):
            pos = torch.arange(p0, min(p0 + 64, S))
            pb, off = table[b].long()[pos // bs], pos % bs
            kk = kc[pb, off][:, hmap].to(F32)              # [L, H, D]
            vv = vc[pb, off][:, hmap].to(F32)
            mul = scale.expand(len(pos), H)
            dv = torch.ones(len(pos), H, dtype=F32)
            if int8:
                per_tok = ks.dim() == 3
                dk = ks[pb, off][:, hmap] if per_tok else ks[hmap].expand(len(pos), H)
                dv = vs[pb, off][:, hmap] if per_tok else vs[hmap].expand(len(pos), H)
                if mutant == "dk_neighbour":
                    dk = dk.roll(1, 0)
                mul = dk * scale
            s = torch.einsum("qhd,shd->qhs", qf, kk) * mul.t()[None]
            seen = pos[None, None, :] <= lim[:, :, None]
            if mutant == "drop_last":
                seen = seen & (pos != S - 1)[None, None, :]
            s = torch.where(seen, s, torch.full_like(s, -1e30))
            m_new = torch.maximum(m, s.amax(-1))
            corr = torch.exp(m - m_new)
            p = torch.where(seen, torch.exp(s - m_new[..., None]),
                            torch.zeros_like(s))
            l = l * corr + p.sum(-1)
            pt = (p * dv.t()[None]).to(BF16).to(F32)       # P~ crosses the MFMA
            o = o * corr[..., None] + torch.einsum("qhs,shd->qhd", pt, vv)
            m = m_new
        inv = torch.where(l > 0, 1.0 / l, torch.zeros_like(l))
        out[t0:t0 + ql] = o * inv[..., None]
    return out.to(BF16)


MUTANTS = ["diag_far", "diag_short", "top_left", "drop_last", "dk_neighbour",
           "kv_neighbour", "row_swap"]
EMU_SHAPES = [(128, 8, 2, 16), (64, 4, 4, 16), (128, 6, 2, 16), (64, 8, 1, 32)]
EMU_CASES = [(k,) + s for k in ("int8_token", "int8_head") for s in EMU_SHAPES]


def pairs_case(kind, D, H, HKV, bs):
    """The PAIRS batch of one (kind, shape).  A case must be answerable (see
    edge_case of test_decode_attn_split_gpu.py): seed bases 3001 and 3101
    draw a V element that is exactly 0 under a position holding all the
    weight; ref_prefill's assert keeps a later change from drawing another."""
    return prefill_case(kind, D, H, HKV, bs, PAIRS, SEED_BASE + D + 8 * HKV + bs)


@pytest.fixture(scope="module")
def cases():
    out = {}
    for kind in KINDS:
        for D, H, HKV, bs in EMU_SHAPES:
            c = pairs_case(kind, D, H, HKV, bs)
            out[(kind, D, H, HKV, bs)] = (c,) + ref_prefill(c)
    return out


@pytest.mark.parametrize("kind,D,H,HKV,bs", EMU_CASES)
def test_bound_accepts_prefill_design(cases, kind, D, H, HKV, bs):
    """Measured: the emulation sits at 0.41-0.47 of the bound on these
    cases."""
    c, ref, bound = cases[(kind, D, H, HKV, bs)]
    out = emulate(c)
    print(f"{kind} D{D} H{H} HKV{HKV} bs{bs}: err/bound {worst(out, ref, bound):.3f}")
    check(f"{kind} D{D} H{H} HKV{HKV} bs{bs}", out, ref, bound)
    assert bool((out[zero_rows(c)] == 0).all())


# one kv head has no neighbour; per-head scales are the same at every position
MUTANT_CASES = [(m,) + c for m in MUTANTS for c in EMU_CASES
                if not (m == "kv_neighbour" and c[3] == 1)
                and not (m == "dk_neighbour" and c[0] == "int8_head")]


@pytest.mark.parametrize("mutant,kind,D,H,HKV,bs", MUTANT_CASES)
def test_bound_rejects_prefill_mistakes(cases, kind, D, H, HKV, bs, mutant):
    c, ref, bound = cases[(kind, D, H, HKV, bs)]
    out = emulate(c, mutant)
    print(f"{mutant} {kind} D{D} H{H}: worst {worst(out, ref, bound):.3g}x")
    assert violations(out, ref, bound) > 0, mutant


# ---------------------------------------------------------------------------
# torch path
# ---------------------------------------------------------------------------
def call_op(c, q=None, max_q=65, **kw):
    return hot.paged_prefill_attention(
        c["q"] if q is None else q, c["kc"], c["vc"], c["table"], c["lens"],
        c["cu_q"], max_q, k_scale=c["ks"], v_scale=c["vs"], **kw)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D,H,HKV,bs", EMU_SHAPES)
def test_paged_prefill_attention_torch_path(cases, kind, D, H, HKV, bs):
    c, ref, bound = cases[(kind, D, H, HKV, bs)]
    for qdt in (BF16, F32):
        out = call_op(c, q=c["q"].to(qdt))
        assert out.dtype == qdt and out.shape == c["q"].shape
        check(f"{kind} D{D} {qdt}", out, ref, bound)
        assert bool((out[zero_rows(c)] == 0).all())


def test_paged_prefill_attention_torch_path_clamps_and_skips():
    """seq_lens past the table is clamped; an out-of-range table entry
    contributes nothing; scale argument errors."""
    D, H, HKV, bs = 64, 4, 2, 16
    c = prefill_case("int8_token", D, H, HKV, bs, [(5, 40), (3, 20)], 11)
    cap = c["table"].shape[1] * bs
    want = dict(c, lens=torch.tensor([cap, cap], dtype=torch.int32))
    over = dict(c, lens=torch.tensor([cap + 1, 2 ** 31 - 1], dtype=torch.int32))
    assert torch.equal(call_op(over), call_op(want))
    # entry 1 of sequence 0 outside the pool: positions 16..31 drop out
    bad = dict(c, table=c["table"].clone())
    bad["table"][0, 1] = c["kc"].shape[0]
    out = call_op(bad)
    assert bool(torch.isfinite(out.float()).all())
    assert not torch.equal(out[:5], call_op(c)[:5])
    assert torch.equal(out[5:], call_op(c)[5:])
    with pytest.raises(ValueError):
        hot.paged_prefill_attention(c["q"], c["kc"], c["vc"], c["table"],
                                    c["lens"], c["cu_q"], 8, k_scale=c["ks"])
    with pytest.raises(ValueError):
        hot.paged_prefill_attention(c["q"], c["kc"].to(BF16), c["vc"].to(BF16),
                                    c["table"], c["lens"], c["cu_q"], 8,
                                    k_scale=c["ks"], v_scale=c["vs"])


@pytest.mark.parametrize("kind", KINDS)
def test_paged_prefill_q_len_1_is_decode_torch_path(kind):
    """With q_len = 1 everywhere the torch path agrees with
    paged_decode_attention's torch path within fp32 rounding, not bit for
    bit: the two einsums contract in different shapes ("qhd,shd->qhs" on one
    row against "hd,shd->hs"), and the outputs are compared after the same
    bf16 cast with one bf16 ulp of slack on the few elements whose fp32
    values straddle a rounding boundary."""
    D, H, HKV, bs = 128, 8, 2, 16
    lens = [1, 63, 64, 65, 250]
    c = prefill_case(kind, D, H, HKV, bs, [(1, s) for s in lens], 17)
    a = call_op(c, max_q=1).float()
    d = hot.paged_decode_attention(c["q"], c["kc"], c["vc"], c["table"],
                                   c["lens"], k_scale=c["ks"],
                                   v_scale=c["vs"]).float()
    assert bool(((a - d).abs() <= U_BF16 * d.abs()).all())
    assert float((a != d).float().mean()) < 0.02
    a32 = call_op(c, q=c["q"].float(), max_q=1)
    d32 = hot.paged_decode_attention(c["q"].float(), c["kc"], c["vc"],
                                     c["table"], c["lens"], k_scale=c["ks"],
                                     v_scale=c["vs"])
    assert bool(((a32 - d32).abs() <= 2.0 ** -20 * d32.abs().amax(-1, keepdim=True)).all())


# ---------------------------------------------------------------------------
# predicate
# ---------------------------------------------------------------------------
def _ok(a, **kw):
    a = dict(a, **kw)
    return hot._paged_prefill_native_ok(a["q"], a["kc"], a["vc"], a["table"],
                                        a["lens"], a["cu_q"], a["max_q"],
                                        a["ks"], a["vs"])


@pytest.mark.parametrize("kind", ["int8_token", "int8_head", "bf16"])
def test_paged_prefill_native_ok_table(kind):
    """The predicate is pure: it is checked on CPU tensors, mirroring the
    binding's contract."""
    D, H, HKV, bs = 128, 8, 2, 16
    a = prefill_case(kind, D, H, HKV, bs, [(5, 40), (3, 20)], 5)
    a["max_q"] = 8
    assert _ok(a)
    assert _ok(a, table=a["table"].long(), lens=a["lens"].long(),
               cu_q=a["cu_q"].long())
    q, kc, vc = a["q"], a["kc"], a["vc"]
    mis = torch.zeros(q.numel() + 4, dtype=BF16)[4:].view_as(q)
    q96 = torch.zeros(q.shape[0], H, 96, dtype=BF16)
    bad = {
        "q fp32": dict(q=q.float()),
        "q 2-D": dict(q=q[0]),
        "q misaligned": dict(q=mis),
        "q not a tensor": dict(q=None),
        "D 96": dict(q=q96),
        "cache D != q D": dict(q=q[..., :64].contiguous()),
        "H % HKV": dict(q=q[:, :7].contiguous()),
        "cache strided": dict(kc=kc.transpose(1, 2).contiguous().transpose(1, 2)),
        "cache shapes differ": dict(vc=vc[:-1]),
        "cache fp32": dict(kc=kc.float(), vc=vc.float()),
        "one scale": dict(ks=torch.ones(HKV), vs=None),
        "table 1-D": dict(table=a["table"][0]),
        "table rows": dict(table=a["table"][:-1]),
        "table fp32": dict(table=a["table"].float()),
        "lens length": dict(lens=a["lens"][:-1]),
        "lens fp32": dict(lens=a["lens"].float()),
        "cu_q length": dict(cu_q=a["cu_q"][:-1]),
        "cu_q 2-D": dict(cu_q=a["cu_q"].reshape(1, -1)),
        "cu_q fp32": dict(cu_q=a["cu_q"].float()),
        "max_q 0": dict(max_q=0),
        "max_q float": dict(max_q=8.0),
        "max_q bool": dict(max_q=True),
        "max_q * G overflow": dict(max_q=2 ** 29),
    }
    if kind == "bf16":
        bad["bf16 cache with scales"] = dict(ks=torch.ones(HKV), vs=torch.ones(HKV))
    else:
        bad["int8 cache without scales"] = dict(ks=None, vs=None)
        bad["scale fp64"] = dict(ks=a["ks"].double(), vs=a["vs"].double())
    for name, kw in bad.items():
        assert not _ok(a, **kw), name


# ---------------------------------------------------------------------------
# runners: chunked prefill scheduling
# ---------------------------------------------------------------------------
PROMPTS = [[3, 7, 11, 2], [5, 9, 4, 8, 15, 16, 23], list(range(20, 53)),
           [3, 7, 11, 2]]
NEW_TOKENS = 6


def budget_rule(lengths, n):
    """Engine step (1-based) in which each prompt completes: every step hands
    out n prompt tokens in admission order."""
    left, first, step = list(lengths), {}, 0
    while len(first) < len(left):
        step += 1
        budget = n
        for i, rest in enumerate(left):
            if budget == 0:
                break
            if i in first:
                continue
            take = min(budget, rest)
            left[i] -= take
            budget -= take
            if left[i] == 0:
                first[i] = step
    return [first[i] for i in range(len(left))]


def serve_recording(runner_cls, model, monkeypatch, **kw):
    """Run PROMPTS to completion.  Returns (requests, step of each first
    token, first-token logits by request, runner, engine); sample_token is
    only called for first tokens here (greedy decode takes one argmax)."""
    from paddle_amd import serving
    rec = []
    real = serving.sample_token
    with monkeypatch.context() as mp:
        mp.setattr(serving, "sample_token",
                   lambda lg, *a: rec.append(lg.detach().float().cpu().clone())
                   or real(lg, *a))
        runner = runner_cls(model, num_blocks=64, block_size=16, max_seq=128,
                            **kw)
        eng = serving.Engine(runner, num_blocks=64, block_size=16, max_batch=4)
        reqs = [serving.Request(prompt_ids=p, max_new_tokens=NEW_TOKENS)
                for p in PROMPTS]
        for r in reqs:
            eng.add_request(r)
        first, step = {}, 0
        while eng.waiting or eng.active:
            eng.step()
            step += 1
            for i, r in enumerate(reqs):
                if r.out_ids and i not in first:
                    first[i] = step
            assert step < 1000
    assert len(rec) == len(reqs)
    if kw.get("prefill_chunk") is None:
        # whole-prompt prefill samples group by group (equal lengths)
        lens = [len(p) for p in PROMPTS]
        order = sorted(range(len(reqs)), key=lambda i: (lens.index(lens[i]), i))
    else:
        order = sorted(range(len(reqs)), key=lambda i: (first[i], i))
    logits = {i: rec[j] for j, i in enumerate(order)}
    return reqs, [first[i] for i in range(len(reqs))], logits, runner, eng


def prompt_refs(model32):
    """First-token logits of the model's plain fp32 forward on each prompt."""
    with torch.no_grad():
        return [model32(torch.tensor([p]))[0, -1].float().cpu() for p in PROMPTS]


def logit_err(logits, refs):
    return max(float((logits[i] - refs[i]).abs().max()) for i in range(len(refs)))


def _runner_scheduling(runner_cls, model, monkeypatch):
    refs = prompt_refs(model)
    base_reqs, first, lg, base_runner, _ = serve_recording(
        runner_cls, model, monkeypatch, use_graphs=False)
    assert first == [1, 1, 1, 1]
    err_none = logit_err(lg, refs)
    errs = {}
    for n in (1, 5, 16, 64):
        reqs, first, lg, runner, eng = serve_recording(
            runner_cls, model, monkeypatch, use_graphs=False, prefill_chunk=n)
        assert all(r.done and len(r.out_ids) == NEW_TOKENS for r in reqs)
        assert first == budget_rule([len(p) for p in PROMPTS], n), n
        # the last generated token is returned, not cached: the bookkeeping
        # of prefill_chunk=None
        for r, b in zip(reqs, base_reqs):
            assert runner.seq_len[r.rid] == len(r.prompt_ids) + NEW_TOKENS - 1
            assert runner.seq_len[r.rid] == base_runner.seq_len[b.rid]
        assert not runner._prefilled
        assert len(eng.alloc.free) == 64
        errs[n] = logit_err(lg, refs)
        print(f"prefill_chunk={n}: err {errs[n]:.3g}, None: {err_none:.3g}")
        assert errs[n] <= 4 * err_none, (n, errs[n], err_none)
    for bad in (0, -1, 2.0, True, "8"):
        with pytest.raises(ValueError):
            runner_cls(model, num_blocks=4, max_seq=64, prefill_chunk=bad)


def test_gpt_runner_chunked_prefill(monkeypatch):
    """Measured (fp32, max over the four prompts of max |logits - ref|):
    None 2.68e-07; prefill_chunk 1: 4.47e-07, 5: 3.87e-07, 16: 2.98e-07,
    64: 2.98e-07."""
    from paddle_amd.models import build_gpt
    from paddle_amd.serving import GPTModelRunner
    paddle.seed(0)
    m = build_gpt("gpt3-tiny", max_seq_len=128).to("cpu").float().eval()
    _runner_scheduling(GPTModelRunner, m, monkeypatch)


def test_llama_runner_chunked_prefill(monkeypatch):
    """Measured (fp32): None 5.36e-07; prefill_chunk 1: 4.77e-07,
    5: 4.77e-07, 16: 2.98e-07, 64: 2.98e-07."""
    from paddle_amd.models.llama import build_llama
    from paddle_amd.serving import LlamaModelRunner
    paddle.seed(0)
    m = build_llama("llama-tiny", num_kv_heads=1,
                    max_seq_len=128).to("cpu").float().eval()
    _runner_scheduling(LlamaModelRunner, m, monkeypatch)


def test_runner_chunked_prefill_int8_cache_under_engine(monkeypatch):
    """With the int8 cache the prompt attends to stored codes; the run
    completes with the same bookkeeping."""
    from paddle_amd.models import build_gpt
    from paddle_amd.serving import GPTModelRunner
    paddle.seed(0)
    m = build_gpt("gpt3-tiny", max_seq_len=128).to("cpu").float().eval()
    reqs, first, _, runner, eng = serve_recording(
        GPTModelRunner, m, monkeypatch, use_graphs=False, prefill_chunk=16,
        kv_cache="int8")
    assert all(r.done and len(r.out_ids) == NEW_TOKENS for r in reqs)
    assert first == budget_rule([len(p) for p in PROMPTS], 16)
    assert len(eng.alloc.free) == 64
    assert bool(runner.k[0].any()) and bool((runner.k_scale[0] > 0).any())
