"""Split-KV paged decode attention on the GPU: the split decode_attn_kernel +
decode_attn_merge_kernel behind C.decode_attention_split, the
paged_decode_attention(num_splits=) dispatch, the binding's contract,
hipGraph capture with lengths changing on the device, and the runners.

int8 caches use the reference and cases of test_kv_int8_gpu.py.  For bf16
caches ref_attn_bf16 below is the same formula, softmax(scale q k^T) v in
fp64 from the stored bf16 values, with the same bound

    |out - ref| <= 2^-7 |ref| + 4 E + 2^-22 A

(E: max over the output row of |fp32 torch evaluation - fp64|, A: sum_pos
p |v|), compared with <=.  A bf16 case is the dequantised image of an int8
case, so it keeps the paged layout, the poisoned last block and the poisoned
unused table entries of make_case.  test_decode_attn_split_cpu.py shows on a
CPU emulation that this bound accepts slice rule + partials + merge for every
split count used here and rejects the mistakes such kernels can make.

Slice rule under test (docs/KERNELS.md): S = min(len, max_blocks * bs),
c = 64 * ceil(S / (64 n)), split s covers [s c, min(S, (s + 1) c)).
"""
import functools
import math

import pytest
import torch

from test_kv_int8_gpu import (BF16, DEV, F32, F64, U_BF16, check, gpu_case,
                              make_case, ref_attn, to_dev, violations)

SPLITS = [1, 2, 3, 4, 8]
EDGE_LENS = [0, 1, 63, 64, 65, 127, 128, 129, 250, 513]
# G = 4 (a full tile), 8 (two int8 tiles), 1 (MHA), 3 (a ragged tile)
SHAPES = [(128, 8, 2, 16), (64, 8, 1, 24), (128, 4, 4, 16), (128, 6, 2, 16)]
KINDS = ["int8_token", "int8_head", "bf16"]


# ---------------------------------------------------------------------------
# reference for bf16 caches
# ---------------------------------------------------------------------------
def _attn_bf16_one(q, kc, vc, table, lens, scale, dt):
    B, H, D = q.shape
    bs, HKV = kc.shape[1], kc.shape[2]
    rep = H // HKV
    out = torch.zeros(B, H, D, dtype=dt)
    A = torch.zeros(B, H, D, dtype=dt)
    for b in range(B):
        S = int(lens[b])
        if S == 0:
            continue
        blocks = table[b, :(S + bs - 1) // bs].long()
        kh = kc[blocks].reshape(-1, HKV, D)[:S].to(dt).repeat_interleave(rep, 1)
        vh = vc[blocks].reshape(-1, HKV, D)[:S].to(dt).repeat_interleave(rep, 1)
        s = torch.einsum("hd,shd->hs", q[b].to(dt), kh) * scale
        p = torch.softmax(s, dim=-1)
        out[b] = torch.einsum("hs,shd->hd", p, vh)
        A[b] = torch.einsum("hs,shd->hd", p, vh.abs())
    return out, A


def ref_attn_bf16(q, kc, vc, table, lens, scale=None):
    """(ref fp64 [B, H, D], bound fp64 [B, H, D]) on CPU copies."""
    q, kc, vc, table, lens = (t.cpu() for t in (q, kc, vc, table, lens))
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    ref, A = _attn_bf16_one(q, kc, vc, table, lens, scale, F64)
    r32, _ = _attn_bf16_one(q, kc, vc, table, lens, scale, F32)
    E = (r32.to(F64) - ref).abs().amax(-1, keepdim=True)
    return ref, U_BF16 * ref.abs() + 4 * E + 2.0 ** -22 * A


def bf16_image(c):
    """The bf16 cache holding the dequantised values of an int8 case (the
    poison block stays large and finite: 127 * 3e4)."""
    def deq(codes, sc):
        s = sc.unsqueeze(-1) if sc.dim() == 3 else sc.reshape(1, 1, -1, 1)
        return (codes.to(F32) * s).to(BF16)
    d = dict(c)
    d["kc"], d["vc"] = deq(c["kc"], c["ks"]), deq(c["vc"], c["vs"])
    d["ks"] = d["vs"] = None
    return d


def case_of_kind(kind, D, H, HKV, bs, lens, seed, rows=None):
    c = make_case(D, H, HKV, bs, lens, seed, static=(kind == "int8_head"),
                  rows=rows)
    return bf16_image(c) if kind == "bf16" else c


def ref_of(c, scale=None):
    if c["ks"] is None:
        return ref_attn_bf16(c["q"], c["kc"], c["vc"], c["table"], c["lens"],
                             scale)
    return ref_attn(c["q"], c["kc"], c["vc"], c["ks"], c["vs"], c["table"],
                    c["lens"], scale)


@functools.lru_cache(maxsize=None)
def edge_case(kind, D, H, HKV, bs):
    """(device tensors, ref, bound): computed once, shared, never modified.
    A case must be answerable: the bound has no absolute term, so where one
    position takes all the weight and its V element is exactly 0, the
    reference is the ~1e-44 contribution of the others, below bf16's
    smallest subnormal (2^-133), and no bf16 output lies within the bound.
    Seed base 2000 draws one such element (bf16, D128 H6 HKV2); the assert
    keeps any later change of the cases from drawing another."""
    c = case_of_kind(kind, D, H, HKV, bs, EDGE_LENS, 2001 + D + 8 * HKV + bs)
    ref, bound = ref_of(c)
    assert violations(ref.to(BF16), ref, bound) == 0, \
        "the correctly rounded reference must lie within the bound"
    return to_dev(c, DEV), ref, bound


def needle_head_case(kind, D, H, HKV, bs, S, n, j, seed):
    """One sequence where K at position n is 8 q of q-head j of every kv
    head's group, so for those heads position n takes nearly all the weight;
    V there is a distinct row."""
    g = torch.Generator().manual_seed(seed)
    k, v = (torch.randn(S, HKV, D, generator=g).to(BF16) for _ in range(2))
    q = torch.randn(1, H, D, generator=g).to(BF16)
    rep = H // HKV
    k[n] = (8.0 * q[0, j::rep].float()).to(BF16)
    v[n] = (3.0 + torch.arange(D).float() / D).to(BF16).expand(HKV, D)
    c = make_case(D, H, HKV, bs, [S], seed, rows={0: (k, v)})
    c["q"] = q
    return bf16_image(c) if kind == "bf16" else c


def _C():
    from paddle_amd import _ext
    return _ext.get_ext(required=True)


def run_split(C, c, n, scale=None):
    if scale is None:
        scale = 1.0 / math.sqrt(c["q"].shape[-1])
    return C.decode_attention_split(c["q"], c["kc"], c["vc"], c["table"],
                                    c["lens"], scale, n, c["ks"], c["vs"])


def run_unsplit(C, c, scale=None):
    """The unsplit binding of the case's cache kind."""
    if scale is None:
        scale = 1.0 / math.sqrt(c["q"].shape[-1])
    if c["ks"] is None:
        return C.decode_attention(c["q"], c["kc"], c["vc"], c["table"],
                                  c["lens"], scale)
    return C.decode_attention_int8(c["q"], c["kc"], c["vc"], c["ks"], c["vs"],
                                   c["table"], c["lens"], scale)


# ---------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D,H,HKV,bs", SHAPES)
def test_decode_attention_split_slice_edges_gpu(D, H, HKV, bs, kind):
    """Every split count lies within the bound of the one reference: lengths
    around the 64-position granule, S = 0, S = 1 with seven empty splits."""
    c, ref, bound = edge_case(kind, D, H, HKV, bs)
    C = _C()
    for n in SPLITS:
        out = run_split(C, c, n)
        assert out.dtype == BF16 and tuple(out.shape) == (len(EDGE_LENS), H, D)
        assert bool((out[0] == 0).all()), f"S = 0 must give zeros (n={n})"
        check(f"{kind} D{D} H{H} HKV{HKV} bs{bs} n{n}", out, ref, bound)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["int8_token", "bf16"])
def test_decode_attention_split_needle_gpu(kind):
    """S = 513 in 4 splits (c = 192): the needle sits at the last position
    of split 0, the first of split 1, in a slice of one position, and at 0,
    for each q-head of the group in turn."""
    D, H, HKV, bs, S = 128, 8, 2, 16, 513
    C = _C()
    for n in (191, 192, 512, 0):
        for j in range(H // HKV):
            c = needle_head_case(kind, D, H, HKV, bs, S, n, j, 500 + 7 * n + j)
            ref, bound = ref_of(c)
            assert float((ref[0, j] - 3.0).abs().max()) < 1.5
            check(f"{kind} needle n={n} head {j}", run_split(C, to_dev(c, DEV), 4),
                  ref, bound)


@pytest.mark.gpu
def test_decode_attention_split_length_past_table_gpu():
    """seq_lens beyond max_blocks * bs is clamped to the table's capacity,
    by the split and by the unsplit bindings of both caches."""
    D, H, HKV, bs = 128, 8, 2, 16
    c = make_case(D, H, HKV, bs, [80, 33], 41)
    cap = c["table"].shape[1] * bs
    # make every table entry a real block so that `cap` positions are data
    c["table"][0, -1] = c["table"][1, 0]
    c["table"][1, 3:] = c["table"][0, :c["table"].shape[1] - 3]
    C = _C()
    for cc in (c, bf16_image(c)):
        want = dict(cc, lens=torch.tensor([cap, cap], dtype=torch.int32))
        ref, bound = ref_of(want)
        over = dict(cc, lens=torch.tensor([cap + 1, 2 ** 31 - 1],
                                          dtype=torch.int32))
        over = to_dev(over, DEV)
        check("clamped", run_split(C, over, 2), ref, bound)
        check("clamped, unsplit", run_unsplit(C, over), ref, bound)


@pytest.mark.gpu
def test_decode_attn_split_grid_matches_python_plan_gpu():
    from paddle_amd.ops import functional as hot
    C = _C()
    for int8 in (False, True):
        for H, HKV in ((8, 8), (8, 4), (6, 2), (8, 2), (8, 1), (32, 2), (5, 1)):
            gt, tiles, blocks = C.decode_attn_split_grid(3, H, HKV, 5, int8)
            assert (gt, tiles) == hot._decode_attn_split_tiles(H, HKV, int8)
            assert blocks == 3 * HKV * tiles * 5
            assert gt * tiles >= H // HKV and gt <= (4 if int8 else 8)


# ---------------------------------------------------------------------------
# dispatch
# ---------------------------------------------------------------------------
def _count(monkeypatch, C, name, calls):
    real = getattr(C, name)
    monkeypatch.setattr(C, name,
                        lambda *a, **k: calls.append(name) or real(*a, **k))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["int8_token", "bf16"])
def test_paged_decode_attention_split_dispatch_gpu(monkeypatch, kind):
    import paddle_amd as paddle
    from paddle_amd.ops import functional as hot
    C = _C()
    calls = []
    for name in ("decode_attention", "decode_attention_int8",
                 "decode_attention_split"):
        _count(monkeypatch, C, name, calls)
    old = "decode_attention" if kind == "bf16" else "decode_attention_int8"

    def call(c, q=None, **kw):
        return hot.paged_decode_attention(
            c["q"] if q is None else q, c["kc"], c["vc"], c["table"],
            c["lens"], k_scale=c["ks"], v_scale=c["vs"], **kw)

    # capacity < 512: today's kernel, exactly once
    small, ref_s, bound_s = gpu_case(128, 8, 2, 16)
    if kind == "bf16":
        small = bf16_image(small)
        ref_s, bound_s = ref_of(small)
    assert small["table"].shape[1] * 16 < 512
    out = call(small)
    assert calls == [old]
    check("today's kernel", out, ref_s, bound_s)
    # ... unless a split count is forced; 0 pins today's kernel
    check("forced n=2", call(small, num_splits=2), ref_s, bound_s)
    assert calls == [old, "decode_attention_split"]
    assert torch.equal(call(small, num_splits=0), out)
    assert calls == [old, "decode_attention_split", old]

    # B = 1, H = 8, HKV = 2, capacity 1024: the heuristic splits
    del calls[:]
    cl = case_of_kind(kind, 128, 8, 2, 16, [1000], 77)
    assert cl["table"].shape[1] * 16 == 1024
    assert hot._decode_attn_split_plan(1, 8, 2, 128, 1024, kind != "bf16") > 1
    ref, bound = ref_of(cl)
    big = to_dev(cl, DEV)
    check("heuristic", call(big), ref, bound)
    assert calls == ["decode_attention_split"]
    # native flag off: torch path
    paddle.set_flags({"FLAGS_use_native_kernels": False})
    try:
        off = call(big, num_splits=4)
    finally:
        paddle.set_flags({"FLAGS_use_native_kernels": True})
    assert calls == ["decode_attention_split"]
    check("torch path", off, ref, bound)
    # fp32 q is outside the contract: torch path, num_splits ignored
    f32 = call(big, q=big["q"].float(), num_splits=4)
    assert calls == ["decode_attention_split"] and f32.dtype == F32
    with pytest.raises(ValueError):
        call(big, num_splits=65)
    with pytest.raises(ValueError):
        call(big, num_splits=-1)


# ---------------------------------------------------------------------------
# contract: every check raises before any launch
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_decode_attention_split_contract_gpu():
    C = _C()
    c, _, _ = edge_case("int8_token", 128, 8, 2, 16)
    cb, _, _ = edge_case("bf16", 128, 8, 2, 16)
    q, kc, vc, ks, vs, tb, ln = (c[n] for n in
                                 ("q", "kc", "vc", "ks", "vs", "table", "lens"))
    kb, vb = cb["kc"], cb["vc"]
    HKV, D = kc.shape[2], kc.shape[3]
    sc = 1.0 / math.sqrt(D)
    hks = torch.ones(HKV, device=DEV)
    f = C.decode_attention_split
    mis = torch.zeros(q.numel() + 4, dtype=BF16, device=DEV)[4:].view_as(q)
    q96 = torch.zeros(q.shape[0], q.shape[1], 96, dtype=BF16, device=DEV)
    k96 = torch.zeros(kb.shape[0], kb.shape[1], HKV, 96, dtype=BF16, device=DEV)
    bad = {
        "q fp32": lambda: f(q.float(), kb, vb, tb, ln, sc, 2),
        "q fp32 int8": lambda: f(q.float(), kc, vc, tb, ln, sc, 2, ks, vs),
        "q on cpu": lambda: f(q.cpu(), kb, vb, tb, ln, sc, 2),
        "cache on cpu": lambda: f(q, kb.cpu(), vb, tb, ln, sc, 2),
        "lens on cpu": lambda: f(q, kb, vb, tb, ln.cpu(), sc, 2),
        "q strided": lambda: f(q.transpose(0, 1).contiguous().transpose(0, 1),
                               kb, vb, tb, ln, sc, 2),
        "q misaligned": lambda: f(mis, kb, vb, tb, ln, sc, 2),
        "q misaligned int8": lambda: f(mis, kc, vc, tb, ln, sc, 2, ks, vs),
        "q 2-D": lambda: f(q[0], kb, vb, tb, ln, sc, 2),
        "num_splits 0": lambda: f(q, kb, vb, tb, ln, sc, 0),
        "num_splits 65": lambda: f(q, kb, vb, tb, ln, sc, 65),
        "num_splits 0 int8": lambda: f(q, kc, vc, tb, ln, sc, 0, ks, vs),
        "num_splits 65 int8": lambda: f(q, kc, vc, tb, ln, sc, 65, ks, vs),
        "one scale": lambda: f(q, kc, vc, tb, ln, sc, 2, ks),
        "scale kinds differ": lambda: f(q, kc, vc, tb, ln, sc, 2, ks, hks),
        "scale fp64": lambda: f(q, kc, vc, tb, ln, sc, 2, ks.double(), vs.double()),
        "int8 cache without scales": lambda: f(q, kc, vc, tb, ln, sc, 2),
        "bf16 cache with scales": lambda: f(q, kb, vb, tb, ln, sc, 2, ks, vs),
        "cache fp32": lambda: f(q, kb.float(), vb.float(), tb, ln, sc, 2),
        "cache strided": lambda: f(
            q, kb.transpose(1, 2).contiguous().transpose(1, 2), vb, tb, ln, sc, 2),
        "cache shapes differ": lambda: f(q, kb, vb[:-1], tb, ln, sc, 2),
        "D 96": lambda: f(q96, k96, k96.clone(), tb, ln, sc, 2),
        "cache D != q D": lambda: f(q[..., :64].contiguous(), kb, vb, tb, ln, sc, 2),
        "H % HKV": lambda: f(q[:, :7].contiguous(), kb, vb, tb, ln, sc, 2),
        "table int64": lambda: f(q, kb, vb, tb.long(), ln, sc, 2),
        "table rows": lambda: f(q, kb, vb, tb[:-1], ln, sc, 2),
        "table strided": lambda: f(q, kb, vb, tb[:, ::2], ln, sc, 2),
        "lens int64": lambda: f(q, kb, vb, tb, ln.long(), sc, 2),
        "lens length": lambda: f(q, kb, vb, tb, ln[:-1], sc, 2),
    }
    for name, fn in bad.items():
        with pytest.raises(RuntimeError):
            fn()
            pytest.fail(f"{name}: no error")
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# hipGraph: captured once, seq_lens changed on the device between replays
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["int8_token", "bf16"])
def test_paged_decode_attention_split_graph_gpu(kind):
    from paddle_amd.ops import functional as hot
    D, H, HKV, bs = 128, 8, 2, 16
    c = to_dev(case_of_kind(kind, D, H, HKV, bs, [513, 513], 91), DEV)
    lens = torch.tensor([65, 64], dtype=torch.int32, device=DEV)

    def step(ln):
        return hot.paged_decode_attention(c["q"], c["kc"], c["vc"], c["table"],
                                          ln, k_scale=c["ks"], v_scale=c["vs"],
                                          num_splits=4)

    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        step(lens)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_g = step(lens)
    seen = []
    for a, b in ((65, 513), (250, 1), (0, 0), (513, 129)):
        lens.copy_(torch.tensor([a, b], dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        eager = step(lens.clone())
        assert torch.equal(out_g, eager), (a, b)
        seen.append(out_g.clone())
    assert bool((seen[2] == 0).all())
    assert not torch.equal(seen[0], seen[3])
    ref, bound = ref_of(dict(c, lens=lens))
    check("last replay", out_g, ref, bound)


# ---------------------------------------------------------------------------
# runners: max_seq = 1024 so that the heuristic splits
# ---------------------------------------------------------------------------
PROMPTS = [[3, 7, 11, 2], [5, 9, 4, 8, 15, 16, 23], list(range(20, 53)),
           [3, 7, 11, 2]]


def _serve(runner_cls, model, use_graphs, kv_cache, monkeypatch, **kw):
    from paddle_amd.serving import Engine, Request
    C = _C()
    calls, outs = [], []
    real_split = C.decode_attention_split

    def split(*a, **k):
        calls.append("decode_attention_split")
        out = real_split(*a, **k)
        if not torch.cuda.is_current_stream_capturing():
            outs.append(out)
        return out

    with monkeypatch.context() as mp:
        for name in ("decode_attention", "decode_attention_int8"):
            _count(mp, C, name, calls)
        mp.setattr(C, "decode_attention_split", split)
        runner = runner_cls(model, num_blocks=64, block_size=16, max_seq=1024,
                            use_graphs=use_graphs, kv_cache=kv_cache, **kw)
        assert runner.use_graphs == use_graphs
        eng = Engine(runner, num_blocks=64, block_size=16, max_batch=4)
        reqs = [Request(prompt_ids=p, max_new_tokens=8) for p in PROMPTS]
        for r in reqs:
            eng.add_request(r)
        eng.run_until_done()
    assert all(r.done and len(r.out_ids) == 8 for r in reqs)
    assert all(bool(torch.isfinite(o.float()).all()) for o in outs)
    vocab = model.cfg.vocab_size
    assert all(0 <= t < vocab for r in reqs for t in r.out_ids)
    return [r.out_ids for r in reqs], calls


def _runner_checks(runner_cls, model, monkeypatch):
    for kv in ("bf16", "int8"):
        a, ca = _serve(runner_cls, model, True, kv, monkeypatch)
        b, cb = _serve(runner_cls, model, False, kv, monkeypatch)
        assert ca and set(ca) == {"decode_attention_split"}
        assert cb and set(cb) == {"decode_attention_split"}
        assert a == b
    old = "decode_attention"
    _, c0 = _serve(runner_cls, model, False, "bf16", monkeypatch,
                   decode_splits=0)
    assert c0 and set(c0) == {old}
    with pytest.raises(ValueError):
        runner_cls(model, num_blocks=4, max_seq=64, decode_splits=65)


@pytest.mark.gpu
def test_gpt_runner_decode_splits_gpu(monkeypatch):
    import paddle_amd as paddle
    from paddle_amd.models import build_gpt
    from paddle_amd.serving import GPTModelRunner
    paddle.seed(0)
    m = build_gpt("gpt3-tiny", num_heads=2, max_seq_len=128).to("cuda", BF16)
    _runner_checks(GPTModelRunner, m, monkeypatch)


@pytest.mark.gpu
def test_llama_runner_decode_splits_gpu(monkeypatch):
    import paddle_amd as paddle
    from paddle_amd.models.llama import build_llama
    from paddle_amd.serving import LlamaModelRunner
    paddle.seed(0)
    m = build_llama("llama-tiny", num_heads=2, num_kv_heads=1,
                    max_seq_len=128).to("cuda", BF16).eval()
    _runner_checks(LlamaModelRunner, m, monkeypatch)


@pytest.mark.gpu
def test_generate_decode_splits_gpu(monkeypatch):
    """generate_gpt / generate_llama pass decode_splits through."""
    import paddle_amd as paddle
    from paddle_amd.models import build_gpt
    from paddle_amd.models.generation import generate_gpt, generate_llama
    from paddle_amd.models.llama import build_llama
    paddle.seed(0)
    C = _C()
    calls = []
    _count(monkeypatch, C, "decode_attention_split", calls)
    ids = torch.randint(0, 100, (2, 9), device=DEV)
    m = build_gpt("gpt3-tiny", num_heads=2, max_seq_len=128).to("cuda", BF16)
    out = generate_gpt(m, ids, max_new_tokens=3, decode_splits=2)
    assert tuple(out.shape) == (2, 3) and len(calls) > 0
    n = len(calls)
    generate_gpt(m, ids, max_new_tokens=3)           # capacity < 512
    assert len(calls) == n
    lm = build_llama("llama-tiny", num_heads=2, num_kv_heads=1,
                     max_seq_len=128).to("cuda", BF16).eval()
    out = generate_llama(lm, ids, max_new_tokens=3, decode_splits=2,
                         kv_cache="int8")
    assert tuple(out.shape) == (2, 3) and len(calls) > n
