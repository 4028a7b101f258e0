"""Paged prefill attention on the GPU: paged_prefill_kernel behind
C.paged_prefill_attention, the paged_prefill_attention dispatch, the
binding's contract, hipGraph capture with cu_q / seq_lens / table changing on
the device, and chunked prefill in the runners.

Reference, bound and cases are those of test_prefill_attn_cpu.py, which
shows on a CPU emulation that the bound

    |out - ref| <= 2^-7 |ref| + 2^-7 A + 4 E        (compared with <=)

accepts the kernel's design and rejects the mistakes such a kernel can make.
"""
import functools
import math

import pytest
import torch

from test_decode_attn_split_gpu import (EDGE_LENS, SHAPES, bf16_image,
                                        case_of_kind, edge_case)
from test_kv_int8_gpu import BF16, DEV, F32, check, to_dev
from test_prefill_attn_cpu import (KINDS, pairs_case, prefill_case,
                                   ref_prefill, worst, zero_rows)


def _C():
    from paddle_amd import _ext
    return _ext.get_ext(required=True)


def run(C, c, max_q, scale=None):
    if scale is None:
        scale = 1.0 / math.sqrt(c["q"].shape[-1])
    return C.paged_prefill_attention(c["q"], c["kc"], c["vc"], c["table"],
                                     c["lens"], c["cu_q"], max_q, scale,
                                     c["ks"], c["vs"])


@functools.lru_cache(maxsize=None)
def gpu_pairs_case(kind, D, H, HKV, bs):
    """(device tensors, ref, bound, zero rows): computed once, shared, never
    modified."""
    c = pairs_case(kind, D, H, HKV, bs)
    return (to_dev(c, DEV),) + ref_prefill(c) + (zero_rows(c),)


# ---------------------------------------------------------------------------
# kernel
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D,H,HKV,bs", SHAPES)
def test_paged_prefill_edges_gpu(D, H, HKV, bs, kind):
    """Measured err / bound (worst element): docs/KERNELS.md "paged prefill
    attention"."""
    c, ref, bound, zero = gpu_pairs_case(kind, D, H, HKV, bs)
    C = _C()
    out = run(C, c, 65)
    assert out.dtype == BF16 and out.shape == c["q"].shape
    print(f"{kind} D{D} H{H} HKV{HKV} bs{bs}: err/bound {worst(out, ref, bound):.3f}")
    check(f"{kind} D{D} H{H} HKV{HKV} bs{bs}", out, ref, bound)
    assert bool((out[zero.to(DEV)] == 0).all())
    assert torch.equal(run(C, c, 200), out), "max_q must not change a bit"


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["int8_token", "bf16"])
def test_paged_prefill_zero_rows_gpu(kind):
    """A token in front of position 0 (more new tokens than cached
    positions, S = 0 included) sees nothing and is exactly zero; its
    neighbours are within the bound."""
    D, H, HKV, bs = 128, 8, 2, 16
    c = prefill_case(kind, D, H, HKV, bs, [(5, 3), (3, 0), (20, 17), (2, 30)], 51)
    ref, bound = ref_prefill(c)
    zero = zero_rows(c)
    assert zero.tolist() == [True] * 2 + [False] * 3 + [True] * 3 + \
        [True] * 3 + [False] * 17 + [False] * 2
    out = run(_C(), to_dev(c, DEV), 20)
    check(f"{kind} zero rows", out, ref, bound)
    assert bool((out[zero.to(DEV)] == 0).all())


def needle_case(kind, D, H, HKV, bs, ql, S, i, g, seed):
    """One sequence where K at token i's own last visible position is 8 q of
    (token i, q-head g of every kv head's group), so for those rows that
    position takes nearly all the weight; V there is a distinct row."""
    gen = torch.Generator().manual_seed(seed)
    k, v = (torch.randn(S, HKV, D, generator=gen).to(BF16) for _ in range(2))
    q = torch.randn(ql, H, D, generator=gen).to(BF16)
    rep = H // HKV
    n = S - ql + i
    k[n] = (8.0 * q[i, g::rep].float()).to(BF16)
    v[n] = (3.0 + torch.arange(D).float() / D).to(BF16).expand(HKV, D)
    c = prefill_case(kind, D, H, HKV, bs, [(ql, S)], seed, rows={0: (k, v)})
    c["q"] = q
    return c


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["int8_token", "bf16"])
@pytest.mark.parametrize("ql,S", [(33, 250), (65, 129)])
def test_paged_prefill_needle_gpu(kind, ql, S):
    """The first and last row of a wave tile (16 rows) and of a block (64
    rows), and the last rows of the sequence."""
    D, H, HKV, bs = 128, 8, 2, 16
    G = H // HKV
    rows = ql * G
    C = _C()
    for r in sorted({0, 15, 16, 63, 64, (rows - 1) // 64 * 64 - 1,
                     (rows - 1) // 64 * 64, rows - 1}):
        i, g = divmod(r, G)
        c = needle_case(kind, D, H, HKV, bs, ql, S, i, g, 700 + 3 * r + ql)
        ref, bound = ref_prefill(c)
        assert float((ref[i, g] - 3.0).abs().max()) < 1.5
        check(f"{kind} needle row {r}", run(C, to_dev(c, DEV), ql), ref, bound)


@pytest.mark.gpu
def test_paged_prefill_length_past_table_gpu():
    """seq_lens beyond max_blocks * bs is clamped to the table's capacity."""
    D, H, HKV, bs = 128, 8, 2, 16
    c = prefill_case("int8_token", D, H, HKV, bs, [(9, 80), (3, 33)], 41)
    cap = c["table"].shape[1] * bs
    # make every table entry a real block so that `cap` positions are data
    c["table"][0, -1] = c["table"][1, 0]
    c["table"][1, 3:] = c["table"][0, :c["table"].shape[1] - 3]
    C = _C()
    for cc in (c, bf16_image(c)):
        cc = dict(cc, q=c["q"], cu_q=c["cu_q"])
        want = dict(cc, lens=torch.tensor([cap, cap], dtype=torch.int32))
        ref, bound = ref_prefill(want)
        over = dict(cc, lens=torch.tensor([cap + 1, 2 ** 31 - 1],
                                          dtype=torch.int32))
        check("clamped", run(C, to_dev(over, DEV), 9), ref, bound)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D,H,HKV,bs", SHAPES)
def test_paged_prefill_q_len_1_gpu(D, H, HKV, bs, kind):
    """q_len = 1 everywhere is decode attention: the decode reference of the
    split-KV edge cases with this file's A term."""
    c, ref, _ = edge_case(kind, D, H, HKV, bs)
    B = len(EDGE_LENS)
    cp = dict(c, cu_q=torch.arange(B + 1, dtype=torch.int32, device=DEV))
    ref_p, bound_p = ref_prefill({k: (v.cpu() if isinstance(v, torch.Tensor)
                                      else v) for k, v in cp.items()})
    assert torch.equal(ref_p, ref)
    out = run(_C(), cp, 1)
    check(f"{kind} D{D} H{H} HKV{HKV} bs{bs}", out, ref_p, bound_p)
    assert bool((out[0] == 0).all()), "S = 0 must give zeros"


# ---------------------------------------------------------------------------
# dispatch
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["int8_token", "bf16"])
def test_paged_prefill_attention_dispatch_gpu(monkeypatch, kind):
    import paddle_amd as paddle
    from paddle_amd.ops import functional as hot
    C = _C()
    c, ref, bound, _ = gpu_pairs_case(kind, 128, 8, 2, 16)
    calls = []
    real = C.paged_prefill_attention
    monkeypatch.setattr(C, "paged_prefill_attention",
                        lambda *a, **k: calls.append(1) or real(*a, **k))

    def call(c, q=None):
        return hot.paged_prefill_attention(
            c["q"] if q is None else q, c["kc"], c["vc"], c["table"],
            c["lens"], c["cu_q"], 65, k_scale=c["ks"], v_scale=c["vs"])

    on = call(c)
    assert calls == [1]
    check("native", on, ref, bound)
    # int64 index tensors are cast at the site
    assert torch.equal(call(dict(c, table=c["table"].long(),
                                 lens=c["lens"].long(),
                                 cu_q=c["cu_q"].long())), on)
    assert calls == [1, 1]
    paddle.set_flags({"FLAGS_use_native_kernels": False})
    try:
        off = call(c)
    finally:
        paddle.set_flags({"FLAGS_use_native_kernels": True})
    assert calls == [1, 1]
    check("torch path", off, ref, bound)
    # fp32 q and non-contiguous caches are outside the contract: torch path
    f32 = call(c, q=c["q"].float())
    assert calls == [1, 1] and f32.dtype == F32
    check("fp32 q", f32, ref, bound)
    if kind == "bf16":
        nc = dict(c, kc=c["kc"].transpose(1, 2).contiguous().transpose(1, 2),
                  vc=c["vc"].transpose(1, 2).contiguous().transpose(1, 2))
        assert not nc["kc"].is_contiguous()
        check("strided caches", call(nc), ref, bound)
        assert calls == [1, 1]
    with pytest.raises(ValueError):
        hot.paged_prefill_attention(c["q"], c["kc"], c["vc"], c["table"],
                                    c["lens"], c["cu_q"], 65,
                                    k_scale=torch.ones(2, device=DEV))


# ---------------------------------------------------------------------------
# contract: every check raises before any launch
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_paged_prefill_contract_gpu():
    C = _C()
    c, _, _, _ = gpu_pairs_case("int8_token", 128, 8, 2, 16)
    cb, _, _, _ = gpu_pairs_case("bf16", 128, 8, 2, 16)
    q, kc, vc, ks, vs, tb, ln, cu = (c[n] for n in ("q", "kc", "vc", "ks", "vs",
                                                    "table", "lens", "cu_q"))
    kb, vb = cb["kc"], cb["vc"]
    HKV, D = kc.shape[2], kc.shape[3]
    sc = 1.0 / math.sqrt(D)
    hks = torch.ones(HKV, device=DEV)
    f = C.paged_prefill_attention
    mis = torch.zeros(q.numel() + 4, dtype=BF16, device=DEV)[4:].view_as(q)
    q96 = torch.zeros(q.shape[0], q.shape[1], 96, dtype=BF16, device=DEV)
    k96 = torch.zeros(kb.shape[0], kb.shape[1], HKV, 96, dtype=BF16, device=DEV)
    bad = {
        "q fp32": lambda: f(q.float(), kb, vb, tb, ln, cu, 65, sc),
        "q fp32 int8": lambda: f(q.float(), kc, vc, tb, ln, cu, 65, sc, ks, vs),
        "q on cpu": lambda: f(q.cpu(), kb, vb, tb, ln, cu, 65, sc),
        "cache on cpu": lambda: f(q, kb.cpu(), vb, tb, ln, cu, 65, sc),
        "lens on cpu": lambda: f(q, kb, vb, tb, ln.cpu(), cu, 65, sc),
        "cu_q on cpu": lambda: f(q, kb, vb, tb, ln, cu.cpu(), 65, sc),
        "q strided": lambda: f(q.transpose(0, 1).contiguous().transpose(0, 1),
                               kb, vb, tb, ln, cu, 65, sc),
        "q misaligned": lambda: f(mis, kb, vb, tb, ln, cu, 65, sc),
        "q 2-D": lambda: f(q[0], kb, vb, tb, ln, cu, 65, sc),
        "max_q 0": lambda: f(q, kb, vb, tb, ln, cu, 0, sc),
        "max_q -1": lambda: f(q, kc, vc, tb, ln, cu, -1, sc, ks, vs),
        "max_q * G >= 2^31": lambda: f(q, kb, vb, tb, ln, cu, 2 ** 29, sc),
        "one scale": lambda: f(q, kc, vc, tb, ln, cu, 65, sc, ks),
        "scale kinds differ": lambda: f(q, kc, vc, tb, ln, cu, 65, sc, ks, hks),
        "scale fp64": lambda: f(q, kc, vc, tb, ln, cu, 65, sc, ks.double(),
                                vs.double()),
        "int8 cache without scales": lambda: f(q, kc, vc, tb, ln, cu, 65, sc),
        "bf16 cache with scales": lambda: f(q, kb, vb, tb, ln, cu, 65, sc, ks, vs),
        "cache fp32": lambda: f(q, kb.float(), vb.float(), tb, ln, cu, 65, sc),
        "cache strided": lambda: f(
            q, kb.transpose(1, 2).contiguous().transpose(1, 2), vb, tb, ln, cu,
            65, sc),
        "cache shapes differ": lambda: f(q, kb, vb[:-1], tb, ln, cu, 65, sc),
        "D 96": lambda: f(q96, k96, k96.clone(), tb, ln, cu, 65, sc),
        "cache D != q D": lambda: f(q[..., :64].contiguous(), kb, vb, tb, ln,
                                    cu, 65, sc),
        "H % HKV": lambda: f(q[:, :7].contiguous(), kb, vb, tb, ln, cu, 65, sc),
        "table int64": lambda: f(q, kb, vb, tb.long(), ln, cu, 65, sc),
        "table 1-D": lambda: f(q, kb, vb, tb[0], ln, cu, 65, sc),
        "table strided": lambda: f(q, kb, vb, tb[:, ::2], ln, cu, 65, sc),
        "lens int64": lambda: f(q, kb, vb, tb, ln.long(), cu, 65, sc),
        "lens length": lambda: f(q, kb, vb, tb, ln[:-1], cu, 65, sc),
        "cu_q int64": lambda: f(q, kb, vb, tb, ln, cu.long(), 65, sc),
        "cu_q length": lambda: f(q, kb, vb, tb, ln, cu[:-1], 65, sc),
        "cu_q strided": lambda: f(q, kb, vb, tb, ln,
                                  torch.stack([cu, cu], 1)[:, 0], 65, sc),
        "tokens without a sequence": lambda: f(q, kb, vb, tb[:0], ln[:0],
                                               cu[:1], 65, sc),
    }
    for name, fn in bad.items():
        with pytest.raises(RuntimeError):
            fn()
            pytest.fail(f"{name}: no error")
    torch.cuda.synchronize()
    # T = 0: an empty tensor, no launch
    out = f(q[:0], kb, vb, tb, ln, cu, 65, sc)
    assert tuple(out.shape) == (0, q.shape[1], D) and out.dtype == BF16


# ---------------------------------------------------------------------------
# hipGraph: captured once with a fixed max_q; cu_q, seq_lens and the table
# change on the device between replays
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["int8_token", "bf16"])
def test_paged_prefill_attention_graph_gpu(kind):
    from paddle_amd.ops import functional as hot
    D, H, HKV, bs = 128, 8, 2, 16
    MAXQ, T = 40, 64
    c = case_of_kind(kind, D, H, HKV, bs, [250, 130, 70], 93)
    g = torch.Generator().manual_seed(94)
    c["q"] = torch.randn(T, H, D, generator=g).to(BF16)
    c["cu_q"] = torch.tensor([0, 40, 41, 64], dtype=torch.int32)
    c = to_dev(c, DEV)
    st = {k: c[k].clone() for k in ("cu_q", "lens", "table")}

    def step(s):
        return hot.paged_prefill_attention(c["q"], c["kc"], c["vc"], s["table"],
                                           s["lens"], s["cu_q"], MAXQ,
                                           k_scale=c["ks"], v_scale=c["vs"])

    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        step(st)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_g = step(st)
    seen = []
    # (q_lens, seq_lens, swap the first two table entries of sequence 0)
    # (swapping two blocks that every token sees in full would permute the
    # sum, not change it: sequence 0 of the last two replays is 24 tokens
    # over 24 positions, so the swap changes what each token sees)
    for qls, lens, swap in (((40, 1, 23), (250, 130, 70), False),
                            ((1, 40, 23), (64, 65, 23), False),
                            ((24, 0, 40), (24, 100, 41), False),
                            ((24, 0, 40), (24, 100, 41), True)):
        cu = torch.tensor([0, qls[0], qls[0] + qls[1], sum(qls)],
                          dtype=torch.int32)
        assert cu[-1] == T
        table = c["table"].clone()
        if swap:
            table[0, :2] = table[0, :2].flip(0)
        st["cu_q"].copy_(cu)
        st["lens"].copy_(torch.tensor(lens, dtype=torch.int32))
        st["table"].copy_(table)
        graph.replay()
        torch.cuda.synchronize()
        now = {k: v.clone() for k, v in st.items()}
        eager = step(now)
        assert torch.equal(out_g, eager), (qls, lens, swap)
        ref, bound = ref_prefill({k: (v.cpu() if isinstance(v, torch.Tensor)
                                      else v) for k, v in dict(c, **now).items()})
        check(f"replay {qls} {lens} {swap}", out_g, ref, bound)
        seen.append(out_g.clone())
    assert not torch.equal(seen[0], seen[1])
    assert not torch.equal(seen[2], seen[3])    # the table is read per replay


# ---------------------------------------------------------------------------
# runners: chunked prefill (D = 64 variants of the tiny presets so the
# kernels run)
# ---------------------------------------------------------------------------
def _gpt():
    import paddle_amd as paddle
    from paddle_amd.models import build_gpt
    from paddle_amd.serving import GPTModelRunner
    paddle.seed(0)
    return GPTModelRunner, build_gpt("gpt3-tiny", num_heads=2,
                                     max_seq_len=128).to("cuda", BF16)


def _llama():
    import paddle_amd as paddle
    from paddle_amd.models.llama import build_llama
    from paddle_amd.serving import LlamaModelRunner
    paddle.seed(0)
    return LlamaModelRunner, build_llama(
        "llama-tiny", num_heads=2, num_kv_heads=1,
        max_seq_len=128).to("cuda", BF16).eval()


@pytest.mark.gpu
@pytest.mark.parametrize("kv", ["bf16", "int8"])
@pytest.mark.parametrize("build", [_gpt, _llama])
def test_runner_chunked_prefill_gpu(monkeypatch, build, kv):
    """Measured err(chunked) / err(None) of the first-token logits against
    the fp32 CPU forward (bf16 cache): docs/KERNELS.md "paged prefill
    attention"."""
    import copy
    from paddle_amd.ops import functional as hot
    from test_prefill_attn_cpu import (PROMPTS, budget_rule, logit_err,
                                       prompt_refs, serve_recording)
    runner_cls, model = build()
    refs = prompt_refs(copy.deepcopy(model).to("cpu", F32).eval())
    C = _C()
    calls = []
    real_pf, real_fa = C.paged_prefill_attention, hot.flash_attention
    monkeypatch.setattr(C, "paged_prefill_attention",
                        lambda *a, **k: calls.append("prefill") or real_pf(*a, **k))
    monkeypatch.setattr(hot, "flash_attention",
                        lambda *a, **k: calls.append("flash") or real_fa(*a, **k))
    err = {}
    for n in (None, 5, 16, 64):
        toks = []
        for graphs in (True, False):
            del calls[:]
            reqs, first, lg, runner, eng = serve_recording(
                runner_cls, model, monkeypatch, use_graphs=graphs,
                kv_cache=kv, prefill_chunk=n)
            assert runner.use_graphs == graphs
            assert all(r.done for r in reqs) and len(eng.alloc.free) == 64
            if n is None:
                assert calls and set(calls) == {"flash"}
                assert first == [1, 1, 1, 1]
            else:
                assert calls and set(calls) == {"prefill"}
                assert first == budget_rule([len(p) for p in PROMPTS], n)
            toks.append([r.out_ids for r in reqs])
        assert toks[0] == toks[1], f"graphs on/off differ at prefill_chunk={n}"
        err[n] = logit_err(lg, refs)
    print(f"{runner_cls.__name__} {kv}: err(None) {err[None]:.4g}, ratios "
          + ", ".join(f"{n}: {err[n] / err[None]:.3f}" for n in (5, 16, 64)))
    if kv == "bf16":
        for n in (5, 16, 64):
            assert err[n] <= 4 * err[None], (n, err[n], err[None])
