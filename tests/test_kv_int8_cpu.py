"""int8 paged KV cache without a GPU: the storage format, the torch paths of
kv_cache_quant_append / paged_decode_attention, the dispatch predicates, the
generation / runner / incubate layers, and self-tests showing that the bound
used by test_kv_int8_gpu.py accepts a fp32 emulation of the kernel's design
and rejects the mistakes an int8 decode kernel can make.
"""
import math

import pytest
import torch

import paddle_amd as paddle
from paddle_amd.ops import functional as hot

from test_kv_int8_gpu import (BF16, F32, F64, I8, case_ref, make_case,
                              make_rows, needle_case, quant_violations,
                              ref_quant, violations)

CPU = "cpu"


# ---------------------------------------------------------------------------
# fp32 emulation of the unsplit int8 decode_attn_kernel<128>: 32 position slots, each an
# online softmax with the scales on the score and on p, then the slot merge
# and the bf16 cast.  `mutant` plants one mistake.
# ---------------------------------------------------------------------------
def emulate(c, mutant=None, slots=32):
    q, kc, vc, ks, vs, table, lens = (c[n] for n in
                                      ("q", "kc", "vc", "ks", "vs", "table", "lens"))
    B, H, D = q.shape
    bs, HKV = kc.shape[1], kc.shape[2]
    rep = H // HKV
    scale = torch.tensor(1.0 / math.sqrt(D), dtype=F32)
    out = torch.zeros(B, H, D, dtype=F32)
    for b in range(B):
        S = int(lens[b])
        if mutant == "drop_last":
            S -= 1
        pos = torch.arange(S)
        pb, po = table[b].long()[pos // bs], pos % bs
        hmap = torch.arange(H) // rep
        if mutant == "wrong_head":
            hmap = (hmap + 1) % HKV
        kcode = kc[pb, po][:, hmap].to(F32)              # [S, H, D]
        vcode = vc[pb, po][:, hmap].to(F32)
        if mutant == "unsigned":
            kcode = torch.where(kcode < 0, kcode + 256, kcode)
            vcode = torch.where(vcode < 0, vcode + 256, vcode)
        dk = ks[pb, po][:, hmap] if ks.dim() == 3 else ks[hmap].expand(S, H)
        dv = vs[pb, po][:, hmap] if vs.dim() == 3 else vs[hmap].expand(S, H)
        if mutant == "dk_neighbour":
            dk = dk.roll(1, 0)
        if mutant == "dv_is_dk":
            dv = dk
        qs = q[b].to(F32) * scale                         # scale folded into q
        sc = torch.einsum("hd,shd->sh", qs, kcode) * dk   # [S, H]
        m = torch.full((slots, H), -1e30, dtype=F32)
        l = torch.zeros(slots, H, dtype=F32)
        o = torch.zeros(slots, H, D, dtype=F32)
        for p0 in range(0, S, slots):
            n = min(slots, S - p0)
            s_ = sc[p0:p0 + n]
            m_new = torch.maximum(m[:n], s_)
            corr = torch.exp(m[:n] - m_new)
            p = torch.exp(s_ - m_new)
            l[:n] = l[:n] * corr + p
            o[:n] = o[:n] * corr.unsqueeze(-1) + \
                (p * dv[p0:p0 + n]).unsqueeze(-1) * vcode[p0:p0 + n]
            m[:n] = m_new
        gm = m.amax(0)
        w = torch.where(l > 0, torch.exp(m - gm), torch.zeros_like(l))
        gl = (l * w).sum(0)
        acc = (w.unsqueeze(-1) * o).sum(0)
        inv = torch.where(gl > 0, 1.0 / gl, torch.zeros_like(gl))
        out[b] = acc * inv.unsqueeze(-1)
    return out.to(BF16)


EMU_LENS = [1, 7, 33, 250, 1000]
MUTANTS = ["unsigned", "dk_neighbour", "dv_is_dk", "wrong_head"]


@pytest.fixture(scope="module")
def emu_case():
    c = make_case(128, 8, 2, 16, EMU_LENS, 11)
    return (c,) + case_ref(c)


def test_bound_accepts_design_emulation(emu_case):
    c, ref, bound = emu_case
    out = emulate(c)
    err = (out.to(F64) - ref).abs()
    assert violations(out, ref, bound) == 0, float((err / bound).max())


@pytest.mark.parametrize("mutant", MUTANTS)
def test_bound_rejects_mutants(emu_case, mutant):
    c, ref, bound = emu_case
    out = emulate(c, mutant)
    for b, S in enumerate(EMU_LENS):
        if S >= 7:
            assert violations(out[b], ref[b], bound[b]) > 0, (mutant, S)


@pytest.mark.parametrize("S", [34, 1000])
def test_needle_probes_catch_a_dropped_position(S):
    for n in (0, 1, 7, 8, 31, 32, 33, S - 2, S - 1):
        c = needle_case(128, 8, 2, 16, S, n, 300 + n)
        ref, bound = case_ref(c)
        assert violations(emulate(c), ref, bound) == 0, n
        if n == S - 1:
            assert violations(emulate(c, "drop_last"), ref, bound) > 0


# ---------------------------------------------------------------------------
# storage format: the torch path of kv_cache_quant_append defines it
# ---------------------------------------------------------------------------
def _append_inputs(T, HKV, D, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(T, 3, HKV, D, generator=g)
    qkv = (qkv * torch.randn(T, 3, HKV, 1, generator=g).exp()).to(BF16)
    qkv[0, 1, 0] = 0
    qkv[1, 2, 0, 5] = 64.0           # a clear absmax
    return qkv[:, 1], qkv[:, 2]


@pytest.mark.parametrize("T,HKV,D", [(1, 1, 64), (5, 2, 128), (67, 8, 64),
                                     (6, 2, 32)])
def test_quant_append_per_token_matches_reference(T, HKV, D):
    bs, nblocks = 16, 6
    k, v = _append_inputs(max(T, 2), HKV, D, T)
    T = k.shape[0]
    slots = torch.randperm(nblocks * bs,
                           generator=torch.Generator().manual_seed(T))[:T]
    blk, off = slots // bs, slots % bs
    kc = torch.full((nblocks, bs, HKV, D), 0x55, dtype=I8)
    vc = kc.clone()
    ks = torch.full((nblocks, bs, HKV), -1.0)
    vs = ks.clone()
    hot.kv_cache_quant_append(k, v, kc, vc, ks, vs, blk, off)
    for x, cache, sc in ((k, kc, ks), (v, vc, vs)):
        code, d = ref_quant(x)
        assert torch.equal(cache[blk, off], code)
        assert torch.equal(sc[blk, off], d)
        assert quant_violations(code, x, d) == 0
        written = torch.zeros(nblocks, bs, dtype=torch.bool)
        written[blk, off] = True
        assert bool((cache[~written] == 0x55).all() and (sc[~written] == -1).all())
    assert float(ks[blk[0], off[0], 0]) == 0.0
    assert bool((kc[blk[0], off[0], 0] == 0).all())
    assert int(vc[blk[1], off[1], 0, 5]) == 127
    assert bool(torch.isfinite(ks).all())


def test_quant_append_per_head_matches_reference():
    T, HKV, D, bs, nblocks = 9, 2, 64, 16, 2
    k, v = _append_inputs(T, HKV, D, 3)
    kq = torch.tensor([127 / 2.0, 127 / 5.0])
    vq = torch.tensor([127 / 3.0, 127 / 70.0])
    blk, off = torch.arange(T) // bs, torch.arange(T) % bs
    kc = torch.zeros(nblocks, bs, HKV, D, dtype=I8)
    vc = kc.clone()
    ks, vs = 1 / kq, 1 / vq
    ks0 = ks.clone()
    hot.kv_cache_quant_append(k, v, kc, vc, ks, vs, blk, off, kq, vq)
    assert torch.equal(ks, ks0)
    for x, cache, qs in ((k, kc, kq), (v, vc, vq)):
        code, _ = ref_quant(x, qs)
        assert torch.equal(cache[blk, off], code)
        assert quant_violations(code, x, qs=qs) == 0
    assert int(kc.abs().max()) == 127          # clamped, never -128


def test_quantiser_bound_rejects_truncation():
    k, _ = _append_inputs(8, 2, 64, 4)
    code, d = ref_quant(k)
    trunc = (k.float() / torch.where(d == 0, torch.ones_like(d), d)
             .unsqueeze(-1)).trunc().to(I8)
    assert quant_violations(trunc, k, d) > 0


# ---------------------------------------------------------------------------
# torch path of paged_decode_attention(k_scale=, v_scale=)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("static", [False, True])
@pytest.mark.parametrize("qdt", [BF16, F32])
def test_paged_decode_attention_int8_torch_path(static, qdt):
    c = make_case(64, 8, 2, 24, [0, 1, 7, 33, 60], 5, static)
    ref, bound = case_ref(c)
    out = hot.paged_decode_attention(c["q"].to(qdt), c["kc"], c["vc"],
                                     c["table"], c["lens"],
                                     k_scale=c["ks"], v_scale=c["vs"])
    assert out.dtype == qdt
    assert violations(out, ref, bound) == 0
    assert bool((out[0] == 0).all())


def test_paged_decode_attention_scale_argument_errors():
    c = make_case(64, 4, 2, 16, [5], 1)
    args = (c["q"], c["kc"], c["vc"], c["table"], c["lens"])
    with pytest.raises(ValueError):
        hot.paged_decode_attention(*args, k_scale=c["ks"])
    with pytest.raises(ValueError):      # scales with a bf16 cache
        hot.paged_decode_attention(c["q"], c["kc"].to(BF16), c["vc"].to(BF16),
                                   c["table"], c["lens"], k_scale=c["ks"],
                                   v_scale=c["vs"])
    with pytest.raises(ValueError):      # scale kinds differ
        hot.paged_decode_attention(*args, k_scale=c["ks"],
                                   v_scale=torch.ones(2))


# ---------------------------------------------------------------------------
# predicates
# ---------------------------------------------------------------------------
def _pred_base():
    c = make_case(128, 8, 2, 16, [5, 20], 2)
    return c["q"], c["kc"], c["vc"], c["ks"], c["vs"], c["table"], c["lens"]


def test_kv_int8_native_ok_table():
    q, kc, vc, ks, vs, tb, ln = _pred_base()
    hk = torch.ones(2)
    ok = hot._kv_int8_native_ok
    accept = {
        "base": (q, kc, vc, ks, vs, tb, ln),
        "per head": (q, kc, vc, hk, hk.clone(), tb, ln),
        "int64 table": (q, kc, vc, ks, vs, tb.long(), ln.long()),
        "strided q": (q.transpose(0, 1).contiguous().transpose(0, 1),
                      kc, vc, ks, vs, tb, ln),
        "D 64": (q[..., :64].contiguous(), kc[..., :64].contiguous(),
                 vc[..., :64].contiguous(), ks, vs, tb, ln),
    }
    reject = {
        "q fp32": (q.float(), kc, vc, ks, vs, tb, ln),
        "q 2-D": (q[0], kc, vc, ks, vs, tb, ln),
        "q misaligned": (torch.zeros(q.numel() + 4, dtype=BF16)[4:].view_as(q),
                         kc, vc, ks, vs, tb, ln),
        "D 32": (q[..., :32].contiguous(), kc[..., :32].contiguous(),
                 vc[..., :32].contiguous(), ks, vs, tb, ln),
        "cache D": (q[..., :64].contiguous(), kc, vc, ks, vs, tb, ln),
        "cache bf16": (q, kc.to(BF16), vc.to(BF16), ks, vs, tb, ln),
        "cache strided": (q, kc.transpose(1, 2).contiguous().transpose(1, 2),
                          vc, ks, vs, tb, ln),
        "cache shapes": (q, kc, vc[:-1], ks, vs, tb, ln),
        "H % HKV": (q[:, :7].contiguous(), kc, vc, ks, vs, tb, ln),
        "scale fp64": (q, kc, vc, ks.double(), vs.double(), tb, ln),
        "scale kinds": (q, kc, vc, ks, hk, tb, ln),
        "scale shape": (q, kc, vc, ks[:-1], vs[:-1], tb, ln),
        "scale strided": (q, kc, vc, ks.transpose(0, 1).contiguous().transpose(0, 1),
                          vs, tb, ln),
        "table rows": (q, kc, vc, ks, vs, tb[:1], ln),
        "table float": (q, kc, vc, ks, vs, tb.float(), ln),
        "lens length": (q, kc, vc, ks, vs, tb, ln[:1]),
        "no scale": (q, kc, vc, None, None, tb, ln),
    }
    for name, a in accept.items():
        assert ok(*a), name
    for name, a in reject.items():
        assert not ok(*a), name


def test_kv_quant_append_native_ok_table():
    _, kc, vc, ks, vs, _, _ = _pred_base()
    T, HKV, D = 4, 2, 128
    qkv = torch.zeros(T, 3, HKV, D, dtype=BF16)
    k, v = qkv[:, 1], qkv[:, 2]
    blk, off = torch.arange(T), torch.arange(T)
    hk = torch.ones(HKV)
    odd = torch.zeros(T, HKV * D + 4, dtype=BF16)
    ok = hot._kv_quant_append_native_ok
    accept = {
        "base": (k, v, kc, vc, ks, vs, blk, off),
        "contiguous": (k.contiguous(), v.contiguous(), kc, vc, ks, vs, blk, off),
        "fixed": (k, v, kc, vc, hk, hk.clone(), blk, off, hk, hk),
    }
    reject = {
        "k fp32": (k.float(), v.float(), kc, vc, ks, vs, blk, off),
        "k HKV": (k[:, :1], v[:, :1], kc, vc, ks, vs, blk, off),
        "v T": (k, v[:-1], kc, vc, ks, vs, blk, off),
        "D strided": (k.transpose(1, 2).contiguous().transpose(1, 2), v, kc, vc,
                      ks, vs, blk, off),
        "token stride % 8": (odd[:, :HKV * D].reshape(T, HKV, D), v, kc, vc, ks,
                             vs, blk, off),
        "misaligned": (odd.reshape(-1)[4:4 + T * HKV * D].reshape(T, HKV, D), v,
                       kc, vc, ks, vs, blk, off),
        "cache bf16": (k, v, kc.to(BF16), vc.to(BF16), ks, vs, blk, off),
        "D 32": (k[..., :32], v[..., :32], kc[..., :32].contiguous(),
                 vc[..., :32].contiguous(), ks, vs, blk, off),
        "blk int32": (k, v, kc, vc, ks, vs, blk.int(), off),
        "off length": (k, v, kc, vc, ks, vs, blk, off[:-1]),
        "one quant scale": (k, v, kc, vc, hk, hk, blk, off, hk, None),
        "quant scales with per-token pools": (k, v, kc, vc, ks, vs, blk, off, hk, hk),
        "per-head pools without quant scales": (k, v, kc, vc, hk, hk, blk, off),
        "quant scale shape": (k, v, kc, vc, hk, hk, blk, off, torch.ones(3),
                              torch.ones(3)),
    }
    for name, a in accept.items():
        assert ok(*a), name
    for name, a in reject.items():
        assert not ok(*a), name


# ---------------------------------------------------------------------------
# generation / runner / incubate layers
# ---------------------------------------------------------------------------
def test_paged_kv_cache_int8_roundtrip():
    from paddle_amd.models.generation import PagedKVCache
    L, bs, HKV, D, B = 2, 16, 2, 64, 2
    cache = PagedKVCache(L, 8, bs, HKV, D, B, 40, CPU, kv_cache="int8")
    assert cache.k[0].dtype == I8 and cache.k_scale[1].dtype == F32
    assert tuple(cache.v_scale[0].shape) == (8, bs, HKV)
    g = torch.Generator().manual_seed(0)
    k, v = (torch.randn(B, 20, HKV, D, generator=g).to(BF16) for _ in range(2))
    cache.append(1, k, v, 0)
    cache.append(1, k[:, :1], v[:, :1], 20)
    code, d = ref_quant(k)
    assert torch.equal(cache.k[1][cache.block_table[1, 1].long(), 3], code[1, 19])
    assert torch.equal(cache.k_scale[1][cache.block_table[0, 0].long(), 5], d[0, 5])
    assert torch.equal(cache.v[1][cache.block_table[0, 1].long(), 4],
                       ref_quant(v)[0][0, 0])
    assert not bool(cache.k[0].any())
    bf = PagedKVCache(L, 8, bs, HKV, D, B, 40, CPU)
    assert bf.k[0].dtype == BF16 and bf.k_scale[0] is None
    with pytest.raises(ValueError):
        PagedKVCache(L, 8, bs, HKV, D, B, 40, CPU, kv_cache="fp4")


def test_generate_int8_kv_cache_runs():
    from paddle_amd.models import build_gpt
    from paddle_amd.models.generation import generate_gpt, generate_llama
    from paddle_amd.models.llama import build_llama
    paddle.seed(0)
    ids = torch.randint(0, 1024, (2, 9))
    m = build_gpt("gpt3-tiny", max_seq_len=64).to(CPU).float()
    out = generate_gpt(m, ids, max_new_tokens=4, kv_cache="int8")
    assert tuple(out.shape) == (2, 4)
    assert torch.equal(out[:, 0], generate_gpt(m, ids, max_new_tokens=1)[:, 0])
    lm = build_llama("llama-tiny", max_seq_len=64).to(CPU).float().eval()
    assert tuple(generate_llama(lm, ids, max_new_tokens=4,
                                kv_cache="int8").shape) == (2, 4)


def test_runner_int8_kv_cache_under_engine():
    from paddle_amd.models import build_gpt
    from paddle_amd.serving import Engine, GPTModelRunner, Request
    paddle.seed(0)
    m = build_gpt("gpt3-tiny", max_seq_len=128).to(CPU).float()
    runner = GPTModelRunner(m, num_blocks=64, block_size=16,
                            device=torch.device(CPU), kv_cache="int8")
    assert runner.k[0].dtype == I8
    assert tuple(runner.k_scale[0].shape) == (65, 16, runner.HKV)
    eng = Engine(runner, num_blocks=64, block_size=16, max_batch=3)
    reqs = [Request(prompt_ids=[3 + i, 7, 11][:2 + i % 2], max_new_tokens=5)
            for i in range(4)]
    for r in reqs:
        eng.add_request(r)
    eng.run_until_done()
    assert all(r.done and len(r.out_ids) == 5 for r in reqs)
    assert len(eng.alloc.free) == 64
    assert bool(runner.k[0].any()) and bool((runner.k_scale[0] > 0).any())
    with pytest.raises(ValueError):
        GPTModelRunner(m, num_blocks=64, block_size=16,
                       device=torch.device(CPU), kv_cache="fp4")


def _bmha_inputs(D=64, H=2, bs=16, prompt=19):
    g = torch.Generator().manual_seed(4)
    nblocks = 6
    tables = torch.tensor([[4, 1, 3], [0, 5, 2]], dtype=torch.int32)
    pre = torch.randn(2 * prompt, 3 * H * D, generator=g)
    dec = torch.randn(2, 3 * H * D, generator=g)
    kq = torch.tensor([127 / 3.0, 127 / 4.0])
    vq = torch.tensor([127 / 3.5, 127 / 2.5])
    return nblocks, tables, pre, dec, kq, vq


def test_block_multihead_attention_static_int8():
    from paddle_amd.incubate.nn import functional as IF
    D, H, bs, S0 = 64, 2, 16, 19
    nblocks, tables, pre, dec, kq, vq = _bmha_inputs(D, H, bs, S0)
    kc = torch.zeros(nblocks, bs, H, D, dtype=I8)
    vc = kc.clone()
    kw = dict(block_tables=tables, cache_k_quant_scales=kq,
              cache_v_quant_scales=vq, cache_k_dequant_scales=1 / kq,
              cache_v_dequant_scales=1 / vq, block_size=bs)
    z, s0, one = (torch.tensor([0, 0]), torch.tensor([S0, S0]),
                  torch.tensor([1, 1]))
    IF.block_multihead_attention(pre, kc, vc, s0, z, s0, **kw)
    out, _, _, _ = IF.block_multihead_attention(dec, kc, vc, z, s0, one, **kw)
    # the reference: every cached row is the documented static quantisation
    k_all = torch.cat([pre.reshape(2, S0, 3, H, D)[:, :, 1],
                       dec.reshape(2, 1, 3, H, D)[:, :, 1]], 1)
    v_all = torch.cat([pre.reshape(2, S0, 3, H, D)[:, :, 2],
                       dec.reshape(2, 1, 3, H, D)[:, :, 2]], 1)
    pos = torch.arange(S0 + 1)
    for b in range(2):
        pb = tables[b].long()[pos // bs]
        assert torch.equal(kc[pb, pos % bs], ref_quant(k_all[b], kq)[0])
        assert torch.equal(vc[pb, pos % bs], ref_quant(v_all[b], vq)[0])
    c = dict(q=dec.reshape(2, 3, H, D)[:, 0], kc=kc, vc=vc, ks=1 / kq, vs=1 / vq,
             table=tables, lens=torch.tensor([S0 + 1, S0 + 1], dtype=torch.int32))
    ref, bound = case_ref(c)
    assert violations(out.reshape(2, H, D), ref, bound) == 0
    with pytest.raises(NotImplementedError, match="paged_decode_attention"):
        IF.block_multihead_attention(dec, kc, vc, z, s0, one,
                                     use_dynamic_cachekv_quant=True, **kw)
    with pytest.raises(NotImplementedError):
        IF.block_multihead_attention(dec, kc, vc, z, s0, one, pre_key_cache=kc,
                                     **kw)
    with pytest.raises(ValueError):
        IF.block_multihead_attention(dec, kc, vc, z, s0, one,
                                     block_tables=tables, block_size=bs)
