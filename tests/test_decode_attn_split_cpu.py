"""Split-KV paged decode attention without a GPU: a fp32 emulation of
the split decode_attn_kernel + decode_attn_merge_kernel (slice rule, per-slot
online softmax, in-block slot merge, partials, split merge, bf16 cast)
showing that the bound of test_decode_attn_split_gpu.py accepts the design
for every split count and rejects the mistakes such kernels can make; the
slice rule as a partition; the split heuristic's properties; the dispatch
predicate; and the CPU behaviour of the new arguments.
"""
import math

import pytest
import torch

import paddle_amd as paddle
from paddle_amd.ops import functional as hot

from test_decode_attn_split_gpu import (EDGE_LENS, KINDS, SHAPES, SPLITS,
                                        bf16_image, case_of_kind,
                                        needle_head_case, ref_of)
from test_kv_int8_gpu import BF16, F32, make_case, violations

CPU = "cpu"


def slices(S, n):
    """The documented slice rule for one sequence of S cached positions."""
    c = 64 * -(-S // (64 * n))
    return [(s * c, min(S, (s + 1) * c)) for s in range(n)]


# ---------------------------------------------------------------------------
# fp32 emulation of the two kernels.  `mutant` plants one mistake.
# ---------------------------------------------------------------------------
def emulate(c, n, mutant=None):
    q, kc, vc, ks, vs, table, lens = (c[k] for k in
                                      ("q", "kc", "vc", "ks", "vs", "table", "lens"))
    int8 = ks is not None
    B, H, D = q.shape
    bs, HKV = kc.shape[1], kc.shape[2]
    rep = H // HKV
    slots = (4 * 64 // (D // 16)) if int8 else 16      # positions per block step
    scale = torch.tensor(1.0 / math.sqrt(D), dtype=F32)
    hmap = torch.arange(H) // rep
    out = torch.zeros(B, H, D, dtype=F32)
    for b in range(B):
        S = max(0, min(int(lens[b]), table.shape[1] * bs))
        pm = torch.full((n, H), -1e30, dtype=F32)       # ml_part / o_part
        pl = torch.zeros(n, H, dtype=F32)
        po = torch.zeros(n, H, D, dtype=F32)
        empty = torch.zeros(n, dtype=torch.bool)
        for s, (beg, end) in enumerate(slices(S, n)):
            if mutant == "drop_slice_end":
                end -= 1
            if beg >= end:
                empty[s] = True
                continue
            pos = torch.arange(beg, end)
            pb, off = table[b].long()[pos // bs], pos % bs
            kk = kc[pb, off][:, hmap].to(F32)            # [L, H, D]
            vv = vc[pb, off][:, hmap].to(F32)
            sc = torch.einsum("hd,shd->sh", q[b].to(F32) * scale, kk)
            dv = torch.ones(len(pos), H, dtype=F32)
            if int8:
                per_tok = ks.dim() == 3
                dk = ks[pb, off][:, hmap] if per_tok else ks[hmap].expand(len(pos), H)
                dv = vs[pb, off][:, hmap] if per_tok else vs[hmap].expand(len(pos), H)
                sc = sc * dk
            m = torch.full((slots, H), -1e30, dtype=F32)
            l = torch.zeros(slots, H, dtype=F32)
            o = torch.zeros(slots, H, D, dtype=F32)
            for p0 in range(0, end - beg, slots):
                k_ = min(slots, end - beg - p0)
                s_ = sc[p0:p0 + k_]
                m_new = torch.maximum(m[:k_], s_)
                corr = torch.exp(m[:k_] - m_new)
                p = torch.exp(s_ - m_new)
                l[:k_] = l[:k_] * corr + p
                o[:k_] = o[:k_] * corr.unsqueeze(-1) + \
                    (p * dv[p0:p0 + k_]).unsqueeze(-1) * vv[p0:p0 + k_]
                m[:k_] = m_new
            gm = m.amax(0)
            w = torch.where(l > 0, torch.exp(m - gm), torch.zeros_like(l))
            pm[s], pl[s], po[s] = gm, (l * w).sum(0), (w.unsqueeze(-1) * o).sum(0)
        if mutant == "neighbour_head":
            # head h merges the partials of its neighbour in the group
            nb = torch.arange(H) ^ 1 if rep > 1 else (torch.arange(H) + 1) % H
            pm, pl, po = pm[:, nb], pl[:, nb], po[:, nb]
        gm = pm.amax(0)
        w = torch.where(pl > 0, torch.exp(pm - gm), torch.zeros_like(pl))
        if mutant == "no_rescale":
            w = (pl > 0).to(F32)
        if mutant == "empty_weighted":
            # an empty split left as unguarded sentinel arithmetic leaves it
            # (one masked position: p = exp(-1e30 - -1e30) = 1, so l = 1,
            # o = 0) and taken into the merge with weight 1
            pl = torch.where(empty.unsqueeze(-1), torch.ones_like(pl), pl)
            w = torch.where(empty.unsqueeze(-1), torch.ones_like(w), w)
        gl = (pl * w).sum(0)
        acc = (w.unsqueeze(-1) * po).sum(0)
        inv = torch.where(gl > 0, 1.0 / gl, torch.zeros_like(gl))
        out[b] = acc * inv.unsqueeze(-1)
    return out.to(BF16)


MUTANTS = ["drop_slice_end", "empty_weighted", "no_rescale", "neighbour_head"]
EMU_CASES = [(k,) + s for k in ("int8_token", "bf16") for s in SHAPES] + \
    [("int8_head",) + SHAPES[0]]


@pytest.fixture(scope="module")
def edge_cases():
    out = {}
    for kind, D, H, HKV, bs in EMU_CASES:
        c = case_of_kind(kind, D, H, HKV, bs, EDGE_LENS, 2001 + D + 8 * HKV + bs)
        out[(kind, D, H, HKV, bs)] = (c,) + ref_of(c)
    return out


@pytest.mark.parametrize("kind,D,H,HKV,bs", EMU_CASES)
def test_bound_accepts_split_design(edge_cases, kind, D, H, HKV, bs):
    c, ref, bound = edge_cases[(kind, D, H, HKV, bs)]
    for n in SPLITS:
        out = emulate(c, n)
        assert violations(out, ref, bound) == 0, n
        assert bool((out[0] == 0).all())            # S = 0


@pytest.mark.parametrize("mutant", MUTANTS)
@pytest.mark.parametrize("kind", ["int8_token", "bf16"])
def test_bound_rejects_split_mutants(edge_cases, kind, mutant):
    c, ref, bound = edge_cases[(kind,) + SHAPES[0]]
    for n in SPLITS[1:]:
        assert violations(emulate(c, n, mutant), ref, bound) > 0, (mutant, n)


@pytest.mark.parametrize("kind", ["int8_token", "bf16"])
def test_needle_probes_catch_slice_and_head_mistakes(kind):
    D, H, HKV, bs, S = 128, 8, 2, 16, 513
    assert slices(S, 4) == [(0, 192), (192, 384), (384, 513), (576, 513)]
    for n in (191, 192, 512, 0):
        for j in (0, 3):
            c = needle_head_case(kind, D, H, HKV, bs, S, n, j, 500 + 7 * n + j)
            ref, bound = ref_of(c)
            assert float((ref[0, j] - 3.0).abs().max()) < 1.5
            assert violations(emulate(c, 4), ref, bound) == 0, (n, j)
            assert violations(emulate(c, 4, "neighbour_head"), ref, bound) > 0
            if n in (191, 512):
                assert violations(emulate(c, 4, "drop_slice_end"), ref, bound) > 0


# ---------------------------------------------------------------------------
# slice rule
# ---------------------------------------------------------------------------
def test_slice_rule_partitions_the_sequence():
    for n in range(1, 9):
        for S in range(0, 601):
            sl = slices(S, n)
            live = [(a, b) for a, b in sl if a < b]
            covered = [p for a, b in live for p in range(a, b)]
            assert covered == list(range(S)), (S, n)
            # live slices come first and begin on the 64-position granule
            assert [a < b for a, b in sl] == sorted((a < b for a, b in sl),
                                                    reverse=True)
            assert all(a % 64 == 0 for a, _ in sl)
            assert len(live) == (0 if S == 0 else -(-S // (64 * -(-S // (64 * n)))))
    assert sum(a < b for a, b in slices(1, 8)) == 1      # seven empty splits


# ---------------------------------------------------------------------------
# heuristic
# ---------------------------------------------------------------------------
def test_decode_attn_split_plan_properties():
    plan = hot._decode_attn_split_plan
    for int8 in (False, True):
        for H, HKV in ((32, 32), (32, 8), (8, 2), (8, 1), (6, 2), (2, 1), (64, 8)):
            for D in (64, 128):
                for cap in (16, 256, 272, 496, 511, 512, 1024, 2048, 4096,
                            16384, 1 << 20):
                    prev = None
                    for B in (1, 2, 3, 4, 8, 16, 32, 64, 256):
                        n = plan(B, H, HKV, D, cap, int8)
                        assert isinstance(n, int) and 1 <= n <= 64
                        if cap < 512:
                            assert n == 1
                        if n > 1:
                            assert cap // n >= 256
                        assert prev is None or n <= prev     # non-increasing in B
                        prev = n
    # the unsplit grid already fills the device: today's kernels
    assert plan(32, 32, 32, 128, 4096, False) == 1
    assert plan(64, 32, 8, 128, 4096, False) == 1
    # the two shapes that motivated the change
    assert plan(1, 32, 32, 128, 4096, False) > 1
    assert plan(1, 32, 8, 128, 4096, True) > 1
    assert plan(1, 7, 2, 128, 4096, False) == 1              # H % HKV


def test_decode_attn_split_tiles():
    tiles = hot._decode_attn_split_tiles
    assert tiles(8, 8, False) == (1, 1) and tiles(8, 4, True) == (2, 1)
    assert tiles(6, 2, False) == (4, 1) and tiles(8, 2, True) == (4, 1)
    assert tiles(8, 1, False) == (8, 1) and tiles(8, 1, True) == (4, 2)
    assert tiles(40, 2, False) == (8, 3) and tiles(5, 1, True) == (4, 2)


# ---------------------------------------------------------------------------
# predicate
# ---------------------------------------------------------------------------
def test_decode_attn_split_native_ok_table():
    c = make_case(128, 8, 2, 16, [5, 20], 2)
    q, kc, vc, ks, vs, tb, ln = (c[k] for k in
                                 ("q", "kc", "vc", "ks", "vs", "table", "lens"))
    cb = bf16_image(c)
    kb, vb = cb["kc"], cb["vc"]
    hk = torch.ones(2)
    ok = hot._decode_attn_split_native_ok
    meta = torch.empty(kb.shape, dtype=BF16, device="meta")
    accept = {
        "bf16": (q, kb, vb, tb, ln),
        "int8 per token": (q, kc, vc, tb, ln, ks, vs),
        "int8 per head": (q, kc, vc, tb, ln, hk, hk.clone()),
        "int64 table": (q, kb, vb, tb.long(), ln.long()),
        "strided q": (q.transpose(0, 1).contiguous().transpose(0, 1), kb, vb,
                      tb, ln),
        "D 64": (q[..., :64].contiguous(), kb[..., :64].contiguous(),
                 vb[..., :64].contiguous(), tb, ln),
    }
    reject = {
        "q fp32": (q.float(), kb, vb, tb, ln),
        "q 2-D": (q[0], kb, vb, tb, ln),
        "q misaligned": (torch.zeros(q.numel() + 4, dtype=BF16)[4:].view_as(q),
                         kb, vb, tb, ln),
        "D 32": (q[..., :32].contiguous(), kb[..., :32].contiguous(),
                 vb[..., :32].contiguous(), tb, ln),
        "D 96": (torch.zeros(2, 8, 96, dtype=BF16),
                 torch.zeros(4, 16, 2, 96, dtype=BF16),
                 torch.zeros(4, 16, 2, 96, dtype=BF16), tb, ln),
        "cache D": (q[..., :64].contiguous(), kb, vb, tb, ln),
        "cache fp32": (q, kb.float(), vb.float(), tb, ln),
        "cache int8 without scales": (q, kc, vc, tb, ln),
        "cache bf16 with scales": (q, kb, vb, tb, ln, ks, vs),
        "cache strided": (q, kb.transpose(1, 2).contiguous().transpose(1, 2),
                          vb, tb, ln),
        "cache shapes": (q, kb, vb[:-1], tb, ln),
        "cache misaligned": (q, torch.zeros(kb.numel() + 4, dtype=BF16)[4:]
                             .view_as(kb), vb, tb, ln),
        "cache on another device": (q, meta, meta, tb, ln),
        "H % HKV": (q[:, :7].contiguous(), kb, vb, tb, ln),
        "one scale": (q, kc, vc, tb, ln, ks, None),
        "scale kinds": (q, kc, vc, tb, ln, ks, hk),
        "table rows": (q, kb, vb, tb[:1], ln),
        "table float": (q, kb, vb, tb.float(), ln),
        "lens length": (q, kb, vb, tb, ln[:1]),
        "lens a list": (q, kb, vb, tb, [5, 20]),
    }
    for name, a in accept.items():
        assert ok(*a), name
    for name, a in reject.items():
        assert not ok(*a), name


PRED_KINDS = ("bf16", "int8_token", "int8_head")


def _pred_args(kind):
    """In-contract arguments of _paged_decode_native_ok, by name."""
    c = make_case(128, 8, 2, 16, [5, 20], 2)
    if kind == "bf16":
        c = bf16_image(c)
    elif kind == "int8_head":
        c["ks"], c["vs"] = torch.ones(2), torch.ones(2)
    return {k: c[k] for k in ("q", "kc", "vc", "table", "lens", "ks", "vs")}


def _pred(a):
    return hot._paged_decode_native_ok(a["q"], a["kc"], a["vc"], a["table"],
                                       a["lens"], a["ks"], a["vs"])


def _cut_d(a, d):
    return dict(a, q=a["q"][..., :d].contiguous(),
                kc=a["kc"][..., :d].contiguous(),
                vc=a["vc"][..., :d].contiguous())


def _misaligned(t):
    return torch.zeros(t.numel() + 4, dtype=t.dtype)[4:].view_as(t)


def _strided(t):
    return t.transpose(0, 1).contiguous().transpose(0, 1)


def _d96(a):
    z = lambda t: torch.zeros(*t.shape[:-1], 96, dtype=t.dtype)
    return dict(a, q=z(a["q"]), kc=z(a["kc"]), vc=z(a["vc"]))


ALL, INT8, TOKEN = PRED_KINDS, PRED_KINDS[1:], PRED_KINDS[1:2]
# (name, kinds it applies to, mutation of the in-contract arguments)
PRED_ACCEPT = [
    ("base", ALL, lambda a: a),
    ("int64 table", ALL, lambda a: dict(a, table=a["table"].long(),
                                        lens=a["lens"].long())),
    ("strided q", ALL, lambda a: dict(a, q=_strided(a["q"]))),
    ("D 64", ALL, lambda a: _cut_d(a, 64)),
]
PRED_REJECT = [
    ("q fp32", ALL, lambda a: dict(a, q=a["q"].float())),
    ("q 2-D", ALL, lambda a: dict(a, q=a["q"][0])),
    ("q misaligned", ALL, lambda a: dict(a, q=_misaligned(a["q"]))),
    ("q a list", ALL, lambda a: dict(a, q=a["q"].tolist())),
    ("D 32", ALL, lambda a: _cut_d(a, 32)),
    ("D 96", ALL, _d96),
    ("cache D", ALL, lambda a: dict(a, q=a["q"][..., :64].contiguous())),
    ("cache fp32", ALL, lambda a: dict(a, kc=a["kc"].float(),
                                       vc=a["vc"].float())),
    ("cache bf16 with scales", INT8, lambda a: dict(a, kc=a["kc"].to(BF16),
                                                    vc=a["vc"].to(BF16))),
    ("cache int8 without scales", INT8, lambda a: dict(a, ks=None, vs=None)),
    ("cache strided", ALL, lambda a: dict(
        a, kc=a["kc"].transpose(1, 2).contiguous().transpose(1, 2))),
    ("v cache strided", ALL, lambda a: dict(
        a, vc=a["vc"].transpose(1, 2).contiguous().transpose(1, 2))),
    ("cache shapes", ALL, lambda a: dict(a, vc=a["vc"][:-1])),
    ("cache misaligned", ALL, lambda a: dict(a, kc=_misaligned(a["kc"]))),
    ("cache on another device", ALL, lambda a: dict(
        a, kc=a["kc"].to("meta"), vc=a["vc"].to("meta"))),
    ("H % HKV", ALL, lambda a: dict(a, q=a["q"][:, :7].contiguous())),
    ("one scale", INT8, lambda a: dict(a, vs=None)),
    ("scale fp64", INT8, lambda a: dict(a, ks=a["ks"].double(),
                                        vs=a["vs"].double())),
    ("scale kinds", TOKEN, lambda a: dict(a, vs=torch.ones(2))),
    ("scale shape", INT8, lambda a: dict(a, ks=a["ks"][:-1], vs=a["vs"][:-1])),
    ("scale strided", TOKEN, lambda a: dict(a, ks=_strided(a["ks"]))),
    ("scale on another device", INT8, lambda a: dict(
        a, ks=a["ks"].to("meta"), vs=a["vs"].to("meta"))),
    ("table rows", ALL, lambda a: dict(a, table=a["table"][:1])),
    ("table float", ALL, lambda a: dict(a, table=a["table"].float())),
    ("table on another device", ALL, lambda a: dict(
        a, table=a["table"].to("meta"))),
    ("lens length", ALL, lambda a: dict(a, lens=a["lens"][:1])),
    ("lens a list", ALL, lambda a: dict(a, lens=[5, 20])),
]


@pytest.mark.parametrize("kind", PRED_KINDS)
def test_paged_decode_native_ok_table(kind):
    """One predicate for decode_attention, decode_attention_int8 and
    decode_attention_split, mirroring check_paged_decode."""
    base = _pred_args(kind)
    for name, kinds, mutate in PRED_ACCEPT:
        if kind in kinds:
            assert _pred(mutate(base)), name
    for name, kinds, mutate in PRED_REJECT:
        if kind in kinds:
            assert not _pred(mutate(base)), name


def test_paged_decode_attention_off_contract_bf16_torch_path_on_cpu():
    """bf16 inputs outside the predicate (which the unsplit dispatch once
    copied with .contiguous()) give what the in-contract call gives."""
    a = _pred_args("bf16")
    call = lambda a: hot.paged_decode_attention(a["q"], a["kc"], a["vc"],
                                                a["table"], a["lens"])
    base = call(a)
    off = {
        "cache strided": dict(
            a, kc=a["kc"].transpose(1, 2).contiguous().transpose(1, 2),
            vc=a["vc"].transpose(1, 2).contiguous().transpose(1, 2)),
        "q misaligned": dict(a, q=_misaligned(a["q"]).copy_(a["q"])),
        "cache misaligned": dict(a, kc=_misaligned(a["kc"]).copy_(a["kc"])),
    }
    for name, b in off.items():
        assert not _pred(b), name
        assert torch.equal(call(b), base), name


# ---------------------------------------------------------------------------
# CPU behaviour of the new arguments
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_paged_decode_attention_num_splits_ignored_on_cpu(kind):
    c = case_of_kind(kind, 128, 8, 2, 16, [0, 1, 65, 250], 5)
    args = (c["q"], c["kc"], c["vc"], c["table"], c["lens"])
    kw = dict(k_scale=c["ks"], v_scale=c["vs"])
    base = hot.paged_decode_attention(*args, **kw)
    for n in (None, 0, 1, 3, 64):
        assert torch.equal(hot.paged_decode_attention(*args, num_splits=n, **kw),
                           base)
    for n in (-1, 65, 2.5):
        with pytest.raises(ValueError, match="num_splits"):
            hot.paged_decode_attention(*args, num_splits=n, **kw)


def test_generate_and_runner_take_decode_splits_on_cpu():
    from paddle_amd.models import build_gpt
    from paddle_amd.models.generation import generate_gpt, generate_llama
    from paddle_amd.models.llama import build_llama
    from paddle_amd.serving import Engine, GPTModelRunner, LlamaModelRunner, Request
    paddle.seed(0)
    ids = torch.randint(0, 1024, (2, 9))
    m = build_gpt("gpt3-tiny", max_seq_len=64).to(CPU).float()
    assert torch.equal(generate_gpt(m, ids, max_new_tokens=3, decode_splits=3),
                       generate_gpt(m, ids, max_new_tokens=3))
    lm = build_llama("llama-tiny", max_seq_len=64).to(CPU).float().eval()
    assert torch.equal(generate_llama(lm, ids, max_new_tokens=3, decode_splits=0),
                       generate_llama(lm, ids, max_new_tokens=3))
    for cls, model in ((GPTModelRunner, m), (LlamaModelRunner, lm)):
        toks = []
        for ds in (None, 0, 4):
            runner = cls(model, num_blocks=16, block_size=16, max_seq=64,
                         device=torch.device(CPU), decode_splits=ds)
            assert runner.decode_splits == ds
            eng = Engine(runner, num_blocks=16, block_size=16, max_batch=2)
            reqs = [Request(prompt_ids=[3, 7, 11 + i], max_new_tokens=3)
                    for i in range(2)]
            for r in reqs:
                eng.add_request(r)
            eng.run_until_done()
            toks.append([r.out_ids for r in reqs])
        assert toks[0] == toks[1] == toks[2]
        for bad in (-1, 65, 1.5):
            with pytest.raises(ValueError, match="decode_splits"):
                cls(model, num_blocks=16, block_size=16, max_seq=64,
                    device=torch.device(CPU), decode_splits=bad)
