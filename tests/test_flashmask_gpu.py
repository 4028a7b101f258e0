"""FlashMask on the GPU (csrc/kernels/flashmask.hip): flashmask_prep + the
forward + the backward through paddle_amd._C, and flashmask_attention through
autograd, against the fp64 reference and the bounds of flashmask_ref.py.  The
backward through _C gets the reference's own bf16 O and fp32 LSE.
test_flashmask_cpu.py shows on the CPU that these bounds accept the design of
the tile walk and reject the mistakes it could make.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from paddle_amd import _ext  # noqa: E402
from paddle_amd.ops import functional as hot  # noqa: E402
from flashmask_ref import OUTPUTS, case, with_forward, worst  # noqa: E402

DEV = "cuda:0"
ALT = dict(sq=200, skv=264, docs=(0, 90, 200))
# (case, D, H, Hm, other shape)
CASES = [(n, 128, 2, 1, {}) for n in ("docs", "prefix_window", "hole", "bidir_docs", "dead")] + [
    ("docs", 64, 2, 1, {}), ("dead", 64, 2, 1, {}), ("hole", 128, 2, 2, {}),
    ("bidir_docs", 128, 2, 1, ALT)]


def _id(c):
    return "%s_d%d_h%d_hm%d%s" % (c[0], c[1], c[2], c[3], "_200x264" if c[4] else "")


def _run(C, c, q, k, v, do, o_ref, outs=(None, None, None, None)):
    fm = C.flashmask_prep(c["idx"].to(DEV), q.shape[2], c["causal"])
    o, lse = C.flash_attn_fwd(q, k, v, outs[0], c["scale"], c["causal"], flashmask=fm)
    dq, dk, dv = C.flash_attn_bwd(do, q, k, v, o_ref, c["lse"].to(DEV), *outs[1:],
                                  c["scale"], c["causal"], flashmask=fm)
    torch.cuda.synchronize()
    return dict(o=o, lse=lse, dq=dq, dk=dk, dv=dv)


def _check(tag, c, got):
    w = {n: worst(c, n, got[n]) for n in OUTPUTS}
    print(f"[flashmask] {tag}: err/bound " + " ".join(f"{n}={w[n]:.4f}" for n in OUTPUTS)
          + " E " + " ".join(f"{n}={c['E'][n]:.3g}" for n in OUTPUTS))
    assert all(x <= 1.0 for x in w.values()), w


@pytest.mark.parametrize("cs", CASES, ids=[_id(c) for c in CASES])
def test_flashmask_kernels(cs):
    C = _ext.get_ext(required=True)
    name, d, h, hm, other = cs
    c = case(name, d, h, hm, **other)
    q, k, v, do, o_ref = (c[n].to(DEV) for n in ("q", "k", "v", "do", "o"))
    got = _run(C, c, q, k, v, do, o_ref)
    _check(_id(cs), c, got)
    if name == "docs" and d == 128:
        # the strides of the packed [B, S, 3, H, D] layout: bit-equal
        qkv = torch.stack([q, k, v], 0).permute(1, 3, 0, 2, 4).contiguous()
        qp, kp, vp = (qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
        bshd = lambda t: t.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)  # noqa: E731
        dqkv = torch.full_like(qkv, float("nan"))
        outs = [torch.full_like(bshd(o_ref), float("nan"))] + \
            [dqkv[:, :, i].permute(0, 2, 1, 3) for i in range(3)]
        gp = _run(C, c, qp, kp, vp, bshd(do), bshd(o_ref), outs)
        for n in OUTPUTS:
            assert torch.equal(gp[n], got[n]), n


@pytest.mark.parametrize("name,kw,h,hkv,hm", [
    ("docs", {}, 2, 2, 1), ("docs", {"window_size": (63, 0)}, 2, 2, 1), ("hole", {}, 4, 2, 2)],
    ids=["docs", "window", "gqa"])
def test_flashmask_autograd(name, kw, h, hkv, hm):
    _ext.get_ext(required=True)
    c = case("window" if kw else name, 128, h, hm, hkv=hkv)
    q, k, v = (c[n].to(DEV).transpose(1, 2).contiguous().requires_grad_() for n in ("q", "k", "v"))
    idx = None if kw else c["idx"].to(DEV)
    o, lse = hot.flashmask_attention(q, k, v, idx, causal=c["causal"],
                                     return_softmax_lse=True, **kw)
    o.backward(c["do"].to(DEV).transpose(1, 2))
    torch.cuda.synchronize()
    got = dict(o=o.transpose(1, 2), lse=lse, dq=q.grad.transpose(1, 2),
               dk=k.grad.transpose(1, 2), dv=v.grad.transpose(1, 2))
    # O and LSE against the case; the grads against the reference of a
    # backward that read the O and LSE this forward saved
    assert worst(c, "o", got["o"]) <= 1.0 and worst(c, "lse", got["lse"]) <= 1.0
    _check("autograd_" + name + ("_window" if kw else ""),
           with_forward(c, got["o"], got["lse"]), got)


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
def test_flashmask_empty_ranges_equal_dense(causal):
    C = _ext.get_ext(required=True)
    c = case("docs")
    q, k, v = (c[n].to(DEV) for n in ("q", "k", "v"))
    idx = torch.full((1, 1, 328, 2), 328, dtype=torch.int32, device=DEV)
    idx[..., 1] = 328 if causal else 0
    fm = C.flashmask_prep(idx, 328, causal)
    o, lse = C.flash_attn_fwd(q, k, v, None, c["scale"], causal, flashmask=fm)
    o0, lse0 = C.flash_attn_fwd(q, k, v, None, c["scale"], causal)
    assert torch.equal(o, o0) and torch.equal(lse, lse0)


def _contract_calls():
    def prep(idx, causal=False):
        return lambda C, t: C.flashmask_prep(idx(t), 328, causal)

    def fwd(fm=None, **kw):
        def f(C, t):
            pair = C.flashmask_prep(t["idx"], 328, False) if fm is None else fm(C, t)
            return C.flash_attn_fwd(t["q"], t["k"], t["v"], None, 0.1, False, flashmask=pair,
                                    **{n: g(t) for n, g in kw.items()})
        return f
    i4 = lambda t, hm=1, skv=328, c=2: torch.zeros((1, hm, skv, c), dtype=torch.int32, device=DEV)  # noqa: E731
    return {
        "dtype": prep(lambda t: i4(t).long()),
        "c3": prep(lambda t: i4(t, c=3)),
        "c4_causal": prep(lambda t: i4(t, c=4), True),
        "hm3": fwd(lambda C, t: C.flashmask_prep(i4(t, hm=3), 328, False)),
        "skv": fwd(lambda C, t: C.flashmask_prep(i4(t, skv=264), 328, False)),
        "noncontiguous": prep(lambda t: i4(t, c=4)[..., ::2]),
        "dropout": fwd(pdrop=lambda t: 0.1),
        "additive_mask": fwd(mask=lambda t: torch.zeros((1, 1, 328, 328), dtype=torch.bfloat16,
                                                        device=DEV)),
    }


@pytest.mark.parametrize("what", list(_contract_calls()))
def test_flashmask_contract(what):
    C = _ext.get_ext(required=True)
    c = case("bidir_docs")
    t = {n: c[n].to(DEV) for n in ("q", "k", "v", "idx")}
    with pytest.raises(RuntimeError, match="flash"):
        _contract_calls()[what](C, t)
