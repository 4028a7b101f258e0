"""MoELayer(dispatch="dropless") on the torch fallback (CPU, fp32) against the
definition out[t] = sum_kk topv[t, kk] * FFN_{topi[t, kk]}(x_t), token by
token in fp64, and fp64 autograd of it.

Tolerance, first order, from the reference's own terms: every fp32 result is
a chain of sums -- fc1 (h + 1 terms), GELU (erf, exp: <= 8 ulp), fc2 (I + 1),
the softmax over E (E + 4) and the combine (K) -- so with n their total
length, |err| <= n 2^-24 S, where S is the same expression over absolute
values with GELU replaced by its majorant 1.13 |z| (|gelu'| <= 1.13): all its
terms are positive, so it bounds both the terms of the last sum and every
propagated error.  For a gradient S is the gradient of that majorant (autograd
of a positive expression is the sum of the absolute terms of the gradient),
plus for x.grad the path through the gate: |dL/dtopv| |softmax Jacobian| |wg|."""
import pytest
import torch

import paddle_amd as paddle
from paddle_amd.models.moe import MoELayer

U = 2.0 ** -24
E, K, H, I, T = 4, 2, 16, 32, 24


def _ffn_sum(x, topv, topi, w1, b1, w2, b2, act):
    rows = []
    for t in range(x.shape[0]):
        acc = 0
        for kk in range(topi.shape[1]):
            e = int(topi[t, kk])
            acc = acc + topv[t, kk] * (act(x[t] @ w1[e] + b1[e]) @ w2[e] + b2[e])
        rows.append(acc)
    return torch.stack(rows)


def test_dropless_layer_matches_definition():
    paddle.seed(0)
    layer = MoELayer(H, I, E, k=K, capacity_factor=0.5, dispatch="dropless")
    with torch.no_grad():
        # feature 0 is a constant 4: expert 0 is every token's first choice and
        # expert E - 1 is nobody's
        layer.gate.wg.weight.mul_(5.0)
        layer.gate.wg.weight[0] = torch.tensor([2.0, 0.0, 0.0, -2.0])
        for b in (layer.experts.b1, layer.experts.b2):
            b.normal_(0.0, 0.1)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(1, T, H, generator=g) * 0.5
    x[..., 0] = 4.0
    x.requires_grad_()
    gout = torch.randn(1, T, H, generator=g)
    out = layer(x)
    (out * gout).sum().backward()

    ex = layer.experts
    names = ("w1", "b1", "w2", "b2")
    p64 = [getattr(ex, n).detach().double().requires_grad_() for n in names]
    x64 = x.detach().double().reshape(T, H).requires_grad_()
    wg = layer.gate.wg.weight.detach().double()
    probs = torch.softmax(x64 @ wg, -1)
    topv, topi = probs.topk(K, -1)
    counts = torch.bincount(topi.reshape(-1), minlength=E)
    cap = max(int(layer.capacity_factor * T * K / E) + 1, 4)
    assert int(counts[E - 1]) == 0 and int(counts[0]) > cap
    ref = _ffn_sum(x64, topv, topi, *p64, torch.nn.functional.gelu)
    g64 = gout.double().reshape(T, H)
    (ref * g64).sum().backward()

    # the positive majorant and its gradients
    a64 = [p.detach().abs().requires_grad_() for p in p64]
    xa = x64.detach().abs().requires_grad_()
    pv = topv.detach()
    y_abs = _ffn_sum(xa, torch.ones_like(pv), topi, *a64, lambda z: 1.13 * z)
    s_out = _ffn_sum(xa, pv, topi, *a64, lambda z: 1.13 * z)
    (s_out * g64.abs()).sum().backward()
    pd = probs.detach()
    jac = (pd.gather(1, topi)[:, :, None]
           * ((torch.arange(E) == topi[:, :, None]).double() - pd[:, None, :])).abs()
    # y_abs summed both choices with weight 1: an upper bound of each |dL/dtopv|
    gate = ((y_abs.detach() * g64.abs()).sum(1)[:, None, None] * jac).sum(1) @ wg.abs().t()
    n = (H + 1) + 8 + (I + 1) + (E + 4) + K

    def inside(got, want, s, what):
        err = (got.detach().double() - want.detach()).abs()
        bound = n * U * s.detach()
        print(f"dropless cpu {what}: worst err/bound {float((err / bound.clamp(min=1e-300)).max()):.3f}")
        assert bool((err <= bound).all()), what

    inside(out.reshape(T, H), ref, s_out, "out")
    inside(x.grad.reshape(T, H), x64.grad, xa.grad + gate, "x.grad")
    for name, p, a in zip(names, p64, a64):
        got = getattr(ex, name).grad
        inside(got, p.grad, a.grad, name + ".grad")
        assert bool((got[E - 1] == 0).all())          # the expert without tokens


@pytest.mark.parametrize("kw", [{"grouped": False}, {"ep_size": 2}])
def test_dropless_refuses(kw):
    class _Group:
        nranks = kw.get("ep_size", 1)
    with pytest.raises(ValueError, match="dispatch='dropless' needs ep_size == 1 .* grouped=True"):
        MoELayer(H, I, E, k=K, dispatch="dropless", grouped=kw.get("grouped", True),
                 ep_group=_Group() if "ep_size" in kw else None)
