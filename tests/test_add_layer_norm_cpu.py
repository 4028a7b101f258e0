"""add_layer_norm and the paired GPT layers on the CPU, in fp32.

Off the GPU hot.add_layer_norm is literally dropout_add followed by
layer_norm, and _AddLayerNorm composes the same reference formulas; the
paired GPTModel differs from layers chained by hand only in where the
residual gradient is added, and every such sum has two terms (a + b ==
b + a bit for bit).  So everything here is torch.equal.
"""
import torch

import paddle_amd as paddle
from paddle_amd.models import GPTPretrainingCriterion, build_gpt
from paddle_amd.ops import functional as hot


def _rn(shape, seed, mean=0.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) + mean


def _leaf(t):
    return t.detach().clone().requires_grad_(True)


def _run(fn, x, res, w, b, dh, dy):
    xl, rl, wl = _leaf(x), _leaf(res), _leaf(w)
    bl = None if b is None else _leaf(b)
    h, y = fn(xl, rl, wl, bl)
    torch.autograd.backward([h, y], [dh, dy])
    return [h.detach(), y.detach(), xl.grad, rl.grad, wl.grad] + ([] if b is None else [bl.grad])


def _unfused(x, res, w, b):
    h = hot.dropout_add(x, res, 0.0, True)
    return h, hot.layer_norm(h, w, b, 1e-5)


def test_add_layer_norm_function_matches_dropout_add_then_layer_norm():
    for has_bias in (True, False):
        x, res = _rn((2, 5, 24), 0), _rn((2, 5, 24), 1)
        w, b = _rn((24,), 2, 1.0), (_rn((24,), 3) if has_bias else None)
        dh, dy = _rn((2, 5, 24), 4), _rn((2, 5, 24), 5)
        ref = _run(_unfused, x, res, w, b, dh, dy)
        fn = _run(lambda *a: hot._AddLayerNorm.apply(*a, 1e-5), x, res, w, b, dh, dy)
        op = _run(lambda *a: hot.add_layer_norm(*a, 1e-5), x, res, w, b, dh, dy)
        names = ("h", "y", "dx", "dres", "dw", "db")
        for name, r, f, o in zip(names, ref, fn, op):
            assert torch.equal(f, r), f"_AddLayerNorm {name} (bias={has_bias})"
            assert torch.equal(o, r), f"add_layer_norm {name} (bias={has_bias})"


def test_add_layer_norm_unused_outputs():
    x, res, w, b = _rn((3, 16), 10), _rn((3, 16), 11), _rn((16,), 12, 1.0), _rn((16,), 13)
    dy = _rn((3, 16), 14)
    # y alone: no gradient arrives at h
    xl, rl, wl, bl = _leaf(x), _leaf(res), _leaf(w), _leaf(b)
    _, y = hot._AddLayerNorm.apply(xl, rl, wl, bl, 1e-5)
    y.backward(dy)
    xr, wr, br = _leaf(x + res), _leaf(w), _leaf(b)
    hot.layer_norm(xr, wr, br, 1e-5).backward(dy)
    assert torch.equal(xl.grad, xr.grad) and torch.equal(rl.grad, xr.grad)
    assert torch.equal(wl.grad, wr.grad) and torch.equal(bl.grad, br.grad)
    # h alone: the norm's parameters get no gradient
    xl, rl, wl, bl = _leaf(x), _leaf(res), _leaf(w), _leaf(b)
    h, _ = hot._AddLayerNorm.apply(xl, rl, wl, bl, 1e-5)
    h.backward(dy)
    assert torch.equal(xl.grad, dy) and torch.equal(rl.grad, dy)
    assert wl.grad is None and bl.grad is None


def test_add_layer_norm_predicate():
    x, w = torch.zeros(4, 16), torch.ones(16)
    ok = hot._add_ln_native_ok
    assert ok(x, x, w) and ok(x, x, w, w, p=0.1, training=False)
    assert not ok(x, x, w, p=0.1, training=True)
    assert not ok(x, x.double(), w)
    assert not ok(x, torch.zeros(16, 4).t(), w)   # not contiguous
    assert not ok(x, torch.zeros(4, 8), w)
    assert not ok(torch.zeros(4, 12), torch.zeros(4, 12), torch.ones(12))
    assert not ok(x.half(), x.half(), w)


def test_gpt_paired_layers_match_layers_chained_by_hand():
    paddle.seed(3)
    model = build_gpt("gpt3-tiny", max_seq_len=32)
    loss_fn = GPTPretrainingCriterion()
    g = torch.Generator().manual_seed(4)
    ids = torch.randint(0, 1024, (2, 32), generator=g)
    labels = torch.randint(0, 1024, (2, 32), generator=g)

    def by_hand(ids_):
        gpt = model.gpt
        x = gpt.embeddings(ids_)
        for layer in gpt.layers:
            x = layer(x)
        return model.lm_head(gpt.final_norm(x))

    res = []
    for fwd in (model, by_hand):
        for p in model.parameters():
            p.grad = None
        loss = loss_fn(fwd(ids), labels)
        loss.backward()
        res.append((loss.detach().clone(),
                    {n: p.grad.clone() for n, p in model.named_parameters()}))
    (l1, g1), (l0, g0) = res
    assert torch.equal(l1, l0), (float(l1), float(l0))
    assert set(g1) == set(g0) and len(g1) > 0
    for n in g0:
        assert torch.equal(g1[n], g0[n]), n
    # the deferred pair sums to what the plain layer returns
    x = model.gpt.embeddings(ids)
    m, h = model.gpt.layers[0](x, defer_add=True)
    assert torch.equal(m + h, model.gpt.layers[0](x))
