"""FlashMask without a GPU: the lowering of startend_row_indices and of
window_size, the CPU fallback of flashmask_attention, and the bounds of
flashmask_ref.py against a torch emulation of the tile walk of
csrc/kernels/flashmask.hip: they accept the design and reject the mistakes
the walk could make.
"""
import pytest
import torch

from paddle_amd.ops import functional as hot
from flashmask_ref import MISTAKES, OUTPUTS, S, case, dense_mask, emulate, indices, worst

FORMS = ["docs", "hole", "bidir_docs", "dead"]     # (causal, C) = (T,1) (T,2) (F,2) (F,4)


@pytest.mark.parametrize("name", FORMS)
def test_lowering_of_the_four_forms(name):
    idx, causal = indices(name)
    gone = hot._flashmask_dense(idx, S, causal)
    if causal:
        gone = gone | (torch.arange(S)[None, :] > torch.arange(S)[:, None])
    assert torch.equal(gone, dense_mask(idx, S, causal))
    with pytest.raises(ValueError):
        hot._flashmask_dense(idx[..., :1].expand(-1, -1, -1, 3), S, causal)


@pytest.mark.parametrize("causal", [True, False])
def test_lowering_of_window_size(causal):
    left, right = 5, 3
    idx = hot._flashmask_window((left, right), 40, causal, "cpu")
    row, col = torch.arange(40)[:, None], torch.arange(40)[None, :]
    want = (row > col + left) | ((col > row) if causal else (row < col - right))
    assert torch.equal(dense_mask(idx, 40, causal)[0, 0], want)
    assert torch.equal(hot._flashmask_window(4, 40, False, "cpu"),
                       hot._flashmask_window((4, 4), 40, False, "cpu"))
    q = torch.zeros(1, 40, 1, 64)
    with pytest.raises(ValueError):
        hot.flashmask_attention(q, q, q, idx, causal=causal, window_size=4)


@pytest.mark.parametrize("name", ["docs", "dead"])
def test_cpu_fallback(name):
    c = case(name, 64)
    q, k, v = (c[n].transpose(1, 2).clone().requires_grad_() for n in ("q", "k", "v"))
    o, lse = hot.flashmask_attention(q, k, v, c["idx"], causal=c["causal"],
                                     return_softmax_lse=True)
    o.backward(c["do"].transpose(1, 2))
    add = torch.zeros(c["gone"].shape).masked_fill(c["gone"], float("-inf"))
    o_ref, _ = hot._sdpa_ref(c["q"], c["k"], c["v"], c["scale"], False, add)
    live = ~c["dead"][0, 0]
    assert torch.equal(o.transpose(1, 2)[:, :, live], o_ref[:, :, live])
    assert bool(c["dead"].any()) == (name == "dead")
    assert bool((o.transpose(1, 2)[:, :, ~live] == 0).all())
    assert bool((q.grad.transpose(1, 2)[:, :, ~live] == 0).all())
    assert all(bool(torch.isfinite(t.grad).all()) for t in (q, k, v))
    assert torch.equal(hot.flashmask_attention(q, k, v, causal=True),
                       hot.flash_attention(q, k, v, causal=True)[0])


@pytest.mark.parametrize("name", ["prefix_window", "hole", "dead"])
def test_bounds_accept_the_walk(name):
    c = case(name)
    got, _ = emulate(c)
    w = {n: worst(c, n, got[n]) for n in OUTPUTS}
    assert all(x <= 1.0 for x in w.values()), w


# the case on which each mistake must act
PLANTED = {"stale_buffer": ("prefix_window",), "skip_min_lo": ("prefix_window",),
           "hi_inclusive": ("hole", "dead"), "second_range_ignored": ("dead",),
           "dead_row_p": ("dead",)}


@pytest.mark.parametrize("mistake", MISTAKES)
def test_bounds_reject(mistake):
    for name in PLANTED[mistake]:
        c = case(name)
        got, applied = emulate(c, mistake)
        assert applied, (mistake, name)
        assert max(worst(c, n, got[n]) for n in OUTPUTS) > 1.0, (mistake, name)
