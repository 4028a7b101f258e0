"""transpose_colsum (csrc/kernels/transpose.hip) and the K-contiguous wgrad
built on it: exact transposes, column sums and weight gradients inside the
bounds of tests/transpose_ref.py, the contract, and the autograd Function
against nn.functional.linear's old calls."""
import pytest
import torch

import paddle_amd.nn.functional as F
from paddle_amd import _ext
from paddle_amd.ops import functional as hot
from paddle_amd.ops import gemm_dispatch as gd

from transpose_ref import SHAPES, colsum_bound, wgrad_bound  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [(r, c, False) for r, c in SHAPES] + [(200, 264, True)]
WGRAD_SHAPES = [(256, 64, 128), (520, 136, 72)]


def _x(r, c, sliced=False, seed=0):
    g = torch.Generator().manual_seed(seed)
    if sliced:   # ld != C, storage offset != 0
        return torch.randn(r, 3 * c, generator=g).to(torch.bfloat16).cuda()[:, c:2 * c]
    return torch.randn(r, c, generator=g).to(torch.bfloat16).cuda()


@pytest.mark.parametrize("r,c,sliced", CASES)
def test_transpose_exact(r, c, sliced):
    x = _x(r, c, sliced)
    assert gd.transpose_ok(x)
    assert x.is_contiguous() != sliced
    out = gd.transpose_colsum(x)
    assert out.shape == (c, r) and out.is_contiguous()
    assert torch.equal(out, x.t().contiguous())


@pytest.mark.parametrize("r,c,sliced", CASES)
def test_colsum_bound_and_determinism(r, c, sliced):
    x = _x(r, c, sliced)
    out, sums = gd.transpose_colsum(x, True)
    out2, sums2 = gd.transpose_colsum(x, True)
    assert sums.dtype == torch.float32 and sums.shape == (c,)
    assert torch.equal(sums, sums2) and torch.equal(out, out2)
    assert torch.equal(out, gd.transpose_colsum(x))
    ref, bound = colsum_bound(x.cpu())
    for got in (sums, sums.to(torch.bfloat16)):
        err = (got.cpu().double() - ref).abs()
        print(f"colsum [{r},{c}] {got.dtype} worst err/bound {float((err / bound).max()):.3f}")
        assert (err <= bound).all()


def test_contract_raises_and_predicate_false():
    C = _ext.get_ext()
    good = _x(16, 16)
    bad = {
        "rows": _x(12, 16),
        "columns": _x(16, 12),
        "bfloat16": good.float(),
        "inner stride": _x(16, 16).t(),
        "GPU": good.cpu(),
    }
    assert gd.transpose_ok(good)
    for word, t in bad.items():
        assert not gd.transpose_ok(t), word
        with pytest.raises(RuntimeError, match=r"transpose_colsum: x .*" + word):
            C.transpose_colsum(t, True)


@pytest.mark.parametrize("form", ["xt", "xt_dyt"])
@pytest.mark.parametrize("t,n_in,n_out", WGRAD_SHAPES)
def test_wgrad_forms_bound(t, n_in, n_out, form):
    x, dy = _x(t, n_in, seed=1), _x(t, n_out, seed=2)
    assert hot._wgrad_form(x, dy) == "tn"      # below the size gate
    dw, db = hot._wgrad(x, dy, want_db=True, form=form)
    ref, bound = wgrad_bound(x.cpu(), dy.cpu())
    err = (dw.cpu().double() - ref).abs()
    print(f"wgrad {form} T{t} in{n_in} out{n_out} worst err/bound "
          f"{float((err / bound).max()):.3f}")
    assert dw.shape == (n_in, n_out) and (err <= bound).all()
    if form == "xt_dyt":
        bref, bbound = colsum_bound(dy.cpu())
        assert db.dtype == dy.dtype
        assert ((db.cpu().double() - bref).abs() <= bbound).all()
        assert torch.equal(hot._wgrad(x, dy, form=form), dw)
    else:
        assert db is None


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("t,n_in,n_out", WGRAD_SHAPES)
def test_autograd_function_against_old_path(t, n_in, n_out, bias):
    g = torch.Generator().manual_seed(3)
    x0 = torch.randn(2, t // 2, n_in, generator=g).to(torch.bfloat16).cuda()
    w0 = (torch.randn(n_in, n_out, generator=g) * 0.05).to(torch.bfloat16).cuda()
    b0 = torch.randn(n_out, generator=g).to(torch.bfloat16).cuda() if bias else None
    dy = torch.randn(2, t // 2, n_out, generator=g).to(torch.bfloat16).cuda()

    def run(fn):
        ts = [v.clone().requires_grad_() if v is not None else None for v in (x0, w0, b0)]
        y = fn(*ts)
        y.backward(dy)
        return [y.detach()] + [v.grad if v is not None else None for v in ts]

    assert not hot._lt_linear_ok(x0, w0.clone().requires_grad_(), b0)
    y_old, dx_old, dw_old, db_old = run(F.linear)
    y, dx, dw, db = run(lambda a, b, c: hot.linear_lt(a, b, c, form="xt_dyt"))
    assert torch.equal(y, y_old)
    assert torch.equal(dx, dx_old)
    x2, dy2 = x0.reshape(-1, n_in).cpu(), dy.reshape(-1, n_out).cpu()
    ref, bound = wgrad_bound(x2, dy2)
    assert ((dw.cpu().double() - ref).abs() <= bound).all()
    assert ((dw_old.cpu().double() - ref).abs() <= bound).all()
    if bias:
        bref, bbound = colsum_bound(dy2)
        assert ((db.cpu().double() - bref).abs() <= bbound).all()
    else:
        assert db is None and db_old is None


def test_tiny_gpt_trains_under_stage3_with_gate_forced(monkeypatch):
    import paddle_amd as paddle
    from paddle_amd.distributed.fleet.sharding import GroupShardedStage3, ShardedAdamW
    from paddle_amd.models import GPTPretrainingCriterion, build_gpt

    calls = []
    real = gd.transpose_colsum

    def counted(x, want_sums=False):
        calls.append((tuple(x.shape), want_sums))
        return real(x, want_sums)

    def step(forced):
        if forced:
            monkeypatch.setattr(hot, "_WGRAD_KC_MIN_T", 8)
            monkeypatch.setattr(hot, "_WGRAD_KC_DIMS", (8, 1 << 30))
            monkeypatch.setattr(gd, "transpose_colsum", counted)
        paddle.set_device("gpu:0")
        paddle.seed(0)
        model = build_gpt("gpt3-tiny").to(device="cuda:0", dtype=torch.bfloat16)
        wrapped = GroupShardedStage3(model)
        opt = ShardedAdamW(wrapped, learning_rate=1e-3)
        ids = torch.randint(0, 1024, (2, 128), device="cuda:0",
                            generator=torch.Generator("cuda:0").manual_seed(5))
        loss = GPTPretrainingCriterion()(wrapped(ids), ids)
        loss.backward()
        opt.step()
        opt.clear_grad()
        with torch.no_grad():
            after = GPTPretrainingCriterion()(wrapped(ids), ids)
        torch.cuda.synchronize()
        return float(loss), float(after)

    loss_old, after_old = step(False)
    assert not calls
    loss_new, after_new = step(True)
    # every linear went through the transposes: per layer qkv, proj and fc2
    # transpose x and dy (with sums: they have a bias), fc1 only x; the head
    # (no bias, in < out) only x
    print(f"{len(calls)} transposes, {sum(s for _, s in calls)} with sums; "
          f"loss {loss_old} -> {after_old} (old), {loss_new} -> {after_new} (forced)")
    assert len(calls) == 2 * 7 + 1 and sum(s for _, s in calls) == 2 * 3
    assert loss_new == loss_old          # the forward is the same calls
    assert after_new == after_new and after_new < loss_new
    assert abs(after_new - after_old) <= 0.05 * abs(loss_old - after_old) + 2.0 ** -7 * abs(after_old)
