"""Kernel contract on a machine without a GPU: the predicates that decide
whether a HIP kernel may take a call, the dispatch around them (with a
stub in place of the extension), the torch path's cross-entropy rules,
and self-tests of the comparator the GPU suite relies on.
"""
import pytest
import torch

import paddle_amd as paddle
from paddle_amd import _ext
from paddle_amd.ops import functional as hot

from test_row_kernels_gpu import (BF16, F16, F32, U, ULP32, ce_ref, compare,
                                  dropout_add_ref, embedding_grad_ref,
                                  gelu_ref, ln_ref, measured, rms_ref,
                                  rope_ref, rope_tables, swiglu_ref)

CPU = "cpu"


def rn(shape, seed, dtype=F32, mean=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) + mean).to(dtype)


def leaf(t):
    return t.detach().clone().requires_grad_(True)


# ---------------------------------------------------------------------------
# truth table
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF16, F32])
def test_predicates_accept_the_contract(dtype):
    x, w, b = rn((4, 64), 0, dtype), rn((64,), 1, dtype), rn((64,), 2, dtype)
    assert hot._norm_native_ok(x, w, b)
    assert hot._norm_native_ok(x, w)
    assert hot._norm_native_ok(x, w, residual=rn((4, 64), 3, dtype))
    assert hot._bias_gelu_native_ok(x, b) and hot._bias_gelu_native_ok(x)
    assert hot._swiglu_native_ok(x)
    assert hot._dropout_add_native_ok(x, x) and hot._dropout_add_native_ok(x)
    assert hot._embedding_native_ok(x, torch.zeros(3, dtype=torch.long))
    assert hot._embedding_native_ok(x, torch.zeros(3, dtype=torch.int32))
    assert hot._ce_native_ok(x, torch.zeros(4, dtype=torch.long))
    assert hot._ce_native_ok(rn((4, 5), 4, dtype), torch.zeros(4, dtype=torch.long))
    assert hot._reduce_native_ok(x) and hot._reduce_native_ok(rn((5,), 5, dtype))
    q = rn((2, 3, 5, 8), 6, dtype)
    c, s = rope_tables(8, 8, dev=CPU)
    assert hot._rope_native_ok(q, c, s, 5)
    m = rn((16,), 7)
    assert hot._adamw_native_ok(m, rn((16,), 8, dtype), rn((16,), 9, dtype), m, m)
    assert hot._adamw_native_ok(m, None, rn((16,), 9, dtype), m, m)
    # a per-column parameter of another float dtype is cast, not rejected
    other = F32 if dtype == BF16 else BF16
    assert hot._norm_native_ok(x, w.to(other), b.to(other))
    assert hot._bias_gelu_native_ok(x, b.to(other))
    # the ops make x contiguous themselves
    assert hot._norm_native_ok(rn((64, 4), 10, dtype).t(), w, b)


def test_predicates_reject_fp16():
    x, w = rn((4, 64), 0, F16), rn((64,), 1, F16)
    ids = torch.zeros(4, dtype=torch.long)
    c, s = rope_tables(4, 16, dev=CPU)
    m = rn((16,), 2)
    assert not hot._norm_native_ok(x, w, w)
    assert not hot._norm_native_ok(x, w, residual=x)
    assert not hot._bias_gelu_native_ok(x, w)
    assert not hot._swiglu_native_ok(x)
    assert not hot._rope_native_ok(rn((1, 4, 2, 16), 3, F16), c, s, 0)
    assert not hot._dropout_add_native_ok(x, x)
    assert not hot._embedding_native_ok(x, ids)
    assert not hot._ce_native_ok(x, ids)
    assert not hot._reduce_native_ok(x)
    assert not hot._adamw_native_ok(m, None, rn((16,), 4, F16), m, m)
    assert not hot._adamw_native_ok(m, rn((16,), 5, F16), m, m, m)


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_predicates_reject_mixed_full_size_operands(dtype):
    other = F32 if dtype == BF16 else BF16
    x, w = rn((4, 64), 0, dtype), rn((64,), 1, dtype)
    assert not hot._norm_native_ok(x, w, residual=x.to(other))
    assert not hot._dropout_add_native_ok(x, x.to(other))
    assert not hot._norm_native_ok(x, w, residual=rn((2, 64), 2, dtype))
    assert not hot._norm_native_ok(x, rn((32,), 3, dtype))
    assert not hot._bias_gelu_native_ok(x, rn((8,), 4, dtype))
    assert not hot._norm_native_ok(x, torch.ones(64, dtype=torch.long))


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("d", [1, 7, 100])
def test_predicates_reject_odd_last_dim(d, dtype):
    x, w = rn((3, d), 0, dtype), rn((d,), 1, dtype)
    assert not hot._norm_native_ok(x, w, w)
    assert not hot._bias_gelu_native_ok(x, w)
    assert not hot._swiglu_native_ok(rn((3, 2 * d), 2, dtype))
    assert not hot._embedding_native_ok(x, torch.zeros(2, dtype=torch.long))
    assert hot._reduce_native_ok(x)           # scalar tails: any size
    assert hot._ce_native_ok(x, torch.zeros(3, dtype=torch.long))


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("numel", [1, 7, 1001])
def test_predicates_reject_dropout_add_numel(numel, dtype):
    assert not hot._dropout_add_native_ok(rn((numel,), 0, dtype))
    assert not hot._dropout_add_native_ok(rn((numel,), 0, dtype), rn((numel,), 1, dtype))


def test_predicates_reject_rope_shapes_and_tables():
    c, s = rope_tables(8, 8, dev=CPU)
    q = rn((2, 3, 5, 8), 0, BF16)
    assert not hot._rope_native_ok(q, c, s, 6)                     # 3 + 6 > 8 rows
    assert not hot._rope_native_ok(q, c[:, :2], s[:, :2], 0)       # wrong width
    assert not hot._rope_native_ok(q, c.double(), s.double(), 0)   # tables are fp32
    c4, s4 = rope_tables(8, 4, dev=CPU)
    assert not hot._rope_native_ok(rn((2, 3, 5, 4), 1, BF16), c4, s4, 0)   # dh/2 % 4
    assert not hot._rope_native_ok(rn((6, 5, 8), 2, BF16), c, s, 0)        # not 4-D
    # the op hands the tables over as they are: they must be contiguous
    wide_c, wide_s = torch.cat([c, c], 1), torch.cat([s, s], 1)
    assert not hot._rope_native_ok(q, wide_c[:, :4], wide_s[:, :4], 0)


def test_predicates_reject_adamw_states():
    m = rn((16,), 0)
    g = rn((16,), 1, BF16)
    assert not hot._adamw_native_ok(m, None, g, m.to(BF16), m)
    assert not hot._adamw_native_ok(m, None, rn((8,), 2), m, m)
    assert not hot._adamw_native_ok(m, torch.zeros(16, dtype=torch.float64), g, m, m)
    nc = rn((16, 2), 3)[:, 0]
    assert not nc.is_contiguous()
    assert not hot._adamw_native_ok(nc, None, g, m, m)
    assert not hot._adamw_native_ok(m, None, g, m, nc)


# ---------------------------------------------------------------------------
# dispatch with a stub extension
# ---------------------------------------------------------------------------
class _Reached:
    """Every attribute raises: no kernel may be reached."""

    def __getattr__(self, name):
        raise AssertionError(f"kernel reached: {name}")


@pytest.fixture
def no_kernel(monkeypatch):
    monkeypatch.setattr(_ext, "use_native", lambda t: True)
    monkeypatch.setattr(_ext, "get_ext", lambda required=False: _Reached())


def _elem(name, out, r64, E, key, dtype):
    compare(name, out, r64[key], u=U[dtype], atol=4 * E[key] + r64["A_" + key], dtype=dtype)


def _red(name, out, r64, key, dtype):
    compare(name, out, r64[key], u=U[dtype], atol=r64["A_" + key], dtype=dtype)


REJECTED_ROWS = [(F16, 64), (BF16, 1), (BF16, 7), (BF16, 100), (F32, 1), (F32, 7), (F32, 100)]


@pytest.mark.parametrize("dtype,d", REJECTED_ROWS)
def test_rejected_inputs_take_the_torch_path_norms(no_kernel, dtype, d):
    x, w, b, dy = rn((5, d), 0, dtype), rn((d,), 1, dtype, 1.0), rn((d,), 2, dtype), rn((5, d), 3, dtype)
    xl, wl, bl = leaf(x), leaf(w), leaf(b)
    y = hot.layer_norm(xl, wl, bl, 1e-5)
    y.backward(dy)
    r64, E = measured(ln_ref, x, w, b, dy)
    _elem("ln y", y, r64, E, "y", dtype)
    _elem("ln dx", xl.grad, r64, E, "dx", dtype)
    _red("ln dw", wl.grad, r64, "dw", dtype)
    _red("ln db", bl.grad, r64, "db", dtype)

    xl, wl = leaf(x), leaf(w)
    y = hot.rms_norm(xl, wl, 1e-6)
    y.backward(dy)
    q64, Eq = measured(rms_ref, x, w, dy)
    _elem("rms y", y, q64, Eq, "y", dtype)
    _elem("rms dx", xl.grad, q64, Eq, "dx", dtype)
    _red("rms dw", wl.grad, q64, "dw", dtype)

    res, dxr = rn((5, d), 4, dtype), rn((5, d), 5, dtype)
    xl, rl, wl = leaf(x), leaf(res), leaf(w)
    y, xr = hot.fused_rms_norm(xl, wl, residual=rl)
    torch.autograd.backward([y, xr], [dy, dxr])
    fn = lambda x_, w_, dy_, r_, dxr_: rms_ref(x_, w_, dy_, r_, dxr_, res_dtype=dtype, stat_from_stored=True)  # noqa: E731
    f64, Ef = measured(fn, x, w, dy, res, dxr)
    _elem("fused res_out", xr, f64, Ef, "res_out", dtype)
    _elem("fused y", y, f64, Ef, "y", dtype)
    extra = U[dtype] * f64["dx_norm"].abs()
    compare("fused dx", xl.grad, f64["dx"], u=U[dtype], atol=4 * Ef["dx"] + f64["A_dx"] + extra, dtype=dtype)
    compare("fused dres", rl.grad, f64["dx"], u=U[dtype], atol=4 * Ef["dx"] + f64["A_dx"] + extra, dtype=dtype)


@pytest.mark.parametrize("dtype,d", REJECTED_ROWS)
def test_rejected_inputs_take_the_torch_path_elementwise(no_kernel, dtype, d):
    x, b, dy = rn((5, d), 10, dtype), rn((d,), 11, dtype), rn((5, d), 12, dtype)
    xl, bl = leaf(x), leaf(b)
    y = hot.bias_gelu(xl, bl)
    y.backward(dy)
    r64, E = measured(gelu_ref, x, b, dy)
    _elem("gelu y", y, r64, E, "y", dtype)
    _elem("gelu dx", xl.grad, r64, E, "dx", dtype)
    # db is the column sum of dx as stored in T
    dxa = r64["dx"].abs()
    compare("gelu db", bl.grad, r64["dx"].sum(0), u=U[dtype],
            atol=(5 * ULP32 * dxa + U[dtype] * dxa + 4 * E["dx"] + r64["A_dx"]).sum(0), dtype=dtype)

    x2, dy2 = rn((5, 2 * d), 13, dtype), rn((5, d), 14, dtype)
    xl = leaf(x2)
    y = hot.swiglu(xl)
    y.backward(dy2)
    s64, Es = measured(swiglu_ref, x2, dy2)
    _elem("swiglu y", y, s64, Es, "y", dtype)
    _elem("swiglu dg", xl.grad[..., :d], s64, Es, "dg", dtype)
    _elem("swiglu du", xl.grad[..., d:], s64, Es, "du", dtype)

    table = rn((9, d), 15, dtype)
    ids = torch.tensor([[0, 8, 3], [3, 3, 1]])
    tl = leaf(table)
    out = hot.embedding(ids, tl, padding_idx=1)
    dout = rn((2, 3, d), 16, dtype)
    out.backward(dout)
    ref = table[ids].clone()
    ref[ids == 1] = 0
    assert torch.equal(out, ref)
    g = embedding_grad_ref(dout.double(), ids, 9, 1)
    _red("embedding dtable", tl.grad, g, "dtable", dtype)


@pytest.mark.parametrize("dtype,numel", [(F16, 64), (BF16, 1), (BF16, 7), (BF16, 1001),
                                         (F32, 1), (F32, 7), (F32, 1001)])
def test_rejected_inputs_take_the_torch_path_dropout_add_l2(no_kernel, dtype, numel):
    x, r, dy = rn((numel,), 20, dtype), rn((numel,), 21, dtype), rn((numel,), 22, dtype)
    xl, rl = leaf(x), leaf(r)
    y = hot.dropout_add(xl, rl, 0.0, True)
    y.backward(dy)
    compare("dropout_add p=0", y, x.double() + r.double(), u=U[dtype] + ULP32, dtype=dtype)
    assert torch.equal(xl.grad, dy) and torch.equal(rl.grad, dy)
    if dtype == F16:      # bf16/fp32 of any size are inside the reduction contract
        ssq = x.double().square().sum()
        compare("l2", hot.l2_norm_squared(x), ssq.reshape(1), atol=float((numel + 8) * ULP32 * ssq))


def test_rejected_inputs_take_the_torch_path_rope_ce_adamw(no_kernel):
    # rope: fp16, and dh/2 not a multiple of 4
    for dtype, dh in [(F16, 16), (BF16, 4), (F32, 12)]:
        q, dy = rn((2, 3, 5, dh), 30, dtype), rn((2, 3, 5, dh), 31, dtype)
        c, s = rope_tables(8, dh, dev=CPU)
        ql = leaf(q)
        y = hot.fused_rotary_position_embedding(ql, sin=torch.cat([s, s], -1),
                                                cos=torch.cat([c, c], -1), pos_offset=5)
        y.backward(dy)
        f = rope_ref(q.double(), c, s, 5)
        bwd = rope_ref(dy.double(), c, s, 5, conj=True)
        compare("rope y", y, f["y"], u=U[dtype], atol=f["A_y"], dtype=dtype)
        compare("rope dx", ql.grad, bwd["y"], u=U[dtype], atol=bwd["A_y"], dtype=dtype)
    # cross entropy: fp16 logits
    lg, lab, dl = rn((7, 40), 32, F16), torch.arange(7) % 40, rn((7,), 33)
    ll = leaf(lg)
    loss = hot.softmax_cross_entropy(ll, lab)
    loss.backward(dl)
    c64, Ec = measured(ce_ref, lg, lab, dl)
    compare("ce loss", loss, c64["loss"], atol=4 * Ec["loss"] + c64["A_loss"], dtype=F32)
    _elem("ce dlogits", ll.grad, c64, Ec, "dlogits", F16)
    # adamw: an fp16 grad, and an fp16 param_out, stay on the torch path
    for grad, pout in [(rn((16,), 35, F16), None), (rn((16,), 35), torch.zeros(16, dtype=F16))]:
        master, m, v = rn((16,), 34), torch.zeros(16), torch.zeros(16)
        g64 = grad.double()
        ref = master.double() - 1e-2 * g64 / (g64.abs() + 1e-8)   # step 1: mhat = g, vhat = g^2
        hot.fused_adamw_step(master, pout, grad, m, v, 1e-2, 0.9, 0.999, 1e-8, 0.0, 1)
        compare("adamw master", master, ref, atol=2.0 ** -22 * (ref.abs() + 1e-2))
        if pout is not None:
            compare("adamw param_out", pout, ref, u=U[F16], atol=2.0 ** -22 * (ref.abs() + 1e-2), dtype=F16)


def test_short_rope_table_raises_before_the_extension(no_kernel):
    q = rn((1, 4, 2, 16), 40, BF16)
    c, s = rope_tables(8, 16, dev=CPU)
    with pytest.raises(ValueError):
        hot.fused_rotary_position_embedding(q, sin=torch.cat([s, s], -1),
                                            cos=torch.cat([c, c], -1), pos_offset=5)


# ---- recording stub: the kernels' arithmetic in torch, arguments logged -----
class _Recorder:
    def __init__(self):
        self.calls = []

    def _log(self, name, *tensors):
        self.calls.append((name, [t.dtype for t in tensors if t is not None
                                  and t.is_floating_point()]))

    def layer_norm_fwd(self, x, w, b, eps):
        self._log("layer_norm_fwd", x, w, b)
        assert x.is_contiguous() and w.is_contiguous()
        r = ln_ref(x.float(), w.float(), None if b is None else b.float(), x.float(), eps)
        return r["y"].to(x.dtype), r["mean"], r["rstd"]

    def layer_norm_bwd(self, dy, x, w, mean, rstd, has_bias):
        self._log("layer_norm_bwd", dy, x, w)
        assert mean.dtype == rstd.dtype == F32
        r = ln_ref(x.float(), w.float(), None, dy.float())
        return r["dx"].to(x.dtype), r["dw"], r["db"]

    def rms_norm_fwd(self, x, res, w, eps):
        self._log("rms_norm_fwd", x, res, w)
        r = rms_ref(x.float(), w.float(), x.float(), None if res is None else res.float(), eps=eps)
        rstd = torch.rsqrt(r["res_out"].square().mean(-1) + eps).reshape(-1)
        if res is None:
            return r["y"].to(x.dtype), rstd
        return r["y"].to(x.dtype), rstd, r["res_out"].to(x.dtype)

    def rms_norm_bwd(self, dy, x, w, rstd):
        self._log("rms_norm_bwd", dy, x, w)
        r = rms_ref(x.float(), w.float(), dy.float())
        return r["dx"].to(x.dtype), r["dw"]

    def bias_gelu_fwd(self, x, bias):
        self._log("bias_gelu_fwd", x, bias)
        return gelu_ref(x.float(), None if bias is None else bias.float(), x.float())["y"].to(x.dtype)

    def bias_gelu_bwd(self, dy, x, bias):
        self._log("bias_gelu_bwd", dy, x, bias)
        return gelu_ref(x.float(), None if bias is None else bias.float(), dy.float())["dx"].to(x.dtype)

    def colsum(self, x):
        self._log("colsum", x)
        return x.float().reshape(-1, x.shape[-1]).sum(0)


@pytest.fixture
def recorder(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(_ext, "use_native", lambda t: True)
    monkeypatch.setattr(_ext, "get_ext", lambda required=False: rec)
    return rec


def _one_dtype_per_call(rec, expect):
    assert rec.calls, "the kernel path was not taken"
    for name, dts in rec.calls:
        assert set(dts) == {expect}, f"{name} received {dts}"


def test_mixed_small_operands_are_cast_for_the_kernel(recorder):
    x, dy = rn((6, 64), 50, BF16), rn((6, 64), 51, BF16)
    w, b = rn((64,), 52, F32, 1.0), rn((64,), 53, F32)
    xl, wl, bl = leaf(x), leaf(w), leaf(b)
    y = hot.layer_norm(xl, wl, bl, 1e-5)
    y.backward(dy)
    assert y.dtype == BF16 and xl.grad.dtype == BF16
    assert wl.grad.dtype == F32 and bl.grad.dtype == F32
    r64, E = measured(ln_ref, x, w.to(BF16), b.to(BF16), dy)
    _elem("ln y", y, r64, E, "y", BF16)
    compare("ln dw", wl.grad, r64["dw"], atol=r64["A_dw"], dtype=F32)

    xl, wl = leaf(x), leaf(w)
    y = hot.rms_norm(xl, wl, 1e-6)
    y.backward(dy)
    assert y.dtype == BF16 and wl.grad.dtype == F32

    xl, rl, wl = leaf(x), leaf(dy), leaf(w)
    y, xr = hot.fused_rms_norm(xl, wl, residual=rl)
    (y.float().sum() + xr.float().sum()).backward()
    assert y.dtype == xr.dtype == BF16 and wl.grad.dtype == F32

    xl, bl = leaf(x), leaf(b)
    y = hot.bias_gelu(xl, bl)
    y.backward(dy)
    assert y.dtype == BF16 and bl.grad.dtype == F32
    g64, Eg = measured(gelu_ref, x, b.to(BF16), dy)
    _elem("gelu y", y, g64, Eg, "y", BF16)
    _one_dtype_per_call(recorder, BF16)
    names = {n for n, _ in recorder.calls}
    assert {"layer_norm_fwd", "layer_norm_bwd", "rms_norm_fwd", "rms_norm_bwd",
            "bias_gelu_fwd", "bias_gelu_bwd", "colsum"} <= names


def test_mixed_full_size_residual_takes_the_torch_path(no_kernel):
    x, res, w = rn((6, 64), 54, BF16), rn((6, 64), 55, F32), rn((64,), 56, BF16, 1.0)
    y, xr = hot.fused_rms_norm(x, w, residual=res)
    ref = x.double() + res.double()
    assert xr.dtype == F32      # what torch's promotion gives
    compare("res_out", xr, ref, atol=ULP32 * ref.abs())
    y2 = hot.dropout_add(x, res, 0.0, True)
    assert y2.dtype == F32
    compare("dropout_add", y2, ref, atol=ULP32 * ref.abs())


def test_amp_decorate_o2_layer_norm_reaches_the_kernel_in_one_dtype(recorder):
    paddle.seed(0)
    ln, lin = paddle.nn.LayerNorm(64), paddle.nn.Linear(64, 64)
    ln, lin = paddle.amp.decorate([ln, lin], level="O2", dtype="bfloat16")
    assert ln.weight.dtype == F32 and lin.weight.dtype == BF16     # O2 keeps norms fp32
    x = rn((4, 64), 57, BF16)
    y = ln(lin(x))
    y.float().sum().backward()
    assert y.dtype == BF16
    fwd = [dts for n, dts in recorder.calls if n == "layer_norm_fwd"]
    assert fwd and all(set(d) == {BF16} for d in fwd)
    _one_dtype_per_call(recorder, BF16)
    assert ln.weight.grad.dtype == F32 and ln.bias.grad.dtype == F32


# ---------------------------------------------------------------------------
# torch-path cross entropy rules
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF16, F32])
def test_cross_entropy_out_of_range_labels_and_neg_inf(dtype):
    n, v = 12, 37
    lg = rn((n, v), 60, F32)
    lg[:, 0] = float("-inf")
    lg[:, 30:] = float("-inf")
    lg = lg.to(dtype)
    lab = torch.tensor([1, 29, -100, -1, v, 5, 7, -100, 2, 3, 10 ** 6, 4])
    dl = rn((n,), 61)
    ll = leaf(lg)
    loss = hot.softmax_cross_entropy(ll, lab, ignore_index=-100)
    loss.backward(dl)
    assert torch.isfinite(loss).all() and torch.isfinite(ll.grad).all()
    skip = (lab == -100) | (lab < 0) | (lab >= v)
    assert int(skip.sum()) == 5
    assert bool((loss[skip] == 0).all()) and bool((ll.grad[skip] == 0).all())
    ok = ~skip
    lr = leaf(lg.double())
    ref = torch.nn.functional.cross_entropy(lr[ok], lab[ok], reduction="none")
    ref.backward(dl[ok].double())
    c64, E = measured(ce_ref, lg, lab, dl)
    compare("loss vs torch", loss[ok], ref, atol=4 * E["loss"] + c64["A_loss"][ok], dtype=F32)
    compare("dlogits vs torch", ll.grad[ok], lr.grad[ok], u=U[dtype],
            atol=4 * E["dlogits"] + c64["A_dlogits"][ok], dtype=dtype)
    compare("loss vs ce_ref", loss, c64["loss"], atol=4 * E["loss"] + c64["A_loss"])
    # mean reduction counts what is not ignore_index, as before
    red = hot.softmax_cross_entropy(lg, lab, ignore_index=-100, reduction="sum")
    compare("sum", red, c64["loss"].sum(), atol=float(n * 4 * E["loss"] + c64["A_loss"].sum() + n * ULP32 * c64["loss"].abs().sum()))


# ---------------------------------------------------------------------------
# comparator self-tests: a subtly wrong kernel must not pass
# ---------------------------------------------------------------------------
def _passes(fn):
    try:
        fn()
    except AssertionError:
        return False
    return True


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_comparator_rejects_row_stats_without_the_last_8_columns(dtype):
    x, w, b, dy = rn((5, 2056), 70, dtype), rn((2056,), 71, dtype, 1.0), rn((2056,), 72, dtype), rn((5, 2056), 73, dtype)
    r64, E = measured(ln_ref, x, w, b, dy)
    good = ln_ref(x.float(), w.float(), b.float(), dy.float())
    bad = ln_ref(x.float(), w.float(), b.float(), dy.float(), stat_cols=2048)
    # a right kernel: the fp32 formula, rounded to T
    assert _passes(lambda: _elem("y", good["y"].to(dtype), r64, E, "y", dtype))
    assert _passes(lambda: compare("rstd", good["rstd"], r64["rstd"], atol=4 * E["rstd"] + r64["A_rstd"]))
    # a kernel whose second sweep over D drops the last lane
    assert not _passes(lambda: compare("rstd", bad["rstd"], r64["rstd"], atol=4 * E["rstd"] + r64["A_rstd"]))
    assert not _passes(lambda: compare("mean", bad["mean"], r64["mean"], atol=4 * E["mean"] + r64["A_mean"]))
    if dtype == F32:
        assert not _passes(lambda: _elem("y", bad["y"].to(dtype), r64, E, "y", dtype))


def test_comparator_rejects_shifted_mean_variance_loss():
    """E[x^2] - mu^2 in fp32 at mu = 1000: the defect the shifted moments fix."""
    x, w, b, dy = rn((8, 1024), 74, F32, 1000.0), rn((1024,), 75, F32, 1.0), rn((1024,), 76), rn((8, 1024), 77)
    r64, E = measured(ln_ref, x, w, b, dy)
    mu = x.mean(-1, keepdim=True)
    var = ((x * x).mean(-1, keepdim=True) - mu * mu).clamp(min=0)
    y_old = (x - mu) * torch.rsqrt(var + 1e-5) * w + b
    k = x[:, :1]
    c = x - k
    dmu = c.mean(-1, keepdim=True)
    var_new = ((c * c).mean(-1, keepdim=True) - dmu * dmu).clamp(min=0)
    y_new = (x - (k + dmu)) * torch.rsqrt(var_new + 1e-5) * w + b
    assert _passes(lambda: _elem("y shifted", y_new, r64, E, "y", F32))
    assert not _passes(lambda: _elem("y raw moments", y_old, r64, E, "y", F32))


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_comparator_rejects_rope_mutations(dtype):
    q = rn((2, 3, 5, 8), 78, dtype)
    c, s = rope_tables(9, 8, dev=CPU)
    f = rope_ref(q.double(), c, s, 5)
    ok = lambda t: compare("rope", t.to(dtype), f["y"], u=U[dtype], atol=f["A_y"], dtype=dtype)  # noqa: E731
    assert _passes(lambda: ok(rope_ref(q.float(), c, s, 5)["y"]))
    assert not _passes(lambda: ok(rope_ref(q.float(), c, s, 6)["y"]))               # pos_offset off by one
    assert not _passes(lambda: ok(rope_ref(q.float(), c, s, 4)["y"]))
    assert not _passes(lambda: ok(rope_ref(q.float(), c, s, 5, sin_sign=-1.0)["y"]))  # sin sign
    # the backward is the conjugate rotation, not the forward one
    bwd = rope_ref(q.double(), c, s, 5, conj=True)
    assert not _passes(lambda: compare("rope bwd", rope_ref(q.float(), c, s, 5)["y"].to(dtype),
                                       bwd["y"], u=U[dtype], atol=bwd["A_y"]))


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_comparator_rejects_bias_shifted_by_8_columns(dtype):
    x, b, dy = rn((3, 24), 79, dtype), rn((24,), 80, dtype), rn((3, 24), 81, dtype)
    r64, E = measured(gelu_ref, x, b, dy)
    good = gelu_ref(x.float(), b.float(), dy.float())
    bad = gelu_ref(x.float(), b.float(), dy.float(), col_shift=8)
    for k in ("y", "dx"):
        assert _passes(lambda: _elem(k, good[k].to(dtype), r64, E, k, dtype))
        assert not _passes(lambda: _elem(k, bad[k].to(dtype), r64, E, k, dtype))


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_comparator_rejects_missing_dropout_scale(dtype, p):
    x, r = rn((64,), 82, dtype), rn((64,), 83, dtype)
    mask = (torch.rand(64, generator=torch.Generator().manual_seed(84)) >= p).to(torch.uint8)
    assert 0 < int(mask.sum()) < 64
    ref = dropout_add_ref(x.double(), r.double(), mask, p)
    a = 2.0 ** -22 * (x.double().abs() / (1 - p) + r.double().abs())
    good = dropout_add_ref(x.float(), r.float(), mask, p).to(dtype)
    bad = dropout_add_ref(x.float(), r.float(), mask, p, scaled=False).to(dtype)
    assert _passes(lambda: compare("y", good, ref, u=U[dtype], atol=a, dtype=dtype))
    assert not _passes(lambda: compare("y", bad, ref, u=U[dtype], atol=a, dtype=dtype))
    if p == 0.5:
        assert not torch.equal(bad, good)


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_comparator_rejects_gradient_of_first_duplicate_only(dtype):
    ids = torch.tensor([3, 3, 1, 0])
    dout = rn((4, 8), 85, dtype)
    r = embedding_grad_ref(dout.double(), ids, 5)
    good = embedding_grad_ref(dout.float(), ids, 5)["dtable"].to(dtype)
    bad = embedding_grad_ref(dout.float(), ids, 5, first_only=True)["dtable"].to(dtype)
    assert _passes(lambda: _red("dtable", good, r, "dtable", dtype))
    assert not _passes(lambda: _red("dtable", bad, r, "dtable", dtype))


def test_comparator_rejects_nan_shape_and_dtype():
    ref = torch.ones(4, dtype=torch.float64)
    assert _passes(lambda: compare("ok", torch.ones(4), ref))
    assert not _passes(lambda: compare("nan", torch.tensor([1.0, float("nan"), 1, 1]), ref, atol=1.0))
    assert not _passes(lambda: compare("shape", torch.ones(2, 2), ref))
    assert not _passes(lambda: compare("dtype", torch.ones(4, dtype=BF16), ref, dtype=F32))


# ---------------------------------------------------------------------------
# own GEMM operand contract (gemm_dispatch.own_gemm_ok)
# ---------------------------------------------------------------------------
def test_own_gemm_ok_truth_table():
    from paddle_amd.ops.gemm_dispatch import own_gemm_ok

    def z(*shape, dtype=torch.bfloat16):
        return torch.zeros(*shape, dtype=dtype)

    m, n, k = 16, 24, 64
    # contiguous operands, each layout
    assert own_gemm_ok(z(m, k), z(n, k), "nt")
    assert own_gemm_ok(z(m, k), z(k, n), "nn")
    assert own_gemm_ok(z(k, m), z(k, n), "tn")
    # a row-sliced view keeps 16-byte rows and base: fine
    assert own_gemm_ok(z(m + 8, k)[8:], z(n, k), "nt")
    assert own_gemm_ok(z(m, 2 * k)[:, k:], z(n, k), "nt")
    # sliced with a storage offset that is not a multiple of 16 bytes
    assert not own_gemm_ok(z(m, k + 8)[:, 1:k + 1], z(n, k), "nt")
    assert not own_gemm_ok(z(m, k), z(n, k + 8)[:, 4:k + 4], "nt")
    assert not own_gemm_ok(z(m * k + 1)[1:].view(m, k), z(n, k), "nt")
    # row stride that is not a multiple of 16 bytes, inner stride != 1
    assert not own_gemm_ok(z(m, k + 4)[:, :k], z(n, k), "nt")
    assert not own_gemm_ok(z(m, k), z(k, n + 4)[:, :n], "nn")
    assert not own_gemm_ok(z(k, m).t(), z(n, k), "nt")
    # dtypes
    assert not own_gemm_ok(z(m, k, dtype=torch.float32), z(n, k), "nt")
    assert not own_gemm_ok(z(m, k), z(n, k, dtype=torch.float16), "nt")
    # ranks
    assert not own_gemm_ok(z(k), z(n, k), "nt")
    assert not own_gemm_ok(z(m, k), z(2, n, k), "nt")
    # inner dimensions, K below the kernel's floor, empty, unknown layout
    assert not own_gemm_ok(z(m, k), z(n, k), "nn")
    assert not own_gemm_ok(z(m, 32), z(n, 32), "nt")
    assert not own_gemm_ok(z(0, k), z(n, k), "nt")
    assert not own_gemm_ok(z(m, k), z(n, k), "tt")


def test_linear_with_misaligned_weight_view_takes_the_library_path(no_kernel, monkeypatch):
    from paddle_amd.ops import gemm_dispatch as gd
    # a shape the table would give to the own kernel, on a "native" device
    monkeypatch.setattr(gd, "_native_ok", lambda x: x.dtype == torch.bfloat16)
    monkeypatch.setattr(gd, "use_own", lambda layout, m, n, k: True)
    k, n = 64, 32
    x = rn((4, k), 0, BF16)
    parent = rn((k, n + 8), 1, BF16)
    w = parent[:, 1:n + 1]                     # base 2 bytes off a 16-byte line
    assert hot._own_linear_ok(x, parent[:, :n].contiguous())
    assert not hot._own_linear_ok(x, w)
    assert not hot._own_linear_ok(x[:, 1:], parent[1:, :n].contiguous())
    bias = rn((n,), 2, BF16)
    y = paddle.nn.functional.linear(x, w, bias)    # _Reached: no kernel, no raise
    torch.testing.assert_close(y, torch.addmm(bias, x, w))
