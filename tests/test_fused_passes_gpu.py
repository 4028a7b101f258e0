"""Fused memory passes against the kernel pairs they replace.

  add + LayerNorm forward   == dropout_add_fwd(p=0) then layer_norm_fwd   (bit-equal)
  one-pass LayerNorm bwd    == ln_bwd_dx (+ tensor add of dres)           (dx bit-equal)
                               dw / db within ln_ref's A_dw / A_db
  bias_gelu bwd with db     == bias_gelu_bwd                              (dx bit-equal)
                               db within the bound of _run_bias_gelu
  fa_bwd delta              vs fp64 row sum, D * 2^-24 * sum|dO*O|
                               (bf16 products are exact in fp32)

Bounds and references come from test_row_kernels_gpu; nothing here adds a
tolerance of its own.  Shapes: one lane, one row, a second / fourth column
strip, more rows than the row-block cap G (grid-stride + partial blocks),
and one shape per op that must take the two-kernel fallback.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from paddle_amd import _ext  # noqa: E402
from paddle_amd.ops import functional as hot  # noqa: E402
from test_row_kernels_gpu import (BF16, DEV, F32, U, ULP32, _leaf, compare,  # noqa: E402
                                  gelu_ref, ln_ref, measured, randn)

G = 1024   # row-block cap of the one-pass LN backward (asserted below)
LN_SHAPES = [(1, 8), (3, 8), (70, 4104), (5, 8192), (2 * G + 3, 64), (3, 8200)]


@pytest.fixture(scope="module")
def C():
    ext = _ext.get_ext(required=True)
    assert ext.ln_bwd_grid_cap() == G
    return ext


def _ln_inputs(n, d, dtype, has_bias, seed):
    x = randn((n, d), seed, dtype)
    w = randn((d,), seed + 1, dtype, mean=1.0)
    b = randn((d,), seed + 2, dtype) if has_bias else None
    return x, w, b


@pytest.mark.parametrize("has_bias", [True, False])
@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("shape", LN_SHAPES)
def test_add_layer_norm_fwd(C, shape, dtype, has_bias):
    n, d = shape
    assert C.ln_fused_ok(d) == (d <= 8192), "8200 must take the two-kernel path"
    x, w, b = _ln_inputs(n, d, dtype, has_bias, 200)
    res = randn((n, d), 203, dtype)
    h, y, mean, rstd = C.add_layer_norm_fwd(x, res, w, b, 1e-5)
    (h0,) = C.dropout_add_fwd(x, res, 0.0, 0, 0)
    y0, mean0, rstd0 = C.layer_norm_fwd(h0, w, b, 1e-5)
    torch.cuda.synchronize()
    assert h.dtype == dtype and y.dtype == dtype
    assert torch.equal(h, h0), "h"
    assert torch.equal(mean, mean0), "mean"
    assert torch.equal(rstd, rstd0), "rstd"
    assert torch.equal(y, y0), "y"


@pytest.mark.parametrize("with_dres", [True, False])
@pytest.mark.parametrize("has_bias", [True, False])
@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("shape", LN_SHAPES)
def test_layer_norm_bwd_one_pass(C, shape, dtype, has_bias, with_dres):
    n, d = shape
    x, w, b = _ln_inputs(n, d, dtype, has_bias, 210)
    dy = randn((n, d), 213, dtype)
    dres = randn((n, d), 214, dtype) if with_dres else None
    _, mean, rstd = C.layer_norm_fwd(x, w, b, 1e-5)
    dx, dw, db = C.layer_norm_bwd(dy, x, w, mean, rstd, has_bias, dres)
    dx0, dw0, db0 = C.layer_norm_bwd(dy, x, w, mean, rstd, has_bias, None, False)
    if with_dres:
        dx0 = dx0 + dres
    torch.cuda.synchronize()
    tag = f"ln_bwd[{n}x{d},{dtype},b={has_bias},dres={with_dres}]"
    nbad = int((dx != dx0).sum())
    print(f"[eq] {tag}: dx differs in {nbad} of {dx.numel()} elements")
    assert dx.dtype == dtype and torch.equal(dx, dx0), tag + " dx"
    r64 = ln_ref(x.double(), w.double(), None if b is None else b.double(), dy.double())
    compare(tag + " dw", dw, r64["dw"], atol=r64["A_dw"], dtype=F32)
    compare(tag + " db", db, r64["db"], atol=r64["A_db"], dtype=F32)
    compare(tag + " dw (two-kernel)", dw0, r64["dw"], atol=r64["A_dw"], dtype=F32)
    compare(tag + " db (two-kernel)", db0, r64["db"], atol=r64["A_db"], dtype=F32)


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_add_layer_norm_op_matches_unfused_ops(C, dtype):
    """hot.add_layer_norm, both outputs used, against dropout_add followed
    by layer_norm: the same kernels' values, with autograd's add replaced by
    the dres input."""
    n, d = 70, 4104
    x, w, b = _ln_inputs(n, d, dtype, True, 220)
    res, dh, dy = randn((n, d), 223, dtype), randn((n, d), 224, dtype), randn((n, d), 225, dtype)
    assert hot._add_ln_native_ok(x, res, w, b)
    assert not hot._add_ln_native_ok(x, res, w, b, p=0.1, training=True)
    assert not hot._add_ln_native_ok(x, res.double(), w, b)
    got, ref = [], []
    for fused, out in ((True, got), (False, ref)):
        xl, rl, wl, bl = _leaf(x), _leaf(res), _leaf(w), _leaf(b)
        if fused:
            h, y = hot.add_layer_norm(xl, rl, wl, bl, 1e-5)
        else:
            h = hot.dropout_add(xl, rl, 0.0, True)
            y = hot.layer_norm(h, wl, bl, 1e-5)
        torch.autograd.backward([h, y], [dh, dy])
        out += [h.detach(), y.detach(), xl.grad, rl.grad, wl.grad, bl.grad]
    torch.cuda.synchronize()
    for name, a, r in zip(("h", "y", "dx", "dres", "dw", "db"), got, ref):
        assert torch.equal(a, r), name
    # y alone used: no dres reaches the kernel
    xl, rl = _leaf(x), _leaf(res)
    _, y = hot.add_layer_norm(xl, rl, w, b, 1e-5)
    y.backward(dy)
    xr = _leaf(x + res)
    hot.layer_norm(xr, w, b, 1e-5).backward(dy)
    assert torch.equal(xl.grad, xr.grad) and torch.equal(rl.grad, xr.grad)


GELU_SHAPES = [(3, 16), (3, 24), (5, 4112), (2 * G + 3, 16), (5, 16384),
               (3, 8 * 2053)]   # 2053 is prime: no grid <= 2048 blocks keeps the columns


@pytest.mark.parametrize("has_bias", [True, False])
@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("shape", GELU_SHAPES)
def test_bias_gelu_bwd_db(C, shape, dtype, has_bias):
    n, d = shape
    assert C.bias_gelu_bwd_db_fused(n, d) == (d != 8 * 2053)
    x = randn((n, d), 230, dtype)
    b = randn((d,), 231, dtype) if has_bias else None
    dy = randn((n, d), 232, dtype)
    dx, db = C.bias_gelu_bwd_db(dy, x, b)
    dx0 = C.bias_gelu_bwd(dy, x, b)
    torch.cuda.synchronize()
    tag = f"bias_gelu_bwd_db[{n}x{d},{dtype},b={has_bias}]"
    assert dx.dtype == dtype and torch.equal(dx, dx0), tag + " dx"
    r64, E = measured(gelu_ref, x, b, dy)
    # the bound of _run_bias_gelu: n fp32 adds of the stored values, each
    # stored value within its own bound of dy*gelu'
    dxa = r64["dx"].abs()
    term_err = U[dtype] * dxa + 4 * E["dx"] + r64["A_dx"]
    bound = n * ULP32 * dxa.sum(0) + term_err.sum(0)
    compare(tag + " db", db, r64["dx"].sum(0), atol=bound, dtype=F32)


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("s", [5, 130])
def test_fa_bwd_delta(C, s, d, packed):
    b, h = 2, 3
    if packed:   # [B, S, H, D] memory seen as [B, H, S, D], as the packed-QKV path passes it
        do = randn((b, s, h, d), 240, BF16).permute(0, 2, 1, 3)
        o = randn((b, s, h, d), 241, BF16).permute(0, 2, 1, 3)
        assert not do.is_contiguous()
    else:
        do, o = randn((b, h, s, d), 240, BF16), randn((b, h, s, d), 241, BF16)
    delta = C.flash_attn_bwd_delta(do, o)
    torch.cuda.synchronize()
    prod = do.double() * o.double()
    compare(f"delta[s={s},d={d},packed={packed}]", delta, prod.sum(-1),
            atol=d * ULP32 * prod.abs().sum(-1), dtype=F32)
    assert delta.is_contiguous() and tuple(delta.shape) == (b, h, s)
