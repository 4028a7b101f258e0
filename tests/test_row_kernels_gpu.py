"""Row / elementwise HIP kernels vs fp64 references, at the shapes where
they take another code path: single active lane, second sweep over D, row
grid-stride (LDS reuse), W=8 vs W=16 bias_gelu, scalar vocab tail, ...

Every reference is evaluated in fp64 from the exact values the kernel
reads (bf16 inputs upcast).  No tolerance is a free constant
(docs/KERNELS.md, "kernel contract and tolerances"):

  elementwise output in dtype T:   |out - ref| <= u_T*|ref| + 4*E + A
      u_bf16 = 2^-7 (one full ulp, 2x over round-to-nearest), u_fp32 = 0
      E = max |formula in fp32 torch - formula in fp64| on the same inputs;
          4x for reduction order and the v_rcp / v_rsq / v_exp fast paths
      A = rounding of the output's last terms only: EPS = 2^-22 times their
          magnitudes (layer_norm y: 2^-22*(|xhat*w| + |b|)), the cancelling
          x - mu (2*2^-24*(|x| + |mu|)), and erf_fast's 1.5e-7 for gelu.
          No reduction-length term: 4*E carries the reductions.
  reduced output over n terms (dw, db, colsum, l2, embedding grad):
      n*2^-24*sum|terms| (+ sum of the terms' own A, + u_T*|ref| when the
      result is cast to T)

Pure 4*E without A is not met by a correct kernel at the smallest shape,
where fp32 torch sits at its correctly-rounded floor: measured on MI355X
with fp32 tensors, rms_norm (3, 8) dx err 8.1e-7 against 4E = 6.6e-7
(bound with A: 4.2e-6).

The reference functions and `compare` are importable without a GPU:
tests/test_kernel_dispatch_cpu.py runs `compare` against deliberately
wrong references.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import paddle_amd as paddle  # noqa: E402
from paddle_amd import _ext  # noqa: E402
from paddle_amd.ops import functional as hot  # noqa: E402

DEV = "cuda:0"
BF16, F32, F16 = torch.bfloat16, torch.float32, torch.float16
U = {BF16: 2.0 ** -7, F32: 0.0, F16: 2.0 ** -10}
EPS = 2.0 ** -22          # a few fp32 roundings / one fast-path intrinsic
ULP32 = 2.0 ** -24        # fp32 unit roundoff


def RED(n):
    """Relative worst-case error of an fp32 sum of n terms in any order
    (n roundings), plus 8 for the ops that produce and consume it.  Used
    for reduced outputs only (l2_norm_squared)."""
    return (n + 8) * ULP32


# ---------------------------------------------------------------------------
# comparator
# ---------------------------------------------------------------------------
def compare(name, out, ref, *, u=0.0, atol=0.0, dtype=None):
    """assert |out - ref| <= u*|ref| + atol elementwise (atol: float or
    tensor broadcastable to ref).  NaN anywhere fails.  Prints the figure
    before asserting."""
    assert tuple(out.shape) == tuple(ref.shape), f"{name}: shape {tuple(out.shape)} vs {tuple(ref.shape)}"
    if dtype is not None:
        assert out.dtype == dtype, f"{name}: dtype {out.dtype}, expected {dtype}"
    o, r = out.detach().double(), ref.detach().double()
    bound = u * r.abs() + atol
    err = (o - r).abs()
    both_inf = torch.isinf(o) & (o == r)
    err = torch.where(both_inf, torch.zeros_like(err), err)
    ok = err <= bound            # False for NaN
    ratio = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    worst = float(ratio.nan_to_num(nan=float("inf")).max())
    print(f"[cmp] {name}: max_err={float(err.nan_to_num(nan=float('inf')).max()):.3e} "
          f"max_bound={float(bound.max()):.3e} worst err/bound={worst:.3f}")
    assert bool(ok.all()), (f"{name}: {int((~ok).sum())} of {ok.numel()} elements outside the "
                            f"bound (worst err/bound {worst:.3g})")


def measured(fn, *args):
    """E per output: max |fn in fp32 - fn in fp64| on the same inputs."""
    r32 = fn(*[a.float() if torch.is_tensor(a) and a.is_floating_point() else a for a in args])
    r64 = fn(*[a.double() if torch.is_tensor(a) and a.is_floating_point() else a for a in args])
    out = {}
    for k in r64:
        if k.startswith("A_") or k.startswith("_"):
            continue
        d = (r32[k].double() - r64[k]).abs()
        d = d[torch.isfinite(d)]
        out[k] = float(d.max()) if d.numel() else 0.0
    return r64, out


def randn(shape, seed, dtype=F32, dev=None, mean=0.0):
    g = torch.Generator().manual_seed(seed)
    t = (torch.randn(shape, generator=g) + mean).to(dtype)
    return t.to(dev or DEV)


# ---------------------------------------------------------------------------
# references (dtype-generic: run in the dtype of their inputs)
# ---------------------------------------------------------------------------
def ln_ref(x, w, b, dy, eps=1e-5, stat_cols=None):
    """stat_cols: number of leading columns the row statistics use (None =
    all).  Only the comparator self-test passes something else."""
    d = x.shape[-1]
    xs = x if stat_cols is None else x[..., :stat_cols]
    mu = xs.mean(-1, keepdim=True)
    var = ((xs - mu) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = (x - mu) * rstd
    bb = b if b is not None else torch.zeros_like(w)
    y = xh * w + bb
    g = dy * w
    s1 = (g * xh).mean(-1, keepdim=True)
    s2 = g.mean(-1, keepdim=True)
    dx = rstd * (g - s2 - xh * s1)
    r = {"y": y, "mean": mu.reshape(-1), "rstd": rstd.reshape(-1), "dx": dx,
         "dw": (dy * xh).reshape(-1, d).sum(0), "db": dy.reshape(-1, d).sum(0)}
    # --- A terms ---------------------------------------------------------
    n = x.numel() // d
    # x - mu cancels: mu carries one fp32 rounding of its own magnitude
    e_xmu = 2 * ULP32 * (x.abs() + mu.abs())
    e_xh = e_xmu * rstd + EPS * xh.abs()
    r["A_mean"] = (EPS * mu.abs()).reshape(-1)
    r["A_rstd"] = (EPS * rstd).reshape(-1)                       # v_rsq
    r["A_y"] = e_xh * w.abs() + EPS * ((xh * w).abs() + bb.abs())
    r["A_dx"] = (rstd * ((g.abs() * e_xh).mean(-1, keepdim=True) * xh.abs() + e_xh * s1.abs())
                 + EPS * rstd * (g.abs() + s2.abs() + (xh * s1).abs()))
    r["A_dw"] = (n * ULP32 * (dy * xh).abs() + dy.abs() * e_xh).reshape(-1, d).sum(0)
    r["A_db"] = n * ULP32 * dy.abs().reshape(-1, d).sum(0)
    return r


def rms_ref(x, w, dy, res=None, dxr=None, eps=1e-6, res_dtype=None, stat_from_stored=False):
    d = x.shape[-1]
    xr_exact = x if res is None else x + res
    # the kernel stores res_out in T and normalises what it stored, with the
    # row statistic taken from the unrounded sum; the torch path takes the
    # statistic from the stored sum too (stat_from_stored)
    xr = xr_exact if res_dtype is None else xr_exact.to(res_dtype).to(x.dtype)
    ms = ((xr if stat_from_stored else xr_exact) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(ms + eps)
    xh = xr * rstd
    y = xh * w
    g = dy * w
    c = (g * xh).mean(-1, keepdim=True)
    dx_n = rstd * (g - xh * c)
    n = x.numel() // d
    e_xh = EPS * xh.abs()
    r = {"y": y, "res_out": xr_exact, "dx_norm": dx_n,
         "dx": dx_n if dxr is None else dx_n + dxr,
         "dw": (dy * xh).reshape(-1, d).sum(0)}
    r["A_y"] = 2 * EPS * y.abs()
    r["A_res_out"] = ULP32 * xr_exact.abs()
    r["A_dx"] = 2 * EPS * rstd * (g.abs() + (xh * c).abs())
    r["A_dw"] = (n * ULP32 * (dy * xh).abs() + dy.abs() * e_xh).reshape(-1, d).sum(0)
    return r


_ERF_FAST = 1.5e-7   # documented bound of erf_fast (Abramowitz-Stegun 7.1.26)


def gelu_ref(x, bias, dy, col_shift=0):
    """col_shift: comparator self-test only (bias rolled by that many columns)."""
    d = x.shape[-1]
    bb = torch.zeros(d, dtype=x.dtype, device=x.device) if bias is None else bias
    if col_shift:
        bb = torch.roll(bb, col_shift)
    v = x + bb
    cdf = 0.5 * (1.0 + torch.erf(v * 0.7071067811865476))
    pdf = 0.3989422804014327 * torch.exp(-0.5 * v * v)
    gp = cdf + v * pdf
    r = {"y": v * cdf, "dx": dy * gp}
    e_v = ULP32 * v.abs()
    # erf_fast adds 1.5e-7 absolute to erf, i.e. 0.75e-7 to cdf
    # ... and is evaluated as 1 - p*exp(-z^2) in fp32: a few roundings at magnitude 1
    e_cdf = 0.5 * _ERF_FAST + 4 * ULP32 + EPS * cdf + pdf * e_v
    e_gp = e_cdf + EPS * (v * pdf).abs() + (pdf * (1 + v * v)) * e_v + EPS * (v * v) * (v * pdf).abs()
    r["A_y"] = v.abs() * e_cdf + EPS * (v * cdf).abs() + cdf * e_v
    r["A_dx"] = dy.abs() * e_gp + EPS * (dy * gp).abs()
    return r


def swiglu_ref(x, dy):
    d = x.shape[-1] // 2
    g, u = x[..., :d], x[..., d:]
    sig = torch.sigmoid(g)
    silu = g * sig
    sg = sig * (1 + g * (1 - sig))
    r = {"y": silu * u, "dg": dy * u * sg, "du": dy * silu}
    # x/(1+exp(-x)): v_exp + v_rcp + a few roundings, all relative.  exp(-x)
    # overflows fp32 for x < -88.7, where sigmoid < 2^-128 and the kernel
    # returns 0 for |silu|, |silu'| < 700 * 2^-128 < 2^-118 (fp64 itself gives
    # 0 below x = -745); results under 2^-126 may flush to zero.
    under, flush = 2.0 ** -118, 2.0 ** -126
    r["A_y"] = 4 * EPS * (silu * u).abs() + under * u.abs() + flush
    r["A_dg"] = (6 * EPS * (dy * u).abs() * (sig * (1 + (g * (1 - sig)).abs()))
                 + under * (dy * u).abs() + flush)
    r["A_du"] = 4 * EPS * (dy * silu).abs() + under * dy.abs() + flush
    return r


def rope_tables(rows, dh, dev=None, dtype=F32):
    half = dh // 2
    inv = 1.0 / (10000.0 ** (torch.arange(half, dtype=torch.float32) / half))
    fr = torch.outer(torch.arange(rows, dtype=torch.float32), inv)
    return fr.cos().to(dev or DEV), fr.sin().to(dev or DEV)


def rope_ref(x, cos_t, sin_t, pos_offset, conj=False, sin_sign=1.0):
    b, s, h, dh = x.shape
    half = dh // 2
    c = cos_t[pos_offset:pos_offset + s].to(x.dtype).view(1, s, 1, half)
    sn = sin_t[pos_offset:pos_offset + s].to(x.dtype).view(1, s, 1, half) * sin_sign
    if conj:
        sn = -sn
    x1, x2 = x[..., :half], x[..., half:]
    y = torch.cat([x1 * c - x2 * sn, x2 * c + x1 * sn], -1)
    a = torch.cat([(x1 * c).abs() + (x2 * sn).abs(), (x2 * c).abs() + (x1 * sn).abs()], -1)
    return {"y": y, "A_y": EPS * a}


def ce_ref(logits, labels, dloss, ignore_index=-100):
    n, v = logits.shape
    lse = torch.logsumexp(logits, -1)
    skip = (labels == ignore_index) | (labels < 0) | (labels >= v)
    safe = labels.masked_fill(skip, 0)
    picked = logits.gather(1, safe[:, None]).squeeze(1)
    zero = torch.zeros_like(lse)
    loss = torch.where(skip, zero, lse - picked)
    p = torch.exp(logits - lse[:, None])
    onehot = torch.zeros_like(p).scatter_(1, safe[:, None], 1.0)
    g = torch.where(skip, zero, dloss)[:, None]
    fin = torch.where(torch.isinf(logits), torch.zeros_like(logits), logits)
    amax = fin.abs().amax(-1)
    # m + log(l): v_log and the final add; x - lse rounds at ULP32*(|x| + |lse|)
    e_lse = EPS * (1 + lse.abs())
    e_arg = e_lse[:, None] + 2 * ULP32 * (fin.abs() + lse.abs()[:, None])
    return {"lse": lse, "loss": loss, "dlogits": g * (p - onehot),
            "A_lse": e_lse,
            "A_loss": torch.where(skip, zero, e_lse + ULP32 * (lse.abs() + picked.abs())),
            "A_dlogits": g.abs() * (p * (e_arg + EPS) + ULP32)}


def embedding_grad_ref(dout, ids, vocab, padding_idx=None, first_only=False):
    """fp64 scatter-add.  first_only: comparator self-test only."""
    d = dout.shape[-1]
    flat = ids.reshape(-1).long()
    do = dout.reshape(-1, d)
    ok = torch.ones_like(flat, dtype=torch.bool)
    if padding_idx is not None:
        ok = flat != padding_idx
    if first_only:
        seen = set()
        keep = []
        for i in flat.tolist():
            keep.append(i not in seen)
            seen.add(i)
        ok = ok & torch.tensor(keep, device=flat.device)
    ref = torch.zeros(vocab, d, dtype=do.dtype, device=do.device).index_add_(0, flat[ok], do[ok])
    mag = torch.zeros(vocab, d, dtype=do.dtype, device=do.device).index_add_(0, flat[ok], do[ok].abs())
    cnt = torch.zeros(vocab, dtype=do.dtype, device=do.device).index_add_(
        0, flat[ok], torch.ones_like(flat[ok], dtype=do.dtype))
    return {"dtable": ref, "A_dtable": cnt[:, None] * ULP32 * mag}


def dropout_add_ref(x, res, mask, p, scaled=True):
    """scaled=False: comparator self-test only (the 1/(1-p) factor dropped)."""
    s = 1.0 / (1.0 - p) if scaled else 1.0
    y = x * mask.to(x.dtype) * s
    return y if res is None else y + res


def adamw_ref(master, grad, m, v, lr, b1, b2, eps, wd, b1pow, b2pow, gscale=1.0):
    g = grad * gscale
    p = master - lr * wd * master
    mo = b1 * m + (1 - b1) * g
    vo = b2 * v + (1 - b2) * g * g
    upd = lr * (mo / (1 - b1pow)) / (torch.sqrt(vo / (1 - b2pow)) + eps)
    return {"master": p - upd, "m": mo, "v": vo,
            "A_master": EPS * (master.abs() + upd.abs()) + 8 * EPS * upd.abs(),
            "A_m": EPS * ((b1 * m).abs() + ((1 - b1) * g).abs()),
            "A_v": EPS * ((b2 * v).abs() + (1 - b2) * g * g)}


# ---------------------------------------------------------------------------
# helpers for the GPU cases
# ---------------------------------------------------------------------------
def _leaf(t):
    return t.detach().clone().requires_grad_(True)


@pytest.fixture(scope="module", autouse=True)
def _native_on():
    assert _ext.has_ext()
    assert paddle.get_flags(["FLAGS_use_native_kernels"])["FLAGS_use_native_kernels"]
    yield


def _check_elem(name, out, r64, E, key, dtype, extra=0.0):
    compare(name, out, r64[key], u=U[dtype], atol=4 * E[key] + r64["A_" + key] + extra, dtype=dtype)


def _check_red(name, out, r64, key, dtype):
    """reduced output: the A term is the whole bound, plus u_T for the cast
    of the fp32 sum to T."""
    compare(name, out, r64[key], u=U[dtype], atol=r64["A_" + key], dtype=dtype)


# ---------------------------------------------------------------------------
# layer_norm
# ---------------------------------------------------------------------------
LN_SHAPES = [(3, 8), (5, 2056), (2051, 64), (70, 4104), (33, 256)]


def _run_layer_norm(n, d, dtype, has_bias, mean=0.0, wdtype=None, seed=0):
    wdtype = wdtype or dtype
    x = randn((n, d), seed, dtype, mean=mean)
    w = randn((d,), seed + 1, wdtype, mean=1.0)
    b = randn((d,), seed + 2, wdtype) if has_bias else None
    dy = randn((n, d), seed + 3, dtype)
    assert hot._norm_native_ok(x, w, b)
    xl, wl = _leaf(x), _leaf(w)
    bl = _leaf(b) if has_bias else None
    C = _ext.get_ext()
    # what the kernel reads: parameters in x.dtype
    wk = w.to(dtype)
    bk = b.to(dtype) if has_bias else None
    y = hot.layer_norm(xl, wl, bl, 1e-5)
    y.backward(dy)
    _, mean_k, rstd_k = C.layer_norm_fwd(x, wk, bk, 1e-5)
    torch.cuda.synchronize()
    r64, E = measured(ln_ref, x, wk, bk, dy)
    tag = f"ln[{n}x{d},{dtype},b={has_bias},mean={mean},w={wdtype}]"
    print(f"[E] {tag}: " + " ".join(f"{k}={v:.2e}" for k, v in E.items()))
    _check_elem(tag + " y", y, r64, E, "y", dtype)
    compare(tag + " mean", mean_k, r64["mean"], atol=4 * E["mean"] + r64["A_mean"], dtype=F32)
    compare(tag + " rstd", rstd_k, r64["rstd"], atol=4 * E["rstd"] + r64["A_rstd"], dtype=F32)
    _check_elem(tag + " dx", xl.grad, r64, E, "dx", dtype)
    _check_red(tag + " dw", wl.grad, r64, "dw", wdtype)
    if has_bias:
        _check_red(tag + " db", bl.grad, r64, "db", wdtype)
    return r64


@pytest.mark.parametrize("has_bias", [True, False])
@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("shape", LN_SHAPES)
def test_layer_norm(shape, dtype, has_bias):
    _run_layer_norm(shape[0], shape[1], dtype, has_bias)


def test_layer_norm_shifted_mean_fp32():
    """x = 1000 + randn: E[x^2] - mu^2 in fp32 loses the variance (max abs
    error 0.45 in y by CPU emulation of the old formula); the shifted
    moments keep it."""
    _run_layer_norm(8, 1024, F32, True, mean=1000.0, seed=10)


def test_layer_norm_shifted_mean_bf16():
    _run_layer_norm(8, 1024, BF16, True, mean=64.0, seed=11)


# ---------------------------------------------------------------------------
# rms_norm / fused_rms_norm
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("shape", LN_SHAPES)
def test_rms_norm(shape, dtype, wdtype=None):
    n, d = shape
    wdtype = wdtype or dtype
    x, w, dy = randn((n, d), 20, dtype), randn((d,), 21, wdtype, mean=1.0), randn((n, d), 22, dtype)
    assert hot._norm_native_ok(x, w)
    xl, wl = _leaf(x), _leaf(w)
    y = hot.rms_norm(xl, wl, 1e-6)
    y.backward(dy)
    torch.cuda.synchronize()
    r64, E = measured(rms_ref, x, w.to(dtype), dy)
    tag = f"rms[{n}x{d},{dtype},w={wdtype}]"
    print(f"[E] {tag}: " + " ".join(f"{k}={v:.2e}" for k, v in E.items()))
    _check_elem(tag + " y", y, r64, E, "y", dtype)
    _check_elem(tag + " dx", xl.grad, r64, E, "dx", dtype)
    _check_red(tag + " dw", wl.grad, r64, "dw", wdtype)


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("shape", LN_SHAPES)
def test_fused_rms_norm_residual(shape, dtype):
    n, d = shape
    x, res = randn((n, d), 30, dtype), randn((n, d), 31, dtype)
    w, dy, dxr = randn((d,), 32, dtype, mean=1.0), randn((n, d), 33, dtype), randn((n, d), 34, dtype)
    assert hot._norm_native_ok(x, w, residual=res)
    xl, rl, wl = _leaf(x), _leaf(res), _leaf(w)
    y, xr = hot.fused_rms_norm(xl, wl, residual=rl)
    torch.autograd.backward([y, xr], [dy, dxr])
    torch.cuda.synchronize()
    fn = lambda x_, w_, dy_, res_, dxr_: rms_ref(x_, w_, dy_, res_, dxr_, res_dtype=dtype)  # noqa: E731
    r64, E = measured(fn, x, w, dy, res, dxr)
    tag = f"fused_rms[{n}x{d},{dtype}]"
    print(f"[E] {tag}: " + " ".join(f"{k}={v:.2e}" for k, v in E.items()))
    _check_elem(tag + " res_out", xr, r64, E, "res_out", dtype)
    _check_elem(tag + " y", y, r64, E, "y", dtype)
    # dx = round_T(round_T(dx_norm) + dxr): the first rounding is u_T*|dx_norm|
    extra = U[dtype] * r64["dx_norm"].abs()
    assert xl.grad is not None and rl.grad is not None
    _check_elem(tag + " dx", xl.grad, r64, E, "dx", dtype, extra)
    _check_elem(tag + " dres", rl.grad, r64, E, "dx", dtype, extra)
    _check_red(tag + " dw", wl.grad, r64, "dw", dtype)


# ---------------------------------------------------------------------------
# mixed dtype on the kernel path (amp O2 / O1 layouts)
# ---------------------------------------------------------------------------
def test_mixed_dtype_layer_norm_rms_norm():
    r = _run_layer_norm(33, 256, BF16, True, wdtype=F32, seed=40)
    assert r["y"].shape == (33, 256)
    test_rms_norm((33, 256), BF16, wdtype=F32)


def test_mixed_dtype_bias_gelu():
    _run_bias_gelu(33, 24, BF16, True, bdtype=F32)


def test_gpt_block_autocast_matches_torch_path():
    """fp32 GPTDecoderLayer under amp.auto_cast(): bias_gelu gets a bf16
    activation with an fp32 bias, dropout_add a bf16 branch with an fp32
    residual.  Kernel path vs the same stack with the kernels switched off."""
    from paddle_amd.models.gpt import GPTConfig, GPTDecoderLayer
    paddle.seed(7)
    cfg = GPTConfig(vocab_size=64, hidden_size=64, num_layers=1, num_heads=1, max_seq_len=32)
    layer = GPTDecoderLayer(cfg).to(DEV)
    x = randn((2, 128, 64), 41)
    dy = randn((2, 128, 64), 42)
    res, seen = {}, []
    real = _ext.get_ext()

    class Spy:
        """the extension, with the operand dtypes of bias_gelu_fwd recorded"""

        def __getattr__(self, name):
            fn = getattr(real, name)
            if name != "bias_gelu_fwd":
                return fn

            def wrapped(x_, bias_):
                seen.append((x_.dtype, bias_.dtype))
                return fn(x_, bias_)
            return wrapped

    get_ext = _ext.get_ext
    for native in (True, False):
        paddle.set_flags({"FLAGS_use_native_kernels": native})
        _ext.get_ext = lambda required=False: Spy()
        try:
            xl = _leaf(x)
            for p in layer.parameters():
                p.grad = None
            with paddle.amp.auto_cast():
                out = layer(xl)
            out.backward(dy)
            torch.cuda.synchronize()
            res[native] = (out.detach(), xl.grad.detach(),
                           layer.mlp.fc1_bias.grad.detach().clone(),
                           layer.ln2.weight.grad.detach().clone())
        finally:
            _ext.get_ext = get_ext
            paddle.set_flags({"FLAGS_use_native_kernels": True})
        if native:
            # the fp32 bias reached the kernel cast to the activation's dtype
            assert seen == [(BF16, BF16)], seen
            assert layer.mlp.fc1_bias.dtype == F32
    assert len(seen) == 1, "the torch-path stack must not reach the kernel"
    (o1, dx1, db1, dw1), (o0, dx0, db0, dw0) = res[True], res[False]
    assert o1.dtype == o0.dtype == F32 and db1.dtype == db0.dtype == F32
    assert dw1.dtype == dw0.dtype == F32
    # Both stacks round to bf16 at the same eight points (qkv, P, attn out,
    # out_proj, fc1, gelu, fc2, and the branch added to the fp32 residual).
    # Each rounding is at most half a bf16 ulp (2^-9) and the two paths may
    # round opposite ways: K = 8 * 2 * 2^-9.  An element of a branch is a dot
    # product, so its error scales with the row's rms as well as with its own
    # value: |a - b| <= K * (|branch_i| + rms_row(branch)).
    K = 16 * 2.0 ** -9

    def scale(t, dim):
        return t.abs() + t.square().mean(dim, keepdim=True).sqrt()

    compare("gpt block out", o1, o0, atol=K * scale((o0 - x).double(), -1), dtype=F32)
    compare("gpt block dx", dx1, dx0, atol=K * scale((dx0 - dy).double(), -1), dtype=F32)
    # parameter gradients sum 256 rows of such terms; independent roundings
    # grow as sqrt(rows), which is the ratio rms(grad) / |term|
    compare("gpt block dbias", db1, db0, atol=K * scale(db0.double(), 0), dtype=F32)
    compare("gpt block dln2w", dw1, dw0, atol=K * scale(dw0.double(), 0), dtype=F32)


# ---------------------------------------------------------------------------
# fallback path on GPU: inputs outside the contract through the public ops
# ---------------------------------------------------------------------------
def test_fallback_fp16_on_gpu():
    x, w, b, dy = randn((5, 64), 50, F16), randn((64,), 51, F16, mean=1.0), randn((64,), 52, F16), randn((5, 64), 53, F16)
    assert not hot._norm_native_ok(x, w, b)
    assert not hot._bias_gelu_native_ok(x, b)
    assert not hot._swiglu_native_ok(x)
    assert not hot._dropout_add_native_ok(x, x)
    assert not hot._reduce_native_ok(x)
    xl, wl, bl = _leaf(x), _leaf(w), _leaf(b)
    y = hot.layer_norm(xl, wl, bl, 1e-5)
    y.backward(dy)
    r64, E = measured(ln_ref, x, w, b, dy)
    _check_elem("fp16 ln y", y, r64, E, "y", F16)
    _check_elem("fp16 ln dx", xl.grad, r64, E, "dx", F16)
    _check_red("fp16 ln dw", wl.grad, r64, "dw", F16)
    xl = _leaf(x)
    yg = hot.bias_gelu(xl, b)
    yg.backward(dy)
    g64, Eg = measured(gelu_ref, x, b, dy)
    _check_elem("fp16 gelu y", yg, g64, Eg, "y", F16)
    _check_elem("fp16 gelu dx", xl.grad, g64, Eg, "dx", F16)
    s64, Es = measured(swiglu_ref, x, dy[:, :32])
    _check_elem("fp16 swiglu y", hot.swiglu(x), s64, Es, "y", F16)
    compare("fp16 dropout_add p=0", hot.dropout_add(x, dy, 0.0, True), x.double() + dy.double(), u=U[F16] + ULP32, dtype=F16)
    compare("fp16 l2", hot.l2_norm_squared(x), x.double().square().sum().reshape(1),
            atol=float(RED(x.numel()) * x.double().square().sum()))
    lg, lab = randn((7, 40), 54, F16), torch.arange(7, device=DEV) % 40
    assert not hot._ce_native_ok(lg, lab)
    c64, Ec = measured(ce_ref, lg, lab, torch.ones(7, device=DEV))
    compare("fp16 ce loss", hot.softmax_cross_entropy(lg, lab), c64["loss"], atol=4 * Ec["loss"] + c64["A_loss"])
    tb = randn((9, 16), 55, F16)
    assert not hot._embedding_native_ok(tb, lab % 9)
    compare("fp16 embedding", hot.embedding(lab % 9, tb), tb[lab % 9].double(), dtype=F16)
    q = randn((1, 4, 2, 16), 56, F16)
    ct, st = rope_tables(4, 16)
    assert not hot._rope_native_ok(q, ct, st, 0)
    rr = rope_ref(q.double(), ct, st, 0)
    compare("fp16 rope", hot.fused_rotary_position_embedding(q), rr["y"], u=U[F16], atol=rr["A_y"], dtype=F16)


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_fallback_d100_on_gpu(dtype):
    x, w, b, dy = randn((6, 100), 60, dtype), randn((100,), 61, dtype, mean=1.0), randn((100,), 62, dtype), randn((6, 100), 63, dtype)
    assert not hot._norm_native_ok(x, w, b)
    assert not hot._bias_gelu_native_ok(x, b)
    assert not hot._swiglu_native_ok(x)
    xl, wl, bl = _leaf(x), _leaf(w), _leaf(b)
    y = hot.layer_norm(xl, wl, bl, 1e-5)
    y.backward(dy)
    r64, E = measured(ln_ref, x, w, b, dy)
    _check_elem("d100 ln y", y, r64, E, "y", dtype)
    _check_elem("d100 ln dx", xl.grad, r64, E, "dx", dtype)
    _check_red("d100 ln dw", wl.grad, r64, "dw", dtype)
    _check_red("d100 ln db", bl.grad, r64, "db", dtype)
    xl, wl = _leaf(x), _leaf(w)
    yr = hot.rms_norm(xl, wl, 1e-6)
    yr.backward(dy)
    q64, Eq = measured(rms_ref, x, w, dy)
    _check_elem("d100 rms y", yr, q64, Eq, "y", dtype)
    _check_elem("d100 rms dx", xl.grad, q64, Eq, "dx", dtype)
    xl = _leaf(x)
    yg = hot.bias_gelu(xl, b)
    yg.backward(dy)
    g64, Eg = measured(gelu_ref, x, b, dy)
    _check_elem("d100 gelu y", yg, g64, Eg, "y", dtype)
    _check_elem("d100 gelu dx", xl.grad, g64, Eg, "dx", dtype)
    s64, Es = measured(swiglu_ref, x, dy[:, :50])
    _check_elem("d100 swiglu y", hot.swiglu(x), s64, Es, "y", dtype)
    tb = randn((9, 100), 64, dtype)
    ids = torch.tensor([0, 8, 3, 3], device=DEV)
    assert not hot._embedding_native_ok(tb, ids)
    compare("d100 embedding", hot.embedding(ids, tb), tb[ids].double(), dtype=dtype)


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_fallback_dropout_add_numel_1001(dtype):
    x, r = randn((7, 143), 65, dtype), randn((7, 143), 66, dtype)
    assert x.numel() == 1001 and not hot._dropout_add_native_ok(x, r)
    xl = _leaf(x)
    y = hot.dropout_add(xl, r, 0.0, True)
    compare("numel1001 p=0", y, x.double() + r.double(), u=U[dtype] + ULP32, dtype=dtype)
    y.backward(torch.ones_like(y))
    compare("numel1001 dx", xl.grad, torch.ones(7, 143, dtype=torch.float64, device=DEV), dtype=dtype)
    y5 = hot.dropout_add(x, r, 0.5, True)
    kept = (y5.double() - r.double()).abs() > 0
    # every element is either r (dropped) or 2x + r (kept)
    ref = torch.where(kept, 2 * x.double() + r.double(), r.double())
    compare("numel1001 p=0.5", y5, ref, u=2 * U[dtype] + 2 * ULP32, dtype=dtype)


# ---------------------------------------------------------------------------
# bias_gelu
# ---------------------------------------------------------------------------
_SPECIAL = [0.0, 1e-3, -1e-3, 6.0, -6.0, 40.0, -40.0]


def _run_bias_gelu(n, d, dtype, has_bias, bdtype=None):
    bdtype = bdtype or dtype
    x = randn((n, d), 70, F32)
    x.view(-1)[:len(_SPECIAL)] = torch.tensor(_SPECIAL, device=DEV)
    x.view(-1)[-len(_SPECIAL):] = torch.tensor(_SPECIAL, device=DEV)
    x = x.to(dtype)
    b = randn((d,), 71, bdtype) if has_bias else None
    if has_bias:
        b[:len(_SPECIAL)] = 0   # keep the special values special after the add
        b[-len(_SPECIAL):] = 0
    dy = randn((n, d), 72, dtype)
    assert hot._bias_gelu_native_ok(x, b)
    xl = _leaf(x)
    bl = _leaf(b) if has_bias else None
    y = hot.bias_gelu(xl, bl)
    y.backward(dy)
    torch.cuda.synchronize()
    bk = b.to(dtype) if has_bias else None
    r64, E = measured(gelu_ref, x, bk, dy)
    tag = f"bias_gelu[{n}x{d},{dtype},b={has_bias},bd={bdtype}]"
    print(f"[E] {tag}: " + " ".join(f"{k}={v:.2e}" for k, v in E.items()))
    _check_elem(tag + " y", y, r64, E, "y", dtype)
    _check_elem(tag + " dx", xl.grad, r64, E, "dx", dtype)
    if has_bias:
        # db = colsum(dx as stored in T): n fp32 adds of the stored values,
        # each stored value within its own bound of dy*gelu'
        dxa = r64["dx"].abs()
        term_err = U[dtype] * dxa + 4 * E["dx"] + r64["A_dx"]
        bound = n * ULP32 * dxa.sum(0) + term_err.sum(0)
        u = U[bdtype] + (U[dtype] if bdtype != dtype else 0.0)
        compare(tag + " db", bl.grad, r64["dx"].sum(0), u=u, atol=bound, dtype=bdtype)


@pytest.mark.parametrize("has_bias", [True, False])
@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("shape", [(3, 16), (3, 24), (5, 4112), (2100, 4096), (175000, 24)])
def test_bias_gelu(shape, dtype, has_bias):
    _run_bias_gelu(shape[0], shape[1], dtype, has_bias)


# ---------------------------------------------------------------------------
# swiglu
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("shape", [(3, 8), (3, 24), (175000, 24)])
def test_swiglu(shape, dtype):
    n, d = shape
    x = randn((n, 2 * d), 80, F32)
    x[0, :4] = torch.tensor([100.0, -100.0, 1e4, -1e4], device=DEV)
    x[-1, d - 4:d] = torch.tensor([100.0, -100.0, 1e4, -1e4], device=DEV)
    x = x.to(dtype)
    dy = randn((n, d), 81, dtype)
    assert hot._swiglu_native_ok(x)
    xl = _leaf(x)
    y = hot.swiglu(xl)
    y.backward(dy)
    torch.cuda.synchronize()
    r64, E = measured(swiglu_ref, x, dy)
    tag = f"swiglu[{n}x{d},{dtype}]"
    print(f"[E] {tag}: " + " ".join(f"{k}={v:.2e}" for k, v in E.items()))
    assert not torch.isnan(y).any() and not torch.isnan(xl.grad).any()
    _check_elem(tag + " y", y, r64, E, "y", dtype)
    _check_elem(tag + " dg", xl.grad[..., :d], r64, E, "dg", dtype)
    _check_elem(tag + " du", xl.grad[..., d:], r64, E, "du", dtype)


# ---------------------------------------------------------------------------
# rope
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pos_offset", [0, 5])
@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("dh", [8, 128, 520])
def test_rope(dh, dtype, pos_offset):
    b, s, h = 2, 3, 5
    x, dy = randn((b, s, h, dh), 90, dtype), randn((b, s, h, dh), 91, dtype)
    cos_t, sin_t = rope_tables(s + pos_offset, dh)          # exactly s + pos_offset rows
    assert hot._rope_native_ok(x, cos_t, sin_t, pos_offset)
    # public signature: full-width [rows, dh] tables (the halves repeated)
    cos_full, sin_full = torch.cat([cos_t, cos_t], -1), torch.cat([sin_t, sin_t], -1)
    xl = _leaf(x)
    y = hot.fused_rotary_position_embedding(xl, sin=sin_full, cos=cos_full, pos_offset=pos_offset)
    y.backward(dy)
    torch.cuda.synchronize()
    f = rope_ref(x.double(), cos_t, sin_t, pos_offset)
    bwd = rope_ref(dy.double(), cos_t, sin_t, pos_offset, conj=True)
    tag = f"rope[dh={dh},{dtype},off={pos_offset}]"
    compare(tag + " y", y, f["y"], u=U[dtype], atol=f["A_y"], dtype=dtype)
    compare(tag + " dx", xl.grad, bwd["y"], u=U[dtype], atol=bwd["A_y"], dtype=dtype)
    # default tables (built internally) give the same rotation
    y2 = hot.fused_rotary_position_embedding(x, pos_offset=pos_offset)
    compare(tag + " y (built-in tables)", y2, f["y"], u=U[dtype], atol=f["A_y"] + EPS * 8 * x.double().abs().amax(), dtype=dtype)


def test_rope_short_table_raises():
    x = randn((1, 4, 2, 16), 92, BF16)
    cos_t, sin_t = rope_tables(8, 16)
    full = lambda t: torch.cat([t, t], -1)  # noqa: E731
    assert not hot._rope_native_ok(x, cos_t, sin_t, 5)
    with pytest.raises(ValueError):
        hot.fused_rotary_position_embedding(x, sin=full(sin_t), cos=full(cos_t), pos_offset=5)


# ---------------------------------------------------------------------------
# dropout_add through the raw bindings (the mask is visible)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("with_res", [True, False])
@pytest.mark.parametrize("dtype", [BF16, F32])
def test_dropout_add_raw(dtype, with_res):
    C = _ext.get_ext()
    n = 65536
    x = randn((n,), 100, dtype)
    res = randn((n,), 101, dtype) if with_res else None
    dy = randn((n,), 102, dtype)
    assert hot._dropout_add_native_ok(x, res)
    for p in (0.5, 0.1):
        y, mask = C.dropout_add_fwd(x, res, p, 1234, 40)
        y2, mask2 = C.dropout_add_fwd(x, res, p, 1234, 40)
        _, mask8 = C.dropout_add_fwd(x, res, p, 1234, 48)
        dx = C.dropout_add_bwd(dy, mask, p)
        torch.cuda.synchronize()
        assert mask.dtype == torch.uint8 and bool(((mask == 0) | (mask == 1)).all())
        assert torch.equal(mask, mask2) and torch.equal(y, y2), "same (seed, offset) must replay"
        assert torch.equal(mask8[:-8], mask[8:]), "offset must shift the stream by whole elements"
        keep = float(mask.double().mean())
        sigma = math.sqrt(p * (1 - p) / n)
        print(f"[dropout] p={p} keep={keep:.5f} expected={1 - p} 6sigma={6 * sigma:.5f}")
        assert abs(keep - (1 - p)) <= 6 * sigma
        ref = dropout_add_ref(x.double(), None if res is None else res.double(), mask, p)
        dref = dropout_add_ref(dy.double(), None, mask, p)
        if p == 0.5:
            # scale 2 is exact, so x*2 is exact and x*2 + res is one fp32
            # rounding whether or not it is fused: the fp32 evaluation of the
            # reference, rounded to T, is the kernel's result bit for bit
            ref32 = dropout_add_ref(x.float(), None if res is None else res.float(), mask, p)
            assert torch.equal(y, ref32.to(dtype)), "y must follow the mask exactly"
            assert torch.equal(dx, dropout_add_ref(dy.float(), None, mask, p).to(dtype)), \
                "dx must follow the mask exactly"
            compare(f"dropout_add y p={p}", y, ref, u=U[dtype], atol=ULP32 * ref.abs(), dtype=dtype)
        else:
            # 1/(1-p) is a rounded fp32 (v_rcp under fast-math): EPS relative
            a = EPS * (x.double().abs() / (1 - p) + (0 if res is None else res.double().abs()))
            compare(f"dropout_add y p={p}", y, ref, u=U[dtype], atol=a, dtype=dtype)
            compare(f"dropout_add dx p={p}", dx, dref, u=U[dtype], atol=EPS * dy.double().abs() / (1 - p), dtype=dtype)
    outs = C.dropout_add_fwd(x, res, 0.0, 1234, 40)
    assert len(outs) == 1, "p = 0 returns no mask"
    exact = x.float() + (0 if res is None else res.float())   # one fp32 rounding
    assert torch.equal(outs[0], exact.to(dtype))


# ---------------------------------------------------------------------------
# cross entropy
# ---------------------------------------------------------------------------
def _run_ce(n, v, dtype, shift=0.0, neg_inf=None, labels=None, seed=110):
    lg = randn((n, v), seed, F32, mean=shift)
    if neg_inf == "first":
        lg[:, 0] = float("-inf")
    elif neg_inf == "tail":
        lg[:, 1000:] = float("-inf")
    lg = lg.to(dtype)
    g = torch.Generator().manual_seed(seed + 1)
    if labels is None:
        lo, hi = (1, v) if neg_inf == "first" else (0, min(v, 1000) if neg_inf == "tail" else v)
        labels = torch.randint(lo, hi, (n,), generator=g)
        labels[::7] = -100
        if n > 3:
            labels[3] = -1        # out of range, not ignore_index
            labels[1] = hi - 1
    labels = labels.to(DEV)
    dloss = randn((n,), seed + 2, F32)
    assert hot._ce_native_ok(lg, labels)
    ll = _leaf(lg)
    loss = hot.softmax_cross_entropy(ll, labels, ignore_index=-100)
    loss.backward(dloss)
    C = _ext.get_ext()
    _, lse_k = C.softmax_ce_fwd(lg, labels, -100)
    torch.cuda.synchronize()
    r64, E = measured(ce_ref, lg, labels, dloss)
    tag = f"ce[{n}x{v},{dtype},shift={shift},inf={neg_inf}]"
    print(f"[E] {tag}: " + " ".join(f"{k}={v_:.2e}" for k, v_ in E.items()))
    assert torch.isfinite(loss).all(), "loss must be finite"
    compare(tag + " lse", lse_k, r64["lse"], atol=4 * E["lse"] + r64["A_lse"], dtype=F32)
    compare(tag + " loss", loss, r64["loss"], atol=4 * E["loss"] + r64["A_loss"], dtype=F32)
    _check_elem(tag + " dlogits", ll.grad, r64, E, "dlogits", dtype)
    skip = (labels == -100) | (labels < 0) | (labels >= v)
    assert bool((loss[skip] == 0).all()) and bool((ll.grad[skip] == 0).all())
    # torch agrees wherever torch defines the loss
    ok = ~skip
    tref = torch.nn.functional.cross_entropy(lg.double()[ok], labels[ok], reduction="none")
    compare(tag + " loss vs torch", loss[ok], tref, atol=4 * E["loss"] + r64["A_loss"][ok])


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("v", [5, 1003, 2056])
def test_cross_entropy(v, dtype):
    _run_ce(2051, v, dtype)


def test_cross_entropy_shifted_logits_fp32():
    _run_ce(9, 1003, F32, shift=1000.0, seed=120)


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("where", ["first", "tail"])
def test_cross_entropy_neg_inf_logits(where, dtype):
    """Banned tokens.  Before the ce_fwd_kernel fix a -inf that a thread
    sees first made exp(-inf - -inf) = NaN for the whole row."""
    _run_ce(9, 2056 if where == "tail" else 1003, dtype, neg_inf=where, seed=130)


# ---------------------------------------------------------------------------
# embedding
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("d", [8, 520])
def test_embedding(d, dtype):
    vocab, pad = 37, 4
    table = randn((vocab, d), 140, dtype)
    g = torch.Generator().manual_seed(141)
    ids = torch.randint(0, vocab, (6, 11), generator=g)
    ids[0, :3] = torch.tensor([vocab - 1, pad, 0])
    ids[2, 5] = pad
    ids = ids.to(DEV)
    assert hot._embedding_native_ok(table, ids)
    tl = _leaf(table)
    out = hot.embedding(ids, tl, padding_idx=pad)
    dout = randn((6, 11, d), 142, dtype)
    out.backward(dout)
    torch.cuda.synchronize()
    ref = table[ids].clone()
    ref[ids == pad] = 0
    assert out.dtype == dtype and torch.equal(out, ref), "lookup is a copy"
    r = embedding_grad_ref(dout.double(), ids, vocab, pad)
    _check_red(f"embedding[{d},{dtype}] dtable", tl.grad, r, "dtable", dtype)
    assert bool((tl.grad[pad] == 0).all())

    # non-contiguous int32 view of the ids
    wide = torch.stack([ids.int(), ids.int() + 1], -1)
    view = wide[..., 0]
    assert not view.is_contiguous() and view.dtype == torch.int32
    assert hot._embedding_native_ok(table, view)
    assert torch.equal(hot.embedding(view, table, padding_idx=pad), ref)


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_embedding_all_ids_identical(dtype):
    vocab, d, n = 5, 8, 4096
    table = randn((vocab, d), 143, dtype)
    ids = torch.full((n,), 3, device=DEV)
    tl = _leaf(table)
    out = hot.embedding(ids, tl)
    dout = randn((n, d), 144, dtype)
    out.backward(dout)
    torch.cuda.synchronize()
    assert torch.equal(out, table[ids])
    r = embedding_grad_ref(dout.double(), ids, vocab)
    _check_red(f"embedding same-id[{dtype}] dtable", tl.grad, r, "dtable", dtype)


# ---------------------------------------------------------------------------
# colsum / l2_norm_squared / amax_abs
# ---------------------------------------------------------------------------
# one row chunk; the scalar path at d % 8 != 0; a partial last strip; 18
# row chunks (the last one short); 64 row chunks (the last one empty)
COLSUM_SHAPES = [(1, 13), (100, 13), (70, 4104), (600, 24), (2051, 64)]


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("shape", COLSUM_SHAPES)
def test_colsum(shape, dtype):
    C = _ext.get_ext()
    x = randn(shape, 150, dtype)
    assert hot._reduce_native_ok(x)
    out = C.colsum(x)
    xd = x.double()
    compare(f"colsum[{shape},{dtype}]", out, xd.sum(0), atol=shape[0] * ULP32 * xd.abs().sum(0), dtype=F32)


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("numel", [1, 3, 5, 4099])
def test_l2_norm_squared_and_amax_abs(numel, dtype):
    C = _ext.get_ext()
    x = randn((numel,), 160, dtype)
    assert hot._reduce_native_ok(x)
    xd = x.double()
    ssq = xd.square().sum()
    compare(f"l2[{numel},{dtype}]", hot.l2_norm_squared(x), ssq.reshape(1), atol=float(RED(numel) * ssq), dtype=F32)
    am = C.amax_abs(x)
    assert am.dtype == F32 and float(am) == float(xd.abs().max()), "amax is exact"


# ---------------------------------------------------------------------------
# fused_adamw_step
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("gdtype,pdtype", [(F32, F32), (BF16, BF16), (F32, None)])
@pytest.mark.parametrize("numel", [5, 4099])
def test_fused_adamw_step(numel, gdtype, pdtype):
    master, grad = randn((numel,), 170), randn((numel,), 171, gdtype)
    m, v = randn((numel,), 172) * 0.1, randn((numel,), 173).square() * 0.01
    pout = None if pdtype is None else torch.zeros(numel, dtype=pdtype, device=DEV)
    assert hot._adamw_native_ok(master, pout, grad, m, v)
    hp = dict(lr=1e-2, b1=0.9, b2=0.999, eps=1e-8, wd=0.1, step=3)
    # the kernel takes its hyper-parameters as fp32 arguments, and beta^step
    # as one fp32 computed on the host: the reference reads those values
    # (1 - beta and 1 - beta^step are then exact in fp32: Sterbenz)
    f32 = lambda a: float(torch.tensor(a, dtype=F32))  # noqa: E731
    ref_hp = dict(lr=f32(hp["lr"]), b1=f32(hp["b1"]), b2=f32(hp["b2"]), eps=f32(hp["eps"]), wd=f32(hp["wd"]),
                  b1pow=f32(hp["b1"] ** hp["step"]), b2pow=f32(hp["b2"] ** hp["step"]))
    fn = lambda ma, g, m_, v_: adamw_ref(ma, g, m_, v_, gscale=0.5, **ref_hp)  # noqa: E731
    r64, E = measured(fn, master, grad, m, v)
    mk, mm, vv = master.clone(), m.clone(), v.clone()
    hot.fused_adamw_step(mk, pout, grad, mm, vv, hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], hp["step"], grad_scale=0.5)
    torch.cuda.synchronize()
    tag = f"adamw[{numel},g={gdtype},p={pdtype}]"
    print(f"[E] {tag}: " + " ".join(f"{k}={v_:.2e}" for k, v_ in E.items()))
    _check_elem(tag + " master", mk, r64, E, "master", F32)
    _check_elem(tag + " m", mm, r64, E, "m", F32)
    _check_elem(tag + " v", vv, r64, E, "v", F32)
    if pout is not None:
        _check_elem(tag + " param_out", pout, r64, E, "master", pdtype)
