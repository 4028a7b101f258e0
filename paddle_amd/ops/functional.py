"""Autograd-integrated wrappers over the gfx950 HIP kernels.

Each op is a torch.autograd.Function whose forward dispatches to
paddle_amd._C on GPU (mandatory -- _ext.use_native raises if the
extension is missing) and to an fp32 torch reference on CPU.  The CPU
path doubles as the numerics oracle in tests/.

Reference op-signature parity anchors are cited per-op.
"""
from __future__ import annotations

import math
from typing import Optional

import torch

from .. import _ext

# jit.save tracing mode: emit plain substrate ops (no autograd.Function
# wrappers -- TorchScript cannot export Python function calls).  Forward
# inference semantics only; toggled by paddle_amd.jit._substrate_only.
_TRACE_SUBSTRATE = False


def _tracing():
    return _TRACE_SUBSTRATE


# ---------------------------------------------------------------------------
# Kernel contract (docs/KERNELS.md "kernel contract and tolerances").
#
# The row/elementwise kernels exist as bf16 and fp32 templates only, read
# and write 8 elements per lane, and reinterpret every operand pointer in
# the dtype of x.  The predicates below decide from dtypes, shapes and
# contiguity alone -- no CUDA call -- whether a kernel may take a call;
# anything outside the contract takes the torch composite path, which
# works on GPU tensors too.  Per-column parameters (weight / bias, D
# elements) of another dtype are cast to x.dtype by the caller instead,
# so amp O2 (fp32 norm parameters, bf16 activations) stays on the kernel.
# ---------------------------------------------------------------------------
_NATIVE_DTYPES = (torch.bfloat16, torch.float32)


def _kernel_ok(x, *, last_mult=1, numel_mult=1, same=(), vecs=(),
               contiguous=()):
    """Shared contract check.  x: the tensor whose dtype picks the kernel
    template.  last_mult / numel_mult: divisibility of x.shape[-1] /
    x.numel().  same: full-size operands (dtype and shape of x, or None).
    vecs: per-column parameters (floating point, x.shape[-1] elements, or
    None).  contiguous: tensors the op hands over without .contiguous()."""
    if not isinstance(x, torch.Tensor) or x.dtype not in _NATIVE_DTYPES:
        return False
    if x.dim() < 1 or x.numel() == 0:
        return False
    if x.shape[-1] % last_mult or x.numel() % numel_mult:
        return False
    for t in same:
        if t is not None and (t.dtype != x.dtype or t.shape != x.shape):
            return False
    for t in vecs:
        if t is not None and not (t.is_floating_point()
                                  and t.numel() == x.shape[-1]):
            return False
    return all(t is None or t.is_contiguous() for t in contiguous)


def _norm_native_ok(x, w, b=None, residual=None):
    """layer_norm / rms_norm / fused_rms_norm."""
    return _kernel_ok(x, last_mult=8, same=(residual,), vecs=(w, b))


def _decode_stream_ok(x, w, k, bias=None):
    """Contract the MFMA decode W-streamers share (docs/KERNELS.md; pure:
    dtypes, shapes, strides, storage offsets -- no CUDA call).  x: bf16
    [..., K] with 1 <= rows <= 32; w: the 2-D weight tensor whose columns
    are N, on x's device; K % 64 == 0, K <= 2^24, N % 256 == 0; x (as the
    contiguous [rows, K] the dispatch site passes) and w start 16-byte
    aligned; bias floating point with N elements (the site casts it)."""
    if not (isinstance(x, torch.Tensor) and isinstance(w, torch.Tensor)
            and x.dtype == torch.bfloat16 and x.dim() >= 1 and w.dim() == 2
            and w.device == x.device):
        return False
    n = w.shape[1]
    if k <= 0 or k % 64 or k > 2 ** 24 or n <= 0 or n % 256:
        return False
    if x.shape[-1] != k or not 1 <= x.numel() // k <= 32:
        return False
    # a non-contiguous x is copied into a fresh (aligned) allocation
    if x.is_contiguous() and (x.storage_offset() * 2) % 16:
        return False
    if (w.storage_offset() * w.element_size()) % 16:
        return False
    return bias is None or (isinstance(bias, torch.Tensor)
                            and bias.is_floating_point() and bias.numel() == n)


def _decode_gemm_native_ok(x, weight, bias=None):
    """decode_gemm_mfma: _decode_stream_ok with a bf16 [K, N] weight of unit
    column stride and a row stride % 8 == 0 (16-byte row starts)."""
    return (isinstance(weight, torch.Tensor) and weight.dtype == torch.bfloat16
            and weight.dim() == 2 and weight.stride(1) == 1
            and weight.stride(0) % 8 == 0
            and _decode_stream_ok(x, weight, weight.shape[0], bias))


def _bias_gelu_native_ok(x, bias=None):
    return _kernel_ok(x, last_mult=8, vecs=(bias,))


def _swiglu_native_ok(x):
    """x: [..., 2*d] with d % 8 == 0."""
    return _kernel_ok(x, last_mult=16)


def _rope_native_ok(x, cos_t, sin_t, pos_offset=0):
    """x: [B, S, H, Dh] with Dh/2 % 4 == 0; fp32 contiguous tables of
    [>= S + pos_offset, Dh/2]."""
    if not (_kernel_ok(x, last_mult=8, contiguous=(cos_t, sin_t))
            and x.dim() == 4 and pos_offset >= 0):
        return False
    half = x.shape[-1] // 2
    return all(t.dtype == torch.float32 and t.dim() == 2
               and t.shape[1] == half and t.shape[0] >= x.shape[1] + pos_offset
               for t in (cos_t, sin_t))


def _dropout_add_native_ok(x, residual=None):
    return _kernel_ok(x, numel_mult=8, same=(residual,))


def _embedding_native_ok(table, ids):
    return (_kernel_ok(table, last_mult=8) and table.dim() == 2
            and not ids.is_floating_point() and ids.dtype != torch.bool)


def _ce_native_ok(logits, labels):
    return (_kernel_ok(logits) and not labels.is_floating_point()
            and labels.dtype != torch.bool
            and labels.numel() == logits.numel() // logits.shape[-1])


def _reduce_native_ok(x):
    """colsum / l2_norm_squared / amax_abs: any shape, scalar tails."""
    return _kernel_ok(x)


def _adamw_native_ok(master, param_out, grad, m, v):
    if not all(t.dtype == torch.float32 and t.numel() == master.numel()
               for t in (master, m, v)):
        return False
    if param_out is not None and not (param_out.dtype in _NATIVE_DTYPES
                                      and param_out.numel() == master.numel()):
        return False
    return (_kernel_ok(grad) and grad.numel() == master.numel()
            and all(t is None or t.is_contiguous()
                    for t in (master, m, v, param_out)))


def _as_dtype(t, dtype):
    """Per-column parameter in the kernel's dtype (contiguous)."""
    if t is None:
        return None
    return (t if t.dtype == dtype else t.to(dtype)).contiguous()


# ---------------------------------------------------------------------------
# layer_norm (paddle/phi/kernels/gpu/layer_norm_kernel.cu parity)
# ---------------------------------------------------------------------------
class _LayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, eps):
        ctx.native = _ext.use_native(x) and _norm_native_ok(x, w, b)
        ctx.w_dtype = w.dtype
        ctx.b_dtype = b.dtype if b is not None else w.dtype
        if ctx.native:
            C = _ext.get_ext()
            # saved for backward in the form the kernel reads
            x, w = x.contiguous(), _as_dtype(w, x.dtype)
            y, mean, rstd = C.layer_norm_fwd(x, w, _as_dtype(b, x.dtype), eps)
        else:
            xf = x.float()
            mean = xf.mean(-1).reshape(-1)
            var = xf.var(-1, unbiased=False).reshape(-1)
            rstd = torch.rsqrt(var + eps)
            d = x.shape[-1]
            xhat = (xf - mean.view(*x.shape[:-1], 1)) * rstd.view(*x.shape[:-1], 1)
            y = xhat * w.float() + (b.float() if b is not None else 0.0)
            y = y.to(x.dtype)
        ctx.save_for_backward(x, w, mean, rstd)
        ctx.has_bias = b is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, mean, rstd = ctx.saved_tensors
        if ctx.native:
            C = _ext.get_ext()
            dx, dw, db = C.layer_norm_bwd(dy.to(x.dtype).contiguous(), x, w,
                                          mean, rstd, ctx.has_bias)
            dw, db = dw.to(ctx.w_dtype), db.to(ctx.b_dtype)
        else:
            d = x.shape[-1]
            xf = x.float()
            dyf = dy.float()
            mu = mean.view(*x.shape[:-1], 1)
            rs = rstd.view(*x.shape[:-1], 1)
            xhat = (xf - mu) * rs
            g = dyf * w.float()
            s1 = (g * xhat).mean(-1, keepdim=True)
            s2 = g.mean(-1, keepdim=True)
            dx = (rs * (g - s2 - xhat * s1)).to(x.dtype)
            dw = (dyf * xhat).reshape(-1, d).sum(0).to(w.dtype)
            db = dyf.reshape(-1, d).sum(0).to(ctx.b_dtype)
        return dx, dw, (db if ctx.has_bias else None), None


def layer_norm(x, weight, bias=None, epsilon=1e-5):
    if _tracing():
        return torch.nn.functional.layer_norm(x, (x.shape[-1],), weight, bias,
                                              epsilon)
    return _LayerNorm.apply(x, weight, bias, epsilon)


# ---------------------------------------------------------------------------
# residual add + layer_norm in one pass: h = x + residual, y = LN(h)
# ---------------------------------------------------------------------------
def _add_ln_native_ok(x, residual, w, b=None, p=0.0, training=True):
    """Fused add + layer_norm: x and residual of one dtype and shape, both
    contiguous, and dropout inactive (p == 0 or eval)."""
    if p != 0 and training:
        return False
    if not (isinstance(x, torch.Tensor) and isinstance(residual, torch.Tensor)):
        return False
    return _kernel_ok(x, last_mult=8, same=(residual,), vecs=(w, b),
                      contiguous=(x, residual))


class _AddLayerNorm(torch.autograd.Function):
    """(h, y) = (x + residual, layer_norm(x + residual)).  The backward
    hands the gradient arriving at h to the layer_norm backward kernel as
    dres, so neither direction spends a pass on the add.  Off the GPU it
    composes the reference formulas of _DropoutAdd(p=0) and _LayerNorm."""

    @staticmethod
    def forward(ctx, x, residual, w, b, eps):
        ctx.set_materialize_grads(False)
        ctx.native = _ext.use_native(x)
        ctx.w_dtype = w.dtype
        ctx.b_dtype = b.dtype if b is not None else w.dtype
        ctx.has_bias = b is not None
        if ctx.native:
            C = _ext.get_ext()
            w = _as_dtype(w, x.dtype)
            h, y, mean, rstd = C.add_layer_norm_fwd(x, residual, w,
                                                    _as_dtype(b, x.dtype), eps)
        else:
            h = x.clone() + residual
            hf = h.float()
            mean = hf.mean(-1).reshape(-1)
            var = hf.var(-1, unbiased=False).reshape(-1)
            rstd = torch.rsqrt(var + eps)
            xhat = (hf - mean.view(*h.shape[:-1], 1)) * rstd.view(*h.shape[:-1], 1)
            y = xhat * w.float() + (b.float() if b is not None else 0.0)
            y = y.to(h.dtype)
        ctx.save_for_backward(h, w, mean, rstd)
        return h, y

    @staticmethod
    def backward(ctx, dh, dy):
        if dy is None:
            return dh, dh, None, None, None
        h, w, mean, rstd = ctx.saved_tensors
        if ctx.native:
            C = _ext.get_ext()
            dres = None if dh is None else dh.to(h.dtype).contiguous()
            dx, dw, db = C.layer_norm_bwd(dy.to(h.dtype).contiguous(), h, w,
                                          mean, rstd, ctx.has_bias, dres)
            dw, db = dw.to(ctx.w_dtype), db.to(ctx.b_dtype)
        else:
            d = h.shape[-1]
            hf = h.float()
            dyf = dy.float()
            mu = mean.view(*h.shape[:-1], 1)
            rs = rstd.view(*h.shape[:-1], 1)
            xhat = (hf - mu) * rs
            g = dyf * w.float()
            s1 = (g * xhat).mean(-1, keepdim=True)
            s2 = g.mean(-1, keepdim=True)
            dx = (rs * (g - s2 - xhat * s1)).to(h.dtype)
            if dh is not None:
                dx = dx + dh
            dw = (dyf * xhat).reshape(-1, d).sum(0).to(w.dtype)
            db = dyf.reshape(-1, d).sum(0).to(ctx.b_dtype)
        return dx, dx, dw, (db if ctx.has_bias else None), None


def add_layer_norm(x, residual, weight, bias=None, epsilon=1e-5, p=0.0,
                   training=True):
    """(h, y) with h = dropout(x, p) + residual and y = layer_norm(h).  One
    kernel each way when dropout is inactive and the operands fit the
    kernel contract; otherwise exactly dropout_add followed by layer_norm
    (CPU, tracing, mixed dtypes under amp.auto_cast, p > 0)."""
    if (not _tracing() and _add_ln_native_ok(x, residual, weight, bias, p, training)
            and _ext.use_native(x)):
        return _AddLayerNorm.apply(x, residual, weight, bias, epsilon)
    h = dropout_add(x, residual, p, training)
    return h, layer_norm(h, weight, bias, epsilon)


# ---------------------------------------------------------------------------
# rms_norm (+ optional fused residual add)
# paddle parity: incubate/nn/functional/fused_rms_norm.py, rms_norm_kernel.cu
# ---------------------------------------------------------------------------
class _RMSNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, eps):
        ctx.native = _ext.use_native(x) and _norm_native_ok(x, w)
        ctx.w_dtype = w.dtype
        if ctx.native:
            C = _ext.get_ext()
            x, w = x.contiguous(), _as_dtype(w, x.dtype)
            y, rstd = C.rms_norm_fwd(x, None, w, eps)
        else:
            xf = x.float()
            rstd = torch.rsqrt(xf.square().mean(-1) + eps).reshape(-1)
            y = (xf * rstd.view(*x.shape[:-1], 1) * w.float()).to(x.dtype)
        ctx.save_for_backward(x, w, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, rstd = ctx.saved_tensors
        if ctx.native:
            C = _ext.get_ext()
            dx, dw = C.rms_norm_bwd(dy.to(x.dtype).contiguous(), x, w, rstd)
            dw = dw.to(ctx.w_dtype)
        else:
            d = x.shape[-1]
            xf, dyf = x.float(), dy.float()
            rs = rstd.view(*x.shape[:-1], 1)
            xhat = xf * rs
            g = dyf * w.float()
            s1 = (g * xhat).mean(-1, keepdim=True)
            dx = (rs * (g - xhat * s1)).to(x.dtype)
            dw = (dyf * xhat).reshape(-1, d).sum(0).to(w.dtype)
        return dx, dw, None


def rms_norm(x, weight, epsilon=1e-6):
    if _tracing():
        xf = x.float()
        y = xf * torch.rsqrt(xf.square().mean(-1, keepdim=True) + epsilon)
        return (y * weight.float()).to(x.dtype)
    return _RMSNorm.apply(x, weight, epsilon)


class _FusedRMSNormResidual(torch.autograd.Function):
    """y, xr = rms_norm(x + residual) -- returns normed out and the new
    residual stream (paddle fused_rms_norm with residual)."""

    @staticmethod
    def forward(ctx, x, residual, w, eps):
        ctx.native = _ext.use_native(x) and _norm_native_ok(x, w, residual=residual)
        ctx.w_dtype = w.dtype
        if ctx.native:
            C = _ext.get_ext()
            w = _as_dtype(w, x.dtype)
            y, rstd, xr = C.rms_norm_fwd(x.contiguous(), residual.contiguous(), w, eps)
        else:
            xr = x + residual
            xf = xr.float()
            rstd = torch.rsqrt(xf.square().mean(-1) + eps).reshape(-1)
            y = (xf * rstd.view(*x.shape[:-1], 1) * w.float()).to(x.dtype)
        ctx.save_for_backward(xr, w, rstd)
        return y, xr

    @staticmethod
    def backward(ctx, dy, dxr):
        xr, w, rstd = ctx.saved_tensors
        if ctx.native:
            C = _ext.get_ext()
            dx, dw = C.rms_norm_bwd(dy.to(xr.dtype).contiguous(), xr, w, rstd)
            dw = dw.to(ctx.w_dtype)
        else:
            d = xr.shape[-1]
            xf, dyf = xr.float(), dy.float()
            rs = rstd.view(*xr.shape[:-1], 1)
            xhat = xf * rs
            g = dyf * w.float()
            s1 = (g * xhat).mean(-1, keepdim=True)
            dx = (rs * (g - xhat * s1)).to(xr.dtype)
            dw = (dyf * xhat).reshape(-1, d).sum(0).to(w.dtype)
        if dxr is not None:
            dx = dx + dxr
        return dx, dx, dw, None


def fused_rms_norm(x, norm_weight, residual=None, epsilon=1e-6):
    if _tracing() and residual is not None:
        xr = x + residual
        return rms_norm(xr, norm_weight, epsilon), xr
    if residual is None:
        return rms_norm(x, norm_weight, epsilon)
    return _FusedRMSNormResidual.apply(x, residual, norm_weight, epsilon)


# ---------------------------------------------------------------------------
# softmax cross entropy (cross_entropy_kernel.cu parity; hard labels)
# ---------------------------------------------------------------------------
class _SoftmaxCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, ignore_index):
        shp = logits.shape
        v = shp[-1]
        l2 = logits.reshape(-1, v)
        lab = labels.reshape(-1)
        ctx.native = _ext.use_native(logits) and _ce_native_ok(logits, labels)
        if ctx.native:
            C = _ext.get_ext()
            l2, lab = l2.contiguous(), lab.long().contiguous()
            loss, lse = C.softmax_ce_fwd(l2, lab, ignore_index)
        else:
            lab = lab.long()
            lf = l2.float()
            lse = torch.logsumexp(lf, -1)
            skip = (lab == ignore_index) | (lab < 0) | (lab >= v)
            safe = lab.masked_fill(skip, 0)
            picked = lf.gather(1, safe.unsqueeze(1)).squeeze(1)
            loss = torch.where(skip, torch.zeros_like(lse), lse - picked)
        ctx.save_for_backward(l2, lab, lse)
        ctx.ignore_index = ignore_index
        ctx.in_shape = shp
        return loss.reshape(shp[:-1])

    @staticmethod
    def backward(ctx, dloss):
        l2, lab, lse = ctx.saved_tensors
        dl = dloss.reshape(-1).float().contiguous()
        if ctx.native:
            C = _ext.get_ext()
            dlogits = C.softmax_ce_bwd(dl, l2, lab, lse, ctx.ignore_index)
        else:
            p = torch.exp(l2.float() - lse.unsqueeze(1))
            onehot = torch.zeros_like(p)
            skip = (lab == ctx.ignore_index) | (lab < 0) | (lab >= l2.shape[-1])
            safe = lab.masked_fill(skip, 0)
            onehot.scatter_(1, safe.unsqueeze(1), 1.0)
            g = torch.where(skip.unsqueeze(1),
                            torch.zeros_like(dl).unsqueeze(1), dl.unsqueeze(1))
            dlogits = (g * (p - onehot)).to(l2.dtype)
        return dlogits.reshape(ctx.in_shape), None, None


def softmax_cross_entropy(logits, labels, ignore_index=-100, reduction="none"):
    """Per-row softmax cross entropy with hard labels.

    A row whose label equals ignore_index, or lies outside [0, V), has
    zero loss and zero gradient on the kernel and the torch path alike;
    the kernel never reads logits at such a label.  -inf logits (banned
    tokens) are handled as by torch: they carry probability 0.  A row
    whose logits are all -inf is outside the contract.

    reduction="mean" divides by the number of labels that differ from
    ignore_index, as before: an out-of-range label adds 0 to the sum but
    still counts in that denominator."""
    if _tracing():
        v = logits.shape[-1]
        loss = torch.nn.functional.cross_entropy(
            logits.reshape(-1, v).float(), labels.reshape(-1),
            ignore_index=ignore_index, reduction="none").reshape(labels.shape)
    else:
        loss = _SoftmaxCE.apply(logits, labels, ignore_index)
    if reduction == "mean":
        n_valid = (labels != ignore_index).sum().clamp(min=1)
        return loss.sum() / n_valid.to(loss.dtype)
    if reduction == "sum":
        return loss.sum()
    return loss


# ---------------------------------------------------------------------------
# bias + gelu (fused_bias_act parity; erf gelu)
# ---------------------------------------------------------------------------
# Below this many elements dx is still L2-resident when colsum re-reads it,
# so the fused bias gradient saves no HBM pass: small calls keep the dx
# kernel followed by colsum.
_BIAS_GELU_DB_FUSE_MIN = 1 << 20


class _BiasGelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bias):
        ctx.save_for_backward(x, bias if bias is not None else torch.empty(0))
        ctx.has_bias = bias is not None
        ctx.native = _ext.use_native(x) and _bias_gelu_native_ok(x, bias)
        if ctx.native:
            C = _ext.get_ext()
            return C.bias_gelu_fwd(x.contiguous(), _as_dtype(bias, x.dtype))
        v = x.float() + (bias.float() if bias is not None else 0.0)
        return torch.nn.functional.gelu(v).to(x.dtype)

    @staticmethod
    def backward(ctx, dy):
        x, bias = ctx.saved_tensors
        b = bias if ctx.has_bias else None
        # d/dx gelu(x+b) == d/db gelu(x+b), so db = colsum(dx)
        if ctx.native:
            C = _ext.get_ext()
            if ctx.has_bias and x.numel() >= _BIAS_GELU_DB_FUSE_MIN:
                # db summed inside the dx kernel (where no grid keeps a
                # thread on its columns the binding itself runs the dx
                # kernel, then colsum)
                dx, db = C.bias_gelu_bwd_db(dy.to(x.dtype).contiguous(),
                                            x.contiguous(), _as_dtype(b, x.dtype))
                db = db.to(b.dtype)
            else:
                dx = C.bias_gelu_bwd(dy.to(x.dtype).contiguous(), x.contiguous(),
                                     _as_dtype(b, x.dtype))
                db = C.colsum(dx).to(b.dtype) if ctx.has_bias else None
        else:
            v = x.float() + (b.float() if b is not None else 0.0)
            cdf = 0.5 * (1.0 + torch.erf(v * 0.7071067811865476))
            pdf = 0.3989422804014327 * torch.exp(-0.5 * v * v)
            dx = (dy.float() * (cdf + v * pdf)).to(x.dtype)
            db = dx.float().reshape(-1, dx.shape[-1]).sum(0).to(b.dtype) if ctx.has_bias else None
        return dx, db


def bias_gelu(x, bias=None):
    if _tracing():
        return torch.nn.functional.gelu(x + bias if bias is not None else x)
    return _BiasGelu.apply(x, bias)


# ---------------------------------------------------------------------------
# swiglu: silu(x[..., :d]) * x[..., d:]
# paddle parity: incubate/nn/functional/swiglu (fused_bias_act swiglu)
# ---------------------------------------------------------------------------
class _SwiGLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.native = _ext.use_native(x) and _swiglu_native_ok(x)
        if ctx.native:
            x = x.contiguous()
        ctx.save_for_backward(x)
        if ctx.native:
            C = _ext.get_ext()
            return C.swiglu_fwd(x)
        d = x.shape[-1] // 2
        g, u = x[..., :d].float(), x[..., d:].float()
        return (torch.nn.functional.silu(g) * u).to(x.dtype)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        if ctx.native:
            C = _ext.get_ext()
            return C.swiglu_bwd(dy.to(x.dtype).contiguous(), x)
        d = x.shape[-1] // 2
        g, u = x[..., :d].float(), x[..., d:].float()
        sig = torch.sigmoid(g)
        silu = g * sig
        dg = dy.float() * u * (sig * (1 + g * (1 - sig)))
        du = dy.float() * silu
        return torch.cat([dg, du], dim=-1).to(x.dtype)


def swiglu(x, y=None):
    if _tracing():
        if y is None:
            g, u = x.chunk(2, -1)
        else:
            g, u = x, y
        return torch.nn.functional.silu(g) * u
    if y is not None:
        x = torch.cat([x, y], dim=-1)
    return _SwiGLU.apply(x)


# ---------------------------------------------------------------------------
# rotary embedding (fused_rope_kernel.cu RotateHalf parity; neox style)
# ---------------------------------------------------------------------------
_rope_cache = {}


def build_rope_cache(seq_len, head_dim, base=10000.0, device=None, dtype=torch.float32):
    key = (seq_len, head_dim, base, str(device))
    if key not in _rope_cache:
        half = head_dim // 2
        inv = 1.0 / (base ** (torch.arange(0, half, dtype=torch.float32, device=device) / half))
        t = torch.arange(seq_len, dtype=torch.float32, device=device)
        freqs = torch.outer(t, inv)  # [S, half]
        _rope_cache[key] = (freqs.cos().contiguous(), freqs.sin().contiguous())
    return _rope_cache[key]


class _Rope(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, cos_t, sin_t, pos_offset):
        ctx.save_for_backward(cos_t, sin_t)
        ctx.pos_offset = pos_offset
        ctx.native = _ext.use_native(x) and _rope_native_ok(x, cos_t, sin_t, pos_offset)
        if ctx.native:
            C = _ext.get_ext()
            return C.rope_fwd(x.contiguous(), cos_t, sin_t, pos_offset, False)
        return _rope_ref(x, cos_t, sin_t, pos_offset, conj=False)

    @staticmethod
    def backward(ctx, dy):
        cos_t, sin_t = ctx.saved_tensors
        if ctx.native and _rope_native_ok(dy, cos_t, sin_t, ctx.pos_offset):
            C = _ext.get_ext()
            return C.rope_fwd(dy.contiguous(), cos_t, sin_t, ctx.pos_offset, True), None, None, None
        return _rope_ref(dy, cos_t, sin_t, ctx.pos_offset, conj=True), None, None, None


def _rope_ref(x, cos_t, sin_t, pos_offset, conj):
    # x: [B, S, H, D]
    b, s, h, d = x.shape
    half = d // 2
    c = cos_t[pos_offset:pos_offset + s].view(1, s, 1, half).float()
    sn = sin_t[pos_offset:pos_offset + s].view(1, s, 1, half).float()
    if conj:
        sn = -sn
    x1, x2 = x[..., :half].float(), x[..., half:].float()
    y1 = x1 * c - x2 * sn
    y2 = x2 * c + x1 * sn
    return torch.cat([y1, y2], dim=-1).to(x.dtype)


def fused_rotary_position_embedding(q, k=None, v=None, sin=None, cos=None,
                                    position_ids=None, use_neox_rotary_style=True,
                                    base=10000.0, pos_offset=0):
    if _tracing():
        b, s, h, d = q.shape
        if cos is None or sin is None:
            cos_t, sin_t = build_rope_cache(s + pos_offset, d, base, q.device)
        else:
            cos_t = cos.float().reshape(-1, d)[..., : d // 2]
            sin_t = sin.float().reshape(-1, d)[..., : d // 2]
        outs = [_rope_ref(q.float(), cos_t, sin_t, pos_offset, False).to(q.dtype)]
        if k is not None:
            outs.append(_rope_ref(k.float(), cos_t, sin_t, pos_offset, False).to(k.dtype))
        if v is not None:
            outs.append(v)
        return tuple(outs) if len(outs) > 1 else outs[0]
    """paddle.incubate.nn.functional.fused_rotary_position_embedding parity
    (SURVEY.md A.7).  q/k/v: [B, S, H, D]."""
    bq, s, hq, d = q.shape
    if cos is None or sin is None:
        cos_t, sin_t = build_rope_cache(s + pos_offset, d, base, q.device)
    else:
        cos_t, sin_t = cos.float().reshape(-1, d)[..., : d // 2].contiguous(), \
                       sin.float().reshape(-1, d)[..., : d // 2].contiguous()
    # checked here, before any kernel: a short table would be read past its end
    if pos_offset < 0 or min(cos_t.shape[0], sin_t.shape[0]) < s + pos_offset:
        raise ValueError(
            f"fused_rotary_position_embedding: cos/sin hold "
            f"{min(cos_t.shape[0], sin_t.shape[0])} positions, need seq_len + "
            f"pos_offset = {s + pos_offset}")
    outs = [_Rope.apply(q, cos_t, sin_t, pos_offset)]
    if k is not None:
        outs.append(_Rope.apply(k, cos_t, sin_t, pos_offset))
    if v is not None:
        outs.append(v)
    return tuple(outs) if len(outs) > 1 else outs[0]


# ---------------------------------------------------------------------------
# flash attention (flash_attn_kernel.cu API parity)
# ---------------------------------------------------------------------------
def _fa_native_ok(q):
    return (_ext.use_native(q) and q.dtype == torch.bfloat16
            and q.shape[-1] in (64, 128) and q.stride(-1) == 1)


def _fa_seed_offset(fixed_seed_offset=None):
    """Reference dropout RNG contract (funcs/dropout_impl.cu.h:129): a
    (seed, offset) pair; fixed_seed_offset pins it (recompute replays the
    torch CPU generator state, so the default path is replay-deterministic
    under fleet.recompute as well)."""
    if fixed_seed_offset is not None:
        return int(fixed_seed_offset[0]), int(fixed_seed_offset[1])
    seed = int(torch.initial_seed()) & 0x7FFFFFFFFFFFFFFF
    offset = int(torch.randint(0, 2 ** 31, (1,)).item())
    return seed, offset


# dK/dV blocks the GQA backward wants before it gives a block more q heads of
# the group: 256 CUs x occupancy 2.  Measured on MI355X (docs/KERNELS.md, "GQA
# backward", sweep over every divisor G): B2 H8 HKV1 S4096 D128 causal backward
# 0.441 ms at 512 blocks (G 1) against 0.545 at 256 (G 2); B4 H32 HKV8 S2048
# D128 0.692 ms at 512 blocks (G 4) against 0.748 at 1024 and 0.808 at 2048.
# Any N in (256, 512] picks the fastest G of all three shapes measured; no
# grid between 256 and 512 blocks was measured.
_FA_GQA_MIN_BLOCKS = 512


def _fa_bwd_gqa_plan(B, H, HKV, n_kv_blocks):
    """q heads per dK/dV block (gqa_heads_per_block) of the GQA backward: the
    largest divisor G of rep = H // HKV whose grid B * (H // G) * n_kv_blocks
    still has _FA_GQA_MIN_BLOCKS blocks, else 1.  G == rep writes bf16 dK/dV
    straight from the kernel; a smaller G trades an fp32 workspace and a
    reduce kernel for more blocks.  Shapes only, never data."""
    rep = max(1, H // HKV)
    for g in range(rep, 0, -1):
        if rep % g == 0 and B * (H // g) * n_kv_blocks >= _FA_GQA_MIN_BLOCKS:
            return g
    return 1


class _FlashAttn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, scale, causal, mask=None, dropout=0.0,
                seed=0, offset=0):
        # q,k,v: [B, H, S, D] bf16 (views allowed; D contiguous)
        if _fa_native_ok(q):
            C = _ext.get_ext()
            mk = mask.to(torch.bfloat16) if mask is not None else None
            o, lse = C.flash_attn_fwd(q, k, v, None, scale, causal, mk,
                                      dropout, seed, offset)
            ctx.native = True
            ctx.mask = mk
        else:
            dm = None
            if dropout > 0.0:
                g = torch.Generator(device="cpu").manual_seed(
                    (seed * 1000003 + offset) & 0x7FFFFFFFFFFFFFFF)
                dm = (torch.rand(q.shape[0], q.shape[1], q.shape[2], k.shape[2],
                                 generator=g) >= dropout).to(q.device)
            o, lse = _sdpa_ref(q, k, v, scale, causal, mask, dm, dropout)
            ctx.native = False
            ctx.mask = mask
            ctx.drop_mask = dm
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.scale, ctx.causal = scale, causal
        ctx.dropout, ctx.seed, ctx.offset = dropout, seed, offset
        ctx.mark_non_differentiable(lse)
        return o, lse

    @staticmethod
    def backward(ctx, do, _dlse):
        q, k, v, o, lse = ctx.saved_tensors
        if ctx.native:
            C = _ext.get_ext()
            if do.stride(-1) != 1:
                do = do.contiguous()
            kw = dict(scale=ctx.scale, causal=ctx.causal, mask=ctx.mask,
                      pdrop=ctx.dropout, seed=ctx.seed, offset=ctx.offset)
            if k.shape[1] != q.shape[1] and ctx.mask is None:
                # GQA: dK/dV summed per kv head in the kernel
                g = _fa_bwd_gqa_plan(q.shape[0], q.shape[1], k.shape[1],
                                     -(-k.shape[2] // 128))
                dq, dk, dv = C.flash_attn_bwd(do, q, k, v, o, lse, **kw,
                                              gqa_heads_per_block=g)
            elif k.shape[1] != q.shape[1]:
                # GQA with a mask has no kernel: expand K/V, sum the groups
                rep = q.shape[1] // k.shape[1]
                ke = k.repeat_interleave(rep, dim=1)
                ve = v.repeat_interleave(rep, dim=1)
                dq, dke, dve = C.flash_attn_bwd(do, q, ke.contiguous(), ve.contiguous(),
                                                o, lse, **kw)
                hkv = k.shape[1]
                dk = dke.view(k.shape[0], hkv, rep, k.shape[2], k.shape[3]).sum(2)
                dv = dve.view(v.shape[0], hkv, rep, v.shape[2], v.shape[3]).sum(2)
            else:
                dq, dk, dv = C.flash_attn_bwd(do, q, k, v, o, lse, **kw)
        else:
            dq, dk, dv = _sdpa_ref_bwd(do, q, k, v, lse, ctx.scale, ctx.causal,
                                       ctx.mask, getattr(ctx, "drop_mask", None),
                                       ctx.dropout)
        return dq, dk, dv, None, None, None, None, None, None


class _QKVFlashAttn(torch.autograd.Function):
    """Zero-copy causal attention on a packed [B, S, 3, H, D] qkv tensor
    (the GPT hot path): q/k/v are strided views, the output is written
    directly in [B, S, H*D] layout, and backward writes dqkv in place --
    no transpose/cat kernels at all."""

    @staticmethod
    def forward(ctx, qkv, scale, causal, dropout=0.0, seed=0, offset=0):
        b, s, three, h, d = qkv.shape
        q = qkv[:, :, 0].permute(0, 2, 1, 3)  # [b,h,s,d] strided view
        k = qkv[:, :, 1].permute(0, 2, 1, 3)
        v = qkv[:, :, 2].permute(0, 2, 1, 3)
        if _fa_native_ok(q):
            C = _ext.get_ext()
            out = torch.empty(b, s, h, d, dtype=qkv.dtype, device=qkv.device)
            o_view = out.permute(0, 2, 1, 3)
            _, lse = C.flash_attn_fwd(q, k, v, o_view, scale, causal, None,
                                      dropout, seed, offset)
            ctx.native = True
            ctx.save_for_backward(qkv, out, lse)
            ctx.drop_mask = None
        else:
            dm = None
            if dropout > 0.0:
                g = torch.Generator(device="cpu").manual_seed(
                    (seed * 1000003 + offset) & 0x7FFFFFFFFFFFFFFF)
                dm = (torch.rand(b, h, s, s, generator=g) >= dropout).to(qkv.device)
            o, lse = _sdpa_ref(q.contiguous(), k.contiguous(), v.contiguous(),
                               scale, causal, None, dm, dropout)
            out = o.permute(0, 2, 1, 3).reshape(b, s, h, d)
            ctx.native = False
            ctx.save_for_backward(qkv, out, lse)
            ctx.drop_mask = dm
        ctx.scale, ctx.causal = scale, causal
        ctx.dropout, ctx.seed, ctx.offset = dropout, seed, offset
        return out.reshape(b, s, h * d)

    @staticmethod
    def backward(ctx, do):
        qkv, out, lse = ctx.saved_tensors
        b, s, three, h, d = qkv.shape
        q = qkv[:, :, 0].permute(0, 2, 1, 3)
        k = qkv[:, :, 1].permute(0, 2, 1, 3)
        v = qkv[:, :, 2].permute(0, 2, 1, 3)
        o_view = out.permute(0, 2, 1, 3)
        do_view = do.reshape(b, s, h, d).permute(0, 2, 1, 3)
        if ctx.native:
            C = _ext.get_ext()
            if do_view.stride(-1) != 1:
                do_view = do.contiguous().reshape(b, s, h, d).permute(0, 2, 1, 3)
            dqkv = torch.empty_like(qkv)
            dq = dqkv[:, :, 0].permute(0, 2, 1, 3)
            dk = dqkv[:, :, 1].permute(0, 2, 1, 3)
            dv = dqkv[:, :, 2].permute(0, 2, 1, 3)
            C.flash_attn_bwd(do_view, q, k, v, o_view, lse, dq, dk, dv,
                             ctx.scale, ctx.causal, None, ctx.dropout,
                             ctx.seed, ctx.offset)
        else:
            dq, dk, dv = _sdpa_ref_bwd(do_view.contiguous(), q.contiguous(),
                                       k.contiguous(), v.contiguous(), lse,
                                       ctx.scale, ctx.causal, None,
                                       ctx.drop_mask, ctx.dropout)
            # each [b,h,s,d]; stack -> [3,b,h,s,d]; permute -> [b,s,3,h,d]
            dqkv = torch.stack([dq, dk, dv], dim=0).permute(1, 3, 0, 2, 4).contiguous()
        return dqkv, None, None, None, None, None


def qkv_flash_attention(qkv, scale=None, causal=True, dropout=0.0,
                        training=True):
    """qkv: [B, S, 3, H, D] packed (straight out of the fused QKV GEMM)."""
    if scale is None:
        scale = 1.0 / math.sqrt(qkv.shape[-1])
    if _tracing():
        b, s, three, h, d = qkv.shape
        q = qkv[:, :, 0].permute(0, 2, 1, 3)
        k = qkv[:, :, 1].permute(0, 2, 1, 3)
        v = qkv[:, :, 2].permute(0, 2, 1, 3)
        o = torch.nn.functional.scaled_dot_product_attention(
            q, k, v, is_causal=causal, scale=scale)
        return o.permute(0, 2, 1, 3).reshape(b, s, h * d)
    p = dropout if training else 0.0
    seed, offset = _fa_seed_offset() if p > 0 else (0, 0)
    return _QKVFlashAttn.apply(qkv, scale, causal, p, seed, offset)


def _sdpa_ref(q, k, v, scale, causal, attn_mask=None, drop_mask=None,
              dropout=0.0):
    # fp32 reference; returns (o, lse) with lse = logsumexp of scaled scores.
    # attn_mask: additive [B|1, H|1, Sq, Skv]; drop_mask: uint8 keep mask
    # (same shape as scores) with 1/(1-p) rescale -- matches the HIP
    # kernel's semantics (normalizer from undropped P).
    qf, kf, vf = q.float(), k.float(), v.float()
    if k.shape[1] != q.shape[1]:
        rep = q.shape[1] // k.shape[1]
        kf = kf.repeat_interleave(rep, dim=1)
        vf = vf.repeat_interleave(rep, dim=1)
    s = torch.matmul(qf, kf.transpose(-1, -2)) * scale
    if attn_mask is not None:
        s = s + attn_mask.float()
    if causal:
        sq, skv = s.shape[-2], s.shape[-1]
        mask = torch.ones(sq, skv, dtype=torch.bool, device=s.device).tril()
        s = s.masked_fill(~mask, float("-inf"))
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse.unsqueeze(-1))
    if drop_mask is not None:
        p = p * drop_mask.float() / (1.0 - dropout)
    o = torch.matmul(p, vf)
    return o.to(q.dtype), lse


def _sdpa_ref_bwd(do, q, k, v, lse, scale, causal, attn_mask=None,
                  drop_mask=None, dropout=0.0):
    qf, kf, vf, dof = q.float(), k.float(), v.float(), do.float()
    rep = 1
    if k.shape[1] != q.shape[1]:
        rep = q.shape[1] // k.shape[1]
        kf = kf.repeat_interleave(rep, dim=1)
        vf = vf.repeat_interleave(rep, dim=1)
    s = torch.matmul(qf, kf.transpose(-1, -2)) * scale
    if attn_mask is not None:
        s = s + attn_mask.float()
    if causal:
        sq, skv = s.shape[-2], s.shape[-1]
        mask = torch.ones(sq, skv, dtype=torch.bool, device=s.device).tril()
        s = s.masked_fill(~mask, float("-inf"))
    p = torch.exp(s - lse.unsqueeze(-1).float())
    if drop_mask is not None:
        keep = drop_mask.float() / (1.0 - dropout)
        pd = p * keep
        dv = torch.matmul(pd.transpose(-1, -2), dof)
        dp_raw = torch.matmul(dof, vf.transpose(-1, -2))
        dp = dp_raw * keep
        # delta = rowsum(dO*O) = rowsum(dPd * Pd)
        delta = (dp_raw * pd).sum(-1, keepdim=True)
        ds = p * (dp - delta) * scale
        dq = torch.matmul(ds, kf)
        dk = torch.matmul(ds.transpose(-1, -2), qf)
        if rep > 1:
            b, h, skv_, d = dk.shape
            dk = dk.view(b, h // rep, rep, skv_, d).sum(2)
            dv = dv.view(b, h // rep, rep, skv_, d).sum(2)
        return dq.to(q.dtype), dk.to(k.dtype), dv.to(v.dtype)
    dv = torch.matmul(p.transpose(-1, -2), dof)
    dp = torch.matmul(dof, vf.transpose(-1, -2))
    delta = (dp * p).sum(-1, keepdim=True)
    ds = p * (dp - delta) * scale
    dq = torch.matmul(ds, kf)
    dk = torch.matmul(ds.transpose(-1, -2), qf)
    if rep > 1:
        b, h, skv, d = dk.shape
        dk = dk.view(b, h // rep, rep, skv, d).sum(2)
        dv = dv.view(b, h // rep, rep, skv, d).sum(2)
    return dq.to(q.dtype), dk.to(k.dtype), dv.to(v.dtype)


def flash_attention(q, k, v, dropout=0.0, causal=False, scale=None,
                    return_softmax_lse=False, layout="bshd", attn_mask=None,
                    training=True, fixed_seed_offset=None, rng_name="",
                    name=None):
    """paddle.nn.functional.flash_attention parity
    (python/paddle/nn/functional/flash_attention.py:195; mask + Philox
    dropout per flash_attn_kernel.cu:41 / dropout_impl.cu.h:129).

    layout "bshd": q [batch, seq, heads, head_dim] (paddle convention);
    internally computed as [b, h, s, d].
    """
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    p = dropout if training else 0.0
    if _tracing():
        qt, kt, vt = (t.transpose(1, 2) for t in (q, k, v)) \
            if layout == "bshd" else (q, k, v)
        o = torch.nn.functional.scaled_dot_product_attention(
            qt, kt, vt, attn_mask=attn_mask, is_causal=causal and attn_mask is None,
            scale=scale, enable_gqa=kt.shape[1] != qt.shape[1])
        o = o.transpose(1, 2) if layout == "bshd" else o
        return o, None
    seed, offset = _fa_seed_offset(fixed_seed_offset) if p > 0 else (0, 0)
    if layout == "bshd":
        # strided views -- the kernel is stride-aware, no copies
        qt = q.transpose(1, 2)
        kt = k.transpose(1, 2)
        vt = v.transpose(1, 2)
    else:
        qt, kt, vt = q, k, v
    o, lse = _FlashAttn.apply(qt, kt, vt, scale, causal, attn_mask, p,
                              seed, offset)
    if layout == "bshd":
        o = o.transpose(1, 2)
    if return_softmax_lse:
        return o, lse  # [B, H, Sq] fp32 logsumexp of scaled scores
    return o, None


def scaled_dot_product_attention(query, key, value, attn_mask=None,
                                 dropout_p=0.0, is_causal=False, training=True):
    """paddle.nn.functional.scaled_dot_product_attention parity (bshd);
    boolean masks become additive -inf masks (kernel takes additive bf16)."""
    if attn_mask is not None and attn_mask.dtype == torch.bool:
        attn_mask = torch.zeros_like(attn_mask, dtype=query.dtype).masked_fill(
            ~attn_mask, float("-inf"))
    if attn_mask is not None and attn_mask.dim() == 3:
        attn_mask = attn_mask.unsqueeze(1)
    if attn_mask is not None and attn_mask.dim() == 2:
        attn_mask = attn_mask.unsqueeze(0).unsqueeze(0)
    out, _ = flash_attention(query, key, value, dropout=dropout_p,
                             causal=is_causal, attn_mask=attn_mask,
                             training=training)
    return out


# ---------------------------------------------------------------------------
# dropout + residual add (fused_dropout_add_kernel.cu parity)
# ---------------------------------------------------------------------------
class _DropoutAdd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, residual, p, training):
        ctx.p = p if training else 0.0
        ctx.native = _ext.use_native(x) and _dropout_add_native_ok(x, residual)
        if ctx.native:
            C = _ext.get_ext()
            seed = int(torch.cuda.default_generators[x.device.index].initial_seed()) & 0x7FFFFFFF \
                if x.is_cuda else 0
            import random
            offset = random.getrandbits(31)
            outs = C.dropout_add_fwd(x.contiguous(),
                                     residual.contiguous() if residual is not None else None,
                                     ctx.p, seed, offset)
            if ctx.p > 0:
                y, mask = outs
                ctx.save_for_backward(mask)
            else:
                y = outs[0]
                ctx.save_for_backward()
        else:
            if ctx.p > 0:
                mask = (torch.rand_like(x, dtype=torch.float32) >= ctx.p)
                y = x * mask.to(x.dtype) / (1 - ctx.p)
                ctx.save_for_backward(mask)
            else:
                y = x.clone()
                ctx.save_for_backward()
            if residual is not None:
                y = y + residual
        ctx.has_res = residual is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        p = ctx.p
        dres = dy if ctx.has_res else None
        if p == 0:
            return dy, dres, None, None
        (mask,) = ctx.saved_tensors
        if ctx.native and _dropout_add_native_ok(dy):
            C = _ext.get_ext()
            dx = C.dropout_add_bwd(dy.contiguous(), mask, p)
        else:
            dx = dy * mask.to(dy.dtype) / (1 - p)
        return dx, dres, None, None


def dropout_add(x, residual=None, p=0.0, training=True):
    if _tracing():
        return x + residual if residual is not None else x
    return _DropoutAdd.apply(x, residual, p, training)


# ---------------------------------------------------------------------------
# embedding (embedding_grad_kernel.cu parity; atomic scatter-add grad)
# ---------------------------------------------------------------------------
class _Embedding(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ids, table, padding_idx):
        ctx.save_for_backward(ids)
        ctx.vocab = table.shape[0]
        ctx.padding_idx = padding_idx
        ctx.table_dtype = table.dtype
        ctx.native = _ext.use_native(table) and _embedding_native_ok(table, ids)
        if ctx.native:
            C = _ext.get_ext()
            return C.embedding_fwd(table.contiguous(), ids.contiguous().long(),
                                   padding_idx if padding_idx is not None else -1)
        out = torch.nn.functional.embedding(ids.long(), table)
        if padding_idx is not None:
            # paddle (and the kernel) return zeros for padded positions;
            # torch's padding_idx only freezes that row's gradient
            out = out.masked_fill((ids == padding_idx).unsqueeze(-1), 0)
        return out

    @staticmethod
    def backward(ctx, dout):
        (ids,) = ctx.saved_tensors
        if ctx.native and _kernel_ok(dout, last_mult=8):
            C = _ext.get_ext()
            dtable = C.embedding_bwd(dout.contiguous(), ids.contiguous().long(), ctx.vocab,
                                     ctx.padding_idx if ctx.padding_idx is not None else -1)
            dtable = dtable.to(ctx.table_dtype)
        else:
            d = dout.shape[-1]
            dtable = torch.zeros(ctx.vocab, d, dtype=torch.float32, device=dout.device)
            flat_ids = ids.reshape(-1).long()
            ok = torch.ones_like(flat_ids, dtype=torch.bool)
            if ctx.padding_idx is not None:
                ok = flat_ids != ctx.padding_idx
            dtable.index_add_(0, flat_ids[ok], dout.reshape(-1, d)[ok].float())
            dtable = dtable.to(ctx.table_dtype)
        return None, dtable, None


def embedding(ids, table, padding_idx=None):
    if _tracing():
        return torch.nn.functional.embedding(ids, table, padding_idx)
    return _Embedding.apply(ids, table, padding_idx)


# ---------------------------------------------------------------------------
# optimizer primitives
# ---------------------------------------------------------------------------
def fused_adamw_step(master, param_out, grad, m, v, lr, beta1, beta2, eps,
                     weight_decay, step, grad_scale=1.0):
    """In-place fused AdamW on a flat fp32 master shard.  param_out may be
    a bf16 view of the model weights (written by the kernel) or None.
    grad may be bf16 (read direct from the flat reduce buffer) or fp32;
    grad_scale folds grad-clip and the 1/world reduce divide into the
    kernel so no separate mul/cast pass touches HBM.
    adamw_ parity: paddle/phi/kernels/gpu/adamw_kernel.cu."""
    if _ext.use_native(master) and _adamw_native_ok(master, param_out, grad, m, v):
        C = _ext.get_ext()
        C.adamw(master, param_out, grad.contiguous(), m, v, lr, beta1, beta2,
                eps, weight_decay, beta1 ** step, beta2 ** step, grad_scale)
        return
    # torch reference (CPU tests)
    g = grad.float()
    if grad_scale != 1.0:
        g = g * grad_scale
    master.mul_(1 - lr * weight_decay)
    m.mul_(beta1).add_(g, alpha=1 - beta1)
    v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    mhat = m / (1 - beta1 ** step)
    vhat = v / (1 - beta2 ** step)
    master.addcdiv_(mhat, vhat.sqrt().add_(eps), value=-lr)
    if param_out is not None:
        param_out.copy_(master.to(param_out.dtype))


def l2_norm_squared(x):
    if _ext.use_native(x) and _reduce_native_ok(x):
        C = _ext.get_ext()
        return C.l2norm_sq(x.contiguous())
    return x.float().square().sum().reshape(1)


# ---------------------------------------------------------------------------
# paged-KV decode attention (serving; block_multihead_attention parity)
# ---------------------------------------------------------------------------
def _kv_int8_pools_ok(k_cache, v_cache, k_scale, v_scale):
    """The int8 KV storage format (docs/KERNELS.md): int8 contiguous
    [nblocks, bs, HKV, D] code pools of equal shape; fp32 contiguous scales
    on the same device, both [nblocks, bs, HKV] (per token) or both [HKV]
    (per head).  Any D: the kernels add D in {64, 128}."""
    ts = (k_cache, v_cache, k_scale, v_scale)
    if not all(isinstance(t, torch.Tensor) for t in ts):
        return False
    if any(t.device != k_cache.device for t in ts):
        return False
    if not (k_cache.dtype == torch.int8 and v_cache.dtype == torch.int8
            and k_cache.dim() == 4 and k_cache.shape == v_cache.shape
            and k_cache.is_contiguous() and v_cache.is_contiguous()
            and k_cache.numel() > 0):
        return False
    if not (k_scale.dtype == torch.float32 and v_scale.dtype == torch.float32
            and k_scale.shape == v_scale.shape
            and k_scale.is_contiguous() and v_scale.is_contiguous()):
        return False
    return (tuple(k_scale.shape) == tuple(k_cache.shape[:3])
            or tuple(k_scale.shape) == (k_cache.shape[2],))


def _kv_quant_append_native_ok(k, v, k_cache, v_cache, k_scale, v_scale, blk,
                               off, k_quant_scale=None, v_quant_scale=None):
    """Contract of kv_quant_append (pure).  k/v bf16 [T, HKV, D] views with
    contiguous D, token/head strides % 8 == 0 and a 16-byte-aligned start;
    pools per _kv_int8_pools_ok; blk/off int64 contiguous [T]; quant scales
    both None (per-token pools) or both fp32 contiguous [HKV] (per-head
    pools)."""
    if not _kv_int8_pools_ok(k_cache, v_cache, k_scale, v_scale):
        return False
    _, _, hkv, d = k_cache.shape
    if d not in (64, 128):
        return False
    for t in (k, v):
        if not (isinstance(t, torch.Tensor) and t.dtype == torch.bfloat16
                and t.dim() == 3 and t.device == k_cache.device
                and tuple(t.shape) == (k.shape[0], hkv, d)
                and t.stride(2) == 1 and t.stride(0) % 8 == 0
                and t.stride(1) % 8 == 0 and (t.storage_offset() * 2) % 16 == 0):
            return False
    for i in (blk, off):
        if not (isinstance(i, torch.Tensor) and i.dtype == torch.int64
                and tuple(i.shape) == (k.shape[0],) and i.is_contiguous()
                and i.device == k_cache.device):
            return False
    per_token = k_scale.dim() == 3
    if (k_quant_scale is None) != (v_quant_scale is None):
        return False
    if k_quant_scale is None:
        return per_token
    return (not per_token) and all(
        isinstance(s, torch.Tensor) and s.dtype == torch.float32
        and tuple(s.shape) == (hkv,) and s.is_contiguous()
        and s.device == k_cache.device
        for s in (k_quant_scale, v_quant_scale))


def kv_cache_quant_append(k, v, k_cache, v_cache, k_scale, v_scale, blk, off,
                          k_quant_scale=None, v_quant_scale=None):
    """Quantise k/v rows [T, HKV, D] to int8 and write them into the paged
    code pools at (blk[t], off[t]) (in place; docs/KERNELS.md "int8 KV
    cache").  Per-token mode (quant scales None; k_scale/v_scale
    [nblocks, bs, HKV]): d = absmax(row) * fp32(1/127) is stored and
    code = clamp(rint(x / d), +-127); a zero row stores d = 0, codes 0.
    Per-head mode (quant scales [HKV]; k_scale/v_scale [HKV] hold the
    caller's dequant steps and are not written):
    code = clamp(rint(x * quant_scale[h]), +-127).
    The torch path below defines the format."""
    if k.shape[0] == 0:
        return
    if _ext.use_native(k_cache) and _kv_quant_append_native_ok(
            k, v, k_cache, v_cache, k_scale, v_scale, blk, off,
            k_quant_scale, v_quant_scale):
        _ext.get_ext().kv_quant_append(k, v, k_cache, v_cache, k_scale,
                                       v_scale, blk, off, k_quant_scale,
                                       v_quant_scale)
        return
    blk, off = blk.long(), off.long()
    for x, cache, sc, qs in ((k, k_cache, k_scale, k_quant_scale),
                             (v, v_cache, v_scale, v_quant_scale)):
        xf = x.float()
        if qs is None:
            d = xf.abs().amax(-1) * torch.tensor(1.0 / 127.0, dtype=torch.float32,
                                                 device=x.device)
            y = xf / d.unsqueeze(-1).masked_fill(d.unsqueeze(-1) == 0, 1.0)
            sc[blk, off] = d
        else:
            y = xf * qs.float().reshape(1, -1, 1)
        cache[blk, off] = torch.round(y).clamp_(-127, 127).to(torch.int8)


def _kv_int8_dequant_rows(cache, sc, blocks, S):
    """Gathered rows [S, HKV, D] of an int8 pool as fp32 x^ = code * scale."""
    hkv, d = cache.shape[2], cache.shape[3]
    x = cache[blocks].reshape(-1, hkv, d)[:S].float()
    if sc.dim() == 3:
        return x * sc[blocks].reshape(-1, hkv)[:S].unsqueeze(-1)
    return x * sc.reshape(1, hkv, 1)


# Split-KV decode attention (docs/KERNELS.md "split-KV decode attention").
# The plan sees shapes only, never seq_lens, so a captured graph keeps its
# kernels whatever the lengths become.
# Blocks the split grid aims at, by head tile GT: about the blocks 256 CUs
# hold at each variant's occupancy (8 | 5 | 3..2 | 1 waves per SIMD), fitted
# to the sweep in profiles/decode_attn_split.txt.
_DECODE_ATTN_SPLIT_TARGET = {1: 2048, 2: 1024, 4: 512, 8: 512}
# B * H blocks of the one-block-per-q-head kernels that already fill the
# device: at or above it those kernels stay (B32 H32, with or without GQA)
_DECODE_ATTN_SPLIT_FULL = 512
_DECODE_ATTN_SPLIT_MIN_CAPACITY = 512  # below: today's kernels, always
_DECODE_ATTN_SPLIT_MIN_SLICE = 256     # positions of capacity per split
_DECODE_ATTN_SPLIT_PLAN_MAX = 32       # the heuristic's cap (sweep: 1..32)
_DECODE_ATTN_SPLIT_MAX = 64            # the binding's cap


def _decode_attn_split_tiles(H, HKV, int8):
    """(GT, tiles per kv head) of decode_attention_split: the smallest
    instantiated head tile >= G = H/HKV, at most 8 (bf16) or 4 (int8)."""
    g = H // HKV
    gt = 1
    while gt < g and gt < (4 if int8 else 8):
        gt *= 2
    return gt, -(-g // gt)


def _decode_attn_split_plan(B, H, HKV, D, capacity, int8):
    """Number of KV splits for a default paged_decode_attention call
    (pure; capacity = max_blocks * block_size).  1 means today's kernels.
    1 whenever capacity < 512, whenever today's grid B * H reaches 512
    blocks, and whenever the unsplit grid B * HKV * tiles already reaches
    the block target of its head tile; else enough splits to reach that
    target, each covering at least 256 positions of capacity, at most 32."""
    if capacity < _DECODE_ATTN_SPLIT_MIN_CAPACITY or B <= 0 or HKV <= 0 \
            or H <= 0 or H % HKV:
        return 1
    if B * H >= _DECODE_ATTN_SPLIT_FULL:
        return 1
    gt, tiles = _decode_attn_split_tiles(H, HKV, int8)
    target = _DECODE_ATTN_SPLIT_TARGET[gt]
    blocks = B * HKV * tiles
    if blocks >= target:
        return 1
    n = min(capacity // _DECODE_ATTN_SPLIT_MIN_SLICE, -(-target // blocks),
            _DECODE_ATTN_SPLIT_PLAN_MAX)
    return max(int(n), 1)


def _paged_caches_ok(k_cache, v_cache, k_scale, v_scale):
    """The paged pools of the attention bindings: int8 pools per
    _kv_int8_pools_ok with scales, bf16 contiguous [nblocks, bs, HKV, D]
    caches of equal shape without; 16-byte aligned."""
    if (k_scale is None) != (v_scale is None):
        return False
    if k_scale is not None:
        if not (_kv_int8_pools_ok(k_cache, v_cache, k_scale, v_scale)):
            return False
    elif not (k_cache.dtype == torch.bfloat16
              and v_cache.dtype == torch.bfloat16 and k_cache.dim() == 4
              and k_cache.shape == v_cache.shape and k_cache.is_contiguous()
              and v_cache.is_contiguous() and k_cache.numel() > 0):
        return False
    return not any((t.storage_offset() * t.element_size()) % 16
                   for t in (k_cache, v_cache))


def _paged_decode_native_ok(q, k_cache, v_cache, block_table, seq_lens,
                            k_scale=None, v_scale=None):
    """Contract of decode_attention / decode_attention_int8 /
    decode_attention_split for the paged layout (pure: dtypes, shapes,
    strides, devices; mirrors check_paged_decode in csrc/bindings.cpp).
    Everything on q's device; with scales int8 pools per _kv_int8_pools_ok,
    without bf16 contiguous [nblocks, bs, HKV, D] caches of equal shape;
    caches 16-byte aligned; q bf16 [B, H, D] (the dispatch site passes it
    contiguous) 16-byte aligned, D in {64, 128} equal to the cache's,
    H % HKV == 0; block_table [B, max_blocks] and seq_lens [B] integer
    tensors (the site casts them to int32)."""
    if (k_scale is None) != (v_scale is None):
        return False
    ts = (q, k_cache, v_cache, block_table, seq_lens)
    if not all(isinstance(t, torch.Tensor) for t in ts):
        return False
    if any(t.device != q.device for t in ts):
        return False
    if not _paged_caches_ok(k_cache, v_cache, k_scale, v_scale):
        return False
    if not (q.dtype == torch.bfloat16 and q.dim() == 3):
        return False
    b, h, d = q.shape
    if d not in (64, 128) or d != k_cache.shape[3] or h == 0 \
            or h % k_cache.shape[2]:
        return False
    if q.is_contiguous() and (q.storage_offset() * 2) % 16:
        return False
    ints = (torch.int32, torch.int64)
    return (block_table.dim() == 2 and block_table.shape[0] == b
            and block_table.dtype in ints and seq_lens.dim() == 1
            and seq_lens.shape[0] == b and seq_lens.dtype in ints)


# the names the int8 and split-KV predicates had before they became one
_decode_attn_split_native_ok = _paged_decode_native_ok


def _kv_int8_native_ok(q, k_cache, v_cache, k_scale, v_scale, block_table,
                       seq_lens):
    return k_scale is not None and _paged_decode_native_ok(
        q, k_cache, v_cache, block_table, seq_lens, k_scale, v_scale)


def paged_decode_attention(q, k_cache, v_cache, block_table, seq_lens, scale=None,
                           k_scale=None, v_scale=None, num_splits=None):
    """One decode step. q: [B, H, D]; k/v_cache: [nblocks, block_size, HKV, D];
    block_table: int32 [B, max_blocks]; seq_lens: int32 [B].
    With k_scale/v_scale the caches are int8 code pools (docs/KERNELS.md
    "int8 KV cache"): fp32 scales [nblocks, block_size, HKV] (per token, as
    kv_cache_quant_append writes them) or [HKV] (per head).
    num_splits chooses the launch (docs/KERNELS.md "split-KV decode
    attention"): None asks _decode_attn_split_plan, whose answer 1 means
    one block per q-head; 0 pins that; n >= 1 forces split-KV with n splits
    (n = 1: group sharing alone).
    Outside _paged_decode_native_ok, on CPU or with native kernels off, the
    torch path below answers and num_splits is ignored."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    int8 = k_scale is not None or v_scale is not None
    if num_splits is not None and (int(num_splits) != num_splits
                                   or not 0 <= num_splits
                                   <= _DECODE_ATTN_SPLIT_MAX):
        raise ValueError("paged_decode_attention: num_splits must be None or "
                         f"an integer in [0, {_DECODE_ATTN_SPLIT_MAX}], got "
                         f"{num_splits!r}")
    if int8:
        if k_scale is None or v_scale is None:
            raise ValueError("paged_decode_attention: give both k_scale and "
                             "v_scale or neither")
        if not _kv_int8_pools_ok(k_cache, v_cache, k_scale, v_scale):
            raise ValueError(
                "paged_decode_attention: k_scale/v_scale need int8 contiguous "
                "[nblocks, bs, HKV, D] caches of equal shape and fp32 "
                "contiguous scales [nblocks, bs, HKV] or [HKV]")
    if _ext.use_native(q) and _paged_decode_native_ok(
            q, k_cache, v_cache, block_table, seq_lens, k_scale, v_scale):
        C = _ext.get_ext()
        q, table, lens = (q.contiguous(), block_table.int().contiguous(),
                          seq_lens.int().contiguous())
        n = num_splits
        if n is None:
            n = _decode_attn_split_plan(
                q.shape[0], q.shape[1], k_cache.shape[2], q.shape[2],
                table.shape[1] * k_cache.shape[1], int8)
            n = n if n > 1 else 0
        if n:
            return C.decode_attention_split(q, k_cache, v_cache, table, lens,
                                            scale, int(n), k_scale, v_scale)
        if int8:
            return C.decode_attention_int8(q, k_cache, v_cache, k_scale,
                                           v_scale, table, lens, scale)
        return C.decode_attention(q, k_cache, v_cache, table, lens, scale)
    # reference: gather each sequence's KV then plain attention
    B, H, D = q.shape
    HKV = k_cache.shape[2]
    bs = k_cache.shape[1]
    rep = H // HKV
    out = torch.empty_like(q)
    for b in range(B):
        S = int(seq_lens[b])
        nb = (S + bs - 1) // bs
        blocks = block_table[b, :nb].long()
        if int8:
            k = _kv_int8_dequant_rows(k_cache, k_scale, blocks, S)
            v = _kv_int8_dequant_rows(v_cache, v_scale, blocks, S)
        else:
            k = k_cache[blocks].reshape(-1, HKV, D)[:S]  # [S, HKV, D]
            v = v_cache[blocks].reshape(-1, HKV, D)[:S]
        kf = k.float().repeat_interleave(rep, dim=1)   # [S, H, D]
        vf = v.float().repeat_interleave(rep, dim=1)
        s = torch.einsum("hd,shd->hs", q[b].float(), kf) * scale
        p = torch.softmax(s, dim=-1)
        out[b] = torch.einsum("hs,shd->hd", p, vf).to(q.dtype)
    return out


# Paged prefill attention (docs/KERNELS.md "paged prefill attention").
def _paged_prefill_native_ok(q, k_cache, v_cache, block_table, seq_lens, cu_q,
                             max_q, k_scale=None, v_scale=None):
    """Contract of the paged_prefill_attention binding (pure: dtypes, shapes,
    strides, devices; mirrors paged_prefill_attention in csrc/bindings.cpp).
    Caches, scales and their alignment as in _paged_decode_native_ok; q bf16
    [T, H, D] (the dispatch site passes it contiguous) 16-byte aligned, D in
    {64, 128} equal to the cache's, H % HKV == 0; block_table
    [B, max_blocks], seq_lens [B] and cu_q [B + 1] integer tensors (the site
    casts them to int32) on q's device; max_q an integer with 1 <= max_q and
    max_q * H / HKV < 2^31; T * H < 2^31, max_blocks * bs < 2^31; B and HKV
    at most 65535 (grid dimensions); B >= 1 unless T == 0."""
    ts = (q, k_cache, v_cache, block_table, seq_lens, cu_q)
    if not all(isinstance(t, torch.Tensor) for t in ts):
        return False
    if block_table.dim() != 2 or q.dim() != 3:
        return False
    B = block_table.shape[0]
    if any(t.device != q.device for t in ts):
        return False
    if not _paged_caches_ok(k_cache, v_cache, k_scale, v_scale):
        return False
    if q.dtype != torch.bfloat16:
        return False
    d = q.shape[2]
    if d not in (64, 128) or d != k_cache.shape[3] or q.shape[1] == 0 \
            or q.shape[1] % k_cache.shape[2]:
        return False
    if q.is_contiguous() and (q.storage_offset() * 2) % 16:
        return False
    ints = (torch.int32, torch.int64)
    if not (block_table.dtype in ints and seq_lens.dim() == 1
            and seq_lens.shape[0] == B and seq_lens.dtype in ints
            and cu_q.dim() == 1 and cu_q.shape[0] == B + 1
            and cu_q.dtype in ints):
        return False
    if isinstance(max_q, bool) or not isinstance(max_q, int) or max_q < 1:
        return False
    T, H = q.shape[0], q.shape[1]
    bs, HKV = k_cache.shape[1], k_cache.shape[2]
    lim = 1 << 31
    return (max_q * (H // HKV) < lim and T * H < lim
            and block_table.shape[1] * bs < lim and k_cache.shape[0] < lim
            and B <= 65535 and HKV <= 65535 and (B >= 1 or T == 0))


def paged_prefill_attention(q, k_cache, v_cache, block_table, seq_lens, cu_q,
                            max_q, scale=None, k_scale=None, v_scale=None):
    """Attention of q_len_b >= 1 new tokens per sequence over the paged cache.
    q: [T, H, D] packed over sequences; cu_q: int [B + 1] prefix sums,
    q_len_b = cu_q[b+1] - cu_q[b]; k/v_cache, block_table [B, max_blocks],
    k_scale/v_scale: the pools of paged_decode_attention.  seq_lens[b] is the
    cached length INCLUDING the new tokens (append them first);
    S_b = clamp(seq_lens[b], 0, max_blocks * bs).  Token i of sequence b sits
    at position S_b - q_len_b + i and sees positions 0 .. that one
    (bottom-right causal); a row that sees nothing is zero.  A table entry
    outside [0, nblocks) contributes nothing.
    max_q: host integer >= max_b q_len_b; it sizes the kernel's grid so that
    nothing is read on the host.  Rows of a sequence with q_len_b > max_q are
    outside the contract: the kernel leaves the surplus rows (unspecified
    values, nothing out of bounds); so are tokens that no sequence covers.
    Outside _paged_prefill_native_ok, on CPU or with native kernels off, the
    torch path below answers (it reads seq_lens and cu_q on the host)."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    int8 = k_scale is not None or v_scale is not None
    if int8:
        if k_scale is None or v_scale is None:
            raise ValueError("paged_prefill_attention: give both k_scale and "
                             "v_scale or neither")
        if not _kv_int8_pools_ok(k_cache, v_cache, k_scale, v_scale):
            raise ValueError(
                "paged_prefill_attention: k_scale/v_scale need int8 contiguous "
                "[nblocks, bs, HKV, D] caches of equal shape and fp32 "
                "contiguous scales [nblocks, bs, HKV] or [HKV]")
    if _ext.use_native(q) and _paged_prefill_native_ok(
            q, k_cache, v_cache, block_table, seq_lens, cu_q, max_q, k_scale,
            v_scale):
        return _ext.get_ext().paged_prefill_attention(
            q.contiguous(), k_cache, v_cache, block_table.int().contiguous(),
            seq_lens.int().contiguous(), cu_q.int().contiguous(), int(max_q),
            scale, k_scale, v_scale)
    # reference: gather each sequence's KV, masked softmax in fp32
    T, H, D = q.shape
    nblocks, bs, HKV = k_cache.shape[0], k_cache.shape[1], k_cache.shape[2]
    rep = H // HKV
    out = torch.zeros_like(q)
    cu = [int(x) for x in cu_q.tolist()]
    lens = [int(x) for x in seq_lens.tolist()]
    for b in range(block_table.shape[0]):
        lo, hi = max(cu[b], 0), min(cu[b + 1], T)
        q_len = cu[b + 1] - cu[b]
        if q_len <= 0 or lo >= hi:
            continue
        S = max(0, min(lens[b], block_table.shape[1] * bs))
        if S == 0:
            continue
        blocks = block_table[b, :(S + bs - 1) // bs].long()
        inside = (blocks >= 0) & (blocks < nblocks)
        blocks = blocks.clamp(0, nblocks - 1)
        if int8:
            k = _kv_int8_dequant_rows(k_cache, k_scale, blocks, S)
            v = _kv_int8_dequant_rows(v_cache, v_scale, blocks, S)
        else:
            k = k_cache[blocks].reshape(-1, HKV, D)[:S]
            v = v_cache[blocks].reshape(-1, HKV, D)[:S]
        kf = k.float().repeat_interleave(rep, dim=1)   # [S, H, D]
        vf = v.float().repeat_interleave(rep, dim=1)
        i = torch.arange(lo - cu[b], hi - cu[b], device=q.device)
        pos = torch.arange(S, device=q.device)
        seen = (pos[None, :] <= (S - q_len + i)[:, None]) \
            & inside.repeat_interleave(bs)[:S][None, :]       # [q, S]
        s = torch.einsum("qhd,shd->qhs", q[lo:hi].float(), kf) * scale
        s = s.masked_fill(~seen[:, None, :], float("-inf"))
        p = torch.softmax(s, dim=-1).masked_fill(~seen[:, None, :], 0.0)
        p = torch.nan_to_num(p, nan=0.0)               # a row that sees nothing
        out[lo:hi] = torch.einsum("qhs,shd->qhd", p, vf).to(q.dtype)
    return out


# ---------------------------------------------------------------------------
# fused FFN: fc1(+bias+GELU in the hipBLASLt epilogue) -> fc2.
# Backward folds dGELU + fc1 bias-grad into fc2's dgrad GEMM (DGELU_BGRAD),
# so the [tokens, 4h] activation is never touched by a separate elementwise
# pass.  GELU is the tanh approximation (Tensile epilogue).
# Parity: paddle incubate FusedFeedForward / fused_gemm_epilogue
# (paddle/phi/kernels/fusion/gpu/fused_gemm_epilogue_kernel.cu).
# ---------------------------------------------------------------------------
class _FusedFFN(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2):
        C = _ext.get_ext()
        xs = x.shape
        x2 = x.reshape(-1, xs[-1]).contiguous()
        g, z = C.fc1_gelu_fwd(x2, w1, b1)
        y = torch.addmm(b2, g, w2)
        ctx.save_for_backward(x2, w1, w2, z, g)
        ctx.xshape = xs
        return y.reshape(*xs[:-1], w2.shape[1])

    @staticmethod
    def backward(ctx, dy):
        C = _ext.get_ext()
        x2, w1, w2, z, g = ctx.saved_tensors
        dy2 = dy.reshape(-1, dy.shape[-1]).contiguous()
        dz1, db1 = C.fc2_dgrad_dgelu(dy2, w2, z)   # dGELU + bias-grad fused
        dw2 = g.t() @ dy2
        db2 = dy2.sum(0)
        dx = dz1 @ w1.t()
        dw1 = x2.t() @ dz1
        return dx.reshape(ctx.xshape), dw1, db1, dw2, db2


def fused_ffn(x, w1, b1, w2, b2):
    """y = gelu(x @ w1 + b1) @ w2 + b2 with epilogue-fused bias/GELU.
    Paddle Linear layout: w1 [K, 4K], w2 [4K, K]."""
    return _FusedFFN.apply(x, w1, b1, w2, b2)


# ---------------------------------------------------------------------------
# own-MFMA fused linear / FFN (gemm.hip 8-phase kernel + epilogues).
# fwd runs NT with a per-step cached W^T; dgrad is NT directly because
# paddle's W[in,out] IS the NT B-operand; wgrad picks own-TN vs hipBLASLt
# from the autotune table.  Reference: fused_gemm_epilogue_kernel.cu +
# matmul_kernel_impl.h:914 dispatch pattern.
# ---------------------------------------------------------------------------
from . import gemm_dispatch as _gd  # noqa: E402


def _own_dgrad_ok(dy2, w):
    # dx = dy2 @ w^T: paddle's W[in, out] is the NT B-operand as stored
    return _gd.use_own("nt", dy2.shape[0], w.shape[0], w.shape[1]) \
        and _gd.own_gemm_ok(dy2, w, "nt")


def _wgrad(x2, dy2):
    if _gd.use_own("tn", x2.shape[1], dy2.shape[1], x2.shape[0]) \
            and _gd.own_gemm_ok(x2, dy2, "tn"):
        return _gd.gemm_tn(x2, dy2)
    return torch.matmul(x2.t(), dy2)


def _colsum(dy2, dtype):
    if not _reduce_native_ok(dy2):
        return dy2.float().sum(0).to(dtype)
    C = _ext.get_ext()
    return C.colsum(dy2).to(dtype)


class _FusedLinearOwn(torch.autograd.Function):
    """y = x @ W (+bias) on the own NT kernel (W paddle-layout [K, N])."""

    @staticmethod
    def forward(ctx, x, w, bias):
        xs = x.shape
        x2 = x.reshape(-1, xs[-1]).contiguous()
        wt = _gd.weight_t(w)
        if bias is not None:
            y2 = _gd.gemm_nt(x2, wt, epilogue=1, bias=bias.contiguous())
        else:
            y2 = _gd.gemm_nt(x2, wt)
        ctx.save_for_backward(x2, w)
        ctx.xshape, ctx.has_bias = xs, bias is not None
        return y2.reshape(*xs[:-1], w.shape[1])

    @staticmethod
    def backward(ctx, dy):
        x2, w = ctx.saved_tensors
        dy2 = dy.reshape(-1, dy.shape[-1]).contiguous()
        dx = _gd.gemm_nt(dy2, w) if _own_dgrad_ok(dy2, w) \
            else torch.matmul(dy2, w.t())
        dw = _wgrad(x2, dy2)
        db = _colsum(dy2, w.dtype) if ctx.has_bias else None
        return dx.reshape(ctx.xshape), dw, db


class _FusedFFNOwn(torch.autograd.Function):
    """FFN pair on the own NT kernel: fc1 carries bias+GELU in the GEMM
    epilogue (pre-activation saved as aux), fc2's dgrad carries dGELU in
    its epilogue -- the [tokens, 4h] tensor never sees a separate
    elementwise pass in either direction."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2):
        xs = x.shape
        x2 = x.reshape(-1, xs[-1]).contiguous()
        g, z = _gd.gemm_nt(x2, _gd.weight_t(w1), epilogue=2, bias=b1.contiguous())
        if b2 is not None:
            y = _gd.gemm_nt(g, _gd.weight_t(w2), epilogue=1, bias=b2.contiguous())
        else:
            y = _gd.gemm_nt(g, _gd.weight_t(w2))
        ctx.save_for_backward(x2, w1, w2, z, g)
        ctx.xshape, ctx.has_b2 = xs, b2 is not None
        return y.reshape(*xs[:-1], w2.shape[1])

    @staticmethod
    def backward(ctx, dy):
        x2, w1, w2, z, g = ctx.saved_tensors
        dy2 = dy.reshape(-1, dy.shape[-1]).contiguous()
        # dz = (dy @ W2^T) * gelu'(z): DGELU epilogue on fc2's dgrad
        dz = _gd.gemm_nt(dy2, w2, epilogue=3, aux=z)
        dw2 = _wgrad(g, dy2)
        db2 = _colsum(dy2, w2.dtype) if ctx.has_b2 else None
        dx = _gd.gemm_nt(dz, w1) if _own_dgrad_ok(dz, w1) \
            else torch.matmul(dz, w1.t())
        dw1 = _wgrad(x2, dz)
        db1 = _colsum(dz, w1.dtype)
        return dx.reshape(ctx.xshape), dw1, db1, dw2, db2


def _own_linear_ok(x, w, layout="nt"):
    if not (_gd._native_ok(x) and w.dtype == torch.bfloat16):
        return False
    m = x.numel() // x.shape[-1]
    # x @ w as stored is the NN operand pair: the forward runs it as NT on
    # W^T, the dgrad reads w itself, so both must meet the operand contract
    return _gd.use_own(layout, m, w.shape[1], w.shape[0]) \
        and _gd.own_gemm_ok(x.reshape(-1, x.shape[-1]), w, "nn")


def fused_linear_own(x, w, bias=None):
    return _FusedLinearOwn.apply(x, w, bias)


def fused_ffn_own(x, w1, b1, w2, b2):
    return _FusedFFNOwn.apply(x, w1, b1, w2, b2)


_lt_ffn_ok = None


def _fused_ffn_available(x):
    global _lt_ffn_ok
    if not (x.is_cuda and x.dtype == torch.bfloat16 and _ext.use_native(x)):
        return False
    if _lt_ffn_ok is None:
        C = _ext.get_ext()
        if not hasattr(C, "lt_epilogue_probe"):
            _lt_ffn_ok = False
        else:
            # GELU_AUX_BIAS=164 fwd, DGELU_BGRAD=208 bwd -- both must have
            # Tensile kernels in this hipBLASLt build
            _lt_ffn_ok = (C.lt_epilogue_probe(1024, 1024, 1024, 164) > 0 and
                          C.lt_epilogue_probe(1024, 1024, 1024, 208) > 0)
    return _lt_ffn_ok


def fused_linear_param_grad_add(x, dy, dweight=None, dbias=None,
                                multi_precision=False, has_bias=True):
    """dW += X^T dY (and db += colsum(dY)) in single accumulating GEMM /
    reduction launches -- no intermediate dW allocation.
    Parity: paddle/phi/kernels/fusion/gpu/fused_linear_param_grad_add_kernel.cu
    (used by the sequence-parallel backward overlap)."""
    x2 = x.reshape(-1, x.shape[-1])
    dy2 = dy.reshape(-1, dy.shape[-1])
    if dweight is None:
        dweight = torch.zeros(x2.shape[1], dy2.shape[1], dtype=x.dtype,
                              device=x.device)
    dweight.addmm_(x2.t(), dy2)   # beta=1 accumulate inside the GEMM epilogue
    if has_bias:
        if dbias is None:
            dbias = torch.zeros(dy2.shape[1], dtype=dy.dtype, device=dy.device)
        if dy.is_cuda and _ext.use_native(dy) and _reduce_native_ok(dy2):
            C = _ext.get_ext()
            dbias.add_(C.colsum(dy2.contiguous()).to(dbias.dtype))
        else:
            dbias.add_(dy2.sum(0).to(dbias.dtype))
        return dweight, dbias
    return dweight, None


class _FlashAttnVarlen(torch.autograd.Function):
    """Single-launch ragged attention over packed [total, H, D] tensors
    (reference flash_attn_unpadded / flash_attn_kernel.cu:41 varlen via
    cu_seqlens; ours maps each 128-row block to its sequence in-kernel)."""

    @staticmethod
    def forward(ctx, q, k, v, cu_q, cu_k, scale, causal, dropout, seed, offset):
        C = _ext.get_ext()
        o, lse = C.flash_attn_varlen_fwd(q, k, v, cu_q, cu_k, scale, causal,
                                         dropout, seed, offset)
        ctx.save_for_backward(q, k, v, o, lse, cu_q, cu_k)
        ctx.scale, ctx.causal = scale, causal
        ctx.dropout, ctx.seed, ctx.offset = dropout, seed, offset
        ctx.mark_non_differentiable(lse)
        return o, lse

    @staticmethod
    def backward(ctx, do, _dlse):
        q, k, v, o, lse, cu_q, cu_k = ctx.saved_tensors
        C = _ext.get_ext()
        # kv blocks from the packed total: a lower bound, no look at cu_k
        g = _fa_bwd_gqa_plan(1, q.shape[1], k.shape[1], -(-k.shape[0] // 128))
        dq, dk, dv = C.flash_attn_varlen_bwd(do, q, k, v, o, lse, cu_q, cu_k,
                                             ctx.scale, ctx.causal, ctx.dropout,
                                             ctx.seed, ctx.offset,
                                             gqa_heads_per_block=g)
        return dq, dk, dv, None, None, None, None, None, None, None


def flash_attn_varlen_func(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q,
                           max_seqlen_k, scale=None, causal=False,
                           dropout=0.0, training=True, return_softmax_lse=False):
    """Varlen (ragged) flash attention over packed [total_tokens, H, D]
    inputs with cu_seqlens boundaries (reference: flash_attn_unpadded,
    python/paddle/nn/functional/flash_attention.py:593).

    Native path: ONE kernel launch for the whole mixed-length batch
    (per-block sequence bounds resolved in-kernel); CPU fallback groups
    by shape."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    p = dropout if training else 0.0
    if (_ext.use_native(q) and q.dtype == torch.bfloat16
            and q.shape[-1] in (64, 128) and k.shape[1] > 0
            and q.shape[1] % k.shape[1] == 0):
        cu_q = cu_seqlens_q.to(torch.int32)
        cu_k = cu_seqlens_k.to(torch.int32)
        seed, offset = _fa_seed_offset() if p > 0 else (0, 0)
        out, lse = _FlashAttnVarlen.apply(q, k, v, cu_q, cu_k, scale, causal,
                                          p, seed, offset)
        return (out, lse) if return_softmax_lse else out
    import collections
    nq = cu_seqlens_q.tolist()
    nk = cu_seqlens_k.tolist()
    out = torch.empty_like(q)
    groups = collections.defaultdict(list)
    for i in range(len(nq) - 1):
        groups[(nq[i + 1] - nq[i], nk[i + 1] - nk[i])].append(i)
    for (lq, lk), idxs in groups.items():
        qg = torch.stack([q[nq[i]:nq[i] + lq] for i in idxs]).transpose(1, 2)
        kg = torch.stack([k[nk[i]:nk[i] + lk] for i in idxs]).transpose(1, 2)
        vg = torch.stack([v[nk[i]:nk[i] + lk] for i in idxs]).transpose(1, 2)
        og, _ = flash_attention(qg.transpose(1, 2), kg.transpose(1, 2),
                                vg.transpose(1, 2), causal=causal, scale=scale)
        for j, i in enumerate(idxs):
            out[nq[i]:nq[i] + lq] = og[j]
    if return_softmax_lse:
        return out, None
    return out
