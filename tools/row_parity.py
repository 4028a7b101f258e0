#!/usr/bin/env python3
"""Row / elementwise / optimizer kernel bit-parity fingerprint.

Prints a SHA-256 of every output of the `_C` row-kernel entry points
(norms, bias_gelu, swiglu, rope, dropout_add, colsum, cross-entropy,
embedding, adamw, l2norm^2, amax) on inputs generated on the CPU from fixed
seeds, in bf16 and fp32.  Run it in two builds (separate processes) and diff
the output: a change that only moves code must leave every line identical.

The inputs keep the atomic kernels deterministic: embedding_bwd gets distinct
ids and l2norm_sq a buffer that one block covers.
"""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import paddle_amd  # noqa: F401,E402
from paddle_amd import _ext  # noqa: E402

DEV = "cuda:0"
# smallest shapes of the test lists (one lane, partial strip, many rows, the
# widest register-resident row, the forced two-kernel path) and one
# flagship-width row block
ROW_SHAPES = [(3, 8), (70, 4104), (2051, 64), (5, 8192), (3, 8200), (16, 4096)]
GELU_SHAPES = [(3, 16), (3, 24), (5, 4112)]          # W = 16, W = 8, W = 16 second sweep
COLSUM_SHAPES = [(1, 13), (100, 13), (600, 24)]      # on top of ROW_SHAPES


def randn(seed, *shape, dtype=torch.float32, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale + shift).to(dtype).to(DEV)


def sha(t):
    t = t.detach().reshape(-1).contiguous().cpu()
    return hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()


def report(name, **tensors):
    torch.cuda.synchronize()
    for k, t in tensors.items():
        print(f"{name:40s} {k:8s} {sha(t)}")


def norms(C, n, d, dt, tag):
    x, res, dy, dres = (randn(s, n, d, dtype=dt) for s in (1, 2, 3, 4))
    w, b = randn(5, d, dtype=dt, shift=1.0), randn(6, d, dtype=dt)
    y, mean, rstd = C.layer_norm_fwd(x, w, b, 1e-5)
    report(f"layer_norm_fwd{tag}", y=y, mean=mean, rstd=rstd)
    report(f"layer_norm_fwd_nobias{tag}", y=C.layer_norm_fwd(x, w, None, 1e-5)[0])
    h, y2, mean2, rstd2 = C.add_layer_norm_fwd(x, res, w, b, 1e-5)
    report(f"add_layer_norm_fwd{tag}", h=h, y=y2, mean=mean2, rstd=rstd2)
    dx, dw, db = C.layer_norm_bwd(dy, x, w, mean, rstd, True)
    report(f"layer_norm_bwd{tag}", dx=dx, dw=dw, db=db)
    dx, dw, db = C.layer_norm_bwd(dy, x, w, mean, rstd, True, dres)
    report(f"layer_norm_bwd_dres{tag}", dx=dx, dw=dw, db=db)
    dx, dw, db = C.layer_norm_bwd(dy, x, w, mean, rstd, True, dres, False)
    report(f"layer_norm_bwd_two_kernel{tag}", dx=dx, dw=dw, db=db)
    y, rstd = C.rms_norm_fwd(x, None, w, 1e-6)
    report(f"rms_norm_fwd{tag}", y=y, rstd=rstd)
    yr, rstdr, res_out = C.rms_norm_fwd(x, res, w, 1e-6)
    report(f"rms_norm_fwd_residual{tag}", y=yr, rstd=rstdr, res_out=res_out)
    dx, dw = C.rms_norm_bwd(dy, x, w, rstd)
    report(f"rms_norm_bwd{tag}", dx=dx, dw=dw)


def eltwise(C, n, d, dt, tag):
    x, r, dy = (randn(s, n, d, dtype=dt) for s in (11, 12, 13))
    if d % 16 == 0:
        report(f"swiglu_fwd{tag}", y=C.swiglu_fwd(x))
        report(f"swiglu_bwd{tag}", dx=C.swiglu_bwd(dy[:, : d // 2].contiguous(), x))
    report(f"add_fwd{tag}", y=C.dropout_add_fwd(x, r, 0.0, 0, 0)[0])   # p = 0: no mask
    y, mask = C.dropout_add_fwd(x, r, 0.3, 1234, 7)
    report(f"dropout_add_fwd{tag}", y=y, mask=mask)
    report(f"dropout_add_bwd{tag}", dx=C.dropout_add_bwd(dy, mask, 0.3))
    report(f"dropout_fwd_nores{tag}", y=C.dropout_add_fwd(x, None, 0.3, 99, 0)[0])


def bias_gelu(C, n, d, dt, tag):
    x, dy, b = randn(21, n, d, dtype=dt), randn(22, n, d, dtype=dt), randn(23, d, dtype=dt)
    report(f"bias_gelu_fwd{tag}", y=C.bias_gelu_fwd(x, b))
    report(f"bias_gelu_fwd_nobias{tag}", y=C.bias_gelu_fwd(x, None))
    report(f"bias_gelu_bwd{tag}", dx=C.bias_gelu_bwd(dy, x, b))
    dx, db = C.bias_gelu_bwd_db(dy, x, b)
    report(f"bias_gelu_bwd_db{tag}", dx=dx, db=db)
    dx, db = C.bias_gelu_bwd_db(dy, x, b, False)
    report(f"bias_gelu_bwd_then_colsum{tag}", dx=dx, db=db)


def singles(C, dt, tag):
    x = randn(31, 2, 5, 3, 64, dtype=dt)
    pos = torch.arange(16, dtype=torch.float32)[:, None] * torch.arange(1, 33, dtype=torch.float32)[None, :] / 32
    cos_t, sin_t = pos.cos().to(DEV), pos.sin().to(DEV)
    report(f"rope_fwd{tag}", y=C.rope_fwd(x, cos_t, sin_t, 3, False))
    report(f"rope_conj{tag}", y=C.rope_fwd(x, cos_t, sin_t, 0, True))

    logits = randn(41, 9, 1003, dtype=dt, scale=3.0)
    labels = torch.tensor([0, 5, 1002, -100, 17, 400, 999, 3, 1], device=DEV)
    loss, lse = C.softmax_ce_fwd(logits, labels, -100)
    dlog = C.softmax_ce_bwd(randn(42, 9), logits, labels, lse, -100)
    report(f"softmax_ce{tag}", loss=loss, lse=lse, dlogits=dlog)

    table = randn(51, 50, 72, dtype=dt)
    ids = torch.tensor([[3, 49, 0, 7], [1, 12, 48, 20]], device=DEV)   # distinct, 1 = padding
    report(f"embedding_fwd{tag}", out=C.embedding_fwd(table, ids, 1))
    report(f"embedding_bwd{tag}", dtable=C.embedding_bwd(randn(52, 2, 4, 72, dtype=dt), ids, 50, 1))

    numel = 4099
    master, m, v = randn(61, numel), randn(62, numel, scale=0.1), randn(63, numel, scale=0.1).square()
    grad = randn(64, numel, dtype=dt)
    for pdt in (torch.bfloat16, torch.float32, None):
        mk, mm, vv = master.clone(), m.clone(), v.clone()
        pout = None if pdt is None else torch.zeros(numel, dtype=pdt, device=DEV)
        C.adamw(mk, pout, grad, mm, vv, 1e-2, 0.9, 0.999, 1e-8, 0.1, 0.9 ** 3, 0.999 ** 3, 0.5)
        outs = dict(master=mk, m=mm, v=vv)
        if pout is not None:
            outs["param"] = pout
        report(f"adamw_out_{pdt}{tag}", **outs)

    report(f"l2norm_sq{tag}", out=C.l2norm_sq(randn(71, 1003, dtype=dt)))
    report(f"amax_abs{tag}", out=C.amax_abs(randn(72, 4099, dtype=dt)))


def main():
    C = _ext.get_ext(required=True)
    for dt in (torch.bfloat16, torch.float32):
        name = "bf16" if dt == torch.bfloat16 else "fp32"
        for n, d in ROW_SHAPES:
            tag = f"[{n}x{d},{name}]"
            norms(C, n, d, dt, tag)
            eltwise(C, n, d, dt, tag)
            report(f"colsum{tag}", out=C.colsum(randn(81, n, d, dtype=dt)))
        for n, d in COLSUM_SHAPES:
            report(f"colsum[{n}x{d},{name}]", out=C.colsum(randn(81, n, d, dtype=dt)))
        for n, d in GELU_SHAPES:
            bias_gelu(C, n, d, dt, f"[{n}x{d},{name}]")
        singles(C, dt, f"[{name}]")


if __name__ == "__main__":
    main()
