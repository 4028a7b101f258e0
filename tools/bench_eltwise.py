"""Microbench the HBM-bound elementwise/reduction kernels at bench shapes.

Prints achieved TB/s against the ~8 TB/s HBM3E peak; run on MI355X.
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
from paddle_amd.ops import functional as hot  # noqa: E402
import paddle_amd._C as C  # noqa: E402

DEV = "cuda"
torch.manual_seed(0)


def timeit(fn, iters=30):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def report(name, sec, gb):
    print(f"{name:28s} {sec * 1e6:9.1f} us   {gb / sec / 1e3:6.2f} TB/s")


# GPT-6.7B shapes: tokens = 8*2048, hidden 4096, ffn 16384
M, H, F = 8 * 2048, 4096, 16384
GB = 1e9

z = torch.randn(M, F, device=DEV, dtype=torch.bfloat16)
b = torch.randn(F, device=DEV, dtype=torch.bfloat16)
dy = torch.randn(M, F, device=DEV, dtype=torch.bfloat16)

t = timeit(lambda: C.bias_gelu_fwd(z, b))
report("bias_gelu fwd [16k,16k]", t, 2 * M * F * 2 / GB)

t = timeit(lambda: C.bias_gelu_bwd(dy, z, b))
report("bias_gelu bwd", t, 3 * M * F * 2 / GB)

t = timeit(lambda: C.colsum(dy))
report("colsum [16k,16k]", t, M * F * 2 / GB)

# the L2-resident case _BiasGelu.backward sends to colsum (below 2^20 elements)
small = torch.randn(256, 4096, device=DEV, dtype=torch.bfloat16)
t = timeit(lambda: C.colsum(small), iters=200)
report("colsum [256,4k]", t, 256 * 4096 * 2 / GB)

x = torch.randn(M, H, device=DEV, dtype=torch.bfloat16)
w = torch.randn(H, device=DEV, dtype=torch.bfloat16)
bb = torch.randn(H, device=DEV, dtype=torch.bfloat16)
y, mean, rstd = C.layer_norm_fwd(x, w, bb, 1e-5)
dyh = torch.randn(M, H, device=DEV, dtype=torch.bfloat16)

t = timeit(lambda: C.layer_norm_fwd(x, w, bb, 1e-5))
report("ln fwd [16k,4k]", t, 2 * M * H * 2 / GB)

t = timeit(lambda: C.layer_norm_bwd(dyh, x, w, mean, rstd, True))
report("ln bwd (dx+dwdb)", t, 5 * M * H * 2 / GB)

_, rrstd = C.rms_norm_fwd(x, None, w, 1e-6)
t = timeit(lambda: C.rms_norm_bwd(dyh, x, w, rrstd))
report("rms_norm_bwd [16k,4k]", t, 5 * M * H * 2 / GB)

r = torch.randn(M, H, device=DEV, dtype=torch.bfloat16)
t = timeit(lambda: C.dropout_add_fwd(x, r, 0.1, 1234, 0))
report("dropout_add fwd [16k,4k]", t, 3 * M * H * 2 / GB)

# ---- fused passes at the flagship shapes: tokens = 12*2048 -----------------
# bytes = the minimum each kernel has to move (bf16 tensors, fp32 partials
# not counted)
M2 = 12 * 2048
del z, dy, x, dyh, r, y
x = torch.randn(M2, H, device=DEV, dtype=torch.bfloat16)
r = torch.randn(M2, H, device=DEV, dtype=torch.bfloat16)
dyh = torch.randn(M2, H, device=DEV, dtype=torch.bfloat16)
T1 = M2 * H * 2 / GB   # one [24576, 4096] bf16 tensor

t = timeit(lambda: (C.dropout_add_fwd(x, r, 0.0, 0, 0), C.layer_norm_fwd(x, w, bb, 1e-5)))
report("add, ln fwd (2 kernels)", t, 5 * T1)
t = timeit(lambda: C.add_layer_norm_fwd(x, r, w, bb, 1e-5))
report("add_ln fwd [24k,4k]", t, 4 * T1)

_, mean, rstd = C.layer_norm_fwd(x, w, bb, 1e-5)
t = timeit(lambda: C.layer_norm_bwd(dyh, x, w, mean, rstd, True, None, False).__getitem__(0).add_(r))
report("ln bwd 2-kernel + add", t, 8 * T1)
t = timeit(lambda: C.layer_norm_bwd(dyh, x, w, mean, rstd, True, None, False))
report("ln bwd 2-kernel", t, 5 * T1)
for cap in (256, 512, 1024, 2048):
    t = timeit(lambda: C.layer_norm_bwd(dyh, x, w, mean, rstd, True, r, True, cap))
    report(f"ln bwd 1-pass+dres G={cap}", t, 4 * T1)
t = timeit(lambda: C.layer_norm_bwd(dyh, x, w, mean, rstd, True))
report("ln bwd 1-pass (default G)", t, 3 * T1)

qkv_do = torch.randn(12, 2048, 32, 128, device=DEV, dtype=torch.bfloat16).permute(0, 2, 1, 3)
qkv_o = torch.randn(12, 2048, 32, 128, device=DEV, dtype=torch.bfloat16).permute(0, 2, 1, 3)
t = timeit(lambda: C.flash_attn_bwd_delta(qkv_do, qkv_o))
report("fa_bwd delta packed [24k,4k]", t, 2 * T1)
do_c, o_c = qkv_do.contiguous(), qkv_o.contiguous()
t = timeit(lambda: C.flash_attn_bwd_delta(do_c, o_c))
report("fa_bwd delta contiguous", t, 2 * T1)
del qkv_do, qkv_o, do_c, o_c, x, r, dyh

z = torch.randn(M2, F, device=DEV, dtype=torch.bfloat16)
dy = torch.randn(M2, F, device=DEV, dtype=torch.bfloat16)
T4 = M2 * F * 2 / GB
t = timeit(lambda: C.bias_gelu_bwd_db(dy, z, b, False))
report("bias_gelu bwd, colsum", t, 4 * T4)
t = timeit(lambda: C.bias_gelu_bwd_db(dy, z, b))
report("bias_gelu bwd+db [24k,16k]", t, 3 * T4)
del z, dy

g = torch.randn(M, device=DEV)
n = 201 * 2 ** 20
master = torch.randn(n, device=DEV)
grad = torch.randn(n, device=DEV, dtype=torch.bfloat16)
mm = torch.zeros(n, device=DEV)
vv = torch.zeros(n, device=DEV)
pb = torch.empty(n, device=DEV, dtype=torch.bfloat16)
t = timeit(lambda: C.adamw(master, pb, grad, mm, vv, 1e-4, 0.9, 0.95, 1e-8,
                           0.1, 0.9, 0.95, 1.0), iters=10)
report("adamw 201M (bf16 grad)", t, n * (4 * 3 * 2 + 2 + 2) / GB)

t = timeit(lambda: C.l2norm_sq(grad), iters=10)
report("l2norm 201M bf16", t, n * 2 / GB)
