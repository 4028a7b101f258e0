"""Weight-only int4 on the GPU: the decode_gemm_int4 W-streamer, the
dequant_int4 kernel, the weight_only_linear dispatch, the binding's contract
and hipGraph capture.

Reference (independent of the code under test): this file unpacks the
documented storage format itself --

    byte (kp, n) = (q[2kp, n] & 0xF) | ((q[2kp+1, n] & 0xF) << 4)
    scale [N] (group_size -1) or [K/gs, N];  w^ = q * scale / 7

-- forms w^ in fp64 and computes ref = x.double() @ w^ + bias.double() from
the bf16 x and bias the kernel reads.

Bound (derived, no free constant), with S = |x| @ |w^| in fp64:

    |out - ref| <= 2^-7 |ref| + (2^-8 + K 2^-24) S

  2^-7     one bf16 ulp for the output cast,
  2^-8     admits one round-to-nearest bf16 rounding of each dequantized
           weight (a kernel may fold scale/7 into the bf16 weight),
  K 2^-24  fp32 accumulation of K terms in any order.

Compared with <=, never by ratio: S is 0 wherever a probed code is 0.  The
helpers below are shared with test_weight_only_int4_cpu.py, which shows on
CPU emulations that the bound rejects a nibble swap, /8 for /7, group
scales shifted by one group and a dropped last k pair.
"""
import functools

import pytest
import torch

DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32
U_BF16 = 2.0 ** -7

# (M, K, N, group_size): the smallest shapes where the kernel can go wrong
CASES = [
    (1, 64, 256, -1),       # single tile: no prefetch, loop guards
    (17, 192, 512, 64),     # odd tile count, 2nd m-tile with 15 dead rows,
                            # 2nd n-block offset into scales
    (32, 320, 256, 64),
    (16, 384, 512, 128),
    (32, 1152, 256, 128),
    (32, 1152, 256, -1),
]
# forced split counts that make kchunk an odd multiple of 64
ODD_KSPLIT = {320: 2, 384: 2, 1152: 4}   # kchunk 192, 192, 320
PROBE_K = [0, 1, 2, 63, 64, 65, 127, 128, 129, 319, 320, 321, 639, 640,
           1150, 1151]


# ---------------------------------------------------------------------------
# the documented format, written out independently of paddle_amd
# ---------------------------------------------------------------------------
def ref_expand(scale, k, gs):
    """scale [N] | [K/gs, N] -> [K, N]."""
    if gs == -1:
        return scale.reshape(1, -1).expand(k, -1)
    assert scale.shape[0] * gs == k
    return scale.repeat_interleave(gs, dim=0)


def ref_quantize(w, gs):
    """fp32 w [K, N] -> (packed int8 [K/2, N], fp32 scale, codes [K, N])."""
    k, n = w.shape
    w = w.float()
    if gs == -1:
        scale = w.abs().amax(dim=0)
    else:
        scale = torch.stack([w[g * gs:(g + 1) * gs].abs().amax(dim=0)
                             for g in range(k // gs)])
    scale = scale.clamp(min=1e-8)
    q = torch.round(w / ref_expand(scale, k, gs) * 7.0).clamp(-7, 7).to(torch.int64)
    byte = (q[0::2] & 0xF) | ((q[1::2] & 0xF) << 4)          # 0..255
    packed = torch.where(byte >= 128, byte - 256, byte).to(torch.int8)
    return packed.contiguous(), scale.contiguous(), q


def ref_unpack(qw):
    """packed int8 [K/2, N] -> codes int64 [K, N]."""
    b = qw.to(torch.int64) & 0xFF
    lo, hi = b & 0xF, b >> 4
    lo = torch.where(lo >= 8, lo - 16, lo)
    hi = torch.where(hi >= 8, hi - 16, hi)
    q = torch.empty(2 * qw.shape[0], qw.shape[1], dtype=torch.int64,
                    device=qw.device)
    q[0::2], q[1::2] = lo, hi
    return q


def ref_what(qw, scale, gs):
    """w^ = q * scale / 7 in fp64, [K, N]."""
    q = ref_unpack(qw)
    return q.double() * ref_expand(scale.double(), q.shape[0], gs) / 7.0


def ref_and_bound(x, what, bias=None):
    """(ref, bound) of the module docstring, both fp64 [M, N]."""
    xd = x.double()
    ref = xd @ what
    if bias is not None:
        ref = ref + bias.double()
    s = xd.abs() @ what.abs()
    k = what.shape[0]
    return ref, U_BF16 * ref.abs() + (2.0 ** -8 + k * 2.0 ** -24) * s


def violations(out, ref, bound, extra=0.0):
    """number of elements outside the bound, and the worst err/bound (inf
    where the bound is 0 and the error is not)."""
    err = (out.double() - ref).abs()
    b = bound + extra
    bad = ~(err <= b)                       # NaN counts as bad
    ratio = torch.where(b > 0, err / b,
                        torch.where(err > 0, torch.full_like(err, float("inf")),
                                    torch.zeros_like(err)))
    return int(bad.sum()), float(ratio.nan_to_num(nan=float("inf")).max())


def check(name, out, ref, bound, extra=0.0):
    assert out.dtype == BF16 and tuple(out.shape) == tuple(ref.shape), name
    nbad, worst = violations(out, ref, bound, extra)
    print(f"[int4] {name}: worst err/bound={worst:.3f}")
    assert nbad == 0, (f"{name}: {nbad} of {ref.numel()} elements outside the "
                       f"bound (worst err/bound {worst:.3g})")


def make_inputs(m, k, n, seed):
    """w = 0.1 randn (fp32), x = randn (bf16), bf16 bias, on the CPU."""
    g = torch.Generator().manual_seed(seed)
    w = 0.1 * torch.randn(k, n, generator=g)
    x = torch.randn(m, k, generator=g).to(BF16)
    bias = torch.randn(n, generator=g).to(BF16)
    return w, x, bias


def make_case(m, k, n, gs, seed, dev):
    """make_inputs with w quantized by ref_quantize."""
    w, x, bias = make_inputs(m, k, n, seed)
    qw, scale, _ = ref_quantize(w, gs)
    return x.to(dev), qw.to(dev), scale.to(dev), bias.to(dev)


@functools.lru_cache(maxsize=None)
def gpu_case(m, k, n, gs):
    x, qw, scale, bias = make_case(m, k, n, gs, 1000 + k + n + m + gs, DEV)
    ref, bound = ref_and_bound(x, ref_what(qw, scale, gs), bias)
    return x, qw, scale, bias, ref, bound


def _C():
    from paddle_amd import _ext
    return _ext.get_ext(required=True)


def _streamer_runs():
    runs = []
    for (m, k, n, gs) in CASES:
        splits = [0] if k < 320 else [1, ODD_KSPLIT[k], 0]
        runs += [(m, k, n, gs, s) for s in splits]
    return runs


# ---------------------------------------------------------------------------
# decode_gemm_int4
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("m,k,n,gs,ksplit", _streamer_runs())
def test_decode_gemm_int4_random_gpu(m, k, n, gs, ksplit):
    """Random cases at ksplit 1, a forced split whose kchunk is an odd
    multiple of 64 (K=1152, ksplit=4: boundaries 320 and 960 fall inside
    128-groups) and the heuristic (ksplit 0)."""
    x, qw, scale, bias, ref, bound = gpu_case(m, k, n, gs)
    out = _C().decode_gemm_int4(x, qw, scale, bias, gs, ksplit)
    check(f"M{m} K{k} N{n} gs{gs} ksplit{ksplit}", out, ref, bound)
    # without bias
    ref0, bound0 = ref_and_bound(x, ref_what(qw, scale, gs))
    out0 = _C().decode_gemm_int4(x, qw, scale, None, gs, ksplit)
    check(f"M{m} K{k} N{n} gs{gs} ksplit{ksplit} nobias", out0, ref0, bound0)


@pytest.mark.gpu
@pytest.mark.parametrize("gs", [-1, 64, 128])
def test_decode_gemm_int4_one_hot_probe_gpu(gs):
    """Rows of x one-hot at tile, group and split edges (forced ksplit=4,
    kchunk 320): output row i must equal w^[k_i, :] -- a pure bf16 ulp."""
    k, n = 1152, 256
    _, qw, scale, _ = make_case(1, k, n, gs, 77 + gs, DEV)
    x = torch.zeros(len(PROBE_K), k, dtype=BF16, device=DEV)
    x[torch.arange(len(PROBE_K)), torch.tensor(PROBE_K)] = 1.0
    what = ref_what(qw, scale, gs)
    ref, bound = ref_and_bound(x, what)
    assert torch.equal(ref, what[torch.tensor(PROBE_K, device=DEV)])
    out = _C().decode_gemm_int4(x, qw, scale, None, gs, 4)
    check(f"one-hot gs{gs}", out, ref, bound)


# ---------------------------------------------------------------------------
# dequant_int4
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k,n,gs", [(64, 8, -1), (128, 264, 64), (384, 512, 128),
                                    (2, 40, -1)])
def test_dequant_int4_gpu(k, n, gs):
    """fp32 output is exact: every element is evaluated as
    float(q) * (scale * fp32(1/7)) -- two fp32 multiplies in that order --
    and must equal that expression evaluated by torch in fp32.  bf16 output
    is within one bf16 ulp of it."""
    _, qw, scale, _ = make_case(1, k, n, gs, 5 + k + n, DEV)
    q = ref_unpack(qw)
    s7 = ref_expand(scale, k, gs) * torch.tensor(1.0 / 7.0, dtype=F32, device=DEV)
    expect = q.to(F32) * s7
    out32 = _C().dequant_int4(qw, scale, gs, F32)
    assert out32.dtype == F32 and torch.equal(out32, expect)
    out16 = _C().dequant_int4(qw, scale, gs, BF16)
    assert out16.dtype == BF16
    err = (out16.double() - expect.double()).abs()
    assert bool((err <= U_BF16 * expect.double().abs()).all())
    # the public wrapper takes the same kernel on GPU tensors
    from paddle_amd.nn import quant as NQ
    got = NQ.weight_dequantize(qw, scale, algo="weight_only_int4",
                                            out_dtype=F32, group_size=gs)
    assert torch.equal(got, expect)


# ---------------------------------------------------------------------------
# weight_only_linear dispatch
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("rows,gs", [(4, 64), (4, -1), (40, 64), (40, 128)])
def test_weight_only_linear_int4_dispatch_gpu(rows, gs, monkeypatch):
    """rows 4 take the streamer, rows 40 dequant_int4 + matmul; both match
    the fp64 reference within the bound.  Rows 40 round the matmul result
    and the bias add to bf16 separately, as the torch composite does: the
    composite's own measured error E against fp64 is allowed on top."""
    from paddle_amd import quantization as Q
    k, n = 256, 512
    x, qw, scale, bias = make_case(rows, k, n, gs, 31 + rows + gs, DEV)
    x = x.reshape(rows // 2, 2, k)
    C = _C()
    calls = []
    real_gemm, real_deq = C.decode_gemm_int4, C.dequant_int4
    monkeypatch.setattr(C, "decode_gemm_int4",
                        lambda *a: (calls.append("gemm"), real_gemm(*a))[1])
    monkeypatch.setattr(C, "dequant_int4",
                        lambda *a: (calls.append("dequant"), real_deq(*a))[1])
    out = Q.weight_only_linear(x, qw, scale, bias, weight_dtype="int4",
                               group_size=gs)
    assert calls == (["gemm"] if rows <= 32 else ["dequant"])
    assert tuple(out.shape) == (rows // 2, 2, n)
    ref, bound = ref_and_bound(x.reshape(rows, k), ref_what(qw, scale, gs), bias)
    extra = 0.0
    if rows > 32:
        comp = (x.reshape(rows, k) @ Q._wo_int4_dequant_torch(qw, scale, gs).to(BF16)) + bias
        extra = float((comp.double() - ref).abs().max())
        print(f"[int4] composite E={extra:.3e}")
    check(f"dispatch rows{rows} gs{gs}", out.reshape(rows, n), ref, bound, extra)


# ---------------------------------------------------------------------------
# contract
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_decode_gemm_int4_contract_gpu():
    """Every off-contract direct _C call raises before any launch."""
    C = _C()

    def args(m=4, k=128, n=256, gs=64):
        x = torch.zeros(m, k, dtype=BF16, device=DEV)
        qw = torch.zeros(k // 2, n, dtype=torch.int8, device=DEV)
        shape = (n,) if gs == -1 else (max(k // gs, 1), n)
        return x, qw, torch.ones(shape, dtype=F32, device=DEV)

    x, qw, sc = args()
    assert tuple(C.decode_gemm_int4(x, qw, sc, None, 64, 0).shape) == (4, 256)
    bad = {
        "M=33": lambda: C.decode_gemm_int4(*args(m=33), None, 64, 0),
        "N=128": lambda: C.decode_gemm_int4(*args(n=128), None, 64, 0),
        "K=96": lambda: C.decode_gemm_int4(*args(k=96, gs=-1), None, -1, 0),
        "scale shape": lambda: C.decode_gemm_int4(x, qw, sc[:1], None, 64, 0),
        "scale per-channel for groups": lambda: C.decode_gemm_int4(
            x, qw, sc[0].contiguous(), None, 64, 0),
        "qw non-contiguous": lambda: C.decode_gemm_int4(
            x, torch.zeros(256, 64, dtype=torch.int8, device=DEV).t(), sc,
            None, 64, 0),
        "group_size=32": lambda: C.decode_gemm_int4(
            x, qw, torch.ones(4, 256, dtype=F32, device=DEV), None, 32, 0),
        "x fp32": lambda: C.decode_gemm_int4(x.float(), qw, sc, None, 64, 0),
        "qw K mismatch": lambda: C.decode_gemm_int4(x, qw[:32], sc[:1], None, 64, 0),
        "bias fp32": lambda: C.decode_gemm_int4(
            x, qw, sc, torch.zeros(256, device=DEV), 64, 0),
        "bias size": lambda: C.decode_gemm_int4(
            x, qw, sc, torch.zeros(128, dtype=BF16, device=DEV), 64, 0),
        "scale fp16": lambda: C.decode_gemm_int4(x, qw, sc.half(), None, 64, 0),
        "negative ksplit": lambda: C.decode_gemm_int4(x, qw, sc, None, 64, -1),
        "dequant N=12": lambda: C.dequant_int4(
            torch.zeros(32, 12, dtype=torch.int8, device=DEV),
            torch.ones(12, dtype=F32, device=DEV), -1, F32),
        "dequant fp16 out": lambda: C.dequant_int4(qw, sc, 64, torch.float16),
    }
    for name, call in bad.items():
        with pytest.raises(RuntimeError):
            call()
            pytest.fail(f"{name}: accepted")
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# hipGraph
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_weight_only_linear_int4_graph_gpu():
    """One capture + replay of weight_only_linear int4 equals eager
    bit-for-bit (no sync, no host read on the path)."""
    from paddle_amd import quantization as Q
    m, k, n, gs = 8, 256, 256, 64
    x, qw, scale, bias = make_case(m, k, n, gs, 99, DEV)

    def run(inp):
        return Q.weight_only_linear(inp, qw, scale, bias, weight_dtype="int4",
                                    group_size=gs)

    eager = run(x)
    static_x = x.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(static_x)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static_out = run(static_x)
    static_out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_out, eager)
    ref, bound = ref_and_bound(x, ref_what(qw, scale, gs), bias)
    check("graph replay", static_out, ref, bound)
