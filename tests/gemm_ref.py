"""fp64 references and the element-wise error rule for the dense MFMA GEMM
family (gemm.hip, gemm_fp8.hip) and for quant_fp8, shared by
test_gemm_ref_cpu.py, test_gemm_bounds_gpu.py, test_quant_fp8_gpu.py and
test_gemm_mx_gpu.py.

The rule (docs/KERNELS.md "Dense GEMM test bounds") for an fp32-accumulated
reduction of length K cast to bf16:

    |out - ref| <= roundings * 2^-7 * |ref| + K * 2^-24 * S_eff + extra_abs

roundings is 1, or 2 when a bias is added; S_eff is |A| @ |B| with whatever
else enters the fp32 sum (|c0| when accumulating, |scale_ab| as a factor for
fp8, where K + 1 stands for K because of the scale multiply).

The GELU epilogues evaluate a degree-5 erf polynomial and exp in fp32.  That
error belongs to the formula, not to the GEMM, so it is measured, not chosen:
gelu_poly_errors() evaluates the kernel's polynomials in torch fp32 at every
bf16 value in [-10, 10] against fp64 exact-erf GELU and GELU'.  Measured:

    GELU_POLY_ERR  = 4.5e-07   (max |gelu_fp32_poly(x)  - gelu(x)|)
    DGELU_POLY_ERR = 2.7e-07   (max |gelu'_fp32_poly(x) - gelu'(x)|)

(the constants below are the measured maxima rounded up to two digits;
test_gemm_ref_cpu.py measures again and compares).  extra_abs is twice the
constant, times |a @ b| for DGELU; the factor 2 is the margin for the device's
__expf against torch's exp.
"""
import math

import torch

GELU_POLY_ERR = 4.5e-07
DGELU_POLY_ERR = 2.7e-07
GELU_GRAD_MAX = 1.13          # max |gelu'(x)| = 1.1290 at x = sqrt(2)

LAYOUTS = ("nt", "nn", "tn")
NONE, BIAS, BIAS_GELU, DGELU = 0, 1, 2, 3
TILE = 256


# ---------------------------------------------------------------------------
# GELU: exact in fp64, and the kernel's polynomial in fp32
# ---------------------------------------------------------------------------
def gelu64(x):
    x = x.double()
    return 0.5 * x * (1.0 + torch.erf(x * math.sqrt(0.5)))


def gelu_grad64(x):
    x = x.double()
    cdf = 0.5 * (1.0 + torch.erf(x * math.sqrt(0.5)))
    return cdf + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def _erf_poly32(x):
    f = lambda v: torch.tensor(v, dtype=torch.float32)  # noqa: E731
    z = x * f(0.70710678118654752440)
    az = z.abs()
    t = f(1.0) / (f(1.0) + f(0.3275911) * az)
    p = t * (f(0.254829592) + t * (f(-0.284496736) + t * (f(1.421413741) +
             t * (f(-1.453152027) + t * f(1.061405429)))))
    r = f(1.0) - p * torch.exp(-az * az)
    return torch.copysign(r, z)


def epi_gelu32(x):
    """epi_gelu of gemm.hip, operation by operation in torch fp32."""
    x = x.float()
    return torch.tensor(0.5) * x * (torch.tensor(1.0) + _erf_poly32(x))


def epi_gelu_grad32(x):
    """epi_gelu_grad of gemm.hip in torch fp32."""
    x = x.float()
    cdf = torch.tensor(0.5) * (torch.tensor(1.0) + _erf_poly32(x))
    pdf = torch.tensor(0.3989422804014327) * torch.exp(torch.tensor(-0.5) * x * x)
    return cdf + x * pdf


def all_bf16():
    """Every bf16 bit pattern, in bit order."""
    return torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)


def gelu_poly_errors():
    """(max abs error of epi_gelu32, of epi_gelu_grad32) over every bf16 value
    in [-10, 10]."""
    x = all_bf16().float()
    x = x[x.abs() <= 10.0]
    e_g = (epi_gelu32(x).double() - gelu64(x)).abs().max().item()
    e_d = (epi_gelu_grad32(x).double() - gelu_grad64(x)).abs().max().item()
    return e_g, e_d


# ---------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------
def gemm_ref(a, b, layout="nt", epilogue=NONE, bias=None, aux=None, c0=None,
             scale_ab=None):
    """fp64 reference of one GEMM call on CPU tensors, 2-D or batched 3-D.

    a, b are the operands as stored: nt A[M,K] Bt[N,K]; nn A[M,K] B[K,N];
    tn At[K,M] B[K,N].  bias is [N] (or [batch, N]), aux the saved
    pre-activation of DGELU, c0 the accumulator's prior content, scale_ab the
    fp8 dequantisation scale.  Returns (ref, S_eff, K_eff, extra_abs, roundings):
    the arguments of check_bound for this call.  For BIAS_GELU ref is
    gelu(pre) in fp64; aux is checked by a second call with epilogue=BIAS.
    """
    assert layout in LAYOUTS
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    if layout == "tn":
        a = a.transpose(-1, -2)
    if layout == "nt":
        b = b.transpose(-1, -2)
    k = a.shape[-1]
    ab = a @ b
    s = a.abs() @ b.abs()
    keff, extra, roundings = k, 0.0, 1
    if scale_ab is not None:
        ab, s, keff = ab * scale_ab, s * abs(scale_ab), k + 1
    ref = ab
    if bias is not None:
        bb = bias.detach().cpu().double()
        ref = ab + (bb.unsqueeze(-2) if bb.dim() == 2 else bb)
        roundings = 2
    if epilogue == BIAS_GELU:
        assert bias is not None
        ref = gelu64(ref)
        s = GELU_GRAD_MAX * s
        extra = 2.0 * GELU_POLY_ERR
    elif epilogue == DGELU:
        g = gelu_grad64(aux.detach().cpu())
        ref = ab * g
        s = s * g.abs()
        extra = 2.0 * DGELU_POLY_ERR * ab.abs()
    if c0 is not None:
        c0 = c0.detach().cpu().double()
        ref = ref + c0
        s = s + c0.abs()
    return ref, s, keff, extra, roundings


def locate(flat_index, shape):
    """Coordinates of an output element in the kernels' terms."""
    cols = shape[-1]
    rows = shape[-2]
    batch, rem = divmod(flat_index, rows * cols)
    row, col = divmod(rem, cols)
    where = f"(row {row}, col {col})"
    if len(shape) == 3:
        where = f"batch {batch} " + where
    return (f"{where}: tile ({row // TILE}, {col // TILE}), "
            f"wave (wr {row % TILE // 128}, wc {col % TILE // 64}), "
            f"fragment (m {row % 128 // 16}, n {col % 64 // 16}), "
            f"in-fragment ({row % 16}, {col % 16})")


def check_bound(out, ref, S, K, extra_abs=0.0, roundings=1, tag=""):
    """Assert |out - ref| <= roundings 2^-7 |ref| + K 2^-24 S + extra_abs for
    every element: the project's rule for a reduced output cast to bf16.  A
    NaN or an Inf in out fails.  Prints the worst err/bound; returns it."""
    assert tuple(out.shape) == tuple(ref.shape), (tuple(out.shape), tuple(ref.shape))
    ref = ref.double()
    bound = roundings * 2.0 ** -7 * ref.abs() + K * 2.0 ** -24 * S.double() + extra_abs
    err = (out.double() - ref).abs()
    ratio = err / bound.clamp(min=1e-300)
    ratio = torch.where(torch.isfinite(err), ratio, torch.full_like(ratio, float("inf")))
    ratio = torch.where((err == 0) & (bound == 0), torch.zeros_like(ratio), ratio)
    worst = ratio.max().item()
    print(f"{tag}: worst err/bound {worst:.3f}")
    bad = ~(err <= bound)
    if bool(bad.any()):
        i = int(ratio.reshape(-1).argmax())
        raise AssertionError(
            f"{tag}: {int(bad.sum())} of {bad.numel()} elements out of bound; worst "
            f"err/bound {worst:.3f} at {locate(i, tuple(out.shape))}: "
            f"out {out.reshape(-1)[i].item()!r} ref {ref.reshape(-1)[i].item()!r} "
            f"bound {bound.reshape(-1)[i].item():.3e}")
    return worst


# ---------------------------------------------------------------------------
# which kernels a shape runs: gemm_plan / gemm_tile_origin of gemm_common.h
# ---------------------------------------------------------------------------
def gemm_path(layout, m, n, k, bk=64):
    """Port of gemm_plan.  bk is the K-step: 64 for bf16, 128 for fp8 (whose
    only layout is nt).  Grids are (tiles along M, tiles along N); a short
    band is the rasteriser's last band of fewer than 8 tile rows."""
    assert layout in LAYOUTS
    mi, ni = m // TILE, n // TILE
    gm, gn = -(-m // TILE), -(-n // TILE)
    has_fast = layout == "nt" and k % bk == 0 and mi > 0 and ni > 0
    has_edge = (not has_fast) or mi < gm or ni < gn

    def short_band(mt):
        return mt > 8 and mt % 8 != 0

    return {
        "has_fast": has_fast,
        "has_edge": has_edge,
        "nkt": -(-k // bk),
        "fast_grid": (mi, ni) if has_fast else None,
        "edge_grid": (gm, gn) if has_edge else None,
        "fast_nwg_mod8": (mi * ni) % 8 if has_fast else None,
        "edge_nwg_mod8": (gm * gn) % 8 if has_edge else None,
        "fast_short_band": has_fast and short_band(mi),
        "edge_short_band": has_edge and short_band(gm),
    }


def tile_order(mt, nt):
    """Port of gemm_tile_origin: (bm, bn) of every linear workgroup index of a
    grid of mt x nt tiles, in launch order."""
    nwg = mt * nt
    q, rr = divmod(nwg, 8)
    out = []
    for orig in range(nwg):
        xcd, pos = orig % 8, orig // 8
        o = (xcd * (q + 1) if xcd < rr else rr * (q + 1) + (xcd - rr) * q) + pos
        band, rem = divmod(o, 8 * nt)
        gm_band = min(mt - band * 8, 8)
        out.append((band * 8 + rem % gm_band, rem // gm_band))
    return out


# ---------------------------------------------------------------------------
# inputs shared by the CPU and GPU tests
# ---------------------------------------------------------------------------
def scaled_rows(rows, cols, gen, batch=None):
    """randn bf16 [rows, cols] whose rows carry magnitudes 2^randint(-3, 3), so
    that fragments differ in scale and a swapped fragment cannot hide."""
    shape = (rows, cols) if batch is None else (batch, rows, cols)
    x = torch.randn(*shape, generator=gen)
    e = torch.randint(-3, 4, shape[:-1] + (1,), generator=gen)
    return (x * torch.exp2(e.float())).to(torch.bfloat16)


def fp8_operand(rows, cols, gen, batch=None):
    shape = (rows, cols) if batch is None else (batch, rows, cols)
    return (torch.randn(*shape, generator=gen) * 0.3).to(torch.float8_e4m3fn)


# ---------------------------------------------------------------------------
# e4m3 (OCP e4m3fn): round to nearest even in fp64
# ---------------------------------------------------------------------------
E4M3_MAX = 448.0


def e4m3_encode(v):
    """Byte of the e4m3fn value nearest to v (ties to even): normals,
    subnormals down to 2^-9 and signed zero.  v: float tensor, every |v| <= 448
    (up to 464 still rounds to 448).  Returns uint8."""
    v = v.double()
    assert bool((v.abs() <= 464.0).all())
    sign = torch.signbit(v).to(torch.int64) << 7
    a = v.abs()
    _, ex = torch.frexp(a)                          # a = m 2^ex, m in [.5, 1)
    e = (ex.to(torch.int64) - 1).clamp(min=-6)       # subnormals share 2^-6
    quantum = torch.exp2((e - 3).double())
    val = torch.round(a / quantum) * quantum         # torch.round: ties to even
    _, ex2 = torch.frexp(val)
    e2 = ex2.to(torch.int64) - 1                     # val may have moved up a binade
    normal = (e2 + 7 << 3) + ((val / torch.exp2(e2.double()) - 1.0) * 8).to(torch.int64)
    subnormal = (val * 512.0).to(torch.int64)        # 0..7 times 2^-9
    mag = torch.where(e2 < -6, subnormal, normal)
    mag = torch.where(val == 0, torch.zeros_like(mag), mag)
    return (sign | mag).to(torch.uint8)


def e4m3_is_nan(byte):
    return (byte & 0x7F) == 0x7F
