"""MXFP4 on the GPU: the scaled-MFMA probe, the quantizer, the GEMM and the
Linear built on them, against a plain torch quantizer of the public rule and
fp64 matmul on dequantized operands."""
import pytest
import torch

import gemm_ref  # noqa: E402

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import paddle_amd as paddle
    from paddle_amd import _ext
    from paddle_amd.incubate import mx

DEV = "cuda:0"
GRID = torch.tensor([0, .5, 1, 1.5, 2, 3, 4, 6], dtype=torch.float64)


def ref_quant(x):
    """The rule of the format, in fp64 on the CPU: x [R, K] -> codes, scales."""
    r, k = x.shape
    b = x.detach().cpu().double().reshape(r, k // 32, 32)
    amax = b.abs().amax(-1)
    _, ex = torch.frexp(amax)                       # amax = m * 2^ex, m in [.5, 1)
    e = torch.where(amax == 0, torch.zeros_like(ex), (ex - 3).clamp(-127, 127))
    y = torch.ldexp(b.abs(), -e.unsqueeze(-1))
    d = (y.unsqueeze(-1) - GRID).abs()
    near = d == d.amin(-1, keepdim=True)            # one code, or two on a tie
    even = near & torch.tensor([True, False] * 4)
    code = torch.where(near.sum(-1) == 2, even.int().argmax(-1), near.int().argmax(-1))
    code = (code + 8 * (b < 0)).reshape(r, k // 2, 2)
    return ((code[..., 0] + 16 * code[..., 1]).to(torch.uint8),
            (e + 127).to(torch.uint8))


def ref_dequant(codes, scales):
    """fp64 [R, K] on the device of codes."""
    lut = torch.cat((GRID, -GRID)).to(codes.device)
    nib = torch.stack((codes & 15, codes >> 4), -1).reshape(codes.shape[0], -1).long()
    return lut[nib] * torch.exp2(scales.double() - 127).repeat_interleave(32, 1)


def no_neg_zero(codes):
    lo, hi = codes & 15, codes >> 4
    lo, hi = lo * (lo != 8), hi * (hi != 8)
    return lo + 16 * hi


@pytest.mark.parametrize("opsel", [0, 1, 2, 3])
def test_probe(opsel):
    """Nibble order, k window per lane, and that the scale applied is byte
    `opsel` of the lane's own register: c equals the fp64 result exactly."""
    g = torch.Generator().manual_seed(40 + opsel)
    a = torch.randint(0, 256, (16, 64), generator=g, dtype=torch.uint8)
    bt = torch.randint(0, 256, (16, 64), generator=g, dtype=torch.uint8)
    sa, sb = (torch.stack([124 + torch.randperm(7, generator=g)[:4] for _ in range(16)])
              .to(torch.uint8) for _ in range(2))
    c = _ext.get_ext().mfma_probe_fp4mx(a.to(DEV), bt.to(DEV), sa.to(DEV), sb.to(DEV), opsel)
    ref = (ref_dequant(a, sa) @ ref_dequant(bt, sb).t()).float()
    assert torch.equal(c.cpu(), ref)


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("shape", [(1, 32), (3, 96), (257, 4096)])
def test_quantizer(shape, strided):
    r, k = shape
    g = torch.Generator().manual_seed(r + k)
    nb = k // 32
    x = torch.randn(r, nb, 32, generator=g) * torch.exp2(
        torch.randint(-20, 21, (r, nb, 1), generator=g).float())
    ties = torch.tensor([.25, .75, 1.25, 1.75, 2.5, 3.5, 5, 7])
    x[0, 0] = torch.cat((ties, -ties, torch.rand(16, generator=g))) * 2.0 ** 5
    if nb > 1:
        x[r // 2, 1] = 0                                          # all-zero block
        x[r - 1, nb - 1] = torch.rand(32, generator=g) * 2.0 ** -9
        x[r - 1, nb - 1, 7] = -2.0 ** -9                          # amax a power of two
    x = x.reshape(r, k).to(torch.bfloat16)
    xd = x.to(DEV)
    if strided:
        wide = torch.zeros(r, k + 64, dtype=torch.bfloat16, device=DEV)
        wide[:, 32:32 + k] = xd
        xd = wide[:, 32:32 + k]
    codes, scales = _ext.get_ext().mx_quant_fp4(xd)
    ref_codes, ref_scales = ref_quant(x)
    assert torch.equal(scales.cpu(), ref_scales)
    assert torch.equal(no_neg_zero(codes.cpu()), no_neg_zero(ref_codes))


@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("m,k", [(256, 8192), (40, 640)])
def test_scale_map_exact(m, k, swap):
    """Which scale byte multiplies which (row, k-block): every output is one
    block's sum, 32 * 2^(scale - 127), a power of two."""
    nb = k // 32
    ones = torch.full((m, k // 2), 0x22, dtype=torch.uint8, device=DEV)
    mi, j = torch.meshgrid(torch.arange(m), torch.arange(nb), indexing="ij")
    s_ones = (127 + (7 * mi + 3 * j) % 13 - 6).to(torch.uint8).to(DEV)
    sel = torch.zeros(nb, nb, 16, dtype=torch.uint8, device=DEV)
    sel[torch.arange(nb), torch.arange(nb)] = 0x22      # row j: 1.0 inside block j
    sel = sel.reshape(nb, k // 2)
    s_sel = torch.full((nb, nb), 127, dtype=torch.uint8, device=DEV)
    want = 32 * torch.exp2(s_ones.float() - 127)
    if swap:
        out = mx.mxfp4_gemm_nt(sel, s_sel, ones, s_ones)
        want = want.t()
    else:
        out = mx.mxfp4_gemm_nt(ones, s_ones, sel, s_sel)
    assert torch.equal(out.float(), want)


def mx_operand(rows, k, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, k // 32, 32, generator=g) * torch.exp2(
        torch.randint(-4, 5, (rows, k // 32, 1), generator=g).float())
    return mx.mx_quantize(x.reshape(rows, k).to(torch.bfloat16).to(DEV))


def check_bound(out, a, b, bias, tag):
    """|out - ref| <= 2^-7 |ref| + K 2^-24 sum_k |a_k b_k| (+ 2^-7 |ref| with a
    bias): the project's rule for a reduced output cast to bf16 (gemm_ref.py)."""
    ref = a @ b.t()
    if bias is not None:
        ref = ref + bias.double()
    gemm_ref.check_bound(out, ref, a.abs() @ b.abs().t(), a.shape[1],
                         roundings=2 if bias is not None else 1, tag=tag)


@pytest.mark.parametrize("has_bias", [False, True])
@pytest.mark.parametrize("m,n,k", [(256, 256, 256), (256, 256, 768), (512, 768, 1024),
                                   (300, 260, 512), (257, 300, 384), (1, 8, 128)])
def test_gemm_numerics(m, n, k, has_bias):
    qa, sa = mx_operand(m, k, 1)
    qb, sb = mx_operand(n, k, 2)
    bias = torch.randn(n, device=DEV).to(torch.bfloat16) if has_bias else None
    out = mx.mxfp4_gemm_nt(qa, sa, qb, sb, bias)
    assert out.dtype == torch.bfloat16 and out.shape == (m, n)
    check_bound(out, ref_dequant(qa, sa), ref_dequant(qb, sb), bias,
                f"gemm {m}x{n}x{k} bias={has_bias}")


def test_linear_and_convert():
    torch.manual_seed(7)
    lin = paddle.nn.Linear(512, 384).to(device=DEV, dtype=torch.bfloat16)
    with torch.no_grad():
        lin.bias.copy_(torch.randn(384))
    layer = mx.MXFP4Linear.from_linear(lin)
    assert layer.qweight.shape == (384, 256) and layer.weight_scale.shape == (384, 16)
    x = torch.randn(2, 5, 512, device=DEV).to(torch.bfloat16)
    out = layer(x)
    assert out.shape == (2, 5, 384)
    qx, sx = mx.mx_quantize(x.reshape(10, 512))
    check_bound(out.reshape(10, 384), ref_dequant(qx, sx),
                ref_dequant(layer.qweight, layer.weight_scale), layer.bias, "linear")
    with pytest.raises(RuntimeError, match="forward only"):
        layer(x.clone().requires_grad_())

    model = torch.nn.Module()
    model.fc1 = paddle.nn.Linear(512, 384).to(device=DEV, dtype=torch.bfloat16)
    model.fc2 = paddle.nn.Linear(320, 384).to(device=DEV, dtype=torch.bfloat16)
    assert mx.convert_linears_to_mxfp4(model) == 1
    assert isinstance(model.fc1, mx.MXFP4Linear) and not isinstance(model.fc2, mx.MXFP4Linear)


@pytest.mark.parametrize("case", ["scale_shape", "codes_dtype", "k_mod_128", "k_mismatch",
                                  "misaligned_row", "cpu_tensor", "quant_fp32"])
def test_contract(case):
    C = _ext.get_ext()
    u8 = dict(dtype=torch.uint8, device=DEV)
    a, sa = torch.zeros(16, 128, **u8), torch.full((16, 8), 127, **u8)
    b, sb = torch.zeros(8, 128, **u8), torch.full((8, 8), 127, **u8)
    name = "gemm_mxfp4_nt"
    if case == "scale_shape":
        sb = torch.full((8, 4), 127, **u8)
    elif case == "codes_dtype":
        a = a.to(torch.int8)
    elif case == "k_mod_128":
        a, sa = torch.zeros(16, 96, **u8), torch.full((16, 6), 127, **u8)
        b, sb = torch.zeros(8, 96, **u8), torch.full((8, 6), 127, **u8)
    elif case == "k_mismatch":
        b, sb = torch.zeros(8, 64, **u8), torch.full((8, 4), 127, **u8)
    elif case == "misaligned_row":
        a = torch.zeros(16, 136, **u8)[:, :128]
    elif case == "cpu_tensor":
        a = a.cpu()
    with pytest.raises(RuntimeError, match="mx_quant_fp4" if case == "quant_fp32" else name):
        if case == "quant_fp32":
            C.mx_quant_fp4(torch.zeros(4, 64, device=DEV))
        else:
            C.gemm_mxfp4_nt(a, sa, b, sb)
