"""MXFP4 weight-only decode on the GPU: the register-streamed fp4 W-streamer,
the dequantizer and their dispatch, against fp64 matmul on operands
dequantized by a plain torch reading of the format."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import paddle_amd as paddle
    from paddle_amd import _ext
    from paddle_amd import quantization as Q
    from paddle_amd.incubate import mx

DEV = "cuda:0"
GRID = torch.tensor([0, .5, 1, 1.5, 2, 3, 4, 6], dtype=torch.float64)


def ref_dequant(codes, scales):
    """fp64 [R, K] on the device of codes."""
    lut = torch.cat((GRID, -GRID)).to(codes.device)
    nib = torch.stack((codes & 15, codes >> 4), -1).reshape(codes.shape[0], -1).long()
    return lut[nib] * torch.exp2(scales.double() - 127).repeat_interleave(32, 1)


@functools.lru_cache(maxsize=None)
def operands(n, k):
    """Random blocks with per-block exponents (scale bytes differ per row and
    block), x for 40 rows, a bias, and the fp64 weight: built once per shape."""
    g = torch.Generator().manual_seed(n + k)
    w = torch.randn(n, k // 32, 32, generator=g) * torch.exp2(
        torch.randint(-4, 5, (n, k // 32, 1), generator=g).float())
    qw, s = mx.mx_quantize(w.reshape(n, k).to(torch.bfloat16).to(DEV))
    x = torch.randn(40, k, generator=g).to(torch.bfloat16).to(DEV)
    bias = torch.randn(n, generator=g).to(torch.bfloat16).to(DEV)
    return qw, s, x, bias, ref_dequant(qw, s)


def check_bound(out, x, wd, bias, tag):
    """|out - ref| <= 2^-7 |ref| + K 2^-24 sum_k |x_k w_k| (+ 2^-7 |ref| with a
    bias): the project's rule for a reduced output cast to bf16."""
    xd = x.double()
    ref = xd @ wd.t()
    if bias is not None:
        ref = ref + bias.double()
    bound = (2.0 ** -7 * (2 if bias is not None else 1)) * ref.abs() \
        + x.shape[1] * 2.0 ** -24 * (xd.abs() @ wd.abs().t())
    err = (out.double() - ref).abs()
    print(f"{tag}: worst err/bound {(err / bound.clamp(min=1e-300)).max().item():.3f}")
    assert out.dtype == torch.bfloat16 and out.shape == ref.shape
    assert bool((err <= bound).all())


@pytest.mark.parametrize("has_bias", [False, True])
@pytest.mark.parametrize("n,k,ksplit", [(64, 128, 0), (320, 384, 0),
                                        (256, 1024, 3), (576, 512, 1)])
@pytest.mark.parametrize("m", [1, 16, 17, 32])
def test_numerics(m, n, k, ksplit, has_bias):
    qw, s, x, bias, wd = operands(n, k)
    b = bias if has_bias else None
    out = _ext.get_ext().decode_gemm_mxfp4(x[:m], qw, s, b, ksplit)
    check_bound(out, x[:m], wd, b, f"M{m} N{n} K{k} ksplit{ksplit} bias={has_bias}")


@pytest.mark.parametrize("ksplit", [0, 1])
def test_scale_and_k_map_exact(ksplit):
    """x row m is 1.0 inside block m, every code is 1.0: y[m, n] is one block's
    sum, 32 * 2^(s[n, m] - 127).  A wrong scale byte per lane, or x and W
    disagreeing on the k order, changes a power of two."""
    n, k = 320, 1024
    x = torch.zeros(32, 32, 32)
    x[torch.arange(32), torch.arange(32)] = 1.0
    x = x.reshape(32, k).to(torch.bfloat16).to(DEV)
    qw = torch.full((n, k // 2), 0x22, dtype=torch.uint8, device=DEV)
    ni, j = torch.meshgrid(torch.arange(n), torch.arange(k // 32), indexing="ij")
    s = (127 + (7 * ni + 3 * j) % 13 - 6).to(torch.uint8).to(DEV)
    out = _ext.get_ext().decode_gemm_mxfp4(x, qw, s, None, ksplit)
    assert torch.equal(out.float(), (32 * torch.exp2(s.float() - 127)).t())


@pytest.mark.parametrize("rows,k", [(64, 128), (80, 384)])
def test_dequant_bit_equal(rows, k):
    """Every code byte under scale bytes 8, 120, 127, 134 and 247: each run of
    16 blocks holds bytes 0..255 once and shares one of the five scales."""
    flat = torch.arange(rows * k // 2)
    codes = (flat % 256).to(torch.uint8).reshape(rows, k // 2).to(DEV)
    blk = torch.arange(rows * k // 32)
    scales = torch.tensor([8, 120, 127, 134, 247], dtype=torch.uint8)[(blk // 16) % 5]
    scales = scales.reshape(rows, k // 32).to(DEV)
    got = _ext.get_ext().mx_dequant_fp4(codes, scales)
    want = mx.mx_dequantize(codes, scales).to(torch.bfloat16)
    assert got.shape == (rows, k) and got.dtype == torch.bfloat16
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


def test_dispatch():
    n, k = 320, 384
    qw, s, x, bias, wd = operands(n, k)
    direct = _ext.get_ext().decode_gemm_mxfp4(x[:8], qw, s, bias, 0)
    via = Q.weight_only_linear(x[:8], qw, s, bias, weight_dtype="mxfp4")
    assert torch.equal(via, direct)
    big = Q.weight_only_linear(x, qw, s, bias, weight_dtype="mxfp4")
    check_bound(big, x, wd, bias, "40 rows: dequant + linear")
    layer = mx.MXFP4Linear(qw, s, bias, activation="bf16")
    assert torch.equal(layer(x[:8]), direct) and torch.equal(layer(x), big)
    # the default activation is the unchanged fp4 x fp4 path
    qx, sx = mx.mx_quantize(x)
    assert torch.equal(mx.MXFP4Linear(qw, s, bias)(x), mx.mxfp4_gemm_nt(qx, sx, qw, s, bias))


def test_llama_runner_fused_qkv():
    from paddle_amd.models.llama import LlamaConfig, LlamaForCausalLM
    from paddle_amd.serving import LlamaModelRunner
    paddle.seed(0)
    cfg = LlamaConfig(vocab_size=512, hidden_size=1024, num_layers=2, num_heads=8,
                      num_kv_heads=8, intermediate_size=1024, max_seq_len=128)
    model = LlamaForCausalLM(cfg).to(device=DEV, dtype=torch.bfloat16).eval()
    runner = LlamaModelRunner(model, num_blocks=64, block_size=16, max_seq=128,
                              use_graphs=False, weight_only="mxfp4")
    kind, qw, sc, _ = runner._qkv_fused[0]
    assert kind == "mxfp4" and qw.shape == (3072, 512) and sc.shape == (3072, 32)
    a = runner.model.llama.layers[0].self_attn
    projs = (a.q_proj, a.k_proj, a.v_proj)
    wd = torch.cat([ref_dequant(p.qweight, p.scale) for p in projs])
    h = torch.randn(4, 1024, generator=torch.Generator().manual_seed(3))
    h = h.to(torch.bfloat16).to(DEV)
    check_bound(Q.weight_only_linear(h, qw, sc, weight_dtype="mxfp4"), h, wd, None, "fused qkv")
    check_bound(torch.cat([p(h) for p in projs], -1), h, wd, None, "module calls")


@pytest.mark.parametrize("case", ["m_33", "k_mod_128", "n_mod_64", "scale_shape",
                                  "codes_dtype", "misaligned_qweight", "cpu_tensor",
                                  "x_dtype"])
def test_contract(case):
    u8 = dict(dtype=torch.uint8, device=DEV)
    m, n, k = 8, 64, 256
    if case == "m_33":
        m = 33
    elif case == "k_mod_128":
        k = 192
    elif case == "n_mod_64":
        n = 96
    x = torch.zeros(m, k, dtype=torch.bfloat16, device=DEV)
    qw, s = torch.zeros(n, k // 2, **u8), torch.full((n, k // 32), 127, **u8)
    if case == "scale_shape":
        s = torch.full((n, k // 32 + 4), 127, **u8)
    elif case == "codes_dtype":
        qw = qw.to(torch.int8)
    elif case == "misaligned_qweight":
        qw = torch.zeros(n * k // 2 + 8, **u8)[8:].reshape(n, k // 2)
    elif case == "cpu_tensor":
        s = s.cpu()
    elif case == "x_dtype":
        x = x.float()
    with pytest.raises(RuntimeError, match="decode_gemm_mxfp4"):
        _ext.get_ext().decode_gemm_mxfp4(x, qw, s)
