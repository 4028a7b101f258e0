"""GPU numerics and contract of the dense MFMA GEMM family (gemm.hip,
gemm_fp8.hip) behind _C.gemm_bf16_ex / gemm_bf16_nt_batched / gemm_fp8_nt /
gemm_fp8_nt_batched, vs plain torch fp32 references."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from paddle_amd import _ext
    from paddle_amd.ops import functional as hot

    DEV = "cuda:0"


def _bf(x):
    return x.to(torch.bfloat16)


# ---------------------------------------------------------------------------
# gemm.hip: 8-phase MFMA GEMM, all layouts + epilogues (vs fp32 torch)
# ---------------------------------------------------------------------------
def _gemm_rel_ok(out, ref, tol=3e-2):
    err = (out.float() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-6)
    assert err < tol, f"relerr {err:.3e}"


@pytest.mark.parametrize("m,n,k", [(512, 512, 512), (768, 1024, 256),
                                   (2048, 2048, 4096)])
def test_gemm_nt_numerics(m, n, k):
    torch.manual_seed(1)
    C = _ext.get_ext()
    a = _bf(torch.randn(m, k, device=DEV))
    bt = _bf(torch.randn(n, k, device=DEV))
    out = C.gemm_bf16_ex(a, bt, 0)[0]
    _gemm_rel_ok(out, a.float() @ bt.float().t())


def test_gemm_fp8_batched_bias():
    torch.manual_seed(7)
    C = _ext.get_ext()
    e, m, n, k = 8, 256, 512, 256
    a = torch.randn(e, m, k, device=DEV).clamp(-2, 2)
    bt = torch.randn(e, n, k, device=DEV).clamp(-2, 2)
    bias = _bf(torch.randn(e, n, device=DEV))
    qa = (a * 16).to(torch.float8_e4m3fn)
    qb = (bt * 16).to(torch.float8_e4m3fn)
    s = 1.0 / 256
    out = C.gemm_fp8_nt_batched(qa, qb, s, bias)
    ref = torch.einsum("emk,enk->emn", qa.float(), qb.float()) * s \
        + bias.float().unsqueeze(1)
    _gemm_rel_ok(out, ref, tol=5e-2)


@pytest.mark.parametrize("e,m,n,k", [(4, 512, 512, 512), (8, 513, 1024, 4096),
                                     (64, 513, 4096, 1024)])
def test_gemm_nt_batched(e, m, n, k):
    torch.manual_seed(2)
    C = _ext.get_ext()
    a = _bf(torch.randn(e, m, k, device=DEV))
    bt = _bf(torch.randn(e, n, k, device=DEV))
    out = C.gemm_bf16_nt_batched(a, bt)
    ref = torch.einsum("emk,enk->emn", a.float(), bt.float())
    _gemm_rel_ok(out, ref)


@pytest.mark.parametrize("m,n,k", [(512, 512, 512), (2048, 1024, 2048)])
def test_gemm_nn_numerics(m, n, k):
    torch.manual_seed(2)
    C = _ext.get_ext()
    a = _bf(torch.randn(m, k, device=DEV))
    b = _bf(torch.randn(k, n, device=DEV))
    out = C.gemm_bf16_ex(a, b, 1)[0]
    _gemm_rel_ok(out, a.float() @ b.float())


@pytest.mark.parametrize("m,n,k", [(512, 512, 512), (1024, 2048, 2048)])
def test_gemm_tn_numerics(m, n, k):
    # wgrad: C[m,n] = At[k,m]^T @ B[k,n], reduction over k (the token dim)
    torch.manual_seed(3)
    C = _ext.get_ext()
    at = _bf(torch.randn(k, m, device=DEV))
    b = _bf(torch.randn(k, n, device=DEV))
    out = C.gemm_bf16_ex(at, b, 2)[0]
    _gemm_rel_ok(out, at.float().t() @ b.float(), tol=5e-2)


def test_gemm_boundary_tiles():
    # M/N not multiples of 256 exercise the guarded kernel + skip-interior
    torch.manual_seed(4)
    C = _ext.get_ext()
    for (m, n, k) in [(300, 520, 512), (512, 777, 256), (130, 200, 128),
                      (1000, 50304 % 2048 + 304, 512)]:
        a = _bf(torch.randn(m, k, device=DEV))
        bt = _bf(torch.randn(n, k, device=DEV))
        out = C.gemm_bf16_ex(a, bt, 0)[0]
        _gemm_rel_ok(out, a.float() @ bt.float().t())


def test_gemm_k_tail():
    # K not a multiple of 64: whole grid takes the guarded path
    torch.manual_seed(5)
    C = _ext.get_ext()
    a = _bf(torch.randn(512, 200, device=DEV))
    bt = _bf(torch.randn(512, 200, device=DEV))
    out = C.gemm_bf16_ex(a, bt, 0)[0]
    _gemm_rel_ok(out, a.float() @ bt.float().t())


def test_gemm_bias_epilogue():
    torch.manual_seed(6)
    C = _ext.get_ext()
    a = _bf(torch.randn(512, 512, device=DEV))
    bt = _bf(torch.randn(768, 512, device=DEV))
    bias = _bf(torch.randn(768, device=DEV))
    out = C.gemm_bf16_ex(a, bt, 0, 1, bias)[0]
    _gemm_rel_ok(out, a.float() @ bt.float().t() + bias.float())


def test_gemm_bias_gelu_epilogue():
    torch.manual_seed(7)
    C = _ext.get_ext()
    a = _bf(torch.randn(512, 512, device=DEV) * 0.5)
    bt = _bf(torch.randn(768, 512, device=DEV) * 0.05)
    bias = _bf(torch.randn(768, device=DEV) * 0.1)
    out, aux = C.gemm_bf16_ex(a, bt, 0, 2, bias)
    pre = a.float() @ bt.float().t() + bias.float()
    _gemm_rel_ok(aux, pre)
    _gemm_rel_ok(out, torch.nn.functional.gelu(pre), tol=4e-2)


def test_gemm_dgelu_epilogue():
    torch.manual_seed(8)
    C = _ext.get_ext()
    dy = _bf(torch.randn(512, 512, device=DEV))
    w = _bf(torch.randn(768, 512, device=DEV) * 0.05)   # NT B-operand [n,k]
    z = _bf(torch.randn(512, 768, device=DEV))          # saved pre-act
    out = C.gemm_bf16_ex(dy, w, 0, 3, None, z)[0]       # [512, 768]
    zf = z.float().requires_grad_(True)
    torch.nn.functional.gelu(zf).backward(dy.float() @ w.float().t())
    # out = (dy @ w^T) * gelu'(z)
    _gemm_rel_ok(out, zf.grad, tol=5e-2)


def test_gemm_accumulate():
    torch.manual_seed(9)
    C = _ext.get_ext()
    at = _bf(torch.randn(512, 512, device=DEV))
    b = _bf(torch.randn(512, 768, device=DEV))
    c0 = _bf(torch.randn(512, 768, device=DEV))
    acc = c0.clone()
    C.gemm_bf16_ex(at, b, 2, 0, None, None, acc)
    _gemm_rel_ok(acc, c0.float() + at.float().t() @ b.float(), tol=5e-2)


def test_fused_linear_own_grads():
    """fused_linear_own fwd+bwd vs fp32 autograd reference."""
    from paddle_amd.ops import gemm_dispatch
    torch.manual_seed(10)
    m, k, n = 1024, 512, 768
    x = _bf(torch.randn(2, m // 2, k, device=DEV)).requires_grad_(True)
    w = (_bf(torch.randn(k, n, device=DEV)) * 0.05).requires_grad_(True)
    bias = (_bf(torch.randn(n, device=DEV)) * 0.1).requires_grad_(True)
    y = hot.fused_linear_own(x, w, bias)
    loss = (y.float() ** 2).mean()
    loss.backward()
    xf = x.detach().float().requires_grad_(True)
    wf = w.detach().float().requires_grad_(True)
    bf_ = bias.detach().float().requires_grad_(True)
    yf = xf @ wf + bf_
    ((yf ** 2).mean()).backward()
    _gemm_rel_ok(y, yf.detach(), tol=4e-2)
    _gemm_rel_ok(x.grad, xf.grad, tol=5e-2)
    _gemm_rel_ok(w.grad, wf.grad, tol=5e-2)
    _gemm_rel_ok(bias.grad, bf_.grad, tol=5e-2)


# ---------------------------------------------------------------------------
# fp8 e4m3 MX GEMM (gemm_fp8.hip)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,k", [(512, 512, 512), (777, 300, 256),
                                   (2048, 1024, 4096)])
def test_gemm_fp8_numerics(m, n, k):
    torch.manual_seed(31)
    C = _ext.get_ext()
    a = (torch.randn(m, k, device=DEV) * 0.3).to(torch.float8_e4m3fn)
    bt = (torch.randn(n, k, device=DEV) * 0.3).to(torch.float8_e4m3fn)
    out = C.gemm_fp8_nt(a, bt, 0.731)
    ref = 0.731 * (a.float() @ bt.float().t())
    _gemm_rel_ok(out, ref, tol=2e-2)
    # bias epilogue
    bias = _bf(torch.randn(n, device=DEV))
    outb = C.gemm_fp8_nt(a, bt, 1.0, bias)
    _gemm_rel_ok(outb, a.float() @ bt.float().t() + bias.float(), tol=2e-2)




# ---------------------------------------------------------------------------
# edge kernel alone, per layout and with blockIdx.z > 0
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("e,m,n,k", [(3, 130, 200, 128), (2, 300, 264, 200)])
def test_gemm_nt_batched_edge_only(e, m, n, k):
    # no interior tile (and a K tail): the guarded kernel alone over grid.z,
    # the shape class of the MoE backward
    torch.manual_seed(12)
    C = _ext.get_ext()
    a = _bf(torch.randn(e, m, k, device=DEV))
    bt = _bf(torch.randn(e, n, k, device=DEV))
    out = C.gemm_bf16_nt_batched(a, bt)
    _gemm_rel_ok(out, torch.einsum("emk,enk->emn", a.float(), bt.float()))


def test_gemm_nn_boundary_tiles():
    torch.manual_seed(13)
    C = _ext.get_ext()
    m, n, k = 300, 520, 256
    a = _bf(torch.randn(m, k, device=DEV))
    b = _bf(torch.randn(k, n, device=DEV))
    _gemm_rel_ok(C.gemm_bf16_ex(a, b, 1)[0], a.float() @ b.float())


def test_gemm_tn_boundary_tiles():
    torch.manual_seed(14)
    C = _ext.get_ext()
    m, n, k = 300, 520, 256
    # At[k][m] is read by 16-byte accesses along m: M = 300 needs a row pitch
    # that is a multiple of 8 elements, so At is a view of a [k, 304] parent
    at = _bf(torch.randn(k, 304, device=DEV))[:, :m]
    b = _bf(torch.randn(k, n, device=DEV))
    _gemm_rel_ok(C.gemm_bf16_ex(at, b, 2)[0], at.float().t() @ b.float(), tol=5e-2)


def test_gemm_accumulate_nt_boundary():
    torch.manual_seed(15)
    C = _ext.get_ext()
    m, n, k = 300, 264, 128
    a = _bf(torch.randn(m, k, device=DEV))
    bt = _bf(torch.randn(n, k, device=DEV))
    c0 = _bf(torch.randn(m, n, device=DEV))
    acc = c0.clone()
    C.gemm_bf16_ex(a, bt, 0, 0, None, None, acc)
    _gemm_rel_ok(acc, c0.float() + a.float() @ bt.float().t(), tol=5e-2)


# ---------------------------------------------------------------------------
# the GemmArgs contract (csrc/kernels/api.h): every rule is refused in the
# binding with a message naming the operand, before anything is launched
# ---------------------------------------------------------------------------
def _z(*shape, dtype=torch.bfloat16, device=None):
    return torch.zeros(*shape, dtype=dtype, device=device or DEV)


def _f8(*shape, device=None):
    return _z(*shape, dtype=torch.uint8, device=device).view(torch.float8_e4m3fn)


def _ex(a, b, layout=0, epilogue=0, bias=None, aux=None, c_in=None):
    return _ext.get_ext().gemm_bf16_ex(a, b, layout, epilogue, bias, aux, c_in)


def _nb(a, bt):
    return _ext.get_ext().gemm_bf16_nt_batched(a, bt)


M_, N_, K_ = 64, 72, 128

BF16_CONTRACT = {
    # one GPU
    "b_cpu": (lambda: _ex(_z(M_, K_), _z(N_, K_, device="cpu")), "b must be on the device"),
    "bias_cpu": (lambda: _ex(_z(M_, K_), _z(N_, K_), 0, 1, _z(N_, device="cpu")), "bias must be on"),
    "aux_cpu": (lambda: _ex(_z(M_, K_), _z(N_, K_), 0, 3, None, _z(M_, N_, device="cpu")), "aux_in"),
    "c_in_cpu": (lambda: _ex(_z(M_, K_), _z(N_, K_), 0, 0, None, None, _z(M_, N_, device="cpu")), "c_in"),
    # dtypes
    "a_fp32": (lambda: _ex(_z(M_, K_, dtype=torch.float32), _z(N_, K_)), "a must be bfloat16"),
    "b_fp32": (lambda: _ex(_z(M_, K_), _z(N_, K_, dtype=torch.float32)), "b must be bfloat16"),
    "bias_fp32": (lambda: _ex(_z(M_, K_), _z(N_, K_), 0, 1, _z(N_, dtype=torch.float32)), "bias must be contiguous bfloat16"),
    "c_in_fp32": (lambda: _ex(_z(M_, K_), _z(N_, K_), 0, 0, None, None, _z(M_, N_, dtype=torch.float32)), "c_in"),
    # ranks and inner stride
    "a_1d": (lambda: _ex(_z(K_), _z(N_, K_)), "a must be 2-D"),
    "b_3d": (lambda: _ex(_z(M_, K_), _z(1, N_, K_)), "b must be 2-D"),
    "a_inner_stride": (lambda: _ex(_z(K_, M_).t(), _z(N_, K_)), "a must be 2-D with unit inner stride"),
    "batched_a_2d": (lambda: _nb(_z(M_, K_), _z(2, N_, K_)), "a must be 3-D"),
    "batched_bt_inner_stride": (lambda: _nb(_z(2, M_, K_), _z(2, K_, N_).transpose(1, 2)), "bt must be 3-D with unit inner stride"),
    "layout": (lambda: _ex(_z(M_, K_), _z(N_, K_), 3), "layout"),
    "epilogue": (lambda: _ex(_z(M_, K_), _z(N_, K_), 0, 4), "epilogue"),
    # inner dimensions
    "inner_nt": (lambda: _ex(_z(M_, K_), _z(N_, K_ + 8)), "inner dims of a and b"),
    "inner_nn": (lambda: _ex(_z(M_, K_), _z(K_ + 8, N_), 1), "inner dims of a and b"),
    "inner_tn": (lambda: _ex(_z(K_, M_), _z(K_ + 8, N_), 2), "inner dims of a and b"),
    "batch_mismatch": (lambda: _nb(_z(2, M_, K_), _z(3, N_, K_)), "same batch size"),
    # 16-byte accesses: leading dimensions, batch strides, base pointers
    "lda": (lambda: _ex(_z(M_, K_ + 4)[:, :K_], _z(N_, K_)), "a row and batch strides"),
    "ldb": (lambda: _ex(_z(M_, K_), _z(N_, K_ + 4)[:, :K_]), "b row and batch strides"),
    "ldb_nn": (lambda: _ex(_z(M_, K_), _z(K_, N_ + 4)[:, :N_], 1), "b row and batch strides"),
    "a_batch_stride": (lambda: _nb(_z(2 * (M_ * K_ + 4)).as_strided((2, M_, K_), (M_ * K_ + 4, K_, 1)),
                                   _z(2, N_, K_)), "a row and batch strides"),
    "a_base": (lambda: _ex(_z(M_, K_ + 8)[:, 1:K_ + 1], _z(N_, K_)), "a data must be 16-byte aligned"),
    "b_base": (lambda: _ex(_z(M_, K_), _z(N_, K_ + 8)[:, 1:K_ + 1]), "b data must be 16-byte aligned"),
    "bt_base_batched": (lambda: _nb(_z(2, M_, K_), _z(2, N_, K_ + 8)[:, :, 4:K_ + 4]), "bt data must be 16-byte aligned"),
    # sizes
    "k_min": (lambda: _ex(_z(M_, 32), _z(N_, 32)), "K must be >= 64"),
    "m_zero": (lambda: _ex(_z(0, K_), _z(N_, K_)), "1 <= M, N, K < 2^31"),
    "m_2_31": (lambda: _ex(_z(1, K_).expand(1 << 31, K_), _z(N_, K_)), "1 <= M, N, K < 2^31"),
    "n_2_31": (lambda: _ex(_z(M_, K_), _z(1, K_).expand(1 << 31, K_)), "1 <= M, N, K < 2^31"),
    "batch_65536": (lambda: _nb(_z(1, 1, K_).expand(65536, 1, K_), _z(1, 1, K_).expand(65536, 1, K_)), "batch <= 65535"),
    # accumulate, bias, aux
    "accumulate_epilogue": (lambda: _ex(_z(M_, K_), _z(N_, K_), 0, 1, _z(N_), None, _z(M_, N_)), "accumulate (c_in) requires epilogue 0"),
    "c_in_shape": (lambda: _ex(_z(M_, K_), _z(N_, K_), 0, 0, None, None, _z(M_, N_ + 8)), "c_in must be"),
    "bias_missing": (lambda: _ex(_z(M_, K_), _z(N_, K_), 0, 1), "bias must be given exactly"),
    "bias_missing_gelu": (lambda: _ex(_z(M_, K_), _z(N_, K_), 0, 2), "bias must be given exactly"),
    "bias_unread": (lambda: _ex(_z(M_, K_), _z(N_, K_), 0, 0, _z(N_)), "bias must be given exactly"),
    "bias_numel": (lambda: _ex(_z(M_, K_), _z(N_, K_), 0, 1, _z(N_ + 8)), "bias must have N elements"),
    "bias_strided": (lambda: _ex(_z(M_, K_), _z(N_, K_), 0, 1, _z(N_, 2)[:, 0]), "bias must be contiguous"),
    "aux_missing": (lambda: _ex(_z(M_, K_), _z(N_, K_), 0, 3), "aux_in must be given exactly"),
    "aux_unread": (lambda: _ex(_z(M_, K_), _z(N_, K_), 0, 0, None, _z(M_, N_)), "aux_in must be given exactly"),
    "aux_shape": (lambda: _ex(_z(M_, K_), _z(N_, K_), 0, 3, None, _z(M_, N_ + 8)), "aux_in must be a contiguous bfloat16 [M, N]"),
    "aux_strided": (lambda: _ex(_z(M_, K_), _z(N_, K_), 0, 3, None, _z(M_, N_ + 8)[:, :N_]), "aux_in must be a contiguous bfloat16 [M, N]"),
}


def _f1(a, bt, bias=None):
    return _ext.get_ext().gemm_fp8_nt(a, bt, 1.0, bias)


def _fb(a, bt, bias=None):
    return _ext.get_ext().gemm_fp8_nt_batched(a, bt, 1.0, bias)


FP8_CONTRACT = {
    "bt_cpu": (lambda: _f1(_f8(M_, K_), _f8(N_, K_, device="cpu")), "bt must be on the device"),
    "bias_cpu": (lambda: _f1(_f8(M_, K_), _f8(N_, K_), _z(N_, device="cpu")), "bias must be on"),
    "a_bf16": (lambda: _f1(_z(M_, K_), _f8(N_, K_)), "a must be float8_e4m3fn or uint8"),
    "bt_fp32": (lambda: _f1(_f8(M_, K_), _z(N_, K_, dtype=torch.float32)), "bt must be float8_e4m3fn or uint8"),
    "bt_bf16_batched": (lambda: _fb(_f8(2, M_, K_), _z(2, N_, K_)), "bt must be float8_e4m3fn or uint8"),
    "bias_fp32": (lambda: _f1(_f8(M_, K_), _f8(N_, K_), _z(N_, dtype=torch.float32)), "bias must be contiguous bfloat16"),
    "a_3d": (lambda: _f1(_f8(1, M_, K_), _f8(N_, K_)), "a must be 2-D"),
    "batched_bt_2d": (lambda: _fb(_f8(2, M_, K_), _f8(N_, K_)), "bt must be 3-D"),
    "a_inner_stride": (lambda: _f1(_f8(K_, M_).t(), _f8(N_, K_)), "a must be 2-D with unit inner stride"),
    "inner": (lambda: _f1(_f8(M_, K_), _f8(N_, K_ + 16)), "inner dims of a and bt"),
    "batch_mismatch": (lambda: _fb(_f8(2, M_, K_), _f8(3, N_, K_)), "same batch size"),
    "lda": (lambda: _f1(_f8(M_, K_ + 8)[:, :K_], _f8(N_, K_)), "a row and batch strides"),
    "ldb": (lambda: _f1(_f8(M_, K_), _f8(N_, K_ + 8)[:, :K_]), "bt row and batch strides"),
    "bt_batch_stride": (lambda: _fb(_f8(2, M_, K_),
                                    _f8(2 * (N_ * K_ + 8)).as_strided((2, N_, K_), (N_ * K_ + 8, K_, 1))),
                        "bt row and batch strides"),
    "a_base": (lambda: _f1(_f8(M_, K_ + 16)[:, 8:K_ + 8], _f8(N_, K_)), "a data must be 16-byte aligned"),
    "bt_base": (lambda: _f1(_f8(M_, K_), _f8(N_, K_ + 16)[:, 1:K_ + 1]), "bt data must be 16-byte aligned"),
    "k_min": (lambda: _f1(_f8(M_, 64), _f8(N_, 64)), "K must be >= 128"),
    "m_zero": (lambda: _f1(_f8(0, K_), _f8(N_, K_)), "1 <= M, N, K < 2^31"),
    "n_2_31": (lambda: _f1(_f8(M_, K_), _f8(1, K_).expand(1 << 31, K_)), "1 <= M, N, K < 2^31"),
    "batch_65536": (lambda: _fb(_f8(1, 1, K_).expand(65536, 1, K_), _f8(1, 1, K_).expand(65536, 1, K_)), "batch <= 65535"),
    "bias_numel": (lambda: _f1(_f8(M_, K_), _f8(N_, K_), _z(N_ + 8)), "bias must have N elements"),
    "bias_batched_shape": (lambda: _fb(_f8(2, M_, K_), _f8(2, N_, K_), _z(N_)), "bias must be [batch, N]"),
}


@pytest.mark.parametrize("case", sorted(BF16_CONTRACT))
def test_gemm_bf16_contract(case):
    call, message = BF16_CONTRACT[case]
    with pytest.raises(RuntimeError) as exc:
        call()
    assert message in str(exc.value), str(exc.value)
    assert "gemm_bf16_" in str(exc.value)


@pytest.mark.parametrize("case", sorted(FP8_CONTRACT))
def test_gemm_fp8_contract(case):
    call, message = FP8_CONTRACT[case]
    with pytest.raises(RuntimeError) as exc:
        call()
    assert message in str(exc.value), str(exc.value)
    assert "gemm_fp8_nt" in str(exc.value)
