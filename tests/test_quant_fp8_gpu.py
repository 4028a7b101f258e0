"""quant_fp8 (gemm_fp8.hip): bf16 -> e4m3 with a uniform fp32 scale, against
the fp64 round-to-nearest-even encoder of gemm_ref.py (itself checked against
torch's cast in test_gemm_ref_cpu.py): bit-exact over every bf16 value, the
out-of-range contract, the per-tensor recipe of incubate/fp8.py for every
possible amax, the grid-stride loop, and what the binding refuses."""
import pytest
import torch

from gemm_ref import all_bf16, e4m3_encode, e4m3_is_nan  # noqa: E402

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from paddle_amd import _ext
    from paddle_amd.incubate import fp8

DEV = "cuda:0"
BF = torch.bfloat16
SCALES = (1.0, 0.731, 2.0 ** -3, 37.0, 448.0 / 3.0)
TIE_SCALES = (1.0, 2.0 ** -3, 448.0 / 3.0)
GRID_STRIDE = 2048 * 256 * 8          # elements one pass of the full grid covers


def quant(x, scale):
    out = _ext.get_ext().quant_fp8(x, scale)
    assert out.dtype == torch.float8_e4m3fn and out.shape == x.shape
    return out.view(torch.uint8).cpu()


def scaled(x, scale):
    """fp32(x) * fp32(scale) in fp32, as the kernel forms it."""
    return x.float() * torch.tensor(scale, dtype=torch.float32)


def mismatch_report(got, want, v, limit=8):
    bad = (got != want).nonzero().flatten()
    head = ", ".join(f"v={v[i].item()!r}: got 0x{got[i].item():02X} want 0x{want[i].item():02X}"
                     for i in bad[:limit].tolist())
    return f"{bad.numel()} mismatches; first: {head}"


def check_in_range(got, x, scale):
    """Every element with finite |v| <= 448 is the RNE encoding of v, sign of
    zero included; returns the mask of those elements."""
    v = scaled(x, scale)
    ok = torch.isfinite(v) & (v.abs() <= 448.0)
    want = e4m3_encode(v[ok])
    assert torch.equal(got[ok], want), mismatch_report(got[ok], want, v[ok])
    return ok, v


@pytest.mark.parametrize("scale", SCALES)
def test_every_bf16_value(scale):
    x = all_bf16()
    assert x.numel() % 8 == 0
    got = quant(x.to(DEV), scale)
    ok, v = check_in_range(got, x, scale)
    # out of range (finite |v| > 448, +-Inf, NaN): +-448 or a NaN byte, never
    # another finite value; see csrc/kernels/api.h for what the kernel gives
    rest = got[~ok]
    assert bool((((rest & 0x7F) == 0x7E) | e4m3_is_nan(rest)).all()), \
        sorted(set(rest.tolist()))[:8]
    # the inputs do hold the hard cases
    vo = v[ok].double()
    steps = vo.abs() / torch.exp2((torch.frexp(vo.abs())[1] - 1).clamp(min=-6).double() - 3)
    if scale in TIE_SCALES:     # no bf16 * 0.731 or * 37 is a tie: the vector below has them
        assert bool(((steps - steps.floor()) == 0.5).any()), "no exact tie"
    assert bool(((vo.abs() >= 2.0 ** -10) & (vo.abs() < 2.0 ** -6)).any()), "no subnormal"
    assert 0x00 in got[ok].tolist() and 0x80 in got[ok].tolist()


def test_ties_subnormals_zeros_by_hand():
    """Explicit vector, scale 1: ties to even, the subnormal range, both zeros."""
    exact = torch.tensor([0.0, -0.0, 2.0 ** -9, 2.0 ** -10, 3 * 2.0 ** -10, -(2.0 ** -10),
                          1.0625, 1.1875, -1.0625, 17.0, 448.0, -448.0, 5 * 2.0 ** -10,
                          2.0 ** -11, 7.5 * 2.0 ** -9, 240.0], dtype=torch.float64)
    v = exact.to(BF)
    assert torch.equal(v.double(), exact)
    want = [0x00, 0x80, 0x01, 0x00, 0x02, 0x80, 0x38, 0x3A, 0xB8, 0x58, 0x7E, 0xFE,
            0x02, 0x00, 0x08, 0x77]
    assert e4m3_encode(v.float()).tolist() == want
    assert quant(v.to(DEV), 1.0).tolist() == want


def test_out_of_range_and_non_finite():
    """Finite |v| > 448, +-Inf and NaN give +-448 (0x7E / 0xFE) or a NaN byte,
    never another finite value; the neighbours in the same 8-group are exact.
    What the kernel gives is printed, and recorded in csrc/kernels/api.h."""
    inf, nan = float("inf"), float("nan")
    x = torch.tensor([450.0, -450.0, 462.0, -462.0, 464.0, -464.0, 480.0, 1e30, -3e38,
                      inf, -inf, nan, 448.0, -448.0, 1.0, 0.0], dtype=torch.float64).to(BF)
    assert x[:9].tolist() == [450.0, -450.0, 462.0, -462.0, 464.0, -464.0, 480.0,
                              x[7].item(), x[8].item()] and bool(torch.isfinite(x[:9].float()).all())
    got = quant(x.to(DEV), 1.0)
    print("quant_fp8 out of range:", [f"{a!r}->0x{b:02X}" for a, b in zip(x.tolist(), got.tolist())])
    assert got[12:].tolist() == [0x7E, 0xFE, 0x38, 0x00]
    assert bool((((got[:12] & 0x7F) == 0x7E) | e4m3_is_nan(got[:12])).all())
    # a product of finite factors that overflows fp32
    got = quant(torch.full((8,), 3e38, dtype=BF, device=DEV), 1e30)
    print("quant_fp8 3e38 * 1e30:", [f"0x{b:02X}" for b in got.tolist()])
    assert bool((((got & 0x7F) == 0x7E) | e4m3_is_nan(got)).all())


def production_amax():
    x = all_bf16()
    x = x[torch.isfinite(x.float()) & (x.float() >= 1e-12)]
    return x


def test_production_recipe_every_amax():
    """scale = fp32(448) / fp32(amax) as incubate/fp8.py forms it: amax itself
    must come out as +-448 for every possible bf16 amax, although
    fp32(amax * scale) can be the fp32 next above 448.  One launch per amax
    (the scale is a launch argument), a few seconds in all."""
    amax = production_amax()
    assert 20000 < amax.numel() < 33000
    a32 = amax.float()
    scales = (fp8.E4M3_MAX / a32.to(DEV).clamp(min=1e-12)).cpu()   # as _Fp8GroupedFFN does
    assert scales.dtype == torch.float32
    assert bool(((a32 * scales) > 448.0).any()), "no amax whose product exceeds 448"
    x = torch.zeros(amax.numel(), 8, dtype=BF)
    x[:, 0], x[:, 1] = amax, -amax
    x[:, 2], x[:, 3] = amax * 0.5, -amax * 0.5
    x[:, 4] = amax * 0.001953125
    xd = x.to(DEV)
    C = _ext.get_ext()
    out = torch.stack([C.quant_fp8(xd[i], s) for i, s in enumerate(scales.tolist())])
    got = out.view(torch.uint8).cpu()
    assert got[:, 0].tolist() == [0x7E] * amax.numel(), \
        [f"amax {amax[i].item()!r}: 0x{got[i, 0].item():02X}"
         for i in (got[:, 0] != 0x7E).nonzero().flatten()[:8].tolist()]
    assert got[:, 1].tolist() == [0xFE] * amax.numel()
    v = x.float() * scales[:, None]
    inside = v.abs() <= 448.0
    inside[:, :2] = False
    assert torch.equal(got[inside], e4m3_encode(v[inside]))


def test_matches_fp8_quant_of_the_training_path():
    g = torch.Generator().manual_seed(77)
    x = torch.randn(512, 384, generator=g).to(BF).to(DEV)
    C = _ext.get_ext()
    ax = C.amax_abs(x).clamp(min=1e-12)
    got = C.quant_fp8(x, float(fp8.E4M3_MAX / ax))
    want = fp8._quant(x)[0]
    assert torch.equal(got.view(torch.uint8), want.view(torch.uint8))


@pytest.mark.parametrize("numel", [GRID_STRIDE + 8, 3 * GRID_STRIDE + 4096])
def test_grid_stride_loop(numel):
    """More 8-element groups than threads in the capped grid, with a tail of
    one group (resp. 512) past the last full stride."""
    assert numel % 8 == 0 and numel % GRID_STRIDE in (8, 4096)
    g = torch.Generator().manual_seed(numel % 1000)
    x = (torch.randn(numel, generator=g) * 50).to(BF)
    x[-8:] = torch.tensor([1, -2, 3, -4, 448, -448, 0.5, -0.0], dtype=BF)
    got = quant(x.to(DEV), 0.731)
    # the reference of every element, through a table over the 65536 inputs
    v = scaled(all_bf16(), 0.731)
    inside = torch.isfinite(v) & (v.abs() <= 448.0)
    table = torch.zeros(65536, dtype=torch.uint8)
    table[inside] = e4m3_encode(v[inside])
    bits = x.view(torch.int16).long() & 0xFFFF
    assert bool(inside[bits].all())
    want = table[bits]
    assert torch.equal(got, want), mismatch_report(got, want, scaled(x, 0.731))
    assert got[-8:].tolist() == e4m3_encode(x[-8:].float() * torch.tensor(0.731)).tolist()


@pytest.mark.parametrize("case", ["numel", "dtype", "cpu", "strided"])
def test_binding_contract(case):
    x = {"numel": lambda: torch.zeros(12, dtype=BF, device=DEV),
         "dtype": lambda: torch.zeros(16, dtype=torch.float16, device=DEV),
         "cpu": lambda: torch.zeros(16, dtype=BF),
         "strided": lambda: torch.zeros(16, 2, dtype=BF, device=DEV)[:, 0]}[case]()
    message = {"numel": "numel must be a multiple of 8", "dtype": "x must be bfloat16",
               "cpu": "x must be a contiguous GPU tensor",
               "strided": "x must be a contiguous GPU tensor"}[case]
    with pytest.raises(RuntimeError) as exc:
        _ext.get_ext().quant_fp8(x, 1.0)
    assert "quant_fp8" in str(exc.value) and message in str(exc.value), str(exc.value)
