"""Dense MFMA GEMM family (gemm.hip, gemm_fp8.hip) against the fp64 reference
of gemm_ref.py, element by element, at the shapes where the kernels change
path: fast-pipeline depth 1..5, the fast + edge launch pair, the guarded
staging's partial 16-byte chunk along K, M and N, one-row operands, row and
batch strides larger than the matrix, strided c_in, the rasteriser's short last
band with an XCD remainder, and batches.  Every case asserts with gemm_path
that it runs the kernels it is meant to run.

Every operand is a slice of a parent filled with NaN (one row above and below,
which also separates batches, and the columns up to the row stride), so a read
outside the logical operand poisons the output.  The exact tests at the end
trace indices with one-hot operands and need no error model."""
import pytest
import torch

from gemm_ref import (BIAS, NONE, check_bound, fp8_operand, gemm_path, gemm_ref,  # noqa: E402
                      scaled_rows)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from paddle_amd import _ext

DEV = "cuda:0"
BF = torch.bfloat16
F8 = torch.float8_e4m3fn
LAY = {"nt": 0, "nn": 1, "tn": 2}
VARIANTS = ("none", "bias", "bias_gelu", "dgelu", "accumulate")


def ext():
    return _ext.get_ext()


def up(x, q):
    return -(-x // q) * q


def embed(t, extra=0):
    """CPU [.., R, C] -> the same values on the GPU as a view of a NaN parent
    [.., R + 2, ld]: ld is C rounded up to 16 bytes plus `extra` columns, and
    the view is the parent's right-hand slice [1:R+1, extra:extra+C]."""
    fp8 = t.dtype == F8
    q = 16 if fp8 else 8
    assert extra % q == 0
    *lead, r, c = t.shape
    ld = up(c, q) + extra
    if fp8:
        parent = torch.full((*lead, r + 2, ld), 0x7F, dtype=torch.uint8, device=DEV)
        parent[..., 1:r + 1, extra:extra + c] = t.view(torch.uint8).to(DEV)
        parent = parent.view(F8)
    else:
        parent = torch.full((*lead, r + 2, ld), float("nan"), dtype=BF, device=DEV)
        parent[..., 1:r + 1, extra:extra + c] = t.to(DEV)
    view = parent[..., 1:r + 1, extra:extra + c]
    assert view.stride(-2) == ld and view.data_ptr() % 16 == 0
    return view


def operands(layout, m, n, k, seed, batch=None, make=scaled_rows):
    """Logical A [M, K] and B' [N, K] of the recipe, stored as the layout asks."""
    g = torch.Generator().manual_seed(seed)
    a, b = make(m, k, g, batch), make(n, k, g, batch)
    if layout == "tn":
        a = a.transpose(-1, -2).contiguous()
    if layout != "nt":
        b = b.transpose(-1, -2).contiguous()
    return a, b, g


def dev(t):
    return None if t is None else t.to(DEV)


def run_bf16(layout, m, n, k, variant="none", extra=0, c_strided=False, seed=0):
    """One gemm_bf16_ex call against the reference.  Returns the raw outputs."""
    a, b, g = operands(layout, m, n, k, 100 + seed)
    bias = aux = c0 = None
    if variant in ("bias", "bias_gelu"):
        bias = torch.randn(n, generator=g).to(BF)
    if variant == "dgelu":
        aux = torch.randn(m, n, generator=g).to(BF)
    if variant == "accumulate":
        c0 = scaled_rows(m, n, g)
    epi = 0 if variant == "accumulate" else VARIANTS.index(variant)
    c_in = parent = None
    if c0 is not None and c_strided:
        # c_in as a column slice of a NaN-free parent that must stay untouched
        parent = torch.randn(m + 2, n + 24, generator=g).to(BF).to(DEV)
        parent[1:m + 1, 8:8 + n] = c0.to(DEV)
        before = parent.clone()
        c_in = parent[1:m + 1, 8:8 + n]
    elif c0 is not None:
        c_in = c0.clone().to(DEV)
    outs = ext().gemm_bf16_ex(embed(a, extra), embed(b, extra), LAY[layout], epi,
                              dev(bias), dev(aux), c_in)
    out = c_in if c0 is not None else outs[0]
    assert out.shape == (m, n) and out.dtype == BF
    tag = f"bf16 {layout} {variant} {m}x{n}x{k}" + (" strided" if extra else "") \
        + (" ldc>N" if c_strided else "")
    check_bound(out.cpu(), *gemm_ref(a, b, layout, epi, bias, aux, c0), tag=tag)
    if variant == "bias_gelu":
        check_bound(outs[1].cpu(), *gemm_ref(a, b, layout, BIAS, bias), tag=tag + " aux")
    if parent is not None:
        inside = torch.zeros_like(parent, dtype=torch.bool)
        inside[1:m + 1, 8:8 + n] = True
        assert torch.equal(parent.view(torch.int16)[~inside], before.view(torch.int16)[~inside]), \
            f"{tag}: store outside c_in"
    return [out.clone()] + [o.clone() for o in outs[1:]]


def run_batched(e, m, n, k, seed=0):
    a, b, _ = operands("nt", m, n, k, 200 + seed, batch=e)
    out = ext().gemm_bf16_nt_batched(embed(a), embed(b))
    assert out.shape == (e, m, n)
    check_bound(out.cpu(), *gemm_ref(a, b), tag=f"bf16 batched {e}x{m}x{n}x{k}")


def f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def run_fp8(m, n, k, has_bias, scale, batch=None, extra=0, seed=0):
    a, b, g = operands("nt", m, n, k, 300 + seed, batch, make=fp8_operand)
    bias = None
    if has_bias:
        bias = torch.randn(*((n,) if batch is None else (batch, n)), generator=g).to(BF)
        assert batch is None or not torch.equal(bias[0], bias[1])
    fn = ext().gemm_fp8_nt if batch is None else ext().gemm_fp8_nt_batched
    out = fn(embed(a, extra), embed(b, extra), scale, dev(bias))
    assert out.shape == ((m, n) if batch is None else (batch, m, n)) and out.dtype == BF
    ref = gemm_ref(a.float(), b.float(), "nt", BIAS if has_bias else NONE, bias,
                   scale_ab=f32(scale))
    check_bound(out.cpu(), *ref, tag=f"fp8 {batch or ''} {m}x{n}x{k} bias={has_bias} "
                                     f"scale={scale:g}" + (" strided" if extra else ""))


# ---------------------------------------------------------------------------
# the fast (4-phase counted-vmcnt) NT kernel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", [64, 128, 192, 256, 320])
def test_fast_pipeline_depth(k):
    """nkt 1: no prefetch; 2: pf1 only, the vmcnt(0) branch; >= 3: pf2, the
    vmcnt(2) branch with A rounds split over phases 1 and 3."""
    p = gemm_path("nt", 256, 256, k)
    assert p["has_fast"] and not p["has_edge"] and p["nkt"] == k // 64
    run_bf16("nt", 256, 256, k)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("m,n,k", [(256, 512, 64), (512, 256, 128), (256, 256, 192)])
def test_fast_every_variant(m, n, k, variant):
    p = gemm_path("nt", m, n, k)
    assert p["has_fast"] and not p["has_edge"] and p["nkt"] == k // 64 <= 3
    run_bf16("nt", m, n, k, variant, seed=1)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("m,n,k", [(257, 256, 128), (256, 264, 192), (300, 520, 192)])
def test_fast_and_edge_pair(m, n, k, variant):
    """Interior tiles by the fast launch, the rest by the guarded launch whose
    interior blocks return early (skip_interior)."""
    p = gemm_path("nt", m, n, k)
    assert p["has_fast"] and p["has_edge"] and p["edge_grid"] != p["fast_grid"]
    run_bf16("nt", m, n, k, variant, seed=2)


# ---------------------------------------------------------------------------
# the guarded kernel's partial 16-byte chunks
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("layout", sorted(LAY))
@pytest.mark.parametrize("m,n", [(130, 200), (256, 256)])
@pytest.mark.parametrize("k", [68, 100, 129])
def test_partial_chunk_along_k(k, m, n, layout):
    """K is no multiple of 8: the last chunk of a row of A[M][K] / Bt[N][K]
    straddles K (scalar branch of stage_rows); the parent's row stride is K
    rounded up to 8 and the columns past K are NaN."""
    p = gemm_path(layout, m, n, k)
    assert not p["has_fast"] and p["edge_grid"] == (1, 1) and k % 8 != 0
    run_bf16(layout, m, n, k, seed=3)


@pytest.mark.parametrize("layout", ["nn", "tn"])
@pytest.mark.parametrize("k", [128, 100])
def test_partial_chunk_along_m_and_n(k, layout):
    """K-major operands At[K][M], B[K][N]: a chunk straddles M = 300 (stride
    304) or N = 260 (stride 264), the scalar branch of stage_transposed."""
    m, n = 300, 260
    p = gemm_path(layout, m, n, k)
    assert not p["has_fast"] and p["edge_grid"] == (2, 2) and m % 8 and n % 8
    for variant in ("none", "bias", "accumulate"):
        run_bf16(layout, m, n, k, variant, seed=4)


@pytest.mark.parametrize("layout", sorted(LAY))
@pytest.mark.parametrize("m,n,k", [(1, 8, 64), (8, 1, 64), (1, 1, 72)])
def test_one_row_one_column(m, n, k, layout):
    """A K-major operand of width 1 is a column of an 8-wide parent."""
    assert gemm_path(layout, m, n, k)["edge_grid"] == (1, 1)
    run_bf16(layout, m, n, k, "bias", seed=5)


# ---------------------------------------------------------------------------
# strides larger than the logical operand
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("layout", sorted(LAY))
@pytest.mark.parametrize("m,n,k", [(256, 256, 128), (300, 264, 100)])
def test_row_stride_larger_than_width(m, n, k, layout):
    """a and b are the right-hand column slices of parents 64 columns wider;
    everything else in the parents is NaN."""
    p = gemm_path(layout, m, n, k)
    assert p["has_fast"] == (layout == "nt" and k == 128)
    run_bf16(layout, m, n, k, extra=64, seed=6)
    run_bf16(layout, m, n, k, "bias_gelu", extra=64, seed=6)


@pytest.mark.parametrize("layout", ["nt", "tn"])
@pytest.mark.parametrize("m,n,k", [(300, 264, 128), (256, 256, 192)])
def test_strided_c_in(m, n, k, layout):
    """Accumulate into a column slice (ldc = N + 24) of a parent whose other
    elements must come back bit for bit."""
    p = gemm_path(layout, m, n, k)
    assert p["has_fast"] == (layout == "nt")
    run_bf16(layout, m, n, k, "accumulate", c_strided=True, seed=7)
    run_bf16(layout, m, n, k, "accumulate", extra=64, c_strided=True, seed=7)


# ---------------------------------------------------------------------------
# rasterisation: last band shorter than 8 tile rows, nwg % 8 != 0
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [256, 512])
def test_raster_short_band_fast_grid(n):
    p = gemm_path("nt", 2304, n, 64)
    assert p["fast_grid"] == (9, n // 256) and p["fast_short_band"] and not p["has_edge"]
    assert p["fast_nwg_mod8"] == n // 256
    run_bf16("nt", 2304, n, 64, seed=8)


@pytest.mark.parametrize("layout", ["nt", "nn"])
def test_raster_short_band_edge_grid(layout):
    p = gemm_path(layout, 2348, 520, 64)
    assert p["edge_grid"] == (10, 3) and p["edge_short_band"] and p["edge_nwg_mod8"] == 6
    assert p["has_fast"] == (layout == "nt")
    if layout == "nt":
        assert p["fast_grid"] == (9, 2) and p["fast_short_band"] and p["fast_nwg_mod8"] == 2
    run_bf16(layout, 2348, 520, 64, "bias", seed=9)


# ---------------------------------------------------------------------------
# batches: blockIdx.z > 0, batch stride > m * k with NaN rows in between
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("e,m,n,k", [(3, 257, 264, 192), (2, 130, 200, 100), (3, 2304, 256, 64)])
def test_batched_strided(e, m, n, k):
    p = gemm_path("nt", m, n, k)
    assert (p["has_fast"], p["has_edge"]) == {257: (True, True), 130: (False, True),
                                              2304: (True, False)}[m]
    run_batched(e, m, n, k)


# ---------------------------------------------------------------------------
# fp8
# ---------------------------------------------------------------------------
FP8_SHAPES = [(256, 256, 128), (256, 256, 256), (256, 256, 384), (257, 264, 256),
              (300, 200, 136), (256, 256, 200)]


@pytest.mark.parametrize("has_bias,scale", [(False, 0.731), (True, 2.0 ** -8),
                                            (True, 0.731), (False, 2.0 ** -8)])
@pytest.mark.parametrize("m,n,k", FP8_SHAPES)
def test_fp8(m, n, k, has_bias, scale):
    """Fast depth 1..3 (BK 128), the edge pair, a K tail of whole chunks
    (136, stride 144) and one with a partial chunk (200, stride 208)."""
    p = gemm_path("nt", m, n, k, bk=128)
    assert p["has_fast"] == (k % 128 == 0) and p["has_edge"] == (k % 128 != 0 or m > 256)
    assert p["nkt"] == -(-k // 128)
    run_fp8(m, n, k, has_bias, scale)


@pytest.mark.parametrize("extra", [0, 64])
def test_fp8_batched_bias_per_batch(extra):
    p = gemm_path("nt", 257, 264, 384, bk=128)
    assert p["has_fast"] and p["has_edge"] and p["nkt"] == 3
    run_fp8(257, 264, 384, True, 0.731, batch=3, extra=extra, seed=1)
    run_fp8(257, 264, 384, False, 2.0 ** -8, batch=3, extra=extra, seed=2)


# ---------------------------------------------------------------------------
# exact index tracing: one-hot operand, integers in the other; torch.equal
# ---------------------------------------------------------------------------
def int_rows(rows, k, lim):
    """Integers in [-lim, lim] from (row, k); no two rows agree."""
    r, kk = torch.arange(rows)[:, None], torch.arange(k)[None, :]
    p = 2 * lim + 1
    v = (37 * r + 101 * kk + 3 * (r // p) * (kk % 7 + 1) + (r // (p * p)) * (kk % 5 + 1)) % p - lim
    assert torch.unique(v, dim=0).shape[0] == rows
    return v.float()


def one_hot_rows(rows, k, batch):
    """[batch, rows, k]: row r of batch z is 1 at k = (7 r + 3 z) % K."""
    z, r = torch.arange(batch)[:, None], torch.arange(rows)[None, :]
    return torch.nn.functional.one_hot((7 * r + 3 * z) % k, k).float()


def tracing_operands(m, n, k, batch, hot_in_a, lim, dtype):
    e = batch or 1
    hot = one_hot_rows(m if hot_in_a else n, k, e)
    ints = int_rows(e * (n if hot_in_a else m), k, lim).reshape(e, -1, k)
    a, b = (hot, ints) if hot_in_a else (ints, hot)
    want = torch.einsum("zmk,znk->zmn", a.double(), b.double())
    # what the test is about: C[m][n] is one element of the integer operand
    z, r = torch.arange(e)[:, None], torch.arange(m if hot_in_a else n)[None, :]
    sel = ints[z, :, (7 * r + 3 * z) % k]              # [e, hot rows, int rows]
    assert torch.equal(want, (sel if hot_in_a else sel.transpose(1, 2)).double())
    if batch is None:
        a, b, want = a[0], b[0], want[0]
    return a.to(dtype), b.to(dtype), want


def store(a, b, layout):
    if layout == "tn":
        a = a.transpose(-1, -2).contiguous()
    if layout != "nt":
        b = b.transpose(-1, -2).contiguous()
    return a, b


@pytest.mark.parametrize("hot_in_a", [True, False])
@pytest.mark.parametrize("layout", sorted(LAY))
@pytest.mark.parametrize("m,n,k", [(300, 520, 192), (2348, 520, 64)])
def test_index_tracing_bf16(m, n, k, layout, hot_in_a):
    """Pins the LDS swizzle, the fragment-to-element map, the raster bijection
    and the epilogue's bias / c_in indexing: every output is one integer."""
    a, b, want = tracing_operands(m, n, k, None, hot_in_a, 128, BF)
    a, b = store(a, b, layout)
    bias = (torch.arange(n) * 5 % 17 - 8).to(BF)
    c0 = ((torch.arange(m)[:, None] * 3 + torch.arange(n)[None, :] * 7) % 17 - 8).to(BF)
    out = ext().gemm_bf16_ex(embed(a), embed(b), LAY[layout], 0, None, None, None)[0]
    assert torch.equal(out.cpu().double(), want)
    out = ext().gemm_bf16_ex(embed(a), embed(b), LAY[layout], 1, bias.to(DEV), None, None)[0]
    assert torch.equal(out.cpu().double(), want + bias.double())
    acc = c0.clone().to(DEV)
    ext().gemm_bf16_ex(embed(a), embed(b), LAY[layout], 0, None, None, acc)
    assert torch.equal(acc.cpu().double(), want + c0.double())


@pytest.mark.parametrize("hot_in_a", [True, False])
def test_index_tracing_bf16_batched(hot_in_a):
    a, b, want = tracing_operands(257, 264, 128, 3, hot_in_a, 128, BF)
    out = ext().gemm_bf16_nt_batched(embed(a), embed(b))
    assert torch.equal(out.cpu().double(), want)


@pytest.mark.parametrize("hot_in_a", [True, False])
@pytest.mark.parametrize("m,n,k,batch", [(300, 520, 192, None), (2348, 520, 128, None),
                                         (257, 264, 128, 3)])
def test_index_tracing_fp8(m, n, k, batch, hot_in_a):
    """fp8 has K >= 128, so the raster shape runs at K = 128.  Integers in
    [-8, 8] are exact in e4m3 and scale_ab = 1/4 keeps the output exact."""
    a, b, want = tracing_operands(m, n, k, batch, hot_in_a, 8, F8)
    fn = ext().gemm_fp8_nt if batch is None else ext().gemm_fp8_nt_batched
    bias = (torch.arange((batch or 1) * n) * 5 % 17 - 8).reshape(-1, n).to(BF)
    if batch is None:
        bias = bias[0]
    out = fn(embed(a), embed(b), 0.25, None)
    assert torch.equal(out.cpu().double(), want * 0.25)
    out = fn(embed(a), embed(b), 0.25, bias.to(DEV))
    shift = bias.double().unsqueeze(-2) if batch else bias.double()
    assert torch.equal(out.cpu().double(), want * 0.25 + shift)


# ---------------------------------------------------------------------------
# determinism
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("layout", sorted(LAY))
def test_deterministic(layout, variant):
    first = run_bf16(layout, 300, 520, 192, variant, seed=10)
    again = run_bf16(layout, 300, 520, 192, variant, seed=10)
    assert len(first) == len(again) == (2 if variant == "bias_gelu" else 1)
    for x, y in zip(first, again):
        assert torch.equal(x.view(torch.int16), y.view(torch.int16))


def test_deterministic_fp8():
    a, b, g = operands("nt", 300, 520, 256, 11, make=fp8_operand)
    bias = torch.randn(520, generator=g).to(BF).to(DEV)
    da, db = embed(a), embed(b)
    first = ext().gemm_fp8_nt(da, db, 0.731, bias)
    again = ext().gemm_fp8_nt(da, db, 0.731, bias)
    assert torch.equal(first.view(torch.int16), again.view(torch.int16))
