"""The dense-GEMM comparator must be able to fail.  out = bf16(ref) is built on
the CPU at (256, 256, 192) with the input recipe of test_gemm_bounds_gpu.py and
then damaged the way a kernel can be wrong; check_bound (gemm_ref.py) has to
reject every damage, and the max-norm comparator of test_gemm_gpu.py, which it
supersedes for these kernels, is shown to accept the first five.

The last 16 rows of A and of Bt are set to the recipe's smallest magnitude
(2^-3), so the output has a quiet corner fragment [240:256, 240:256]: that is
where a max-norm comparator is blind, and where the fragment-sized damages are
placed.  Also here: gemm_path against hand-written expectations, the tile
rasteriser's bijection, the measured GELU constants, and the e4m3 encoder
against torch's cast."""
import pytest
import torch

from gemm_ref import (BIAS, BIAS_GELU, DGELU, DGELU_POLY_ERR, GELU_POLY_ERR,  # noqa: E402
                      all_bf16, check_bound, e4m3_encode, gelu64, gelu_poly_errors,
                      gemm_path, gemm_ref, scaled_rows, tile_order)
from test_gemm_gpu import _gemm_rel_ok  # noqa: E402

M, N, K = 256, 256, 192
R0, C0 = 240, 240                  # the quiet corner fragment
BF = torch.bfloat16
SCALE = 0.731


def _passes(fn):
    try:
        fn()
    except AssertionError:
        return False
    return True


def _inputs():
    g = torch.Generator().manual_seed(2024)
    a, bt = scaled_rows(M, K, g), scaled_rows(N, K, g)
    a[R0:] = (torch.randn(16, K, generator=g) * 2.0 ** -3).to(BF)
    bt[C0:] = (torch.randn(16, K, generator=g) * 2.0 ** -3).to(BF)
    bias = torch.randn(N, generator=g).to(BF)
    c0 = scaled_rows(M, N, g)
    return a, bt, bias, c0


A, BT, BIAS_V, C_0 = _inputs()
AD, BD = A.double(), BT.double()
AB = AD @ BD.t()
FRAG = (slice(R0, R0 + 16), slice(C0, C0 + 16))


def _partial(rows, cols, ks):
    return AD[rows, ks] @ BD[cols, ks].t()


def _plain(mutate):
    out = AB.clone()
    mutate(out)
    return out.to(BF), gemm_ref(A, BT)


def m_slab_dropped(out):
    out[FRAG] -= _partial(FRAG[0], FRAG[1], slice(32, 64))


def m_ktile_twice(out):
    out[FRAG] += _partial(FRAG[0], FRAG[1], slice(64, 128))


def m_fragments_swapped(out):
    upper = (slice(R0 - 16, R0), FRAG[1])
    out[FRAG], out[upper] = out[upper].clone(), out[FRAG].clone()


def case_bias_shifted():
    out = (AB + torch.roll(BIAS_V.double(), 16)).to(BF)
    return out, gemm_ref(A, BT, "nt", BIAS, bias=BIAS_V)


def case_missing_scale(region=FRAG):
    out = AB * SCALE
    out[region] = AB[region]
    return out.to(BF), gemm_ref(A, BT, scale_ab=SCALE)


FIRST_FIVE = {
    "slab_dropped": lambda: _plain(m_slab_dropped),
    "ktile_twice": lambda: _plain(m_ktile_twice),
    "fragments_swapped": lambda: _plain(m_fragments_swapped),
    "bias_shifted_16": case_bias_shifted,
    "missing_scale_ab": case_missing_scale,
}


def test_unmutated_has_headroom():
    """The inputs leave half the bound free when the only error is the final
    rounding, for every variant."""
    z = torch.randn(M, N, generator=torch.Generator().manual_seed(5)).to(BF)
    cases = {
        "none": ({}, AB),
        "bias": (dict(epilogue=BIAS, bias=BIAS_V), AB + BIAS_V.double()),
        "bias_gelu": (dict(epilogue=BIAS_GELU, bias=BIAS_V), gelu64(AB + BIAS_V.double())),
        "dgelu": (dict(epilogue=DGELU, aux=z), None),
        "accumulate": (dict(c0=C_0), AB + C_0.double()),
        "fp8_scale": (dict(scale_ab=SCALE), AB * SCALE),
    }
    for name, (kw, exact) in cases.items():
        args = gemm_ref(A, BT, "nt", **kw)
        if exact is not None:
            assert torch.equal(args[0], exact), name
        assert check_bound(args[0].to(BF), *args, tag=name) <= 0.5, name


def test_reference_layouts_and_batch_agree():
    ref = gemm_ref(A, BT)[0]
    assert torch.equal(gemm_ref(A, BT.t().contiguous(), "nn")[0], ref)
    assert torch.equal(gemm_ref(A.t().contiguous(), BT.t().contiguous(), "tn")[0], ref)
    a3, b3 = torch.stack((A, A.flip(0))), torch.stack((BT, BT.flip(0)))
    bias2 = torch.stack((BIAS_V, BIAS_V.flip(0)))
    r3, s3, k3, _, rd = gemm_ref(a3, b3, bias=bias2, scale_ab=SCALE)
    assert (k3, rd) == (K + 1, 2)
    assert torch.equal(r3[1], gemm_ref(a3[1], b3[1], bias=bias2[1], scale_ab=SCALE)[0])
    assert torch.equal(s3[0], (AD.abs() @ BD.abs().t()) * SCALE)


@pytest.mark.parametrize("name", sorted(FIRST_FIVE))
def test_check_bound_rejects(name):
    out, args = FIRST_FIVE[name]()
    assert not _passes(lambda: check_bound(out, *args, tag=name))


@pytest.mark.parametrize("name", sorted(FIRST_FIVE))
def test_old_comparator_accepts(name):
    """Why _gemm_rel_ok is superseded: a damage in the quiet corner, or of the
    size of the bias, is far below 3e-2 of the largest output."""
    out, args = FIRST_FIVE[name]()
    _gemm_rel_ok(out, args[0].float())


def test_check_bound_rejects_whole_tile_damage():
    whole = (slice(0, M), slice(0, N))
    out, args = case_missing_scale(whole)
    assert not _passes(lambda: check_bound(out, *args, tag="scale, whole tile"))
    out = (AB + _partial(whole[0], whole[1], slice(64, 128))).to(BF)
    assert not _passes(lambda: check_bound(out, *gemm_ref(A, BT), tag="k-tile, whole tile"))


def test_check_bound_rejects_accumulate_damage():
    args = gemm_ref(A, BT, c0=C_0)
    good = AB + C_0.double()
    skipped = good.clone()
    skipped[FRAG] = C_0.double()[FRAG]
    assert not _passes(lambda: check_bound(skipped.to(BF), *args, tag="left at c0"))
    twice = (good + C_0.double()).to(BF)
    assert not _passes(lambda: check_bound(twice, *args, tag="accumulated twice"))


def test_check_bound_accepts_gelu_of_rounded_aux():
    """gelu(bf16(pre)) in place of gelu(pre) is a second rounding of the
    pre-activation.  For pre >= 0, where |gelu'| <= 1.13 and gelu(pre) >=
    pre / 2, it is inside the two roundings the bias rule grants: the
    comparator cannot tell the two apart, and every such element passes.  On
    the negative tail |gelu(pre)| << |pre|, so 2^-8 |pre| |gelu'| can exceed
    2 * 2^-7 |gelu(pre)|: there the rule is tight enough to see the second
    rounding in a handful of elements (14 of 65536 here, worst err/bound 1.16).
    The kernel applies GELU to the unrounded fp32 value; aux is checked on
    its own by the bias rule."""
    pre = AB + BIAS_V.double()
    out = gelu64(pre.to(BF)).to(BF)
    exact = gelu64(pre).to(BF)
    args = gemm_ref(A, BT, "nt", BIAS_GELU, bias=BIAS_V)
    assert int((pre >= 0).sum()) > M * N // 3
    check_bound(torch.where(pre >= 0, out, exact), *args, tag="gelu(rounded aux), pre >= 0")
    assert not torch.equal(torch.where(pre >= 0, out, exact), exact)
    ref, s, k, extra, rd = args
    over = (out.double() - ref).abs() > rd * 2.0 ** -7 * ref.abs() + k * 2.0 ** -24 * s + extra
    assert bool((pre[over] < 0).all()) and int(over.sum()) < M * N // 1000
    # ... while GELU left out, or applied twice, is caught
    assert not _passes(lambda: check_bound(pre.to(BF), *args, tag="no gelu"))


def test_check_bound_rejects_row_of_neighbouring_batch():
    a3 = torch.stack((A, A.flip(0)))
    b3 = torch.stack((BT, BT.flip(0)))
    args = gemm_ref(a3, b3)
    out = args[0].clone()
    out[0, 255] = args[0][1, 255]
    assert not _passes(lambda: check_bound(out.to(BF), *args, tag="row of batch 1"))
    with pytest.raises(AssertionError, match=r"batch 0 \(row 255, col \d+\): tile \(0, 0\), "
                                             r"wave \(wr 1, wc \d\), fragment \(m 7, n \d\)"):
        check_bound(out.to(BF), *args, tag="row of batch 1")


def test_check_bound_ulps_at_the_largest_output():
    """At |ref| near its maximum the rule is 2^-7 |ref|, between 1 and 2 bf16
    ulps: half an ulp (correct rounding) and a whole ulp pass, 2 ulps fail."""
    ref, s, k, extra, rd = gemm_ref(A, BT)
    order = ref.abs().reshape(-1).argsort(descending=True)
    mant, _ = torch.frexp(ref.reshape(-1)[order])
    i = int(order[(mant.abs() < 0.99).nonzero()[0, 0]])   # not at the top of its binade
    x = ref.reshape(-1)[i]
    assert x.abs() > 0.5 * ref.abs().max()
    ulp = torch.exp2(torch.frexp(x)[1].double() - 8)      # bf16: 8 significand bits
    for n_ulp, ok in ((0.5, True), (1.0, True), (2.0, False)):
        out = ref.clone()
        out.reshape(-1)[i] = x + n_ulp * ulp
        assert _passes(lambda: check_bound(out, ref, s, k, extra, rd, f"{n_ulp} ulp")) == ok
    r, c = divmod(i, N)
    with pytest.raises(AssertionError, match=rf"\(row {r}, col {c}\)"):
        check_bound(out, ref, s, k, extra, rd, "2 ulp")


def test_check_bound_rejects_nan_and_shape():
    ref, s, k, extra, rd = gemm_ref(A, BT)
    out = ref.to(BF)
    out[3, 5] = float("nan")
    assert not _passes(lambda: check_bound(out, ref, s, k, extra, rd, "nan"))
    assert not _passes(lambda: check_bound(ref[:, :-1].to(BF), ref, s, k, extra, rd, "shape"))


def test_gelu_constants_are_the_measured_ones():
    e_g, e_d = gelu_poly_errors()
    assert e_g <= GELU_POLY_ERR <= 1.1 * e_g, e_g
    assert e_d <= DGELU_POLY_ERR <= 1.1 * e_d, e_d


# ---------------------------------------------------------------------------
# gemm_path: the shape table of test_gemm_bounds_gpu.py, by hand
# ---------------------------------------------------------------------------
def P(has_fast, has_edge, nkt, fast_grid=None, edge_grid=None, fast_short=False,
      edge_short=False):
    return {
        "has_fast": has_fast, "has_edge": has_edge, "nkt": nkt,
        "fast_grid": fast_grid, "edge_grid": edge_grid,
        "fast_nwg_mod8": fast_grid[0] * fast_grid[1] % 8 if fast_grid else None,
        "edge_nwg_mod8": edge_grid[0] * edge_grid[1] % 8 if edge_grid else None,
        "fast_short_band": fast_short, "edge_short_band": edge_short,
    }


PATHS = [
    (("nt", 256, 256, 64), P(True, False, 1, (1, 1))),
    (("nt", 256, 256, 128), P(True, False, 2, (1, 1))),
    (("nt", 256, 256, 192), P(True, False, 3, (1, 1))),
    (("nt", 256, 256, 320), P(True, False, 5, (1, 1))),
    (("nt", 256, 512, 64), P(True, False, 1, (1, 2))),
    (("nt", 512, 256, 128), P(True, False, 2, (2, 1))),
    (("nt", 257, 256, 128), P(True, True, 2, (1, 1), (2, 1))),
    (("nt", 256, 264, 192), P(True, True, 3, (1, 1), (1, 2))),
    (("nt", 300, 520, 192), P(True, True, 3, (1, 2), (2, 3))),
    (("nt", 256, 256, 100), P(False, True, 2, None, (1, 1))),
    (("nt", 130, 200, 129), P(False, True, 3, None, (1, 1))),
    (("nn", 256, 256, 128), P(False, True, 2, None, (1, 1))),
    (("tn", 300, 260, 128), P(False, True, 2, None, (2, 2))),
    (("nt", 1, 8, 64), P(False, True, 1, None, (1, 1))),
    (("nt", 1, 1, 72), P(False, True, 2, None, (1, 1))),
    (("nt", 2304, 256, 64), P(True, False, 1, (9, 1), None, True)),
    (("nt", 2304, 512, 64), P(True, False, 1, (9, 2), None, True)),
    (("nt", 2348, 520, 64), P(True, True, 1, (9, 2), (10, 3), True, True)),
    (("nn", 2348, 520, 64), P(False, True, 1, None, (10, 3), False, True)),
    (("nt", 256, 256, 384, 128), P(True, False, 3, (1, 1))),
    (("nt", 257, 264, 256, 128), P(True, True, 2, (1, 1), (2, 2))),
    (("nt", 256, 256, 200, 128), P(False, True, 2, None, (1, 1))),
    (("nt", 256, 256, 192, 128), P(False, True, 2, None, (1, 1))),
]


@pytest.mark.parametrize("args,want", PATHS, ids=["-".join(map(str, p[0])) for p in PATHS])
def test_gemm_path(args, want):
    assert gemm_path(*args) == want
    if len(args) == 4:
        assert gemm_path(*args, bk=64) == want


def test_gemm_path_remainders():
    assert gemm_path("nt", 2304, 256, 64)["fast_nwg_mod8"] == 1
    assert gemm_path("nt", 2304, 512, 64)["fast_nwg_mod8"] == 2
    assert gemm_path("nt", 2348, 520, 64)["edge_nwg_mod8"] == 6


@pytest.mark.parametrize("mt,nt", [(1, 1), (2, 3), (8, 2), (9, 1), (9, 2), (10, 3), (17, 5)])
def test_tile_order_is_a_bijection(mt, nt):
    tiles = tile_order(mt, nt)
    assert sorted(tiles) == [(i, j) for i in range(mt) for j in range(nt)]


# ---------------------------------------------------------------------------
# e4m3 encoder against torch's cast
# ---------------------------------------------------------------------------
QUANT_SCALES = (1.0, 0.731, 2.0 ** -3, 37.0, 448.0 / 3.0)


@pytest.mark.parametrize("scale", QUANT_SCALES)
def test_e4m3_encoder_matches_torch(scale):
    v = all_bf16().float() * torch.tensor(scale, dtype=torch.float32)
    v = v[torch.isfinite(v) & (v.abs() <= 448.0)]
    assert v.numel() > 30000
    assert torch.equal(e4m3_encode(v), v.to(torch.float8_e4m3fn).view(torch.uint8))


def test_e4m3_encoder_by_hand():
    v = torch.tensor([0.0, -0.0, 2.0 ** -9, 2.0 ** -10, 3 * 2.0 ** -10, -2.0 ** -6,
                      1.0, 1.0625, 1.1875, 448.0, -448.0, 464.0 - 2.0 ** -10, 17.0])
    want = [0x00, 0x80, 0x01, 0x00, 0x02, 0x88, 0x38, 0x38, 0x3A, 0x7E, 0xFE, 0x7E, 0x58]
    assert e4m3_encode(v).tolist() == want
