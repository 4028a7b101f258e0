"""The MFMA decode W-streamer (decode_stream_kernel) with bf16 and int8
weights: LDS-tile-count and M-tile edges, a tile-position probe, a strided
weight, the bindings' contract and the dispatch sites' fall-back.  The int4
format has its own file (test_weight_only_int4_gpu.py).

Tolerances are the neighbouring tests' (test_kernels_gpu.py): max relative
error 2e-2 for bf16, atol 0.5 / rtol 0.05 against the dequantized fp32
product for int8.  The case tables are shared with
test_kernel_dispatch_cpu.py, which runs the pure predicates over them.
"""
import functools

import pytest
import torch

from test_kernels_gpu import _gemm_rel_ok

DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32

# K = 1, 2, 3, 5 LDS tiles: nothing to prefetch, and tile counts that leave
# the DEPTH-unrolled loop (DEPTH 1 bf16, 2 int8) after each of its steps.
# M = the two MTILES instantiations and their boundaries.
EDGE_K = [64, 128, 192, 320]
EDGE_M = [1, 16, 17, 32]
# one-hot positions, K = 320: every tile, both 32-halves of a tile, k % 8 in
# {0, 1, 2, 4, 5, 6, 7}
PROBE_K = sorted([t * 64 + o for t in range(5) for o in (0, 9, 18, 31, 36, 63)]
                 + [2 * 64 + 45, 4 * 64 + 54])


def _C():
    from paddle_amd import _ext
    return _ext.get_ext(required=True)


def _int8_ok(out, ref):
    torch.testing.assert_close(out.float(), ref, atol=0.5, rtol=0.05)


@functools.lru_cache(maxsize=None)
def _edge_case(fmt, m, k):
    """(x, weight operands, bias, ref without bias) for N = 256."""
    n = 256
    g = torch.Generator().manual_seed(1000 + m + k)
    x = torch.randn(m, k, generator=g).to(BF16).to(DEV)
    bias = torch.randn(n, generator=g).to(BF16).to(DEV)
    if fmt == "bf16":
        w = (torch.randn(k, n, generator=g) * 0.02).to(BF16).to(DEV)
        return x, (w,), bias, x.float() @ w.float()
    from paddle_amd import quantization as Q
    qw, sc = Q.weight_quantize(torch.randn(k, n, generator=g) * 0.1)
    qw, sc = qw.to(DEV), sc.to(DEV)
    return x, (qw, sc), bias, x.float() @ (qw.float() * sc.unsqueeze(0) / 127.0)


@pytest.mark.gpu
@pytest.mark.parametrize("k", EDGE_K)
@pytest.mark.parametrize("m", EDGE_M)
@pytest.mark.parametrize("fmt", ["bf16", "int8"])
def test_decode_stream_tile_edges_gpu(fmt, m, k):
    x, wargs, bias, ref = _edge_case(fmt, m, k)
    if fmt == "bf16":
        call, ok = _C().decode_gemm_mfma, functools.partial(_gemm_rel_ok, tol=2e-2)
    else:
        call, ok = _C().decode_gemm_int8, _int8_ok
    out = call(x, *wargs, bias)
    assert out.dtype == BF16 and tuple(out.shape) == (m, 256)
    ok(out, ref + bias.float())
    ok(call(x, *wargs, None), ref)


def _one_hot():
    x = torch.zeros(32, 320, dtype=BF16, device=DEV)
    x[torch.arange(32), torch.tensor(PROBE_K)] = 1.0
    return x


@pytest.mark.gpu
def test_decode_gemm_mfma_one_hot_probe_gpu():
    """Row m of x is one-hot at PROBE_K[m]: output row m must equal
    W[PROBE_K[m], :] exactly (one exact product, zeros added in fp32, an
    exact cast back).  W[k, n] is the p-th finite normal bf16 bit pattern,
    p = k * 256 + n: distinct for every (k, n) with k < 254, which is all
    bf16 has to offer (65024 patterns); rows k and k - 254 repeat, 254 being
    no multiple of a tile, a half tile or a chunk."""
    assert len(PROBE_K) == 32 and len(set(PROBE_K)) == 32
    assert {k // 64 for k in PROBE_K} == set(range(5))
    assert {(k % 64) // 32 for k in PROBE_K} == {0, 1}
    assert len({k % 8 for k in PROBE_K}) >= 6
    p = torch.arange(320 * 256, dtype=torch.int64).reshape(320, 256)
    bits = 0x0080 + p % 32512 + 0x8000 * ((p // 32512) & 1)
    w = torch.where(bits >= 0x8000, bits - 0x10000, bits).to(torch.int16)
    w = w.view(BF16).to(DEV)
    assert bool(torch.isfinite(w.float()).all())
    assert len(torch.unique(w[:254].view(torch.int16))) == 254 * 256
    out = _C().decode_gemm_mfma(_one_hot(), w, None)
    expect = w[torch.tensor(PROBE_K, device=DEV)]
    assert torch.equal(out.view(torch.int16), expect.view(torch.int16))


@pytest.mark.gpu
def test_decode_gemm_int8_one_hot_probe_gpu():
    """As above for int8: output row m must match the dequantized row
    PROBE_K[m] within the int8 tolerance.  Codes are a pseudo-random function
    of (k, n) and the scale makes one code step 4..8, so a row, column or
    nibble taken from elsewhere is far outside the tolerance."""
    kk = torch.arange(320, dtype=torch.int64).reshape(320, 1)
    nn = torch.arange(256, dtype=torch.int64).reshape(1, 256)
    qw = ((kk * 131 + nn * 37 + (kk * nn) % 53) % 255 - 127).to(torch.int8).to(DEV)
    sc = (127.0 * (4 + torch.arange(256) % 5)).to(F32).to(DEV)
    out = _C().decode_gemm_int8(_one_hot(), qw, sc, None)
    rows = torch.tensor(PROBE_K, device=DEV)
    what = qw.float() * sc.unsqueeze(0) / 127.0
    _int8_ok(out, what[rows])
    # the tolerance does tell rows apart: the neighbouring row is outside it
    with pytest.raises(AssertionError):
        _int8_ok(out, what[(rows + 1) % 320])


@pytest.mark.gpu
def test_decode_gemm_mfma_strided_weight_gpu():
    """ldw != N: a column slice of a wider matrix (row stride 512, base
    offset 256 elements = 512 bytes), as linear() dispatches it."""
    g = torch.Generator().manual_seed(7)
    big = (torch.randn(128, 512, generator=g) * 0.02).to(BF16).to(DEV)
    x = torch.randn(17, 128, generator=g).to(BF16).to(DEV)
    w = big[:, 256:512]
    assert w.stride(0) == 512 and w.storage_offset() == 256
    y = _C().decode_gemm_mfma(x, w, None)
    _gemm_rel_ok(y, x.float() @ w.float(), tol=2e-2)


# ---------------------------------------------------------------------------
# contract: one valid call and the ways to leave it.  Each entry maps the
# valid operands to off-contract ones and says whether the pure predicate
# still accepts them (True where the dispatch site repairs the operand
# before the call: it makes x contiguous and casts a floating-point bias).
# ---------------------------------------------------------------------------
def mfma_valid(dev, m=4, k=128, n=256):
    return {"x": torch.zeros(m, k, dtype=BF16, device=dev),
            "w": torch.zeros(k, n, dtype=BF16, device=dev),
            "bias": torch.zeros(n, dtype=BF16, device=dev)}


def int8_valid(dev, m=4, k=128, n=256):
    return {"x": torch.zeros(m, k, dtype=BF16, device=dev),
            "qw": torch.zeros(k, n, dtype=torch.int8, device=dev),
            "scale": torch.ones(n, dtype=F32, device=dev),
            "bias": torch.zeros(n, dtype=BF16, device=dev)}


def _common_bad(valid):
    """name -> (operands(dev), predicate still accepts)"""
    return {
        "M=33": (lambda dev: valid(dev, m=33), False),
        "N=128": (lambda dev: valid(dev, n=128), False),
        "K=96": (lambda dev: valid(dev, k=96), False),
        "x fp32": (lambda dev: {**valid(dev), "x": valid(dev)["x"].float()}, False),
        "x non-contiguous": (lambda dev: {
            **valid(dev), "x": torch.zeros(128, 4, dtype=BF16, device=dev).t()}, True),
        "bias fp32": (lambda dev: {
            **valid(dev), "bias": torch.zeros(256, dtype=F32, device=dev)}, True),
        "bias wrong length": (lambda dev: {
            **valid(dev), "bias": torch.zeros(128, dtype=BF16, device=dev)}, False),
    }


MFMA_BAD = {
    **_common_bad(mfma_valid),
    "w fp32": (lambda dev: {**mfma_valid(dev), "w": mfma_valid(dev)["w"].float()}, False),
    "w row stride 260": (lambda dev: {
        **mfma_valid(dev),
        "w": torch.zeros(128, 260, dtype=BF16, device=dev)[:, :256]}, False),
    "w base misaligned by 2 bytes": (lambda dev: {
        **mfma_valid(dev),
        "w": torch.zeros(128, 264, dtype=BF16, device=dev)[:, 1:257]}, False),
}

INT8_BAD = {
    **_common_bad(int8_valid),
    "qw non-contiguous": (lambda dev: {
        **int8_valid(dev),
        "qw": torch.zeros(256, 128, dtype=torch.int8, device=dev).t()}, False),
    "qw base misaligned by 1 byte": (lambda dev: {
        **int8_valid(dev),
        "qw": torch.zeros(128 * 256 + 16, dtype=torch.int8,
                          device=dev)[1:128 * 256 + 1].view(128, 256)}, False),
    "scale fp16": (lambda dev: {
        **int8_valid(dev), "scale": int8_valid(dev)["scale"].half()}, False),
    "scale wrong length": (lambda dev: {
        **int8_valid(dev), "scale": torch.ones(128, dtype=F32, device=dev)}, False),
}


@pytest.mark.gpu
@pytest.mark.parametrize("op", ["decode_gemm_mfma", "decode_gemm_int8"])
def test_decode_stream_contract_gpu(op):
    """Every off-contract direct _C call raises before any launch."""
    call = getattr(_C(), op)
    valid, bad = ((mfma_valid, MFMA_BAD) if op == "decode_gemm_mfma"
                  else (int8_valid, INT8_BAD))
    assert tuple(call(*valid(DEV).values()).shape) == (4, 256)
    for name, (make, _) in bad.items():
        with pytest.raises(RuntimeError):
            call(*make(DEV).values())
            pytest.fail(f"{op} {name}: accepted")
    assert tuple(call(*valid(DEV).values()).shape) == (4, 256)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# dispatch: operands outside the contract take the torch path, they do not
# raise and are not streamed
# ---------------------------------------------------------------------------
def _record(monkeypatch, name):
    C = _C()
    calls, real = [], getattr(C, name)
    monkeypatch.setattr(C, name, lambda *a: (calls.append(name), real(*a))[1])
    return calls


@pytest.mark.gpu
def test_linear_off_contract_weight_falls_back_gpu(monkeypatch):
    import paddle_amd.nn.functional as F
    calls = _record(monkeypatch, "decode_gemm_mfma")
    g = torch.Generator().manual_seed(3)
    x = torch.randn(4, 512, generator=g).to(BF16).to(DEV)
    big = (torch.randn(512, 260, generator=g) * 0.02).to(DEV)
    bias = torch.randn(256, generator=g).to(BF16).to(DEV)
    with torch.no_grad():
        # the tall-K shape is dispatched to the streamer ...
        w = big[:, :256].to(BF16).contiguous()
        _gemm_rel_ok(F.linear(x, w, bias), x.float() @ w.float() + bias.float(),
                     tol=2e-2)
        assert calls == ["decode_gemm_mfma"]
        # ... a row stride of 260 is not
        ws = big.to(BF16)[:, :256]
        assert ws.stride(0) == 260
        _gemm_rel_ok(F.linear(x, ws, bias), x.float() @ ws.float() + bias.float(),
                     tol=2e-2)
        # ... nor an fp32 weight next to a bf16 x (autocast O1)
        w32 = big[:, :256].contiguous()
        with torch.autocast("cuda", dtype=BF16):
            out = F.linear(x, w32, bias)
        _gemm_rel_ok(out, x.float() @ w32.to(BF16).float() + bias.float(), tol=2e-2)
    assert calls == ["decode_gemm_mfma"]


@pytest.mark.gpu
def test_weight_only_linear_int8_fp16_scale_falls_back_gpu(monkeypatch):
    from paddle_amd import quantization as Q
    calls = _record(monkeypatch, "decode_gemm_int8")
    x, (qw, sc), bias, ref = _edge_case("int8", 16, 128)
    _int8_ok(Q.weight_only_linear(x, qw, sc, bias), ref + bias.float())
    assert calls == ["decode_gemm_int8"]
    out = Q.weight_only_linear(x, qw, sc.half(), bias)
    assert calls == ["decode_gemm_int8"]
    _int8_ok(out, x.float() @ (qw.float() * sc.half().float().unsqueeze(0) / 127.0)
             + bias.float())
