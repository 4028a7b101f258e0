"""The decode W-streamer contract without a GPU: the pure predicates of the
bf16 and int8 formats over the case tables of test_decode_stream_gpu.py, and
their agreement with the contract rows of docs/KERNELS.md.
"""
import os
import re

import pytest
import torch

from paddle_amd import quantization as Q
from paddle_amd.ops import functional as hot

from test_decode_stream_gpu import (BF16, F32, INT8_BAD, MFMA_BAD, int8_valid,
                                    mfma_valid)

CPU = "cpu"
FORMATS = {
    "decode_gemm_mfma": (hot._decode_gemm_native_ok, mfma_valid, MFMA_BAD),
    "decode_gemm_int8": (Q._wo_int8_native_ok, int8_valid, INT8_BAD),
}


def _accepted(op):
    """name -> operands the predicate must accept."""
    _, valid, _ = FORMATS[op]
    v = valid(CPU)
    cases = {
        "valid": v,
        "no bias": {**v, "bias": None},
        "M=1": valid(CPU, m=1),
        "M=32": valid(CPU, m=32),
        "K=64": valid(CPU, k=64),
        "x [2, 2, K]": {**v, "x": v["x"].reshape(2, 2, 128)},
        "x aligned view": {**v, "x": torch.zeros(5, 128, dtype=BF16)[1:]},
    }
    if op == "decode_gemm_mfma":
        cases["w column slice, stride 512"] = {
            **v, "w": torch.zeros(128, 512, dtype=BF16)[:, 256:512]}
    return cases


def _rejected(op):
    """name -> operands the predicate must reject: the contract table's, and
    what only a predicate can be handed."""
    _, valid, bad = FORMATS[op]
    v = valid(CPU)
    wkey = "w" if op == "decode_gemm_mfma" else "qw"
    cases = {name: make(CPU) for name, (make, pred_ok) in bad.items()
             if not pred_ok}
    cases.update({
        "x fp16": {**v, "x": v["x"].half()},
        "no rows": {**v, "x": v["x"][:0]},
        "K mismatch": {**v, "x": v["x"][:, :64]},
        "x view misaligned by 2 bytes": {
            **v, "x": torch.zeros(4 * 128 + 8, dtype=BF16)[1:513].view(4, 128)},
        "integer bias": {**v, "bias": torch.zeros(256, dtype=torch.int32)},
        "x None": {**v, "x": None},
        "weight None": {**v, wkey: None},
        "weight 3-D": {**v, wkey: v[wkey].reshape(1, 128, 256)},
    })
    if op == "decode_gemm_int8":
        cases["qw int16"] = {**v, "qw": v["qw"].to(torch.int16)}
        cases["scale [1, N]"] = {**v, "scale": v["scale"].reshape(1, 256)}
        cases["scale strided"] = {**v, "scale": torch.ones(512)[::2]}
    return cases


@pytest.mark.parametrize("op", list(FORMATS))
def test_decode_stream_predicates(op):
    ok = FORMATS[op][0]
    for name, args in _accepted(op).items():
        assert ok(*args.values()), f"{op} {name}: rejected"
    for name, args in _rejected(op).items():
        assert not ok(*args.values()), f"{op} {name}: accepted"
    # operands the dispatch site repairs before the call stay on the kernel
    repaired = [n for n, (_, pred_ok) in FORMATS[op][2].items() if pred_ok]
    assert sorted(repaired) == ["bias fp32", "x non-contiguous"]
    for name in repaired:
        assert ok(*FORMATS[op][2][name][0](CPU).values()), f"{op} {name}"


# ---------------------------------------------------------------------------
# docs/KERNELS.md: the contract row, read back
# ---------------------------------------------------------------------------
def _doc_row(op):
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                        "docs", "KERNELS.md")
    with open(path, encoding="utf-8") as f:
        rows = [l for l in f if l.startswith(f"| `{op}` |")]
    assert len(rows) == 1, f"{op}: expected one contract row, found {len(rows)}"
    return rows[0]


def _doc_ok(op, row, x, w, *rest):
    """The documented row, evaluated with the numbers it states."""
    def num(pattern):
        m = re.search(pattern, row)
        assert m, f"{op}: contract row does not state {pattern!r}"
        return int(m.group(1))
    rows_min, rows_max = num(r"(\d+) ≤ rows"), num(r"rows ≤ (\d+)")
    n_mult, k_mult = num(r"N % (\d+) == 0"), num(r"K % (\d+) == 0")
    k_max, align = 2 ** num(r"K ≤ 2\^(\d+)"), num(r"(\d+)-byte aligned")
    bias = rest[-1]
    tensors = [x, w] + list(rest[:-1])
    if not all(isinstance(t, torch.Tensor) for t in tensors):
        return False
    if x.dtype != BF16 or w.dim() != 2 or x.dim() < 1:
        return False
    k, n = w.shape
    if x.shape[-1] != k or k == 0 or not rows_min <= x.numel() // k <= rows_max:
        return False
    if n == 0 or n % n_mult or k % k_mult or k > k_max:
        return False
    # x reaches the kernel as a contiguous [rows, K]: a copy is aligned
    if x.is_contiguous() and x.storage_offset() * x.element_size() % align:
        return False
    if w.storage_offset() * w.element_size() % align:
        return False
    if op == "decode_gemm_mfma":
        assert "w bf16" in row and "column stride 1" in row
        if (w.dtype != BF16 or w.stride(1) != 1
                or w.stride(0) % num(r"row stride % (\d+) == 0")):
            return False
    else:
        assert "qw int8 contiguous" in row and "scale fp32 contiguous `[N]`" in row
        scale = rest[0]
        if not (w.dtype == torch.int8 and w.is_contiguous() and scale.dtype == F32
                and scale.is_contiguous() and tuple(scale.shape) == (n,)):
            return False
    assert "floating-point bias" in row and "N elements" in row
    return bias is None or (bias.is_floating_point() and bias.numel() == n)


@pytest.mark.parametrize("op", list(FORMATS))
def test_decode_stream_predicate_agrees_with_documented_row(op):
    ok, _, bad = FORMATS[op]
    row = _doc_row(op)
    cases = {**_accepted(op), **_rejected(op),
             **{name: make(CPU) for name, (make, _) in bad.items()}}
    seen = set()
    for name, args in cases.items():
        want = _doc_ok(op, row, *args.values())
        assert ok(*args.values()) == want, f"{op} {name}: documented {want}"
        seen.add(want)
    assert seen == {True, False}
