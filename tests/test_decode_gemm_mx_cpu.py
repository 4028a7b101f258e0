"""MXFP4 weight-only surface without a GPU: storage layout, the torch path of
weight_only_linear, the streamer's pure contract predicate, and that the int8 /
int4 formats did not move."""
import pytest
import torch

import paddle_amd as paddle
from paddle_amd import quantization as Q
from paddle_amd.incubate import mx


def _wx(k=256, n=128, rows=5):
    g = torch.Generator().manual_seed(11)
    return torch.randn(k, n, generator=g) * 0.05, torch.randn(rows, k, generator=g)


def test_quantize_and_linear_cpu():
    w, x = _wx()
    qw, sc = Q.weight_quantize(w, algo="weight_only_mxfp4")
    assert qw.dtype == sc.dtype == torch.uint8
    assert qw.shape == (128, 128) and sc.shape == (128, 8)          # N-major
    eq, es = mx.mx_quantize(w.t().contiguous())
    assert torch.equal(qw, eq) and torch.equal(sc, es)
    bias = torch.linspace(-1, 1, 128)
    wd = mx.mx_dequantize(qw, sc, torch.float64)
    ref = x.double() @ wd.t() + bias.double()
    # fp32 matmul: K roundings of the running sum, one more for the bias
    bound = 2.0 ** -23 * ref.abs() + 256 * 2.0 ** -24 * (x.double().abs() @ wd.abs().t())
    out = Q.weight_only_linear(x, qw, sc, bias, weight_dtype="mxfp4")
    assert bool(((out.double() - ref).abs() <= bound).all())

    lin = paddle.nn.Linear(256, 128)
    layer = Q.WeightOnlyLinear.from_linear(lin, algo="weight_only_mxfp4")
    assert (layer.weight_dtype, layer.in_features, layer.out_features) == ("mxfp4", 256, 128)
    assert torch.equal(layer(x), Q.weight_only_linear(
        x, layer.qweight, layer.scale, layer.wo_bias, weight_dtype="mxfp4"))
    soft = mx.MXFP4Linear(qw, sc, bias, activation="bf16")
    assert torch.equal(soft(x), out)
    with pytest.raises(ValueError, match="activation"):
        mx.MXFP4Linear(qw, sc, activation="fp8")


def test_native_predicate_and_check():
    x = torch.zeros(8, 256, dtype=torch.bfloat16)
    qw = torch.zeros(64, 128, dtype=torch.uint8)
    sc = torch.zeros(64, 8, dtype=torch.uint8)
    ok = Q._wo_mxfp4_native_ok
    assert ok(x, qw, sc) and ok(x.reshape(2, 4, 256), qw, sc, torch.zeros(64))
    shifted = torch.zeros(64 * 128 + 8, dtype=torch.uint8)[8:].reshape(64, 128)
    refused = [
        (torch.zeros(33, 256, dtype=torch.bfloat16), qw, sc),              # rows
        (x.float(), qw, sc),                                               # x dtype
        (x[:, :192], qw[:, :96].contiguous(), sc[:, :6].contiguous()),     # K % 128
        (x, torch.zeros(96, 128, dtype=torch.uint8), torch.zeros(96, 8, dtype=torch.uint8)),
        (x, qw, torch.zeros(64, 12, dtype=torch.uint8)),                   # scale shape
        (x, qw.to(torch.int8), sc),                                        # codes dtype
        (x, shifted, sc),                                                  # alignment
        (x, qw, sc, torch.zeros(32)),                                      # bias length
    ]
    assert not any(ok(*args) for args in refused)
    assert Q._wo_check(algo="weight_only_mxfp4") == "mxfp4"
    with pytest.raises(NotImplementedError):
        Q._wo_check(weight_dtype="mxfp4", group_size=64)


def test_int8_int4_unchanged():
    w, _ = _wx(128, 16)
    q8, s8 = Q.weight_quantize(w, algo="weight_only_int8")
    amax = w.abs().amax(0).clamp(min=1e-8)
    assert torch.equal(s8, amax)
    assert torch.equal(q8, torch.round(w / amax * 127.0).clamp(-127, 127).to(torch.int8))
    q4, s4 = Q.weight_quantize(w, algo="weight_only_int4", group_size=64)
    gmax = w.reshape(2, 64, 16).abs().amax(1).clamp(min=1e-8)
    codes = torch.round(w / gmax.repeat_interleave(64, 0) * 7.0).clamp(-7, 7).int()
    packed = ((codes[0::2] & 15) | ((codes[1::2] & 15) << 4)).to(torch.uint8).view(torch.int8)
    assert torch.equal(s4, gmax) and torch.equal(q4, packed)


def test_convert_and_runner_cpu():
    model = torch.nn.Module()
    model.a = paddle.nn.Linear(256, 128)
    model.b = paddle.nn.Linear(192, 128)      # in % 128 != 0
    model.c = paddle.nn.Linear(256, 96)       # out % 64 != 0
    assert Q.quantize_linears_(model, min_features=64, algo="weight_only_mxfp4") == 1
    assert isinstance(model.a, Q.WeightOnlyLinear) and model.a.weight_dtype == "mxfp4"
    assert mx.convert_linears_to_mxfp4(model, min_features=64, activation="bf16") == 1
    assert model.c.activation == "bf16"

    from paddle_amd.models.llama import LlamaConfig, LlamaForCausalLM
    from paddle_amd.serving import Engine, LlamaModelRunner, Request
    paddle.seed(0)
    cfg = LlamaConfig(vocab_size=512, hidden_size=1024, num_layers=2, num_heads=8,
                      num_kv_heads=8, intermediate_size=1024, max_seq_len=128)
    kw = dict(num_blocks=64, block_size=16, device=torch.device("cpu"), max_seq=128)
    model = LlamaForCausalLM(cfg).to("cpu").float().eval()
    with pytest.raises(ValueError, match="mxfp4"):
        LlamaModelRunner(model, weight_only="int2", **kw)
    runner = LlamaModelRunner(model, weight_only="mxfp4", **kw)
    for kind, qw, sc, gs in runner._qkv_fused:
        assert (kind, gs) == ("mxfp4", -1)
        assert tuple(qw.shape) == (3072, 512) and tuple(sc.shape) == (3072, 32)
    eng = Engine(runner, num_blocks=64, block_size=16, max_batch=2)
    reqs = [Request(prompt_ids=[3, 7, 11, 20], max_new_tokens=2) for _ in range(2)]
    for r in reqs:
        eng.add_request(r)
    eng.run_until_done()
    assert all(r.done and len(r.out_ids) == 2 for r in reqs)
