"""paddle.nn.quant (reference: python/paddle/nn/quant/__init__.py --
weight_only linear + quant stubs)."""
from ...quantization import (  # noqa: F401
    weight_only_linear,
    weight_quantize,
)


def weight_dequantize(qweight, scale, algo="weight_only_int8", out_dtype=None,
                      group_size=-1):
    """Inverse of weight_quantize: [K, N] in out_dtype (default float16).
    int4 operands use the packed weight_quantize storage format; on GPU
    tensors bf16 / fp32 outputs take the dequant_int4 kernel."""
    import torch
    from ... import _ext
    from ... import quantization as Q
    wd = Q._wo_check(algo=algo, group_size=group_size)
    out_dtype = out_dtype or torch.float16
    if wd == "int8":
        # weight_quantize layout: qweight [K, N], per-output-channel scale [N]
        w = qweight.float() * scale.unsqueeze(0) / 127.0
        return w.to(out_dtype)
    if (qweight.is_cuda and _ext.use_native(qweight)
            and Q._wo_int4_dequant_native_ok(qweight, scale, group_size,
                                             out_dtype)):
        return _ext.get_ext().dequant_int4(qweight, scale, group_size, out_dtype)
    return Q._wo_int4_dequant_torch(qweight, scale, group_size).to(out_dtype)


def llm_int8_linear(x, qweight, scale, bias=None, threshold=6.0):
    return weight_only_linear(x, qweight, scale, bias)
