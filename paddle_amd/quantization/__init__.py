"""paddle.quantization parity subset: PTQ observers + weight quant utils.

Reference: python/paddle/quantization/ -- config + quanter registry.
MI355X note: the serving-grade path is fp8 (OCP e4m3) for MFMA; int8
abs-max quant provided for parity/export.
"""
from __future__ import annotations

import torch


def abs_max_quant(x, bits=8):
    qmax = 2 ** (bits - 1) - 1
    scale = x.abs().amax().clamp(min=1e-8) / qmax
    q = torch.clamp(torch.round(x / scale), -qmax - 1, qmax).to(torch.int8)
    return q, scale


def channel_wise_abs_max_quant(x, axis=0, bits=8):
    qmax = 2 ** (bits - 1) - 1
    dims = [i for i in range(x.dim()) if i != axis]
    scale = x.abs().amax(dim=dims, keepdim=True).clamp(min=1e-8) / qmax
    q = torch.clamp(torch.round(x / scale), -qmax - 1, qmax).to(torch.int8)
    return q, scale.squeeze()


def dequant(q, scale):
    return q.float() * scale


def fp8_quant(x):
    """OCP e4m3fn cast + per-tensor scale (gfx950 MFMA fp8 format)."""
    amax = x.abs().amax().clamp(min=1e-8)
    scale = 448.0 / amax  # e4m3fn max normal
    return (x * scale).to(torch.float8_e4m3fn), scale


def fp8_dequant(q, scale):
    return q.to(torch.float32) / scale


class BaseObserver(__import__("torch").nn.Module):
    """Activation-range observer (reference paddle/quantization/observer.py
    family): tracks running abs-max during calibration forwards."""

    def __init__(self, quant_bits=8):
        super().__init__()
        import torch
        self.quant_bits = quant_bits
        self.register_buffer("absmax", torch.zeros(()))

    def forward(self, x):
        import torch
        with torch.no_grad():
            m = x.detach().abs().amax().float()
            if m > self.absmax:
                self.absmax.fill_(m)
        return x

    def scale(self):
        qmax = 2 ** (self.quant_bits - 1) - 1
        return (self.absmax.clamp(min=1e-8) / qmax)


class BaseQuanter(__import__("torch").nn.Module):
    """Fake-quantizer (reference paddle/quantization/quanters/abs_max.py):
    quantize-dequantize with a straight-through estimator so QAT
    backprops through the rounding."""

    def __init__(self, quant_bits=8):
        super().__init__()
        import torch
        self.quant_bits = quant_bits
        self.register_buffer("absmax", torch.zeros(()))

    def forward(self, x):
        import torch
        qmax = 2 ** (self.quant_bits - 1) - 1
        with torch.no_grad():
            m = x.detach().abs().amax().float()
            if self.training and m > self.absmax:
                self.absmax.fill_(m)
        s = self.absmax.clamp(min=1e-8) / qmax
        q = (x / s).round().clamp(-qmax, qmax) * s
        # straight-through: forward quantized, backward identity
        return x + (q - x.to(q.dtype)).detach()


def quanter(name):
    """Reference paddle.quantization.quanter class decorator: registers a
    quanter factory under `name`."""
    def deco(cls):
        _QUANTER_REGISTRY[name] = cls
        return cls
    return deco


_QUANTER_REGISTRY = {"FakeQuanterWithAbsMax": BaseQuanter}


class QuantConfig:
    """reference paddle/quantization/config.py: which layers get which
    activation/weight quanters."""

    def __init__(self, activation=None, weight=None):
        self.activation = activation
        self.weight = weight
        self._types = None

    def add_type_config(self, layer_types, activation=None, weight=None):
        self._types = tuple(layer_types) if isinstance(layer_types, (list, tuple)) \
            else (layer_types,)
        if activation is not None:
            self.activation = activation
        if weight is not None:
            self.weight = weight

    def _match(self, layer):
        import torch
        if self._types is not None:
            return isinstance(layer, self._types)
        w = getattr(layer, "weight", None)
        return (type(layer).__name__ in ("Linear", "Conv2D", "Conv2d")
                and isinstance(w, torch.Tensor))


class _QuantedLayer(__import__("torch").nn.Module):
    """Wrapper inserted by PTQ/QAT: observer/fake-quant on the input and
    (for QAT) on the weight."""

    def __init__(self, layer, act_q, weight_q=None):
        super().__init__()
        self.layer = layer
        self.act_q = act_q
        self.weight_q = weight_q

    def forward(self, *args, **kwargs):
        args = (self.act_q(args[0]),) + args[1:]
        if self.weight_q is not None:
            w = self.layer.weight
            orig = w.data
            self.layer.weight.data = self.weight_q(orig)
            try:
                return self.layer(*args, **kwargs)
            finally:
                self.layer.weight.data = orig
        return self.layer(*args, **kwargs)


def _wrap_layers(model, config, make_act, make_w):
    n = 0
    for mod in list(model.modules()):
        for name, child in list(mod._modules.items()):
            if child is None or isinstance(child, _QuantedLayer):
                continue
            if config._match(child):
                mod._modules[name] = _QuantedLayer(child, make_act(),
                                                   make_w() if make_w else None)
                n += 1
    return n


class PTQ:
    """Post-training quantization (reference paddle/quantization/ptq.py):
    quantize() inserts observers, run calibration forwards, convert()
    bakes int8 weights + the observed activation fake-quant."""

    def __init__(self, config: QuantConfig = None):
        self.config = config or QuantConfig()

    def quantize(self, model, inplace=False):
        import copy
        m = model if inplace else copy.deepcopy(model)
        _wrap_layers(m, self.config, lambda: BaseObserver(), None)
        return m

    def convert(self, model, inplace=True):
        import torch
        qmax = 127
        for mod in model.modules():
            if isinstance(mod, _QuantedLayer):
                if isinstance(mod.act_q, BaseObserver):
                    fq = BaseQuanter()
                    fq.absmax.copy_(mod.act_q.absmax)
                    fq.eval()
                    mod.act_q = fq
                w = getattr(mod.layer, "weight", None)
                if isinstance(w, torch.Tensor):
                    with torch.no_grad():
                        s = w.abs().amax().clamp(min=1e-8) / qmax
                        w.copy_(((w / s).round().clamp(-qmax, qmax)) * s)
        return model


class QAT:
    """Quantization-aware training (reference paddle/quantization/qat.py):
    quantize() inserts straight-through fake-quanters on activations and
    weights so training sees int8 rounding."""

    def __init__(self, config: QuantConfig = None):
        self.config = config or QuantConfig()

    def quantize(self, model, inplace=False):
        import copy
        m = model if inplace else copy.deepcopy(model)
        act_cls = self.config.activation or BaseQuanter
        w_cls = self.config.weight or BaseQuanter
        act_f = act_cls if callable(act_cls) else BaseQuanter
        _wrap_layers(m, self.config, lambda: _mk(act_f), lambda: _mk(w_cls))
        return m

    def convert(self, model, inplace=True):
        for mod in model.modules():
            if isinstance(mod, _QuantedLayer):
                mod.eval()
        return model


def _mk(cls_or_inst):
    import copy
    if isinstance(cls_or_inst, type):
        return cls_or_inst()
    try:
        return copy.deepcopy(cls_or_inst)
    except Exception:
        return BaseQuanter()


# -- weight-only int8 / int4 (serving decode path) ---------------------------
# parity: paddle/phi/kernels/weight_quantize_kernel.cu + funcs/weight_only_gemv.cu
_WO_ALGOS = {"weight_only_int8": "int8", "weight_only_int4": "int4"}
_WO_GROUP_SIZES = (-1, 64, 128)


def _wo_check(algo=None, weight_dtype=None, group_size=-1):
    """Validate the weight-only arguments; returns "int8" | "int4"."""
    if algo is not None:
        if algo not in _WO_ALGOS:
            raise ValueError(f"unknown weight-only algo {algo!r}; expected one "
                             f"of {sorted(_WO_ALGOS)}")
        weight_dtype = _WO_ALGOS[algo]
    if weight_dtype not in ("int8", "int4"):
        raise ValueError(f"weight_dtype must be 'int8' or 'int4', got "
                         f"{weight_dtype!r}")
    if group_size not in _WO_GROUP_SIZES:
        raise ValueError(f"group_size must be one of {_WO_GROUP_SIZES}, got "
                         f"{group_size!r}")
    if weight_dtype == "int8" and group_size != -1:
        raise NotImplementedError("int8 weight-only supports per-channel "
                                  "scales only (group_size=-1)")
    return weight_dtype


def weight_quantize(w, algo="weight_only_int8", group_size=-1):
    """w [K, N] (paddle Linear layout) -> (qweight, scale).

    weight_only_int8: qweight [K, N] int8 row-major, scale [N] fp32,
    per-output-channel absmax; w ~ qw * scale / 127.

    weight_only_int4 storage format (K even; K % group_size == 0 with
    groups):
      * scale, fp32, absmax clamped at 1e-8: [N] over all of k for
        group_size=-1, or [K/gs, N] with scale[g, n] taken over
        k in [g*gs, (g+1)*gs) for group_size gs in (64, 128);
      * codes q = round(w / scale * 7) clamped to [-7, 7] (never -8), so
        w ~ q * scale / 7 -- the int8 convention with 7 for 127;
      * qweight int8 [K/2, N] row-major: byte (kp, n) =
        (q[2kp, n] & 0xF) | ((q[2kp+1, n] & 0xF) << 4), two's-complement
        nibbles, even k in the low nibble.
    Dequantization evaluates q * (scale * fp32(1/7)) in fp32.

    The [K, N]-derived layouts feed the MFMA W-streaming decode kernels
    with coalesced rows (the round-1 [N, K] GEMV layout read 180-330 GB/s;
    the streamer reads at the memory roofline on HALF the bytes)."""
    import torch
    wd = _wo_check(algo=algo, group_size=group_size)
    wf = w.detach().float()                          # [K, N]
    if wd == "int8":
        scale = wf.abs().amax(dim=0).clamp(min=1e-8)     # [N]
        q = torch.round(wf / scale.unsqueeze(0) * 127.0).clamp(-127, 127).to(torch.int8)
        return q.contiguous(), scale
    k, n = wf.shape
    if k % 2:
        raise ValueError(f"weight_only_int4 needs an even K, got {k}")
    if group_size == -1:
        scale = wf.abs().amax(dim=0).clamp(min=1e-8)     # [N]
    else:
        if k % group_size:
            raise ValueError(f"K={k} is not a multiple of group_size={group_size}")
        scale = wf.reshape(k // group_size, group_size, n).abs().amax(dim=1)
        scale = scale.clamp(min=1e-8)                    # [K/gs, N]
    q = torch.round(wf / _wo_int4_expand_scale(scale, k, group_size) * 7.0)
    q = q.clamp(-7, 7).to(torch.int32)
    packed = (q[0::2] & 0xF) | ((q[1::2] & 0xF) << 4)    # 0..255
    return packed.to(torch.uint8).view(torch.int8).contiguous(), scale.contiguous()


def _wo_int4_expand_scale(scale, k, group_size):
    """scale [N] | [K/gs, N] -> broadcastable against [K, N]."""
    if group_size == -1:
        return scale.reshape(1, -1)
    return scale.repeat_interleave(group_size, dim=0)


def _wo_int4_unpack(qweight):
    """packed int8 [K/2, N] -> codes int8 [K, N] (even k = low nibble)."""
    import torch
    lo = (((qweight & 0xF) ^ 8) - 8).to(torch.int8)   # sign-extend 4 bits
    hi = qweight >> 4                                 # arithmetic shift
    return torch.stack((lo, hi), dim=1).reshape(2 * qweight.shape[0],
                                                qweight.shape[1])


def _wo_int4_scale_ok(qweight, scale, group_size):
    """scale has the documented shape for qweight / group_size."""
    if qweight.dim() != 2 or group_size not in _WO_GROUP_SIZES:
        return False
    k, n = 2 * qweight.shape[0], qweight.shape[1]
    if group_size == -1:
        return tuple(scale.shape) == (n,)
    return k % group_size == 0 and tuple(scale.shape) == (k // group_size, n)


def _wo_int4_dequant_torch(qweight, scale, group_size):
    """torch composite of the documented format: fp32 [K, N]."""
    if not _wo_int4_scale_ok(qweight, scale, group_size):
        raise ValueError(
            f"int4 scale shape {tuple(scale.shape)} does not fit qweight "
            f"{tuple(qweight.shape)} with group_size={group_size}")
    k = 2 * qweight.shape[0]
    s = _wo_int4_expand_scale(scale.float(), k, group_size)
    return _wo_int4_unpack(qweight).float() * (s * (1.0 / 7.0))


def _wo_int4_dequant_native_ok(qweight, scale, group_size, out_dtype):
    """Contract of the dequant_int4 kernel (pure: dtypes, shapes,
    contiguity)."""
    import torch
    return (isinstance(qweight, torch.Tensor) and isinstance(scale, torch.Tensor)
            and qweight.dtype == torch.int8 and qweight.dim() == 2
            and qweight.is_contiguous() and qweight.numel() > 0
            and qweight.shape[1] % 8 == 0
            and scale.dtype == torch.float32 and scale.is_contiguous()
            and _wo_int4_scale_ok(qweight, scale, group_size)
            and out_dtype in (torch.bfloat16, torch.float32))


def _wo_int4_native_ok(x, qweight, scale, bias=None, group_size=-1):
    """Contract of the decode_gemm_int4 streamer (pure: dtypes, shapes,
    contiguity, storage offsets -- no CUDA call): the shared streamer
    contract (bf16 x with 1..32 rows, N % 256 == 0, K % 64 == 0, 16-byte
    aligned starts) with packed int4 storage, group_size in (-1, 64, 128)
    and K % group_size == 0."""
    import torch
    from ..ops.functional import _decode_stream_ok
    return (_wo_int4_dequant_native_ok(qweight, scale, group_size,
                                       torch.bfloat16)
            and _decode_stream_ok(x, qweight, 2 * qweight.shape[0], bias))


def _wo_int8_native_ok(x, qweight, scale, bias=None):
    """Contract of the decode_gemm_int8 streamer (pure, as above): the
    shared streamer contract with an int8 contiguous [K, N] qweight and a
    contiguous fp32 [N] scale on its device."""
    import torch
    from ..ops.functional import _decode_stream_ok
    return (isinstance(qweight, torch.Tensor) and isinstance(scale, torch.Tensor)
            and qweight.dtype == torch.int8 and qweight.dim() == 2
            and qweight.is_contiguous()
            and scale.dtype == torch.float32 and scale.is_contiguous()
            and scale.device == qweight.device
            and tuple(scale.shape) == (qweight.shape[1],)
            and _decode_stream_ok(x, qweight, qweight.shape[0], bias))


def weight_only_linear(x, qweight, scale, bias=None, weight_dtype="int8",
                       group_size=-1):
    """x [..., K] @ dequant(qweight) + bias.  Decode shapes (<= 32 rows)
    run the int8 / int4 MFMA W-streaming kernel; int4 prefill shapes
    dequantize in one dequant_int4 pass; the fallback dequantizes in
    torch.  int4 operands use the weight_quantize storage format."""
    from .. import _ext
    wd = _wo_check(weight_dtype=weight_dtype, group_size=group_size)
    if wd == "int4":
        return _wo_int4_linear(x, qweight, scale, bias, group_size)
    k, n = qweight.shape
    if (x.is_cuda and _ext.use_native(x)
            and _wo_int8_native_ok(x, qweight, scale, bias)):
        C = _ext.get_ext()
        b = bias.to(x.dtype).contiguous() if bias is not None else None
        out = C.decode_gemm_int8(x.reshape(-1, k).contiguous(), qweight,
                                 scale, b)
        return out.reshape(*x.shape[:-1], n)
    w = (qweight.float() * scale.unsqueeze(0) / 127.0).to(x.dtype)  # [K,N]
    out = x @ w
    if bias is not None:
        out = out + bias
    return out


def _wo_int4_linear(x, qweight, scale, bias, group_size):
    from .. import _ext
    n = qweight.shape[1]
    w = None
    if x.is_cuda and _ext.use_native(x):
        C = _ext.get_ext()
        if _wo_int4_native_ok(x, qweight, scale, bias, group_size):
            b = bias.to(x.dtype).contiguous() if bias is not None else None
            out = C.decode_gemm_int4(x.reshape(-1, x.shape[-1]).contiguous(),
                                     qweight, scale, b, group_size, 0)
            return out.reshape(*x.shape[:-1], n)
        if _wo_int4_dequant_native_ok(qweight, scale, group_size, x.dtype):
            w = C.dequant_int4(qweight, scale, group_size, x.dtype)
    if w is None:
        w = _wo_int4_dequant_torch(qweight, scale, group_size).to(x.dtype)
    out = x @ w
    if bias is not None:
        out = out + bias
    return out


class WeightOnlyLinear(__import__("torch").nn.Module):
    """Drop-in replacement for a (paddle-layout) nn.Linear holding int8
    or packed int4 weights; decode shapes run the MFMA W-streaming
    kernels, larger shapes dequantize on the fly.  Reference:
    paddle/nn/quant weight-only path."""

    def __init__(self, qweight, scale, bias=None, weight_dtype="int8",
                 group_size=-1):
        super().__init__()
        self.weight_dtype = _wo_check(weight_dtype=weight_dtype,
                                      group_size=group_size)
        self.group_size = group_size
        self.register_buffer("qweight", qweight)
        self.register_buffer("scale", scale)
        self.register_buffer("wo_bias", bias)
        # int4 packs two k rows per byte
        self.in_features = qweight.shape[0] * (2 if self.weight_dtype == "int4" else 1)
        self.out_features = qweight.shape[1]

    @classmethod
    def from_linear(cls, linear, algo="weight_only_int8", group_size=-1):
        qw, sc = weight_quantize(linear.weight.detach(), algo=algo,
                                 group_size=group_size)
        dev = linear.weight.device
        bias = getattr(linear, "bias", None)
        return cls(qw.to(dev), sc.to(dev),
                   bias.detach().clone() if bias is not None else None,
                   weight_dtype=_WO_ALGOS[algo], group_size=group_size)

    def forward(self, x):
        return weight_only_linear(x, self.qweight, self.scale, self.wo_bias,
                                  weight_dtype=self.weight_dtype,
                                  group_size=self.group_size)


def quantize_linears_(model, min_features=1024, skip=("lm_head",),
                      algo="weight_only_int8", group_size=-1):
    """Replace every Linear child of `model` (recursively) whose weight
    is at least [min_features, min_features] with a WeightOnlyLinear --
    int8 weights (~2x less weight memory for serving) or, with
    algo="weight_only_int4", packed int4 weights (~4x less).  Returns the
    number of layers converted."""
    import torch
    _wo_check(algo=algo, group_size=group_size)
    n = 0

    def walk(mod, prefix=""):
        nonlocal n
        for name, child in list(mod._modules.items()):
            if child is None:
                continue
            full = f"{prefix}{name}"
            if any(s in full for s in skip):
                continue
            w = getattr(child, "weight", None)
            if (type(child).__name__ == "Linear" and isinstance(w, torch.Tensor)
                    and w.dim() == 2 and min(w.shape) >= min_features):
                mod._modules[name] = WeightOnlyLinear.from_linear(
                    child, algo=algo, group_size=group_size)
                n += 1
            else:
                walk(child, full + ".")

    walk(model)
    return n
