"""MXFP4 (OCP microscaling fp4) storage and compute for gfx950.

Format: e2m1 codes, two per byte (element 2i in the low nibble of byte i),
uint8 [R, K/2]; one e8m0 scale per 32 elements along K, uint8 [R, K/32], value
2^(byte - 127).  About 4.25 bits per value.

Quantization rule (finite inputs), per 32-element block: e = floor(log2 amax)
- 2 from the exponent bits of the fp32 amax, clamped to [-127, 127]; scale
byte e + 127; amax == 0 gives byte 127 and zero codes; each element is
x * 2^-e rounded to the nearest of {0, .5, 1, 1.5, 2, 3, 4, 6}, ties to the
even code, saturating at 6.

GPU bf16 tensors are quantized by the HIP kernel and multiplied by the
block-scaled fp4 MFMA GEMM (csrc/kernels/gemm_mx.hip); everything else (CPU
tensors, checkpoint loaders) follows the torch implementation of the same
rule below.  Forward only.
"""
from __future__ import annotations

import torch

E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
BLOCK = 32


def _ext():
    from .. import _ext
    return _ext.get_ext(required=True)


def _quantize_torch(x):
    r, k = x.shape
    xf = x.detach().float()
    blocks = xf.reshape(r, k // BLOCK, BLOCK)
    mag = blocks.abs()
    amax = mag.amax(-1)
    ebits = (amax.contiguous().view(torch.int32) >> 23) & 0xFF
    sbyte = torch.where(amax == 0, torch.full_like(ebits, 127),
                        ebits.clamp(min=2) - 2)
    y = mag * torch.ldexp(torch.ones_like(amax), 127 - sbyte).unsqueeze(-1)
    code = ((y > 0.25).int() + (y >= 0.75).int() + (y > 1.25).int()
            + (y >= 1.75).int() + (y > 2.5).int() + (y >= 3.5).int()
            + (y > 5.0).int())
    code = (code | (torch.signbit(blocks).int() << 3)).reshape(r, k // 2, 2)
    codes = (code[..., 0] | (code[..., 1] << 4)).to(torch.uint8)
    return codes, sbyte.to(torch.uint8)


def mx_quantize(x):
    """x [R, K] (K % 32 == 0) -> (codes uint8 [R, K/2], scales uint8 [R, K/32])."""
    if x.dim() != 2 or x.shape[1] % BLOCK != 0 or x.shape[1] == 0:
        raise ValueError(f"mx_quantize: x must be [R, K] with K a multiple of "
                         f"{BLOCK}, got {tuple(x.shape)}")
    if x.is_cuda and x.dtype == torch.bfloat16:
        if x.stride(1) != 1 or x.stride(0) % 8 != 0 or x.data_ptr() % 16 != 0:
            x = x.contiguous()
        codes, scales = _ext().mx_quant_fp4(x)
        return codes, scales
    return _quantize_torch(x)


def mx_dequantize(codes, scales, dtype=torch.float32):
    """(codes [R, K/2], scales [R, K/32]) -> [R, K] of `dtype`."""
    r, kb = codes.shape
    work = torch.float64 if dtype == torch.float64 else torch.float32
    lut = torch.tensor(E2M1_VALUES + tuple(-v for v in E2M1_VALUES),
                       dtype=work, device=codes.device)
    nib = torch.stack((codes & 0xF, codes >> 4), dim=-1).reshape(r, 2 * kb)
    vals = lut[nib.long()].reshape(r, 2 * kb // BLOCK, BLOCK)
    out = torch.ldexp(vals, (scales.to(torch.int32) - 127).unsqueeze(-1))
    return out.reshape(r, 2 * kb).to(dtype)


def mxfp4_gemm_nt(qa, sa, qb, sb, bias=None):
    """bf16 [M, N] = dequant(qa, sa) @ dequant(qb, sb)^T (+ bias[N]) on the
    block-scaled fp4 MFMA kernel; fp32 accumulation."""
    return _ext().gemm_mxfp4_nt(qa, sa, qb, sb, bias)


class MXFP4Linear(torch.nn.Module):
    """Linear whose weight is held in MXFP4.  Inference only.

    activation="mxfp4" (default): the forward quantizes the activations per
    call and runs the fp4 GEMM.  activation="bf16": the activations stay bf16
    (W4A16) and the forward is quantization.weight_only_linear(weight_dtype=
    "mxfp4") -- the decode W-streamer for up to 32 rows, dequantize + linear
    above that."""

    def __init__(self, qweight, weight_scale, bias=None, activation="mxfp4"):
        super().__init__()
        if activation not in ("mxfp4", "bf16"):
            raise ValueError("MXFP4Linear: activation must be 'mxfp4' or 'bf16', "
                             f"got {activation!r}")
        self.activation = activation
        self.out_features = qweight.shape[0]
        self.in_features = qweight.shape[1] * 2
        self.register_buffer("qweight", qweight)            # [out, in/2]
        self.register_buffer("weight_scale", weight_scale)  # [out, in/32]
        self.register_buffer("bias", bias)

    @classmethod
    def from_linear(cls, linear, activation="mxfp4"):
        """From a paddle-layout Linear (weight [in, out]), quantized once along in."""
        w = linear.weight.detach()
        if w.dim() != 2 or w.shape[0] % 128 != 0:
            raise ValueError("MXFP4Linear.from_linear: weight must be [in, out] "
                             f"with in a multiple of 128, got {tuple(w.shape)}")
        q, s = mx_quantize(w.t().contiguous())
        b = getattr(linear, "bias", None)
        if b is not None:
            b = b.detach().to(torch.bfloat16).contiguous()
        return cls(q, s, b, activation=activation)

    def forward(self, x):
        if torch.is_grad_enabled() and x.requires_grad:
            raise RuntimeError("MXFP4Linear is forward only: the input requires "
                               "grad; run it under torch.no_grad() or detach it")
        if self.activation == "bf16":
            from ..quantization import weight_only_linear
            return weight_only_linear(x, self.qweight, self.weight_scale,
                                      self.bias, weight_dtype="mxfp4")
        x2 = x.reshape(-1, self.in_features)
        if x2.is_cuda:
            qx, sx = mx_quantize(x2.to(torch.bfloat16))
            out = mxfp4_gemm_nt(qx, sx, self.qweight, self.weight_scale, self.bias)
        else:
            qx, sx = mx_quantize(x2)
            out = mx_dequantize(qx, sx) @ mx_dequantize(self.qweight, self.weight_scale).t()
            if self.bias is not None:
                out = out + self.bias.float()
        return out.to(x.dtype).reshape(*x.shape[:-1], self.out_features)

    def extra_repr(self):
        return (f"in={self.in_features}, out={self.out_features}, mxfp4, "
                f"activation={self.activation}")


def convert_linears_to_mxfp4(model, min_features=256, skip=("lm_head",),
                             activation="mxfp4"):
    """Replace paddle Linear layers by MXFP4Linear(activation=...) in place
    (weights quantized once).  Small layers, skipped names and layers whose
    `in` is not a multiple of 128 are left alone.  Returns the converted count."""
    todo = []
    for name, mod in model.named_modules():
        if type(mod).__name__ != "Linear" or not hasattr(mod, "weight"):
            continue
        if mod.weight.dim() != 2 or any(s in name for s in skip):
            continue
        in_f, out_f = mod.weight.shape
        if min(in_f, out_f) < min_features or in_f % 128 != 0 or not name:
            continue
        todo.append(name)
    for name in todo:
        parent_name, _, child = name.rpartition(".")
        parent = model.get_submodule(parent_name) if parent_name else model
        setattr(parent, child, MXFP4Linear.from_linear(getattr(parent, child),
                                                       activation=activation))
    return len(todo)
