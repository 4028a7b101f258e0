"""MXFP4 torch path (CPU tensors, checkpoint loaders): the rule's error
bound, the scale rule and the packed byte order."""
import torch

from paddle_amd.incubate import mx


def test_roundtrip_error_is_half_a_grid_step():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(16, 256, generator=g) * torch.exp2(
        torch.randint(-10, 11, (16, 8, 1), generator=g).float()).expand(16, 8, 32).reshape(16, 256)
    codes, scales = mx.mx_quantize(x)
    assert codes.shape == (16, 128) and scales.shape == (16, 8)
    back = mx.mx_dequantize(codes, scales, torch.float64)
    step = torch.exp2(scales.double() - 127).repeat_interleave(32, 1)     # 2^e
    y = x.double().abs() / step
    # grid step is .5 below 2, 1 in [2, 4], 2 in [4, 6]: half of it in each
    # binade; y in (6, 8) saturates to 6 (amax < 2^(e+3) keeps y below 8)
    half = torch.where(y <= 2, 0.25, torch.where(y <= 4, 0.5,
                       torch.where(y <= 7, 1.0, y - 6)))
    assert bool(((back - x.double()).abs() <= half * step).all())


def test_scale_is_floor_log2_amax_minus_2():
    for p in (-126, -20, 0, 3, 100):
        for top in (1.0, 1.5, 1.9921875):
            x = torch.zeros(1, 32, dtype=torch.float64)
            x[0, 5] = -top * 2.0 ** p
            _, scales = mx.mx_quantize(x.float())
            assert int(scales[0, 0]) == max(p - 2, -127) + 127
    assert int(mx.mx_quantize(torch.zeros(1, 32))[1][0, 0]) == 127


def test_packed_byte_order():
    x = torch.zeros(1, 32)
    x[0, :4] = torch.tensor([6.0, -0.5, 1.5, 3.0])     # codes 7, 9, 3, 5
    codes, scales = mx.mx_quantize(x)
    assert int(scales[0, 0]) == 127 and codes[0, :2].tolist() == [0x97, 0x53]
    assert mx.mx_dequantize(codes, scales)[0, :4].tolist() == [6.0, -0.5, 1.5, 3.0]
