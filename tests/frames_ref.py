"""The definition of clc_amd/frames.py in plain torch float64: BT.709 full range, F.interpolate(scale_factor=2,
align_corners=False) for the chroma, F.pad(mode="replicate"), F.avg_pool2d, torch.round (half to even).  CPU only; the kernels are
checked against this, never the other way round."""
import math

import torch
import torch.nn.functional as F

KR, KG, KB = 0.2126, 0.7152, 0.0722


def rgb2ycbcr(rgb):
    """[..., 3, H, W] -> [..., 3, H, W] (y, cb, cr)"""
    r, g, b = rgb.unbind(-3)
    y = KR * r + KG * g + KB * b
    return torch.stack((y, 0.5 * (b - y) / (1 - KB) + 0.5, 0.5 * (r - y) / (1 - KR) + 0.5), dim=-3)


def ycbcr2rgb(ycc):
    y, cb, cr = ycc.unbind(-3)
    r = y + (2 - 2 * KR) * (cr - 0.5)
    b = y + (2 - 2 * KB) * (cb - 0.5)
    return torch.stack((r, (y - KR * r - KB * b) / KG, b), dim=-3)


def samples(p):
    """a sample plane (uint8, or int16 holding 16-bit patterns) -> its values as float64"""
    return (p.to(torch.int64) & (0xFF if p.dtype == torch.uint8 else 0xFFFF)).double()


def yuv420_to_rgb(Y, U, V, bit_depth, mode="bilinear", size=None):
    """-> float64 [N, 3, Hp, Wp], unclamped, replicate-padded"""
    mx = float(2 ** bit_depth - 1)
    c = F.interpolate(torch.stack((samples(U), samples(V)), dim=1) / mx, scale_factor=2, mode=mode, align_corners=False)
    rgb = ycbcr2rgb(torch.cat((samples(Y)[:, None] / mx, c), dim=1))
    if size is not None:
        rgb = F.pad(rgb, (0, size[1] - rgb.shape[3], 0, size[0] - rgb.shape[2]), mode="replicate")
    return rgb


def rgb_to_yuv420_values(rgb, size, bit_depth):
    """float [N, 3, Hp, Wp] -> the float64 values BEFORE the clamp and the rounding, in samples: (y [N, H, W], u, v [N, H/2, W/2])"""
    mx = float(2 ** bit_depth - 1)
    ycc = rgb2ycbcr(rgb.double()[:, :, :size[0], :size[1]].clamp(0, 1))
    c = F.avg_pool2d(ycc[:, 1:], 2)
    return ycc[:, 0] * mx, c[:, 0] * mx, c[:, 1] * mx


def quantise(v, bit_depth):
    """pre-rounding float64 values -> integer samples as int64"""
    return torch.round(v.clamp(0, float(2 ** bit_depth - 1))).to(torch.int64)


def psnr(a, b, bit_depth):
    """float64 PSNR of two sample planes over all their elements"""
    mse = ((samples(a) - samples(b)) ** 2).mean().item()
    return math.inf if mse == 0 else 10 * math.log10((2 ** bit_depth - 1) ** 2 / mse)


def psnr_yuv(pa, pb, bit_depth):
    y, u, v = (psnr(a, b, bit_depth) for a, b in zip(pa, pb))
    return (4 * y + u + v) / 6
