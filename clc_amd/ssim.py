"""pytorch_msssim's 2-D API on the HIP SSIM kernels: `ssim`, `ms_ssim`, and the modules `SSIM`, `MS_SSIM`.

Same signatures, defaults (data_range=255) and argument checks as pytorch_msssim, for 4-D fp32 images on the GPU with any
number of channels and any size.  Both inputs are differentiable.  The windowed statistics, the 2x2 average pooling between
scales (padding H % 2, W % 2) and their backward passes run in clc_amd/csrc/msssim.hip; what remains in torch is the product of
powers over [levels, B, C] values.

Differences from pytorch_msssim:
  * the window is a 1-D Gaussian of 3 to 15 taps (odd); a custom `win` must carry the same taps for every channel;
  * an image side smaller than the window raises ValueError (pytorch_msssim warns and skips filtering along that axis);
  * no 5-D (video) inputs, and fp32 only.
`clc_amd.ops.ms_ssim` / `clc_amd.train.ms_ssim` are the same computation with data_range=1.0 by default and without the
minimum-size rule of `ms_ssim` below.
"""
from __future__ import annotations

import torch

from . import ops

__all__ = ["ssim", "ms_ssim", "SSIM", "MS_SSIM"]


def _check_pair(X, Y):
    if not X.shape == Y.shape:
        raise ValueError(f"Input images should have the same dimensions, but got {X.shape} and {Y.shape}.")
    if X.dim() != 4:
        raise ValueError(f"Input images should be 4-d tensors (5-d video inputs are not supported), but got {X.shape}")
    if X.dtype != torch.float32 or Y.dtype != torch.float32:
        raise ValueError(f"Input images should be float32, but got {X.dtype} and {Y.dtype}")


def ssim(X, Y, data_range=255, size_average=True, win_size=11, win_sigma=1.5, win=None, K=(0.01, 0.03), nonnegative_ssim=False):
    """pytorch_msssim.ssim: mean SSIM of X against Y, a scalar, or [B] when size_average=False."""
    _check_pair(X, Y)
    taps = ops.ssim_window_taps(win_size, win_sigma, win)
    if min(X.shape[-2:]) < len(taps):
        raise ValueError(f"Image sides {tuple(X.shape[-2:])} should be at least the window size {len(taps)}")
    v = ops.ssim_stats(X, Y, 1, taps, data_range, K)[0, :, :, 1]
    if nonnegative_ssim:
        v = torch.relu(v)
    return v.mean() if size_average else v.mean(1)


def ms_ssim(X, Y, data_range=255, size_average=True, win_size=11, win_sigma=1.5, win=None, weights=None, K=(0.01, 0.03)):
    """pytorch_msssim.ms_ssim: multi-scale SSIM over len(weights) scales (default 5), a scalar, or [B] when size_average=False."""
    _check_pair(X, Y)
    taps = ops.ssim_window_taps(win_size, win_sigma, win)
    smaller_side = min(X.shape[-2:])
    if not smaller_side > (len(taps) - 1) * 2 ** 4:
        raise ValueError("Image size should be larger than %d due to the 4 downsamplings in ms-ssim" % ((len(taps) - 1) * 2 ** 4))
    weights = ops.MS_SSIM_WEIGHTS if weights is None else tuple(float(w) for w in weights)
    side = smaller_side
    for _ in range(len(weights) - 1):
        side = (side + 1) // 2
    if side < len(taps):
        raise ValueError(f"{len(weights)} scales shrink the smaller side {smaller_side} to {side}, below the window size {len(taps)}")
    return ops.ms_ssim_combine(ops.ssim_stats(X, Y, len(weights), taps, data_range, K), weights, size_average)


class SSIM(torch.nn.Module):
    """pytorch_msssim.SSIM.  `channel` sets the shape of `self.win` ([channel, 1, 1, win_size]); any channel count is accepted."""

    def __init__(self, data_range=255, size_average=True, win_size=11, win_sigma=1.5, channel=3, spatial_dims=2, K=(0.01, 0.03),
                 nonnegative_ssim=False):
        super().__init__()
        if spatial_dims != 2:
            raise ValueError("only spatial_dims=2 is supported")
        self.win_size = win_size
        self.win = torch.tensor(ops.ssim_window(win_size, win_sigma)).repeat([channel, 1, 1, 1])
        self.size_average = size_average
        self.data_range = data_range
        self.K = K
        self.nonnegative_ssim = nonnegative_ssim

    def forward(self, X, Y):
        return ssim(X, Y, data_range=self.data_range, size_average=self.size_average, win=self.win, K=self.K,
                    nonnegative_ssim=self.nonnegative_ssim)


class MS_SSIM(torch.nn.Module):
    """pytorch_msssim.MS_SSIM."""

    def __init__(self, data_range=255, size_average=True, win_size=11, win_sigma=1.5, channel=3, spatial_dims=2, weights=None,
                 K=(0.01, 0.03)):
        super().__init__()
        if spatial_dims != 2:
            raise ValueError("only spatial_dims=2 is supported")
        self.win_size = win_size
        self.win = torch.tensor(ops.ssim_window(win_size, win_sigma)).repeat([channel, 1, 1, 1])
        self.size_average = size_average
        self.data_range = data_range
        self.weights = weights
        self.K = K

    def forward(self, X, Y):
        return ms_ssim(X, Y, data_range=self.data_range, size_average=self.size_average, win=self.win, weights=self.weights, K=self.K)
