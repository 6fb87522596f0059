"""The two operators of the scale-space-flow video model (``ssf2020``) on the HIP kernels of csrc/scale_space.hip, with autograd:

    volume = scale_space_volume(x, sigma0=1.5, num_levels=5)     # [N, 3, H, W] -> [N, 3, D, H, W], D = num_levels + 1
    y      = scale_space_warp(volume, flow, scale)               # F.grid_sample(volume, identity grid + (flow | scale),
                                                                 #               padding_mode="border", align_corners=False)

Definition: V0 = x, V1 = blur(x), and per further level a 2x2 average pool, a blur and i bilinear x2 upsamplings
(align_corners=False) back to full resolution; blur = the normalised Gaussian of 2 ceil(3 sigma0) + 1 taps with replicate padding.
flow [N, 2, H, W] holds normalised displacements (channel 0 along the width, 1 along the height), scale [N, 1, H, W] the normalised
depth coordinate; coordinates are clamped to the border and a clamped coordinate takes no gradient (torch's rule).

Gradients reach the frame, the volume, the flow and the scale.  Every sum has a fixed order — the volume gradient of the warp is a
sorted gather, not float atomics — so forward and backward are bit-identical run to run and for an image alone or inside a batch.

The volume tensor is a view of the kernels' [N, H, W, D, 4] buffer (depth and channel innermost, channels padded to four);
scale_space_warp takes it without a copy, and repacks any other 5-D tensor of that shape.  GPU float32 only: no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math

import torch
from torch.autograd import Function

from . import lib as _lib
from . import ops
from .ops import _L, _require_gpu, _stream, new_act, nhwc

__all__ = ["gaussian_taps", "scale_space_volume", "scale_space_warp"]


def gaussian_taps(sigma0):
    """the k = 2 ceil(3 sigma0) + 1 taps exp(-0.5 (t / sigma0)^2), t = -(k-1)/2 .. (k-1)/2, normalised to sum 1 (float64 -> float32)"""
    sigma0 = float(sigma0)
    if not sigma0 > 0.0:
        raise ValueError(f"scale_space: sigma0 must be positive (got sigma0={sigma0})")
    k = 2 * int(math.ceil(3.0 * sigma0)) + 1
    if k > _lib.SS_MAX_TAPS:
        raise ValueError(f"scale_space: sigma0={sigma0} needs {k} taps; the kernels take at most {_lib.SS_MAX_TAPS} (sigma0 <= {(_lib.SS_MAX_TAPS - 1) // 2 / 3.0:.3f})")
    g = [math.exp(-0.5 * ((i - (k - 1) / 2.0) / sigma0) ** 2) for i in range(k)]
    s = math.fsum(g)
    return tuple(v / s for v in g)


def _check_levels(num_levels, H, W):
    if int(num_levels) != num_levels or num_levels < 1:
        raise ValueError(f"scale_space: num_levels must be an integer >= 1 (got num_levels={num_levels})")
    m = 2 ** (int(num_levels) - 1)
    if H % m or W % m:
        raise ValueError(f"scale_space: H and W must be divisible by 2^(num_levels-1) = {m} (got H={H}, W={W})")


def _desc(N, H, W, levels, taps):
    d = _lib.SsDesc()
    d.N, d.H, d.W, d.levels, d.ntaps = N, H, W, levels, len(taps)
    for i, v in enumerate(taps):
        d.taps[i] = v
    return d


def _bytes(n, like):
    return torch.empty(max(int(n), 1), device=like.device, dtype=torch.uint8)


def _as_volume(buf):
    """the kernels' [N, H, W, D, 4] buffer as the logical [N, 3, D, H, W] tensor (a view)"""
    return buf.permute(0, 4, 3, 1, 2)[:, :3]


def _volume_buffer(v, zero_pad):
    """logical [N, 3, D, H, W] -> the [N, H, W, D, 4] buffer: the tensor's own storage when it is a view made by _as_volume, else a repack"""
    N, Cc, D, H, W = v.shape
    want = (H * W * D * 4, 1, 4, W * D * 4, D * 4)
    if (v.stride() == want and v.data_ptr() % 16 == 0
            and (v.storage_offset() + N * H * W * D * 4) * 4 <= v.untyped_storage().nbytes()):
        return v.as_strided((N, H, W, D, 4), (H * W * D * 4, W * D * 4, D * 4, 4, 1), v.storage_offset())
    buf = (torch.zeros if zero_pad else torch.empty)((N, H, W, D, 4), device=v.device, dtype=torch.float32)
    buf[..., :3] = v.permute(0, 3, 4, 2, 1)
    return buf


class _VolumeFn(Function):
    @staticmethod
    def forward(ctx, x, taps, levels):
        x, xp, N, H, W, _c, ldx = nhwc(x)
        d = _desc(N, H, W, levels, taps)
        nbytes = _L().clc_ss_volume_workspace_bytes(C.byref(d))
        ws = _bytes(nbytes, x)
        buf = torch.empty((N, H, W, levels + 1, 4), device=x.device, dtype=torch.float32)
        _lib.check(_L().clc_ss_volume_fwd(C.byref(d), xp, ldx, buf.data_ptr(), ws.data_ptr(), nbytes, _stream()), "clc_ss_volume_fwd")
        ctx.cfg = (taps, levels)
        return _as_volume(buf)

    @staticmethod
    def backward(ctx, g):
        taps, levels = ctx.cfg
        N, _c, D, H, W = g.shape
        gb = _volume_buffer(g, False)
        d = _desc(N, H, W, levels, taps)
        nbytes = _L().clc_ss_volume_workspace_bytes(C.byref(d))
        ws = _bytes(nbytes, g)
        dx = new_act(N, 3, H, W, g)
        _lib.check(_L().clc_ss_volume_bwd(C.byref(d), gb.data_ptr(), dx.data_ptr(), 3, ws.data_ptr(), nbytes, _stream()), "clc_ss_volume_bwd")
        return dx, None, None


def scale_space_volume(x, sigma0=1.5, num_levels=5):
    """x [N, 3, H, W] -> the scale-space volume [N, 3, num_levels + 1, H, W]; differentiable in x."""
    taps = gaussian_taps(sigma0)
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"scale_space_volume: x must be [N, 3, H, W] (got {tuple(x.shape)})")
    _check_levels(num_levels, x.shape[2], x.shape[3])
    if num_levels > 12:
        raise ValueError(f"scale_space_volume: num_levels must be at most 12 (got num_levels={num_levels})")
    _require_gpu(x, "scale_space_volume")
    return _VolumeFn.apply(x, taps, int(num_levels))


class _WarpFn(Function):
    @staticmethod
    def forward(ctx, volume, flow, scale):
        N, _c, D, H, W = volume.shape
        vb = _volume_buffer(volume, True)
        flow, fp, *_a, ldf = nhwc(flow)
        scale, sp, *_b, lds = nhwc(scale)
        y = new_act(N, 3, H, W, flow)
        _lib.check(_L().clc_ss_warp_fwd(vb.data_ptr(), N, H, W, D, fp, ldf, sp, lds, y.data_ptr(), 3, _stream()), "clc_ss_warp_fwd")
        ctx.dims = (N, H, W, D)
        ctx.save_for_backward(vb, flow, scale)
        return y

    @staticmethod
    def backward(ctx, dy):
        N, H, W, D = ctx.dims
        vb, flow, scale = ctx.saved_tensors
        flow, fp, *_a, ldf = nhwc(flow)
        scale, sp, *_b, lds = nhwc(scale)
        dy, dp, *_c, lddy = nhwc(dy)
        need_v, need_f, need_s = ctx.needs_input_grad
        dfs = new_act(N, 3, H, W, dy) if (need_f or need_s) else None   # (dflow | dscale) as one map: the model's flow and scale are one, too
        dvb, ws, nbytes = None, None, 0
        if need_v:
            dvb = torch.empty((N, H, W, D, 4), device=dy.device, dtype=torch.float32)
            nbytes = _L().clc_ss_warp_bwd_workspace_bytes(N, H, W, D)
            if nbytes == 0:
                _lib.check(-1, "clc_ss_warp_bwd_workspace_bytes")
            ws = _bytes(nbytes, dy)
        _lib.check(_L().clc_ss_warp_bwd(vb.data_ptr(), N, H, W, D, fp, ldf, sp, lds, dp, lddy,
                                        dfs.data_ptr() if need_f else None, 3, dfs.data_ptr() + 8 if need_s else None, 3,
                                        dvb.data_ptr() if need_v else None, ws.data_ptr() if ws is not None else None, nbytes, _stream()),
                   "clc_ss_warp_bwd")
        return (_as_volume(dvb) if need_v else None), (dfs[:, :2] if need_f else None), (dfs[:, 2:3] if need_s else None)


def scale_space_warp(volume, flow, scale):
    """volume [N, 3, D, H, W], flow [N, 2, H, W], scale [N, 1, H, W] -> the warped frame [N, 3, H, W]; differentiable in all three."""
    if volume.dim() != 5 or volume.shape[1] != 3:
        raise ValueError(f"scale_space_warp: volume must be [N, 3, D, H, W] (got {tuple(volume.shape)})")
    N, _c, D, H, W = volume.shape
    if tuple(flow.shape) != (N, 2, H, W):
        raise ValueError(f"scale_space_warp: flow must be [N, 2, H, W] = {(N, 2, H, W)} (got {tuple(flow.shape)})")
    if tuple(scale.shape) != (N, 1, H, W):
        raise ValueError(f"scale_space_warp: scale must be [N, 1, H, W] = {(N, 1, H, W)} (got {tuple(scale.shape)})")
    for name, t in (("volume", volume), ("flow", flow), ("scale", scale)):
        _require_gpu(t, f"scale_space_warp: {name}")
    return _WarpFn.apply(volume, flow, scale)
