"""Video frames in and out of the model's layout on the HIP kernels of csrc/frame_io.hip:

    rgb      = yuv420_to_rgb(Y, U, V, bit_depth=8, mode="bilinear", size=(Hp, Wp))   # planes -> [N, 3, Hp, Wp] f32, unclamped, replicate-padded
    Y, U, V  = rgb_to_yuv420(rgb, (H, W), bit_depth=8)                                # crop, clamp, 2x2 chroma mean, round half to even
    sse      = plane_sse(a, b, bit_depth=8)                                           # int64 [N]: exact sum of squared sample differences
    blob     = encode_yuv420(model, planes, bit_depth=8, lanes=4)                     # a list of (Y, U, V) -> one CLV1 container
    planes   = decode_yuv420(model, blob)
    metrics  = sequence_metrics(planes_a, planes_b, bit_depth, blob=blob)

Sample planes are device tensors: uint8 at bit_depth 8, int16 at 9 .. 16 bits holding the samples' 16-bit patterns (values in
[0, 2^bit_depth - 1]; at 16 bits 65535 is -1 as an int16).  Y is [N, H, W]; U and V are [N, H/2, W/2]; contiguous; H and W even.
Colour is BT.709 full range; the formulae and the f32 operation order are in include/clc_hip.h.  The frame is what
ScaleSpaceFlow._prep produces: channels-last f32, so only sample planes and stream words cross PCIe.

At 8 bits neutral chroma is 0.5 * 255 = 127.5, an exact rounding tie: a grey RGB frame lands on 127 or 128 depending on the last bit
of b - y.  That is a property of the definition.

No file reading: a raw .yuv file is numpy.fromfile plus a reshape on the caller's side.  GPU only: no CPU fallback.
"""
from __future__ import annotations

import math
import struct

import torch

from . import lib as _lib
from .ops import CL, _L, _stream, nhwc

__all__ = ["yuv420_to_rgb", "rgb_to_yuv420", "plane_sse", "psnr_yuv420", "encode_yuv420", "decode_yuv420", "sequence_metrics"]

MODES = {"bilinear": 0, "bicubic": 1}   # CLC_CHROMA_BILINEAR, CLC_CHROMA_BICUBIC


def _bit_depth(who, bit_depth):
    if isinstance(bit_depth, bool) or not isinstance(bit_depth, int) or not 8 <= bit_depth <= 16:
        raise ValueError(f"{who}: bit_depth must be an integer 8 .. 16 (got bit_depth={bit_depth!r})")
    return bit_depth, (torch.uint8 if bit_depth == 8 else torch.int16)


def _mode(who, mode):
    if mode not in MODES:
        raise ValueError(f"{who}: mode must be 'bilinear' or 'bicubic' (got mode={mode!r})")
    return MODES[mode]


def _even(who, H, W):
    if H < 2 or W < 2 or H % 2 or W % 2:
        raise ValueError(f"{who}: H and W must be even and at least 2, 4:2:0 has one chroma sample per 2x2 block (got H={H}, W={W})")


def _padded(who, size, H, W):
    Hp, Wp = (H, W) if size is None else (int(size[0]), int(size[1]))
    if Hp < H or Wp < W or Hp % 2 or Wp % 2:
        raise ValueError(f"{who}: the frame size must be even with Hp >= H and Wp >= W (got Hp={Hp}, Wp={Wp} for H={H}, W={W})")
    return Hp, Wp


def _gpu_only(who, *tensors):
    for t in tensors:
        if not t.is_cuda:
            raise _lib.ClcError(f"{who}: tensor is on {t.device}; frame I/O runs on the GPU only (no CPU fallback by design)")


def _check_planes(who, Y, U, V, bit_depth):
    """-> (N, H, W) of a (Y, U, V) triple of the bit depth's dtype and 4:2:0 shapes; everything else is refused by name"""
    bit_depth, dtype = _bit_depth(who, bit_depth)
    for name, t in (("Y", Y), ("U", U), ("V", V)):
        if not isinstance(t, torch.Tensor) or t.dim() != 3:
            raise ValueError(f"{who}: {name} must be a [N, rows, columns] tensor (got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__})")
        if t.dtype != dtype:
            raise ValueError(f"{who}: {name} is {t.dtype}; bit_depth={bit_depth} planes are {dtype}")
    N, H, W = (int(v) for v in Y.shape)
    _even(who, H, W)
    for name, t in (("U", U), ("V", V)):
        if tuple(t.shape) != (N, H // 2, W // 2):
            raise ValueError(f"{who}: {name} must be [N, H/2, W/2] = {(N, H // 2, W // 2)} for Y {tuple(Y.shape)} (got {tuple(t.shape)})")
    if N < 1:
        raise ValueError(f"{who}: empty batch")
    return N, H, W


def yuv420_to_rgb(Y, U, V, bit_depth=8, mode="bilinear", size=None, out=None):
    """(Y, U, V) sample planes -> the unclamped f32 frame [N, 3, Hp, Wp], channels-last.  size=(Hp, Wp) >= (H, W), even (default: the
    true size): output pixel (h, w) is the converted pixel (min(h, H - 1), min(w, W - 1)) — replicate padding.  mode: the x2 chroma
    upsampling, 'bilinear' or 'bicubic' (F.interpolate, align_corners=False).  out: a pixel-major [N, 3, Hp, Wp] f32 map to write."""
    who = "yuv420_to_rgb"
    N, H, W = _check_planes(who, Y, U, V, bit_depth)
    m = _mode(who, mode)
    Hp, Wp = _padded(who, size, H, W)
    _gpu_only(who, Y, U, V)
    Y, U, V = Y.contiguous(), U.contiguous(), V.contiguous()
    if out is None:
        out = torch.empty((N, 3, Hp, Wp), device=Y.device, dtype=torch.float32, memory_format=CL)
    if not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or not out.is_cuda or tuple(out.shape) != (N, 3, Hp, Wp):
        raise ValueError(f"{who}: out must be a float32 device tensor of shape {(N, 3, Hp, Wp)}")
    o, op, *_a, ld = nhwc(out)
    if o.data_ptr() != out.data_ptr() or o.stride() != out.stride():
        raise ValueError(f"{who}: out must be stored pixel-major (strides {out.stride()})")
    _lib.check(_L().clc_yuv420_to_rgb(Y.data_ptr(), U.data_ptr(), V.data_ptr(), bit_depth, N, H, W, m, op, ld, Hp, Wp, _stream()), "clc_yuv420_to_rgb")
    return out


def rgb_to_yuv420(rgb, size=None, bit_depth=8):
    """The f32 frame [N, 3, Hp, Wp] -> (Y, U, V) of its top-left size=(H, W) (default: the whole frame): RGB clamped to [0, 1], the
    matrix, chroma averaged over its 2x2 block, rint(clamp(v, 0, 1) * max) with round half to even."""
    who = "rgb_to_yuv420"
    bit_depth, dtype = _bit_depth(who, bit_depth)
    if not isinstance(rgb, torch.Tensor) or rgb.dim() != 4 or rgb.shape[1] != 3:
        raise ValueError(f"{who}: rgb must be a [N, 3, Hp, Wp] tensor (got {tuple(rgb.shape) if isinstance(rgb, torch.Tensor) else type(rgb).__name__})")
    N, _c, Hp, Wp = (int(v) for v in rgb.shape)
    H, W = (Hp, Wp) if size is None else (int(size[0]), int(size[1]))
    _even(who, H, W)
    _padded(who, (Hp, Wp), H, W)
    if N < 1:
        raise ValueError(f"{who}: empty batch")
    _gpu_only(who, rgb)
    if rgb.dtype != torch.float32:
        raise _lib.ClcError(f"{who}: dtype {rgb.dtype} (fp32 only)")
    rgb, rp, *_a, ld = nhwc(rgb)
    Y = torch.empty((N, H, W), device=rgb.device, dtype=dtype)
    U = torch.empty((N, H // 2, W // 2), device=rgb.device, dtype=dtype)
    V = torch.empty((N, H // 2, W // 2), device=rgb.device, dtype=dtype)
    _lib.check(_L().clc_rgb_to_yuv420(rp, ld, Hp, Wp, N, H, W, bit_depth, Y.data_ptr(), U.data_ptr(), V.data_ptr(), _stream()), "clc_rgb_to_yuv420")
    return Y, U, V


def plane_sse(a, b, bit_depth=8, out=None):
    """Two sample planes [N, ...] of one shape -> int64 [N] on the device: per image the exact sum of squared sample differences
    (64-bit integer sums in two fixed stages: the same bits run to run)."""
    who = "plane_sse"
    bit_depth, dtype = _bit_depth(who, bit_depth)
    for name, t in (("a", a), ("b", b)):
        if not isinstance(t, torch.Tensor) or t.dim() < 2 or t.dtype != dtype:
            raise ValueError(f"{who}: {name} must be a [N, ...] {dtype} tensor at bit_depth={bit_depth}")
    if a.shape != b.shape or a.shape[0] < 1 or a[0].numel() < 1:
        raise ValueError(f"{who}: a and b must have one non-empty shape (got {tuple(a.shape)}, {tuple(b.shape)})")
    _gpu_only(who, a, b)
    a, b = a.contiguous(), b.contiguous()
    N, n = int(a.shape[0]), int(a[0].numel())
    nbytes = _L().clc_plane_sse_workspace_bytes(N, n)
    if nbytes == 0:
        _lib.check(-1, "clc_plane_sse_workspace_bytes")
    ws = torch.empty((nbytes // 8,), device=a.device, dtype=torch.int64)
    if out is None:
        out = torch.empty((N,), device=a.device, dtype=torch.int64)
    if out.dtype != torch.int64 or not out.is_cuda or not out.is_contiguous() or out.numel() != N:
        raise ValueError(f"{who}: out must be a contiguous int64 [N = {N}] device tensor")
    _lib.check(_L().clc_plane_sse(a.data_ptr(), b.data_ptr(), bit_depth, N, n, out.data_ptr(), ws.data_ptr(), nbytes, _stream()), "clc_plane_sse")
    return out


def psnr_yuv420(sse_y, sse_u, sse_v, n_y, bit_depth=8):
    """Host float64: integer SSE sums of the three planes over n_y luma samples (n_y / 4 per chroma plane) ->
    {"psnr_y", "psnr_u", "psnr_v", "psnr_yuv"}, psnr = 10 log10(max^2 n / sse) (inf for identical planes), psnr_yuv = (4 Y + U + V) / 6."""
    bit_depth, _ = _bit_depth("psnr_yuv420", bit_depth)
    n_y = int(n_y)
    if n_y < 4 or n_y % 4 or min(int(sse_y), int(sse_u), int(sse_v)) < 0:
        raise ValueError(f"psnr_yuv420: n_y must be a positive multiple of 4 and the sums non-negative (got n_y={n_y}, sums {int(sse_y)}, {int(sse_u)}, {int(sse_v)})")
    peak = float((1 << bit_depth) - 1) ** 2
    one = lambda sse, n: math.inf if int(sse) == 0 else 10.0 * math.log10(peak * n / float(int(sse)))
    y, u, v = one(sse_y, n_y), one(sse_u, n_y // 4), one(sse_v, n_y // 4)
    return {"psnr_y": y, "psnr_u": u, "psnr_v": v, "psnr_yuv": (4.0 * y + u + v) / 6.0}


# ------------------------------------------------------------------------------------------------ end to end
def _check_sequence(who, planes, bit_depth):
    if not isinstance(planes, (list, tuple)) or len(planes) < 1:
        raise ValueError(f"{who}: planes must be a non-empty list of (Y, U, V)")
    shape = None
    for t, p in enumerate(planes):
        if not isinstance(p, (list, tuple)) or len(p) != 3:
            raise ValueError(f"{who}: frame {t} is not a (Y, U, V) triple")
        got = _check_planes(f"{who}: frame {t}", *p, bit_depth)
        if shape is not None and got != shape:
            raise ValueError(f"{who}: frames of differing shapes (frame 0 is {shape}, frame {t} is {got})")
        shape = got
    return shape


def encode_yuv420(model, planes, bit_depth=8, lanes=4, mode="bilinear", q=None):
    """A list of (Y, U, V) device planes -> one CLV1 container (codec.pack_sequence): yuv420_to_rgb pads each frame to the next
    multiples of 128 (replicate), model.compress(frames, lanes=lanes) codes them.  lanes=None: the default stream format.
    q (variable rate; a model built with rate_levels > 0): one quality for every frame or a list of one per frame -> the CLVQ wrapper
    around the same container (codec.pack_sequence_q), which carries the qualities as f32 — the values the frames are coded under."""
    from . import codec
    from .vbr import check_quality, frame_qualities

    N, H, W = _check_sequence("encode_yuv420", planes, bit_depth)
    _mode("encode_yuv420", mode)
    Hp, Wp = -(-H // 128) * 128, -(-W // 128) * 128
    if q is None:
        frames = [yuv420_to_rgb(*p, bit_depth=bit_depth, mode=mode, size=(Hp, Wp)) for p in planes]
        frame_strings, shape_infos = model.compress(frames, lanes=lanes)
        return codec.pack_sequence(frame_strings, shape_infos, lanes=lanes, image_hw=(H, W), bit_depth=bit_depth)
    qs = frame_qualities(q, len(planes), "encode_yuv420")
    table_owner = getattr(model, "img_hyperprior", model)   # every refusal of q comes before the first launch
    qs = [check_quality(table_owner, qt, f"encode_yuv420 (frame {t})") for t, qt in enumerate(qs)]
    qs = [struct.unpack("<f", struct.pack("<f", float(qt)))[0] for qt in qs]   # the decoder reads f32: code under what it will read
    frames = [yuv420_to_rgb(*p, bit_depth=bit_depth, mode=mode, size=(Hp, Wp)) for p in planes]
    frame_strings, shape_infos = model.compress(frames, lanes=lanes, q=qs)
    return codec.pack_sequence_q(codec.pack_sequence(frame_strings, shape_infos, lanes=lanes, image_hw=(H, W), bit_depth=bit_depth), qs)


def decode_yuv420(model, blob, mode="bilinear", bit_depth=None):
    """A CLV1 container -> the list of (Y, U, V) of the true size: codec.unpack_sequence, model.decompress under the container's lanes,
    then rgb_to_yuv420 crops and quantises.  bit_depth: default the container's.  mode: the encoder's chroma mode, checked by name;
    the way back is the 2x2 mean under both.  A CLVQ wrapper (encode_yuv420(..., q=)) is recognised by its magic and decoded under
    the qualities it carries."""
    from . import codec

    _mode("decode_yuv420", mode)
    qs = None
    if bytes(blob[:4]) == codec.SEQ_Q_MAGIC:
        blob, qs = codec.unpack_sequence_q(blob)
    frame_strings, shape_infos, meta = codec.unpack_sequence(blob)
    bit_depth = meta["bit_depth"] if bit_depth is None else bit_depth
    if bit_depth is None:
        raise ValueError("decode_yuv420: the container records no bit depth; pass bit_depth=")
    if qs is None:
        recs = model.decompress(frame_strings, shape_infos, lanes=meta["lanes"])
    else:
        recs = model.decompress(frame_strings, shape_infos, lanes=meta["lanes"], q=qs)
    return [rgb_to_yuv420(x, meta["image_hw"], bit_depth=bit_depth) for x in recs]


def sequence_metrics(planes_a, planes_b, bit_depth=8, blob=None):
    """Two lists of (Y, U, V) -> {"frames": [per frame psnr_y / psnr_u / psnr_v / psnr_yuv], "mean": their means over the frames,
    "bpp": 8 len(blob) / (frames x N x H x W) when a container is given}.  A frame's sums run over its whole batch.  The sums are
    formed on the device (plane_sse) and come to the host in ONE copy; the PSNRs are float64 on the host (psnr_yuv420)."""
    who = "sequence_metrics"
    N, H, W = _check_sequence(who, planes_a, bit_depth)
    if len(planes_b) != len(planes_a) or _check_sequence(who, planes_b, bit_depth) != (N, H, W):
        raise ValueError(f"{who}: the two sequences differ in length or shape")
    F = len(planes_a)
    sums = torch.empty((F, 3, N), device=planes_a[0][0].device, dtype=torch.int64)
    for t, (pa, pb) in enumerate(zip(planes_a, planes_b)):
        for k in range(3):
            plane_sse(pa[k], pb[k], bit_depth, out=sums[t, k])
    host = sums.cpu().numpy().sum(axis=2)
    frames = [psnr_yuv420(int(host[t, 0]), int(host[t, 1]), int(host[t, 2]), N * H * W, bit_depth) for t in range(F)]
    out = {"frames": frames, "mean": {k: sum(f[k] for f in frames) / F for k in frames[0]}}
    if blob is not None:
        out["bpp"] = 8.0 * len(blob) / (F * N * H * W)
    return out
