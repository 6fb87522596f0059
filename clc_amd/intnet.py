"""Integer hyper-synthesis: the entropy parameters of a hyperprior model in integer arithmetic, so that a stream is not tied
to the build that wrote it.  Balle, Johnston, Minnen, "Integer networks for data compression with latent-variable models" (ICLR 2019),
as a post-training conversion of the float ``h_s``; the kernels are csrc/int_conv.hip (int8 on the i8 matrix cores, requantising
epilogue fused), the arithmetic is stated in include/clc_hip.h.

Integer sums are exact and do not depend on summation order: the scales and means this net hands to the quantise / index / step kernels
are the same f32 bits under every kernel state (``set_precision``, ``CLC_TUNING``), every build and every machine — a CPU included.
"""
from __future__ import annotations

import ctypes as C
import zlib

import numpy as np
import torch
import torch.nn as nn

from . import lib as _lib
from . import ops

BIAS_MAX = 1 << 30
W_FLOOR = 2.0 ** -16   # floor of max|w| of an output channel and of a layer's amax: a dead channel does not divide by zero
F0_CAP = 4
_FIELDS = ("w", "bias", "mult_pos", "mult_neg", "shift")


def check_channels(channels, who="IntegerHyperSynthesis"):
    """every layer's Cin and Cout must be a multiple of 32 (one i8 MFMA tile); refused by name before any launch"""
    channels = tuple(int(c) for c in channels)
    if len(channels) != 4 or any(c < 32 or c % 32 for c in channels):
        raise ValueError(f"{who}: the integer hyper-synthesis net needs every layer's channel count to be a positive multiple of 32 "
                         f"(the i8 matrix-core tile); got {channels}")
    return channels


def choose_f0(z_absmax):
    """the largest f0 <= 4 with max|z| * 2^f0 <= 127"""
    f0 = F0_CAP
    while f0 > 0 and float(z_absmax) * 2.0 ** f0 > 127.0:
        f0 -= 1
    return f0


def multiplier(rho, slope):
    """the real factor rho > 0 -> (mult_pos in [2^30, 2^31), mult_neg = rint(rho * slope * 2^shift), shift)"""
    mant, e = np.frexp(np.float64(rho))   # rho = mant * 2^e, mant in [0.5, 1)
    mp = int(np.rint(np.ldexp(mant, 31)))
    if mp == 1 << 31:
        mp, e = 1 << 30, e + 1
    shift = 31 - int(e)
    if not 1 <= shift <= 62:
        raise ValueError(f"integer hyper-synthesis: the requantising factor {float(rho)!r} needs shift {shift}, outside 1 .. 62")
    mn = mp if slope == 1.0 else min(int(np.rint(np.ldexp(np.float64(rho) * np.float64(slope), shift))), (1 << 31) - 1)
    return mp, mn, shift


def convert(weights, biases, amax, slopes, f0, f_out=8):
    """THE CONVERSION, float64 on the host and deterministic.  weights / biases: the three float layers in torch's layouts (layers 1, 2
    ConvTranspose2d [Cin, Cout, 5, 5]; layer 3 Conv2d [Cout, Cin, 3, 3]); amax[i]: the largest |activation| after layer i's activation
    over the calibration inputs (i = 0, 1; the last layer's output step is 2^-f_out); slopes[i]: the negative-side slope of layer i's
    activation (0 ReLU, 0.01 LeakyReLU, 1 none).  Per output channel s_w = max|w| / 127, w_q = clamp(rint(w / s_w), +-127),
    bias_q = clamp(rint(b / (s_in s_w)), +-2^30), and the real factor s_in s_w / s_out as (mult_pos, mult_neg, shift).
    -> per layer a dict of numpy arrays (w int8, the rest int32)."""
    layers = []
    s_in = 2.0 ** -int(f0)
    for i in range(3):
        w = np.asarray(weights[i], dtype=np.float64)
        b = np.asarray(biases[i], dtype=np.float64)
        co_axis = 1 if i < 2 else 0
        wmax = np.abs(w).max(axis=tuple(a for a in range(4) if a != co_axis))
        s_w = np.maximum(wmax, W_FLOOR) / 127.0
        shape = [1, 1, 1, 1]
        shape[co_axis] = -1
        w_q = np.clip(np.rint(w / s_w.reshape(shape)), -127, 127).astype(np.int8)
        s_out = max(float(amax[i]), W_FLOOR) / 127.0 if i < 2 else 2.0 ** -int(f_out)
        bias_q = np.clip(np.rint(b / (s_in * s_w)), -BIAS_MAX, BIAS_MAX).astype(np.int32)
        mp, mn, sh = (np.empty(len(s_w), dtype=np.int32) for _ in range(3))
        for c in range(len(s_w)):
            mp[c], mn[c], sh[c] = multiplier(s_in * s_w[c] / s_out, float(slopes[i]))
        layers.append({"w": w_q, "bias": bias_q, "mult_pos": mp, "mult_neg": mn, "shift": sh})
        s_in = s_out
    return layers


def pack_filter(w_q, transposed):
    """THE PACKED FILTER of clc_int_conv (include/clc_hip.h): the canonical int8 filter -> int8 [Cout / 32][T][Cin / 32][2][32][16],
    entry [ct][t][kc][h][r][j] = the weight of output channel 32 ct + r, tap t = kh * K + kw, input channel 32 kc + 16 h + j — lane
    h * 32 + r of the wave's A fragment, 16 bytes, one aligned load."""
    w = np.asarray(w_q, dtype=np.int8)
    g = w.transpose(1, 2, 3, 0) if transposed else w.transpose(0, 2, 3, 1)   # [Cout][kh][kw][Cin]
    Cout, K, _, Cin = g.shape
    g = g.reshape(Cout // 32, 32, K * K, Cin // 32, 2, 16)                   # [ct][r][t][kc][h][j]
    return np.ascontiguousarray(g.transpose(0, 2, 3, 4, 1, 5))


def int_conv(x, w_packed, bias, mult_pos, mult_neg, shift, Cout, transposed, out=None, f32_out=False, f_out=0):
    """One layer on clc_int_conv.  x: int8 [B, H, W, Cin] NHWC (a leading dimension above Cin is taken from stride(2)); out: the
    caller's buffer ([B, OH, OW, >= Cout], int8 or f32) or None -> allocated dense."""
    if not x.is_cuda or x.dtype != torch.int8 or x.dim() != 4 or x.stride(3) != 1:
        raise _lib.ClcError(f"int_conv: x must be an int8 NHWC [B, H, W, Cin] tensor on the GPU (got {x.dtype} {tuple(x.shape)} on {x.device})")
    B, H, W, Cin = x.shape
    ldx = x.stride(2)
    if x.stride(1) != W * ldx or x.stride(0) != H * W * ldx:
        raise _lib.ClcError(f"int_conv: x must be dense in its pixels (strides {x.stride()})")
    OH, OW = (2 * H, 2 * W) if transposed else (H, W)
    dt = torch.float32 if f32_out else torch.int8
    if out is None:
        out = torch.empty((B, OH, OW, Cout), device=x.device, dtype=dt)
    if out.dtype != dt or out.dim() != 4 or tuple(out.shape[:3]) != (B, OH, OW) or out.shape[3] < Cout or out.stride(3) != 1 or \
            out.stride(1) != OW * out.stride(2) or out.stride(0) != OH * OW * out.stride(2) or out.device != x.device:
        raise _lib.ClcError(f"int_conv: out must be a {dt} [B, {OH}, {OW}, >= {Cout}] NHWC tensor on {x.device} "
                            f"(got {out.dtype} {tuple(out.shape)} strides {out.stride()})")
    d = _lib.IntConvDesc(x=x.data_ptr(), B=B, H=H, W=W, Cin=Cin, ldx=ldx, w_packed=w_packed.data_ptr(), bias=bias.data_ptr(),
                         mult_pos=mult_pos.data_ptr(), mult_neg=mult_neg.data_ptr(), shift=shift.data_ptr(), y=out.data_ptr(), Cout=Cout,
                         ldy=out.stride(2), transposed=int(bool(transposed)), out_kind=_lib.INT_OUT_F32 if f32_out else _lib.INT_OUT_I8,
                         f_out=int(f_out))
    _lib.check(_lib.load().clc_int_conv(C.byref(d), ops._stream()), "clc_int_conv")
    return out


def int_quantize(z_hat, f0):
    """z_hat f32 [B, C, H, W] (channels-last) -> x0 int8 NHWC [B, H, W, C] = clamp(rint(z * 2^f0), -128, 127) on clc_int_quantize"""
    ops._require_gpu(z_hat, "int_quantize")
    z = z_hat.contiguous(memory_format=ops.CL)
    B, Cc, H, W = z.shape
    x0 = torch.empty((B, H, W, Cc), device=z.device, dtype=torch.int8)
    _lib.check(_lib.load().clc_int_quantize(z.data_ptr(), z.numel(), int(f0), x0.data_ptr(), ops._stream()), "clc_int_quantize")
    return x0


class IntegerHyperSynthesis(nn.Module):
    """The int8 ``h_s`` of a hyperprior model: two 5x5 / stride-2 transposed convolutions and one 3x3 convolution, int8 NHWC
    activations, int8 weights in [-127, 127], one requantising expression for ReLU, LeakyReLU and the linear last layer.

    ``channels`` = (C0, C1, C2, C3), each a multiple of 32; ``split``: the last layer's output is chunked into (scales, means).
    THE BUFFERS (canonical layouts, all in ``state_dict``; zero-filled until from_float / fill / load_state_dict): per layer i = 0, 1, 2
    ``w{i}`` int8 in torch's layout of the float layer, ``bias{i}``, ``mult_pos{i}``, ``mult_neg{i}``, ``shift{i}`` int32 [Cout];
    ``fixed_point`` int32 [2] = (f0, f_out).  The packed filter images of the kernel are derived from them per device and rebuilt when
    a buffer is replaced or rewritten (its object or _version moves), the way the entropy models keep their host tables."""

    def __init__(self, channels, split=False):
        super().__init__()
        self.channels = c = check_channels(channels, type(self).__name__)
        self.split = bool(split)
        if self.split and c[3] % 64:
            raise ValueError(f"{type(self).__name__}: a (scales | means) net needs an even split of multiples of 32 (got Cout = {c[3]})")
        for i in range(3):
            shape = (c[i], c[i + 1], 5, 5) if i < 2 else (c[3], c[2], 3, 3)
            self.register_buffer(f"w{i}", torch.zeros(shape, dtype=torch.int8))
            for k in _FIELDS[1:]:
                self.register_buffer(f"{k}{i}", torch.zeros(c[i + 1], dtype=torch.int32))
        self.register_buffer("fixed_point", torch.zeros(2, dtype=torch.int32))
        self._cache = None

    # ---- filling ----
    def fill(self, layers, f0, f_out):
        """convert()'s layers and the two fixed-point positions into the buffers"""
        for i, layer in enumerate(layers):
            for k in _FIELDS:
                buf = getattr(self, f"{k}{i}")
                t = torch.from_numpy(np.ascontiguousarray(layer[k]))
                if t.shape != buf.shape or t.dtype != buf.dtype:
                    raise ValueError(f"{type(self).__name__}.fill: {k}{i} must be {buf.dtype} {tuple(buf.shape)} (got {t.dtype} {tuple(t.shape)})")
                buf.copy_(t)
        self.fixed_point.copy_(torch.tensor([int(f0), int(f_out)], dtype=torch.int32))
        return self

    @classmethod
    def from_float(cls, weights, biases, amax, slopes, f0, f_out=8, split=False):
        """post-training conversion (convert) of three float layers -> a filled net on the CPU"""
        to_np = lambda t: t.detach().double().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)
        weights, biases = [to_np(w) for w in weights], [to_np(b) for b in biases]
        channels = (weights[0].shape[0], weights[0].shape[1], weights[1].shape[1], weights[2].shape[0])
        net = cls(channels, split=split)
        return net.fill(convert(weights, biases, amax, slopes, f0, f_out), f0, f_out)

    # ---- the host copy: validated integers, the hash, the packed images ----
    def _buffers_key(self):
        return tuple((t, t._version) for t in self.buffers())

    def _state(self):
        key = self._buffers_key()
        c = self._cache
        if c is None or len(c["key"]) != len(key) or any(a[0] is not b[0] or a[1] != b[1] for a, b in zip(c["key"], key)):
            host = {name: t.detach().cpu().numpy() for name, t in self.named_buffers()}
            h = 0
            for i in range(3):
                h = zlib.crc32(np.ascontiguousarray(host[f"w{i}"], dtype=np.int8).tobytes(), h)
                for k in _FIELDS[1:]:
                    h = zlib.crc32(np.ascontiguousarray(host[f"{k}{i}"]).astype("<i4").tobytes(), h)
            h = zlib.crc32(host["fixed_point"].astype("<i4").tobytes(), h) & 0xFFFFFFFF
            f0, f_out = (int(v) for v in host["fixed_point"])
            ready = all(((host[f"shift{i}"] >= 1) & (host[f"shift{i}"] <= 62)).all() and (host[f"mult_pos{i}"] >= 0).all()
                        and (host[f"mult_neg{i}"] >= 0).all() and (np.abs(host[f"bias{i}"].astype(np.int64)) <= BIAS_MAX).all()
                        and (host[f"w{i}"] >= -127).all() for i in range(3)) and 0 <= f0 <= 16 and 0 <= f_out <= 30
            self._cache = c = {"key": key, "host": host, "hash": h, "ready": bool(ready), "f0": f0, "f_out": f_out, "packed": {}}
        return c

    @property
    def ready(self):
        """the buffers hold a converted net (every shift in 1 .. 62, multipliers non-negative, |bias| <= 2^30, weights >= -127)"""
        return self._state()["ready"]

    def spec_hash(self):
        """zlib.crc32, as a u32, over the little-endian bytes of: per layer in order w (int8, C order of its canonical layout), bias,
        mult_pos, mult_neg, shift (int32 each); then (f0, f_out) as int32.  It names the entropy model a stream was written under."""
        return self._state()["hash"]

    def _packed(self, dev):
        st = self._state()
        if dev not in st["packed"]:
            st["packed"][dev] = [torch.from_numpy(pack_filter(st["host"][f"w{i}"], i < 2)).to(dev) for i in range(3)]
        return st["packed"][dev]

    def require_ready(self, who):
        if not self.ready:
            raise ValueError(f"{who}: the integer hyper-synthesis net is not filled (its shifts are outside 1 .. 62): call "
                             "model.integerize(x_calib) or load a state_dict of an integerised model")

    @torch.no_grad()
    def forward(self, z_hat):
        """z_hat f32 [B, C0, h, w] = symbol + median -> (scales, means or None), f32 [B, ., 4h, 4w] channels-last views of the last
        layer's fixed-point output; four launches on the current stream"""
        who = f"{type(self).__name__}.forward"
        self.require_ready(who)
        ops._require_gpu(z_hat, who)
        c = self.channels
        if z_hat.dim() != 4 or z_hat.shape[1] != c[0]:
            raise ValueError(f"{who}: z_hat must be [B, {c[0]}, h, w] (got {tuple(z_hat.shape)})")
        if self.w0.device != z_hat.device:
            raise ValueError(f"{who}: the net is on {self.w0.device}, z_hat on {z_hat.device}")
        st = self._state()
        wp = self._packed(z_hat.device)
        x = int_quantize(z_hat, st["f0"])
        for i in range(3):
            x = int_conv(x, wp[i], getattr(self, f"bias{i}"), getattr(self, f"mult_pos{i}"), getattr(self, f"mult_neg{i}"),
                         getattr(self, f"shift{i}"), c[i + 1], transposed=i < 2, f32_out=i == 2, f_out=st["f_out"])
        out = x.permute(0, 3, 1, 2)
        return tuple(out.chunk(2, 1)) if self.split else (out, None)


def refuse_integer_hyper(who, kwargs):
    """the model families without an integer parameter net refuse its arguments by name (in the manner of vbr.refuse_rate_levels)"""
    for name in ("integer_hyper", "exact"):
        if name in kwargs and kwargs[name] not in (None, False):
            raise ValueError(f"{who} has no integer hyper-synthesis net: {name} is built for ScaleHyperprior and MeanScaleHyperprior only, "
                             f"whose entropy parameters depend on z alone (got {name}={kwargs[name]!r})")
