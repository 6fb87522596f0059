"""Integer hyper-synthesis: the entropy parameters of a hyperprior model in integer arithmetic, so that a stream is not tied
to the build that wrote it.  Balle, Johnston, Minnen, "Integer networks for data compression with latent-variable models" (ICLR 2019),
as a post-training conversion of the float ``h_s``; the kernels are csrc/int_conv.hip (int8 on the i8 matrix cores, requantising
epilogue fused), the arithmetic is stated in include/clc_hip.h.

Integer sums are exact and do not depend on summation order: the scales and means this net hands to the quantise / index / step kernels
are the same f32 bits under every kernel state (``set_precision``, ``CLC_TUNING``), every build and every machine — a CPU included.

The integer context model is the same arithmetic for mbt2018-checkerboard, whose parameters also read the coded y:
IntegerContextParameters holds the context layer and entropy_parameters, csrc/int_rows.hip (clc_int_rows) is their pixel-list int8
GEMM with a tap gather, and IntegerHyperSynthesis(int8_out=True) hands them h_s's output as an int8 map.
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


def layers_crc(host, n, h):
    """zlib.crc32 continued from h over the per-layer bytes of n layers of a host copy: w (int8, C order of its canonical layout), bias,
    mult_pos, mult_neg, shift (little-endian int32 each)"""
    for i in range(n):
        h = zlib.crc32(np.ascontiguousarray(host[f"w{i}"], dtype=np.int8).tobytes(), h)
        for k in _FIELDS[1:]:
            h = zlib.crc32(np.ascontiguousarray(host[f"{k}{i}"]).astype("<i4").tobytes(), h)
    return h


def layers_ready(host, n):
    """every shift in 1 .. 62, multipliers non-negative, |bias| <= 2^30, weights >= -127"""
    return all(((host[f"shift{i}"] >= 1) & (host[f"shift{i}"] <= 62)).all() and (host[f"mult_pos{i}"] >= 0).all()
               and (host[f"mult_neg{i}"] >= 0).all() and (np.abs(host[f"bias{i}"].astype(np.int64)) <= BIAS_MAX).all()
               and (host[f"w{i}"] >= -127).all() for i in range(n))


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


def amax_scale(amax):
    """the output scale of an int8 layer whose largest |activation| over the calibration inputs is amax"""
    return max(float(amax), W_FLOOR) / 127.0


def convert_layers(specs, s_in):
    """THE CONVERSION, float64 on the host and deterministic, of a chain of layers.  specs: per layer (w, b, co_axis, slope, s_out,
    s_in or None) — the float weight in any layout whose axis co_axis is the output channel, the bias, the negative-side slope of the
    layer's activation (0 ReLU, 0.01 LeakyReLU, 1 none), the scale of its output, and the scale of its input where that is not the
    previous layer's output.  Per output channel s_w = max|w| / 127, w_q = clamp(rint(w / s_w), +-127),
    bias_q = clamp(rint(b / (s_in s_w)), +-2^30), and the real factor s_in s_w / s_out as (mult_pos, mult_neg, shift).
    -> per layer a dict of numpy arrays (w int8 in the layout given, the rest int32)."""
    layers = []
    for w, b, co_axis, slope, s_out, s_own in specs:
        if s_own is not None:
            s_in = s_own
        w = np.asarray(w, dtype=np.float64)
        b = np.asarray(b, dtype=np.float64)
        wmax = np.abs(w).max(axis=tuple(a for a in range(w.ndim) if a != co_axis))
        s_w = np.maximum(wmax, W_FLOOR) / 127.0
        shape = [1] * w.ndim
        shape[co_axis] = -1
        w_q = np.clip(np.rint(w / s_w.reshape(shape)), -127, 127).astype(np.int8)
        bias_q = np.clip(np.rint(b / (s_in * s_w)), -BIAS_MAX, BIAS_MAX).astype(np.int32)
        mp, mn, sh = (np.empty(len(s_w), dtype=np.int32) for _ in range(3))
        for c in range(len(s_w)):
            mp[c], mn[c], sh[c] = multiplier(s_in * s_w[c] / s_out, float(slope))
        layers.append({"w": w_q, "bias": bias_q, "mult_pos": mp, "mult_neg": mn, "shift": sh})
        s_in = s_out
    return layers


def convert(weights, biases, amax, slopes, f0, f_out=8, s_last=None):
    """convert_layers for the three layers of h_s in torch's layouts (layers 1, 2 ConvTranspose2d [Cin, Cout, 5, 5]; layer 3 Conv2d
    [Cout, Cin, 3, 3]); amax[i]: the largest |activation| after layer i's activation over the calibration inputs (i = 0, 1); the last
    layer's output step is 2^-f_out, or s_last where its output is int8 (the context models' psi)."""
    s_outs = [amax_scale(amax[0]), amax_scale(amax[1]), 2.0 ** -int(f_out) if s_last is None else float(s_last)]
    return convert_layers([(weights[i], biases[i], 1 if i < 2 else 0, slopes[i], s_outs[i], None) for i in range(3)], 2.0 ** -int(f0))


def choose_f_y(y_absmax):
    """the largest f_y <= 4 with max|y_hat| * 2^f_y <= 127, floor 0 (beyond that both ends saturate alike)"""
    return choose_f0(y_absmax)


def ckbd_live_taps(w):
    """the checkerboard context filter [2M, M, 5, 5] -> its canonical layout [2M][12][M]: the 12 live taps in the order of ops.CKBD_TAPS"""
    w = np.asarray(w)
    return np.ascontiguousarray(np.stack([w[:, :, kh, kw] for kh, kw in ops.CKBD_TAPS], axis=1))


def convert_context_model(hs, ctx, ep, amax, z_absmax, y_absmax, hs_slopes=(0.01, 0.01, 1.0), f_out=8):
    """THE CONVERSION of the checkerboard model's whole entropy model.  hs: [(w, b)] of h_s's three layers; ctx: (w, b) of
    the context layer, [2M, M, 5, 5]; ep: [(w [Cout, Cin], b)] of entropy_parameters; amax: the calibration's largest |activation| as
    a dict — "hs1", "hs2" (after h_s's first two activations), "psi" and "ctx" (h_s's output and the context layer's at non-anchors:
    they share ONE scale, max(psi, ctx, 2^-16) / 127, so that entropy_parameters' first layer has one s_in), "ep1", "ep2".
    -> (h_s layers, context-net layers (context, ep1, ep2, ep3), f0, f_y, f_out)."""
    f0, f_y = choose_f0(z_absmax), choose_f_y(y_absmax)
    s_psi = amax_scale(max(float(amax["psi"]), float(amax["ctx"])))
    hs_layers = convert([w for w, _ in hs], [b for _, b in hs], [amax["hs1"], amax["hs2"]], hs_slopes, f0, f_out, s_last=s_psi)
    specs = [(ckbd_live_taps(ctx[0]), ctx[1], 0, 1.0, s_psi, 2.0 ** -f_y),
             (ep[0][0], ep[0][1], 0, 0.01, amax_scale(amax["ep1"]), s_psi),
             (ep[1][0], ep[1][1], 0, 0.01, amax_scale(amax["ep2"]), None),
             (ep[2][0], ep[2][1], 0, 1.0, 2.0 ** -int(f_out), None)]
    return hs_layers, convert_layers(specs, s_psi), f0, f_y, int(f_out)


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


def pack_rows(w_q):
    """THE PACKED FILTER of clc_int_rows (include/clc_hip.h): int8 [Cout, K] (K the concatenated ranges, a taps range tap-major) ->
    int8 [Cout / 32][K / 32][2][32][16], entry [ct][kc][h][r][j] = the weight of output channel 32 ct + r and k = 32 kc + 16 h + j"""
    w = np.asarray(w_q, dtype=np.int8)
    Cout, K = w.shape
    return np.ascontiguousarray(w.reshape(Cout // 32, 32, K // 32, 2, 16).transpose(0, 2, 3, 1, 4))


K_MAX = 65536   # clc_int_rows' largest total K: |acc| <= K * 128 * 127 <= 2^30, and with |bias| <= 2^30, |a| < 2^31
INT_KINDS = {"pixel": _lib.INT_SRC_PIXEL, "dense": _lib.INT_SRC_DENSE, "taps": _lib.INT_SRC_TAPS}


def int_rows(srcs, pix, B, H, W, w_packed, bias, mult_pos, mult_neg, shift, Cout, out, taps=None, f32_out=False, f_out=0):
    """clc_int_rows: out[r, :Cout] = requant(sum_k in(r, k) w[co, k]) for the rows r = b * P + p of the pixel list (int32 [P, 2] on
    the device) — ops.ar_linear's contract in int8.  srcs: one or two (kind, tensor) ranges of the K axis: ("pixel", map) and
    ("taps", map) take an int8 NHWC [B, H, W, C] map (a leading dimension above C from stride(2)), ("dense", buf) an int8 [>= rows, C]
    buffer (leading dimension stride(0)); taps: the (dh, dw) offsets of a taps range, at most 25.  out: int8 or (f32_out) f32
    [>= rows, >= Cout]."""
    if not 1 <= len(srcs) <= 2:
        raise ValueError(f"int_rows: one or two K ranges (got {len(srcs)})")
    pp, P = ops._ar_pix(pix)
    rows = B * P
    d = _lib.IntRowsDesc(nsrc=len(srcs), pix=pp, P=P, B=int(B), H=int(H), W=int(W), w_packed=w_packed.data_ptr(), bias=bias.data_ptr(),
                         mult_pos=mult_pos.data_ptr(), mult_neg=mult_neg.data_ptr(), shift=shift.data_ptr(), Cout=int(Cout),
                         out_kind=_lib.INT_OUT_F32 if f32_out else _lib.INT_OUT_I8, f_out=int(f_out))
    for i, (kind, t) in enumerate(srcs):
        if kind not in INT_KINDS:
            raise ValueError(f"int_rows: unknown source kind {kind!r} (pixel, dense or taps)")
        if not t.is_cuda or t.dtype != torch.int8 or t.stride(-1) != 1:
            raise ValueError(f"int_rows: range {i} must be an int8 device tensor with unit channel stride (got {t.dtype} {tuple(t.shape)} on {t.device})")
        if kind == "dense":
            if t.dim() != 2 or t.shape[0] < rows:
                raise ValueError(f"int_rows: a dense range needs an int8 [>= {rows} rows, C] buffer (got {tuple(t.shape)})")
            ld = t.stride(0)
        else:
            if t.dim() != 4 or tuple(t.shape[:3]) != (B, H, W):
                raise ValueError(f"int_rows: a {kind} range needs an int8 NHWC [B, H, W, C] = [{B}, {H}, {W}, C] map (got {tuple(t.shape)})")
            # (the stride of a dimension of size 1 says nothing)
            ld = t.stride(2) if W > 1 else (t.stride(1) if H > 1 else (t.stride(0) if B > 1 else t.shape[3]))
            if (H > 1 and t.stride(1) != W * ld) or (B > 1 and t.stride(0) != H * W * ld):
                raise ValueError(f"int_rows: a {kind} range must be dense in its pixels (shape {tuple(t.shape)} strides {t.stride()})")
        d.src[i] = _lib.IntSrc(t.data_ptr(), int(ld), int(t.shape[-1]), INT_KINDS[kind])
    if any(kind == "taps" for kind, _ in srcs):
        if taps is None or not 1 <= len(taps) <= _lib.INT_ROWS_MAX_TAPS:
            raise ValueError(f"int_rows: a taps range needs 1 .. {_lib.INT_ROWS_MAX_TAPS} (dh, dw) offsets (got {None if taps is None else len(taps)})")
        flat = [int(v) for off in taps for v in off]
        arr = (C.c_int * len(flat))(*flat)
        d.taps, d.ntaps = arr, len(taps)
    K = sum(int(t.shape[-1]) * (len(taps) if kind == "taps" else 1) for kind, t in srcs)
    if K > K_MAX:
        raise ValueError(f"int_rows: K = {K} is above {K_MAX}: the int32 sum could overflow (|acc| <= K * 128 * 127 must stay within 2^30)")
    if w_packed.dtype != torch.int8 or not w_packed.is_cuda or w_packed.numel() != Cout * K or not w_packed.is_contiguous():
        raise ValueError(f"int_rows: w_packed must be pack_rows' contiguous int8 image of a [{Cout}, K = {K}] filter on the device "
                         f"(got {w_packed.dtype} {tuple(w_packed.shape)})")
    for name, t in (("bias", bias), ("mult_pos", mult_pos), ("mult_neg", mult_neg), ("shift", shift)):
        if t.dtype != torch.int32 or not t.is_cuda or t.numel() != Cout or not t.is_contiguous():
            raise ValueError(f"int_rows: {name} must be a contiguous int32 [{Cout}] device tensor (got {t.dtype} {tuple(t.shape)})")
    dt = torch.float32 if f32_out else torch.int8
    if out.dtype != dt or out.dim() != 2 or not out.is_cuda or out.stride(1) != 1 or out.shape[0] < rows or out.shape[1] < Cout:
        raise ValueError(f"int_rows: out must be a row-major {dt} [>= {rows}, >= {Cout}] device buffer (got {out.dtype} {tuple(out.shape)})")
    d.y, d.ldy = out.data_ptr(), int(out.stride(0))
    _lib.check(_lib.load().clc_int_rows(C.byref(d), ops._stream()), "clc_int_rows")
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

    def __init__(self, channels, split=False, int8_out=False):
        super().__init__()
        self.channels = c = check_channels(channels, type(self).__name__)
        self.split = bool(split)
        self.int8_out = bool(int8_out)   # the context models' psi: the last layer's output stays int8 at a calibrated scale
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
            hl = layers_crc(host, 3, 0)
            h = zlib.crc32(host["fixed_point"].astype("<i4").tobytes(), hl) & 0xFFFFFFFF
            f0, f_out = (int(v) for v in host["fixed_point"])
            ready = layers_ready(host, 3) and 0 <= f0 <= 16 and 0 <= f_out <= 30
            self._cache = c = {"key": key, "host": host, "hash": h, "layers_crc": hl, "ready": bool(ready), "f0": f0, "f_out": f_out, "packed": {}}
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
        layer's fixed-point output; four launches on the current stream.  int8_out: -> psi, the last layer's int8 NHWC [B, 4h, 4w, C3]"""
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
                         getattr(self, f"shift{i}"), c[i + 1], transposed=i < 2, f32_out=i == 2 and not self.int8_out, f_out=st["f_out"])
        if self.int8_out:
            return x
        out = x.permute(0, 3, 1, 2)
        return tuple(out.chunk(2, 1)) if self.split else (out, None)


CKBD_OFFSETS = tuple((kh - 2, kw - 2) for kh, kw in ops.CKBD_TAPS)   # the 12 live taps as (dh, dw) around the pixel


def check_context_channels(N, M, who):
    """the integer context net's widths N, M, 3M/2, 2M, 10M/3, 8M/3 must all be multiples of 32: M a multiple of 192, N of 32"""
    if int(M) < 192 or int(M) % 192 or int(N) < 32 or int(N) % 32:
        raise ValueError(f"{who}: integer_context needs M to be a multiple of 192 and N a multiple of 32, so that every width of the "
                         f"entropy model (N, M, 3M/2, 2M, 10M/3, 8M/3) is a multiple of 32, the i8 matrix-core tile; got N={N}, M={M}")


class IntegerContextParameters(nn.Module):
    """The int8 context layer and ``entropy_parameters`` of the checkerboard model on clc_int_rows.

    THE BUFFERS (canonical layouts, all in ``state_dict``; zero-filled until fill / load_state_dict): layer 0 is the context layer,
    ``w0`` int8 [2M][12][M] — its 12 live taps in the order of ops.CKBD_TAPS; layers 1 .. 3 are the 1x1 layers, ``w{i}`` int8
    [Cout][Cin] (layer 1's Cin = 4M: psi's 2M channels, then the context's); per layer ``bias{i}``, ``mult_pos{i}``, ``mult_neg{i}``,
    ``shift{i}`` int32 [Cout]; ``fixed_point`` int32 [2] = (f_y, f_out).  The packed filter images are kept per device and rebuilt when
    a buffer is replaced or rewritten, as IntegerHyperSynthesis keeps its own."""

    def __init__(self, M):
        super().__init__()
        self.M = M = int(M)
        check_context_channels(32, M, type(self).__name__)
        self.widths = ((2 * M, 12 * M), (M * 10 // 3, 4 * M), (M * 8 // 3, M * 10 // 3), (2 * M, M * 8 // 3))   # (Cout, K) per layer
        for i, (co, k) in enumerate(self.widths):
            self.register_buffer(f"w{i}", torch.zeros((co, 12, M) if i == 0 else (co, k), dtype=torch.int8))
            for f in _FIELDS[1:]:
                self.register_buffer(f"{f}{i}", torch.zeros(co, dtype=torch.int32))
        self.register_buffer("fixed_point", torch.zeros(2, dtype=torch.int32))
        self._cache = None

    def fill(self, layers, f_y, f_out):
        """convert_context_model()'s four layers and the two fixed-point positions into the buffers"""
        for i, layer in enumerate(layers):
            for k in _FIELDS:
                buf = getattr(self, f"{k}{i}")
                t = torch.from_numpy(np.ascontiguousarray(layer[k]))
                if t.shape != buf.shape or t.dtype != buf.dtype:
                    raise ValueError(f"{type(self).__name__}.fill: {k}{i} must be {buf.dtype} {tuple(buf.shape)} (got {t.dtype} {tuple(t.shape)})")
                buf.copy_(t)
        self.fixed_point.copy_(torch.tensor([int(f_y), int(f_out)], dtype=torch.int32))
        return self

    def _state(self):
        key = tuple((t, t._version) for t in self.buffers())
        c = self._cache
        if c is None or len(c["key"]) != len(key) or any(a[0] is not b[0] or a[1] != b[1] for a, b in zip(c["key"], key)):
            host = {name: t.detach().cpu().numpy() for name, t in self.named_buffers()}
            f_y, f_out = (int(v) for v in host["fixed_point"])
            ready = layers_ready(host, 4) and 0 <= f_y <= 16 and 0 <= f_out <= 30
            self._cache = c = {"key": key, "host": host, "ready": bool(ready), "f_y": f_y, "f_out": f_out, "packed": {}}
        return c

    @property
    def ready(self):
        return self._state()["ready"]

    @property
    def f_y(self):
        return self._state()["f_y"]

    def layers_crc(self, h):
        """zlib.crc32 continued from h over the four layers' bytes (layers_crc); kept with the host copy, since every exact call asks"""
        st = self._state()
        if st.get("crc_from") != h:
            st["crc_from"], st["crc"] = h, layers_crc(st["host"], 4, h)
        return st["crc"]

    def require_ready(self, who):
        if not self.ready:
            raise ValueError(f"{who}: the integer context net is not filled (its shifts are outside 1 .. 62): call "
                             "model.integerize(x_calib) or load a state_dict of an integerised model")

    def _packed(self, dev):
        """per device: the packed images of the context layer, layer 1 whole (non-anchor passes), layer 1's psi columns alone (anchor
        passes), layers 2 and 3"""
        st = self._state()
        if dev not in st["packed"]:
            host, M = st["host"], self.M
            mats = [host["w0"].reshape(2 * M, 12 * M), host["w1"], host["w1"][:, :2 * M], host["w2"], host["w3"]]
            st["packed"][dev] = [torch.from_numpy(pack_rows(np.ascontiguousarray(m))).to(dev) for m in mats]
        return st["packed"][dev]

    def workspace(self, rows, dev):
        M = self.M
        mk = lambda c, dt: torch.empty((rows, c), device=dev, dtype=dt)
        return {"ctx": mk(2 * M, torch.int8), "h1": mk(M * 10 // 3, torch.int8), "h2": mk(M * 8 // 3, torch.int8), "gp": mk(2 * M, torch.float32)}

    @torch.no_grad()
    def chain(self, px, B, H, W, psi_map, yq_map, ws):
        """(scales | means) of the listed pixels of every image -> ws["gp"] (f32 rows, r 2^-f_out).  psi_map: int8 NHWC [B, H, W, 2M];
        yq_map: int8 NHWC [B, H, W, M], the quantised y_hat — a non-anchor pass, four launches; None — an anchor pass, three: no
        context range at all."""
        self.require_ready(f"{type(self).__name__}.chain")
        st, M = self._state(), self.M
        wp = self._packed(psi_map.device)
        par = lambda i: (getattr(self, f"bias{i}"), getattr(self, f"mult_pos{i}"), getattr(self, f"mult_neg{i}"), getattr(self, f"shift{i}"))
        if yq_map is not None:
            int_rows([("taps", yq_map)], px, B, H, W, wp[0], *par(0), 2 * M, ws["ctx"], taps=CKBD_OFFSETS)
            int_rows([("pixel", psi_map), ("dense", ws["ctx"])], px, B, H, W, wp[1], *par(1), M * 10 // 3, ws["h1"])
        else:
            int_rows([("pixel", psi_map)], px, B, H, W, wp[2], *par(1), M * 10 // 3, ws["h1"])
        int_rows([("dense", ws["h1"])], px, B, H, W, wp[3], *par(2), M * 8 // 3, ws["h2"])
        int_rows([("dense", ws["h2"])], px, B, H, W, wp[4], *par(3), 2 * M, ws["gp"], f32_out=True, f_out=st["f_out"])
        return ws["gp"]


def context_spec_hash(h_s_int, ctx_int):
    """THE HASH of the checkerboard model's entropy model, one u32: zlib.crc32 over the per-layer bytes of the seven layers in order
    (h_s's three, the context layer, entropy_parameters' three), then (f0, f_y, f_out) as little-endian int32"""
    hs, cs = h_s_int._state(), ctx_int._state()
    h = ctx_int.layers_crc(hs["layers_crc"])
    return zlib.crc32(np.array([hs["f0"], cs["f_y"], cs["f_out"]], dtype="<i4").tobytes(), h) & 0xFFFFFFFF


def refuse_integer_context(who, kwargs):
    """mbt2018's serial context model refuses the integer context net by name: a follow-up"""
    if kwargs.get("integer_context") not in (None, False):
        raise ValueError(f"{who} has no integer context net: integer_context is built for JointCheckerboardHierarchicalPriors only; the "
                         f"serial context model is a follow-up (got integer_context={kwargs['integer_context']!r})")
    kwargs.pop("integer_context", None)


def refuse_integer_hyper(who, kwargs):
    """the model families without an integer parameter net refuse its arguments by name (in the manner of vbr.refuse_rate_levels)"""
    for name in ("integer_hyper", "exact"):
        if name in kwargs and kwargs[name] not in (None, False):
            raise ValueError(f"{who} has no integer hyper-synthesis net: {name} is built for ScaleHyperprior and MeanScaleHyperprior only, "
                             f"whose entropy parameters depend on z alone (got {name}={kwargs[name]!r})")
