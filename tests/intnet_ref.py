"""The specification of the integer hyper-synthesis net (include/clc_hip.h restates it) in plain numpy with int64 and float64:
Balle, Johnston, Minnen, "Integer networks for data compression with latent-variable models" (ICLR 2019), post-training.  The kernels
(csrc/int_conv.hip) and the Python layer (clc_amd/intnet.py) must agree with this file bit for bit.  It depends on nothing but numpy.

A NET is a dict: ``f0``, ``f_out`` (ints) and ``layers``, a list of three dicts with ``w`` int8 (layers 1, 2: torch's ConvTranspose2d
layout [Cin, Cout, 5, 5]; layer 3: Conv2d's [Cout, Cin, 3, 3]), ``bias``, ``mult_pos``, ``mult_neg``, ``shift`` int32 [Cout].
Activations are int8 NHWC.
"""
import zlib

import numpy as np

BIAS_MAX = 1 << 30
W_FLOOR = 2.0 ** -16      # floor of max|w| of an output channel and of a layer's amax: a dead channel does not divide by zero
F0_CAP = 4


# ---- the arithmetic ----
def quantize_input(z_hat, f0):
    """z_hat float32 [B, C, H, W] (symbol + median, one rounded add) -> x0 int8 NHWC [B, H, W, C]: clamp(rint(z * 2^f0), -128, 127),
    rint half to even; the multiply by a power of two is exact"""
    z = np.asarray(z_hat, dtype=np.float32) * np.float32(2.0 ** int(f0))
    return np.clip(np.rint(z), -128, 127).astype(np.int8).transpose(0, 2, 3, 1).copy()


def deconv5_acc(x, w):
    """The 5x5 / stride 2 / padding 2 / output_padding 1 transposed convolution by output parity classes -> int64 [B, 2H, 2W, Cout].
    out[oh, ow, co] = sum over (kh, kw, ci) with oh = 2 ih - 2 + kh, ow = 2 iw - 2 + kw of x[ih, iw, ci] * w[ci, co, kh, kw]: the
    rows of parity ph take kh = ph, ph + 2, (ph + 4), from input row i + 1 - a for kh = 2 a + ph."""
    x = np.asarray(x).astype(np.int64)
    w = np.asarray(w).astype(np.int64)
    B, H, W, Cin = x.shape
    Cout = w.shape[1]
    out = np.zeros((B, 2 * H, 2 * W, Cout), dtype=np.int64)
    xp = np.zeros((B, H + 2, W + 2, Cin), dtype=np.int64)   # one ring of zeros: the taps off the map
    xp[:, 1:H + 1, 1:W + 1] = x
    for ph in (0, 1):
        for pw in (0, 1):
            acc = np.zeros((B, H, W, Cout), dtype=np.int64)
            for a in range(3 - ph):
                for c in range(3 - pw):
                    # input (i + 1 - a, j + 1 - c) -> padded (i + 2 - a, j + 2 - c)
                    acc += xp[:, 2 - a:2 - a + H, 2 - c:2 - c + W] @ w[:, :, 2 * a + ph, 2 * c + pw]
            out[:, ph::2, pw::2] = acc
    return out


def conv3_acc(x, w):
    """The 3x3 / stride 1 / padding 1 convolution -> int64 [B, H, W, Cout]"""
    x = np.asarray(x).astype(np.int64)
    w = np.asarray(w).astype(np.int64)
    B, H, W, Cin = x.shape
    xp = np.zeros((B, H + 2, W + 2, Cin), dtype=np.int64)
    xp[:, 1:H + 1, 1:W + 1] = x
    acc = np.zeros((B, H, W, w.shape[0]), dtype=np.int64)
    for kh in range(3):
        for kw in range(3):
            acc += xp[:, kh:kh + H, kw:kw + W] @ w[:, :, kh, kw].T
    return acc


def requant(acc, bias, mult_pos, mult_neg, shift):
    """r = ((int64)a * m + (1 << (shift - 1))) >> shift with a = acc + bias, m = mult_pos where a >= 0 else mult_neg: arithmetic shift,
    round half up.  Unclamped int64; the last axis is the channel."""
    a = np.asarray(acc).astype(np.int64) + np.asarray(bias).astype(np.int64)
    assert np.all(np.abs(a) < (1 << 31)), "|acc + bias| must stay below 2^31"
    m = np.where(a >= 0, np.asarray(mult_pos).astype(np.int64), np.asarray(mult_neg).astype(np.int64))
    s = np.asarray(shift).astype(np.int64)
    assert np.all((s >= 1) & (s <= 62)) and np.all((m >= 0) & (m < (1 << 31)))
    return (a * m + (np.int64(1) << (s - 1))) >> s


def layer_acc(x, layer, transposed):
    return deconv5_acc(x, layer["w"]) if transposed else conv3_acc(x, layer["w"])


def layer_int8(x, layer, transposed):
    r = requant(layer_acc(x, layer, transposed), layer["bias"], layer["mult_pos"], layer["mult_neg"], layer["shift"])
    return np.clip(r, -128, 127).astype(np.int8)


def layer_f32(x, layer, transposed, f_out):
    r = requant(layer_acc(x, layer, transposed), layer["bias"], layer["mult_pos"], layer["mult_neg"], layer["shift"])
    return np.clip(r, -32768, 32767).astype(np.float32) * np.float32(2.0 ** -int(f_out))   # exact in f32


def forward(net, z_hat):
    """z_hat f32 [B, N, h, w] -> the last layer's f32 output as NCHW [B, Cout, 4h, 4w] (scales, or scales | means)"""
    x = quantize_input(z_hat, net["f0"])
    x = layer_int8(x, net["layers"][0], True)
    x = layer_int8(x, net["layers"][1], True)
    return layer_f32(x, net["layers"][2], False, net["f_out"]).transpose(0, 3, 1, 2)


def acc_bound(taps, cin):
    """the largest |acc| of a layer: every activation -128 against weights of +-127"""
    return taps * cin * 128 * 127


# ---- the conversion ----
def choose_f0(z_absmax):
    """the largest f0 <= F0_CAP with max|z| * 2^f0 <= 127"""
    f0 = F0_CAP
    while f0 > 0 and float(z_absmax) * 2.0 ** f0 > 127.0:
        f0 -= 1
    return f0


def multiplier(rho, slope):
    """the real factor rho > 0 -> (mult_pos in [2^30, 2^31), mult_neg = rint(rho * slope * 2^shift), shift)"""
    mant, e = np.frexp(np.float64(rho))          # rho = mant * 2^e, mant in [0.5, 1)
    mp = int(np.rint(np.ldexp(mant, 31)))
    if mp == 1 << 31:
        mp, e = 1 << 30, e + 1
    shift = 31 - int(e)
    if not 1 <= shift <= 62:
        raise ValueError(f"integer hyper-synthesis: the requantising factor {float(rho)!r} needs shift {shift}, outside 1 .. 62")
    mn = mp if slope == 1.0 else min(int(np.rint(np.ldexp(np.float64(rho) * np.float64(slope), shift))), (1 << 31) - 1)
    return mp, mn, shift


def convert(weights, biases, amax, slopes, f0, f_out=8):
    """weights / biases: the three float layers in torch's layouts; amax[i]: the largest |activation| after layer i's activation
    (i = 0, 1; the last layer's scale is 2^-f_out); slopes[i]: the negative-side slope of layer i's activation (0 ReLU, 0.01
    LeakyReLU, 1 none).  float64 on the host, deterministic -> a net."""
    layers = []
    s_in = 2.0 ** -int(f0)
    for i in range(3):
        w = np.asarray(weights[i], dtype=np.float64)
        b = np.asarray(biases[i], dtype=np.float64)
        co_axis = 1 if i < 2 else 0
        wmax = np.abs(w).max(axis=tuple(a for a in range(4) if a != co_axis))
        s_w = np.maximum(wmax, W_FLOOR) / 127.0                                   # [Cout]
        shape = [1, 1, 1, 1]
        shape[co_axis] = -1
        w_q = np.clip(np.rint(w / s_w.reshape(shape)), -127, 127).astype(np.int8)
        s_out = max(float(amax[i]), W_FLOOR) / 127.0 if i < 2 else 2.0 ** -int(f_out)
        bias_q = np.clip(np.rint(b / (s_in * s_w)), -BIAS_MAX, BIAS_MAX).astype(np.int32)
        mp = np.empty(len(s_w), dtype=np.int32)
        mn = np.empty(len(s_w), dtype=np.int32)
        sh = np.empty(len(s_w), dtype=np.int32)
        for c in range(len(s_w)):
            mp[c], mn[c], sh[c] = multiplier(s_in * s_w[c] / s_out, float(slopes[i]))
        layers.append({"w": w_q, "bias": bias_q, "mult_pos": mp, "mult_neg": mn, "shift": sh, "s_in": s_in, "s_w": s_w, "s_out": s_out})
        s_in = s_out
    return {"f0": int(f0), "f_out": int(f_out), "layers": layers}


def spec_hash(net):
    """zlib.crc32, as a u32, over the little-endian bytes of: per layer in order w (int8, C order of its torch layout), bias, mult_pos,
    mult_neg, shift (int32 each); then f0 and f_out as int32"""
    h = 0
    for layer in net["layers"]:
        h = zlib.crc32(np.ascontiguousarray(layer["w"], dtype=np.int8).tobytes(), h)
        for k in ("bias", "mult_pos", "mult_neg", "shift"):
            h = zlib.crc32(np.ascontiguousarray(layer[k]).astype("<i4").tobytes(), h)
    return zlib.crc32(np.array([net["f0"], net["f_out"]], dtype="<i4").tobytes(), h) & 0xFFFFFFFF


# ---- the scale index of the coder (coder_device.h: scale_index_linear), restated ----
def scale_indexes(scales, table, step=None):
    """n - 1 - #{k < n - 1: sg <= table[k]} with sg = max(scale, 0.11f) (/ step) in f32"""
    sg = np.maximum(np.asarray(scales, dtype=np.float32), np.float32(0.11))
    if step is not None:
        sg = (sg / np.asarray(step, dtype=np.float32).reshape(1, -1, 1, 1)).astype(np.float32)
    t = np.asarray(table, dtype=np.float32)
    return (len(t) - 1 - (sg[..., None] <= t[:-1]).sum(-1)).astype(np.int32)
