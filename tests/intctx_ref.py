"""The specification of the integer context model of mbt2018-checkerboard (include/clc_hip.h restates it) in plain numpy with
int64 and float64, on top of tests/intnet_ref.py's requantiser.  The kernel (csrc/int_rows.hip) and the Python layer (clc_amd/intnet.py)
must agree with this file bit for bit.  It depends on nothing but numpy.

A CONTEXT NET is a dict: ``f0``, ``f_y``, ``f_out`` (ints), ``hs`` — the three layers of h_s as tests/intnet_ref.py takes them, the last
one's output int8 — and ``ctx`` — four layers: the context layer, ``w`` int8 [2M][12][M] (its 12 live taps in the order of CKBD_TAPS),
and the three 1x1 layers of entropy_parameters, ``w`` int8 [Cout][Cin] (layer 1's Cin = 4M: psi's channels, then the context's); per
layer ``bias``, ``mult_pos``, ``mult_neg``, ``shift`` int32 [Cout].  Maps are int8 NHWC.
"""
import zlib

import numpy as np

import intnet_ref as R

CKBD_TAPS = tuple((kh, kw) for kh in range(5) for kw in range(5) if (kh + kw) & 1)   # the 12 live taps, (kh, kw) ascending
CKBD_OFFSETS = tuple((kh - 2, kw - 2) for kh, kw in CKBD_TAPS)
K_MAX = 65536
FY_CAP = 4


# ---- the arithmetic ----
def quantize_y(y_hat, f_y):
    """y_hat float32 [B, M, H, W] (symbol + mean, one rounded add; 0 where nothing is coded yet) -> yq int8 NHWC:
    clamp(rint(y * 2^f_y), -128, 127), half to even"""
    return R.quantize_input(y_hat, f_y)


def psi_map(net, z_hat):
    """h_s in int8: z_hat f32 [B, N, h, w] -> psi int8 NHWC [B, 4h, 4w, 2M]"""
    x = R.quantize_input(z_hat, net["f0"])
    x = R.layer_int8(x, net["hs"][0], True)
    x = R.layer_int8(x, net["hs"][1], True)
    return R.layer_int8(x, net["hs"][2], False)


def gather_taps(m, pixels, offsets=CKBD_OFFSETS):
    """m int8 NHWC [B, H, W, C]; pixels [(h, w)] -> int64 [B, P, T * C], tap-major: the map at (h + dh, w + dw), 0 off the map"""
    m = np.asarray(m).astype(np.int64)
    B, H, W, Cc = m.shape
    out = np.zeros((B, len(pixels), len(offsets), Cc), dtype=np.int64)
    for p, (h, w) in enumerate(pixels):
        for t, (dh, dw) in enumerate(offsets):
            ih, iw = h + dh, w + dw
            if 0 <= ih < H and 0 <= iw < W:
                out[:, p, t] = m[:, ih, iw]
    return out.reshape(B, len(pixels), -1)


def gather_pixels(m, pixels):
    """m int8 NHWC -> int64 [B, P, C] at the listed pixels"""
    m = np.asarray(m).astype(np.int64)
    return np.stack([m[:, h, w] for h, w in pixels], axis=1)


def rows_acc(x, w):
    """x int64 [..., K]; w int8 [Cout, K] (any trailing layout, flattened) -> int64 [..., Cout]"""
    w = np.asarray(w).astype(np.int64)
    w = w.reshape(w.shape[0], -1)
    assert x.shape[-1] == w.shape[1] <= K_MAX, "K above 65536 is refused: |acc| <= K * 128 * 127 must stay within 2^30"
    return x @ w.T


def rows_int8(x, layer, cols=None):
    w = np.asarray(layer["w"]).reshape(len(layer["bias"]), -1)
    r = R.requant(rows_acc(x, w if cols is None else w[:, :cols]), layer["bias"], layer["mult_pos"], layer["mult_neg"], layer["shift"])
    return np.clip(r, -128, 127).astype(np.int8)


def rows_f32(x, layer, f_out):
    r = R.requant(rows_acc(x, layer["w"]), layer["bias"], layer["mult_pos"], layer["mult_neg"], layer["shift"])
    return np.clip(r, -32768, 32767).astype(np.float32) * np.float32(2.0 ** -int(f_out))   # exact in f32


def is_anchor(pixels):
    """a pass is an anchor pass or a non-anchor pass by the parity of its pixels"""
    par = {(h + w) & 1 for h, w in pixels}
    assert len(par) == 1
    return bool(par.pop())


def chain(net, pixels, psi, yq):
    """the (scales | means) rows of one pass -> f32 [B, P, 2M] (and the int8 rows on the way).  An anchor pass (yq None) has no context
    range at all; a non-anchor pass always evaluates the context layer — on a 1x1 latent every tap is off the map and the context row
    is the requantised bias."""
    L = net["ctx"]
    x = gather_pixels(psi, pixels)
    out = {}
    if yq is not None:
        out["ctx"] = rows_int8(gather_taps(yq, pixels), L[0])
        x = np.concatenate((x, out["ctx"].astype(np.int64)), axis=-1)
        out["h1"] = rows_int8(x, L[1])
    else:
        out["h1"] = rows_int8(x, L[1], cols=x.shape[-1])
    out["h2"] = rows_int8(out["h1"].astype(np.int64), L[2])
    out["gp"] = rows_f32(out["h2"].astype(np.int64), L[3], net["f_out"])
    return out


def passes(H, W):
    """the non-empty passes of an H x W latent in stream order: the anchors ((h + w) odd) in raster order, then the non-anchors"""
    a = [(h, w) for h in range(H) for w in range(W) if (h + w) & 1]
    o = [(h, w) for h in range(H) for w in range(W) if not (h + w) & 1]
    return [p for p in (a, o) if p]


def acc_bound(K):
    """the largest |acc| of a layer of K products: every activation -128 against weights of +-127"""
    return K * 128 * 127


# ---- the conversion ----
def choose_f_y(y_absmax):
    """the largest f_y <= 4 with max|y_hat| * 2^f_y <= 127, floor 0"""
    f = FY_CAP
    while f > 0 and float(y_absmax) * 2.0 ** f > 127.0:
        f -= 1
    return f


def amax_scale(amax):
    return max(float(amax), R.W_FLOOR) / 127.0


def convert_layer(w, b, co_axis, slope, s_in, s_out):
    """one layer of tests/intnet_ref.py's conversion with its layout and scales given: per output channel s_w = max|w| / 127,
    w_q = clamp(rint(w / s_w), +-127), bias_q = clamp(rint(b / (s_in s_w)), +-2^30), the factor s_in s_w / s_out as a multiplier"""
    w = np.asarray(w, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    wmax = np.abs(w).max(axis=tuple(a for a in range(w.ndim) if a != co_axis))
    s_w = np.maximum(wmax, R.W_FLOOR) / 127.0
    shape = [1] * w.ndim
    shape[co_axis] = -1
    w_q = np.clip(np.rint(w / s_w.reshape(shape)), -127, 127).astype(np.int8)
    bias_q = np.clip(np.rint(b / (s_in * s_w)), -R.BIAS_MAX, R.BIAS_MAX).astype(np.int32)
    mp, mn, sh = (np.empty(len(s_w), dtype=np.int32) for _ in range(3))
    for c in range(len(s_w)):
        mp[c], mn[c], sh[c] = R.multiplier(s_in * s_w[c] / s_out, float(slope))
    return {"w": w_q, "bias": bias_q, "mult_pos": mp, "mult_neg": mn, "shift": sh, "s_in": s_in, "s_w": s_w, "s_out": s_out, "slope": float(slope)}


def live_taps(w):
    """[2M, M, 5, 5] -> [2M][12][M]"""
    w = np.asarray(w)
    return np.ascontiguousarray(np.stack([w[:, :, kh, kw] for kh, kw in CKBD_TAPS], axis=1))


def convert(hs, ctx, ep, amax, z_absmax, y_absmax, hs_slopes=(0.01, 0.01, 1.0), f_out=8):
    """hs: [(w, b)] of h_s in torch's layouts; ctx: (w [2M, M, 5, 5], b); ep: [(w [Cout, Cin], b)] x 3; amax: "hs1", "hs2", "psi",
    "ctx", "ep1", "ep2".  psi and the context rows share one scale: max(amax psi, amax ctx, 2^-16) / 127 -> a context net"""
    f0, f_y = R.choose_f0(z_absmax), choose_f_y(y_absmax)
    s_psi = amax_scale(max(float(amax["psi"]), float(amax["ctx"])))
    s1, s2 = amax_scale(amax["hs1"]), amax_scale(amax["hs2"])
    hs_l = [convert_layer(hs[0][0], hs[0][1], 1, hs_slopes[0], 2.0 ** -f0, s1),
            convert_layer(hs[1][0], hs[1][1], 1, hs_slopes[1], s1, s2),
            convert_layer(hs[2][0], hs[2][1], 0, hs_slopes[2], s2, s_psi)]
    e1, e2 = amax_scale(amax["ep1"]), amax_scale(amax["ep2"])
    ctx_l = [convert_layer(live_taps(ctx[0]), ctx[1], 0, 1.0, 2.0 ** -f_y, s_psi),
             convert_layer(ep[0][0], ep[0][1], 0, 0.01, s_psi, e1),
             convert_layer(ep[1][0], ep[1][1], 0, 0.01, e1, e2),
             convert_layer(ep[2][0], ep[2][1], 0, 1.0, e2, 2.0 ** -int(f_out))]
    return {"f0": f0, "f_y": f_y, "f_out": int(f_out), "hs": hs_l, "ctx": ctx_l}


def spec_hash(net):
    """zlib.crc32, as a u32, over the seven layers' bytes in order (h_s's three, the context layer, entropy_parameters' three; per layer
    w int8 in C order of its canonical layout, then bias, mult_pos, mult_neg, shift as little-endian int32), then (f0, f_y, f_out) as
    little-endian int32"""
    h = 0
    for layer in list(net["hs"]) + list(net["ctx"]):
        h = zlib.crc32(np.ascontiguousarray(layer["w"], dtype=np.int8).tobytes(), h)
        for k in ("bias", "mult_pos", "mult_neg", "shift"):
            h = zlib.crc32(np.ascontiguousarray(layer[k]).astype("<i4").tobytes(), h)
    return zlib.crc32(np.array([net["f0"], net["f_y"], net["f_out"]], dtype="<i4").tobytes(), h) & 0xFFFFFFFF


def net_of_state_dict(sd):
    """a context net from a model's state_dict alone (numpy arrays under "h_s_int." and "ctx_int.")"""
    get = lambda pre, k, i: np.asarray(sd[f"{pre}.{k}{i}"])
    lay = lambda pre, n: [{k: get(pre, k, i) for k in ("w", "bias", "mult_pos", "mult_neg", "shift")} for i in range(n)]
    fy, fo = (int(v) for v in np.asarray(sd["ctx_int.fixed_point"]))
    return {"f0": int(np.asarray(sd["h_s_int.fixed_point"])[0]), "f_y": fy, "f_out": fo, "hs": lay("h_s_int", 3), "ctx": lay("ctx_int", 4)}
