"""clc_int_rows (csrc/int_rows.hip) against tests/intctx_ref.py at the smallest shapes at which it can go wrong: row counts
around the 32-row tile and across image boundaries, maps on which every tap is off the map, edges and corners, every range kind, both
outputs with leading dimensions into sentinel-filled buffers.  Integer sums have no tolerance: every comparison is exact."""
import numpy as np
import pytest
import torch

import intctx_ref as X
import intnet_ref as R

pytestmark = pytest.mark.gpu

ROWS = [(1, 1), (1, 31), (1, 33), (1, 70), (3, 1), (3, 11), (2, 35)]   # (B, P): B P = 1, 31, 33, 70 at B = 1; 3, 33 at B = 3; 70 at B = 2
MAPS = [(1, 1), (1, 2), (2, 1), (3, 3), (5, 4)]
ALL25 = tuple((dh, dw) for dh in range(-2, 3) for dw in range(-2, 3))
COMBOS = {"pixel": ("pixel",), "pixel+dense": ("pixel", "dense"), "taps12": ("taps",), "taps25": ("taps",)}
PAD = 16   # the leading dimensions are above C / Cout by this much


def _params(rng, Cout, acc_mag, out_max):
    """per-channel requantising parameters that spread the outputs over (and a little beyond) the clamp range"""
    mp = rng.integers(1 << 30, 1 << 31, Cout).astype(np.int64)
    mn = (mp * rng.choice([0.0, 0.01, 0.5, 1.0], Cout)).astype(np.int64)
    # r ~ acc * mp * 2^-shift should reach ~1.5 out_max: shift = log2(acc_mag * 2^30.5 / (1.5 out_max))
    shift = np.clip(np.rint(np.log2(acc_mag * 2.0 ** 30.5 / (1.5 * out_max))) + rng.integers(-1, 2, Cout), 1, 62).astype(np.int64)
    bias = rng.integers(-acc_mag // 4, acc_mag // 4 + 1, Cout).astype(np.int64)
    return {"bias": bias.astype(np.int32), "mult_pos": mp.astype(np.int32), "mult_neg": mn.astype(np.int32), "shift": shift.astype(np.int32)}


def _launch(dev, srcs_np, kinds, pixels, B, H, W, w, layer, f32_out, f_out, taps):
    """one clc_int_rows launch on padded, sentinel-filled buffers -> (the whole output buffer, rows)"""
    from clc_amd import intnet as P

    rows, Cout = B * len(pixels), w.shape[0]
    srcs = []
    for kind, a in zip(kinds, srcs_np):
        buf = torch.full(a.shape[:-1] + (a.shape[-1] + PAD,), 77, dtype=torch.int8, device=dev)   # (a read past C would change the sums)
        buf[..., :a.shape[-1]] = torch.from_numpy(a).to(dev)
        srcs.append((kind, buf[..., :a.shape[-1]]))
    sentinel = 12345.0 if f32_out else 0x5A
    out = torch.full((rows + 3, Cout + PAD), sentinel, dtype=torch.float32 if f32_out else torch.int8, device=dev)
    t = lambda k: torch.from_numpy(layer[k]).to(dev)
    pix = torch.tensor(pixels, dtype=torch.int32, device=dev).reshape(-1, 2)
    P.int_rows(srcs, pix, B, H, W, torch.from_numpy(P.pack_rows(w)).to(dev), t("bias"), t("mult_pos"), t("mult_neg"), t("shift"), Cout, out,
               taps=taps, f32_out=f32_out, f_out=f_out)
    torch.cuda.synchronize()
    return out.cpu().numpy(), rows, sentinel


def _check(got, rows, sentinel, want, Cout):
    assert np.array_equal(got[:rows, :Cout], want.reshape(rows, Cout))
    assert (got[rows:] == sentinel).all() and (got[:, Cout:] == sentinel).all()   # rows beyond B P and columns beyond Cout: never written


@pytest.mark.parametrize("f32_out", [False, True], ids=["int8", "f32"])
@pytest.mark.parametrize("combo", list(COMBOS))
def test_rows_against_the_reference(dev, combo, f32_out):
    kinds = COMBOS[combo]
    taps = {"taps12": X.CKBD_OFFSETS, "taps25": ALL25}.get(combo)
    rng = np.random.default_rng(list(COMBOS).index(combo) * 2 + int(f32_out))
    n = 0
    for B, Pn in ROWS:
        for H, W in MAPS:
            for Cc, Cout in ((32, 32), (64, 96), (32, 96), (64, 32)):
                pixels = [(int(rng.integers(H)), int(rng.integers(W))) for _ in range(Pn)]
                if Pn >= H * W:   # every pixel of the map, corners and edges included, then repeats
                    pixels[:H * W] = [(h, w) for h in range(H) for w in range(W)]
                srcs_np, parts = [], []
                for kind in kinds:
                    if kind == "dense":
                        a = rng.integers(-128, 128, (B * Pn, Cc)).astype(np.int8)
                        parts.append(a.astype(np.int64).reshape(B, Pn, Cc))
                    else:
                        a = rng.integers(-128, 128, (B, H, W, Cc)).astype(np.int8)
                        parts.append(X.gather_taps(a, pixels, taps) if kind == "taps" else X.gather_pixels(a, pixels))
                    srcs_np.append(a)
                x = np.concatenate(parts, -1)
                K = x.shape[-1]
                w = rng.integers(-127, 128, (Cout, K)).astype(np.int8)
                layer = _params(rng, Cout, int(np.sqrt(K) * 74 * 74), 32767 if f32_out else 127)
                layer["w"] = w
                f_out = int(rng.integers(0, 13))
                want = X.rows_f32(x, layer, f_out) if f32_out else X.rows_int8(x, layer)
                got, rows, sentinel = _launch(dev, srcs_np, kinds, pixels, B, H, W, w, layer, f32_out, f_out, taps)
                _check(got, rows, sentinel, want, Cout)
                n += 1
                if combo == "taps12" and H == W == 1:   # every tap off the map: the requantised bias
                    zero = X.rows_f32(np.zeros_like(x), layer, f_out) if f32_out else X.rows_int8(np.zeros_like(x), layer)
                    assert np.array_equal(want, zero)
    assert n == len(ROWS) * len(MAPS) * 4


@pytest.mark.parametrize("f32_out", [False, True], ids=["int8", "f32"])
def test_clamps_extreme_shifts_and_ties(dev, f32_out):
    """operands at +-127 / -128 with multipliers that drive both clamps; shifts 1 and 62; exact ties of both signs (round half up)"""
    B, H, W, Cc, Cout = 1, 2, 2, 32, 32
    m = np.zeros((B, H, W, Cc), np.int8)
    m[0, 0, 0], m[0, 0, 1], m[0, 1, 0] = -128, 127, 0
    m[0, 1, 1] = np.where(np.arange(Cc) & 1, 127, -128)
    pixels = [(0, 0), (0, 1), (1, 0), (1, 1)]
    w = np.where(np.arange(Cout)[:, None] & 1, -127, 127).astype(np.int8) * np.ones((1, Cc), np.int8)
    big, one = (1 << 31) - 1, 1 << 30
    bias, mp, mn, sh = (np.zeros(Cout, np.int64) for _ in range(4))
    mp[:], mn[:], sh[:] = one, one, 31
    mp[0:8], mn[0:8], sh[0:8] = big, big, 1                      # shift 1: |a| * (2^31 - 1) / 2 — both clamps
    mp[8:16], mn[8:16], sh[8:16] = big, one, 62                  # shift 62: a m 2^-62, a handful of steps at most
    bias[8:12] = [1 << 30, -(1 << 30), (1 << 30) - 7, -(1 << 30) + 7]
    bias[16:24] = [1, -1, 3, -3, 5, -5, 7, -7]                   # row 2 (acc = 0): (a + 1) >> 1 — ties of both signs, half up
    sh[24:32] = 24                                               # a * 2^6: clamps from moderate sums, int8 and 16-bit alike
    layer = {"w": w, "bias": bias.astype(np.int32), "mult_pos": mp.astype(np.int32), "mult_neg": mn.astype(np.int32), "shift": sh.astype(np.int32)}
    x = X.gather_pixels(m, pixels)
    want = X.rows_f32(x, layer, 8) if f32_out else X.rows_int8(x, layer)
    got, rows, sentinel = _launch(dev, [m], ("pixel",), pixels, B, H, W, w, layer, f32_out, 8, None)
    _check(got, rows, sentinel, want, Cout)
    r = R.requant(X.rows_acc(x, w), layer["bias"], layer["mult_pos"], layer["mult_neg"], layer["shift"])
    lo, hi = (-32768, 32767) if f32_out else (-128, 127)
    assert (r < lo).any() and (r > hi).any() and r[0, 0, 0] < lo and r[0, 0, 1] > hi                # both clamps are driven
    assert r[0, 2, 16:24].tolist() == [1, 0, 2, -1, 3, -2, 4, -3]                                   # 0.5 -> 1, -0.5 -> 0, ...
    scale = 1.0 / 256 if f32_out else 1
    assert (got[2, 16:24] / scale).tolist() == [1, 0, 2, -1, 3, -2, 4, -3]
    assert got[0, 0] == lo * scale and got[0, 1] == hi * scale
    assert np.abs(r[0, :, 8:16]).max() == 1                                                         # shift 62: 0, and 1 from |a| just above 2^30


def test_wrapper_refusals(dev):
    from clc_amd import intnet as P
    from clc_amd import lib as L

    i8 = lambda *s: torch.zeros(s, dtype=torch.int8, device=dev)
    i32 = lambda n: torch.ones(n, dtype=torch.int32, device=dev)
    pix = torch.zeros((2, 2), dtype=torch.int32, device=dev)
    wp = i8(32 * 32)
    args = (wp, i32(32), i32(32), i32(32), i32(32), 32)
    with pytest.raises(ValueError, match="one or two K ranges"):
        P.int_rows([("pixel", i8(1, 1, 1, 32))] * 3, pix, 1, 1, 1, *args, i8(2, 32))
    with pytest.raises(ValueError, match="unknown source kind"):
        P.int_rows([("map", i8(1, 1, 1, 32))], pix, 1, 1, 1, *args, i8(2, 32))
    with pytest.raises(ValueError, match=r"\[1, 1, 1, C\]"):
        P.int_rows([("pixel", i8(1, 2, 1, 32))], pix, 1, 1, 1, *args, i8(2, 32))
    with pytest.raises(ValueError, match="offsets"):
        P.int_rows([("taps", i8(1, 1, 1, 32))], pix, 1, 1, 1, *args, i8(2, 32))
    with pytest.raises(ValueError, match="offsets"):
        P.int_rows([("taps", i8(1, 1, 1, 32))], pix, 1, 1, 1, *args, i8(2, 32), taps=[(0, 0)] * 26)
    with pytest.raises(ValueError, match="out must be"):
        P.int_rows([("pixel", i8(1, 1, 1, 32))], pix, 1, 1, 1, *args, i8(1, 32))
    with pytest.raises(ValueError, match="w_packed must be"):
        P.int_rows([("pixel", i8(1, 1, 1, 64))], pix, 1, 1, 1, *args, i8(2, 32))
    with pytest.raises(L.ClcError, match="multiple of 32"):   # the C ABI's own refusal, by name, before any launch
        P.int_rows([("pixel", i8(1, 1, 1, 48))], pix, 1, 1, 1, i8(32 * 48), *args[1:], i8(2, 32))
