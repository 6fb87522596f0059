"""The int8 convolution kernels of the integer hyper-synthesis net (csrc/int_conv.hip) against tests/intnet_ref.py: every output
must be torch.equal to the int64 reference, for both geometries (5x5 / stride-2 transposed, 3x3 / stride-1) and both output kinds
(int8; f32 fixed point).  Integer sums are exact, so there is no tolerance anywhere in this file.

Shapes: Cin, Cout in {32, 96} (one K chunk; three — not a power of two) on maps 1x1 (every tap but the centre off the map), 3x5 (odd, a
partial 32-pixel tile), 9x9 (several tiles and a remainder) at B = 1 and 5x4 at B = 2 (a tile that crosses the image boundary; there the
input also comes through a leading dimension above Cin); Cin = 480 -> 32 and 32 -> Cout = 640, the extremes the models use, on 2x2.
Data: asymmetric random int8 including -128 and 127; per-channel multipliers and shifts that differ across channels, with mult_neg
cycling through 0 (ReLU), a small value (LeakyReLU) and mult_pos (linear); one all-extreme input against all-+-127 weights (the largest
accumulator); accumulators on exact ties of both signs.  Outputs go through a leading dimension above Cout into a sentinel-filled
buffer with spare rows: sentinels and the rows past the end must survive.
"""
import numpy as np
import pytest
import torch

import intnet_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(ci, co, b, h, w) for ci in (32, 96) for co in (32, 96) for (b, h, w) in ((1, 1, 1), (1, 3, 5), (1, 9, 9), (2, 5, 4))]
SHAPES += [(480, 32, 1, 2, 2), (32, 640, 1, 2, 2)]
IDS = [f"{ci}to{co}-b{b}-{h}x{w}" for ci, co, b, h, w in SHAPES]
KINDS = [(True, False), (True, True), (False, False), (False, True)]   # (transposed, f32 output)
KIND_IDS = ["deconv-i8", "deconv-f32", "conv-i8", "conv-f32"]
PAD_COLS, SPARE_ROWS, F_OUT = 32, 8, 8
SENT_I8, SENT_F32 = 85, -777.25


def _weights(rng, ci, co, transposed, lo=-127, hi=127):
    return rng.integers(lo, hi + 1, (ci, co, 5, 5) if transposed else (co, ci, 3, 3)).astype(np.int8)


def _params(rng, acc, co, f32):
    """per-channel multipliers and shifts that differ across channels, sized so that most results land inside the output range and
    some are clamped"""
    p90 = max(float(np.percentile(np.abs(acc), 90)), 1.0)
    base = 31 + int(np.ceil(np.log2(p90 / (20000.0 if f32 else 100.0))))
    c = np.arange(co)
    shift = np.clip(base + (c % 3) - 1, 1, 62).astype(np.int32)
    mult_pos = rng.integers(1 << 30, 1 << 31, co).astype(np.int32)
    mult_neg = np.where(c % 3 == 0, 0, np.where(c % 3 == 1, mult_pos // 100, mult_pos)).astype(np.int32)
    bias = rng.integers(-int(p90), int(p90) + 1, co).astype(np.int32)
    return {"bias": bias, "mult_pos": mult_pos, "mult_neg": mult_neg, "shift": shift}


def _run(dev, x, layer, transposed, f32, ldx_extra=0):
    """the kernel through clc_amd.intnet.int_conv into a sentinel-filled buffer -> (result, whole buffer as [rows + spare, ld])"""
    from clc_amd import intnet as P

    B, H, W, ci = x.shape
    co = layer["w"].shape[1] if transposed else layer["w"].shape[0]
    OH, OW = (2 * H, 2 * W) if transposed else (H, W)
    rows, ld = B * OH * OW, co + PAD_COLS
    buf = torch.full((rows + SPARE_ROWS, ld), SENT_F32 if f32 else SENT_I8, dtype=torch.float32 if f32 else torch.int8, device=dev)
    out = buf[:rows].view(B, OH, OW, ld)[..., :co]
    xd = torch.zeros((B, H, W, ci + ldx_extra), dtype=torch.int8, device=dev)
    xd[..., :ci] = torch.from_numpy(x).to(dev)
    xd[..., ci:] = 77   # never read
    wp = torch.from_numpy(P.pack_filter(layer["w"], transposed)).to(dev)
    t = {k: torch.from_numpy(layer[k]).to(dev) for k in ("bias", "mult_pos", "mult_neg", "shift")}
    got = P.int_conv(xd[..., :ci], wp, t["bias"], t["mult_pos"], t["mult_neg"], t["shift"], co, transposed, out=out, f32_out=f32, f_out=F_OUT)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    return out.cpu(), buf.cpu()


def _expect(x, layer, transposed, f32):
    return torch.from_numpy(R.layer_f32(x, layer, transposed, F_OUT) if f32 else R.layer_int8(x, layer, transposed))


def _check(dev, x, layer, transposed, f32, ldx_extra=0):
    out, buf = _run(dev, x, layer, transposed, f32, ldx_extra)
    want = _expect(x, layer, transposed, f32)
    assert out.dtype == want.dtype and torch.equal(out, want), f"{int((out != want).sum())} of {want.numel()} elements differ"
    co, rows = want.shape[3], want.shape[0] * want.shape[1] * want.shape[2]
    sent = SENT_F32 if f32 else SENT_I8
    assert bool((buf[:rows, co:] == sent).all()), "columns beyond Cout were written"
    assert bool((buf[rows:] == sent).all()), "rows past the end were written"
    return out


@pytest.mark.parametrize("transposed,f32", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("ci,co,b,h,w", SHAPES, ids=IDS)
def test_random_data_equals_reference(dev, ci, co, b, h, w, transposed, f32):
    rng = np.random.default_rng(1000 * ci + co + 7 * h + w + (2 if transposed else 0) + (1 if f32 else 0))
    x = rng.integers(-128, 100, (b, h, w, ci)).astype(np.int8)   # asymmetric
    x.flat[0], x.flat[-1] = -128, 127
    x[:, :, :, 1] = rng.integers(-128, 128, (b, h, w)).astype(np.int8)
    wq = _weights(rng, ci, co, transposed)
    layer = {"w": wq}
    layer.update(_params(rng, R.layer_acc(x, layer, transposed), co, f32))
    out = _check(dev, x, layer, transposed, f32, ldx_extra=16 if b > 1 else 0)
    again, _ = _run(dev, x, layer, transposed, f32, ldx_extra=16 if b > 1 else 0)
    assert torch.equal(out, again), "a second run gave other bits"
    if b > 1:   # the same bits for an image alone as for that image inside the batch
        alone, _ = _run(dev, x[1:2], layer, transposed, f32)
        assert torch.equal(alone, out[1:2])


@pytest.mark.parametrize("transposed", [True, False], ids=["deconv", "conv"])
@pytest.mark.parametrize("ci,co,h,w", [(96, 32, 3, 5), (480, 32, 2, 2)], ids=["96to32-3x5", "480to32-2x2"])
def test_largest_accumulator(dev, ci, co, h, w, transposed):
    """every input -128 against weights of +127 (even channels) and -127 (odd): |acc| = live taps x Cin x 128 x 127; the f32 kind with a
    shift that keeps the result inside 16 bits, so the value itself is compared, and the int8 kind at its clamps"""
    x = np.full((1, h, w, ci), -128, dtype=np.int8)
    wq = np.full((ci, co, 5, 5) if transposed else (co, ci, 3, 3), 127, dtype=np.int8)
    if transposed:
        wq[:, 1::2] = -127
    else:
        wq[1::2] = -127
    layer = {"w": wq, "bias": np.zeros(co, np.int32), "mult_pos": np.full(co, (1 << 31) - 1, np.int32), "mult_neg": np.full(co, (1 << 31) - 1, np.int32),
             "shift": np.full(co, 31 + 12, np.int32)}
    acc = R.layer_acc(x, layer, transposed)
    taps = min(3, h) * min(3, w)   # the live taps of the best-placed pixel, in both geometries (a parity class has 3 x 3 at most)
    assert np.abs(acc).max() == taps * ci * 128 * 127 and np.abs(acc).max() <= R.acc_bound(25, 480)
    out = _check(dev, x, layer, transposed, True)
    assert float(out.abs().max()) * 2 ** F_OUT < 32767   # not clamped: the accumulator itself is checked
    _check(dev, x, layer, transposed, False)


@pytest.mark.parametrize("transposed", [True, False], ids=["deconv", "conv"])
def test_exact_ties(dev, transposed):
    """mult = 2^30 with shift 31 halves the accumulator: every odd a is an exact tie, of both signs, and must round half up;
    mult_neg = 2^29 quarters the negative side (a = 2 mod 4 ties)"""
    rng = np.random.default_rng(5)
    ci, co = 32, 32
    x = rng.integers(-2, 3, (1, 3, 5, ci)).astype(np.int8)
    wq = _weights(rng, ci, co, transposed, -3, 3)
    c = np.arange(co)
    layer = {"w": wq, "bias": (c % 5 - 2).astype(np.int32), "mult_pos": np.full(co, 1 << 30, np.int32),
             "mult_neg": np.where(c % 2 == 0, 1 << 30, 1 << 29).astype(np.int32), "shift": np.full(co, 31, np.int32)}
    a = R.layer_acc(x, layer, transposed) + layer["bias"]
    assert ((a % 2 != 0) & (a > 0)).sum() > 20 and ((a % 2 != 0) & (a < 0)).sum() > 20 and ((a % 4 == 2) & (a < 0))[..., 1::2].sum() > 5
    for f32 in (False, True):
        _check(dev, x, layer, transposed, f32)


def test_input_quantiser(dev):
    """clc_int_quantize: clamp(rint(z * 2^f0), -128, 127), half to even, at ties of both signs and both clamps"""
    from clc_amd import intnet as P

    rng = np.random.default_rng(9)
    z = (rng.standard_normal((2, 32, 3, 5)) * 6).astype(np.float32)
    z.flat[:8] = [0.125, -0.125, 0.375, -0.375, 100.0, -100.0, 15.875, -16.0]   # f0 = 2: ties at .5 / 1.5, the clamps, the edges
    for f0 in (0, 2, 4):
        got = P.int_quantize(torch.from_numpy(z).to(dev).contiguous(memory_format=torch.channels_last), f0).cpu()
        assert torch.equal(got, torch.from_numpy(R.quantize_input(z, f0)))


def test_c_abi_refuses_by_name(dev):
    from clc_amd import intnet as P
    from clc_amd.lib import ClcError

    x = torch.zeros((1, 2, 2, 48), dtype=torch.int8, device=dev)
    t = torch.zeros(64, dtype=torch.int32, device=dev)
    wp = torch.zeros(64 * 9 * 64, dtype=torch.int8, device=dev)
    with pytest.raises(ClcError, match="multiples of 32"):
        P.int_conv(x, wp, t, t, t, t, 32, False)
    with pytest.raises(ClcError, match="int8 NHWC"):
        P.int_conv(x.float(), wp, t, t, t, t, 32, False)
