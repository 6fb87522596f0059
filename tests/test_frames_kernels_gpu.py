"""clc_yuv420_to_rgb, clc_rgb_to_yuv420 and clc_plane_sse (csrc/frame_io.hip through clc_amd/frames.py) against the float64
restatement (tests/frames_ref.py), at 8 and 10 bits and in both chroma modes.

SHAPES (N, H, W -> Hp, Wp).  The first four are the smallest at which each clamp and the row tail can go wrong; none of them is
16-byte aligned, so they run the block-by-block path.  The last two have W a multiple of 16 and run the wide path (16-byte luma
loads and RGB stores), the second with a padded frame whose last run and last rows are padding; every wide-path result is also
compared bit for bit with the same call through a 4-channel buffer (ld = 4), which takes the block-by-block path.

THE BOUND of yuv420_to_rgb is derived from the documented operation order (_to_rgb_bound), not observed; the worst observed error
is printed.  rgb_to_yuv420 must return the restatement's integers: its inputs are seeded so that every float64 pre-rounding value is
at least 1e-3 samples from a half-integer and every pre-clamp value at least 1e-3 inside [0, max] (after the RGB clamp no value lies
beyond it), asserted on the float64 side with no element excluded.  SEED SEARCH: see SEEDS.
"""
import numpy as np
import pytest
import torch

import frames_ref
from frames_ref import KB, KG, KR

pytestmark = pytest.mark.gpu

SHAPES = [(1, 2, 2, 2, 2),       # one chroma sample, every clamp active at once
          (2, 4, 6, 4, 6),
          (1, 6, 10, 8, 16),     # padded
          (3, 16, 34, 16, 34),   # a row tail that is not a multiple of the vector run
          (2, 8, 48, 8, 48),     # the wide path: 3 (6 at 10 bits) full runs per block row, edge clamps in the first and last
          (2, 6, 80, 8, 96)]     # the wide path inside a padded frame
BITS = [8, 10]
MODES = ["bilinear", "bicubic"]
MARGIN = 1e-3

# SEED SEARCH (CPU, the restatement alone: python tests/test_frames_kernels_gpu.py prints it).  Per (case, shape, bit depth) the seeds
# 0, 1, 2, ... are tried in order and the first whose margins (_margins) both clear 1e-3 is recorded; about 2e-3 of all values lie
# within 1e-3 of a half-integer, so a case of n values clears with probability exp(-2e-3 n): the 2448 values of (3, 16, 34) need
# some hundred seeds, the 6 values of (1, 2, 2) the first.  The search's result, with the two margins of the seed it stopped at:
SEEDS = {
    ("rgb", 0, 8): 0,       # tie 6.72e-02, edge 7.90e+01
    ("rgb", 0, 10): 0,      # tie 1.67e-02, edge 3.17e+02
    ("rgb", 1, 8): 0,       # tie 9.15e-03, edge 1.68e+01
    ("rgb", 1, 10): 0,      # tie 2.57e-03, edge 6.73e+01
    ("rgb", 2, 8): 0,       # tie 3.75e-03, edge 2.54e+01
    ("rgb", 2, 10): 0,      # tie 1.12e-02, edge 1.02e+02
    ("rgb", 3, 8): 390,     # tie 1.01e-03, edge 1.67e+01
    ("rgb", 3, 10): 62,     # tie 1.44e-03, edge 6.29e+01
    ("rgb", 4, 8): 7,       # tie 2.34e-03, edge 9.64e+00
    ("rgb", 4, 10): 2,      # tie 1.95e-03, edge 3.23e+01
    ("rgb", 5, 8): 5,       # tie 1.74e-03, edge 1.36e+01
    ("rgb", 5, 10): 6,      # tie 1.40e-03, edge 5.46e+01
    ("clamp", 3, 8): 227,   # tie 1.13e-03, edge 5.84e+00
    ("clamp", 3, 10): 13,   # tie 1.24e-03, edge 1.99e+01
    ("clamp", 4, 8): 16,    # tie 1.35e-03, edge 5.43e+00
    ("clamp", 4, 10): 2,    # tie 1.09e-03, edge 2.40e+01
}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _dtype(bits):
    return torch.uint8 if bits == 8 else torch.int16


def _plane(shape, bits, g, lo=0, hi=None):
    hi = 2 ** bits if hi is None else hi
    v = torch.randint(lo, hi, shape, generator=g, dtype=torch.int64).numpy()
    return torch.from_numpy(v.astype(np.uint8) if bits == 8 else v.astype(np.uint16).view(np.int16))


def _planes(N, H, W, bits, seed):
    g = torch.Generator().manual_seed(seed)
    return _plane((N, H, W), bits, g), _plane((N, H // 2, W // 2), bits, g), _plane((N, H // 2, W // 2), bits, g)


def _rgb(case, si, bits, seed=None):
    """the seeded f32 frame [N, 3, Hp, Wp] of a rgb_to_yuv420 case.  "rgb": uniform in [0.02, 0.98].  "clamp": uniform in
    [0.05, 0.95] with ONE channel of every pixel pushed outside, to -0.2 or 1.2 — RGB outside [0, 1] on both sides, and no pixel
    turned grey by the clamp (grey is the tie: neutral chroma is max / 2, a half-integer at every bit depth)."""
    N, H, W, Hp, Wp = SHAPES[si]
    g = torch.Generator().manual_seed(SEEDS[(case, si, bits)] if seed is None else seed)
    if case == "rgb":
        return torch.rand((N, 3, Hp, Wp), generator=g) * 0.96 + 0.02
    x = torch.rand((N, 3, Hp, Wp), generator=g) * 0.9 + 0.05
    which = torch.randint(0, 3, (N, 1, Hp, Wp), generator=g)
    push = torch.where(torch.rand((N, 1, Hp, Wp), generator=g) < 0.5, -0.2, 1.2)
    return torch.where(torch.arange(3).view(1, 3, 1, 1) == which, push, x)


def _margins(rgb, size, bits):
    """(closest distance of any pre-rounding value to a half-integer, smallest distance of any pre-clamp value to the inside of
    [0, max]; negative: a value lies outside or on the edge) in samples, every element counted"""
    v = torch.cat([t.reshape(-1) for t in frames_ref.rgb_to_yuv420_values(rgb, size, bits)])
    tie = ((v - torch.floor(v)) - 0.5).abs().min().item()
    edge = torch.minimum(v, (2 ** bits - 1) - v).min().item()
    return tie, edge


def _to_rgb_bound(mode):
    """|error| of one output value of clc_yuv420_to_rgb against exact arithmetic, from the operation order in include/clc_hip.h; u = 2^-24
    bounds the relative rounding of one f32 operation or constant.  Carried per stage: M, the largest magnitude; e, the error.
      sample * (1 / max):       M = 1, e = 2 u (the constant, the product)
      x2 along one axis:        weights exact, S = sum |w| (1; bicubic (27 + 225 + 67 + 9) / 256), T roundings (2; 4) of partial sums
                                of at most S M:  e <- S e + T u S M;  M <- S M; twice (rows, then along the row)
      c - 0.5:                  |c - 0.5| <= S^2 / 2 =: M3;  e3 = e + u M3
      r, b = fma(C, c - 0.5, y) with C <= 2 - 2 Kb:  |.| <= R = 1 + C M3;  e_rb = C e3 + u C M3 (the constant) + 2 u (y) + u R
      g = fma(-Kb, b, fma(-Kr, r, y)) * (1 / Kg):  partial sums t1 <= 1 + Kr R, t2 <= 1 + (Kr + Kb) R;
          e_g = (2 u + Kr e_rb + u Kr R + u t1 + Kb e_rb + u Kb R + u t2) / Kg + 2 u t2 / Kg (the constant 1 / Kg, the product)
    Second-order terms (u^2) and the float64 restatement's own error are below the 1e-12 added at the end."""
    u = 2.0 ** -24
    S, T = (1.0, 2) if mode == "bilinear" else (328.0 / 256.0, 4)
    M, e = 1.0, 2 * u
    for _ in range(2):
        e, M = S * e + T * u * S * M, S * M
    M3 = S * S / 2
    e3 = e + u * M3
    C = 2 - 2 * KB
    R = 1 + C * M3
    e_rb = C * e3 + u * C * M3 + 2 * u + u * R
    t1, t2 = 1 + KR * R, 1 + (KR + KB) * R
    e_g = (2 * u + KR * e_rb + u * KR * R + u * t1 + KB * e_rb + u * KB * R + u * t2) / KG + 2 * u * t2 / KG
    return max(e_rb, e_g) + 1e-12


def _dev_planes(planes, dev):
    return tuple(p.to(dev) for p in planes)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("si", range(len(SHAPES)))
def test_yuv420_to_rgb_against_float64(dev, si, bits, mode):
    from clc_amd import frames

    N, H, W, Hp, Wp = SHAPES[si]
    planes = _planes(N, H, W, bits, 100 + si)
    want = frames_ref.yuv420_to_rgb(*planes, bits, mode, size=(Hp, Wp))
    d = _dev_planes(planes, dev)
    got = frames.yuv420_to_rgb(*d, bit_depth=bits, mode=mode, size=(Hp, Wp))
    assert got.shape == (N, 3, Hp, Wp) and got.is_contiguous(memory_format=torch.channels_last)
    err, bound = (got.double().cpu() - want).abs().max().item(), _to_rgb_bound(mode)
    print(f"shape {SHAPES[si]} bits {bits} {mode}: worst |error| {err:.3e}, derived bound {bound:.3e}")
    assert err <= bound
    # the padded call equals the unpadded call followed by torch's replicate pad, bit for bit
    tight = frames.yuv420_to_rgb(*d, bit_depth=bits, mode=mode)
    assert torch.equal(got, torch.nn.functional.pad(tight, (0, Wp - W, 0, Hp - H), mode="replicate"))
    # the same bits through a 4-channel buffer (ld = 4: never the wide path), and for image i alone
    buf = torch.full((N, 4, Hp, Wp), -7.0, device=dev).contiguous(memory_format=torch.channels_last)
    frames.yuv420_to_rgb(*d, bit_depth=bits, mode=mode, size=(Hp, Wp), out=buf[:, :3])
    assert torch.equal(buf[:, :3], got) and bool((buf[:, 3] == -7.0).all())
    for i in range(N):
        alone = frames.yuv420_to_rgb(*(p[i:i + 1] for p in d), bit_depth=bits, mode=mode, size=(Hp, Wp))
        assert torch.equal(alone[0], got[i]), i


def _check_to_yuv(dev, case, si, bits):
    from clc_amd import frames

    N, H, W, Hp, Wp = SHAPES[si]
    rgb = _rgb(case, si, bits)
    tie, edge = _margins(rgb, (H, W), bits)
    print(f"{case} shape {SHAPES[si]} bits {bits}: closest value to a half-integer {tie:.3e}, to the edge of [0, max] {edge:.3e} samples")
    assert tie >= MARGIN and edge >= MARGIN, (tie, edge)
    want = [frames_ref.quantise(v, bits) for v in frames_ref.rgb_to_yuv420_values(rgb, (H, W), bits)]
    x = rgb.to(dev).contiguous(memory_format=torch.channels_last)
    got = frames.rgb_to_yuv420(x, (H, W), bit_depth=bits)
    for name, g, w in zip("YUV", got, want):
        assert g.dtype == _dtype(bits) and g.is_contiguous()
        assert torch.equal(frames_ref.samples(g.cpu()).to(torch.int64), w), name
    assert got[0].shape == (N, H, W) and got[1].shape == (N, H // 2, W // 2) and got[2].shape == (N, H // 2, W // 2)
    wide = torch.zeros((N, 4, Hp, Wp), device=dev).contiguous(memory_format=torch.channels_last)
    wide[:, :3] = x
    for g, s in zip(got, frames.rgb_to_yuv420(wide[:, :3], (H, W), bit_depth=bits)):   # ld = 4: the block-by-block path, same integers
        assert torch.equal(g, s)
    for i in range(N):
        for g, a in zip(got, frames.rgb_to_yuv420(x[i:i + 1], (H, W), bit_depth=bits)):
            assert torch.equal(a[0], g[i]), i
    return rgb


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("si", range(len(SHAPES)))
def test_rgb_to_yuv420_returns_the_restatements_integers(dev, si, bits):
    rgb = _check_to_yuv(dev, "rgb", si, bits)
    assert 0.0 < float(rgb.min()) and float(rgb.max()) < 1.0


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("si", [3, 4])
def test_rgb_to_yuv420_clamps_rgb(dev, si, bits):
    rgb = _check_to_yuv(dev, "clamp", si, bits)
    assert float(rgb.min()) < -0.1 and float(rgb.max()) > 1.1
    # without the clamp the integers would differ: the case holds the clamp
    N, H, W, Hp, Wp = SHAPES[si]
    mx = 2 ** bits - 1
    unclamped = frames_ref.rgb2ycbcr(rgb.double()[:, :, :H, :W])[:, 0] * mx
    assert not torch.equal(frames_ref.quantise(unclamped, bits), frames_ref.quantise(frames_ref.rgb_to_yuv420_values(rgb, (H, W), bits)[0], bits))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("si", [0, 3, 5])
def test_exact_round_trip(dev, si, bits, mode):
    """random Y and constant U, V with RGB strictly inside [0, 1] (asserted in float64): rgb_to_yuv420(yuv420_to_rgb(.)) returns the
    same integers — y is recovered to rounding error of an integer, the constant chroma likewise"""
    from clc_amd import frames

    N, H, W, Hp, Wp = SHAPES[si]
    mx = 2 ** bits - 1
    g = torch.Generator().manual_seed(7 + si)
    Y = _plane((N, H, W), bits, g, lo=int(0.3 * mx), hi=int(0.7 * mx))
    U = torch.full((N, H // 2, W // 2), int(0.47 * mx), dtype=torch.int64).to(_dtype(bits))
    V = torch.full((N, H // 2, W // 2), int(0.55 * mx), dtype=torch.int64).to(_dtype(bits))
    ref = frames_ref.yuv420_to_rgb(Y, U, V, bits, mode)
    assert 0.0 < ref.min().item() and ref.max().item() < 1.0
    d = _dev_planes((Y, U, V), dev)
    back = frames.rgb_to_yuv420(frames.yuv420_to_rgb(*d, bit_depth=bits, mode=mode, size=(Hp, Wp)), (H, W), bit_depth=bits)
    for name, a, b in zip("YUV", d, back):
        assert torch.equal(a, b), name


@pytest.mark.parametrize("bits,shape", [(8, (3, 37, 53)), (8, (2, 64, 96)), (10, (2, 30, 50)), (10, (2, 64, 96)), (16, (1, 520, 520)),
                                        (16, (3, 5, 7))])
def test_plane_sse_is_the_exact_integer_sum(dev, bits, shape):
    """odd shapes take the scalar loads, 16-byte multiples the wide ones; 520 x 520 has 67 partial sums per image: more than one
    round of the second stage's wave"""
    from clc_amd import frames

    g = torch.Generator().manual_seed(bits + shape[1])
    a, b = _plane(shape, bits, g), _plane(shape, bits, g)
    want = ((frames_ref.samples(a).numpy().astype(np.int64) - frames_ref.samples(b).numpy().astype(np.int64)) ** 2).reshape(shape[0], -1).sum(axis=1)
    da, db = a.to(dev), b.to(dev)
    got = frames.plane_sse(da, db, bit_depth=bits)
    assert got.dtype == torch.int64 and got.cpu().numpy().tolist() == want.tolist()
    assert torch.equal(frames.plane_sse(da, db, bit_depth=bits), got)   # two runs are identical
    for i in range(shape[0]):
        assert torch.equal(frames.plane_sse(da[i:i + 1], db[i:i + 1], bit_depth=bits)[0], got[i]), i


def test_plane_sse_all_extreme_at_16_bits(dev):
    from clc_amd import frames

    N, H, W = 2, 128, 160
    a = torch.zeros((N, H, W), dtype=torch.int16, device=dev)
    b = torch.full((N, H, W), -1, dtype=torch.int16, device=dev)   # the pattern 0xFFFF: 65535 everywhere
    want = int(np.int64(H * W) * np.int64(65535) ** 2)              # 8.8e13: beyond 2^32 and beyond float32's integers
    got = frames.plane_sse(a, b, bit_depth=16)
    assert got.cpu().tolist() == [want, want]
    assert torch.equal(frames.plane_sse(b, a, bit_depth=16), got) and torch.equal(frames.plane_sse(a, b, bit_depth=16), got)
    assert frames.plane_sse(a, a, bit_depth=16).cpu().tolist() == [0, 0]


if __name__ == "__main__":   # the seed search, on the CPU
    for case, si, bits in SEEDS:
        N, H, W, Hp, Wp = SHAPES[si]
        for seed in range(100000):
            tie, edge = _margins(_rgb(case, si, bits, seed), (H, W), bits)
            if tie >= MARGIN and edge >= MARGIN:
                print(f'("{case}", {si}, {bits}): {seed},   # tie {tie:.2e}, edge {edge:.2e}')
                break
