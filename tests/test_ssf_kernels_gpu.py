"""The scale-space volume and the trilinear warp (csrc/scale_space.hip through clc_amd/scale_space.py) against the float64 plain-torch
restatement (tests/ssf_ref.py) evaluated on the same float32 inputs.

Shapes (N, H, W, L), the smallest at which each failure mode is reachable:
  (1, 4, 4, 1)    the map is smaller than the 11-tap blur: every tap of a row lands on an edge pixel or next to one
  (2, 8, 16, 3)   powers of two and D = 4: pixel-unit flows and slice coordinates are exact in f32 (the EXACT tests)
  (3, 16, 48, 5)  non-square, width not a power of two, coarsest level 1 x 3, batch of 3, more than one 256-thread block
  (1, 32, 32, 5)  pile-up: every pixel of the image is sent to one corner voxel

BOUNDS (u = 2^-24, S = the largest input magnitude, 1 here; K = 11 taps).
Volume forward.  One blur pass is a K-term fmaf chain with f32 taps: |error| <= (K + 2) u S.  Slice d >= 1 has gone through d blurs
(2 passes each), d - 1 pools (3 additions and a multiply: 4 u S) and d - 1 upsamplings (6 roundings: 6 u S); every operator is an
average, so earlier errors are not amplified: |error(d)| <= [2 d (K + 2) + 10 (d - 1)] u S = 170 u = 1.0e-5 at d = 5.  Slice 0 is exact.
Volume backward.  The adjoint chain has the same lengths, but an edge pixel's blur weight is itself a sum of up to K taps (K more
roundings per pass: 2 K + 2) and the adjoint upsampling sums 16 products (pool and upsampling together 20 roundings).  With a
non-negative dvolume no term cancels, so the relative error of a dx element is at most sum_d [2 d (2 K + 2) + 20 (d - 1)] u = 920 u =
5.5e-5 at L = 5, inside the project's 1e-4 of the channel maximum.
Warp forward.  ix = fmaf(flow, W / 2, w) carries one rounding, |d ix| <= u |ix| < u W for an unclamped coordinate (a clamped one is an
exact integer), likewise iy, iz; the output moves by at most the coordinate error times the largest neighbour difference (<= S) per
axis, plus 12 roundings of weights and sums: |error| <= (W + H + D + 12) u S = 82 u = 4.9e-6 at 16 x 48 x 6.
Warp backward.  Every gradient is a sum of at most a few tens of products with a handful of roundings each — relative error of order
30 u = 2e-6 of the sum of magnitudes — checked at the project's bar, 1e-4 of the channel maximum.  The coordinate gradient jumps where
an index crosses an integer, so the gradient cases keep the fraction of every unclamped ix, iy, iz in [1/8, 7/8] and every clamped
index at least 1/8 past the border; the test asserts this on the float64 side.
Pile-up.  n = 1024 terms in [0, 1) summed in sequence: |error| <= (n - 1) u sum = 6.1e-5 of the sum.
"""
import functools

import pytest
import torch

import ssf_ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
K = 11
SHAPES = [(1, 4, 4, 1), (2, 8, 16, 3), (3, 16, 48, 5), (1, 32, 32, 5)]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _ops():
    from clc_amd.scale_space import scale_space_volume, scale_space_warp

    return scale_space_volume, scale_space_warp


@functools.lru_cache(maxsize=None)
def _frame(shape):
    N, H, W, L = shape
    return torch.rand((N, 3, H, W), generator=torch.Generator().manual_seed(100 + H * W + L))


@functools.lru_cache(maxsize=None)
def _volume_ref(shape):
    """(float64 volume of the f32 frame, float64 dx for the f32 dvolume g, g): computed once, read by every test that needs it"""
    N, H, W, L = shape
    x = _frame(shape).double().requires_grad_()
    v = ssf_ref.volume(x, 1.5, L)
    g = torch.rand(v.shape, generator=torch.Generator().manual_seed(7))   # f32, non-negative
    v.backward(g.double())
    return v.detach(), x.grad.detach(), g


def _slice_bound(d):
    return (2 * d * (K + 2) + 10 * (d - 1)) * U if d else 0.0


def _adjoint_bound(d):
    return (2 * d * (2 * K + 2) + 20 * (d - 1)) * U if d else 0.0


@pytest.mark.parametrize("shape", SHAPES)
def test_volume_forward_bounded(dev, shape):
    volume, _ = _ops()
    N, H, W, L = shape
    x = _frame(shape)
    v = volume(x.to(dev), 1.5, L)
    assert tuple(v.shape) == (N, 3, L + 1, H, W)
    ref = _volume_ref(shape)[0]
    got = v.double().cpu()
    assert torch.equal(v[:, :, 0].cpu(), x)
    for d in range(1, L + 1):
        err = (got[:, :, d] - ref[:, :, d]).abs().max().item()
        print(f"volume {shape} slice {d}: err {err:.3e} bound {_slice_bound(d):.3e}")
        assert err <= _slice_bound(d) and err <= 2e-5, (d, err)


def _assert_grad(got, ref, name, bar=1e-4):
    """per channel (dim 1): max |got - ref| <= bar * max |ref|"""
    got, ref = got.double().cpu(), ref.double()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    for c in range(ref.shape[1]):
        top = ref[:, c].abs().max().item()
        err = (got[:, c] - ref[:, c]).abs().max().item()
        print(f"{name}[{c}]: err {err:.3e} of max {top:.3e}")
        assert top > 0 and err <= bar * top, (name, c, err, top)


@pytest.mark.parametrize("shape", SHAPES)
def test_volume_backward_bounded(dev, shape):
    volume, _ = _ops()
    N, H, W, L = shape
    _, dx_ref, g = _volume_ref(shape)
    x = _frame(shape).to(dev).requires_grad_()
    volume(x, 1.5, L).backward(g.to(dev))
    rel = ((x.grad.double().cpu() - dx_ref).abs() / dx_ref.abs()).max().item()
    print(f"volume backward {shape}: largest relative error {rel:.3e}")
    assert rel <= sum(_adjoint_bound(d) for d in range(L + 1)) and rel <= 1e-4
    _assert_grad(x.grad, dx_ref, "dx")


# ---- warp inputs ----
def _coords_case(N, H, W, D, seed):
    """flow, scale (f32) whose indices have fractions in [0.15, 0.85], with integer parts from 3 before the volume to 2 past it"""
    g = torch.Generator().manual_seed(seed)

    def axis(size):
        tgt = torch.randint(-3, size + 2, (N, H, W), generator=g).double()
        return tgt + 0.15 + 0.7 * torch.rand((N, H, W), generator=g, dtype=torch.float64)

    ix, iy, iz = axis(W), axis(H), axis(D)
    fx = (ix - torch.arange(W, dtype=torch.float64).view(1, 1, W)) * 2 / W
    fy = (iy - torch.arange(H, dtype=torch.float64).view(1, H, 1)) * 2 / H
    gz = (2 * iz + 1) / D - 1
    return torch.stack((fx, fy), 1).float(), gz.unsqueeze(1).float()


def _assert_away_from_integers(flow, scale, D):
    """the precondition of the gradient comparisons, on the float64 side"""
    N, _, H, W = flow.shape
    for i, size in zip(ssf_ref.pixel_indices(flow.double(), scale.double(), D), (W, H, D)):
        un = (i > 0) & (i < size - 1)
        fr = i - torch.floor(i)
        assert bool(((fr[un] >= 0.125) & (fr[un] <= 0.875)).all())
        assert bool(((i[~un] <= -0.125) | (i[~un] >= size - 1 + 0.125)).all())
        assert bool(un.any()) and bool((~un).any())


@functools.lru_cache(maxsize=None)
def _warp_case(shape):
    """f32 inputs and the float64 reference (output and the three gradients), computed once"""
    N, H, W, L = shape
    D = L + 1
    g = torch.Generator().manual_seed(31 + H)
    vol = torch.rand((N, 3, D, H, W), generator=g)
    flow, scale = _coords_case(N, H, W, D, 17 + W)
    dy = torch.rand((N, 3, H, W), generator=g) - 0.5
    _assert_away_from_integers(flow, scale, D)
    v64, f64, s64 = (t.double().requires_grad_() for t in (vol, flow, scale))
    y = ssf_ref.warp(v64, f64, s64)
    y.backward(dy.double())
    return vol, flow, scale, dy, y.detach(), v64.grad, f64.grad, s64.grad


@pytest.mark.parametrize("shape", SHAPES[:3])
def test_warp_forward_and_backward_bounded(dev, shape):
    _, warp = _ops()
    N, H, W, L = shape
    vol, flow, scale, dy, y_ref, dv_ref, df_ref, ds_ref = _warp_case(shape)
    v, f, s = (t.to(dev).requires_grad_() for t in (vol, flow, scale))
    y = warp(v, f, s)
    err = (y.double().cpu() - y_ref).abs().max().item()
    bound = (W + H + L + 1 + 12) * U
    print(f"warp forward {shape}: err {err:.3e} bound {bound:.3e}")
    assert err <= bound and err <= 2e-5
    y.backward(dy.to(dev))
    _assert_grad(f.grad, df_ref, "dflow")
    _assert_grad(s.grad, ds_ref, "dscale")
    _assert_grad(v.grad, dv_ref, "dvolume")
    # clamped coordinates take no gradient at all
    ix, iy, iz = ssf_ref.pixel_indices(flow.double(), scale.double(), L + 1)
    assert bool((f.grad[:, 0].cpu()[(ix <= 0) | (ix >= W - 1)] == 0).all()) and bool((f.grad[:, 1].cpu()[(iy <= 0) | (iy >= H - 1)] == 0).all())
    assert bool((s.grad[:, 0].cpu()[(iz <= 0) | (iz >= L)] == 0).all())


def _integer_case(N, H, W, D, seed):
    """integer voxel targets, up to 2 outside the volume on every side, and the flow / scale that address them exactly (H, W, D powers of two)"""
    g = torch.Generator().manual_seed(seed)
    tx = torch.randint(-2, W + 2, (N, H, W), generator=g)
    ty = torch.randint(-2, H + 2, (N, H, W), generator=g)
    tz = torch.randint(-1, D + 1, (N, H, W), generator=g)
    fx = (tx - torch.arange(W).view(1, 1, W)).float() * (2.0 / W)
    fy = (ty - torch.arange(H).view(1, H, 1)).float() * (2.0 / H)
    gz = (2 * tz + 1).float() / D - 1
    return (tx.clamp(0, W - 1), ty.clamp(0, H - 1), tz.clamp(0, D - 1)), torch.stack((fx, fy), 1), gz.unsqueeze(1)


def test_exact_addressing(dev):
    """integer-pixel flows and exact slice coordinates, targets outside the frame on every side included: the output IS the addressed
    voxel, and dvolume of a one-hot dy is one-hot there"""
    _, warp = _ops()
    N, H, W, L = SHAPES[1]
    D = L + 1
    (cx, cy, cz), flow, scale = _integer_case(N, H, W, D, 5)
    assert int(cx.min()) == 0 and int(cx.max()) == W - 1 and int(cy.min()) == 0 and int(cy.max()) == H - 1 and int(cz.min()) == 0 and int(cz.max()) == D - 1
    vol = torch.rand((N, 3, D, H, W), generator=torch.Generator().manual_seed(6))
    n = torch.arange(N).view(N, 1, 1).expand(N, H, W)
    want = vol[n, :, cz, cy, cx].permute(0, 3, 1, 2)   # [N, 3, H, W]
    v = vol.to(dev).requires_grad_()
    y = warp(v, flow.to(dev), scale.to(dev))
    assert torch.equal(y.cpu(), want)
    # also the integer-on-the-border coordinates of the zero flow: slice coordinates d = 0 .. D - 1 return the slices
    for d in range(D):
        gz = torch.full((N, 1, H, W), (2 * d + 1) / D - 1)
        assert torch.equal(warp(v, torch.zeros(N, 2, H, W, device=dev), gz.to(dev)).cpu(), vol[:, :, d])
    for (b, h, w, c) in [(0, 0, 0, 0), (1, H - 1, W - 1, 2), (0, 3, 5, 1), (1, 4, 9, 0), (0, 7, 0, 2), (1, 0, 15, 1)]:
        dy = torch.zeros((N, 3, H, W))
        dy[b, c, h, w] = 1.0
        (dv,) = torch.autograd.grad(y, v, dy.to(dev), retain_graph=True)
        hot = torch.zeros((N, 3, D, H, W))
        hot[b, c, cz[b, h, w], cy[b, h, w], cx[b, h, w]] = 1.0
        assert torch.equal(dv.cpu(), hot), (b, h, w, c)


def test_forward_on_integers_and_borders(dev):
    """forward only: coordinates exactly on integers and exactly on the border (first and last voxel of every axis), 32 x 32 x 6"""
    _, warp = _ops()
    N, H, W, L = SHAPES[3]
    D = L + 1
    vol = torch.rand((N, 3, D, H, W), generator=torch.Generator().manual_seed(8))
    g = torch.Generator().manual_seed(9)
    tx = torch.randint(0, W, (N, H, W), generator=g)
    ty = torch.randint(0, H, (N, H, W), generator=g)
    tx[:, :, 0], tx[:, :, 1], ty[:, 0], ty[:, 1] = 0, W - 1, H - 1, 0   # exactly on the border
    fx = (tx - torch.arange(W).view(1, 1, W)).float() * (2.0 / W)
    fy = (ty - torch.arange(H).view(1, H, 1)).float() * (2.0 / H)
    flow = torch.stack((fx, fy), 1)
    scale = torch.where(torch.rand((N, 1, H, W), generator=g) < 0.5, torch.tensor(-1.0 + 1.0 / D), torch.tensor(1.0 - 1.0 / D))   # iz = 0 or D - 1, to f32 rounding
    y = warp(vol.to(dev), flow.to(dev), scale.to(dev))
    ref = ssf_ref.warp(vol.double(), flow.double(), scale.double())
    err = (y.double().cpu() - ref).abs().max().item()
    print(f"warp forward on integers and borders: err {err:.3e}")
    assert err <= (W + H + D + 12) * U


def _chain(dev, x, flow, scale, dy, L):
    """volume -> warp forward and backward on the device -> (y, dx, dflow, dscale)"""
    volume, warp = _ops()
    x, f, s = (t.to(dev).requires_grad_() for t in (x, flow, scale))
    y = warp(volume(x, 1.5, L), f, s)
    y.backward(dy.to(dev))
    return y.detach(), x.grad, f.grad, s.grad


def test_bits_run_to_run_and_batch_invariance(dev):
    shape = SHAPES[2]
    N, H, W, L = shape
    _, flow, scale, dy = _warp_case(shape)[:4]
    x = _frame(shape)
    a = _chain(dev, x, flow, scale, dy, L)
    b = _chain(dev, x, flow, scale, dy, L)
    for name, p, q in zip(("y", "dx", "dflow", "dscale"), a, b):
        assert torch.equal(p, q), f"{name} differs between two runs"
    assert float(a[1].abs().max()) > 0
    for i in range(N):
        one = _chain(dev, x[i:i + 1], flow[i:i + 1], scale[i:i + 1], dy[i:i + 1], L)
        for name, p, q in zip(("y", "dx", "dflow", "dscale"), a, one):
            assert torch.equal(p[i:i + 1], q), f"{name}: image {i} alone differs from image {i} in the batch"
    # the chain's dx against float64 (the volume gradient arrives from the warp's sorted gather)
    x64, f64, s64 = (t.double().requires_grad_() for t in (x, flow, scale))
    ssf_ref.warp(ssf_ref.volume(x64, 1.5, L), f64, s64).backward(dy.double())
    _assert_grad(a[1], x64.grad, "dx through the chain")


@pytest.mark.parametrize("corner", ["first", "last"])
def test_pile_up_on_one_voxel(dev, corner):
    """every pixel of a 32 x 32 image lands on ONE corner voxel (border clamping): its dvolume is the sum of all 1024 dy, in pixel order"""
    _, warp = _ops()
    N, H, W, L = SHAPES[3]
    D = L + 1
    sgn = -1.0 if corner == "first" else 1.0
    flow = torch.full((N, 2, H, W), 4.0 * sgn)    # two volume widths away: clamped for every pixel
    scale = torch.full((N, 1, H, W), 3.0 * sgn)
    vol = torch.rand((N, 3, D, H, W), generator=torch.Generator().manual_seed(12))
    dy = torch.rand((N, 3, H, W), generator=torch.Generator().manual_seed(13))
    at = (0, 0, 0) if corner == "first" else (D - 1, H - 1, W - 1)
    runs = []
    for _ in range(2):
        v = vol.to(dev).requires_grad_()
        y = warp(v, flow.to(dev), scale.to(dev))
        assert torch.equal(y.cpu(), vol[:, :, at[0], at[1], at[2]].view(N, 3, 1, 1).expand(N, 3, H, W))
        y.backward(dy.to(dev))
        runs.append(v.grad.cpu())
    assert torch.equal(runs[0], runs[1])
    got = runs[0][0, :, at[0], at[1], at[2]].double()
    ref = dy.double().sum(dim=(0, 2, 3))
    n = H * W
    print(f"pile-up {corner}: {got.tolist()} vs {ref.tolist()}")
    assert bool(((got - ref).abs() <= (n - 1) * U * ref).all()) and bool(((got - ref).abs() <= 1e-4 * ref).all())
    rest = runs[0].clone()
    rest[0, :, at[0], at[1], at[2]] = 0
    assert float(rest.abs().max()) == 0.0
