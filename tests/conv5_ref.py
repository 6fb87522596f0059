"""Float64 CPU references of the 5x5 layers (clc_amd.layers.Conv2d(.., 5, ..) / ConvTranspose2d): F.conv2d / F.conv_transpose2d and
autograd through them, plus the worst-case f32 error bound of each sum.

Bound of an f32 fma chain of K terms in ANY order against the exact sum: |got - exact| <= (K + 2) * 2^-24 * S, S = the same sum on
absolute values (the + 2 covers the bias add and the activation's multiply).  Every helper returns (reference, K, S) per quantity.
"""
import torch
import torch.nn.functional as F

EPS = 2.0 ** -24
ACT_NONE, ACT_LRELU, ACT_RELU = 0, 1, 2


def act64(v, act):
    if act == ACT_RELU:
        return F.relu(v)
    if act == ACT_LRELU:
        return F.leaky_relu(v, 0.01)
    return v


def operands(shape_x, shape_w, n_bias, shape_dy, seed, integer):
    """x, w, bias, dy as float32 CPU tensors: small integers (every sum exact in f32) or standard normals."""
    g = torch.Generator().manual_seed(seed)
    if integer:
        r = lambda s, k: torch.randint(-k, k + 1, s, generator=g).float()
        return r(shape_x, 3), r(shape_w, 2), r((n_bias,), 3), r(shape_dy, 3)
    r = lambda s: torch.randn(s, generator=g)
    return r(shape_x), r(shape_w), r((n_bias,)), r(shape_dy)


def live_taps(parity):
    """taps of one axis that reach an output coordinate of that parity in the stride-2 / pad-2 transposed convolution"""
    return [k for k in range(5) if (parity + 2 - k) % 2 == 0]


def tap_table():
    """{(py, px): number of live taps}: 9 / 6 / 6 / 4"""
    return {(py, px): len(live_taps(py)) * len(live_taps(px)) for py in (0, 1) for px in (0, 1)}


def tap_count_map(OH, OW, stride):
    """[OH, OW] number of filter taps that contribute to each pixel of a transposed convolution's output"""
    if stride == 1:
        return torch.full((OH, OW), 25.0, dtype=torch.float64)
    ty = torch.tensor([len(live_taps(y % 2)) for y in range(OH)], dtype=torch.float64)
    tx = torch.tensor([len(live_taps(x % 2)) for x in range(OW)], dtype=torch.float64)
    return ty[:, None] * tx[None, :]


def deconv_identity_gap(seed=0):
    """max |conv_transpose2d(x, w, 2, 2, 1) - d/dz <conv2d(z, w, 2, 2), x>| in float64 on a 2H x 2W input z: 0.0"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-3, 4, (2, 6, 3, 5), generator=g).double()
    w = torch.randint(-2, 3, (6, 4, 5, 5), generator=g).double()
    z = torch.zeros(2, 4, 6, 10, dtype=torch.float64, requires_grad=True)
    (F.conv2d(z, w, stride=2, padding=2) * x).sum().backward()
    return (F.conv_transpose2d(x, w, stride=2, padding=2, output_padding=1) - z.grad).abs().max().item()


def conv_case(x, w, b, dy, stride, act, grads=True):
    """Conv2d(5, stride, pad 2) + act.  Returns {name: (ref, K, S)} for y [, dx, dw, db]."""
    xd, wd, bd = x.double().requires_grad_(grads), w.double().requires_grad_(grads), b.double().requires_grad_(grads)
    pre = F.conv2d(xd, wd, bd, stride=stride, padding=2)
    y = act64(pre, act)
    Cin, Cout = w.shape[1], w.shape[0]
    out = {"y": (y.detach(), 25 * Cin, F.conv2d(x.double().abs(), w.double().abs(), b.double().abs(), stride=stride, padding=2))}
    if not grads:
        return out
    dyd = dy.double()
    y.backward(dyd)
    p = pre.detach().requires_grad_()
    act64(p, act).backward(dyd)
    dz = p.grad
    H, W = x.shape[2], x.shape[3]
    oph, opw = (H + 4 - 5) % stride, (W + 4 - 5) % stride
    Sx = F.conv_transpose2d(dz.abs(), w.double().abs(), stride=stride, padding=2, output_padding=(oph, opw))
    out["dx"] = (xd.grad, tap_count_map(H, W, stride) * Cout, Sx)
    zabs = x.double().abs().requires_grad_()
    wz = torch.zeros_like(wd, requires_grad=True)
    (F.conv2d(zabs.detach(), wz, stride=stride, padding=2) * dz.abs()).sum().backward()
    npix = dy.shape[0] * dy.shape[2] * dy.shape[3]
    out["dw"] = (wd.grad, npix, wz.grad)
    out["db"] = (bd.grad, npix, dz.abs().sum((0, 2, 3)))
    return out


def deconv_case(x, w, b, dy, act, grads=True):
    """ConvTranspose2d(5, 2, 2, 1) + act, w = [in, out, 5, 5].  Returns {name: (ref, K, S)}."""
    xd, wd, bd = x.double().requires_grad_(grads), w.double().requires_grad_(grads), b.double().requires_grad_(grads)
    pre = F.conv_transpose2d(xd, wd, bd, stride=2, padding=2, output_padding=1)
    y = act64(pre, act)
    cin, cout = w.shape[0], w.shape[1]
    OH, OW = pre.shape[2], pre.shape[3]
    Sy = F.conv_transpose2d(x.double().abs(), w.double().abs(), b.double().abs(), stride=2, padding=2, output_padding=1)
    out = {"y": (y.detach(), tap_count_map(OH, OW, 2) * cin, Sy)}
    if not grads:
        return out
    dyd = dy.double()
    y.backward(dyd)
    p = pre.detach().requires_grad_()
    act64(p, act).backward(dyd)
    dz = p.grad
    out["dx"] = (xd.grad, 25 * cout, F.conv2d(dz.abs(), w.double().abs(), stride=2, padding=2))
    wz = torch.zeros_like(wd, requires_grad=True)
    (F.conv_transpose2d(x.double().abs(), wz, stride=2, padding=2, output_padding=1) * dz.abs()).sum().backward()
    npix = x.shape[0] * x.shape[2] * x.shape[3]
    out["dw"] = (wd.grad, npix, wz.grad)
    out["db"] = (bd.grad, dy.shape[0] * OH * OW, dz.abs().sum((0, 2, 3)))
    return out


def chan_axis(name, transposed_weight=False):
    """axis of the 'channel' of a quantity for the project's relative-to-channel-maximum bars"""
    if name in ("y", "dx"):
        return 1
    if name == "dw":
        return 1 if transposed_weight else 0
    return 0


def check(name, got, ref, K, S, exact, transposed_weight=False):
    """exact: element-for-element equality.  Otherwise the derived bound and the project's bars (2e-5 forward, 1e-4 gradients,
    relative to the channel maximum).  Returns the worst ratio error / bound (for printing)."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert torch.isfinite(got).all(), name
    err = (got - ref).abs()
    if exact:
        assert err.max().item() == 0.0, f"{name}: {int((err > 0).sum())} of {err.numel()} elements differ, worst {err.max().item()}"
        return 0.0
    bound = (torch.as_tensor(K, dtype=torch.float64) + 2) * EPS * S
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    assert (err <= bound).all(), f"{name}: worst error / bound = {ratio:.3f}"
    ax = chan_axis(name, transposed_weight)
    dims = [d for d in range(ref.dim()) if d != ax] if ref.dim() > 1 else []
    cmax = ref.abs().amax(dims, keepdim=True) if dims else ref.abs().max()   # (a bias gradient: against the largest of the vector)
    bar = 2e-5 if name == "y" else 1e-4
    rel = (err / cmax.clamp_min(1e-30)).max().item()
    assert rel <= bar, f"{name}: {rel:.3e} of the channel maximum (bar {bar})"
    return ratio
