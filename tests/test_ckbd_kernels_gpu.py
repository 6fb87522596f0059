"""The checkerboard context layer (layers.CheckerboardMaskedConv2d -> csrc/ckbd_context.hip), forward and autograd backward, against
float64: F.conv2d of the anchors-only input with the masked filter, the anchors of the result zeroed (anchors: (h + w) odd).

dy is random at EVERY pixel, anchors included: an anchor's dy reaching dx, dw or db fails the exact test.

  exact    integer operands (x, dy in [-3, 3], w in [-2, 2], integer bias): every product and partial sum is an integer below 2^24
           (worst case 6 * 12 * 68), so ANY summation order is exact in f32 and y, dx, dw, db must equal float64 element for element.
           Anchor outputs are exactly 0, non-anchor dx is exactly 0, masked-tap dw is exactly 0 (in every mode).
           With LeakyReLU the negative outputs are v * 0.01f: the reference multiplies by the float32 slope and rounds the (exact)
           float64 product to float32, which is what the kernel computes, so y is still held element for element; the gradients then
           carry the factor 0.01f on some terms, are no longer integers and have no order-independent exact value — they are held to
           the derived bound below instead (and to the exact structural zeros).
  bounded  standard-normal operands: |got - ref64| <= (K + 2) 2^-24 S per element (K terms, S the same sum on absolute values), and
           the project's bars (2e-5 forward, 1e-4 gradients of the channel maximum).
  bits     image 1 of the batch of 3 equals the same image run alone (forward and dx); two runs agree bit for bit, dw included; the
           output for a 5x7 map does not depend on the input's leading dimension (a channel slice of a wider buffer).
The shapes are the smallest that reach each way the kernel can go wrong (see SHAPES).
"""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

import ckbd_ref
import conv5_ref as R

pytestmark = pytest.mark.gpu

CL = torch.channels_last

# (B, Cin, Cout, H, W)
SHAPES = [
    (1, 4, 4, 1, 1),        # a lone non-anchor: all taps outside, output = bias
    (1, 4, 8, 2, 3),        # padding slots from odd W, anchors at the border
    (3, 12, 20, 5, 7),      # both sizes odd, Cin below one K-chunk, Cout tail, the batch for the bit test
    (2, 36, 72, 9, 6),      # one K-chunk + 4, Cout over one 64-tile
    (2, 68, 132, 16, 17),   # more than two chunks with a tail, Cout past 128, 144 slots per image: a 128-row tile crosses an image boundary
]
ACTS = [R.ACT_NONE, R.ACT_LRELU]
SLOPE32 = float(torch.tensor(0.01, dtype=torch.float32).double())


def _mask():
    m = torch.zeros(5, 5, dtype=torch.float64)
    for kh in range(5):
        for kw in range(5):
            if (kh + kw) % 2:
                m[kh, kw] = 1
    return m


def _act(v, act, slope):
    return torch.where(v > 0, v, v * slope) if act == R.ACT_LRELU else v


@functools.lru_cache(maxsize=None)
def _ref(shape, integer, act):
    """operands and {name: (ref, K, S)}; computed once per case and shared"""
    B, Cin, Cout, H, W = shape
    x, w, b, dy = R.operands((B, Cin, H, W), (Cout, Cin, 5, 5), Cout, (B, Cout, H, W), 3000 + 7 * Cin + H, integer)
    anchor, other = ckbd_ref.parity_maps(H, W, torch.float64)
    mask = _mask()
    slope = SLOPE32 if integer else 0.01
    xd, wd, bd = x.double().requires_grad_(), w.double().requires_grad_(), b.double().requires_grad_()
    pre = F.conv2d(xd * anchor, wd * mask, bd, padding=2)
    y = _act(pre, act, slope) * other
    if integer and act == R.ACT_LRELU:
        y_ref = y.detach().float().double()   # the exact product v * 0.01f, rounded to float32 as the kernel's multiply does
    else:
        y_ref = y.detach()
    out = {"y": (y_ref, 12 * Cin, F.conv2d(x.double().abs() * anchor, w.double().abs() * mask, b.double().abs(), padding=2) * other)}
    dyd = dy.double()
    y.backward(dyd)
    p = pre.detach().requires_grad_()
    (_act(p, act, slope) * other).backward(dyd)
    dz = p.grad
    assert float((dz * anchor).abs().max()) == 0.0
    out["dx"] = (xd.grad, 12 * Cout, F.conv_transpose2d(dz.abs(), w.double().abs() * mask, padding=2) * anchor)
    wz = torch.zeros_like(wd, requires_grad=True)
    (F.conv2d(x.double().abs() * anchor, wz * mask, padding=2) * dz.abs()).sum().backward()
    nterms = B * int(other.sum())
    out["dw"] = (wd.grad, nterms, wz.grad)
    out["db"] = (bd.grad, nterms, dz.abs().sum((0, 2, 3)))
    return (x, w, b, dy), out


def _run(shape, x, w, b, dy, act, grads=True, x_view=None):
    from clc_amd import layers

    B, Cin, Cout, H, W = shape
    dev = torch.device("cuda:0")
    layer = layers.CheckerboardMaskedConv2d(Cin, Cout).to(dev)
    with torch.no_grad():
        layer.weight.copy_(w.to(dev))
        layer.bias.copy_(b.to(dev))
    if x_view is None:
        xg = x.to(dev).contiguous(memory_format=CL).requires_grad_(grads)
    else:
        xg = x_view(x.to(dev)).requires_grad_(grads)
    y = layer(xg, act=act)
    if not grads:
        return {"y": y}
    y.backward(dy.to(dev).contiguous(memory_format=CL))
    return {"y": y, "dx": xg.grad, "dw": layer.weight.grad, "db": layer.bias.grad}


def _structural_zeros(shape, got):
    B, Cin, Cout, H, W = shape
    anchor, other = ckbd_ref.parity_maps(H, W)
    anchor, other = anchor.to(got["y"].device), other.to(got["y"].device)
    assert float((got["y"].detach() * anchor).abs().max()) == 0.0, "anchor outputs are exactly 0"
    assert float((got["dx"] * other).abs().max()) == 0.0, "non-anchor dx is exactly 0"
    dead = (1 - _mask()).float().to(got["dw"].device)
    assert float((got["dw"] * dead).abs().max()) == 0.0, "masked-tap dw is exactly 0"
    assert tuple(got["dw"].shape) == (Cout, Cin, 5, 5)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("integer", [True, False], ids=["exact", "bounded"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ckbd_layer(shape, integer, act):
    (x, w, b, dy), ref = _ref(shape, integer, act)
    got = _run(shape, x, w, b, dy, act)
    _structural_zeros(shape, got)
    for name, (r, K, S) in ref.items():
        exact = integer and (act == R.ACT_NONE or name == "y")
        ratio = R.check(name, got[name], r, K, S, exact)
        print(f"ckbd {shape} act {act} {name}: {'exact' if exact else f'worst error / bound {ratio:.3f}'}")
    if shape == SHAPES[0]:   # a lone non-anchor: the output is the (activated) bias
        want = _act(b.double(), act, SLOPE32 if integer else 0.01).float()
        assert torch.allclose(got["y"].detach().reshape(-1).cpu(), want, rtol=1e-6, atol=0) and (not integer or torch.equal(got["y"].detach().reshape(-1).cpu(), want))


def test_bits_batch_invariant_repeatable_and_leading_dimension():
    shape = (3, 12, 20, 5, 7)
    (x, w, b, dy), _ = _ref(shape, False, R.ACT_LRELU)
    full = _run(shape, x, w, b, dy, R.ACT_LRELU)
    one = _run((1,) + shape[1:], x[1:2], w, b, dy[1:2], R.ACT_LRELU)
    assert torch.equal(full["y"][1:2], one["y"]) and torch.equal(full["dx"][1:2], one["dx"])
    again = _run(shape, x, w, b, dy, R.ACT_LRELU)
    for k in full:
        assert torch.equal(full[k], again[k]), k

    # the same map read as channels [4:16] of a 24-channel buffer (ld = 24), and image 1 alone as a slice of it
    def view(xd):
        buf = torch.full((xd.shape[0], 24, 5, 7), float("nan"), device=xd.device).contiguous(memory_format=CL)
        buf[:, 4:16] = xd
        leaf = buf[:, 4:16].detach()
        assert leaf.stride(3) == 24
        return leaf

    wide = _run(shape, x, w, b, dy, R.ACT_LRELU, x_view=view)
    for k in full:
        assert torch.equal(full[k], wide[k]), k
    wide_one = _run((1,) + shape[1:], x[1:2], w, b, dy[1:2], R.ACT_LRELU, grads=False, x_view=view)
    assert torch.equal(full["y"][1:2], wide_one["y"])
    # dy through a channel slice of a wider gradient buffer: the same gradients
    from clc_amd import ops

    dev = torch.device("cuda:0")
    layer_w = w.to(dev).contiguous(memory_format=CL)
    dbuf = torch.full((3, 32, 5, 7), float("nan"), device=dev).contiguous(memory_format=CL)
    dbuf[:, 8:28] = dy.to(dev)
    xg = x.to(dev).contiguous(memory_format=CL)
    mask = _mask().float().to(dev)
    w12 = ops.ckbd_filter(layer_w * mask)
    dw_a = ops.ckbd_wgrad_raw(xg, dy.to(dev).contiguous(memory_format=CL), 20, 12)
    dw_b = ops.ckbd_wgrad_raw(xg, dbuf[:, 8:28], 20, 12)
    assert torch.equal(dw_a, dw_b)
    wt = ops.filter_transpose(w12, 20, 12, 12)
    dx_a = ops.ckbd_conv_raw(dy.to(dev).contiguous(memory_format=CL), wt, None, 12, transposed=True)
    dx_b = ops.ckbd_conv_raw(dbuf[:, 8:28], wt, None, 12, transposed=True)
    assert torch.equal(dx_a, dx_b)
    # accumulate: dw += is the single launch's value added once
    acc = dw_a.clone()
    ops.ckbd_wgrad_raw(xg, dbuf[:, 8:28], 20, 12, dw_out=acc)
    assert torch.equal(acc, dw_a + dw_a)


def test_refused_arguments_are_named():
    from clc_amd import lib, ops

    dev = torch.device("cuda:0")
    x = torch.randn(2, 8, 4, 6, device=dev).contiguous(memory_format=CL)
    w = torch.randn(8, 8, 5, 5, device=dev).contiguous(memory_format=CL)
    with torch.no_grad():
        with pytest.raises(lib.ClcError, match="Cin % 4"):
            ops.ckbd_conv(torch.randn(2, 6, 4, 6, device=dev).contiguous(memory_format=CL), torch.randn(8, 6, 5, 5, device=dev))
        with pytest.raises(lib.ClcError, match="does not match the filter"):
            ops.ckbd_conv(x, torch.randn(8, 4, 5, 5, device=dev))
        with pytest.raises(lib.ClcError, match="act must be"):
            ops.ckbd_conv(x, w, None, act=R.ACT_RELU)
        with pytest.raises(lib.ClcError, match="the GPU only"):
            ops.ckbd_conv(x.cpu(), w.cpu())
    L = lib.load()
    y = torch.empty(2, 8, 4, 6, device=dev).contiguous(memory_format=CL)
    w12 = ops.ckbd_filter(w)

    def desc(**kw):
        d = lib.CkbdDesc()
        d.x, d.B, d.H, d.W, d.Cin, d.ldx = x.data_ptr(), 2, 4, 6, 8, 8
        d.w, d.bias, d.y, d.Cout, d.ldy, d.transposed, d.act = w12.data_ptr(), None, y.data_ptr(), 8, 8, 0, 0
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def wdesc(**kw):
        d = lib.CkbdWgradDesc()
        d.x, d.B, d.H, d.W, d.Cin, d.ldx = x.data_ptr(), 2, 4, 6, 8, 8
        d.dy, d.Cout, d.lddy, d.dw, d.accumulate = y.data_ptr(), 8, 8, w12.data_ptr(), 0
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def refused(fn, d, pattern):
        assert fn(ctypes.byref(d), None) < 0
        msg = L.clc_last_error().decode()
        assert pattern in msg, msg

    for field in ("x", "w", "y"):
        refused(L.clc_ckbd_conv, desc(**{field: None}), "clc_ckbd_conv: null pointer")
    refused(L.clc_ckbd_conv, desc(x=x.data_ptr() + 4), "16-byte aligned")
    refused(L.clc_ckbd_conv, desc(w=w12.data_ptr() + 8), "16-byte aligned")
    refused(L.clc_ckbd_conv, desc(Cin=6), "Cin % 4 == 0")
    refused(L.clc_ckbd_conv, desc(ldx=10), "ldx % 4 == 0")
    refused(L.clc_ckbd_conv, desc(ldy=4), "ldy < Cout")
    refused(L.clc_ckbd_conv, desc(H=0), "bad dims")
    refused(L.clc_ckbd_conv, desc(act=R.ACT_RELU), "act must be none or LeakyReLU")
    refused(L.clc_ckbd_conv, desc(transposed=2), "transposed must be 0 or 1")
    refused(L.clc_ckbd_conv, desc(B=1 << 20, H=1 << 6, W=1 << 6), "below 2^31")
    for field in ("x", "dy", "dw"):
        refused(L.clc_ckbd_wgrad, wdesc(**{field: None}), "clc_ckbd_wgrad: null pointer")
    refused(L.clc_ckbd_wgrad, wdesc(x=x.data_ptr() + 4), "16-byte aligned")
    refused(L.clc_ckbd_wgrad, wdesc(Cin=6), "Cin % 4 == 0")
    refused(L.clc_ckbd_wgrad, wdesc(lddy=4), "lddy < Cout")
    refused(L.clc_ckbd_wgrad, wdesc(W=-1), "bad dims")
    # none of the refused calls launched anything: a good call still runs
    assert L.clc_ckbd_conv(ctypes.byref(desc()), None) == 0
    torch.cuda.synchronize()
