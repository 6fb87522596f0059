"""The 5x5 kernels (csrc/conv5.hip) through layers.Conv2d(.., 5, ..) / layers.ConvTranspose2d, forward and autograd backward, against
the float64 references of tests/conv5_ref.py.

Three criteria per shape:
  exact    integer operands (x, dy in [-3, 3], w in [-2, 2], integer bias; activation none / ReLU): every product and partial sum is
           an integer below 2^24 (worst case 6 * 25 * 68), so ANY summation order is exact in f32 and y, dx, dw, db must equal float64
           element for element — one dropped or misplaced term shows.
  bounded  standard-normal operands, none / ReLU / LeakyReLU: |got - ref64| <= (K + 2) 2^-24 S per element (K terms, S the same sum on
           absolute values: the worst case of an f32 fma chain in any order), and the project's bars (2e-5 forward, 1e-4 gradients of the
           channel maximum).
  bits     an image's result does not depend on the batch around it; two runs agree bit for bit, gradients included.
The shapes are the smallest that reach each way the kernel can go wrong (see SHAPES).
"""
import functools

import pytest
import torch

import conv5_ref as R

pytestmark = pytest.mark.gpu

CL = torch.channels_last

# (N, Cin, Cout, H, W, stride)
SHAPES = [
    (1, 4, 4, 1, 1, 1),        # only the centre tap is live
    (1, 4, 8, 2, 2, 2),        # map smaller than the filter, 1x1 output
    (3, 12, 20, 6, 10, 2),     # tile rows cross image borders; Cin below one K-chunk; Cout tail; non-square
    (2, 36, 72, 9, 7, 1),      # odd sizes; one K-chunk + 4; Cout = two tiles + 8
    (2, 68, 132, 16, 16, 2),   # more than two K-chunks per tap with a tail; Cout past a 128-wide tile; exactly 128 output pixels
]
# the stride-2 shapes as ConvTranspose2d(Cout, Cin) on the output-sized map (all four parity classes), and the 3-channel tail
DECONV_SHAPES = [(N, Cout, Cin, (H + 1) // 2, (W + 1) // 2) for (N, Cin, Cout, H, W, s) in SHAPES if s == 2] + [(2, 8, 3, 4, 6)]
MODES = [(True, R.ACT_NONE), (True, R.ACT_RELU), (False, R.ACT_NONE), (False, R.ACT_RELU), (False, R.ACT_LRELU)]


def _layers():
    from clc_amd import layers
    return layers


@functools.lru_cache(maxsize=None)
def _conv_ref(shape, integer, act, grads=True):
    N, Cin, Cout, H, W, s = shape
    OH, OW = (H - 1) // s + 1, (W - 1) // s + 1
    ops = R.operands((N, Cin, H, W), (Cout, Cin, 5, 5), Cout, (N, Cout, OH, OW), 1000 + 7 * Cin + H, integer)
    return ops, R.conv_case(*ops, s, act, grads=grads)


@functools.lru_cache(maxsize=None)
def _deconv_ref(shape, integer, act):
    N, cin, cout, H, W = shape
    ops = R.operands((N, cin, H, W), (cin, cout, 5, 5), cout, (N, cout, 2 * H, 2 * W), 2000 + 7 * cin + H, integer)
    return ops, R.deconv_case(*ops, act)


def _run(layer, x, dy, act, w, b, grads=True, x_view=None):
    dev = torch.device("cuda:0")
    layer = layer.to(dev)
    with torch.no_grad():
        layer.weight.copy_(w.to(dev))
        layer.bias.copy_(b.to(dev))
    if x_view is None:
        xg = x.to(dev).contiguous(memory_format=CL).requires_grad_(grads)
        xin = xg
    else:
        xg, xin = x_view(x.to(dev), grads)
    y = layer(xin, act=act)
    if not grads:
        return {"y": y}
    y.backward(dy.to(dev).contiguous(memory_format=CL))
    return {"y": y, "dx": xg.grad, "dw": layer.weight.grad, "db": layer.bias.grad}


def _compare(got, ref, exact, transposed_weight=False, label=""):
    for name, (r, K, S) in ref.items():
        ratio = R.check(name, got[name], r, K, S, exact, transposed_weight)
        print(f"{label} {name}: worst error / bound {ratio:.3f}")


@pytest.mark.parametrize("integer,act", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv5(shape, integer, act):
    N, Cin, Cout, H, W, s = shape
    (x, w, b, dy), ref = _conv_ref(shape, integer, act)
    got = _run(_layers().Conv2d(Cin, Cout, 5, stride=s), x, dy, act, w, b)
    _compare(got, ref, integer, label=f"conv {shape} act {act}")


@pytest.mark.parametrize("integer,act", MODES)
def test_conv5_odd_input_stride2_forward(integer, act):
    shape = (1, 8, 8, 7, 5, 2)
    (x, w, b, dy), ref = _conv_ref(shape, integer, act, False)
    with torch.no_grad():
        got = _run(_layers().Conv2d(8, 8, 5, stride=2), x, dy, act, w, b, grads=False)
    _compare(got, ref, integer, label=f"conv {shape} act {act}")


@pytest.mark.parametrize("integer,act", MODES)
@pytest.mark.parametrize("shape", DECONV_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_deconv5(shape, integer, act):
    N, cin, cout, H, W = shape
    (x, w, b, dy), ref = _deconv_ref(shape, integer, act)
    got = _run(_layers().ConvTranspose2d(cin, cout), x, dy, act, w, b)
    _compare(got, ref, integer, transposed_weight=True, label=f"deconv {shape} act {act}")


@pytest.mark.parametrize("integer,act", MODES)
def test_conv5_rgb_head(integer, act):
    """Conv2d(3, 12, 5, stride=2): patch rows + the 1x1 kernels; the image takes no gradient"""
    shape = (2, 3, 12, 8, 12, 2)
    (x, w, b, dy), ref = _conv_ref(shape, integer, act)
    dev = torch.device("cuda:0")
    layer = _layers().Conv2d(3, 12, 5, stride=2).to(dev)
    with torch.no_grad():
        layer.weight.copy_(w.to(dev))
        layer.bias.copy_(b.to(dev))
    y = layer(x.to(dev).contiguous(memory_format=CL), act=act)
    y.backward(dy.to(dev).contiguous(memory_format=CL))
    got = {"y": y, "dw": layer.weight.grad, "db": layer.bias.grad}
    _compare(got, {k: v for k, v in ref.items() if k != "dx"}, integer, label=f"rgb head act {act}")


@pytest.mark.parametrize("integer,act", MODES)
def test_conv5_leading_dimension(integer, act):
    """input = channels [4:40] of a 48-channel buffer, output into channels [8:80] of a 96-channel one"""
    shape = (2, 36, 72, 9, 7, 1)
    (x, w, b, dy), ref = _conv_ref(shape, integer, act)

    def view(xd, grads):
        buf = torch.full((2, 48, 9, 7), float("nan"), device=xd.device).contiguous(memory_format=CL)
        buf[:, 4:40] = xd
        leaf = buf[:, 4:40].detach().requires_grad_(grads)   # a strided view (ld = 48) as the autograd leaf
        assert leaf.stride(3) == 48
        return leaf, leaf

    got = _run(_layers().Conv2d(36, 72, 5), x, dy, act, w, b, x_view=view)
    _compare(got, ref, integer, label=f"ld act {act}")
    # ldy: the forward kernel writing a channel slice of a wider buffer leaves the rest alone
    from clc_amd import ops
    dev = torch.device("cuda:0")
    out = torch.full((2, 96, 9, 7), -7.0, device=dev).contiguous(memory_format=CL)
    wk = w.to(dev).contiguous(memory_format=CL)
    ops.conv_raw(x.to(dev).contiguous(memory_format=CL), wk, b.to(dev), ks=5, act=act, out=out[:, 8:80])
    R.check("y", out[:, 8:80], *ref["y"], integer)
    assert (out[:, :8] == -7.0).all() and (out[:, 80:] == -7.0).all()


def test_bits_batch_invariant_and_repeatable():
    L = _layers()
    dev = torch.device("cuda:0")
    shape = (3, 12, 20, 6, 10, 2)
    (x, w, b, dy), _ = _conv_ref(shape, False, R.ACT_LRELU)
    conv = L.Conv2d(12, 20, 5, stride=2)
    with torch.no_grad():
        full = _run(conv, x, dy, R.ACT_LRELU, w, b, grads=False)["y"]
        one = _run(conv, x[1:2], dy, R.ACT_LRELU, w, b, grads=False)["y"]
    assert torch.equal(full[1:2], one)
    dshape = (3, 20, 12, 3, 5)
    (dx_, dw_, db_, ddy), _ = _deconv_ref(dshape, False, R.ACT_LRELU)
    dec = L.ConvTranspose2d(20, 12)
    with torch.no_grad():
        full = _run(dec, dx_, ddy, R.ACT_LRELU, dw_, db_, grads=False)["y"]
        one = _run(dec, dx_[1:2], ddy, R.ACT_LRELU, dw_, db_, grads=False)["y"]
    assert torch.equal(full[1:2], one)
    for layer, ops_ in ((lambda: L.Conv2d(12, 20, 5, stride=2), (x, w, b, dy)), (lambda: L.ConvTranspose2d(20, 12), (dx_, dw_, db_, ddy))):
        a = _run(layer(), ops_[0], ops_[3], R.ACT_LRELU, ops_[1], ops_[2])
        c = _run(layer(), ops_[0], ops_[3], R.ACT_LRELU, ops_[1], ops_[2])
        for k in a:
            assert torch.equal(a[k], c[k]), k


def test_refused_fields_are_named():
    from clc_amd import lib, ops
    L = _layers()
    dev = torch.device("cuda:0")
    x = torch.randn(2, 8, 8, 8, device=dev).contiguous(memory_format=CL)
    w = torch.randn(8, 8, 5, 5, device=dev).contiguous(memory_format=CL)
    with torch.no_grad():
        with pytest.raises(lib.ClcError, match="shuffle"):
            ops.conv2d(x, w, shuffle=True)
        with pytest.raises(lib.ClcError, match="res"):
            ops.conv2d(x, w, res=torch.zeros_like(x))
        with pytest.raises(lib.ClcError, match="w2"):
            ops.conv2d(x, w, w2=w)
    with pytest.raises(ValueError, match="kernel_size"):
        L.Conv2d(8, 8, 7)
    with pytest.raises(ValueError, match="kernel_size"):
        L.ConvTranspose2d(8, 8, kernel_size=3, stride=1, padding=1, output_padding=0)
    with pytest.raises(ValueError, match="output_padding"):
        L.ConvTranspose2d(8, 8, kernel_size=5, stride=2, padding=2, output_padding=0)
