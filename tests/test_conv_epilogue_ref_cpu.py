"""The float64 reference of the convolution contract (tests/conv_epilogue_ref.py) against independent torch compositions: every activation and
derivative against torch's own functions / autograd, PixelShuffle against F.pixel_shuffle, the data-gradient GEMM against the autograd
gradient of F.conv2d, GDN / IGDN against the CompressAI formula and MUL2 against the autograd gradient of GDN.  The GPU tests hold every
kernel family to this reference, so a wrong reference must fail here first."""
import pytest
import torch
import torch.nn.functional as F

import conv_epilogue_ref as R


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float64) * scale


def _close(a, b, tol=1e-9):
    err = (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)
    assert err <= tol, f"rel err {err:.3e}"


def _kernel_layout(W):
    """OIHW -> [O][kh][kw][I] (ops.to_kernel_weight)"""
    return W.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("act,fn", [(R.ACT_LRELU, lambda v: F.leaky_relu(v, 0.01)), (R.ACT_RELU, F.relu), (R.ACT_GELU, F.gelu),
                                    (R.ACT_HALFTANH, lambda v: 0.5 * torch.tanh(v)), (R.ACT_SIGMOID, torch.sigmoid), (R.ACT_NONE, lambda v: v)])
def test_activation_and_derivative_match_torch(act, fn):
    v = _rand((4096,), 1, 3.0)
    _close(R.act_f(v, act), fn(v))
    if act == R.ACT_SIGMOID:
        return   # (forward only: no kernel takes its derivative)
    vg = v.clone().requires_grad_()
    (g,) = torch.autograd.grad(fn(vg).sum(), vg)
    _close(R.act_d(v, act, True), g)
    if act != R.ACT_GELU:   # from the activation OUTPUT: the form the gates take for LeakyReLU / ReLU / HALFTANH
        _close(R.act_d(fn(v), act, False), g)
    _close(R.act_d(g, R.ACT_SAVED_DERIV, False), g)


@pytest.mark.parametrize("res_first", [False, True])
def test_epilogue_order_against_torch_composition(res_first):
    x, W, b = _rand((2, 16, 9, 7), 1), _rand((24, 16, 3, 3), 2, 0.1), _rand((24,), 3)
    res, rg, og = _rand((2, 24, 9, 7), 4), _rand((2, 24, 9, 7), 5), _rand((2, 24, 9, 7), 6)
    y, pre = R.ref_conv(x, _kernel_layout(W), b, ks=3, act=R.ACT_HALFTANH, res=res, res_scale=0.5, res_first=res_first,
                        res_gate=(rg, R.ACT_LRELU, False), y_pre=True, out_gate=(og, R.ACT_HALFTANH, True))
    z = F.conv2d(x, W, b, padding=1)
    rt = 0.5 * res * torch.where(rg > 0, 1.0, 0.01)
    want_pre = z + rt if res_first else z
    want = 0.5 * torch.tanh(want_pre) + (0 if res_first else rt)
    want = want * 0.5 * (1 - torch.tanh(og) ** 2)
    _close(y, want)
    _close(pre, want_pre)
    # pre_deriv: y_pre holds act'(v) instead of v
    y2, pre2 = R.ref_conv(x, _kernel_layout(W), b, ks=3, act=R.ACT_GELU, y_pre=True, pre_deriv=True)
    zg = z.clone().requires_grad_()
    (g,) = torch.autograd.grad(F.gelu(zg).sum(), zg)
    _close(y2, F.gelu(z))
    _close(pre2, g)


def test_shuffle_against_pixel_shuffle():
    x, W, b = _rand((2, 8, 5, 6), 1), _rand((32, 8, 3, 3), 2, 0.2), _rand((32,), 3)
    res = _rand((2, 8, 10, 12), 4)
    y, pre = R.ref_conv(x, _kernel_layout(W), b, ks=3, act=R.ACT_LRELU, res=res, res_scale=0.5, y_pre=True, shuffle=True)
    z = F.pixel_shuffle(F.conv2d(x, W, b, padding=1), 2)
    _close(y, F.leaky_relu(z, 0.01) + 0.5 * res)
    _close(pre, z)
    yf, pref = R.ref_conv(x, _kernel_layout(W), b, ks=3, act=R.ACT_RELU, res=res, res_first=True, y_pre=True, shuffle=True)
    _close(yf, F.relu(z + res))
    _close(pref, z + res)


@pytest.mark.parametrize("ks,stride,H,W", [(3, 1, 7, 9), (3, 2, 8, 10), (1, 2, 6, 8), (1, 1, 5, 5), (3, 2, 16, 16)])
def test_transposed_gemm_is_the_autograd_data_gradient(ks, stride, H, W):
    Cin, Cout, pad = 12, 20, ks // 2
    x = _rand((2, Cin, H, W), 1).requires_grad_()
    Wt = _rand((Cout, Cin, ks, ks), 2, 0.2)
    y = F.conv2d(x, Wt, None, stride=stride, padding=pad)
    dy = _rand(y.shape, 3)
    (dx,) = torch.autograd.grad(y, x, dy)
    # the transposed filter image clc_filter_transpose writes: [Cin][kh][kw][Cout]
    wt = Wt.permute(1, 2, 3, 0).contiguous().view(Cin, ks * ks * Cout)
    got = R.gemm(dy, wt, ks=ks, stride=stride, transposed=True, out_hw=(H, W))
    assert got.shape == dx.shape
    _close(got, dx)
    # with an xs prologue: the data gradient of act(conv(x)) from the saved pre-activation
    z = F.conv2d(x.detach(), Wt, None, stride=stride, padding=pad).requires_grad_()
    (dz,) = torch.autograd.grad(F.leaky_relu(z, 0.01), z, dy)
    got2 = R.gemm(dy, wt, ks=ks, stride=stride, transposed=True, out_hw=(H, W), xs=z.detach(), xs_act=R.ACT_LRELU, xs_pre=True)
    _close(got2, R.gemm(dz, wt, ks=ks, stride=stride, transposed=True, out_hw=(H, W)))


def _compressai_gdn(x, gamma, beta, inverse):
    norm = F.conv2d(x ** 2, gamma.reshape(gamma.shape[0], gamma.shape[1], 1, 1), beta)
    return x * (torch.sqrt(norm) if inverse else torch.rsqrt(norm))


@pytest.mark.parametrize("inverse", [False, True])
def test_gdn_and_mul2_against_compressai(inverse):
    C = 16
    x = _rand((2, C, 6, 5), 1).requires_grad_()
    gamma = _rand((C, C), 2).abs() * 0.1
    beta = 0.5 + torch.rand(C, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    y = _compressai_gdn(x, gamma, beta, inverse)
    got, v = R.ref_conv(x.detach(), gamma, beta, ks=1, in_op=R.IN_SQUARE, norm=R.NORM_IGDN if inverse else R.NORM_GDN, mul=x.detach(), y_pre=True)
    _close(got, y.detach())
    _close(v, F.conv2d(x.detach() ** 2, gamma.view(C, C, 1, 1), beta))
    # _GDNParamFn.backward: dx = dx_direct + 2 x (gamma^T dv), the factor 2 x and the add in a MUL2 data-gradient epilogue
    dy = _rand(y.shape, 4)
    (dx,) = torch.autograd.grad(y, x, dy)
    xd = x.detach()
    if inverse:
        dx_direct, dv = dy * torch.sqrt(v), dy * xd * 0.5 / torch.sqrt(v)
    else:
        dx_direct, dv = dy / torch.sqrt(v), -0.5 * dy * xd * v ** -1.5
    gt = gamma.t().contiguous()   # transposed 1x1 filter [Cin][Cout]
    got_dx, _ = R.ref_conv(dv, gt, None, ks=1, transposed=True, out_hw=(6, 5), norm=R.NORM_MUL2, mul=xd, res=dx_direct)
    _close(got_dx, dx)


def test_stored_geometry_of_shuffled_operands():
    """res / mul / gates of a shuffled launch are read at the STORED pixel: channel c of sub-pixel (i, j) is pre-shuffle channel 4c + 2i + j"""
    acc = _rand((1, 8, 3, 3), 1)
    og = _rand((1, 2, 6, 6), 2)
    y, _ = R.epilogue(acc, out_gate=(og, R.ACT_RELU, False), shuffle=True)
    want = torch.empty(1, 2, 6, 6, dtype=torch.float64)
    for c in range(2):
        for i in range(2):
            for j in range(2):
                want[0, c, i::2, j::2] = acc[0, 4 * c + 2 * i + j]
    _close(y, want * (og > 0))
