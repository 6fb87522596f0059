"""Float64 reference of the clc_conv2d contract (include/clc_hip.h, clc_amd/csrc/conv_common.h: epilogue_store), in plain PyTorch.

Imported by tests/test_conv_epilogue_ref_cpu.py, which pins it against independent torch compositions, and by
tests/test_conv_epilogue_gpu.py, which holds every convolution family to it.  Tensors are logical NCHW; filters are given exactly as
ops.conv_raw takes them (kernel layout): forward [Cout][ks][ks][Cin], data gradient the transposed filter [Cin_fwd][ks][ks][Cout_fwd].

The contract, in this order:
    v     = acc + bias
    rt    = res_scale * res * (act'(res_gate; rg_act, rg_pre) if res_gate else 1)
    v    += rt                                     if res_first
    y_pre = act'(v; act, pre=1) if pre_deriv else v
    v     = mul * rsqrt(v) | mul * sqrt(v) | 2 * (mul * v)      norm = GDN | IGDN | MUL2
    v     = act(v)
    v    += rt                                     if not res_first
    v    *= act'(out_gate; og_act, og_pre)         if out_gate
    stored PixelShuffle(2)-ed when shuffle (res, mul and the gates are read in the stored geometry)
with acc = conv(in_op(x) * act'(xs; xs_act, xs_pre), w) for forward launches and its data gradient for transposed ones.
"""
import math

import torch
import torch.nn.functional as F

ACT_NONE, ACT_LRELU, ACT_RELU, ACT_GELU, ACT_HALFTANH, ACT_SIGMOID, ACT_SAVED_DERIV = 0, 1, 2, 3, 4, 5, 6
IN_NONE, IN_SQUARE = 0, 1
NORM_NONE, NORM_GDN, NORM_IGDN, NORM_MUL2 = 0, 1, 2, 3
ACT_NAMES = {ACT_NONE: "none", ACT_LRELU: "lrelu", ACT_RELU: "relu", ACT_GELU: "gelu", ACT_HALFTANH: "halftanh", ACT_SIGMOID: "sigmoid",
             ACT_SAVED_DERIV: "saved"}


def act_f(v, act):
    """act(v) (common.h: apply_act)"""
    if act == ACT_NONE:
        return v
    if act == ACT_LRELU:
        return torch.where(v > 0, v, 0.01 * v)
    if act == ACT_RELU:
        return torch.where(v > 0, v, torch.zeros_like(v))
    if act == ACT_GELU:
        return v * 0.5 * (1.0 + torch.erf(v / math.sqrt(2.0)))
    if act == ACT_HALFTANH:
        return 0.5 * torch.tanh(v)
    if act == ACT_SIGMOID:
        return 1.0 / (1.0 + torch.exp(-v))
    raise ValueError(f"act {act} has no forward form")


def act_d(s, act, use_pre):
    """act'(.) from the saved tensor s: the pre-activation (use_pre) or the activation output (common.h: act_deriv)"""
    if act == ACT_NONE:
        return torch.ones_like(s)
    if act in (ACT_LRELU, ACT_RELU):   # (LeakyReLU / ReLU keep the sign: output and pre-activation give the same branch)
        return torch.where(s > 0, torch.ones_like(s), torch.full_like(s, 0.01 if act == ACT_LRELU else 0.0))
    if act == ACT_GELU:
        assert use_pre, "GELU's derivative needs the pre-activation"
        return 0.5 * (1.0 + torch.erf(s / math.sqrt(2.0))) + s * torch.exp(-0.5 * s * s) / math.sqrt(2.0 * math.pi)
    if act == ACT_HALFTANH:
        t = torch.tanh(s) if use_pre else 2.0 * s
        return 0.5 * (1.0 - t * t)
    if act == ACT_SAVED_DERIV:
        return s
    raise ValueError(f"act {act} has no derivative form")


def torch_filter(w, *, ks, transposed):
    """kernel-layout filter -> the OIHW weight of the FORWARD convolution (for transposed launches: of the layer whose data gradient it is)"""
    w = w.double().reshape(w.shape[0], ks, ks, -1)
    if transposed:   # [Cin_fwd][kh][kw][Cout_fwd] -> [Cout_fwd][Cin_fwd][kh][kw]
        return w.permute(3, 0, 1, 2).contiguous()
    return w.permute(0, 3, 1, 2).contiguous()


def gemm(x, w, *, ks, stride=1, pad=None, transposed=False, out_hw=None, in_op=IN_NONE, xs=None, xs_act=ACT_NONE, xs_pre=False):
    """The accumulator of a clc_conv2d launch in float64: [N, Cout, OH, OW] before any epilogue (PixelShuffle is an epilogue step)."""
    pad = ks // 2 if pad is None else pad
    x = x.double()
    if in_op == IN_SQUARE:
        x = x * x
    if xs is not None:
        x = x * act_d(xs.double(), xs_act, xs_pre)
    W = torch_filter(w, ks=ks, transposed=transposed)
    if not transposed:
        return F.conv2d(x, W, None, stride=stride, padding=pad)
    OH, OW = out_hw
    H, Wd = x.shape[2], x.shape[3]
    oph, opw = OH - ((H - 1) * stride - 2 * pad + ks), OW - ((Wd - 1) * stride - 2 * pad + ks)
    return F.conv_transpose2d(x, W, None, stride=stride, padding=pad, output_padding=(oph, opw))


def epilogue(acc, bias=None, *, act=ACT_NONE, res=None, res_scale=1.0, res_first=False, res_gate=None, y_pre=False, pre_deriv=False,
             norm=NORM_NONE, mul=None, out_gate=None, shuffle=False):
    """acc [N, C, H, W] float64 -> (y, y_pre or None).  res / mul / res_gate[0] / out_gate[0] are in the STORED geometry (after the shuffle);
    res_gate / out_gate = (saved tensor, act, saved_is_pre)."""
    d = lambda t: None if t is None else t.double()
    un = (lambda t: F.pixel_unshuffle(t, 2)) if shuffle else (lambda t: t)
    v = acc.double()
    if bias is not None:
        v = v + bias.double().view(1, -1, 1, 1)
    rt = None
    if res is not None:
        rt = res_scale * un(d(res))
        if res_gate is not None:
            rt = rt * act_d(un(d(res_gate[0])), res_gate[1], res_gate[2])
        if res_first:
            v = v + rt
    pre = (act_d(v, act, True) if pre_deriv else v) if y_pre else None
    if norm == NORM_GDN:
        v = un(d(mul)) / torch.sqrt(v)
    elif norm == NORM_IGDN:
        v = un(d(mul)) * torch.sqrt(v)
    elif norm == NORM_MUL2:
        v = 2.0 * (un(d(mul)) * v)
    v = act_f(v, act)
    if rt is not None and not res_first:
        v = v + rt
    if out_gate is not None:
        v = v * act_d(un(d(out_gate[0])), out_gate[1], out_gate[2])
    if shuffle:
        v = F.pixel_shuffle(v, 2)
        pre = F.pixel_shuffle(pre, 2) if pre is not None else None
    return v, pre


def ref_conv(x, w, bias=None, *, ks, stride=1, pad=None, transposed=False, out_hw=None, in_op=IN_NONE, xs=None, xs_act=ACT_NONE, xs_pre=False,
             **epi):
    """(y, y_pre) of one clc_conv2d launch in float64 (epi: the keyword arguments of `epilogue`)."""
    acc = gemm(x, w, ks=ks, stride=stride, pad=pad, transposed=transposed, out_hw=out_hw, in_op=in_op, xs=xs, xs_act=xs_act, xs_pre=xs_pre)
    return epilogue(acc, bias, **epi)


def away_from_zero(shape, seed, scale=1.0):
    """sign * (0.1 + |n|): gate / xs operands that sit clear of every activation kink"""
    g = torch.Generator().manual_seed(seed)
    n = torch.randn(shape, generator=g, dtype=torch.float64)
    return (torch.sign(n) * (0.1 + n.abs()) * scale).float()
