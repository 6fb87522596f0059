"""Conditional Latent Matching modules of /root/reference/models/CLM.py on the HIP engine, forward and backward.

Same class names, constructor arguments and parameter names as the reference file (``CLM``, ``SimpleCLM``,
``DeformableAlignment``): ``feature_transform.{0,2}``, ``alignment.{offset_conv,modulation_conv}``, ``attention_conv``,
``fusion_conv.{0,2}``.  The reference module is an orphan (nothing imports it) whose deformable alignment is a Python
quadruple loop; here the similarity softmax is reduced to its column sums on the fly (the only thing the reference's
``weighted_x`` loop uses), the 9-tap modulated bilinear sampling is one kernel, and all convs run on the implicit GEMM.

Two paths, chosen per call:
  * under ``torch.no_grad()`` (or when nothing requires a gradient) the inference forward: ``clc_clm_sim_colsum`` and the convolutions
    through ``ops.conv_raw``, the sigmoid of the modulation head fused into its epilogue;
  * otherwise the recorded forward: the similarity column sums on the matrix cores (``clc_clm_sim_colsum_train``, which also keeps the
    softmax row statistics), the convolutions through ``ops.conv2d``, and one ``torch.autograd.Function`` per CLM op whose backward is
    one HIP entry point (csrc/clm_train.hip).  No op uses floating-point atomics: two backward passes give the same bits.
The data gradient of a convolution needs its output channel count to be a multiple of 4, so the recorded path zero-pads the 18-, 9-
and 1-channel heads to 20 / 12 / 4 filter rows (built from the parameters with plain torch ops, so the parameters keep the
reference's shapes and receive their gradients through the pad) and hands the padded leading dimensions to the CLM kernels.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import lib as _lib
from . import ops
from .layers import Conv2d
from .lib import ACT_NONE, ACT_RELU, ACT_SIGMOID
from .ops import CL, _L, _stream, dense, new_act, nhwc

# list -> every backward below appends (op name, {output: was it computed}) — which sweeps needs_input_grad let through
TRACE = None


def _trace(name, **ran):
    if TRACE is not None:
        TRACE.append((name, ran))


def _records(module, *tensors) -> bool:
    """does this call have to record an autograd graph?"""
    return torch.is_grad_enabled() and (any(t.requires_grad for t in tensors) or any(p.requires_grad for p in module.parameters()))


def _pad_rows(conv: Conv2d, rows):
    """(filter, bias) of `conv` with zero output channels appended up to `rows` (differentiable: the parameters get the gradient's first rows)"""
    w, b = conv.weight, conv.bias
    n = rows - w.shape[0]
    w = torch.cat([w, w.new_zeros((n,) + tuple(w.shape[1:]))], 0).contiguous(memory_format=CL)
    return w, torch.cat([b, b.new_zeros(n)], 0)


class _SimColsumFn(torch.autograd.Function):
    """colsum[b, q] = sum_p softmax_q(yt[b, p, :] . yr[b, q, :] / temperature); saves the row statistics, never the matrix."""

    @staticmethod
    def forward(ctx, yt, yr, temperature):
        ops._require_gpu(yt, "clm.sim_colsum")
        ops._require_gpu(yr, "clm.sim_colsum")
        if yt.shape != yr.shape:
            raise _lib.ClcError(f"clm.sim_colsum: shapes {tuple(yt.shape)} and {tuple(yr.shape)} differ")
        yt, yr = dense(yt), dense(yr)
        B, Cc, H, W = yt.shape
        colsum = torch.empty((B, H * W), device=yt.device, dtype=torch.float32)
        m, l = torch.empty_like(colsum), torch.empty_like(colsum)
        _lib.check(_L().clc_clm_sim_colsum_train(yt.data_ptr(), Cc, yr.data_ptr(), Cc, B, H * W, Cc, float(temperature), colsum.data_ptr(),
                                                 m.data_ptr(), l.data_ptr(), _stream()), "clc_clm_sim_colsum_train")
        ctx.temperature = float(temperature)
        ctx.save_for_backward(yt, yr, m, l)
        return colsum

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        yt, yr, m, l = ctx.saved_tensors
        B, Cc, H, W = yt.shape
        g = g.contiguous()
        dyt = new_act(B, Cc, H, W, yt) if ctx.needs_input_grad[0] else None
        dyr = new_act(B, Cc, H, W, yt) if ctx.needs_input_grad[1] else None
        _trace("sim_colsum_bwd", dyt=dyt is not None, dyr=dyr is not None)
        L = _L()
        nbytes = L.clc_clm_sim_colsum_bwd_workspace_bytes(B, H * W)
        ws = torch.empty((nbytes + 3) // 4, device=yt.device, dtype=torch.float32)
        _lib.check(L.clc_clm_sim_colsum_bwd(yt.data_ptr(), Cc, yr.data_ptr(), Cc, m.data_ptr(), l.data_ptr(), g.data_ptr(), B, H * W, Cc, ctx.temperature,
                                            dyt.data_ptr() if dyt is not None else None, Cc, dyr.data_ptr() if dyr is not None else None, Cc,
                                            ws.data_ptr(), nbytes, _stream()), "clc_clm_sim_colsum_bwd")
        return dyt, dyr, None


def sim_colsum(yt, yr, temperature):
    """recorded similarity column sums of two [B,C,H,W] latents -> [B, H*W] (differentiable in both)"""
    return _SimColsumFn.apply(yt, yr, temperature)


class _ScaleCatFn(torch.autograd.Function):
    """cat([x, colsum * x], dim=1)  (CLM.py:16-23)"""

    @staticmethod
    def forward(ctx, x, colsum):
        x = dense(x)
        B, Cc, H, W = x.shape
        cat = new_act(B, 2 * Cc, H, W, x)
        L = _L()
        _lib.check(L.clc_copy2d(x.data_ptr(), Cc, cat.data_ptr(), 2 * Cc, B * H * W, Cc, _stream()), "clc_copy2d")
        _lib.check(L.clc_clm_scale_rows(x.data_ptr(), Cc, colsum.data_ptr(), cat.data_ptr() + 4 * Cc, 2 * Cc, B * H * W, Cc, _stream()), "clc_clm_scale_rows")
        ctx.save_for_backward(x, colsum)
        return cat

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dcat):
        x, colsum = ctx.saved_tensors
        B, Cc, H, W = x.shape
        dcat = dense(dcat)
        L = _L()
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = new_act(B, Cc, H, W, x)
            _lib.check(L.clc_copy2d(dcat.data_ptr(), 2 * Cc, dx.data_ptr(), Cc, B * H * W, Cc, _stream()), "clc_copy2d")
        if ctx.needs_input_grad[1]:
            dw = torch.empty_like(colsum)
        _trace("scale_rows_bwd", dx=dx is not None, dw=dw is not None)
        if dx is not None or dw is not None:
            _lib.check(L.clc_clm_scale_rows_bwd(dcat.data_ptr() + 4 * Cc, 2 * Cc, x.data_ptr(), Cc, colsum.data_ptr(), dw.data_ptr() if dw is not None else None,
                                                dx.data_ptr() if dx is not None else None, Cc, B * H * W, Cc, _stream()), "clc_clm_scale_rows_bwd")
        return dx, dw


class _DeformFn(torch.autograd.Function):
    """9-tap modulated bilinear sampling (CLM.py:35-60) of x at p + offset, modulation = sigmoid(logit); offset / logit rows may be padded."""

    @staticmethod
    def forward(ctx, x, offset, logit):
        ops._require_gpu(x, "clm.deform")
        x, offset, logit = dense(x), dense(offset), dense(logit)
        B, Cc, H, W = x.shape
        ldo, ldm = offset.shape[1], logit.shape[1]
        if offset.shape[0] != B or tuple(offset.shape[2:]) != (H, W) or tuple(logit.shape[2:]) != (H, W) or logit.shape[0] != B:
            raise _lib.ClcError(f"clm.deform: x {tuple(x.shape)}, offset {tuple(offset.shape)}, modulation {tuple(logit.shape)} do not fit")
        L = _L()
        mod = new_act(B, ldm, H, W, x)
        _lib.check(L.clc_clm_sigmoid(logit.data_ptr(), ldm, mod.data_ptr(), ldm, B * H * W, ldm, _stream()), "clc_clm_sigmoid")
        out = new_act(B, Cc, H, W, x)
        _lib.check(L.clc_clm_deform(x.data_ptr(), Cc, offset.data_ptr(), ldo, mod.data_ptr(), ldm, out.data_ptr(), Cc, B, H, W, Cc, _stream()), "clc_clm_deform")
        ctx.save_for_backward(x, offset, mod)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, da):
        x, offset, mod = ctx.saved_tensors
        B, Cc, H, W = x.shape
        ldo, ldm = offset.shape[1], mod.shape[1]
        da = dense(da)
        L = _L()
        dx = doff = dlogit = None
        nbytes = 0
        ws = None
        if ctx.needs_input_grad[0]:
            dx = new_act(B, Cc, H, W, x)
            nbytes = L.clc_clm_deform_bwd_workspace_bytes(B, H, W)
            ws = torch.empty((nbytes + 3) // 4, device=x.device, dtype=torch.float32)
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            doff, dlogit = new_act(B, ldo, H, W, x), new_act(B, ldm, H, W, x)
        _trace("deform_bwd", dx=dx is not None, doff=doff is not None)
        if dx is not None or doff is not None:
            _lib.check(L.clc_clm_deform_bwd(x.data_ptr(), Cc, offset.data_ptr(), ldo, mod.data_ptr(), ldm, da.data_ptr(), Cc,
                                            doff.data_ptr() if doff is not None else None, ldo, dlogit.data_ptr() if dlogit is not None else None, ldm,
                                            dx.data_ptr() if dx is not None else None, Cc, B, H, W, Cc, ws.data_ptr() if ws is not None else None, nbytes,
                                            _stream()), "clc_clm_deform_bwd")
        return dx, doff, dlogit


def deform(x, offset, logit):
    """recorded modulated deformable sampling: x [B,C,H,W], offset [B,>=18,H,W] (channel 2k + {0: dh, 1: dw}), logit [B,>=9,H,W] (pre-sigmoid)"""
    return _DeformFn.apply(x, offset, logit)


class _FuseFn(torch.autograd.Function):
    """sum_m softmax_m(att_m) * feat_m (* sigmoid(att_m) if gate) + y  (CLM.py:118-125, SimpleCLM :166-179); att rows may be padded."""

    @staticmethod
    def forward(ctx, gate, y, *fa):
        M = len(fa) // 2
        if M < 1 or M > 8:
            raise _lib.ClcError("clm.fuse: 1..8 reference features")
        ops._require_gpu(y, "clm.fuse")
        y = dense(y)
        feats, atts = [dense(f) for f in fa[:M]], [dense(a) for a in fa[M:]]
        B, Cc, H, W = y.shape
        lda = atts[0].shape[1]
        if any(f.shape != y.shape for f in feats) or any(tuple(a.shape) != (B, lda, H, W) for a in atts):
            raise _lib.ClcError("clm.fuse: features shaped like y, each with an attention map of the same size")
        out = new_act(B, Cc, H, W, y)
        fp = _lib.ptr_array([f.data_ptr() for f in feats])
        ap = _lib.ptr_array([a.data_ptr() for a in atts])
        _lib.check(_L().clc_clm_fuse(fp, ap, M, Cc, lda, y.data_ptr(), Cc, out.data_ptr(), Cc, B * H * W, Cc, int(gate), _stream()), "clc_clm_fuse")
        ctx.gate, ctx.M = int(gate), M
        ctx.save_for_backward(*feats, *atts)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        M = ctx.M
        saved = ctx.saved_tensors
        feats, atts = saved[:M], saved[M:]
        dout = dense(dout)
        B, Cc, H, W = dout.shape
        lda = atts[0].shape[1]
        dfeats = [new_act(B, Cc, H, W, dout) for _ in range(M)]
        datts = [new_act(B, lda, H, W, dout) for _ in range(M)]
        fp = _lib.ptr_array([f.data_ptr() for f in feats])
        ap = _lib.ptr_array([a.data_ptr() for a in atts])
        dfp = _lib.ptr_array([f.data_ptr() for f in dfeats])
        dap = _lib.ptr_array([a.data_ptr() for a in datts])
        _lib.check(_L().clc_clm_fuse_bwd(fp, ap, M, Cc, lda, dout.data_ptr(), Cc, dfp, Cc, dap, lda, B * H * W, Cc, ctx.gate, _stream()), "clc_clm_fuse_bwd")
        return (None, dout) + tuple(dfeats) + tuple(datts)


def fuse(feats, atts, y, gate):
    """recorded fusion over the references: feats M x [B,C,H,W], atts M x [B,>=1,H,W] (logit in channel 0)"""
    return _FuseFn.apply(bool(gate), y, *feats, *atts)


def _conv_infer(conv: Conv2d, x, act=ACT_NONE):
    with torch.no_grad():
        return ops.conv_raw(x, ops.to_kernel_weight(conv.weight), conv.bias, ks=conv.kernel_size[0], stride=1, act=act)


class DeformableAlignment(nn.Module):
    def __init__(self, input_dim):
        super().__init__()
        self.offset_conv = Conv2d(input_dim * 2, 2 * 3 * 3, 3)
        self.modulation_conv = Conv2d(input_dim * 2, 3 * 3, 3)
        self.last_offset = None

    def forward(self, x, colsum):
        """x: reference latent [B,C,H,W]; colsum: [B, H*W] column sums of the similarity softmax."""
        if _records(self, x, colsum):
            return self._forward_recorded(x, colsum)
        with torch.no_grad():
            return self._forward_infer(x, colsum)

    def _forward_recorded(self, x, colsum):
        ops._require_gpu(x, "clm.DeformableAlignment")
        cat = _ScaleCatFn.apply(x, colsum)
        wo, bo = _pad_rows(self.offset_conv, 20)
        wm, bm = _pad_rows(self.modulation_conv, 12)
        offset = ops.conv2d(cat, wo, bo)   # [B,20,H,W], channels 18, 19 zero
        logit = ops.conv2d(cat, wm, bm)    # [B,12,H,W] pre-sigmoid: the deform backward hands back the gradient of the pre-activation
        self.last_offset = offset.detach()[:, :18]   # (debug: the sampling offsets of the last recorded call)
        return deform(x, offset, logit)

    def _forward_infer(self, x, colsum):
        x = dense(x)
        B, Cc, H, W = x.shape
        cat = new_act(B, 2 * Cc, H, W, x)
        L = _L()
        _lib.check(L.clc_copy2d(x.data_ptr(), Cc, cat.data_ptr(), 2 * Cc, B * H * W, Cc, _stream()), "clc_copy2d")
        _lib.check(L.clc_clm_scale_rows(x.data_ptr(), Cc, colsum.data_ptr(), cat.data_ptr() + 4 * Cc, 2 * Cc, B * H * W, Cc, _stream()), "clc_clm_scale_rows")
        offset = _conv_infer(self.offset_conv, cat)                      # [B,18,H,W] pixel-major
        modulation = _conv_infer(self.modulation_conv, cat, ACT_SIGMOID)  # sigmoid fused in the epilogue
        out = new_act(B, Cc, H, W, x)
        _lib.check(L.clc_clm_deform(x.data_ptr(), Cc, offset.data_ptr(), 18, modulation.data_ptr(), 9, out.data_ptr(), Cc, B, H, W, Cc, _stream()), "clc_clm_deform")
        return out


def _fuse(feats, atts, y, gate):
    y = dense(y)
    B, Cc, H, W = y.shape
    feats = [dense(f) for f in feats]
    atts = [dense(a) for a in atts]
    out = new_act(B, Cc, H, W, y)
    fp = _lib.ptr_array([f.data_ptr() for f in feats])
    ap = _lib.ptr_array([a.data_ptr() for a in atts])
    _lib.check(_L().clc_clm_fuse(fp, ap, len(feats), Cc, 1, y.data_ptr(), Cc, out.data_ptr(), Cc, B * H * W, Cc, int(gate), _stream()), "clc_clm_fuse")
    return out


class CLM(nn.Module):
    """Conditional Latent Matching (CLM.py:62-128)."""

    def __init__(self, input_dim, temperature=0.5):
        super().__init__()
        self.temperature = temperature
        self.feature_transform = nn.Sequential(Conv2d(input_dim, input_dim, 1), nn.ReLU(inplace=True), Conv2d(input_dim, input_dim, 1))
        self.alignment = DeformableAlignment(input_dim)
        self.attention_conv = Conv2d(input_dim, 1, 1)
        self.fusion_conv = nn.Sequential(Conv2d(input_dim, input_dim, 3), nn.ReLU(inplace=True), Conv2d(input_dim, input_dim, 3))
        self.last_offsets = []

    def _ft(self, x):
        return _conv_infer(self.feature_transform[2], _conv_infer(self.feature_transform[0], x, ACT_RELU))

    def forward(self, y, y_refs):
        if not y.is_cuda:
            raise _lib.ClcError("clc_amd.clm runs on the GPU only")
        if len(y_refs) > 8:
            raise ValueError("at most 8 reference latents")
        if _records(self, y, *y_refs):
            return self._forward_recorded(y, y_refs)
        with torch.no_grad():
            return self._forward_infer(y, y_refs)

    def _forward_recorded(self, y, y_refs):
        ft0, ft2 = self.feature_transform[0], self.feature_transform[2]
        y = y.float().contiguous(memory_format=CL)
        y_t = ft2(ft0(y, act=ACT_RELU))
        wa, ba = _pad_rows(self.attention_conv, 4)
        aligned, atts = [], []
        self.last_offsets = []   # (debug: the sampling offsets [B,18,H,W] of this call, one per reference)
        for y_ref in y_refs:
            y_ref = y_ref.float().contiguous(memory_format=CL)
            colsum = sim_colsum(y_t, ft2(ft0(y_ref, act=ACT_RELU)), self.temperature)
            a = self.alignment(y_ref, colsum)
            self.last_offsets.append(self.alignment.last_offset)
            aligned.append(a)
            atts.append(ops.conv2d(a, wa, ba))
        s = fuse(aligned, atts, y, gate=False)
        return self.fusion_conv[2](self.fusion_conv[0](s, act=ACT_RELU))

    def _forward_infer(self, y, y_refs):
        y = y.float().contiguous(memory_format=CL)
        B, Cc, H, W = y.shape
        y_t = self._ft(y)
        aligned, atts = [], []
        L = _L()
        for y_ref in y_refs:
            y_ref = y_ref.float().contiguous(memory_format=CL)
            y_ref_t = self._ft(y_ref)
            nbytes = L.clc_clm_sim_colsum_workspace_bytes(B, H * W)
            ws = torch.empty((nbytes + 3) // 4, device=y.device, dtype=torch.float32)
            colsum = torch.empty(B * H * W, device=y.device, dtype=torch.float32)
            _lib.check(L.clc_clm_sim_colsum(y_t.data_ptr(), Cc, y_ref_t.data_ptr(), Cc, B, H * W, Cc, float(self.temperature), colsum.data_ptr(),
                                            ws.data_ptr(), nbytes, _stream()), "clc_clm_sim_colsum")
            a = self.alignment(y_ref, colsum)
            aligned.append(a)
            atts.append(_conv_infer(self.attention_conv, a))
        s = _fuse(aligned, atts, y, gate=False)
        return _conv_infer(self.fusion_conv[2], _conv_infer(self.fusion_conv[0], s, ACT_RELU))


class SimpleCLM(nn.Module):
    """Simplified variant (CLM.py:130-187)."""

    def __init__(self, input_dim, temperature=0.5):
        super().__init__()
        self.temperature = temperature
        self.feature_transform = Conv2d(input_dim, input_dim, 1)
        self.attention_conv = Conv2d(input_dim, 1, 1)
        self.fusion_conv = nn.Sequential(Conv2d(input_dim, input_dim, 3), nn.ReLU(inplace=True))

    def forward(self, y, y_refs):
        if not y.is_cuda:
            raise _lib.ClcError("clc_amd.clm runs on the GPU only")
        if _records(self, y, *y_refs):
            return self._forward_recorded(y, y_refs)
        with torch.no_grad():
            return self._forward_infer(y, y_refs)

    def _forward_recorded(self, y, y_refs):
        y = y.float().contiguous(memory_format=CL)
        wa, ba = _pad_rows(self.attention_conv, 4)
        feats = [self.feature_transform(r.float().contiguous(memory_format=CL)) for r in y_refs]
        atts = [ops.conv2d(f, wa, ba) for f in feats]
        s = fuse(feats, atts, y, gate=True)
        return self.fusion_conv[0](s, act=ACT_RELU)

    def _forward_infer(self, y, y_refs):
        y = y.float().contiguous(memory_format=CL)
        feats = [_conv_infer(self.feature_transform, r.float().contiguous(memory_format=CL)) for r in y_refs]
        atts = [_conv_infer(self.attention_conv, f) for f in feats]
        s = _fuse(feats, atts, y, gate=True)
        return _conv_infer(self.fusion_conv[0], s, ACT_RELU)
