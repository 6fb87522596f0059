"""Plain-torch restatement of the checkerboard context model (He et al., CVPR 2021) on ar_ref's mbt2018: an nn.Conv2d context layer
with the registered checkerboard mask buffer (ones at (kh + kw) odd), the usual "zero the non-anchors, convolve with weight * mask, zero
the anchors' outputs" forward, a two-pass coding loop and a one-pass teacher-forced evaluation.  Anchors are the latent pixels with
(h + w) odd.  The reference of tests/test_ckbd_cpu.py and, run in float64, of tests/test_ckbd_model_gpu.py.

The stream order (anchors in raster order, then non-anchors in raster order, channels inner) is the project's own: CompressAI is not
installed where this is built, so nothing here is pinned against its checkerboard classes.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

import ar_ref


def parity_maps(H, W, dtype=torch.float32):
    """(anchor, non-anchor) indicator maps [1, 1, H, W]"""
    odd = ((torch.arange(H).view(H, 1) + torch.arange(W).view(1, W)) % 2).to(dtype).view(1, 1, H, W)
    return odd, 1 - odd


class CheckerboardMaskedConv2d(nn.Conv2d):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.register_buffer("mask", torch.zeros_like(self.weight.data))
        _, _, h, w = self.mask.size()
        for kh in range(h):
            for kw in range(w):
                if (kh + kw) % 2:
                    self.mask[:, :, kh, kw] = 1

    def forward(self, x):
        self.weight.data *= self.mask
        anchor, other = parity_maps(x.shape[2], x.shape[3], x.dtype)
        anchor, other = anchor.to(x.device), other.to(x.device)
        # weight * mask again, as a graph node: the masked taps' gradients are exactly 0
        return F.conv2d(x * anchor, self.weight * self.mask, self.bias, padding=self.padding) * other


class JointCheckerboardHierarchicalPriors(ar_ref.JointAutoregressiveHierarchicalPriors):
    def __init__(self, N=192, M=192):
        super().__init__(N, M)
        self.context_prediction = CheckerboardMaskedConv2d(M, 2 * M, kernel_size=5, padding=2, stride=1)

    def _gaussian_params(self, params, ctx):
        return self.entropy_parameters(torch.cat((params, ctx), dim=1)).chunk(2, 1)

    @torch.no_grad()
    def compress_ckbd(self, y, params):
        """The two passes for a batch: -> (symbols int32 [B, H*W, M], indexes int32 [B, H*W, M], y_hat [B, M, H, W], scales, means);
        the lists are in raster order (the coder takes the anchors first, then the non-anchors)."""
        B, M, H, W = y.shape
        gc = self.gaussian_conditional
        anchor, other = parity_maps(H, W, y.dtype)
        # pass 1: anchors from the hyperprior alone (a zero context)
        s1, m1 = self._gaussian_params(params, torch.zeros((B, 2 * M, H, W), dtype=y.dtype))
        q1 = gc.quantize(y, "symbols", m1)
        y_hat = (q1 + m1) * anchor
        # pass 2: non-anchors from the hyperprior and the context of the anchors
        s2, m2 = self._gaussian_params(params, self.context_prediction(y_hat))
        q2 = gc.quantize(y, "symbols", m2)
        y_hat = y_hat + (q2 + m2) * other
        pick = lambda a, b: torch.where(anchor.bool(), a, b)
        scales, means = pick(s1, s2), pick(m1, m2)
        rows = lambda t: t.permute(0, 2, 3, 1).reshape(B, H * W, M)
        sym = rows(pick(q1, q2)).to(torch.int32)
        idx = rows(pick(gc.build_indexes(s1), gc.build_indexes(s2))).to(torch.int32)
        return sym, idx, y_hat, scales, means

    @torch.no_grad()
    def teacher_forced(self, y_hat, params):
        """(scales, means) of every pixel in one pass from a FINISHED y_hat"""
        return self._gaussian_params(params, self.context_prediction(y_hat))
