"""Plain-torch restatement of ``mbt2018`` (JointAutoregressiveHierarchicalPriors as CompressAI publishes it) on hyperprior_ref's
MeanScaleHyperprior: an nn.Conv2d context layer with the registered mask buffer, the three 1x1 layers of ``entropy_parameters``, the
published forward and the published raster coding loop (``_compress_ar``: zero-padded y_hat, one 5x5 crop per pixel).  The reference of
tests/test_ar_cpu.py (state_dict keys and shapes) and, run in float64, of tests/test_ar_model_gpu.py.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from hyperprior_ref import MeanScaleHyperprior


class MaskedConv2d(nn.Conv2d):
    def __init__(self, *args, mask_type="A", **kwargs):
        super().__init__(*args, **kwargs)
        assert mask_type in ("A", "B")
        self.register_buffer("mask", torch.ones_like(self.weight.data))
        _, _, h, w = self.mask.size()
        self.mask[:, :, h // 2, w // 2 + (mask_type == "B"):] = 0
        self.mask[:, :, h // 2 + 1:] = 0

    def forward(self, x):
        self.weight.data *= self.mask
        return super().forward(x)


class JointAutoregressiveHierarchicalPriors(MeanScaleHyperprior):
    def __init__(self, N=192, M=192):
        super().__init__(N, M)
        self.entropy_parameters = nn.Sequential(nn.Conv2d(M * 12 // 3, M * 10 // 3, 1), nn.LeakyReLU(inplace=True),
                                                nn.Conv2d(M * 10 // 3, M * 8 // 3, 1), nn.LeakyReLU(inplace=True),
                                                nn.Conv2d(M * 8 // 3, M * 6 // 3, 1))
        self.context_prediction = MaskedConv2d(M, 2 * M, kernel_size=5, padding=2, stride=1)

    def forward(self, x):
        y = self.g_a(x)
        z = self.h_a(y)
        z_hat, z_likelihoods = self.entropy_bottleneck(z)
        params = self.h_s(z_hat)
        y_hat = self.gaussian_conditional.quantize(y, "noise" if self.training else "dequantize")
        ctx_params = self.context_prediction(y_hat)
        gaussian_params = self.entropy_parameters(torch.cat((params, ctx_params), dim=1))
        scales_hat, means_hat = gaussian_params.chunk(2, 1)
        _, y_likelihoods = self.gaussian_conditional(y, scales_hat, means=means_hat)
        return {"x_hat": self.g_s(y_hat), "likelihoods": {"y": y_likelihoods, "z": z_likelihoods}}

    @torch.no_grad()
    def compress_ar(self, y, params):
        """The published raster loop for a batch: -> (symbols int32 [B, H*W, M], indexes int32 [B, H*W, M], y_hat [B, M, H, W],
        scales [B, M, H, W], means [B, M, H, W]); per image the lists are in the coder's order (raster pixels, channels inner)."""
        k, pad = 5, 2
        B, M, H, W = y.shape
        cp = self.context_prediction
        masked_weight = cp.weight * cp.mask
        y_hat = F.pad(torch.zeros_like(y), (pad, pad, pad, pad))
        sym = torch.zeros((B, H * W, M), dtype=torch.int32)
        idx = torch.zeros((B, H * W, M), dtype=torch.int32)
        scales, means = torch.zeros_like(y), torch.zeros_like(y)
        for h in range(H):
            for w in range(W):
                y_crop = y_hat[:, :, h:h + k, w:w + k]
                ctx_p = F.conv2d(y_crop, masked_weight, bias=cp.bias)
                p = params[:, :, h:h + 1, w:w + 1]
                gaussian_params = self.entropy_parameters(torch.cat((p, ctx_p), dim=1)).squeeze(3).squeeze(2)
                s, m = gaussian_params.chunk(2, 1)
                y_q = self.gaussian_conditional.quantize(y[:, :, h, w], "symbols", m)
                sym[:, h * W + w] = y_q
                idx[:, h * W + w] = self.gaussian_conditional.build_indexes(s)
                y_hat[:, :, h + pad, w + pad] = y_q + m
                scales[:, :, h, w], means[:, :, h, w] = s, m
        return sym, idx, y_hat[:, :, pad:-pad, pad:-pad].contiguous(), scales, means

    @torch.no_grad()
    def teacher_forced(self, y_hat, params, whole_map=False):
        """(scales, means) of every pixel in one parallel pass from a FINISHED y_hat: the masked convolution of the whole map, then
        entropy_parameters.  The convolution is evaluated in its patch-row form — every pixel's zero-padded 5x5 crop as one sample of a
        batch — because torch's float64 convolution multiplies sample by sample: a crop is then the very matrix-vector product the
        sequential loop runs, while the whole map as one sample is a matrix-matrix product that the BLAS sums in another order (a few
        float64 ulps apart: 0.9e-15 .. 1.2e-15 on values up to 1.6, measured, more than the 1e-15 this pass is held to against the
        loop).  whole_map=True is that direct form, kept for comparison."""
        cp = self.context_prediction
        if whole_map:
            return self.entropy_parameters(torch.cat((params, cp(y_hat)), dim=1)).chunk(2, 1)
        B, M, H, W = y_hat.shape
        crops = F.unfold(F.pad(y_hat, (2, 2, 2, 2)), 5).transpose(1, 2).reshape(B * H * W, M, 5, 5)
        ctx = F.conv2d(crops, cp.weight * cp.mask, bias=cp.bias)
        p = params.permute(0, 2, 3, 1).reshape(B * H * W, -1, 1, 1)
        gp = self.entropy_parameters(torch.cat((p, ctx), dim=1))
        return gp.reshape(B, H, W, -1).permute(0, 3, 1, 2).chunk(2, 1)
