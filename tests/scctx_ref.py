"""Plain-torch restatement of ``elic2022`` (ELIC, He et al., CVPR 2022: unevenly grouped space-channel context model) with the
``state_dict`` keys of clc_amd.models.Elic2022: nn.Conv2d / nn.ConvTranspose2d transforms with residual bottleneck blocks and the
oracle's AttentionBlock, per channel group a 5x5 channel-context net over the earlier groups, ckbd_ref's checkerboard layer over the
group's own anchors and a 1x1 aggregation net on cat((hyper parameters, spatial context, channel context)).  It holds the forward (any
dtype), the 2 K-pass coding loop, the one-pass teacher-forced evaluation and the stream order.  Anchors are the latent pixels with
(h + w) odd.  The reference of tests/test_scctx_cpu.py and, run in float64, of tests/test_scctx_model_gpu.py.

Written from the paper; the module names and the stream order (groups ascending; a group's anchors in raster order, then its
non-anchors in raster order; channels inner) are the project's own, nothing is pinned against another implementation.
"""
import torch
import torch.nn as nn

from ckbd_ref import CheckerboardMaskedConv2d, parity_maps
from hyperprior_ref import conv, deconv
from oracle.leaves import AttentionBlock, CompressionModel, GaussianConditional

# the small configuration of the CPU and GPU tests and the weights both use
SMALL = dict(N=8, M=32, groups=(4, 4, 8, 16), ch_widths=(12, 8), agg_widths=(40, 24))


def small_reference():
    """The restatement at SMALL in float32 with the weight recipe (seed 3) and the scalings that make the predictions informative (latent
    spread of +-16 .. 20, predicted scales up to about 2.4, means up to about +-4): g_a's last convolution x 8, h_s's last layer x 4 and
    + 0.6, every group's last aggregation layer x 8 and + 0.6 on its scale half."""
    from clc_amd.recipe import apply_weight_recipe

    r = Elic2022(**SMALL)
    apply_weight_recipe(r, 3)
    with torch.no_grad():
        r.g_a[13].weight.mul_(8.0)
        r.h_s[4].weight.mul_(4.0)
        r.h_s[4].bias.add_(0.6)
        for k, c in enumerate(SMALL["groups"]):
            r.aggregation[k][4].weight.mul_(8.0)
            r.aggregation[k][4].bias[:c].add_(0.6)
    return r


def scctx_order(H, W, groups):
    """[(raster position h * W + w, channel)] in the stream's order"""
    anchors = [h * W + w for h in range(H) for w in range(W) if (h + w) % 2]
    others = [h * W + w for h in range(H) for w in range(W) if not (h + w) % 2]
    out, s = [], 0
    for c in groups:
        for p in anchors + others:
            out += [(p, ch) for ch in range(s, s + c)]
        s += c
    return out


class ResidualBottleneck(nn.Module):
    def __init__(self, C):
        super().__init__()
        self.conv = nn.Sequential(nn.Conv2d(C, C // 2, 1), nn.ReLU(inplace=True), nn.Conv2d(C // 2, C // 2, 3, padding=1), nn.ReLU(inplace=True),
                                  nn.Conv2d(C // 2, C, 1))

    def forward(self, x):
        return x + self.conv(x)


class Elic2022(CompressionModel):
    def __init__(self, N=192, M=320, groups=(16, 16, 32, 64, 192), ch_widths=(224, 128), agg_widths=(640, 512)):
        super().__init__(entropy_bottleneck_channels=N)
        assert sum(groups) == M
        self.N, self.M, self.groups = N, M, tuple(groups)
        self.starts = tuple(sum(groups[:k]) for k in range(len(groups)))
        RBB = ResidualBottleneck
        self.g_a = nn.Sequential(conv(3, N), RBB(N), RBB(N), RBB(N), conv(N, N), RBB(N), RBB(N), RBB(N), AttentionBlock(N),
                                 conv(N, N), RBB(N), RBB(N), RBB(N), conv(N, M), AttentionBlock(M))
        self.g_s = nn.Sequential(AttentionBlock(M), deconv(M, N), RBB(N), RBB(N), RBB(N), deconv(N, N), AttentionBlock(N), RBB(N), RBB(N), RBB(N),
                                 deconv(N, N), RBB(N), RBB(N), RBB(N), deconv(N, 3))
        self.h_a = nn.Sequential(conv(M, N, stride=1, kernel_size=3), nn.ReLU(inplace=True), conv(N, N), nn.ReLU(inplace=True), conv(N, N))
        self.h_s = nn.Sequential(deconv(N, N), nn.ReLU(inplace=True), deconv(N, N * 3 // 2), nn.ReLU(inplace=True),
                                 conv(N * 3 // 2, 2 * M, stride=1, kernel_size=3))
        c0, c1 = ch_widths
        a0, a1 = agg_widths
        c5 = lambda i, o: nn.Conv2d(i, o, 5, padding=2)
        self.channel_context = nn.ModuleList(
            nn.Sequential() if k == 0 else nn.Sequential(c5(s, c0), nn.ReLU(inplace=True), c5(c0, c1), nn.ReLU(inplace=True), c5(c1, 2 * c))
            for k, (s, c) in enumerate(zip(self.starts, groups)))
        self.spatial_context = nn.ModuleList(CheckerboardMaskedConv2d(c, 2 * c, kernel_size=5, padding=2, stride=1) for c in groups)
        self.aggregation = nn.ModuleList(
            nn.Sequential(nn.Conv2d(2 * M + 2 * c + (2 * c if k else 0), a0, 1), nn.ReLU(inplace=True), nn.Conv2d(a0, a1, 1), nn.ReLU(inplace=True),
                          nn.Conv2d(a1, 2 * c, 1))
            for k, c in enumerate(groups))
        self.gaussian_conditional = GaussianConditional(None)

    def _group_params(self, k, params, sp, y_hat):
        """(scales, means) of group k from the hyper parameters, a spatial context map and the earlier groups of y_hat"""
        parts = [params, sp]
        if k:
            parts.append(self.channel_context[k](y_hat[:, :self.starts[k]]))
        return self.aggregation[k](torch.cat(parts, dim=1)).chunk(2, 1)

    def teacher_forced(self, y_hat, params):
        """(scales, means) of every element in one pass per group from a FINISHED y_hat (also the entropy model of forward)"""
        scales, means = [], []
        for k, (s, c) in enumerate(zip(self.starts, self.groups)):
            sc, mu = self._group_params(k, params, self.spatial_context[k](y_hat[:, s:s + c]), y_hat)
            scales.append(sc)
            means.append(mu)
        return torch.cat(scales, 1), torch.cat(means, 1)

    def forward(self, x):
        y = self.g_a(x)
        z = self.h_a(y)
        z_hat, z_likelihoods = self.entropy_bottleneck(z)
        params = self.h_s(z_hat)
        y_hat = self.gaussian_conditional.quantize(y, "noise" if self.training else "dequantize")
        scales_hat, means_hat = self.teacher_forced(y_hat, params)
        _, y_likelihoods = self.gaussian_conditional(y, scales_hat, means=means_hat)
        return {"x_hat": self.g_s(y_hat), "likelihoods": {"y": y_likelihoods, "z": z_likelihoods}}

    @torch.no_grad()
    def compress_scctx(self, y, params):
        """The 2 K passes for a batch: -> (symbols int32 [B, H*W, M], indexes int32 [B, H*W, M], y_hat [B, M, H, W], scales, means); the
        lists are in raster order, channels inner (the coder takes them in scctx_order)."""
        B, M, H, W = y.shape
        gc = self.gaussian_conditional
        anchor, other = parity_maps(H, W, y.dtype)
        pick = lambda a, b: torch.where(anchor.bool(), a, b)
        y_hat = torch.zeros_like(y)
        scales, means, syms, idxs = [], [], [], []
        for k, (s, c) in enumerate(zip(self.starts, self.groups)):
            yk = y[:, s:s + c]
            # pass A: the group's anchors from the hyperprior and the earlier groups (a zero spatial context)
            s1, m1 = self._group_params(k, params, torch.zeros((B, 2 * c, H, W), dtype=y.dtype), y_hat)
            q1 = gc.quantize(yk, "symbols", m1)
            y_hat[:, s:s + c] = (q1 + m1) * anchor
            # pass B: its non-anchors, additionally from the checkerboard context of its anchors
            s2, m2 = self._group_params(k, params, self.spatial_context[k](y_hat[:, s:s + c]), y_hat)
            q2 = gc.quantize(yk, "symbols", m2)
            y_hat[:, s:s + c] = y_hat[:, s:s + c] + (q2 + m2) * other
            scales.append(pick(s1, s2))
            means.append(pick(m1, m2))
            syms.append(pick(q1, q2))
            idxs.append(pick(gc.build_indexes(s1), gc.build_indexes(s2)))
        rows = lambda t: t.permute(0, 2, 3, 1).reshape(B, H * W, M)
        return (rows(torch.cat(syms, 1)).to(torch.int32), rows(torch.cat(idxs, 1)).to(torch.int32), y_hat, torch.cat(scales, 1),
                torch.cat(means, 1))
