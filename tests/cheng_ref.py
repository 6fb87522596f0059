"""Plain-torch restatement of ``cheng2020-anchor`` / ``cheng2020-attn`` (Cheng et al., CVPR 2020), float64-capable: the two models on the
oracle's leaves (layer list from the published CompressAI classes and the paper), the K-component mixture likelihood, the integer
CDF-row rule of the table-free coder and the stream order.  The reference of tests/test_cheng_cpu.py, tests/test_gmm_kernels_gpu.py and
tests/test_cheng_model_gpu.py.

The K > 1 layout: ``entropy_parameters`` ends in 3 K N channels, channel part * K N + k N + c with part 0 the scales, 1 the means, 2 the
weight logits.

THE ROW RULE, per element, from its 3 K parameters (``cdf_rows``):
  pi = softmax(logits), s_k = max(scale_k, 0.11), ctr = round(sum_k pi_k mu_k) clamped to [-2^20, 2^20] (NaN: -2^20);
  L = 2 R + 1 regular symbols j = 0 .. L - 1 for the values offset + j, offset = ctr - R; one tail symbol j = L for everything outside;
  F_j = sum_k pi_k Phi((offset + j - 1/2 - mu_k) / s_k), j = 0 .. L, sent into [0, 1] with a NaN at 0; G_0 = F_0, G_j = max(G_{j-1}, F_j);
  cdf[j] = j + floor((G_j - G_0) S), S = 65535 - L; cdf[L + 1] = 65536.
"""
import numpy as np
import torch
import torch.nn as nn

import ar_ref
from oracle.leaves import (AttentionBlock, LowerBound, ResidualBlock, ResidualBlockUpsample, ResidualBlockWithStride, conv3x3,
                           subpel_conv3x3)

R = 32
L = 2 * R + 1
STRIDE = L + 2
SCALE_BOUND, LIK_BOUND = 0.11, 1e-9
CTR_BOUND, SYM_BOUND = float(1 << 20), float(1 << 24)


def std_cum(x):
    return 0.5 * torch.erfc(-(2 ** -0.5) * x)


def mixture_likelihood(v, scales, means, weights, K, bounds=None):
    """[B, C, H, W] likelihood of v under the mixture; the groups are [B, K C, H, W], component k of channel c at channel k C + c.
    bounds: (LowerBound(0.11), LowerBound(1e-9)) modules (autograd with the LowerBound gradient rule), or None for plain clamps."""
    B, C, H, W = v.shape
    sc, mu, wt = (t.reshape(B, K, C, H, W) for t in (scales, means, weights))
    sc = bounds[0](sc) if bounds else sc.clamp_min(SCALE_BOUND)
    pi = torch.softmax(wt, dim=1)
    d = torch.abs(v.unsqueeze(1) - mu)
    lik = (pi * (std_cum((0.5 - d) / sc) - std_cum((-0.5 - d) / sc))).sum(1)
    return bounds[1](lik) if bounds else lik.clamp_min(LIK_BOUND)


def ar_wavefront_order(H, W):
    """pixels by t = w + 3 h ascending, raster inside a step"""
    return sorted(((h, w) for h in range(H) for w in range(W)), key=lambda p: (p[1] + 3 * p[0], p[0], p[1]))


def _fixed_clamp(v, bound):
    v = torch.where(v >= -bound, v, torch.full_like(v, -bound))   # NaN -> -bound
    return torch.where(v <= bound, v, torch.full_like(v, bound))


def cdf_rows(scales, means, logits, dtype=torch.float64):
    """scales / means / logits [n, K] -> (rows int64 [n, L + 2], offsets int64 [n]) by THE ROW RULE, evaluated in ``dtype``"""
    sc, mu, lg = (t.to(dtype) for t in (scales, means, logits))
    sg = torch.where(sc >= SCALE_BOUND, sc, torch.full_like(sc, SCALE_BOUND))   # fmaxf: a NaN scale is the bound
    pi = torch.softmax(lg, dim=1)
    ctr = _fixed_clamp(torch.round((pi * mu).sum(1)), CTR_BOUND)
    offset = ctr - R
    edges = offset[:, None] + torch.arange(L + 1, dtype=dtype)[None, :] - 0.5                    # [n, L + 1]
    F = (pi[:, None, :] * std_cum((edges[:, :, None] - mu[:, None, :]) / sg[:, None, :])).sum(2)
    F = torch.where(F >= 0, F, torch.zeros_like(F))
    F = torch.where(F <= 1, F, torch.ones_like(F))
    G = torch.cummax(F, dim=1).values
    body = torch.arange(L + 1)[None, :] + torch.floor((G - G[:, :1]) * (65535 - L)).to(torch.int64)
    rows = torch.cat((body, torch.full((body.shape[0], 1), 65536, dtype=torch.int64)), 1)
    return rows, offset.to(torch.int64)


def triple_of(row, offset, sym):
    """(start, freq, esc) of one symbol through its row: what the encoder sends to the coder"""
    v = int(sym) - int(offset)
    if v < 0:
        return int(row[L]), int(row[L + 1] - row[L]), -2 * v - 1
    if v >= L:
        return int(row[L]), int(row[L + 1] - row[L]), 2 * (v - L)
    return int(row[v]), int(row[v + 1] - row[v]), -1


def check_row_structure(rows):
    """the structural properties of THE ROW RULE, exactly; rows integer [n, L + 2]"""
    rows = torch.as_tensor(np.asarray(rows)).to(torch.int64)
    assert rows.shape[1] == L + 2
    assert bool((rows[:, 0] == 0).all()) and bool((rows[:, L + 1] == 65536).all())
    assert bool((rows[:, 1:] - rows[:, :-1] >= 1).all()), "a row is not strictly increasing"


class Cheng2020Anchor(ar_ref.JointAutoregressiveHierarchicalPriors):
    def __init__(self, N=192, K=1):
        super().__init__(N, N)
        self.N, self.K = N, K
        self.g_a, self.g_s = self._build_transforms(N)
        lrelu = lambda: nn.LeakyReLU(inplace=True)
        self.h_a = nn.Sequential(conv3x3(N, N), lrelu(), conv3x3(N, N), lrelu(), conv3x3(N, N, stride=2), lrelu(), conv3x3(N, N), lrelu(),
                                 conv3x3(N, N, stride=2))
        self.h_s = nn.Sequential(conv3x3(N, N), lrelu(), subpel_conv3x3(N, N, 2), lrelu(), conv3x3(N, N * 3 // 2), lrelu(),
                                 subpel_conv3x3(N * 3 // 2, N * 3 // 2, 2), lrelu(), conv3x3(N * 3 // 2, N * 2))
        if K > 1:
            self.entropy_parameters[4] = nn.Conv2d(N * 8 // 3, 3 * K * N, 1)
            self.gaussian_conditional = nn.Module()   # the mixture has no table: no state_dict entries
            self.lower_bound_scale = [LowerBound(SCALE_BOUND)]   # (in lists: not registered, no state_dict entries)
            self.likelihood_lower_bound = [LowerBound(LIK_BOUND)]

    @staticmethod
    def _build_transforms(N):
        RBWS, RBU, RB = ResidualBlockWithStride, ResidualBlockUpsample, ResidualBlock
        g_a = nn.Sequential(RBWS(3, N, 2), RB(N, N), RBWS(N, N, 2), RB(N, N), RBWS(N, N, 2), RB(N, N), conv3x3(N, N, stride=2))
        g_s = nn.Sequential(RB(N, N), RBU(N, N, 2), RB(N, N), RBU(N, N, 2), RB(N, N), RBU(N, N, 2), RB(N, N), subpel_conv3x3(N, 3, 2))
        return g_a, g_s

    def _bounds(self, like):
        for m in (self.lower_bound_scale[0], self.likelihood_lower_bound[0]):
            m.to(dtype=like.dtype, device=like.device)
        return self.lower_bound_scale[0], self.likelihood_lower_bound[0]

    def forward(self, x):
        if self.K == 1:
            return super().forward(x)
        y = self.g_a(x)
        z = self.h_a(y)
        z_hat, z_likelihoods = self.entropy_bottleneck(z)
        params = self.h_s(z_hat)
        if self.training:
            noise = torch.empty_like(y).uniform_(-0.5, 0.5)
            y_hat = y + noise
            v = y + torch.empty_like(y).uniform_(-0.5, 0.5)   # the likelihood draws its own noise, as GaussianConditional.forward does
        else:
            y_hat = torch.round(y)
            v = y_hat
        gp = self.entropy_parameters(torch.cat((params, self.context_prediction(y_hat)), dim=1))
        KN = self.K * self.N
        lik = mixture_likelihood(v, gp[:, :KN], gp[:, KN:2 * KN], gp[:, 2 * KN:], self.K, self._bounds(y))
        return {"x_hat": self.g_s(y_hat), "likelihoods": {"y": lik, "z": z_likelihoods}}

    @torch.no_grad()
    def teacher_forced_params(self, y_hat, params):
        """every pixel's entropy_parameters output in one parallel pass from a finished y_hat -> [B, P, H, W]"""
        return self.entropy_parameters(torch.cat((params, self.context_prediction(y_hat)), dim=1))


class Cheng2020Attention(Cheng2020Anchor):
    @staticmethod
    def _build_transforms(N):
        RBWS, RBU, RB, AB = ResidualBlockWithStride, ResidualBlockUpsample, ResidualBlock, AttentionBlock
        g_a = nn.Sequential(RBWS(3, N, 2), RB(N, N), RBWS(N, N, 2), AB(N), RB(N, N), RBWS(N, N, 2), RB(N, N), conv3x3(N, N, stride=2), AB(N))
        g_s = nn.Sequential(AB(N), RB(N, N), RBU(N, N, 2), RB(N, N), RBU(N, N, 2), AB(N), RB(N, N), RBU(N, N, 2), RB(N, N),
                            subpel_conv3x3(N, 3, 2))
        return g_a, g_s
