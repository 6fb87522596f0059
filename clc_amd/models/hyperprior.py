"""The hyperprior baselines of the RD plot — ``bmshj2018-hyperprior`` (ScaleHyperprior) and ``mbt2018-mean`` (MeanScaleHyperprior) — on
the engine's own kernels: CompressAI's ``conv(k=5, s=2)`` / ``deconv(k=5, s=2)`` layers run on csrc/conv5.hip, GDN / IGDN, the entropy
models, the rANS coder and the RD loss are the ones CLC and TCM use.

Written from CompressAI's published model definitions (layer order, hence the ``nn.Sequential`` indexes and ``state_dict`` keys;
``abs(y)`` into ``h_a`` of the scale-only model; ReLU there, LeakyReLU in the mean-scale model; ``chunk(2, 1)`` into scales and means),
so CompressAI checkpoints load.  CompressAI itself is not a dependency and nothing here is pinned against it: like the leaves, these
models are checked against a plain-torch restatement of the same definitions (tests/hyperprior_ref.py).

They train through plain autograd and code through the model methods; TrainEngine, graphed_training, CodecEngine and ReferenceBank
do not take them.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from .. import ans, ops
from ..entropy_models import EntropyBottleneck, GaussianConditional
from ..layers import GDN, conv, deconv
from ..ops import ACT_LRELU, ACT_NONE, ACT_RELU, CL
from .clc import CompressionModel, _resize_registered_buffers, get_scale_table


class ScaleHyperprior(CompressionModel):
    """Balle et al. 2018, scale hyperprior: y ~ N(0, sigma(z)^2)."""

    _h_act = ACT_RELU

    def __init__(self, N=128, M=192, **kwargs):
        super().__init__(entropy_bottleneck_channels=N)
        self._check_channels(N, M)
        self.g_a = nn.Sequential(conv(3, N), GDN(N), conv(N, N), GDN(N), conv(N, N), GDN(N), conv(N, M))
        self.g_s = nn.Sequential(deconv(M, N), GDN(N, inverse=True), deconv(N, N), GDN(N, inverse=True), deconv(N, N), GDN(N, inverse=True),
                                 deconv(N, 3))
        self._build_hyper(N, M)
        self.gaussian_conditional = GaussianConditional(None)
        self.N, self.M = int(N), int(M)

    @staticmethod
    def _check_channels(N, M):
        if N % 4 or M % 4 or (M * 3 // 2) % 4 or M * 3 % 2:
            raise ValueError(f"hyperprior models need N, M and M*3/2 to be multiples of 4 (the kernels' aligned path); got N={N}, M={M}")

    def _build_hyper(self, N, M):
        self.h_a = nn.Sequential(conv(M, N, stride=1, kernel_size=3), nn.ReLU(inplace=True), conv(N, N), nn.ReLU(inplace=True), conv(N, N))
        self.h_s = nn.Sequential(deconv(N, N), nn.ReLU(inplace=True), deconv(N, N), nn.ReLU(inplace=True),
                                 conv(N, M, stride=1, kernel_size=3), nn.ReLU(inplace=True))

    @property
    def downsampling_factor(self) -> int:
        return 2 ** (4 + 2)

    # ---- the transforms (the activation placeholders of the Sequentials are fused into the producing layer's epilogue) ----
    @staticmethod
    def _prep(x):
        ops._require_gpu(x, "hyperprior")
        if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] % 64 or x.shape[3] % 64:
            raise ValueError(f"hyperprior models take [N, 3, H, W] images with H and W multiples of 64; got {tuple(x.shape)}")
        return x.detach().contiguous(memory_format=CL)   # (the image takes no gradient: the RGB head runs on patch rows)

    def _analysis(self, x):
        t = x
        for m in self.g_a:
            t = m(t)
        return t

    def _synthesis(self, y_hat):
        t = y_hat
        for m in self.g_s:
            t = m(t)
        return t

    def _hyper_analysis(self, y):
        a = self._h_act
        t = self.h_a[0](torch.abs(y), act=a)
        return self.h_a[4](self.h_a[2](t, act=a))

    def _hyper_synthesis(self, z_hat):
        a = self._h_act
        return self.h_s[4](self.h_s[2](self.h_s[0](z_hat, act=a), act=a), act=a)

    def _params(self, z_hat):
        """(scales, means or None) of y from z_hat"""
        return self._hyper_synthesis(z_hat), None

    def forward(self, x):
        x = self._prep(x)
        y = self._analysis(x)
        z = self._hyper_analysis(y)
        z_hat, z_likelihoods = self.entropy_bottleneck(z)
        scales_hat, means_hat = self._params(z_hat)
        y_hat, y_likelihoods = self.gaussian_conditional(y, scales_hat, means=means_hat)
        x_hat = self._synthesis(y_hat)
        return {"x_hat": x_hat, "likelihoods": {"y": y_likelihoods, "z": z_likelihoods}}

    # ---- codec: one y stream and one z stream per image, on the host rANS coder ----
    def _zeros_like(self, t):
        return torch.zeros_like(t, memory_format=CL)

    @torch.no_grad()
    def compress(self, x):
        x = self._prep(x)
        y = self._analysis(x)
        z = self._hyper_analysis(y)
        z_strings = self.entropy_bottleneck.compress(z)
        z_hat = self.entropy_bottleneck.decompress(z_strings, z.size()[-2:])
        scales_hat, means_hat = self._params(z_hat)
        gc = self.gaussian_conditional
        cdf, ln, off = gc.host_tables()
        sym, idx, _ = gc.quantize_and_index(y, means_hat if means_hat is not None else self._zeros_like(y), scales_hat)
        sym = sym.contiguous().cpu().numpy()   # [N, C, H, W]: the element order of CompressAI's symbols[i].reshape(-1)
        idx = idx.contiguous().cpu().numpy()
        y_strings = [ans.encode(sym[i].reshape(-1), idx[i].reshape(-1), cdf, ln, off) for i in range(sym.shape[0])]
        from ..codec import kernel_config

        return {"strings": [y_strings, z_strings], "shape": z.size()[-2:], "kernel_config": kernel_config()}

    @torch.no_grad()
    def decompress(self, strings, shape):
        assert isinstance(strings, (list, tuple)) and len(strings) == 2
        z_hat = self.entropy_bottleneck.decompress(strings[1], shape)
        scales_hat, means_hat = self._params(z_hat)
        gc = self.gaussian_conditional
        cdf, ln, off = gc.host_tables()
        idx = gc.build_indexes(scales_hat).contiguous().cpu().numpy()
        out = np.empty(idx.shape, dtype=np.float32)
        for i, s in enumerate(strings[0]):
            out[i] = ans.decode(s, idx[i].reshape(-1), cdf, ln, off).reshape(idx.shape[1:])
        y_hat = torch.from_numpy(out).to(z_hat.device).contiguous(memory_format=CL)
        if means_hat is not None:
            y_hat = y_hat + means_hat
        return {"x_hat": self._synthesis(y_hat).clamp_(0, 1)}

    def update(self, scale_table=None, force=False):
        if scale_table is None:
            scale_table = get_scale_table()
        updated = self.gaussian_conditional.update_scale_table(scale_table, force=force)
        updated |= self.entropy_bottleneck.update(force=force)
        return updated

    def load_state_dict(self, state_dict, strict=True):
        _resize_registered_buffers(self.gaussian_conditional, "gaussian_conditional",
                                   ["_quantized_cdf", "_offset", "_cdf_length", "scale_table"], state_dict)
        _resize_registered_buffers(self.entropy_bottleneck, "entropy_bottleneck", ["_quantized_cdf", "_offset", "_cdf_length"], state_dict)
        return nn.Module.load_state_dict(self, state_dict, strict=strict)


class MeanScaleHyperprior(ScaleHyperprior):
    """Minnen et al. 2018 without the context model: y ~ N(mu(z), sigma(z)^2)."""

    _h_act = ACT_LRELU

    def _build_hyper(self, N, M):
        self.h_a = nn.Sequential(conv(M, N, stride=1, kernel_size=3), nn.LeakyReLU(inplace=True), conv(N, N), nn.LeakyReLU(inplace=True),
                                 conv(N, N))
        self.h_s = nn.Sequential(deconv(N, M), nn.LeakyReLU(inplace=True), deconv(M, M * 3 // 2), nn.LeakyReLU(inplace=True),
                                 conv(M * 3 // 2, M * 2, stride=1, kernel_size=3))

    def _hyper_analysis(self, y):
        a = self._h_act
        return self.h_a[4](self.h_a[2](self.h_a[0](y, act=a), act=a))

    def _hyper_synthesis(self, z_hat):
        a = self._h_act
        return self.h_s[4](self.h_s[2](self.h_s[0](z_hat, act=a), act=a))

    def _params(self, z_hat):
        scales_hat, means_hat = self._hyper_synthesis(z_hat).chunk(2, 1)
        return scales_hat, means_hat
