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
from ..layers import GDN, Conv2d, MaskedConv2d, conv, deconv
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


def ar_schedule(H, W, order="wavefront"):
    """The steps of the autoregressive pass over an H x W latent, each a list of (h, w).  Under mask A pixel (h, w) reads rows h - 2 and
    h - 1 at columns w - 2 .. w + 2 and row h at columns w - 2 and w - 1, so all pixels of equal t = w + 3 h are independent:
    ``"wavefront"`` returns the W + 3 (H - 1) steps t = 0, 1, ... (for W < 3 some are empty), ``"raster"`` one pixel per step."""
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError(f"ar_schedule: H and W must be positive (got {H}, {W})")
    if order == "raster":
        return [[(h, w)] for h in range(H) for w in range(W)]
    if order != "wavefront":
        raise ValueError(f"ar_schedule: order must be 'wavefront' or 'raster' (got {order!r})")
    steps = [[] for _ in range(W + 3 * (H - 1))]
    for h in range(H):
        for w in range(W):
            steps[w + 3 * h].append((h, w))
    return steps


class JointAutoregressiveHierarchicalPriors(MeanScaleHyperprior):
    """Minnen et al. 2018 with the context model (``mbt2018``): the mean-scale hyperprior plus a masked 5x5 convolution over the coded
    latent and a three-layer 1x1 ``entropy_parameters`` net on cat((hyper parameters, context)).

    forward runs the full-map kernels.  The coder is sequential in the latent: per pixel, gather the 12 live taps -> M -> 2M -> (with the
    pixel's hyper parameters) 4M -> 10M/3 -> 8M/3 -> 2M -> quantise / index, on the row kernels of csrc/ar_context.hip, whose summation
    order depends on K alone — an encoder step of many pixels and a decoder step of one give the same bits.  compress runs the
    wavefront schedule (W + 3 (H - 1) steps) and serialises in CompressAI's raster-pixel, channel-inner order; decompress must follow the
    stream, one raster pixel at a time for the whole batch."""

    def __init__(self, N=192, M=192, **kwargs):
        if M % 12:
            raise ValueError(f"JointAutoregressiveHierarchicalPriors needs M % 12 == 0 (then 10M/3, 8M/3 and 3M/2 are whole and multiples of 4, the "
                             f"kernels' aligned path); got M = {M}" + (": M = 320 (mbt2018 qualities 5-8) is not built" if M == 320 else ""))
        super().__init__(N=N, M=M, **kwargs)
        self.entropy_parameters = nn.Sequential(Conv2d(M * 4, M * 10 // 3, 1), nn.LeakyReLU(inplace=True),
                                                Conv2d(M * 10 // 3, M * 8 // 3, 1), nn.LeakyReLU(inplace=True),
                                                Conv2d(M * 8 // 3, M * 2, 1))
        self.context_prediction = MaskedConv2d(M, 2 * M, kernel_size=5, padding=2, stride=1)

    def _entropy_parameters(self, t):
        ep = self.entropy_parameters
        return ep[4](ep[2](ep[0](t, act=ACT_LRELU), act=ACT_LRELU))

    def forward(self, x):
        x = self._prep(x)
        y = self._analysis(x)
        z = self._hyper_analysis(y)
        z_hat, z_likelihoods = self.entropy_bottleneck(z)
        params = self._hyper_synthesis(z_hat)
        # quantize(y, "noise" if training else "dequantize"): no means here — the context model must see what a decoder can know
        if self.training:
            y_hat = y + torch.empty_like(y, memory_format=CL).uniform_(-0.5, 0.5)
        else:
            y_hat = torch.round(y.detach())
        ctx_params = self.context_prediction(y_hat)
        gaussian_params = self._entropy_parameters(torch.cat((params, ctx_params), 1))
        scales_hat, means_hat = gaussian_params.chunk(2, 1)
        _, y_likelihoods = self.gaussian_conditional(y, scales_hat, means=means_hat)
        x_hat = self._synthesis(y_hat)
        return {"x_hat": x_hat, "likelihoods": {"y": y_likelihoods, "z": z_likelihoods}}

    # ---- the sequential coder ----
    def _ar_filters(self):
        """[(filter [N, K] row-major, bias)] of the four layers of the chain.  The context layer's is the masked parameter's 12 live taps,
        [2M][12][M]: the first 12 of the 25 (kh, kw) positions of the channels-last parameter."""
        M = self.M
        cp, ep = self.context_prediction, self.entropy_parameters
        wc = cp.weight.detach().permute(0, 2, 3, 1).reshape(2 * M, 25, M)[:, :12].reshape(2 * M, 12 * M).contiguous()
        out = [(wc, cp.bias.detach().contiguous())]
        for i in (0, 2, 4):
            w = ep[i].weight.detach()
            out.append((w.reshape(w.shape[0], w.shape[1]).contiguous(), ep[i].bias.detach().contiguous()))
        return out

    def _ar_workspace(self, rows, dev):
        M = self.M
        mk = lambda c: torch.empty((rows, c), device=dev, dtype=torch.float32)
        return {"ctx": mk(2 * M), "h1": mk(M * 10 // 3), "h2": mk(M * 8 // 3), "gp": mk(2 * M)}

    def _ar_chain(self, px, B, H, W, y_hat, params, ws, filt):
        """(scales | means) of the listed pixels of every image -> ws["gp"]; four launches"""
        ops.ar_linear([("taps", y_hat)], px, B, H, W, filt[0][0], filt[0][1], ws["ctx"])
        ops.ar_linear([("pixel", params), ("dense", ws["ctx"])], px, B, H, W, filt[1][0], filt[1][1], ws["h1"], act=ACT_LRELU)
        ops.ar_linear([("dense", ws["h1"])], px, B, H, W, filt[2][0], filt[2][1], ws["h2"], act=ACT_LRELU)
        ops.ar_linear([("dense", ws["h2"])], px, B, H, W, filt[3][0], filt[3][1], ws["gp"])

    @staticmethod
    def _ar_pixels(steps, dev):
        steps = [s for s in steps if s]
        return steps, torch.tensor([p for s in steps for p in s], dtype=torch.int32).reshape(-1, 2).to(dev)

    @torch.no_grad()
    def _ar_encode(self, y, params, order="wavefront"):
        """The autoregressive pass of compress -> (symbols int32 [B, H*W, M], indexes int32 [B, H*W, M], y_hat): all launches on the current
        stream, no host sync.  The schedule decides the order of computation only; the buffers are in raster order either way."""
        ops._require_gpu(y, "mbt2018 compress")
        B, M, H, W = y.shape
        y = y.contiguous(memory_format=CL)
        params = params.contiguous(memory_format=CL)
        steps, pix = self._ar_pixels(ar_schedule(H, W, order), y.device)
        ws = self._ar_workspace(B * max(len(s) for s in steps), y.device)
        filt = self._ar_filters()
        table = self.gaussian_conditional.scale_table
        y_hat = torch.zeros_like(y, memory_format=CL)
        sym = torch.empty((B, H * W, M), device=y.device, dtype=torch.int32)
        idx = torch.empty((B, H * W, M), device=y.device, dtype=torch.int32)
        off = 0
        for s in steps:
            px = pix[off:off + len(s)]
            self._ar_chain(px, B, H, W, y_hat, params, ws, filt)
            ops.ar_finish_encode(ws["gp"], M, px, y, y_hat, table, sym, idx)
            off += len(s)
        return sym, idx, y_hat

    @torch.no_grad()
    def _code_inputs(self, x):
        """(y, hyper parameters from the coded z, z streams, z's map size): what the autoregressive pass starts from"""
        x = self._prep(x)
        y = self._analysis(x)
        z = self._hyper_analysis(y)
        z_strings = self.entropy_bottleneck.compress(z)
        z_hat = self.entropy_bottleneck.decompress(z_strings, z.size()[-2:])
        return y, self._hyper_synthesis(z_hat), z_strings, z.size()[-2:]

    @torch.no_grad()
    def compress(self, x, order="wavefront"):
        y, params, z_strings, z_size = self._code_inputs(x)
        cdf, ln, off = self.gaussian_conditional.host_tables()
        sym, idx, _ = self._ar_encode(y, params, order)
        both = torch.stack((sym, idx)).cpu().numpy()   # the one device -> host copy: [2, B, H*W, M], raster pixels, channels inner
        y_strings = [ans.encode(both[0, i].reshape(-1), both[1, i].reshape(-1), cdf, ln, off) for i in range(both.shape[1])]
        from ..codec import kernel_config

        return {"strings": [y_strings, z_strings], "shape": z_size, "kernel_config": kernel_config()}

    @torch.no_grad()
    def decompress(self, strings, shape):
        assert isinstance(strings, (list, tuple)) and len(strings) == 2
        z_hat = self.entropy_bottleneck.decompress(strings[1], shape)
        params = self._hyper_synthesis(z_hat).contiguous(memory_format=CL)
        dev = params.device
        B, M, (H, W) = params.shape[0], self.M, params.shape[2:]
        if len(strings[0]) != B:
            raise ValueError(f"decompress: {len(strings[0])} y streams for {B} z streams")
        cdf, ln, off = self.gaussian_conditional.host_tables()
        table = self.gaussian_conditional.scale_table
        steps, pix = self._ar_pixels(ar_schedule(H, W, "raster"), dev)
        ws = self._ar_workspace(B, dev)
        filt = self._ar_filters()
        y_hat = torch.zeros((B, M, H, W), device=dev, dtype=torch.float32).contiguous(memory_format=CL)
        decoders = []
        for s in strings[0]:
            d = ans.RansDecoder()
            d.set_stream(s)
            decoders.append(d)
        idx_dev = torch.empty((B, M), device=dev, dtype=torch.int32)
        sym_dev = torch.empty((B, M), device=dev, dtype=torch.int32)
        idx_host = torch.empty((B, M), dtype=torch.int32).pin_memory()
        sym_host = torch.empty((B, M), dtype=torch.int32).pin_memory()
        idx_np, sym_np = idx_host.numpy(), sym_host.numpy()
        stream = torch.cuda.current_stream(dev)
        for i in range(len(steps)):
            px = pix[i:i + 1]
            self._ar_chain(px, B, H, W, y_hat, params, ws, filt)
            ops.ar_finish_decode(ws["gp"], M, px, B, H, W, table, idx_dev)
            idx_host.copy_(idx_dev, non_blocking=True)
            stream.synchronize()   # (also: the previous pixel's symbol upload has left sym_host)
            for b, d in enumerate(decoders):
                sym_np[b] = d.decode_stream(idx_np[b], cdf, ln, off)
            sym_dev.copy_(sym_host, non_blocking=True)
            ops.ar_commit(sym_dev, ws["gp"], M, px, y_hat)
        return {"x_hat": self._synthesis(y_hat).clamp_(0, 1)}
