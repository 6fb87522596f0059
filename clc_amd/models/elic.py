"""``elic2022`` — ELIC (He et al., "ELIC: Efficient Learned Image Compression with Unevenly Grouped Space-Channel Contextual Adaptive
Coding", CVPR 2022) on the engine's own kernels: the "He (CVPR22)" curve of the RD plot.

The entropy model is the checkerboard model of ``mbt2018-checkerboard`` applied once per CHANNEL GROUP, with uneven groups
(16, 16, 32, 64, M - 128 channels): group k is coded in two parallel passes — its anchors ((h + w) odd) from the hyperprior and a 5x5
net over every earlier group, its non-anchors additionally from a checkerboard convolution over the group's own anchors.  Encoder and
decoder are both 2 K parallel passes, whatever the image size.

Written from the paper: the transforms (residual bottleneck blocks and attention, no GDN), the group sizes, the three per-group nets
and their widths.  The module names, hence the ``state_dict`` keys, and the stream order are the project's own; no other
implementation is a dependency and nothing here is pinned against one.  Like the other baselines the model is checked against a
plain-torch restatement of the same definitions (tests/scctx_ref.py).

Kernels.  forward trains through plain autograd on the full-map kernels (conv5.hip, ckbd_context.hip, the 1x1 / 3x3 families).  The
coder runs the per-pass 1x1 "parameter aggregation" nets on clc_row_gemm (csrc/row_gemm.hip: f32 MFMAs, a summation order fixed by the
channel counts of its K ranges alone), the channel-context nets on the 5x5 kernels, the spatial context on ckbd_conv_kernel, h_s on the
batch-invariant routes ``mbt2018-mean`` codes with: a stream written at batch 8 decodes at batch 1.

STREAM ORDER: one rANS stream per image for y — for k ascending, group k's anchors in raster order, then its non-anchors in raster
order, channels inner; z as in the other hyperprior models.

TrainEngine, graphed_training, CodecEngine and ReferenceBank do not take this model.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from .. import ans, ops
from ..entropy_models import GaussianConditional
from ..layers import AttentionBlock, CheckerboardMaskedConv2d, Conv2d, conv, conv1x1, conv3x3, deconv
from ..ops import ACT_NONE, ACT_RELU, CL
from .clc import CompressionModel, _resize_registered_buffers, get_scale_table
from .hyperprior import ckbd_pixels


def scctx_order(H, W, groups):
    """The stream's order as (raster position h * W + w, channel) pairs: groups ascending, inside a group the anchors in raster order and
    then the non-anchors in raster order, channels inner.  -> int64 [H * W * sum(groups), 2]"""
    anchors, others = ckbd_pixels(H, W)
    pos = np.array([h * W + w for h, w in anchors + others], dtype=np.int64)
    out, s = [], 0
    for c in groups:
        ch = np.arange(s, s + int(c), dtype=np.int64)
        out.append(np.stack((np.repeat(pos, len(ch)), np.tile(ch, len(pos))), axis=1))
        s += int(c)
    return np.concatenate(out, axis=0)


class ResidualBottleneck(nn.Module):
    """x + conv1x1(C/2 -> C)(relu(conv3x3(relu(conv1x1(C -> C/2)(x))))): ResidualUnit without the trailing ReLU, on the same epilogues
    (the ReLUs in the producing layers' stores, the identity in the last layer's)."""

    def __init__(self, C):
        super().__init__()
        self.conv = nn.Sequential(conv1x1(C, C // 2), nn.ReLU(inplace=True), conv3x3(C // 2, C // 2), nn.ReLU(inplace=True), conv1x1(C // 2, C))

    def forward(self, x):
        g0, g1 = ops.ActGate(), ops.ActGate()   # each ReLU' rides in the NEXT layer's data-gradient epilogue
        t = self.conv[0](x, act=ACT_RELU, gate_out=g0)
        t = self.conv[2](t, act=ACT_RELU, gate_in=g0, gate_out=g1)
        return self.conv[4](t, res=x, gate_in=g1)


def _run(seq, x):
    """a Sequential of layers whose ReLU placeholders are fused into the producing layer's epilogue"""
    mods = list(seq)
    i = 0
    while i < len(mods):
        if i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU):
            x = mods[i](x, act=ACT_RELU)
            i += 2
        else:
            x = mods[i](x)
            i += 1
    return x


class Elic2022(CompressionModel):
    """ELIC, written from the paper (He et al., CVPR 2022); nothing is pinned against any other implementation.  See the module
    docstring for the kernels and the stream order."""

    def __init__(self, N=192, M=320, groups=(16, 16, 32, 64, 192), ch_widths=(224, 128), agg_widths=(640, 512), **kwargs):
        super().__init__(entropy_bottleneck_channels=N)
        groups, ch_widths, agg_widths = tuple(int(c) for c in groups), tuple(int(c) for c in ch_widths), tuple(int(c) for c in agg_widths)
        if len(groups) < 1 or sum(groups) != M:
            raise ValueError(f"Elic2022: sum(groups) must equal M (got groups={groups}, sum {sum(groups)}, M={M})")
        if len(ch_widths) != 2 or len(agg_widths) != 2:
            raise ValueError(f"Elic2022: ch_widths and agg_widths take two widths each (got {ch_widths}, {agg_widths})")
        named = [("N", N), ("N//2", N // 2), ("N*3//2", N * 3 // 2)] + [(f"groups[{i}]", c) for i, c in enumerate(groups)] + \
                [(f"ch_widths[{i}]", c) for i, c in enumerate(ch_widths)] + [(f"agg_widths[{i}]", c) for i, c in enumerate(agg_widths)]
        for name, v in named:
            if v < 4 or v % 4:
                raise ValueError(f"Elic2022: {name} must be a positive multiple of 4 (the kernels' aligned path); got {name} = {v}")
        if (M // 2) % 4:
            raise ValueError(f"Elic2022: M//2 must be a multiple of 4 (the attention blocks' bottleneck); got M = {M}")
        self.N, self.M, self.groups = int(N), int(M), groups
        self.starts = tuple(int(s) for s in np.cumsum((0,) + groups[:-1]))
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
        self.channel_context = nn.ModuleList(
            nn.Sequential() if k == 0 else nn.Sequential(Conv2d(s, c0, 5), nn.ReLU(inplace=True), Conv2d(c0, c1, 5), nn.ReLU(inplace=True),
                                                         Conv2d(c1, 2 * c, 5))
            for k, (s, c) in enumerate(zip(self.starts, groups)))
        self.spatial_context = nn.ModuleList(CheckerboardMaskedConv2d(c, 2 * c, kernel_size=5, padding=2, stride=1) for c in groups)
        self.aggregation = nn.ModuleList(
            nn.Sequential(Conv2d(2 * M + 2 * c + (2 * c if k else 0), a0, 1), nn.ReLU(inplace=True), Conv2d(a0, a1, 1), nn.ReLU(inplace=True),
                          Conv2d(a1, 2 * c, 1))
            for k, c in enumerate(groups))
        self.gaussian_conditional = GaussianConditional(None)

    @property
    def downsampling_factor(self) -> int:
        return 2 ** (4 + 2)

    @staticmethod
    def _prep(x):
        ops._require_gpu(x, "elic2022")
        if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] % 64 or x.shape[3] % 64:
            raise ValueError(f"Elic2022 takes [N, 3, H, W] images with H and W multiples of 64; got {tuple(x.shape)}")
        return x.detach().contiguous(memory_format=CL)   # (the image takes no gradient: the RGB head runs on patch rows)

    def _analysis(self, x):
        return _run(self.g_a, x)

    def _synthesis(self, y_hat):
        return _run(self.g_s, y_hat)

    def _hyper_analysis(self, y):
        return _run(self.h_a, y)

    def _hyper_synthesis(self, z_hat):
        return _run(self.h_s, z_hat)

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
        scales, means = [], []
        for k, (s, c) in enumerate(zip(self.starts, self.groups)):
            # one pass per group: spatial_context reads the group's anchors only and returns 0 at anchors, so this teacher-forced pass
            # equals the coder's two
            parts = [params, self.spatial_context[k](y_hat[:, s:s + c])]
            if k:
                parts.append(_run(self.channel_context[k], y_hat[:, :s]))
            sc, mu = _run(self.aggregation[k], torch.cat(parts, 1)).chunk(2, 1)
            scales.append(sc)
            means.append(mu)
        _, y_likelihoods = self.gaussian_conditional(y, torch.cat(scales, 1), means=torch.cat(means, 1))
        x_hat = self._synthesis(y_hat)
        return {"x_hat": x_hat, "likelihoods": {"y": y_likelihoods, "z": z_likelihoods}}

    # ---- the 2 K-pass coder ----
    def _scctx_filters(self):
        """per group the [(filter [N, K] row-major, bias)] of the three aggregation layers"""
        out = []
        for agg in self.aggregation:
            f = []
            for i in (0, 2, 4):
                w = agg[i].weight.detach()
                f.append((w.reshape(w.shape[0], w.shape[1]).contiguous(), agg[i].bias.detach().contiguous()))
            out.append(f)
        return out

    def _scctx_workspace(self, rows, dev):
        mk = lambda c: torch.empty((rows, c), device=dev, dtype=torch.float32)
        a0, a1 = self.aggregation[0][0].out_channels, self.aggregation[0][2].out_channels
        return {"h1": mk(a0), "h2": mk(a1), "gp": mk(2 * max(self.groups))}

    @staticmethod
    def _scctx_lists(H, W, dev):
        """(number of anchors, number of non-anchors, the uploaded pixel list: anchors first)"""
        anchors, others = ckbd_pixels(H, W)
        return len(anchors), len(others), torch.tensor(anchors + others, dtype=torch.int32).reshape(-1, 2).to(dev)

    def _scctx_chain(self, px, B, H, W, params, sp, ch, ws, filt):
        """(scales | means) of one group at the listed pixels of every image -> the first 2 c columns of ws["gp"]; three launches.  The K
        ranges are (hyper parameters, spatial context, channel context): pass A feeds an all-zero spatial map rather than dropping the
        range, so both passes share one filter image and one K order."""
        srcs = [("pixel", params), ("pixel", sp)] + ([("pixel", ch)] if ch is not None else [])
        ops.row_gemm(srcs, px, B, H, W, filt[0][0], filt[0][1], ws["h1"], act=ACT_RELU)
        ops.row_gemm([("dense", ws["h1"])], px, B, H, W, filt[1][0], filt[1][1], ws["h2"], act=ACT_RELU)
        ops.row_gemm([("dense", ws["h2"])], px, B, H, W, filt[2][0], filt[2][1], ws["gp"], act=ACT_NONE)

    def _channel_ctx(self, k, y_hat):
        return _run(self.channel_context[k], y_hat[:, :self.starts[k]]).contiguous(memory_format=CL) if k else None

    @torch.no_grad()
    def _scctx_encode(self, y, params):
        """The 2 K passes of compress -> (per group symbols int32 [B, H*W, c_k], per group indexes int32 [B, H*W, c_k], y_hat), the buffers
        in raster order: all launches on the current stream, no host sync."""
        ops._require_gpu(y, "elic2022 compress")
        B, M, H, W = y.shape
        y = y.contiguous(memory_format=CL)
        params = params.contiguous(memory_format=CL)
        dev = y.device
        na, nn_, pix = self._scctx_lists(H, W, dev)
        ws = self._scctx_workspace(B * max(na, nn_), dev)
        filt = self._scctx_filters()
        table = self.gaussian_conditional.scale_table
        y_hat = torch.zeros_like(y, memory_format=CL)
        syms, idxs = [], []
        for k, (s, c) in enumerate(zip(self.starts, self.groups)):
            sym = torch.empty((B, H * W, c), device=dev, dtype=torch.int32)
            idx = torch.empty((B, H * W, c), device=dev, dtype=torch.int32)
            yk, yhk = y[:, s:s + c], y_hat[:, s:s + c]
            ch = self._channel_ctx(k, y_hat)
            if na:
                zero_sp = torch.zeros((B, 2 * c, H, W), device=dev, dtype=torch.float32).contiguous(memory_format=CL)
                self._scctx_chain(pix[:na], B, H, W, params, zero_sp, ch, ws, filt[k])
                ops.ar_finish_encode(ws["gp"], c, pix[:na], yk, yhk, table, sym, idx)
            sp = self.spatial_context[k](yhk)
            self._scctx_chain(pix[na:], B, H, W, params, sp, ch, ws, filt[k])
            ops.ar_finish_encode(ws["gp"], c, pix[na:], yk, yhk, table, sym, idx)
            syms.append(sym)
            idxs.append(idx)
        return syms, idxs, y_hat

    @torch.no_grad()
    def _code_inputs(self, x):
        """(y, hyper parameters from the coded z, z streams, z's map size): what the passes start from"""
        x = self._prep(x)
        y = self._analysis(x)
        z = self._hyper_analysis(y)
        z_strings = self.entropy_bottleneck.compress(z)
        z_hat = self.entropy_bottleneck.decompress(z_strings, z.size()[-2:])
        return y, self._hyper_synthesis(z_hat), z_strings, z.size()[-2:]

    @torch.no_grad()
    def compress(self, x):
        y, params, z_strings, z_size = self._code_inputs(x)
        cdf, ln, off = self.gaussian_conditional.host_tables()
        syms, idxs, _ = self._scctx_encode(y, params)
        B, _, H, W = y.shape
        na, nn_, pix = self._scctx_lists(H, W, y.device)
        order = (pix[:, 0].long() * W + pix[:, 1].long())   # raster positions in the stream's pixel order: anchors, then non-anchors
        flat = lambda ts: torch.cat([t.index_select(1, order).reshape(B, -1) for t in ts], 1)
        both = torch.stack((flat(syms), flat(idxs))).cpu().numpy()   # the one device -> host copy: [2, B, H*W*M] in stream order
        y_strings = [ans.encode(np.ascontiguousarray(both[0, i]), np.ascontiguousarray(both[1, i]), cdf, ln, off) for i in range(B)]
        from ..codec import kernel_config

        return {"strings": [y_strings, z_strings], "shape": z_size, "kernel_config": kernel_config()}

    @torch.no_grad()
    def _scctx_decode(self, y_strings, params):
        """The 2 K passes of decompress -> y_hat: per pass one index download, one incremental decode per image, one symbol upload."""
        params = params.contiguous(memory_format=CL)
        dev = params.device
        B, M, (H, W) = params.shape[0], self.M, params.shape[2:]
        if len(y_strings) != B:
            raise ValueError(f"decompress: {len(y_strings)} y streams for {B} z streams")
        cdf, ln, off = self.gaussian_conditional.host_tables()
        table = self.gaussian_conditional.scale_table
        na, nn_, pix = self._scctx_lists(H, W, dev)
        rows = B * max(na, nn_)
        ws = self._scctx_workspace(rows, dev)
        filt = self._scctx_filters()
        y_hat = torch.zeros((B, M, H, W), device=dev, dtype=torch.float32).contiguous(memory_format=CL)
        decoders = []
        for s in y_strings:
            d = ans.RansDecoder()
            d.set_stream(s)
            decoders.append(d)
        cmax = max(self.groups)
        idx_host = torch.empty((rows * cmax,), dtype=torch.int32).pin_memory()
        sym_host = torch.empty((rows * cmax,), dtype=torch.int32).pin_memory()
        stream = torch.cuda.current_stream(dev)
        for k, (s, c) in enumerate(zip(self.starts, self.groups)):
            yhk = y_hat[:, s:s + c]
            ch = self._channel_ctx(k, y_hat)
            sp = torch.zeros((B, 2 * c, H, W), device=dev, dtype=torch.float32).contiguous(memory_format=CL)
            for lo, cnt in ((0, na), (na, nn_)):
                if not cnt:
                    continue
                px = pix[lo:lo + cnt]
                if lo:
                    sp = self.spatial_context[k](yhk)
                n = B * cnt
                idx_dev = torch.empty((n, c), device=dev, dtype=torch.int32)
                sym_dev = torch.empty((n, c), device=dev, dtype=torch.int32)
                ih, sh = idx_host[:n * c].view(n, c), sym_host[:n * c].view(n, c)
                idx_np, sym_np = ih.numpy(), sh.numpy()
                self._scctx_chain(px, B, H, W, params, sp, ch, ws, filt[k])
                ops.ar_finish_decode(ws["gp"], c, px, B, H, W, table, idx_dev)
                ih.copy_(idx_dev, non_blocking=True)
                stream.synchronize()   # (also: the previous pass's symbol upload has left sym_host)
                for b, d in enumerate(decoders):   # rows b * cnt .. of the pass are image b's pixels in list order, channels inner
                    sym_np[b * cnt:(b + 1) * cnt] = d.decode_stream(idx_np[b * cnt:(b + 1) * cnt].reshape(-1), cdf, ln, off).reshape(cnt, c)
                sym_dev.copy_(sh, non_blocking=True)
                ops.ar_commit(sym_dev, ws["gp"], c, px, yhk)
        return y_hat

    @torch.no_grad()
    def decompress(self, strings, shape):
        assert isinstance(strings, (list, tuple)) and len(strings) == 2
        z_hat = self.entropy_bottleneck.decompress(strings[1], shape)
        y_hat = self._scctx_decode(strings[0], self._hyper_synthesis(z_hat))
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
