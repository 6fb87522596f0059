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

TrainEngine, graphed_training, CodecEngine, ContextCodecEngine and ReferenceBank do not take this model.  Owners: the schedule of the 2 K passes is
_scctx_passes, for encoder and decoder; the decoder's loop is _scctx_decode_from, over a source of symbols.  The host side of the
coder is coding.py's: the start of the decoder's loop, the sources (a hop to the host's one-stream or lanes decoder,
the device's lanes decoder on one upload image), and the lanes strings — count, parser, refusal, assembly, end-state check.
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
from .coding import (CodeInputs, DeviceLanesSymbols, HostSymbols, coded_item, decoder_start, lanes_check, lanes_count, lanes_parse,
                     lanes_strings, linear_filters, open_decoders, refuse_lanes_strings)
from .hyperprior import ckbd_lists, ckbd_pixels


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


class Elic2022(CodeInputs, CompressionModel):
    """ELIC, written from the paper (He et al., CVPR 2022); nothing is pinned against any other implementation.  See the module
    docstring for the kernels and the stream order."""

    def __init__(self, N=192, M=320, groups=(16, 16, 32, 64, 192), ch_widths=(224, 128), agg_widths=(640, 512), **kwargs):
        from ..intnet import refuse_integer_hyper
        from ..vbr import refuse_rate_levels

        refuse_rate_levels("Elic2022", kwargs)
        refuse_integer_hyper("Elic2022", kwargs)
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
        return [linear_filters(agg) for agg in self.aggregation]

    def _scctx_workspace(self, rows, dev):
        mk = lambda c: torch.empty((rows, c), device=dev, dtype=torch.float32)
        a0, a1 = self.aggregation[0][0].out_channels, self.aggregation[0][2].out_channels
        return {"h1": mk(a0), "h2": mk(a1), "gp": mk(2 * max(self.groups))}

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

    def _scctx_passes(self, params, y_hat):
        """THE SCHEDULE, for encoder and decoder alike: groups ascending x (anchors, non-anchors); an empty pass is skipped.  The channel
        context of group k is computed once, over the groups before it; pass A reads a zero spatial map, pass B the spatial context of
        the anchors that pass A committed.  Per pass the chain, then (group, its pixel list, the group's channels of y_hat, its
        (scales | means) rows) to the caller's body, which finishes the pass into y_hat before the next one reads it."""
        B, _, H, W = y_hat.shape
        na, nn_, pix = ckbd_lists(H, W, y_hat.device)
        ws, filt = self._scctx_workspace(B * max(na, nn_), y_hat.device), self._scctx_filters()
        for k, (s, c) in enumerate(zip(self.starts, self.groups)):
            yhk = y_hat[:, s:s + c]
            ch = self._channel_ctx(k, y_hat)
            for lo, cnt in ((0, na), (na, nn_)):
                if not cnt:
                    continue
                if lo:
                    sp = self.spatial_context[k](yhk)
                else:
                    sp = torch.zeros((B, 2 * c, H, W), device=y_hat.device, dtype=torch.float32).contiguous(memory_format=CL)
                px = pix[lo:lo + cnt]
                self._scctx_chain(px, B, H, W, params, sp, ch, ws, filt[k])
                yield k, px, yhk, ws["gp"]

    @torch.no_grad()
    def _scctx_encode(self, y, params):
        """The 2 K passes of compress -> (per group symbols int32 [B, H*W, c_k], per group indexes int32 [B, H*W, c_k], y_hat), the buffers
        in raster order: all launches on the current stream, no host sync."""
        ops._require_gpu(y, "elic2022 compress")
        B, M, H, W = y.shape
        y = y.contiguous(memory_format=CL)
        params = params.contiguous(memory_format=CL)
        table = self.gaussian_conditional.scale_table
        y_hat = torch.zeros_like(y, memory_format=CL)
        yks = [y[:, s:s + c] for s, c in zip(self.starts, self.groups)]
        syms = [torch.empty((B, H * W, c), device=y.device, dtype=torch.int32) for c in self.groups]
        idxs = [torch.empty((B, H * W, c), device=y.device, dtype=torch.int32) for c in self.groups]
        for k, px, yhk, gp in self._scctx_passes(params, y_hat):
            ops.ar_finish_encode(gp, self.groups[k], px, yks[k], yhk, table, syms[k], idxs[k])
        return syms, idxs, y_hat

    def _lanes_segments(self, H, W):
        """the lanes stream's segments: the 2 K passes in scctx_order, n = pixels of the pass x channels of the group"""
        anchors, others = ckbd_pixels(H, W)
        return [cnt * c for c in self.groups for cnt in (len(anchors), len(others))]

    def _lanes_encode_device(self, sym, idx, segments, W):
        """int32 [B, T] device symbols / indexes in stream order -> per image its lanes string: one clc_rans_lanes_encode for the batch,
        then two device -> host copies (the [B, W] results, the packed words); the host half is coding.lanes_strings, which raises by
        name on a negative code."""
        gc = self.gaussian_conditional
        out, _, result = ops.rans_lanes_encode(sym, idx, segments, W, (gc._quantized_cdf, gc._cdf_length, gc._offset))
        res = result.cpu().numpy()   # [B, W, 2]: (first word, word count), or (a negative code, 0)
        words = torch.cat([out[f:f + n] for f, n in res.reshape(-1, 2)]).cpu().numpy()   # (a code's span is empty)
        header = np.append(np.where(res[..., 0] < 0, res[..., 0], res[..., 1]).reshape(-1), res[..., 1].sum())
        return lanes_strings(header, words, res.shape[0], W)

    @torch.no_grad()
    def compress(self, x, lanes=None):
        """lanes=None: the one-stream format.  lanes=W: THE LANES STREAM (clc_amd/ans.py: lanes_pack; include/clc_hip.h), W wave streams
        of 64 rANS lanes per image, encoded on the device, and "lanes": W in the result; pass the same W to decompress."""
        Wn = lanes_count(lanes, "Elic2022.compress")
        y, params, z_strings, z_size = self._code_inputs(x)
        if Wn is None:
            cdf, ln, off = self.gaussian_conditional.host_tables()
        syms, idxs, _ = self._scctx_encode(y, params)
        B, _, H, W = y.shape
        na, nn_, pix = ckbd_lists(H, W, y.device)
        order = (pix[:, 0].long() * W + pix[:, 1].long())   # raster positions in the stream's pixel order: anchors, then non-anchors
        flat = lambda ts: torch.cat([t.index_select(1, order).reshape(B, -1) for t in ts], 1)
        if Wn is not None:   # the flat buffers stay on the device
            y_strings = self._lanes_encode_device(flat(syms), flat(idxs), self._lanes_segments(H, W), Wn)
            return coded_item(y_strings, z_strings, z_size, lanes=Wn)
        both = torch.stack((flat(syms), flat(idxs))).cpu().numpy()   # the one device -> host copy: [2, B, H*W*M] in stream order
        y_strings = [ans.encode(np.ascontiguousarray(both[0, i]), np.ascontiguousarray(both[1, i]), cdf, ln, off) for i in range(B)]
        return coded_item(y_strings, z_strings, z_size)

    def _scctx_decode_from(self, source, params, y_hat):
        """The 2 K passes of decompress over a source of symbols (coding.HostSymbols, coding.DeviceLanesSymbols): per non-empty pass
        the chain, ar_finish_decode, the source's step and ar_commit."""
        B, _, H, W = y_hat.shape
        table = self.gaussian_conditional.scale_table
        for k, px, yhk, gp in self._scctx_passes(params, y_hat):
            c, cnt = self.groups[k], px.shape[0]
            idx, sym = source.views(B * cnt, c)
            ops.ar_finish_decode(gp, c, px, B, H, W, table, idx)
            source.decode(idx, sym, cnt * c)
            ops.ar_commit(sym, gp, c, px, yhk)
        return y_hat

    def _scctx_most(self, y_hat):
        """the elements of the largest pass: the non-anchors ((0, 0) is one) of the widest group"""
        return y_hat.shape[0] * ((y_hat.shape[2] * y_hat.shape[3] + 1) // 2) * max(self.groups)

    @torch.no_grad()
    def _scctx_decode(self, y_strings, params):
        """The 2 K passes of decompress -> y_hat: per pass one index download, one incremental decode per image, one symbol upload."""
        params, y_hat = decoder_start(params, len(y_strings), self.M)
        fns = [d.decode_stream for d in open_decoders(y_strings)]
        source = HostSymbols(fns, self.gaussian_conditional.host_tables(), self._scctx_most(y_hat), y_hat.device)
        return self._scctx_decode_from(source, params, y_hat)

    @torch.no_grad()
    def _scctx_decode_lanes(self, subs, params, device_coder=True):
        """The 2 K passes over lanes streams (subs[b][w]: bytes) -> (y_hat, state).
        device_coder: one pinned upload of every wave stream's states, spans and words, then per non-empty pass the chain,
        ar_finish_decode, one clc_rans_lanes_decode_step and ar_commit — stream-ordered launches only, no download, no synchronize, no
        per-image loop; state is the device's int32 [B, W, 130] (64 x (x low, x high), pos, pad) as the last pass left it.
        Host coder: the hop per pass of _scctx_decode with one ans.LanesDecoder per image; state is the list of decoders."""
        params, y_hat = decoder_start(params, len(subs), self.M)
        gc, most = self.gaussian_conditional, self._scctx_most(y_hat)
        if device_coder:
            source = DeviceLanesSymbols(subs, (gc._quantized_cdf, gc._cdf_length, gc._offset), most, y_hat.device)
        else:
            decoders = [ans.LanesDecoder(img) for img in subs]
            source = HostSymbols([d.decode for d in decoders], gc.host_tables(), most, y_hat.device, state=decoders)
        return self._scctx_decode_from(source, params, y_hat), source.state

    @torch.no_grad()
    def decompress(self, strings, shape, lanes=None, device_coder=True, check=True):
        """lanes=None: the one-stream format.  lanes=W: the lanes stream of compress(x, lanes=W); its headers are parsed on the host before
        any device work.  device_coder=True decodes it on the device: no device -> host copy and no synchronize between the upload of the
        streams and the finished y_hat; check=True adds ONE download of the final coder states, after the synthesis transform has been
        launched, and raises ValueError naming the image and the wave streams that did not end where a whole stream ends — a check
        against streams out of step or cut short, NOT a checksum: a changed bit inside an escape's raw payload decodes to another symbol
        and ends clean.  device_coder=False runs the same format on the host coder (ans.LanesDecoder), a hop per pass: the oracle."""
        Wn = lanes_count(lanes, "Elic2022.decompress")
        assert isinstance(strings, (list, tuple)) and len(strings) == 2
        if Wn is None:
            refuse_lanes_strings(strings[0])
            z_hat = self.entropy_bottleneck.decompress(strings[1], shape)
            y_hat = self._scctx_decode(strings[0], self._hyper_synthesis(z_hat))
            return {"x_hat": self._synthesis(y_hat).clamp_(0, 1)}
        subs = lanes_parse(strings[0], Wn)
        z_hat = self.entropy_bottleneck.decompress(strings[1], shape)
        y_hat, state = self._scctx_decode_lanes(subs, self._hyper_synthesis(z_hat), device_coder)
        x_hat = self._synthesis(y_hat).clamp_(0, 1)
        if check:
            lanes_check(state, subs)
        return {"x_hat": x_hat}

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
