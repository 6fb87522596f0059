"""``ssf2020`` — the scale-space-flow video model of Agustsson et al. (CVPR 2020) as CompressAI publishes it — on the engine's own
kernels: its nine sub-networks are ``conv(k=5, s=2)`` / ``deconv(k=5, s=2)`` stacks with ReLU (csrc/conv5.hip, the ReLU in the producing
layer's epilogue), its three hyperpriors use the entropy models and the host rANS coder of the plain hyperprior baselines, and the two
operators that make it a video model — the scale-space volume of the reference frame and the trilinear warp through it — run on
csrc/scale_space.hip (clc_amd/scale_space.py).

Written from CompressAI's published definition (module order and names, hence the ``state_dict`` keys; QReLU on the scale decoder;
``quantize_ste(y - means) + means``; the keyframe's reconstruction detached, later ones not), so CompressAI checkpoints load.
CompressAI is not a dependency: the model is checked against a plain-torch restatement (tests/ssf_ref.py).  CompressAI builds the three
hyperpriors with its defaults (192, 192); here they are ``Hyperprior(planes, planes)``, the same at the default width, and
``mid_planes`` sizes the six encoders / decoders only.

A frame is coded against the previous RECONSTRUCTION: keyframe -> y, z; every later frame -> motion (y, z) and residual (y, z).
``forward`` returns unclamped reconstructions, ``decompress`` too (callers clamp); both sides of the codec run the same unclamped
chain, so ``decompress(compress(frames))`` equals the eval-mode forward bit for bit.

The 3-channel residual head and the 6-channel motion head need an input gradient, which the few-channel patch-row path of
layers.Conv2d does not give: their inputs are zero-padded to 4 / 8 channels and the filter likewise inside the forward (the
Parameter keeps CompressAI's shape; autograd slices its gradient), so they run on the aligned 5x5 kernel.  The keyframe head keeps the
patch rows (the image takes no gradient).

THE LANES STREAM (``compress(frames, lanes=W)`` / ``decompress(..., lanes=W)``; DESIGN 30, clc_amd/ans.py: lanes_pack) is opt-in: every
y string becomes the CLN1 container with ONE segment, the latent's h w planes symbols in NHWC order; z stays the default stream.  The
device decoder finishes a latent with one clc_rans_lanes_decode_gauss, so a whole sequence decodes with no device -> host copy and no
synchronize between its first and its last launch (the default format takes one hop per latent, 2 F - 1 for F frames).  With
lanes=None nothing of it runs and the bytes are the default format's.

Plain autograd and the model's own compress / decompress only: TrainEngine, graphed_training and CodecEngine do not take this model.
Video frames come in and go out as YUV 4:2:0 sample planes through clc_amd/frames.py; codec.pack_sequence is the container.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ans, ops
from ..entropy_models import EntropyBottleneck, GaussianConditional
from ..layers import conv, deconv
from ..ops import ACT_NONE, ACT_RELU, CL
from ..scale_space import gaussian_taps, scale_space_volume, scale_space_warp
from ..vbr import StepTable, check_quality, frame_qualities, model_step
from .clc import CompressionModel, _resize_registered_buffers
from .coding import (check_stream_ends, device_ends, lanes_check, lanes_count, lanes_parse, lanes_strings, refuse_lanes_strings,
                     upload_streams)

__all__ = ["ScaleSpaceFlow"]


class _QReLUFn(torch.autograd.Function):
    """CompressAI's QReLU: clamp(0, 2^bit_depth - 1) forward; backward passes the gradient inside the range and multiplies it by
    exp(-alpha^beta |2 x / max - 1|^beta) outside (plain torch: three small maps per hyperprior)."""

    @staticmethod
    def forward(ctx, x, bit_depth, beta):
        ctx.alpha, ctx.beta, ctx.max_value = 0.9943258522851727, beta, 2 ** bit_depth - 1
        ctx.save_for_backward(x)
        return x.clamp(min=0, max=ctx.max_value)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        sub = torch.exp(-ctx.alpha ** ctx.beta * torch.abs(2.0 * x / ctx.max_value - 1) ** ctx.beta) * g
        return torch.where((x < 0) | (x > ctx.max_value), sub, g), None, None


class QReLU(nn.Module):
    def __init__(self, bit_depth=8, beta=100):
        super().__init__()
        self.bit_depth, self.beta = int(bit_depth), beta

    def forward(self, x):
        return _QReLUFn.apply(x, self.bit_depth, self.beta)


def _head(layer, x, act):
    """a 5x5 / stride-2 layer whose input has Cin % 4 != 0 AND takes a gradient: input and filter zero-padded to the next multiple of 4"""
    pad = -layer.in_channels % 4
    if pad == 0:
        return layer(x, act=act)
    xp = F.pad(x, (0, 0, 0, 0, 0, pad)).contiguous(memory_format=CL)
    wp = F.pad(layer.weight, (0, 0, 0, 0, 0, pad))
    return ops.conv2d(xp, wp, layer.bias, stride=layer.stride[0], act=act)


class _Stack(nn.Sequential):
    """conv / deconv layers with ReLU placeholders between them (CompressAI's Sequential indexes); the ReLUs run in the epilogues"""

    input_grad = False   # True: the first layer's input takes a gradient (see _head)

    def forward(self, x):
        layers = [m for m in self if not isinstance(m, nn.ReLU)]
        for i, m in enumerate(layers):
            act = ACT_RELU if i + 1 < len(layers) else ACT_NONE
            x = _head(m, x, act) if (i == 0 and self.input_grad) else m(x, act=act)
        return x


class Encoder(_Stack):
    def __init__(self, in_planes, mid_planes=128, out_planes=192, input_grad=False):
        super().__init__(conv(in_planes, mid_planes), nn.ReLU(inplace=True), conv(mid_planes, mid_planes), nn.ReLU(inplace=True),
                         conv(mid_planes, mid_planes), nn.ReLU(inplace=True), conv(mid_planes, out_planes))
        self.input_grad = bool(input_grad)


class Decoder(_Stack):
    def __init__(self, out_planes, in_planes=192, mid_planes=128):
        super().__init__(deconv(in_planes, mid_planes), nn.ReLU(inplace=True), deconv(mid_planes, mid_planes), nn.ReLU(inplace=True),
                         deconv(mid_planes, mid_planes), nn.ReLU(inplace=True), deconv(mid_planes, out_planes))


class HyperEncoder(_Stack):
    def __init__(self, in_planes=192, mid_planes=192, out_planes=192):
        super().__init__(conv(in_planes, mid_planes), nn.ReLU(inplace=True), conv(mid_planes, mid_planes), nn.ReLU(inplace=True),
                         conv(mid_planes, out_planes))


class HyperDecoder(_Stack):
    def __init__(self, in_planes=192, mid_planes=192, out_planes=192):
        super().__init__(deconv(in_planes, mid_planes), nn.ReLU(inplace=True), deconv(mid_planes, mid_planes), nn.ReLU(inplace=True),
                         deconv(mid_planes, out_planes))


class HyperDecoderWithQReLU(nn.Module):
    def __init__(self, in_planes=192, mid_planes=192, out_planes=192):
        super().__init__()
        self.deconv1 = deconv(in_planes, mid_planes)
        self.qrelu1 = QReLU(8, 100)
        self.deconv2 = deconv(mid_planes, mid_planes)
        self.qrelu2 = QReLU(8, 100)
        self.deconv3 = deconv(mid_planes, out_planes)
        self.qrelu3 = QReLU(8, 100)

    def forward(self, x):
        return self.qrelu3(self.deconv3(self.qrelu2(self.deconv2(self.qrelu1(self.deconv1(x))))))


class Hyperprior(CompressionModel):
    """mean-scale hyperprior of one latent: y -> (y_hat, {"y", "z"} likelihoods); compress / decompress on the host rANS coder.
    rate_levels > 0 (VARIABLE RATE): a StepTable ``y_step`` for the latent, and ``q`` on forward / compress / decompress —
    the quality, a float in [0, rate_levels - 1]; q=None is the fixed-rate path with today's launches."""

    def __init__(self, planes=192, mid_planes=192, rate_levels=0):
        super().__init__(entropy_bottleneck_channels=mid_planes)
        if int(rate_levels) < 0:
            raise ValueError(f"Hyperprior: rate_levels must not be negative (got {rate_levels})")
        if int(rate_levels):
            self.y_step = StepTable(planes, int(rate_levels))
        self.hyper_encoder = HyperEncoder(planes, mid_planes, planes)
        self.hyper_decoder_mean = HyperDecoder(planes, mid_planes, planes)
        self.hyper_decoder_scale = HyperDecoderWithQReLU(planes, mid_planes, planes)
        self.gaussian_conditional = GaussianConditional(None)

    def forward(self, y, q=None):
        step = model_step(self, q, "Hyperprior.forward")
        z = self.hyper_encoder(y)
        z_hat, z_likelihoods = self.entropy_bottleneck(z)
        scales = self.hyper_decoder_scale(z_hat)
        means = self.hyper_decoder_mean(z_hat)
        # (likelihood of the noisy / dequantised y, ste_round(y - means) + means) in one kernel
        if step is None:
            y_likelihoods, y_hat = self.gaussian_conditional.likelihood_and_ste(y, scales, means)
        else:
            y_likelihoods, y_hat = self.gaussian_conditional.likelihood_and_ste(y, scales, means, step=step)
        return y_hat, {"y": y_likelihoods, "z": z_likelihoods}

    @staticmethod
    def _dequantise(sym, means, step):
        """y_hat from decoded symbols, as every side of the codec forms it in torch ops: (float)symbol + mean, and under a step
        (float)symbol * step + mean as two rounded operations — clc_quantize_build_indexes_step's expression"""
        vals = sym.to(torch.float32)
        if step is not None:
            vals = vals * step.reshape(1, -1, 1, 1)
        return vals + means

    @torch.no_grad()
    def rate_sweep(self, y, qs):
        """estimated bits of y per image under each quality of qs (at most 16) -> f32 [B, len(qs)] on the device, one
        ops.gauss_rate_sweep: what a per-frame byte budget would be chosen from (z's bits are not in it)"""
        steps = torch.stack([model_step(self, q, "Hyperprior.rate_sweep") for q in qs])
        z_hat, _ = self.entropy_bottleneck(self.hyper_encoder(y), training=False)
        return ops.gauss_rate_sweep(y, self.hyper_decoder_mean(z_hat), self.hyper_decoder_scale(z_hat), steps)

    @torch.no_grad()
    def compress(self, y, lanes=None, q=None):
        """lanes=None: one host-coded y stream per image.  lanes=W: the lanes stream, one segment of the latent's symbols in NHWC
        order, encoded on the device (two downloads: the header, the packed words); pass the same W — and the same q — to decompress."""
        Wn = lanes_count(lanes, "Hyperprior.compress")
        step = model_step(self, q, "Hyperprior.compress")
        z = self.hyper_encoder(y)
        z_strings = self.entropy_bottleneck.compress(z)
        z_hat = self.entropy_bottleneck.decompress(z_strings, z.size()[-2:])
        scales = self.hyper_decoder_scale(z_hat)
        means = self.hyper_decoder_mean(z_hat)
        gc = self.gaussian_conditional
        sym, idx, _ = gc.quantize_and_index(y, means, scales) if step is None else gc.quantize_and_index(y, means, scales, step=step)
        y_hat = self._dequantise(sym, means, step)   # formed as decompress forms it: the two sides run one chain
        if Wn is not None:   # the int32 buffers stay on the device
            return y_hat, {"strings": [self._lanes_y_strings(sym, idx, Wn), z_strings], "shape": z.size()[-2:]}
        cdf, ln, off = gc.host_tables()
        sym = sym.contiguous().cpu().numpy()   # [N, C, H, W]: the element order of CompressAI's symbols[i].reshape(-1)
        idx = idx.contiguous().cpu().numpy()
        y_strings = [ans.encode(sym[i].reshape(-1), idx[i].reshape(-1), cdf, ln, off) for i in range(sym.shape[0])]
        return y_hat, {"strings": [y_strings, z_strings], "shape": z.size()[-2:]}

    def _lanes_y_strings(self, sym, idx, W):
        """quantize_build_indexes' int32 buffers (NCHW views of NHWC memory) -> one lanes string per image: one clc_rans_lanes_encode
        with the latent as its one segment, one clc_rans_lanes_pack, then two device -> host copies (the header, the packed words)"""
        gc = self.gaussian_conditional
        B = sym.shape[0]
        flat = lambda t: t.permute(0, 2, 3, 1).reshape(B, -1)   # (the buffer's own order: a view)
        out, _, result = ops.rans_lanes_encode(flat(sym), flat(idx), [int(sym[0].numel())], W, (gc._quantized_cdf, gc._cdf_length, gc._offset))
        packed, header = ops.rans_lanes_pack(out, result)
        head = header.cpu().numpy()
        words = packed[:int(head[B * W])].cpu().numpy() if (head[:B * W] >= 0).all() else np.zeros(0, np.int32)
        return lanes_strings(head, words, B, W)   # (raises by name on a negative code)

    def _decode_lanes(self, subs, z_strings, shape, device_coder=True, out=None, step=None):
        """The decoder over parsed lanes streams (subs[b][w]: bytes; coding.lanes_parse) -> (y_hat, state).  The z strings are decoded
        on the host and uploaded, which waits on nothing the device computes.
        device_coder: one pinned upload of every wave stream's states, spans and words, the two hyper-decoder chains and ONE
        clc_rans_lanes_decode_gauss — no download, no synchronize; state is the device's int32 [B, W, 130] as the decode left it.
        Host coder: one index download and one ans.LanesDecoder per image; state is the list of decoders.
        out: a pixel-major [B, planes, h, w] map to write, e.g. a channel slice of a wider buffer."""
        if len(subs) != len(z_strings):
            raise ValueError(f"decompress: {len(subs)} y streams for {len(z_strings)} z streams")
        z_hat = self.entropy_bottleneck.decompress(z_strings, shape)
        gc = self.gaussian_conditional
        if device_coder:
            state, spans, words = upload_streams(subs, 2 * ans.LANES, z_hat.device)   # a wave stream starts with its 64 lane states
        scales = self.hyper_decoder_scale(z_hat)
        means = self.hyper_decoder_mean(z_hat)
        if device_coder:
            tables = (gc._quantized_cdf, gc._cdf_length, gc._offset)
            if step is None:
                return ops.rans_lanes_decode_gauss(scales, means, gc.scale_table, tables, words, spans, state, y_hat=out), state
            return ops.rans_lanes_decode_gauss(scales, means, gc.scale_table, tables, words, spans, state, y_hat=out, step=step), state
        decoders = [ans.LanesDecoder(img) for img in subs]
        cdf, ln, off = gc.host_tables()
        idx = gc.build_indexes(scales) if step is None else gc.build_indexes(scales, step=step)
        idx = idx.permute(0, 2, 3, 1).contiguous().cpu().numpy()   # NHWC: the segment's order
        sym = np.stack([d.decode(idx[b].reshape(-1), cdf, ln, off).reshape(idx.shape[1:]) for b, d in enumerate(decoders)])
        y_hat = self._dequantise(torch.from_numpy(sym).to(z_hat.device).permute(0, 3, 1, 2), means, step)
        return (y_hat if out is None else out.copy_(y_hat)), decoders

    @torch.no_grad()
    def decompress(self, strings, shape, lanes=None, device_coder=True, out=None, q=None):
        """lanes=None: the one-stream format, one hop.  lanes=W: the lanes stream of compress(y, lanes=W), its headers parsed before
        any device work; device_coder=False decodes the same format on the host coder (ans.LanesDecoder): the oracle and the
        fallback.  out: the pixel-major map y_hat is written into (the lanes kernel writes it in place at its leading dimension)."""
        Wn = lanes_count(lanes, "Hyperprior.decompress")
        step = model_step(self, q, "Hyperprior.decompress")
        assert isinstance(strings, (list, tuple)) and len(strings) == 2
        if Wn is not None:
            return self._decode_lanes(lanes_parse(strings[0], Wn), strings[1], shape, device_coder, out, step)[0]
        refuse_lanes_strings(strings[0])
        z_hat = self.entropy_bottleneck.decompress(strings[1], shape)
        scales = self.hyper_decoder_scale(z_hat)
        means = self.hyper_decoder_mean(z_hat)
        gc = self.gaussian_conditional
        cdf, ln, off = gc.host_tables()
        idx = (gc.build_indexes(scales) if step is None else gc.build_indexes(scales, step=step)).contiguous().cpu().numpy()
        sym = np.empty(idx.shape, dtype=np.float32)
        for i, s in enumerate(strings[0]):
            sym[i] = ans.decode(s, idx[i].reshape(-1), cdf, ln, off).reshape(idx.shape[1:])
        y_hat = self._dequantise(torch.from_numpy(sym).to(z_hat.device).contiguous(memory_format=CL), means, step)
        return y_hat if out is None else out.copy_(y_hat)


class ScaleSpaceFlow(CompressionModel):
    """ScaleSpaceFlow(num_levels=5, sigma0=1.5, scale_field_shift=1.0): ``scale_field_shift`` is stored and unused, as in CompressAI.
    mid_planes / planes (multiples of 4; 128 / 192 in the published model) size the sub-networks.
    rate_levels > 0 (VARIABLE RATE): one StepTable inside each of the three hyperpriors, and ``q`` on forward / compress /
    decompress: a float for every frame or a list of one float per frame; one q serves both latents of a P-frame."""

    def __init__(self, num_levels=5, sigma0=1.5, scale_field_shift=1.0, mid_planes=128, planes=192, rate_levels=0, **kwargs):
        from ..intnet import refuse_integer_hyper

        refuse_integer_hyper("ScaleSpaceFlow", kwargs)   # its hyperpriors' integer nets are a follow-up
        if set(kwargs) - {"integer_hyper", "exact"}:
            raise TypeError(f"ScaleSpaceFlow.__init__() got an unexpected keyword argument {sorted(set(kwargs) - {'integer_hyper', 'exact'})[0]!r}")
        super().__init__()
        if int(rate_levels) < 0:
            raise ValueError(f"ScaleSpaceFlow: rate_levels must not be negative (got {rate_levels})")
        if int(num_levels) != num_levels or num_levels < 1:
            raise ValueError(f"ScaleSpaceFlow: num_levels must be an integer >= 1 (got num_levels={num_levels})")
        if num_levels > 8:
            raise ValueError(f"ScaleSpaceFlow: num_levels must be at most 8, since frames are multiples of 128 (got num_levels={num_levels})")
        gaussian_taps(sigma0)   # (refuses sigma0 <= 0, and a sigma0 whose window the kernels do not take, by name)
        if mid_planes % 4 or planes % 4 or mid_planes < 4 or planes < 4:
            raise ValueError(f"ScaleSpaceFlow: mid_planes and planes must be positive multiples of 4 (the kernels' aligned path); got "
                             f"mid_planes={mid_planes}, planes={planes}")
        self.img_encoder = Encoder(3, mid_planes, planes)
        self.img_decoder = Decoder(3, planes, mid_planes)
        self.img_hyperprior = Hyperprior(planes, planes, rate_levels)
        self.res_encoder = Encoder(3, mid_planes, planes, input_grad=True)
        self.res_decoder = Decoder(3, 2 * planes, mid_planes)
        self.res_hyperprior = Hyperprior(planes, planes, rate_levels)
        self.motion_encoder = Encoder(2 * 3, mid_planes, planes, input_grad=True)
        self.motion_decoder = Decoder(2 + 1, planes, mid_planes)
        self.motion_hyperprior = Hyperprior(planes, planes, rate_levels)
        self.sigma0 = float(sigma0)
        self.num_levels = int(num_levels)
        self.scale_field_shift = scale_field_shift
        self.planes = int(planes)

    # ---- argument checks ----
    @staticmethod
    def _prep(frames):
        if not isinstance(frames, (list, tuple)):
            raise ValueError(f"ScaleSpaceFlow: frames must be a list of [N, 3, H, W] tensors (got {type(frames).__name__})")
        if len(frames) < 1:
            raise ValueError("ScaleSpaceFlow: fewer than one frame (frames is empty)")
        shape = tuple(frames[0].shape)
        for i, f in enumerate(frames):
            if tuple(f.shape) != shape:
                raise ValueError(f"ScaleSpaceFlow: frames of differing shapes (frame 0 is {shape}, frame {i} is {tuple(f.shape)})")
        if len(shape) != 4 or shape[1] != 3 or shape[2] % 128 or shape[3] % 128 or shape[2] < 128 or shape[3] < 128:
            raise ValueError(f"ScaleSpaceFlow: frames must be [N, 3, H, W] with H and W multiples of 128 (got {shape})")
        for f in frames:
            ops._require_gpu(f, "ScaleSpaceFlow")
        return [f.detach().contiguous(memory_format=CL) for f in frames]   # (the frames take no gradient)

    def _predict(self, x_ref, y_m_hat):
        """the motion-compensated prediction of a frame from the reference reconstruction and the decoded motion latent"""
        info = self.motion_decoder(y_m_hat)   # channels 0-1: the flow, channel 2: the scale field
        volume = scale_space_volume(x_ref, self.sigma0, self.num_levels)
        return scale_space_warp(volume, info[:, :2], info[:, 2:3])

    def _qualities(self, q, frames, who):
        """one checked quality per frame (None: the fixed-rate path) — before any device work"""
        qs = frame_qualities(q, frames, f"ScaleSpaceFlow.{who}")
        for t, qt in enumerate(qs):
            if qt is not None:
                check_quality(self.img_hyperprior, qt, f"ScaleSpaceFlow.{who} (frame {t})")
        return qs

    # ---- training / evaluation forward ----
    def forward(self, frames, q=None):
        qs = self._qualities(q, len(frames) if isinstance(frames, (list, tuple)) else 0, "forward")
        frames = self._prep(frames)
        x_hat, lik = self.forward_keyframe(frames[0], qs[0])
        recs, liks = [x_hat], [lik]
        x_ref = x_hat.detach()
        for x, qt in zip(frames[1:], qs[1:]):
            x_ref, lik = self.forward_inter(x, x_ref, qt)
            recs.append(x_ref)
            liks.append(lik)
        return {"x_hat": recs, "likelihoods": liks}

    def forward_keyframe(self, x, q=None):
        y_hat, lik = self.img_hyperprior(self.img_encoder(x)) if q is None else self.img_hyperprior(self.img_encoder(x), q=q)
        return self.img_decoder(y_hat), {"keyframe": lik}

    def forward_inter(self, x_cur, x_ref, q=None):
        kw = {} if q is None else {"q": q}
        y_m_hat, m_lik = self.motion_hyperprior(self.motion_encoder(torch.cat((x_cur, x_ref), dim=1)), **kw)
        x_pred = self._predict(x_ref, y_m_hat)
        y_r_hat, r_lik = self.res_hyperprior(self.res_encoder(x_cur - x_pred), **kw)
        x_rec = x_pred + self.res_decoder(torch.cat((y_r_hat, y_m_hat), dim=1))
        return x_rec, {"motion": m_lik, "residual": r_lik}

    # ---- codec ----
    @torch.no_grad()
    def compress(self, frames, lanes=None, q=None):
        """-> (frame_strings, shape_infos): the keyframe's [y_strings, z_strings] and z size, then per frame
        {"motion": [y, z], "residual": [y, z]} and {"motion": z size, "residual": z size}.  lanes=W: every y string is the lanes
        stream (Hyperprior.compress); pass the same W to decompress.  q: the quality, one float or one per frame (needs
        rate_levels > 0); the strings do not carry it — pass the same q to decompress (frames.encode_yuv420 stores it)."""
        Wn = lanes_count(lanes, "ScaleSpaceFlow.compress")
        qs = self._qualities(q, len(frames) if isinstance(frames, (list, tuple)) else 0, "compress")
        frames = self._prep(frames)
        y_hat, item = self.img_hyperprior.compress(self.img_encoder(frames[0]), lanes=Wn, q=qs[0])
        x_ref = self.img_decoder(y_hat)
        frame_strings, shape_infos = [item["strings"]], [item["shape"]]
        for x, qt in zip(frames[1:], qs[1:]):
            y_m_hat, m = self.motion_hyperprior.compress(self.motion_encoder(torch.cat((x, x_ref), dim=1)), lanes=Wn, q=qt)
            x_pred = self._predict(x_ref, y_m_hat)
            y_r_hat, r = self.res_hyperprior.compress(self.res_encoder(x - x_pred), lanes=Wn, q=qt)
            x_ref = x_pred + self.res_decoder(torch.cat((y_r_hat, y_m_hat), dim=1))
            frame_strings.append({"motion": m["strings"], "residual": r["strings"]})
            shape_infos.append({"motion": m["shape"], "residual": r["shape"]})
        return frame_strings, shape_infos

    @staticmethod
    def _latents(t, strings, shapes):
        """the coded latents of frame t in decoding order: [(name, [y strings, z strings], z size)]"""
        if t == 0:
            return [("keyframe", strings, shapes)]
        return [(k, strings[k], shapes[k]) for k in ("motion", "residual")]

    @torch.no_grad()
    def _decompress_lanes(self, frame_strings, shape_infos, Wn, device_coder, check, qs):
        parsed = []   # every frame's headers, before any device work
        for t, (strings, shapes) in enumerate(zip(frame_strings, shape_infos)):
            row = []
            for name, s, shape in self._latents(t, strings, shapes):
                try:
                    row.append((name, lanes_parse(s[0], Wn), s[1], shape))
                except ValueError as e:
                    raise ValueError(f"frame {t}, {name} latent: {e}") from None
            parsed.append(row)
        ends = []   # (frame, latent, wave streams, coder state) of every latent
        (name, subs, zs, shape), = parsed[0]
        # the step vectors each frame needs — the keyframe's one, a later frame's (motion, residual) — None without q
        steps = [(model_step(self.img_hyperprior, qt, "ScaleSpaceFlow.decompress"),) if t == 0 else
                 tuple(model_step(h, qt, "ScaleSpaceFlow.decompress") for h in (self.motion_hyperprior, self.res_hyperprior))
                 for t, qt in enumerate(qs)]
        y_hat, state = self.img_hyperprior._decode_lanes(subs, zs, shape, device_coder, step=steps[0][0])
        ends.append((0, name, subs, state))
        x_ref = self.img_decoder(y_hat)
        recs = [x_ref]
        P = self.planes
        for t in range(1, len(parsed)):
            (mn, m_subs, m_zs, m_shape), (rn, r_subs, r_zs, r_shape) = parsed[t]
            # ONE [B, 2 planes, h, w] buffer per frame, (residual | motion): each latent is decoded into its half, no torch.cat
            both = torch.empty((len(m_subs), 2 * P, 8 * int(m_shape[0]), 8 * int(m_shape[1])), device=x_ref.device, dtype=torch.float32,
                               memory_format=CL)
            y_m_hat, state = self.motion_hyperprior._decode_lanes(m_subs, m_zs, m_shape, device_coder, out=both[:, P:], step=steps[t][0])
            ends.append((t, mn, m_subs, state))
            x_pred = self._predict(x_ref, y_m_hat)
            _, state = self.res_hyperprior._decode_lanes(r_subs, r_zs, r_shape, device_coder, out=both[:, :P], step=steps[t][1])
            ends.append((t, rn, r_subs, state))
            x_ref = x_pred + self.res_decoder(both)
            recs.append(x_ref)
        if check:
            self._check_ends(ends, device_coder)
        return recs

    @staticmethod
    def _check_ends(ends, device_coder):
        """coding.check_stream_ends over every wave stream of every latent of every frame, after the last frame's launches; the
        device coder's states are gathered on the device and come down in ONE copy.  Raises naming the frame and the latent."""
        if device_coder:
            x, pos = device_ends(torch.cat([state for *_, state in ends]))
        lo = 0
        for t, name, subs, state in ends:
            try:
                if device_coder:
                    hi = lo + len(subs)
                    check_stream_ends(x[lo:hi], pos[lo:hi], [[len(blob) // 4 for blob in img] for img in subs], ans.LANES_STREAM.noun)
                    lo = hi
                else:
                    lanes_check(state, subs)
            except ValueError as e:
                raise ValueError(f"frame {t}, {name} latent: {e}") from None

    @torch.no_grad()
    def decompress(self, frame_strings, shape_infos, lanes=None, device_coder=True, check=True, q=None):
        """-> the list of reconstructions, unclamped as forward returns them.  lanes=None: the default format, one hop per latent
        (2 F - 1 for F frames).  lanes=W: the strings of compress(frames, lanes=W); every frame's headers are parsed first, and with
        device_coder=True there is no device -> host copy and no synchronize between the keyframe's first launch and the last
        frame's last, whatever F; check=True adds exactly ONE download after that, the final coder states of every stream of every
        frame, and raises ValueError naming the frame, the latent and the wave streams that did not end where a whole stream ends
        (not a checksum).  device_coder=False runs the same format on the host coder: the oracle and the fallback."""
        Wn = lanes_count(lanes, "ScaleSpaceFlow.decompress")
        if len(frame_strings) < 1 or len(frame_strings) != len(shape_infos):
            raise ValueError(f"ScaleSpaceFlow.decompress: {len(frame_strings)} frame strings for {len(shape_infos)} shape infos (at least one of each)")
        qs = self._qualities(q, len(frame_strings), "decompress")
        if Wn is not None:
            return self._decompress_lanes(frame_strings, shape_infos, Wn, device_coder, check, qs)
        for t, (strings, shapes) in enumerate(zip(frame_strings, shape_infos)):
            for _name, s, _shape in self._latents(t, strings, shapes):
                refuse_lanes_strings(s[0])
        x_ref = self.img_decoder(self.img_hyperprior.decompress(frame_strings[0], shape_infos[0], q=qs[0]))
        recs = [x_ref]
        for strings, shapes, qt in zip(frame_strings[1:], shape_infos[1:], qs[1:]):
            y_m_hat = self.motion_hyperprior.decompress(strings["motion"], shapes["motion"], q=qt)
            x_pred = self._predict(x_ref, y_m_hat)
            y_r_hat = self.res_hyperprior.decompress(strings["residual"], shapes["residual"], q=qt)
            x_ref = x_pred + self.res_decoder(torch.cat((y_r_hat, y_m_hat), dim=1))
            recs.append(x_ref)
        return recs

    def load_state_dict(self, state_dict, strict=True):
        for name, m in self.named_modules():
            if isinstance(m, EntropyBottleneck):
                _resize_registered_buffers(m, name, ["_quantized_cdf", "_offset", "_cdf_length"], state_dict)
            if isinstance(m, GaussianConditional):
                _resize_registered_buffers(m, name, ["_quantized_cdf", "_offset", "_cdf_length", "scale_table"], state_dict)
        return nn.Module.load_state_dict(self, state_dict, strict=strict)
