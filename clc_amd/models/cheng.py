"""``cheng2020-anchor`` / ``cheng2020-attn`` — Cheng et al., "Learned Image Compression with Discretized Gaussian Mixture Likelihoods and
Attention Modules" (CVPR 2020) on the engine's own kernels: the "Cheng" curve of the RD plot.

Transforms: residual blocks with 3x3 convolutions, sub-pixel upsampling and (``-attn``) the simplified attention block — exactly the leaves
CLC runs on the 3x3 kernels.  Entropy model: the ``mbt2018`` context model (masked 5x5 convolution + three 1x1 layers) predicting, per
latent element, a K-component Gaussian mixture.

The layer list is written from the published CompressAI classes (``Cheng2020Anchor`` / ``Cheng2020Attention``: module names, hence the
``state_dict`` keys) and the paper; CompressAI is not a dependency and is not installed where this is built, so nothing here is pinned
against it.  Like the other baselines the models are checked against a plain-torch restatement of the same definitions
(tests/cheng_ref.py).  The ``K > 1`` parameter layout and stream are the project's own.

K = 1 is the published single-Gaussian model: forward, compress and decompress are ``mbt2018``'s, stream, schedule and bits as
JointAutoregressiveHierarchicalPriors defines them; only the four transforms differ.

K > 1.  ``entropy_parameters`` ends in 3 K N channels, output channel part * K N + k N + c with part 0 the scales, 1 the means, 2 the
weight logits; ``gaussian_conditional`` is a GaussianMixtureConditional (csrc/gmm.hip), which reads the three groups of that one map in
place.  With a mixture there is no mean to subtract before rounding: y_hat = round(y) is known before the context model runs, so the
ENCODER's autoregressive pass is one parallel step over all pixels; the DECODER follows the wavefront, W + 3 (H - 1) steps.

STREAM ORDER (K > 1): one rANS stream per image for y — the pixels of ``ar_wavefront_order(H, W)`` (the steps of
``ar_schedule(H, W, "wavefront")`` ascending, raster inside a step), channels inner; every symbol through its own integer CDF row (THE ROW
RULE of include/clc_hip.h), built on the device by the same scan on both sides; z as in the other hyperprior models.  The four-layer
chain runs on clc_ar_linear on both sides (its summation order depends on K alone), h_s on the batch-invariant 3x3 routes the CLC codec
relies on: a stream written at batch 8 decodes at batch 1.

THE SPLIT STREAM (K > 1, opt-in: ``compress(x, substreams=S)`` / ``decompress(..., substreams=S)``).  The y string becomes
``ans.split_pack`` of S independent rANS sub-streams: element (position i of ar_wavefront_order, channel c) belongs to sub-stream c mod S,
inside a sub-stream i ascending then c ascending, and sub-stream s is exactly ``ans.encode_direct(triples[:, s::S])`` — same triples, same
host coder.  8 + 12 S bytes more per image (200 at S = 16).  Its decoder runs on the device, one wave per (image, sub-stream)
(clc_gmm_decode_step): the whole wavefront pass is stream-ordered launches with no host hop.  The default stays the one-stream format,
byte for byte.

TrainEngine, graphed_training, CodecEngine, ContextCodecEngine and ReferenceBank do not take these models.  The walk over the wavefront's steps is
``mbt2018``'s (_ar_walk), for both decoders.  The host side of the coder — the start of a decoder's loop, the hop of a host-decoded step,
the upload image of the device-decoded split stream, its parser and its end-state check — is coding.py's.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from .. import ans, ops
from ..entropy_models import GaussianMixtureConditional
from ..layers import (AttentionBlock, Conv2d, ResidualBlock, ResidualBlockUpsample, ResidualBlockWithStride, conv3x3, subpel_conv3x3)
from ..ops import ACT_LRELU, CL
from .clc import _resize_registered_buffers
from .coding import HostHop, coded_item, decoder_start, open_decoders, stream_check, stream_parse, upload_streams
from .hyperprior import JointAutoregressiveHierarchicalPriors, ar_schedule

_SYM_BOUND = float(1 << 24)
_CHUNK_ROWS = 8192   # rows of the chain's workspace in the encoder's one parallel step (the order rule makes the chunking invisible)


def ar_wavefront_order(H, W):
    """The pixels of an H x W latent in the order of the K > 1 stream: the steps of ar_schedule(H, W, "wavefront") ascending, raster inside
    a step.  -> list of (h, w)"""
    return [p for s in ar_schedule(H, W, "wavefront") for p in s]


def _run_lrelu(seq, x):
    """a Sequential whose LeakyReLU placeholders are fused into the producing layer's epilogue"""
    mods = list(seq)
    i = 0
    while i < len(mods):
        if i + 1 < len(mods) and isinstance(mods[i + 1], nn.LeakyReLU):
            x = mods[i](x, act=ACT_LRELU)
            i += 2
        else:
            x = mods[i](x)
            i += 1
    return x


class Cheng2020Anchor(JointAutoregressiveHierarchicalPriors):
    """cheng2020-anchor (no attention), M = N; K mixture components (K = 1: the published single-Gaussian model).  See the module
    docstring for the layer list's source, the K > 1 layout and the stream."""

    def __init__(self, N=192, K=1, **kwargs):
        name = type(self).__name__
        if N == 128:
            raise ValueError(f"{name}: N = 128: cheng2020 qualities 1–3 are not built (N % 12 != 0: 10N/3 and 8N/3 must be whole multiples of 4)")
        if N % 12:
            raise ValueError(f"{name} needs N % 12 == 0 (then 10N/3, 8N/3 and 3N/2 are whole and multiples of 4, the kernels' aligned "
                             f"path); got N = {N}")
        if not 1 <= int(K) <= 4:
            raise ValueError(f"{name}: K must be between 1 and 4 mixture components (got K = {K})")
        super().__init__(N=N, M=N, **kwargs)
        self.K = int(K)
        self.g_a, self.g_s = self._build_transforms(N)
        lrelu = lambda: nn.LeakyReLU(inplace=True)
        self.h_a = nn.Sequential(conv3x3(N, N), lrelu(), conv3x3(N, N), lrelu(), conv3x3(N, N, stride=2), lrelu(), conv3x3(N, N), lrelu(),
                                 conv3x3(N, N, stride=2))
        self.h_s = nn.Sequential(conv3x3(N, N), lrelu(), subpel_conv3x3(N, N, 2), lrelu(), conv3x3(N, N * 3 // 2), lrelu(),
                                 subpel_conv3x3(N * 3 // 2, N * 3 // 2, 2), lrelu(), conv3x3(N * 3 // 2, N * 2))
        if self.K > 1:
            self.entropy_parameters[4] = Conv2d(N * 8 // 3, 3 * self.K * N, 1)
            self.gaussian_conditional = GaussianMixtureConditional(self.K)

    @staticmethod
    def _build_transforms(N):
        RBWS, RBU, RB = ResidualBlockWithStride, ResidualBlockUpsample, ResidualBlock
        g_a = nn.Sequential(RBWS(3, N, 2), RB(N, N), RBWS(N, N, 2), RB(N, N), RBWS(N, N, 2), RB(N, N), conv3x3(N, N, stride=2))
        g_s = nn.Sequential(RB(N, N), RBU(N, N, 2), RB(N, N), RBU(N, N, 2), RB(N, N), RBU(N, N, 2), RB(N, N), subpel_conv3x3(N, 3, 2))
        return g_a, g_s

    def _hyper_analysis(self, y):
        return _run_lrelu(self.h_a, y)

    def _hyper_synthesis(self, z_hat):
        return _run_lrelu(self.h_s, z_hat)

    # ---- K > 1: the mixture ----
    def forward(self, x):
        if self.K == 1:
            return super().forward(x)
        x = self._prep(x)
        y = self._analysis(x)
        z = self._hyper_analysis(y)
        z_hat, z_likelihoods = self.entropy_bottleneck(z)
        params = self._hyper_synthesis(z_hat)
        if self.training:
            y_hat = y + torch.empty_like(y, memory_format=CL).uniform_(-0.5, 0.5)
        else:
            y_hat = torch.round(y.detach())
        ctx_params = self.context_prediction(y_hat)
        mixture = self._entropy_parameters(torch.cat((params, ctx_params), 1))   # [B, 3 K N, H, W]: read in place, no chunk copies
        _, y_likelihoods = self.gaussian_conditional.forward_packed(y, mixture)
        x_hat = self._synthesis(y_hat)
        return {"x_hat": x_hat, "likelihoods": {"y": y_likelihoods, "z": z_likelihoods}}

    def update(self, scale_table=None, force=False):
        if self.K == 1:
            return super().update(scale_table, force=force)
        return self.entropy_bottleneck.update(force=force)   # the mixture has no table

    def load_state_dict(self, state_dict, strict=True):
        if self.K == 1:
            return super().load_state_dict(state_dict, strict=strict)
        _resize_registered_buffers(self.entropy_bottleneck, "entropy_bottleneck", ["_quantized_cdf", "_offset", "_cdf_length"], state_dict)
        return nn.Module.load_state_dict(self, state_dict, strict=strict)

    def _gmm_workspace(self, rows, dev):
        N, K = self.N, self.K
        mk = lambda c: torch.empty((rows, c), device=dev, dtype=torch.float32)
        return {"ctx": mk(2 * N), "h1": mk(N * 10 // 3), "h2": mk(N * 8 // 3), "gp": mk(3 * K * N)}

    @torch.no_grad()
    def _gmm_encode(self, y, params):
        """The encoder's one parallel step -> (triples int32 [B, H*W, N, 3] in ar_wavefront_order, y_hat = round(y)): all launches on the
        current stream, no host sync."""
        ops._require_gpu(y, "cheng2020 compress")
        B, N, H, W = y.shape
        y = y.contiguous(memory_format=CL)
        params = params.contiguous(memory_format=CL)
        # known before the context model runs: no mean enters the quantiser.  (The symbol range of THE ROW RULE: +-2^24, NaN at the bottom.)
        y_hat = torch.round(y).nan_to_num_(nan=-_SYM_BOUND, posinf=_SYM_BOUND, neginf=-_SYM_BOUND).clamp_(-_SYM_BOUND, _SYM_BOUND)
        pix = torch.tensor(ar_wavefront_order(H, W), dtype=torch.int32).reshape(-1, 2).to(y.device)
        chunk = max(1, _CHUNK_ROWS // B)
        ws = self._gmm_workspace(B * min(chunk, H * W), y.device)
        filt = self._ar_filters()
        parts = []
        for lo in range(0, H * W, chunk):
            px = pix[lo:lo + chunk]
            self._ar_chain(px, B, H, W, y_hat, params, ws, filt)
            t = torch.empty((B, px.shape[0], N, 3), device=y.device, dtype=torch.int32)
            ops.gmm_finish_encode(ws["gp"], N, self.K, px, y, y_hat, t)   # (rewrites y_hat[pixel] with the value it already holds)
            parts.append(t)
        return (parts[0] if len(parts) == 1 else torch.cat(parts, 1)), y_hat

    def _split_count(self, substreams, what):
        """the checked S of a ``substreams=`` keyword (None: the one-stream format)"""
        if substreams is None:
            return None
        name = type(self).__name__
        if self.K == 1:
            raise ValueError(f"{name}.{what}: substreams= needs a mixture model (K > 1); the K = 1 stream is CompressAI's and stays one stream")
        S = ans.stream_count(ans.SPLIT_STREAM, int(substreams), f"{name}.{what}", "substreams")
        if S > self.N:
            raise ValueError(f"{name}.{what}: substreams = {S} > N = {self.N} (channel c belongs to sub-stream c mod S: some would be empty)")
        return S

    @torch.no_grad()
    def compress(self, x, order="wavefront", substreams=None):
        """substreams=None: the one-stream format.  substreams=S (K > 1): THE SPLIT STREAM of the module docstring, and "substreams": S
        in the result; pass the same S to decompress."""
        S = self._split_count(substreams, "compress")
        if self.K == 1:
            return super().compress(x, order)
        y, params, z_strings, z_size = self._code_inputs(x)
        triples, _ = self._gmm_encode(y, params)
        t = triples.cpu().numpy()   # the one device -> host copy
        if S is None:
            return coded_item([ans.encode_direct(t[i]) for i in range(t.shape[0])], z_strings, z_size)
        y_strings = [ans.split_pack([ans.encode_direct(t[i][:, s::S, :]) for s in range(S)]) for i in range(t.shape[0])]
        return coded_item(y_strings, z_strings, z_size, substreams=S)

    def _gmm_start(self, n_streams, params):
        """what both decoders open with -> (steps, pix, y_hat, params, ws, filt): the arguments of _ar_walk over the wavefront"""
        params, y_hat = decoder_start(params, n_streams, self.N)
        steps, pix = self._ar_pixels(ar_schedule(y_hat.shape[2], y_hat.shape[3], "wavefront"), y_hat.device)
        ws = self._gmm_workspace(y_hat.shape[0] * max(len(s) for s in steps), y_hat.device)
        return steps, pix, y_hat, params, ws, self._ar_filters()

    @torch.no_grad()
    def _gmm_decode(self, y_strings, params):
        """The wavefront pass of decompress -> y_hat: per non-empty step, for the whole batch, one row download, one incremental decode
        per image on a decoder opened once, one symbol upload."""
        start = self._gmm_start(len(y_strings), params)
        decoders = open_decoders(y_strings)

        def decode(rows_np, offs_np, sym_np):
            e = sym_np.size // len(decoders)   # image b's elements of the step: rows b * cnt .. in list order, channels inner
            for b, d in enumerate(decoders):
                sym_np[b * e:(b + 1) * e] = d.decode_rows(rows_np[b * e:(b + 1) * e], offs_np[b * e:(b + 1) * e])
        self._gmm_hops(*start, decode)
        return start[2]   # y_hat

    def _gmm_hops(self, steps, pix, y_hat, params, ws, filt, decode):
        """The host-decoded wavefront pass: per non-empty step the chain, gmm_finish_decode, one hop and gmm_commit.  A hop downloads
        ONE buffer, the step's rows and behind them its offsets, and uploads the symbols that
        decode(rows int32 [n N, GMM_ROW_STRIDE], offsets int32 [n N], symbols int32 [n N]) wrote."""
        (B, N, H, W), K, R = y_hat.shape, self.K, ops.GMM_ROW_STRIDE
        split = lambda down_np, sym_np: decode(down_np[:sym_np.size * R].reshape(-1, R), down_np[sym_np.size * R:], sym_np)
        rows = B * max(len(s) for s in steps)
        hop = HostHop(rows * N * (R + 1), rows * N, y_hat.device)
        for cnt, px, gp in self._ar_walk(steps, pix, y_hat, params, ws, filt):
            n = B * cnt
            down, sym_dev = hop.step(n * N * (R + 1), n * N)
            ops.gmm_finish_decode(gp, N, K, px, B, H, W, down[:n * N * R].view(n, N, R), down[n * N * R:].view(n, N))
            hop.run(split)
            ops.gmm_commit(sym_dev.view(n, N), N, px, y_hat)

    @torch.no_grad()
    def _gmm_decode_split(self, subs, params, device_decoder=True):
        """The wavefront pass over split streams (subs[b][s]: bytes) -> (y_hat, state).
        device_decoder: one pinned upload of every sub-stream's words, spans and initial states, then per non-empty step the chain and
        one clc_gmm_decode_step — stream-ordered launches only, no download, no synchronize, no per-image loop; state is the device's
        int32 [B, S, 4] (x low, x high, pos, pad) as the last step left it.
        Host decoder: the hop per step of _gmm_decode with one RansDecoder per (image, sub-stream); state is None."""
        start = self._gmm_start(len(subs), params)
        y_hat = start[2]
        B, N, S = y_hat.shape[0], self.N, len(subs[0])
        if device_decoder:
            state, spans, words = upload_streams(subs, 2, y_hat.device)   # a sub-stream starts with the two words of its coder state
            for _, px, gp in self._ar_walk(*start):
                ops.gmm_decode_step(gp, N, self.K, px, words, spans, state, y_hat)
            return y_hat, state
        decoders = [open_decoders(img) for img in subs]

        def decode(rows_np, offs_np, sym_np):
            R = rows_np.shape[1]
            rows_np, offs_np, sym_np = rows_np.reshape(B, -1, N, R), offs_np.reshape(B, -1, N), sym_np.reshape(B, -1, N)
            for b in range(B):
                for k, dd in enumerate(decoders[b]):   # sub-stream k's elements of the step: list order, then its channels ascending
                    r = np.ascontiguousarray(rows_np[b, :, k::S]).reshape(-1, R)
                    o = np.ascontiguousarray(offs_np[b, :, k::S]).reshape(-1)
                    sym_np[b, :, k::S] = dd.decode_rows(r, o).reshape(sym_np.shape[1], -1)
        self._gmm_hops(*start, decode)
        return y_hat, None

    @torch.no_grad()
    def decompress(self, strings, shape, substreams=None, device_decoder=True, check=True):
        """substreams=None: the one-stream format.  substreams=S: the split stream of compress(x, substreams=S), decoded on the device
        (device_decoder=True: no device -> host copy and no synchronize between the upload of the streams and the finished y_hat;
        check=True adds ONE download of the final coder states, after the synthesis transform has been launched, and raises ValueError
        naming the image and the sub-streams that did not end where a whole stream ends — a check against streams out of step or cut
        short, not a checksum: a changed bit inside an escape's raw payload decodes to another symbol and ends clean) or on the host (device_decoder=False: a hop per
        step, the rows of clc_gmm_finish through RansDecoder.decode_rows — the same symbols)."""
        S = self._split_count(substreams, "decompress")
        if self.K == 1:
            return super().decompress(strings, shape)
        assert isinstance(strings, (list, tuple)) and len(strings) == 2
        if S is None:
            z_hat = self.entropy_bottleneck.decompress(strings[1], shape)
            y_hat = self._gmm_decode(strings[0], self._hyper_synthesis(z_hat))
            return {"x_hat": self._synthesis(y_hat).clamp_(0, 1)}
        subs = stream_parse(ans.SPLIT_STREAM, strings[0], S, "substreams")
        z_hat = self.entropy_bottleneck.decompress(strings[1], shape)
        y_hat, state = self._gmm_decode_split(subs, self._hyper_synthesis(z_hat), device_decoder)
        x_hat = self._synthesis(y_hat).clamp_(0, 1)
        if check and state is not None:
            stream_check(ans.SPLIT_STREAM, state, subs)
        return {"x_hat": x_hat}


class Cheng2020Attention(Cheng2020Anchor):
    """cheng2020-attn: the anchor model with the simplified attention block after the second strided block and at the end of g_a, and
    first and after the second upsampling block of g_s."""

    @staticmethod
    def _build_transforms(N):
        RBWS, RBU, RB, AB = ResidualBlockWithStride, ResidualBlockUpsample, ResidualBlock, AttentionBlock
        g_a = nn.Sequential(RBWS(3, N, 2), RB(N, N), RBWS(N, N, 2), AB(N), RB(N, N), RBWS(N, N, 2), RB(N, N), conv3x3(N, N, stride=2), AB(N))
        g_s = nn.Sequential(AB(N), RB(N, N), RBU(N, N, 2), RB(N, N), RBU(N, N, 2), AB(N), RB(N, N), RBU(N, N, 2), RB(N, N),
                            subpel_conv3x3(N, 3, 2))
        return g_a, g_s
