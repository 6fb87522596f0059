"""The hyperprior baselines of the RD plot — ``bmshj2018-hyperprior`` (ScaleHyperprior) and ``mbt2018-mean`` (MeanScaleHyperprior) — on
the engine's own kernels: CompressAI's ``conv(k=5, s=2)`` / ``deconv(k=5, s=2)`` layers run on csrc/conv5.hip, GDN / IGDN, the entropy
models, the rANS coder and the RD loss are the ones CLC and TCM use.

Written from CompressAI's published model definitions (layer order, hence the ``nn.Sequential`` indexes and ``state_dict`` keys;
``abs(y)`` into ``h_a`` of the scale-only model; ReLU there, LeakyReLU in the mean-scale model; ``chunk(2, 1)`` into scales and means),
so CompressAI checkpoints load.  CompressAI itself is not a dependency and nothing here is pinned against it: like the leaves, these
models are checked against a plain-torch restatement of the same definitions (tests/hyperprior_ref.py).

They train through plain autograd and code through the model methods; TrainEngine, graphed_training, CodecEngine and ReferenceBank
do not take them.  ``mbt2018`` and ``mbt2018-checkerboard`` on the lanes stream have a batched service of their own,
clc_amd.codec.ContextCodecEngine (one captured graph per compress / decompress): its plans run the pass code below on a
PassSchedule they keep — the pixel list, the chain's workspace, the stream's gather index and segment list, everything a pass would
otherwise upload or allocate per call.  The plain hyperpriors have no such service.  The host side of the context-model coders —
the start of a decoder's pass loop, the symbols of a host-decoded step, the result item — is coding.py's; ``mbt2018`` and ``mbt2018-checkerboard`` each state their schedule once (_ar_passes, _ckbd_passes) and
share one encoder loop and one decoder loop over it (_encode_passes, _decode_passes / _decode_from).

THE LANES STREAM (``compress(x, lanes=W)`` / ``decompress(..., lanes=W)``; DESIGN 27, include/clc_hip.h, clc_amd/ans.py) is opt-in and
shared by both models: the y string becomes the CLN1 container cut by the model's dependent steps — mbt2018's wavefront steps
(ar_lanes_order), the checkerboard's two passes (_ckbd_order) — and _decode_lanes decodes it on the device, per step the chain and ONE
clc_ar_lanes_decode, with no download and no synchronize.  With lanes=None nothing of it runs.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from .. import ans, ops
from ..entropy_models import EntropyBottleneck, GaussianConditional
from ..layers import GDN, CheckerboardMaskedConv2d, Conv2d, MaskedConv2d, conv, deconv
from ..ops import ACT_LRELU, ACT_NONE, ACT_RELU, CL
from ..intnet import (IntegerContextParameters, IntegerHyperSynthesis, check_channels, check_context_channels, choose_f0, context_spec_hash,
                      convert, convert_context_model, int_quantize, refuse_integer_context, refuse_integer_hyper)
from ..vbr import StepTable, model_step, refuse_rate_levels
from .clc import CompressionModel, _resize_registered_buffers, get_scale_table
from .coding import (CodeInputs, HostSymbols, coded_item, decoder_start, lanes_check, lanes_count, lanes_parse, lanes_strings, linear_filters,
                     open_decoders, refuse_lanes_strings, upload_streams)


class ScaleHyperprior(CompressionModel):
    """Balle et al. 2018, scale hyperprior: y ~ N(0, sigma(z)^2).

    BUILD-INDEPENDENT STREAMS (``integer_hyper=True``, ``exact=True``; DESIGN 32, clc_amd/intnet.py): the entropy parameters come from
    ``h_s_int``, an int8 restatement of ``h_s`` on the i8 matrix cores whose outputs are the same bits under every kernel state, build
    and machine, so a stream coded with ``exact=True`` decodes wherever the integers are — the quantiser, the scale index and the rANS
    coder downstream were build-independent already.  ``g_a``, ``h_a`` and ``g_s`` stay float: the first two run only in the encoder,
    and ``g_s``'s rounding moves the reconstruction by float noise across builds but cannot desynchronise the coder."""

    _h_act = ACT_RELU
    _h_slopes = (0.0, 0.0, 0.0)   # the negative-side slopes of h_s's three activations, for the integer net's conversion
    _h_split = False

    def __init__(self, N=128, M=192, rate_levels=0, integer_hyper=False, **kwargs):
        super().__init__(entropy_bottleneck_channels=N)
        self._check_channels(N, M)
        if integer_hyper:   # refused by name before anything is built
            check_channels(self._hyper_channels(N, M), type(self).__name__)
        rate_levels = int(rate_levels)
        if rate_levels < 0:
            raise ValueError(f"{type(self).__name__}: rate_levels must not be negative (got {rate_levels})")
        if rate_levels:   # VARIABLE RATE: a table of quantisation steps for y; without it no module and no state_dict key
            self.y_step = StepTable(M, rate_levels)
        self.g_a = nn.Sequential(conv(3, N), GDN(N), conv(N, N), GDN(N), conv(N, N), GDN(N), conv(N, M))
        self.g_s = nn.Sequential(deconv(M, N), GDN(N, inverse=True), deconv(N, N), GDN(N, inverse=True), deconv(N, N), GDN(N, inverse=True),
                                 deconv(N, 3))
        self._build_hyper(N, M)
        self.gaussian_conditional = GaussianConditional(None)
        self.N, self.M = int(N), int(M)
        if integer_hyper:   # zero-filled buffers of the right shapes, so that a checkpoint that holds them loads; without the flag
            self.h_s_int = IntegerHyperSynthesis(self._hyper_channels(N, M), split=self._h_split)   # no module and no state_dict key

    @staticmethod
    def _hyper_channels(N, M):
        """(Cin of h_s, its three layers' Cout)"""
        return (N, N, N, M)

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

    # ---- the integer parameter net ----
    def _exact_net(self, who):
        """h_s_int, filled; refused by name otherwise"""
        net = getattr(self, "h_s_int", None)
        if net is None:
            raise ValueError(f"{who}: exact needs the integer hyper-synthesis net — build the model with integer_hyper=True")
        net.require_ready(who)
        return net

    def _check_exact(self, exact, who):
        """exact of a decoder -> bool: None / False off; True on; an int is the spec_hash the stream was written under"""
        if exact is None or exact is False:
            return False
        mine = self._exact_hash(who)
        if exact is not True:
            if isinstance(exact, bool) or not isinstance(exact, (int, np.integer)):
                raise TypeError(f"{who}: exact must be True or the stream's spec_hash as an int (got {type(exact).__name__})")
            if int(exact) != mine:
                raise ValueError(f"{who}: the stream was written under integer net 0x{int(exact):08x}, this model's is 0x{mine:08x}")
        return True

    def _exact_hash(self, who):
        """the hash that names the model's integer entropy model; refused by name where it has none or it is not filled"""
        return self._exact_net(who).spec_hash()

    @torch.no_grad()
    def integerize(self, x_calib, f_out=8):
        """Post-training conversion of h_s into h_s_int (intnet.convert): runs the float model on the calibration images up to each h_s
        layer, records the largest |activation| after layers 1 and 2 and max|z_hat|, and fills the integer buffers -> spec_hash."""
        who = f"{type(self).__name__}.integerize"
        net = getattr(self, "h_s_int", None)
        if net is None:
            raise ValueError(f"{who}: the model has no integer hyper-synthesis net — build it with integer_hyper=True")
        x = self._prep(x_calib)
        z = self._hyper_analysis(self._analysis(x))
        z_hat = self.entropy_bottleneck(z, training=False)[0]
        a = self._h_act
        t1 = self.h_s[0](z_hat, act=a)
        t2 = self.h_s[2](t1, act=a)
        amax = [float(t1.abs().max()), float(t2.abs().max())]
        f0 = choose_f0(float(z_hat.abs().max()))
        layers = [self.h_s[0], self.h_s[2], self.h_s[4]]
        net.fill(convert([m.weight.detach().double().cpu().numpy() for m in layers], [m.bias.detach().double().cpu().numpy() for m in layers],
                         amax, self._h_slopes, f0, f_out), f0, f_out)
        return net.spec_hash()

    def _step(self, q, who):
        """the step vector of quality q from the model's step table (vbr.model_step: None for q None, refusals by name)"""
        return model_step(self, q, f"{type(self).__name__}.{who}")

    def forward(self, x, q=None, exact=False):
        """q: the quality, a float in [0, rate_levels - 1] (higher: finer steps, more bits); None: the fixed-rate model.  With q the
        eval x_hat is decoded from step * ste_round((y - mu) / step) + mu, so the distortion reaches the step table too.
        exact=True (eval / no_grad only: the integer net takes no gradient): the entropy parameters of h_s_int, what
        compress(exact=True) codes under."""
        step = self._step(q, "forward")
        net = None
        if exact:
            who = f"{type(self).__name__}.forward"
            if self.training:
                raise ValueError(f"{who}: exact=True is refused in training mode — the integer hyper-synthesis net takes no gradient (call model.eval())")
            net = self._exact_net(who)
        x = self._prep(x)
        y = self._analysis(x)
        z = self._hyper_analysis(y)
        z_hat, z_likelihoods = self.entropy_bottleneck(z)
        scales_hat, means_hat = self._params(z_hat) if net is None else net(z_hat)
        if step is None:
            y_hat, y_likelihoods = self.gaussian_conditional(y, scales_hat, means=means_hat)
        else:
            y_hat, y_likelihoods = self.gaussian_conditional(y, scales_hat, means=means_hat, step=step)
        x_hat = self._synthesis(y_hat)
        out = {"x_hat": x_hat, "likelihoods": {"y": y_likelihoods, "z": z_likelihoods}}
        if step is not None:
            out["q"] = q
        return out

    # ---- codec: one y stream and one z stream per image, on the host rANS coder ----
    def _zeros_like(self, t):
        return torch.zeros_like(t, memory_format=CL)

    def _encode_y(self, y, means, scales_hat, step):
        """the y strings of a batch under a step vector (None: the unit step)"""
        gc = self.gaussian_conditional
        cdf, ln, off = gc.host_tables()
        sym, idx, _ = gc.quantize_and_index(y, means, scales_hat) if step is None else gc.quantize_and_index(y, means, scales_hat, step=step)
        sym = sym.contiguous().cpu().numpy()   # [N, C, H, W]: the element order of CompressAI's symbols[i].reshape(-1)
        idx = idx.contiguous().cpu().numpy()
        return [ans.encode(sym[i].reshape(-1), idx[i].reshape(-1), cdf, ln, off) for i in range(sym.shape[0])]

    def rate_sweep(self, y, means, scales_hat, qs):
        """estimated bits of y per image under each quality of qs (at most 16) -> f32 [B, len(qs)] on the device: one
        ops.gauss_rate_sweep over the step vectors"""
        steps = torch.stack([self._step(q, "rate_sweep") for q in qs])
        return ops.gauss_rate_sweep(y, means, scales_hat, steps)

    def _compress_to_target(self, y, means, scales_hat, z_strings, target_bytes):
        """THE BYTE BUDGET: the finest of 16 evenly spaced qualities whose estimate plus the z bytes fits every image, then the encode;
        while an image's actual bytes exceed the target, the next coarser candidate — 16 encodes at most -> (y strings, q)"""
        who = f"{type(self).__name__}.compress"
        qs = self.y_step.candidates(16)
        z_bytes = np.array([len(s) for s in z_strings], dtype=np.float64)
        est = self.rate_sweep(y, means, scales_hat, qs).double().cpu().numpy() / 8.0 + z_bytes[:, None]   # [B, 16] bytes
        fits = (est <= target_bytes).all(axis=0)
        k = int(np.nonzero(fits)[0].max()) if fits.any() else 0
        while True:
            y_strings = self._encode_y(y, means, scales_hat, self._step(qs[k], "compress"))
            sizes = [len(a) + len(b) for a, b in zip(y_strings, z_strings)]
            if max(sizes) <= target_bytes:
                return y_strings, qs[k]
            if k == 0:
                raise ValueError(f"{who}: target_bytes={target_bytes} is out of reach: at the coarsest step (q=0) the images take "
                                 f"{sizes} bytes, of which z takes {[len(s) for s in z_strings]}")
            k -= 1

    @torch.no_grad()
    def compress(self, x, q=None, target_bytes=None, exact=False):
        """q: the quality (see forward); target_bytes=T: the finest quality at which y and z of EVERY image of the batch fit T bytes
        together (the chosen q is in the result; ValueError naming the sizes if the coarsest does not fit).  The result carries "q"
        when a step was used; pass it to decompress.  exact=True: the entropy parameters of the integer net h_s_int — a stream that
        is not tied to this build; the result carries "exact": spec_hash, pass it to decompress (codec.pack_item writes version 4)."""
        who = f"{type(self).__name__}.compress"
        net = self._exact_net(who) if exact else None
        if q is not None and target_bytes is not None:
            raise ValueError(f"{who}: q and target_bytes exclude each other (got q={q!r}, target_bytes={target_bytes!r})")
        if target_bytes is not None:
            if isinstance(target_bytes, bool) or not isinstance(target_bytes, int) or target_bytes < 1:
                raise ValueError(f"{who}: target_bytes must be a positive int, the bytes of one image (got {target_bytes!r})")
            if getattr(self, "y_step", None) is None:
                raise ValueError(f"{who}: target_bytes={target_bytes} needs a step table — build the model with rate_levels > 0")
        step = self._step(q, "compress")
        x = self._prep(x)
        y = self._analysis(x)
        z = self._hyper_analysis(y)
        z_strings = self.entropy_bottleneck.compress(z)
        z_hat = self.entropy_bottleneck.decompress(z_strings, z.size()[-2:])
        scales_hat, means_hat = self._params(z_hat) if net is None else net(z_hat)
        means = means_hat if means_hat is not None else self._zeros_like(y)
        extra = {} if net is None else {"exact": net.spec_hash()}
        if target_bytes is not None:
            y_strings, q = self._compress_to_target(y, means, scales_hat, z_strings, target_bytes)
            return coded_item(y_strings, z_strings, z.size()[-2:], q=q, **extra)
        y_strings = self._encode_y(y, means, scales_hat, step)
        if step is not None:
            extra["q"] = q
        return coded_item(y_strings, z_strings, z.size()[-2:], **extra)

    @torch.no_grad()
    def decompress(self, strings, shape, q=None, exact=None):
        """exact: True, or the "exact" hash of the compress result (a hash that is not this model's raises ValueError naming both)"""
        return {"x_hat": self._synthesis(self._decode_y_hat(strings, shape, q, exact)).clamp_(0, 1)}

    @torch.no_grad()
    def _decode_y_hat(self, strings, shape, q=None, exact=None):
        """the part of decompress before g_s -> y_hat"""
        step = self._step(q, "decompress")
        exact = self._check_exact(exact, f"{type(self).__name__}.decompress")
        assert isinstance(strings, (list, tuple)) and len(strings) == 2
        z_hat = self.entropy_bottleneck.decompress(strings[1], shape)
        scales_hat, means_hat = self.h_s_int(z_hat) if exact else self._params(z_hat)
        gc = self.gaussian_conditional
        cdf, ln, off = gc.host_tables()
        idx = (gc.build_indexes(scales_hat) if step is None else gc.build_indexes(scales_hat, step=step)).contiguous().cpu().numpy()
        out = np.empty(idx.shape, dtype=np.float32)
        for i, s in enumerate(strings[0]):
            out[i] = ans.decode(s, idx[i].reshape(-1), cdf, ln, off).reshape(idx.shape[1:])
        y_hat = torch.from_numpy(out).to(z_hat.device).contiguous(memory_format=CL)
        if step is not None:   # the encoder's expression: a rounded multiply, then a rounded add
            y_hat = y_hat * step.reshape(1, -1, 1, 1)
        if means_hat is not None:
            y_hat = y_hat + means_hat
        return y_hat

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
    _h_slopes = (0.01, 0.01, 1.0)   # the last layer is linear
    _h_split = True

    @staticmethod
    def _hyper_channels(N, M):
        return (N, M, M * 3 // 2, M * 2)

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


def ar_lanes_order(H, W):
    """THE PIXEL ORDER of mbt2018's lanes stream, as raster positions h * W + w -> int64 [H * W]: the non-empty steps of
    ar_schedule(H, W, "wavefront") in ascending t, inside a step its pixels in list order (ascending h).  The stream's segments are
    those steps (JointAutoregressiveHierarchicalPriors._lanes_segments); channels are inner."""
    return np.array([h * int(W) + w for step in ar_schedule(H, W, "wavefront") for h, w in step], dtype=np.int64)


def ckbd_lists(H, W, dev):
    """(number of anchors, number of non-anchors, the uploaded pixel list: anchors first)"""
    anchors, others = ckbd_pixels(H, W)
    return len(anchors), len(others), torch.tensor(anchors + others, dtype=torch.int32).reshape(-1, 2).to(dev)


def ckbd_pixels(H, W):
    """(anchors, non-anchors) of an H x W latent under the checkerboard context model, each a raster-ordered list of (h, w): anchors are
    the pixels with (h + w) odd, coded from the hyperprior alone; non-anchors ((h + w) even, (0, 0) among them) are coded from the
    hyperprior and the 12 (kh + kw)-odd taps of the 5x5 window, every one of which is an anchor or outside the map."""
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError(f"ckbd_pixels: H and W must be positive (got {H}, {W})")
    anchors = [(h, w) for h in range(H) for w in range(W) if (h + w) & 1]
    others = [(h, w) for h in range(H) for w in range(W) if not (h + w) & 1]
    return anchors, others


class PassSchedule:
    """What the passes of a context model over a [B, M, H, W] latent need besides the latent and the weights, made ONCE and outside any
    graph capture (every entry is an upload or an allocation): ``steps``, the non-empty steps in order, each a list of (h, w);
    ``pix``, their pixels back to back as the device's int32 [P, 2]; ``ws``, the chain's workspace for the largest step; ``ctx0``, the
    checkerboard's zero context map (read only; None for mbt2018).  A model's own call makes one per call (_pass_schedule), a
    ContextCodecEngine plan keeps one for its graph's lifetime.
    ``_lanes_schedule`` adds what the lanes stream is cut by: ``segments`` (_lanes_segments), ``order`` (_lanes_order as the device's
    int64 gather index) and ``seg_dev`` (the segments as the device's int32 list, for clc_rans_lanes_encode_list)."""

    segments = order = seg_dev = ctx0 = None

    def __init__(self, shape, steps, pix, ws):
        self.shape, self.steps, self.pix, self.ws = shape, steps, pix, ws   # shape: (B, H, W, device)

    def check(self, y_hat):
        B, _, H, W = y_hat.shape
        if self.shape != (B, H, W, y_hat.device):
            raise ValueError(f"the schedule was made for (B, H, W, device) = {self.shape}, the latent is {(B, H, W, y_hat.device)}")
        return self


class JointAutoregressiveHierarchicalPriors(CodeInputs, MeanScaleHyperprior):
    """Minnen et al. 2018 with the context model (``mbt2018``): the mean-scale hyperprior plus a masked 5x5 convolution over the coded
    latent and a three-layer 1x1 ``entropy_parameters`` net on cat((hyper parameters, context)).

    forward runs the full-map kernels.  The coder is sequential in the latent: per pixel, gather the 12 live taps -> M -> 2M -> (with the
    pixel's hyper parameters) 4M -> 10M/3 -> 8M/3 -> 2M -> quantise / index, on the row kernels of csrc/ar_context.hip, whose summation
    order depends on K alone — an encoder step of many pixels and a decoder step of one give the same bits.  compress runs the
    wavefront schedule (W + 3 (H - 1) steps) and serialises in CompressAI's raster-pixel, channel-inner order; decompress must follow the
    stream, one raster pixel at a time for the whole batch."""

    def __init__(self, N=192, M=192, **kwargs):
        refuse_rate_levels(type(self).__name__, kwargs)   # the context models code y under the unit step only
        refuse_integer_hyper(type(self).__name__, kwargs)   # their parameters depend on the coded y too: the checkerboard model has
        refuse_integer_context(type(self).__name__, kwargs)   # integer_context, a keyword of its own; mbt2018 is a follow-up
        if M % 12:
            raise ValueError(f"{type(self).__name__} needs M % 12 == 0 (then 10M/3, 8M/3 and 3M/2 are whole and multiples of 4, the "
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
        return [(wc, cp.bias.detach().contiguous())] + linear_filters(ep)

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

    def _ar_walk(self, steps, pix, y_hat, params, ws, filt):
        """One walk over the steps of a schedule, for encoders and decoders alike: per step the chain over its pixels, then
        (pixels of the step, its pixel list, its (scales | means) rows) to the caller's body, which finishes the step into y_hat
        before the next one reads it.  One slice per step and nothing else on the host: mbt2018's decoder takes one step per pixel."""
        (B, _, H, W), gp, off = y_hat.shape, ws["gp"], 0
        for s in steps:
            cnt = len(s)
            px = pix[off:off + cnt]
            off += cnt
            self._ar_chain(px, B, H, W, y_hat, params, ws, filt)
            yield cnt, px, gp

    def _pass_schedule(self, B, H, W, dev, order="wavefront"):
        """the PassSchedule of ar_schedule(H, W, order): the pixel list's upload and the workspace's allocation, in one place"""
        steps, pix = self._ar_pixels(ar_schedule(H, W, order), dev)
        return PassSchedule((B, H, W, dev), steps, pix, self._ar_workspace(B * max(len(s) for s in steps), dev))

    def _ar_passes(self, params, y_hat, order, sched=None):
        """THE SCHEDULE of mbt2018: the non-empty steps of ar_schedule(H, W, order).  The encoder takes whole wavefront steps, the
        decoder must follow the stream: one raster pixel per step.  sched: the caller's PassSchedule of that order (default: made
        here, for this call); with one, the walk uploads and allocates nothing."""
        B, _, H, W = y_hat.shape
        sched = self._pass_schedule(B, H, W, y_hat.device, order) if sched is None else sched.check(y_hat)
        return self._ar_walk(sched.steps, sched.pix, y_hat, params, sched.ws, self._ar_filters())

    @torch.no_grad()
    def _encode_passes(self, who, y, params, passes, *schedule):
        """The encoder of a table-coded model over its schedule ``passes(params, y_hat, *schedule)`` -> (symbols int32 [B, H*W, M],
        indexes int32 [B, H*W, M], y_hat): all launches on the current stream, no host sync.  The schedule decides the order of
        computation only; the buffers are in raster order either way."""
        ops._require_gpu(y, f"{who} compress")
        B, M, H, W = y.shape
        y = y.contiguous(memory_format=CL)
        params = params.contiguous(memory_format=CL)
        table = self.gaussian_conditional.scale_table
        y_hat = torch.zeros_like(y, memory_format=CL)
        sym = torch.empty((B, H * W, M), device=y.device, dtype=torch.int32)
        idx = torch.empty((B, H * W, M), device=y.device, dtype=torch.int32)
        for _, px, gp in passes(params, y_hat, *schedule):
            ops.ar_finish_encode(gp, M, px, y, y_hat, table, sym, idx)
        return sym, idx, y_hat

    @torch.no_grad()
    def _decode_passes(self, y_strings, params, most, passes, *schedule):
        """The decoder of a table-coded model over its schedule -> y_hat: per step one index download, one incremental decode per
        image on a decoder opened once, one symbol upload.  most: the pixels of the schedule's largest step."""
        params, y_hat = decoder_start(params, len(y_strings), self.M)
        B, M, H, W = y_hat.shape
        src = HostSymbols([d.decode_stream for d in open_decoders(y_strings)], self.gaussian_conditional.host_tables(), B * most * M, y_hat.device)
        return self._decode_from(src, params, y_hat, passes, *schedule)

    def _decode_from(self, src, params, y_hat, passes, *schedule):
        """The decoder's loop over a source of symbols with a hop per step (coding.HostSymbols over one-stream or lanes decoders;
        coding.DeviceLanesSymbols fits too): per step the chain, ar_finish_decode, the source's step and ar_commit -> y_hat."""
        B, M, H, W = y_hat.shape
        table = self.gaussian_conditional.scale_table
        cut = None
        for cnt, px, gp in passes(params, y_hat, *schedule):
            if cnt != cut:   # the views are cut when the step's size changes: once for mbt2018's pixel per step, whatever the latent
                cut, (idx, sym) = cnt, src.views(B * cnt, M)
            ops.ar_finish_decode(gp, M, px, B, H, W, table, idx)
            src.decode(idx, sym, cnt * M)
            ops.ar_commit(sym, gp, M, px, y_hat)
        return y_hat

    def _ar_encode(self, y, params, order="wavefront"):
        """The autoregressive pass of compress: _encode_passes over the steps of ``order``"""
        return self._encode_passes("mbt2018", y, params, self._ar_passes, order)

    # ---- the lanes stream: its order and segments (one owner each per model), the encoder's tail, the decoder's loop ----
    _lanes_order = staticmethod(ar_lanes_order)
    _lanes_encoder = staticmethod(ops.rans_lanes_encode_list)   # a wavefront has more segments than clc_rans_lanes_encode takes by value

    def _lanes_segments(self, H, W):
        """the lanes stream's segments: the non-empty wavefront steps in ar_lanes_order, n = pixels of the step x M"""
        return [len(s) * self.M for s in ar_schedule(H, W, "wavefront") if s]

    def _lanes_passes(self, params, y_hat, sched=None):
        """the schedule the lanes stream is cut by: the decoder runs the wavefront too"""
        return self._ar_passes(params, y_hat, "wavefront", sched)

    def _lanes_schedule(self, B, H, W, dev):
        """the PassSchedule of _lanes_passes with the stream's cut: segments, the gather index of _lanes_order and the segments' device
        list, each uploaded here"""
        sched = self._pass_schedule(B, H, W, dev)
        sched.segments = self._lanes_segments(H, W)
        sched.order = torch.from_numpy(self._lanes_order(H, W)).to(dev)
        sched.seg_dev = torch.tensor(sched.segments, dtype=torch.int32).to(dev)
        return sched

    def _lanes_encoder_keywords(self, sched):
        """what the model's lanes encoder takes from a schedule: clc_rans_lanes_encode_list reads its lengths from device memory"""
        return {"segments_dev": sched.seg_dev}

    def _lanes_encode(self, y, params, sched):
        """_encode_passes over _lanes_passes on the caller's schedule: the encoder as a captured graph runs it"""
        return self._encode_passes(type(self).__name__, y, params, self._lanes_passes, sched)

    @staticmethod
    def _lanes_most(H, W):
        """the pixels of the largest step"""
        return max(len(s) for s in ar_schedule(H, W, "wavefront"))

    def _lanes_launch(self, sym, idx, segments, W, header=None, **keywords):
        """int32 [B, T] device symbols / indexes in stream order -> (packed words, header [B W + 1]) on the device: one launch of the
        model's lanes encoder and one clc_rans_lanes_pack for the batch.  keywords: the encoder's regions / regions_dev /
        segments_dev; without them it derives and uploads them, which a capture cannot."""
        gc = self.gaussian_conditional
        out, _, result = self._lanes_encoder(sym, idx, segments, W, (gc._quantized_cdf, gc._cdf_length, gc._offset), **keywords)
        return ops.rans_lanes_pack(out, result, header=header)

    def _lanes_encode_device(self, sym, idx, segments, W):
        """int32 [B, T] device symbols / indexes in stream order -> per image its lanes string: _lanes_launch, then two device -> host
        copies (the header, the packed words)."""
        B = sym.shape[0]
        packed, header = self._lanes_launch(sym, idx, segments, W)
        head = header.cpu().numpy()
        words = packed[:int(head[B * W])].cpu().numpy() if (head[:B * W] >= 0).all() else np.zeros(0, np.int32)
        return lanes_strings(head, words, B, W)   # (raises by name on a negative code)

    @staticmethod
    def _lanes_gather(t, order):
        """_encode_passes' raster [B, H*W, M] buffer -> [B, T] in stream order, by the device's index tensor"""
        return t.index_select(1, order).reshape(t.shape[0], -1)

    def _lanes_y_strings(self, sym, idx, H, W, Wn):
        """_encode_passes' raster [B, H*W, M] buffers -> the lanes strings: gathered into stream order on the device by one index tensor"""
        order = torch.from_numpy(self._lanes_order(H, W)).to(sym.device)
        return self._lanes_encode_device(self._lanes_gather(sym, order), self._lanes_gather(idx, order), self._lanes_segments(H, W), Wn)

    def _lanes_pack_scheduled(self, sym, idx, sched, W, regions, regions_dev, header):
        """_lanes_y_strings' device half on a caller's schedule and regions (ops.rans_lanes_regions and their device copy): the gather,
        the encoder and the pack with nothing uploaded, allocated on the host or read back -> (packed words, header)"""
        return self._lanes_launch(self._lanes_gather(sym, sched.order), self._lanes_gather(idx, sched.order), sched.segments, W, header=header,
                                  regions=regions, regions_dev=regions_dev, **self._lanes_encoder_keywords(sched))

    @torch.no_grad()
    def _decode_lanes(self, subs, params, device_coder=True):
        """The decoder over lanes streams (subs[b][w]: bytes), for both models -> (y_hat, state).
        device_coder: one pinned upload of every wave stream's states, spans and words, then per step of _lanes_passes the chain and ONE
        clc_ar_lanes_decode — stream-ordered launches only, no download, no synchronize, no per-image loop; state is the device's
        int32 [B, W, 130] (64 x (x low, x high), pos, pad) as the last step left it.
        Host coder: _decode_from with one ans.LanesDecoder per image, a hop per step; state is the list of decoders."""
        params, y_hat = decoder_start(params, len(subs), self.M)
        B, M, H, W = y_hat.shape
        gc = self.gaussian_conditional
        if not device_coder:
            decoders = [ans.LanesDecoder(img) for img in subs]
            src = HostSymbols([d.decode for d in decoders], gc.host_tables(), B * self._lanes_most(H, W) * M, y_hat.device, state=decoders)
            return self._decode_from(src, params, y_hat, self._lanes_passes), decoders
        state, spans, words = upload_streams(subs, 2 * ans.LANES, y_hat.device)   # a wave stream starts with its 64 lane states
        return self._lanes_decode_pass(params, y_hat, (state, spans, words)), state

    def _lanes_decode_pass(self, params, y_hat, streams, sched=None):
        """The device decoder's pass over the caller's (state, spans, words) views of an uploaded coding.stream_image -> y_hat: per step
        of _lanes_passes the chain and ONE clc_ar_lanes_decode; state is advanced in place.  params, y_hat: decoder_start's.  With a
        schedule the pass is launches only — what a graph captures."""
        B, M, H, W = y_hat.shape
        gc = self.gaussian_conditional
        tables, table = (gc._quantized_cdf, gc._cdf_length, gc._offset), gc.scale_table
        state, spans, words = streams
        for _, px, gp in self._lanes_passes(params, y_hat, sched):
            ops.ar_lanes_decode(gp, M, px, B, H, W, table, tables, words, spans, state, y_hat)
        return y_hat

    @torch.no_grad()
    def _decompress_lanes(self, strings, shape, Wn, device_coder, check, params_of=None):
        """params_of: z_hat -> what the passes read as the hyper parameters (default: the float h_s)"""
        subs = lanes_parse(strings[0], Wn)   # the headers, before any device work
        if len(subs) != len(strings[1]):
            raise ValueError(f"decompress: {len(subs)} y streams for {len(strings[1])} z streams")
        z_hat = self.entropy_bottleneck.decompress(strings[1], shape)
        y_hat, state = self._decode_lanes(subs, (params_of or self._hyper_synthesis)(z_hat), device_coder)
        x_hat = self._synthesis(y_hat).clamp_(0, 1)
        if check:
            lanes_check(state, subs)
        return {"x_hat": x_hat}

    @torch.no_grad()
    def compress(self, x, order="wavefront", lanes=None):
        """order: the encoder's schedule of computation only; the bytes do not depend on it.  lanes=None: CompressAI's raster stream.
        lanes=W: THE LANES STREAM (clc_amd/ans.py: lanes_pack; include/clc_hip.h), W wave streams of 64 rANS lanes per image cut by
        wavefront steps, encoded on the device, and "lanes": W in the result; pass the same W to decompress."""
        Wn = lanes_count(lanes, f"{type(self).__name__}.compress")
        y, params, z_strings, z_size = self._code_inputs(x)
        sym, idx, _ = self._ar_encode(y, params, order)
        if Wn is not None:   # the buffers stay on the device
            return coded_item(self._lanes_y_strings(sym, idx, y.shape[2], y.shape[3], Wn), z_strings, z_size, lanes=Wn)
        cdf, ln, off = self.gaussian_conditional.host_tables()
        both = torch.stack((sym, idx)).cpu().numpy()   # the one device -> host copy: [2, B, H*W, M], raster pixels, channels inner
        y_strings = [ans.encode(both[0, i].reshape(-1), both[1, i].reshape(-1), cdf, ln, off) for i in range(both.shape[1])]
        return coded_item(y_strings, z_strings, z_size)

    @torch.no_grad()
    def decompress(self, strings, shape, lanes=None, device_coder=True, check=True):
        """lanes=None: the one-stream format, one hop per raster pixel.  lanes=W: the lanes stream of compress(x, lanes=W); its headers
        are parsed on the host before any device work.  device_coder=True decodes it on the device, W + 3 (H - 1) wavefront steps of
        the chain and one clc_ar_lanes_decode each: no device -> host copy and no synchronize between the upload of the streams and the
        finished y_hat; check=True adds ONE download of the final coder states, after the synthesis transform has been launched, and
        raises ValueError naming the image and the wave streams that did not end where a whole stream ends (a check against streams
        out of step or cut short, not a checksum).  device_coder=False runs the same format on the host coder (ans.LanesDecoder), a
        hop per step: the oracle and the fallback."""
        Wn = lanes_count(lanes, f"{type(self).__name__}.decompress")
        assert isinstance(strings, (list, tuple)) and len(strings) == 2
        if Wn is not None:
            return self._decompress_lanes(strings, shape, Wn, device_coder, check)
        refuse_lanes_strings(strings[0])
        z_hat = self.entropy_bottleneck.decompress(strings[1], shape)
        y_hat = self._decode_passes(strings[0], self._hyper_synthesis(z_hat), 1, self._ar_passes, "raster")
        return {"x_hat": self._synthesis(y_hat).clamp_(0, 1)}


class JointCheckerboardHierarchicalPriors(JointAutoregressiveHierarchicalPriors):
    """The checkerboard context model of He et al. (CVPR 2021) on the ``mbt2018`` architecture: the same g_a / g_s / h_a / h_s, the same
    ``entropy_parameters`` and the same ``state_dict`` keys, with ``context_prediction`` a CheckerboardMaskedConv2d (csrc/ckbd_context.hip).
    Half of the latent pixels — the anchors, (h + w) odd — are coded from the hyperprior alone, the other half from the hyperprior plus a
    5x5 convolution over the anchors only: encoder and decoder both take two parallel passes, whatever the image size.

    forward is a single pass in training and in eval: the layer reads anchors only and returns 0 at anchors, which equals the usual "zero
    the non-anchors, convolve, zero the anchors' outputs".

    The coder.  Pass 1 runs the three 1x1 layers on the anchor list with a zero context map (fmaf(0, w, acc) == acc, so the zero range
    changes nothing) and finishes the anchors; pass 2 evaluates the context layer over the whole map in one launch and runs the same
    layers on the non-anchor list.  The 1x1 layers run on clc_ar_linear, whose summation order is a function of K alone; the context
    layer on ckbd_conv_kernel, whose order is a function of Cin alone; h_s on the batch-invariant kernels: a stream written at batch 8
    decodes at batch 1.

    STREAM ORDER: one rANS stream per image for y — all anchors in raster order, then all non-anchors in raster order, channels inner;
    z as in the other hyperprior models.  This is the project's own order: CompressAI is not a dependency and is not installed where
    this is built, so nothing here is pinned against its checkerboard classes.

    BUILD-INDEPENDENT STREAMS (``integer_context=True``, ``exact=True``; DESIGN 33, clc_amd/intnet.py): ``h_s_int`` (int8 output) and
    ``ctx_int`` restate the whole entropy model — h_s, the context layer over the int8-quantised y_hat, entropy_parameters — in int8 on
    the i8 matrix cores (csrc/int_conv.hip, csrc/int_rows.hip).  The passes, the stream formats and the device decoder are the same
    code; only the (scales | means) rows come from integer sums, the same bits under every kernel state, build and machine.  M must be
    a multiple of 192 and N of 32.  Without the flag: no new module, state_dict key, launch or byte."""

    def __init__(self, N=192, M=192, integer_context=False, **kwargs):
        if integer_context:   # refused by name before anything is built
            check_context_channels(N, M, type(self).__name__)
        super().__init__(N=N, M=M, **kwargs)
        self.context_prediction = CheckerboardMaskedConv2d(M, 2 * M, kernel_size=5, padding=2, stride=1)
        if integer_context:   # zero-filled until integerize / load_state_dict; without the flag no module and no state_dict key
            self.h_s_int = IntegerHyperSynthesis(self._hyper_channels(N, M), int8_out=True)
            self.ctx_int = IntegerContextParameters(M)

    def _ar_encode(self, y, params, order="wavefront"):
        raise NotImplementedError("JointCheckerboardHierarchicalPriors has no autoregressive pass (mask A): the coder is _ckbd_encode / _ckbd_decode")

    # ---- BUILD-INDEPENDENT STREAMS (integer_context=True, exact=True): h_s_int's int8 psi map and ctx_int's chain ----
    def _exact_net(self, who):
        """(h_s_int, ctx_int), both filled; refused by name otherwise"""
        hs, cx = getattr(self, "h_s_int", None), getattr(self, "ctx_int", None)
        if hs is None or cx is None:
            raise ValueError(f"{who}: exact needs the integer context net — build the model with integer_context=True")
        hs.require_ready(who)
        cx.require_ready(who)
        return hs, cx

    def _exact_hash(self, who):
        return context_spec_hash(*self._exact_net(who))

    def spec_hash(self):
        """the u32 that names the integer entropy model (intnet.context_spec_hash)"""
        return self._exact_hash(f"{type(self).__name__}.spec_hash")

    def _psi(self, z_hat):
        """h_s_int's int8 psi as the passes take their hyper parameters: a channels-last [B, 2M, H, W] view of the NHWC map"""
        return self.h_s_int(z_hat).permute(0, 3, 1, 2)

    @torch.no_grad()
    def integerize(self, x_calib, f_out=8):
        """Post-training conversion of the whole entropy model (intnet.convert_context_model): runs the float coder's two passes on the
        calibration images, records max|z_hat|, max|y_hat| and each layer's largest post-activation value — psi and the context
        layer's output jointly — and fills h_s_int and ctx_int -> the hash."""
        who = f"{type(self).__name__}.integerize"
        if getattr(self, "ctx_int", None) is None:
            raise ValueError(f"{who}: the model has no integer context net — build it with integer_context=True")
        x = self._prep(x_calib)
        y = self._analysis(x)
        z_hat = self.entropy_bottleneck(self._hyper_analysis(y), training=False)[0]
        a = self._h_act
        t1 = self.h_s[0](z_hat, act=a)
        t2 = self.h_s[2](t1, act=a)
        params = self.h_s[4](t2)
        amax = {"hs1": float(t1.abs().max()), "hs2": float(t2.abs().max()), "psi": float(params.abs().max()), "ep1": 0.0, "ep2": 0.0}
        B, _, H, W = y.shape
        sched = self._pass_schedule(B, H, W, y.device)

        def passes(params, y_hat):
            for cnt, px, gp in self._ckbd_passes(params, y_hat, sched):
                for k, name in (("ep1", "h1"), ("ep2", "h2")):
                    amax[k] = max(amax[k], float(sched.ws[name][:B * cnt].abs().max()))
                yield cnt, px, gp

        _, _, y_hat = self._encode_passes(who, y, params, passes)
        amax["ctx"] = float(self.context_prediction(y_hat).abs().max())   # (the layer returns 0 at anchors)
        np64 = lambda t: t.detach().double().cpu().numpy()
        hs = [(np64(m.weight), np64(m.bias)) for m in (self.h_s[0], self.h_s[2], self.h_s[4])]
        ep = [(np64(w), np64(b)) for w, b in linear_filters(self.entropy_parameters)]
        cp = self.context_prediction
        hs_layers, ctx_layers, f0, f_y, f_out = convert_context_model(hs, (np64(cp.weight), np64(cp.bias)), ep, amax, float(z_hat.abs().max()),
                                                                      float(y_hat.abs().max()), self._h_slopes, f_out)
        self.h_s_int.fill(hs_layers, f0, f_out)
        self.ctx_int.fill(ctx_layers, f_y, f_out)
        return self.spec_hash()

    def forward(self, x, exact=False):
        """exact=True (eval / no_grad only): the likelihoods under the coder's own two-pass integer parameters — the (scales | means)
        rows of both passes scattered back to a map — and x_hat from the coder's y_hat: the rate of the stream compress(exact=True)
        writes."""
        if not exact:
            return super().forward(x)
        who = f"{type(self).__name__}.forward"
        if self.training:
            raise ValueError(f"{who}: exact=True is refused in training mode — the integer context net takes no gradient (call model.eval())")
        self._exact_net(who)
        with torch.no_grad():
            x = self._prep(x)
            y = self._analysis(x)
            z_hat, z_likelihoods = self.entropy_bottleneck(self._hyper_analysis(y))
            B, M, H, W = y.shape
            gp_map = torch.empty((B, H, W, 2 * M), device=y.device, dtype=torch.float32)

            def passes(params, y_hat):
                for cnt, px, gp in self._ckbd_passes(params, y_hat):
                    gp_map[:, px[:, 0].long(), px[:, 1].long()] = gp[:B * cnt].view(B, cnt, 2 * M)
                    yield cnt, px, gp

            _, _, y_hat = self._encode_passes(who, y, self._psi(z_hat), passes)
            scales_hat, means_hat = gp_map.permute(0, 3, 1, 2).chunk(2, 1)
            _, y_likelihoods = self.gaussian_conditional(y, scales_hat, means=means_hat)
            return {"x_hat": self._synthesis(y_hat), "likelihoods": {"y": y_likelihoods, "z": z_likelihoods}}

    # ---- the two-pass coder ----
    _ckbd_lists = staticmethod(ckbd_lists)

    def _ckbd_workspace(self, rows, dev):
        M = self.M
        mk = lambda c: torch.empty((rows, c), device=dev, dtype=torch.float32)
        return {"h1": mk(M * 10 // 3), "h2": mk(M * 8 // 3), "gp": mk(2 * M)}

    def _ckbd_chain(self, px, B, H, W, params, ctx_map, ws, filt):
        """(scales | means) of the listed pixels of every image -> ws["gp"]; three launches.  filt: _ckbd_filters()"""
        ops.ar_linear([("pixel", params), ("pixel", ctx_map)], px, B, H, W, filt[0][0], filt[0][1], ws["h1"], act=ACT_LRELU)
        ops.ar_linear([("dense", ws["h1"])], px, B, H, W, filt[1][0], filt[1][1], ws["h2"], act=ACT_LRELU)
        ops.ar_linear([("dense", ws["h2"])], px, B, H, W, filt[2][0], filt[2][1], ws["gp"])

    def _ckbd_filters(self):
        return linear_filters(self.entropy_parameters)

    def _pass_schedule(self, B, H, W, dev, exact=False):
        """the PassSchedule of the two passes: the pixel list's upload, the workspace and the zero context map, in one place.
        exact: the integer chain's int8 workspace instead, and no zero map — an anchor pass has no context range"""
        anchors, others = ckbd_pixels(H, W)
        na, nn_, pix = self._ckbd_lists(H, W, dev)
        rows = B * max(na, nn_)
        sched = PassSchedule((B, H, W, dev), [s for s in (anchors, others) if s], pix,
                             self.ctx_int.workspace(rows, dev) if exact else self._ckbd_workspace(rows, dev))
        if not exact:
            sched.ctx0 = torch.zeros((B, 2 * self.M, H, W), device=dev, dtype=torch.float32).contiguous(memory_format=CL)
        return sched

    def _ckbd_passes(self, params, y_hat, sched=None):
        """THE SCHEDULE of the checkerboard model, for encoder and decoder alike: the anchors, then the non-anchors; an empty pass is
        skipped.  Pass 1 reads a zero context map, pass 2 the context layer over the anchors that pass 1 committed.  Per pass the
        chain, then (pixels of the pass, its pixel list, its (scales | means) rows) to the caller's body.  sched: the caller's
        PassSchedule (default: made here, for this call); with one, the passes upload and allocate nothing but the context map.
        THE EXACT PATH (params is _psi's int8 map): ctx_int's integer chain writes the same f32 rows in place of _ckbd_chain, and the
        int8 quantised y_hat stands in place of context_prediction; a pass is an anchor pass or a non-anchor pass by its pixels'
        parity, so the single pass of a 1x1 latent evaluates the context layer (every tap off the map: its requantised bias)."""
        B, M, H, W = y_hat.shape
        exact = params.dtype == torch.int8
        sched = self._pass_schedule(B, H, W, y_hat.device, exact) if sched is None else sched.check(y_hat)
        pix, ws = sched.pix, sched.ws
        if exact:
            net, psi = self.ctx_int, params.permute(0, 2, 3, 1)
        else:
            filt = self._ckbd_filters()
        lo = 0
        for s in sched.steps:
            cnt = len(s)
            px = pix[lo:lo + cnt]
            if exact:
                anchor = (s[0][0] + s[0][1]) & 1
                net.chain(px, B, H, W, psi, None if anchor else int_quantize(y_hat, net.f_y), ws)
            else:
                ctx_map = self.context_prediction(y_hat) if lo else sched.ctx0   # (ctx0 is never written)
                self._ckbd_chain(px, B, H, W, params, ctx_map, ws, filt)
            lo += cnt
            yield cnt, px, ws["gp"]

    def _ckbd_encode(self, y, params):
        """The two passes of compress: _encode_passes over _ckbd_passes"""
        return self._encode_passes("mbt2018-checkerboard", y, params, self._ckbd_passes)

    @staticmethod
    def _ckbd_order(H, W):
        """raster positions h * W + w in the stream's order: anchors, then non-anchors"""
        anchors, others = ckbd_pixels(H, W)
        return np.array([h * W + w for h, w in anchors + others], dtype=np.int64)

    # ---- the lanes stream: two segments in _ckbd_order, today's symbol order; the tail and the decoder's loop are inherited ----
    _lanes_encoder = staticmethod(ops.rans_lanes_encode)

    @staticmethod
    def _lanes_order(H, W):
        return JointCheckerboardHierarchicalPriors._ckbd_order(H, W)

    def _lanes_segments(self, H, W):
        """the lanes stream's segments: the anchors, then the non-anchors, n = pixels of the pass x M"""
        anchors, others = ckbd_pixels(H, W)
        return [len(anchors) * self.M, len(others) * self.M]

    def _lanes_passes(self, params, y_hat, sched=None):
        return self._ckbd_passes(params, y_hat, sched)

    def _lanes_encoder_keywords(self, sched):
        return {}   # clc_rans_lanes_encode takes its two segments by value

    @staticmethod
    def _lanes_most(H, W):
        return (H * W + 1) // 2

    @torch.no_grad()
    def _exact_inputs(self, x):
        """_code_inputs with h_s_int's psi map in place of the float hyper parameters"""
        x = self._prep(x)
        y = self._analysis(x)
        z = self._hyper_analysis(y)
        z_strings = self.entropy_bottleneck.compress(z)
        z_hat = self.entropy_bottleneck.decompress(z_strings, z.size()[-2:])
        return y, self._psi(z_hat), z_strings, z.size()[-2:]

    @torch.no_grad()
    def compress(self, x, lanes=None, exact=False):
        """lanes=None: the one-stream format.  lanes=W: the lanes stream, the same symbols cut into the two passes as segments and encoded
        on the device; "lanes": W in the result; pass the same W to decompress.  exact=True: the entropy parameters of the integer
        nets — a stream that is not tied to this build, in either format; the result carries "exact": the hash, pass it to
        decompress (codec.pack_item writes version 4)."""
        who = f"{type(self).__name__}.compress"
        Wn = lanes_count(lanes, who)
        extra = {"exact": self._exact_hash(who)} if exact else {}
        y, params, z_strings, z_size = self._exact_inputs(x) if exact else self._code_inputs(x)
        sym, idx, _ = self._ckbd_encode(y, params)
        if Wn is not None:   # the buffers stay on the device
            return coded_item(self._lanes_y_strings(sym, idx, y.shape[2], y.shape[3], Wn), z_strings, z_size, lanes=Wn, **extra)
        cdf, ln, off = self.gaussian_conditional.host_tables()
        both = torch.stack((sym, idx)).cpu().numpy()   # the one device -> host copy: [2, B, H*W, M], raster pixels, channels inner
        order = self._ckbd_order(y.shape[2], y.shape[3])
        y_strings = [ans.encode(np.ascontiguousarray(both[0, i][order]).reshape(-1), np.ascontiguousarray(both[1, i][order]).reshape(-1), cdf, ln, off)
                     for i in range(both.shape[1])]
        return coded_item(y_strings, z_strings, z_size, **extra)

    def _ckbd_decode(self, y_strings, params):
        """The two passes of decompress -> y_hat: _decode_passes over _ckbd_passes, whose larger pass is the non-anchors ((0, 0) is one)"""
        return self._decode_passes(y_strings, params, (params.shape[2] * params.shape[3] + 1) // 2, self._ckbd_passes)

    @torch.no_grad()
    def decompress(self, strings, shape, lanes=None, device_coder=True, check=True, exact=None):
        """lanes, device_coder, check: as for mbt2018 (JointAutoregressiveHierarchicalPriors.decompress); the device decoder takes the
        two passes with one clc_ar_lanes_decode each.  exact: True, or the "exact" hash of the compress result (a hash that is not
        this model's raises ValueError naming both), on either stream format."""
        who = f"{type(self).__name__}.decompress"
        Wn = lanes_count(lanes, who)
        exact = self._check_exact(exact, who)
        assert isinstance(strings, (list, tuple)) and len(strings) == 2
        if Wn is not None:
            return self._decompress_lanes(strings, shape, Wn, device_coder, check, self._psi if exact else None)
        refuse_lanes_strings(strings[0])
        z_hat = self.entropy_bottleneck.decompress(strings[1], shape)
        y_hat = self._ckbd_decode(strings[0], self._psi(z_hat) if exact else self._hyper_synthesis(z_hat))
        return {"x_hat": self._synthesis(y_hat).clamp_(0, 1)}

    @torch.no_grad()
    def _decode_y_hat(self, strings, shape, lanes=None, exact=None, device_coder=True, check=True):
        """the part of decompress before g_s -> y_hat"""
        who = f"{type(self).__name__}.decompress"
        Wn = lanes_count(lanes, who)
        params_of = self._psi if self._check_exact(exact, who) else self._hyper_synthesis
        assert isinstance(strings, (list, tuple)) and len(strings) == 2
        if Wn is None:
            refuse_lanes_strings(strings[0])
            return self._ckbd_decode(strings[0], params_of(self.entropy_bottleneck.decompress(strings[1], shape)))
        subs = lanes_parse(strings[0], Wn)
        if len(subs) != len(strings[1]):
            raise ValueError(f"decompress: {len(subs)} y streams for {len(strings[1])} z streams")
        y_hat, state = self._decode_lanes(subs, params_of(self.entropy_bottleneck.decompress(strings[1], shape)), device_coder)
        if check:
            lanes_check(state, subs)
        return y_hat
