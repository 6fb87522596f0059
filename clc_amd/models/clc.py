"""CLC / TCM compression models on the MI355X engine — same surface as the reference classes.

Mirrors /root/reference/models/CLC_run.py:316-814 (CLC) and /root/reference/models/tcm.py:310-626 (TCM):
constructor signature, ``forward(x, ref_frames=None)`` output dict, ``compress`` / ``decompress`` /
``update`` / ``aux_loss`` / ``load_state_dict`` and every parameter / buffer name,
so ``train_CLC.py`` / ``eval_CLC.py`` can construct and drive it unchanged.

What is different underneath (MI355X-first, not a translation):
  * activations are channels_last (NHWC) end to end; ``y.chunk`` / ``split`` are strided views the kernels
    read through their leading dimension; no Rearrange/permute/roll/mask tensor is ever built;
  * the R reference images go through the shared ReferenceEncoder as ONE batched call;
  * per slice, likelihood + STE rounding is one kernel, the LRP head's ``0.5*tanh(.) + y_hat`` is the
    last conv's epilogue, GELU/LeakyReLU/ReLU/GDN/residual adds are conv epilogues;
  * compress(): symbols and CDF indexes come from one integer kernel per slice into int32 buffers, the CDF
    tables are copied to the host once per model (not ``.tolist()`` per call), and the C++ rANS coder works
    on those arrays directly.
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch
import torch.nn as nn

from .. import ans, graphed, ops
from ..entropy_models import EntropyBottleneck, GaussianConditional
from ..layers import (GELU, ConvTransBlock, Conv2d, ResidualBlockUpsample, ResidualBlockWithStride, SWAtten, conv1x1,
                      conv3x3, subpel_conv3x3)
from ..ops import ACT_GELU, ACT_HALFTANH, ACT_NONE, CL
from ..intnet import refuse_integer_hyper
from ..vbr import refuse_rate_levels
from . import coding

SCALES_MIN, SCALES_MAX, SCALES_LEVELS = 0.11, 256, 64
CODEC_GRAPH = os.environ.get("CLC_CODEC_GRAPH", "1") != "0"   # compress() / decompress() of one image on captured hipGraph segments
CODEC_GRAPH_PLANS = int(os.environ.get("CLC_CODEC_GRAPH_PLANS", "6"))   # captured image sizes kept per model and direction (LRU)


def get_scale_table(min=SCALES_MIN, max=SCALES_MAX, levels=SCALES_LEVELS):
    return torch.exp(torch.linspace(math.log(min), math.log(max), levels))


class SliceTransform(nn.Sequential):
    """conv3x3 -> GELU -> conv3x3 -> GELU -> conv3x3 (``cc_*`` / ``lrp_*`` nets, CLC_run.py:412-474); names 0, 2, 4."""

    def __init__(self, cin, cout):
        super().__init__(Conv2d(cin, 224, 3), GELU(), Conv2d(224, 128, 3), GELU(), Conv2d(128, cout, 3))

    def forward(self, x, final_act=ACT_NONE, res=None, pair=None, out=None):
        """pair: a second SliceTransform of the same shape for the second half of the batch (one launch per layer).
        out: destination of the result (a channel range of a wider buffer)."""
        q = pair if pair is not None else (None,) * 5
        g0, g1 = ops.ActGate(), ops.ActGate()   # each GELU' (stored forward) rides in the NEXT layer's data-gradient epilogue
        t = self[0](x, act=ACT_GELU, pair=q[0], gate_out=g0)
        t = self[2](t, act=ACT_GELU, pair=q[2], gate_in=g0, gate_out=g1)
        return self[4](t, act=final_act, res=res, pair=q[4], gate_in=g1, out=out)


class PointwiseMLP(nn.Sequential):
    """conv1x1 -> GELU -> conv1x1 (``ref_feature_adapter``, ``multi_ref_fusion``, CLM.fusion); names 0, 2."""

    def __init__(self, cin, mid, cout):
        super().__init__(conv1x1(cin, mid), GELU(), conv1x1(mid, cout))

    def forward(self, x):
        g = ops.ActGate()
        return self[2](self[0](x, act=ACT_GELU, gate_out=g), gate_in=g)


class ReferenceEncoder(nn.Module):
    def __init__(self, N=128, M=320):
        super().__init__()
        self.encoder = nn.Sequential(ResidualBlockWithStride(3, N, stride=2), ResidualBlockWithStride(N, N, stride=2),
                                     ResidualBlockWithStride(N, M, stride=2), conv3x3(M, M, stride=2))

    def forward(self, x):
        return self.encoder(x)


class CLM(nn.Module):
    """In-file CLM of the reference (CLC_run.py:284-313): constructed for state_dict parity, never called there."""

    def __init__(self, channels, head_dim=8, window_size=8):
        super().__init__()
        self.channels = channels
        self.alignment = SWAtten(channels * 2, channels, head_dim, window_size, 0, inter_dim=channels)
        self.fusion = PointwiseMLP(channels * 2, channels, channels)

    def forward(self, x, ref_feat):
        aligned = self.alignment(torch.cat([x, ref_feat], dim=1))
        return self.fusion(torch.cat([x, aligned], dim=1))


def _stage(N, head_dim, ws, tail):
    return [ConvTransBlock(N, N, head_dim, ws, 0.0, "W" if i % 2 == 0 else "SW") for i in range(2)] + [tail]


def _resize_registered_buffers(module, module_name, names, state_dict):
    for n in names:
        key = f"{module_name}.{n}"
        if key in state_dict:
            buf = dict(module.named_buffers()).get(n)
            if buf is None:
                raise ValueError(f'Invalid buffer name "{n}"')
            if buf.numel() == 0:
                buf.resize_(state_dict[key].size())


class CompressionModel(nn.Module):
    """compressai.models.CompressionModel surface (legacy kwarg as used at CLC_run.py:319)."""

    def __init__(self, entropy_bottleneck_channels=None, init_weights=None):
        super().__init__()
        if entropy_bottleneck_channels is not None:
            self.entropy_bottleneck = EntropyBottleneck(entropy_bottleneck_channels)

    def aux_loss(self):
        return sum(m.loss() for m in self.modules() if isinstance(m, EntropyBottleneck))

    def update(self, scale_table=None, force=False):
        if scale_table is None:
            scale_table = get_scale_table()
        updated = False
        for m in self.modules():
            if isinstance(m, GaussianConditional):
                updated |= m.update_scale_table(scale_table, force=force)
            if isinstance(m, EntropyBottleneck):
                updated |= m.update(force=force)
        return updated


class _SliceCodec(CompressionModel):
    """Shared backbone + channel-slice entropy model of TCM and CLC."""

    _boundary_ok = True   # forward() can expose (y, ref_features) for the two-phase backward of clc_amd.train.TrainEngine
    _boundary = None

    def _build_backbone(self, N, M, head_dim):
        ws = self.window_size
        self.g_a = nn.Sequential(
            ResidualBlockWithStride(3, 2 * N, 2),
            *_stage(N, head_dim[0], ws, ResidualBlockWithStride(2 * N, 2 * N, stride=2)),
            *_stage(N, head_dim[1], ws, ResidualBlockWithStride(2 * N, 2 * N, stride=2)),
            *_stage(N, head_dim[2], ws, conv3x3(2 * N, M, stride=2)))
        self.g_s = nn.Sequential(
            ResidualBlockUpsample(M, 2 * N, 2),
            *_stage(N, head_dim[3], ws, ResidualBlockUpsample(2 * N, 2 * N, 2)),
            *_stage(N, head_dim[4], ws, ResidualBlockUpsample(2 * N, 2 * N, 2)),
            *_stage(N, head_dim[5], ws, subpel_conv3x3(2 * N, 3, 2)))

    def _build_hyper(self, N):
        self.h_a = nn.Sequential(ResidualBlockWithStride(320, 2 * N, 2), *_stage(N, 32, 4, conv3x3(2 * N, 192, stride=2)))
        self.h_mean_s = nn.Sequential(ResidualBlockUpsample(192, 2 * N, 2), *_stage(N, 32, 4, subpel_conv3x3(2 * N, 320, 2)))
        self.h_scale_s = nn.Sequential(ResidualBlockUpsample(192, 2 * N, 2), *_stage(N, 32, 4, subpel_conv3x3(2 * N, 320, 2)))

    def _w(self, i, extra=0):
        return 320 + (320 // self.num_slices) * min(i + extra, 5 + extra)

    def _swatten(self, i):
        return nn.Sequential(SWAtten(self._w(i), self._w(i), 16, self.window_size, 0, inter_dim=128))

    # ------------------------------------------------------------------ shared slice machinery
    def _ref(self, ref_frames):
        return None

    def _fuse_z(self, z):
        return z

    def _slice_params(self, i, latent_means, latent_scales, y_hat_slices, ref_features, y_shape, ref_pair=None, sup=None):
        support = y_hat_slices if self.max_support_slices < 0 else y_hat_slices[: self.max_support_slices]
        rows = latent_means.shape[0] * latent_means.shape[2] * latent_means.shape[3]
        if ops.PAIR_SLICES and rows % 128 == 0:   # (the paired launch needs the batch halves to fall on tile boundaries)
            # The mean- and the scale-parameter nets are the same architecture on different inputs: stack the inputs along
            # the batch and run every layer of the two nets as ONE launch (second half of the batch on the second net's
            # filters).  These 16x16-map layers are latency-bound: twice the rows cost about the same time.
            if sup is not None:   # (ops.SliceSupport: the stacked input is a channel prefix of one buffer, no concatenation)
                both, fold, slot = sup.take(i, support, last=(i == self.num_slices - 1))
                both = self.atten_mean[i][0](both, pair=self.atten_scale[i][0], in_fold=fold, in_slot=slot)
            else:
                both = torch.cat((torch.cat([latent_means] + support, dim=1), torch.cat([latent_scales] + support, dim=1)), dim=0)
                both = self.atten_mean[i][0](both, pair=self.atten_scale[i][0])
            both, mean_support = ops.whole_and_first_half(both)
            if ref_features is not None:
                if ref_pair is None:
                    ref_pair = torch.cat((ref_features, ref_features), dim=0)
                ps = self.ref_cc_mean_transforms[i](torch.cat((both, ref_pair), dim=1), pair=self.ref_cc_scale_transforms[i])
            else:
                ps = self.cc_mean_transforms[i](both, pair=self.cc_scale_transforms[i])
            mu, scale = ops.split_batch(ps)
            if mu.shape[2] != y_shape[0] or mu.shape[3] != y_shape[1]:
                mu, scale = mu[:, :, : y_shape[0], : y_shape[1]], scale[:, :, : y_shape[0], : y_shape[1]]
            return mean_support, mu, scale

        mean_support = self.atten_mean[i](torch.cat([latent_means] + support, dim=1))
        if ref_features is not None:
            mu = self.ref_cc_mean_transforms[i](torch.cat([mean_support, ref_features], dim=1))
        else:
            mu = self.cc_mean_transforms[i](mean_support)
        ss = self.atten_scale[i](torch.cat([latent_scales] + support, dim=1))
        if ref_features is not None:
            scale = self.ref_cc_scale_transforms[i](torch.cat([ss, ref_features], dim=1))
        else:
            scale = self.cc_scale_transforms[i](ss)
        if mu.shape[2] != y_shape[0] or mu.shape[3] != y_shape[1]:
            mu, scale = mu[:, :, : y_shape[0], : y_shape[1]], scale[:, :, : y_shape[0], : y_shape[1]]
        return mean_support, mu, scale

    def _refine(self, i, mean_support, y_hat_slice, ref_features, out=None):
        """y_hat_slice + 0.5*tanh(lrp(...)) with the tanh and the add fused in the last conv's epilogue."""
        if ref_features is not None:
            return self.ref_lrp_transforms[i](torch.cat([mean_support, y_hat_slice, ref_features], dim=1), final_act=ACT_HALFTANH, res=y_hat_slice, out=out)
        return self.lrp_transforms[i](torch.cat([mean_support, y_hat_slice], dim=1), final_act=ACT_HALFTANH, res=y_hat_slice, out=out)

    def _hyper_synthesis(self, z_hat, stacked=False):
        """(latent_means, latent_scales) = (h_mean_s(z_hat), h_scale_s(z_hat)) (CLC_run.py:532-533): the two nets are the same
        architecture on the same input — stacked along the batch they run as ONE launch per layer.
        stacked: return the stacked result [means; scales] itself (ops.SliceSupport takes it whole)."""
        rows = z_hat.shape[0] * z_hat.shape[2] * z_hat.shape[3]
        if ops.PAIR_SLICES and rows % 128 == 0 and z_hat.shape[0] % 2 == 0:
            both = torch.cat((z_hat, z_hat), dim=0)
            for m, q in zip(self.h_mean_s, self.h_scale_s):
                both = m(both, pair=q)
            return both if stacked else ops.split_batch(both)
        assert not stacked
        return self.h_mean_s(z_hat), self.h_scale_s(z_hat)

    @staticmethod
    def _prep(x):
        if not x.is_cuda:
            raise ops._lib.ClcError("clc_amd models run on the GPU only (no CPU fallback by design); move the model and inputs to 'cuda'")
        return x.float().contiguous(memory_format=CL)

    def forward(self, x, ref_frames=None):
        # clc_amd.graphed_training / CLC_GRAPH_TRAIN=1: a training forward replays a captured hipGraph behind ONE autograd node
        if graphed.GRAPH_TRAIN or self.__dict__.get("_clc_graph_train"):
            out = graphed.forward(self, x, ref_frames)
            if out is not None:
                return out
        return self._forward_eager(x, ref_frames)

    def _forward_eager(self, x, ref_frames=None):
        x = self._prep(x)
        prof = ops.PROFILE is not None   # bench.py's roofline leg: launches are tagged with the sub-network they belong to
        if prof:
            ops.set_owner("ref_encoder")
        ref_features = self._ref(ref_frames)
        if prof:
            ops.set_owner("g_a")
        y = self.g_a(x)
        if prof:
            ops.set_owner("other")
        if getattr(self, "_keep_boundary", False):
            # outputs of the analysis transform / reference branch: where clc_amd.train.TrainEngine cuts the backward pass in two
            # so that the gradient exchange of everything downstream overlaps the backward of these two encoders
            y, ref_features = ops.cut(y), ops.cut(ref_features)
            self._boundary = (y, ref_features)
        y_shape = y.shape[2:]
        z = self._fuse_z(self.h_a(y))
        z_likelihoods, z_hat = self.entropy_bottleneck.likelihood_and_ste(z)
        S = y.shape[1] // self.num_slices
        sup = y_buf = lik_buf = None
        rows = z_hat.shape[0] * z_hat.shape[2] * z_hat.shape[3]
        if (ops.SUPPORT_BUFFER and ops.PAIR_SLICES and rows % 128 == 0 and z_hat.shape[0] % 2 == 0
                and (y.shape[0] * y.shape[2] * y.shape[3]) % 128 == 0
                # (the shared gradient buffer relies on the slices running backward strictly last-to-first, which autograd's dependencies
                #  only enforce when every slice reads its predecessor: ops.SliceSupport)
                and self.num_slices - 1 <= self.max_support_slices <= self.num_slices):
            both = self._hyper_synthesis(z_hat, stacked=True)
            if tuple(both.shape[2:]) == tuple(y.shape[2:]):
                sup = ops.SliceSupport(both, self.max_support_slices, S)
                latent_means, latent_scales = both[:y.shape[0]], both[y.shape[0]:]   # (shapes only: the nets read them through `sup`)
                y_buf = ops.new_act(y.shape[0], y.shape[1], y.shape[2], y.shape[3], y)   # y_hat: every slice's refined result, written in place
                lik_buf = ops.new_act(y.shape[0], y.shape[1], y.shape[2], y.shape[3], y)  # ... and every slice's likelihoods
            else:
                latent_means, latent_scales = ops.split_batch(both)
        else:
            latent_means, latent_scales = self._hyper_synthesis(z_hat)
        y_hat_slices, y_lik, mus, scales = [], [], [], []
        # the reference features feed every slice's cc pair and lrp net: one alias per consumer, the gradients summed in one launch each
        # (ops.fanout) instead of a chain of pairwise adds
        NS = self.num_slices
        ref_lrp = ref_cc = None
        if ref_features is not None:
            fan = ops.fanout(ref_features, NS + 2)
            ref_lrp = fan[:NS]
            if ops.PAIR_SLICES:
                ref_cc = ops.fanout(torch.cat((fan[NS], fan[NS + 1]), dim=0), NS)
        ref_pair = None
        # the additive-noise proxy of training (one uniform draw per latent element): all slices' noise in ONE launch
        noise_all = torch.empty_like(y, memory_format=CL).uniform_(-0.5, 0.5) if self.gaussian_conditional.training else None
        for i, y_slice in enumerate(ops.split_channels(y, [S] * self.num_slices)):
            mean_support, mu, scale = self._slice_params(i, latent_means, latent_scales, y_hat_slices, ref_features, y_shape,
                                                         ref_cc[i] if ref_cc is not None else ref_pair, sup)
            mus.append(mu)
            scales.append(scale)
            lik, y_hat_slice = self.gaussian_conditional.likelihood_and_ste(
                y_slice, scale, mu, noise=noise_all[:, i * S:(i + 1) * S] if noise_all is not None else None,
                lik_out=lik_buf[:, i * S:(i + 1) * S] if lik_buf is not None else None)
            y_lik.append(lik)
            y_hat_slices.append(self._refine(i, mean_support, y_hat_slice, ref_lrp[i] if ref_lrp is not None else None,
                                             out=y_buf[:, i * S:(i + 1) * S] if y_buf is not None else None))
            if sup is not None and i < sup.n:
                sup.add(i, y_hat_slices[-1])
        y_hat = ops.gather_channels(y_buf, y_hat_slices) if y_buf is not None else torch.cat(y_hat_slices, dim=1)
        if prof:
            ops.set_owner("g_s")
        x_hat = self.g_s(y_hat)
        if prof:
            ops.set_owner("other")
        y_likelihoods = ops.gather_channels(lik_buf, y_lik) if lik_buf is not None else torch.cat(y_lik, dim=1)
        out = {"x_hat": x_hat, "likelihoods": {"y": y_likelihoods, "z": z_likelihoods}}
        if not getattr(self, "_lean_outputs", False):   # (clc_amd.train.TrainEngine: the criterion never reads these two concatenations)
            out["para"] = {"means": torch.cat(mus, dim=1), "scales": torch.cat(scales, dim=1), "y": y}
        return out

    # ---- compress() / decompress() of ONE image ride on the captured segments of clc_amd.codec.CodecEngine (one hipGraph for the whole
    # encoder, six for the decoder: everything between two hops through the host arithmetic decoder), built lazily per input signature.
    # The reference evaluates exactly like this — one padded image per call (eval_CLC.py:314-338) — and eager launches made that surface
    # launch-bound (~550 dependent kernels, 10 ms per 256x256 image); the streams are byte-identical either way
    # (tests/test_codec_service_gpu.py).  CLC_CODEC_GRAPH=0 keeps the eager path; batches > 1 always take it (the reference's y stream of a
    # batch is ONE joint stream, CLC_run.py:695-714, which the per-image engine does not produce).
    def _codec_stamp(self):
        from ..codec import kernel_config

        # (the Parameter / buffer OBJECTS are stable; walking the module tree for them costs 3 ms per call, their data_ptr()s 30 us)
        probe = self.__dict__.get("_codec_probe")
        if probe is None:
            ps = list(self.parameters())
            probe = self.__dict__["_codec_probe"] = (ps[::8], list(self.buffers()), len(ps))
        # (parameter VALUES may change under the captured graphs: they read the same storage, and every derived image of a parameter — GDN
        #  re-parametrisation, fragment-order filters — is computed inside the graphs)
        return (kernel_config(), probe[2], sum(q.data_ptr() for q in probe[0]), sum(b.data_ptr() for b in probe[1]),
                bool(getattr(self, "wire_clm", False)), getattr(self, "max_support_slices", None), getattr(self, "use_ref", None))

    def __getstate__(self):   # (copy.deepcopy / pickling of the model: the lazily built engine — graphs, a thread pool — stays behind)
        d = dict(self.__dict__)
        d.pop("_codec_eng", None)
        d.pop("_codec_eng_stamp", None)
        d.pop("_codec_probe", None)
        d.pop("_clc_graphed", None)   # (clc_amd.graphed: captured plans of THIS instance's storage, and whether they were released)
        d.pop("_clc_graph_released", None)
        return d

    def _codec_engine(self, x_like):
        if not CODEC_GRAPH or self.training or not x_like.is_cuda or torch.cuda.is_current_stream_capturing():
            return None
        st = self._codec_stamp()    # parameters re-homed (TrainEngine's arenas, .to()), tables rebuilt, tuning / precision changed -> new graphs
        eng = self.__dict__.get("_codec_eng")
        if eng is None or self.__dict__.get("_codec_eng_stamp") != st:
            from ..codec import CodecEngine

            if eng is not None:
                eng.close()
            import weakref

            was_training = self.training
            # (a proxy: model -> engine -> model would be a reference cycle, freed only by a garbage collection at some later time — e.g.
            #  inside another engine's graph capture, where releasing this one's graphs and pinned buffers is illegal)
            eng = CodecEngine(weakref.proxy(self), threads=1, max_plans=CODEC_GRAPH_PLANS)
            self.train(was_training)
            self.__dict__["_codec_eng"], self.__dict__["_codec_eng_stamp"] = eng, self._codec_stamp()
        return eng

    @torch.no_grad()
    def compress(self, x, ref_frames=None, lanes=None):
        """lanes=None: the reference's one-stream format.  lanes=W (1 .. 16): THE LANES STREAM (include/clc_hip.h) — the y
        string of every image is W wave streams of 64 rANS lanes, the slices as segments in NHWC order, coded on the device; the result
        carries "lanes": W and one y string per image; pass the same W to decompress.  The z strings are the default's."""
        Wn = coding.lanes_count(lanes, f"{type(self).__name__}.compress")
        if x.shape[0] == 1:
            eng = self._codec_engine(x)
            if eng is not None:
                if Wn is not None:
                    o = eng.compress(self._prep(x), ref_frames, lanes=Wn)[0]
                    return {"strings": o["strings"], "shape": o["shape"], "kernel_config": o["kernel_config"], "lanes": Wn}
                o = eng.compress(self._prep(x), ref_frames)[0]
                return {"strings": o["strings"], "shape": o["shape"], "kernel_config": o["kernel_config"]}
        if Wn is not None:
            return self._compress_eager(x, ref_frames, lanes=Wn)
        return self._compress_eager(x, ref_frames)

    @torch.no_grad()
    def decompress(self, strings, shape, ref_frames=None, lanes=None, device_coder=True, check=True):
        """lanes=W: the strings of compress(x, lanes=W); their headers are parsed on the host before any device work.  device_coder=True
        decodes on the device with the coder inside the slice step (one image: ONE upload and one replay of one graph, no copy back, no
        synchronize); check=True adds ONE download of the coder's end states after everything is issued and raises ValueError naming the
        image and the wave streams that did not end where a whole stream ends (not a checksum).  device_coder=False decodes the same
        format with one ans.LanesDecoder per image and a hop per slice: the oracle and the fallback."""
        Wn = coding.lanes_count(lanes, f"{type(self).__name__}.decompress")
        if Wn is not None:
            if device_coder and len(strings[1]) == 1:
                eng = self._codec_engine(next(self.parameters()))
                if eng is not None:
                    return {"x_hat": eng.decompress([{"strings": strings, "shape": shape}], ref_frames, lanes=Wn, check=check)}
            return self._decompress_eager(strings, shape, ref_frames, lanes=Wn, device_coder=device_coder, check=check)
        coding.refuse_lanes_strings(strings[0])
        if len(strings[1]) == 1:
            eng = self._codec_engine(next(self.parameters()))
            if eng is not None:
                return {"x_hat": eng.decompress([{"strings": strings, "shape": shape}], ref_frames)}
        return self._decompress_eager(strings, shape, ref_frames)

    @torch.no_grad()
    def _compress_eager(self, x, ref_frames=None, lanes=None):
        Wn = coding.lanes_count(lanes, f"{type(self).__name__}.compress")
        x = self._prep(x)
        ref_features = self._ref(ref_frames)
        y = self.g_a(x)
        y_shape = y.shape[2:]
        z = self._fuse_z(self.h_a(y))
        z_strings = self.entropy_bottleneck.compress(z)
        z_hat = self.entropy_bottleneck.decompress(z_strings, z.size()[-2:])
        latent_scales = self.h_scale_s(z_hat)
        latent_means = self.h_mean_s(z_hat)
        gc = self.gaussian_conditional
        cdf, cdf_len, off = gc.host_tables()
        sym_parts, idx_parts, y_hat_slices = [], [], []
        for i, y_slice in enumerate(y.chunk(self.num_slices, 1)):
            mean_support, mu, scale = self._slice_params(i, latent_means, latent_scales, y_hat_slices, ref_features, y_shape)
            sym, idx, y_hat_slice = gc.quantize_and_index(y_slice, mu, scale)
            sym_parts.append(sym)
            idx_parts.append(idx)
            y_hat_slices.append(self._refine(i, mean_support, y_hat_slice, ref_features))
        from ..codec import kernel_config

        if Wn is not None:
            return {"strings": [self._encode_y_lanes(sym_parts, idx_parts, Wn), z_strings], "shape": z.size()[-2:],
                    "kernel_config": kernel_config(), "lanes": Wn}
        # (`kernel_config`: beyond the reference's two keys — which kernel state encoded, for clc_amd.codec.pack_item)
        return {"strings": [self._encode_y(sym_parts, idx_parts), z_strings], "shape": z.size()[-2:], "kernel_config": kernel_config()}

    def _encode_y(self, sym_parts, idx_parts):
        """Per-slice int32 symbol / index tensors (logical NCHW) -> [one y stream]: slices concatenated in order, element order
        inside a slice = the reference's NCHW reshape(-1) (CLC_run.py:695-696, 712-714); ONE D2H copy for all slices."""
        cdf, cdf_len, off = self.gaussian_conditional.host_tables()
        sym_all = torch.stack([s.contiguous() for s in sym_parts]).cpu().numpy().reshape(-1)
        idx_all = torch.stack([s.contiguous() for s in idx_parts]).cpu().numpy().reshape(-1)
        return [ans.encode(sym_all, idx_all, cdf, cdf_len, off)]

    def _encode_y_lanes(self, sym_parts, idx_parts, W):
        """Per-slice int32 symbol / index tensors (NCHW views of NHWC buffers) -> one lanes string per image: the slices are the
        segments, each in the order it lies in memory; one clc_rans_lanes_encode and one clc_rans_lanes_pack for the batch, then two
        device -> host copies (the header, the packed words)."""
        gc = self.gaussian_conditional
        B = sym_parts[0].shape[0]
        flat = lambda ts: torch.cat([t.permute(0, 2, 3, 1).reshape(B, -1) for t in ts], dim=1)
        out, _, result = ops.rans_lanes_encode(flat(sym_parts), flat(idx_parts), [int(t[0].numel()) for t in sym_parts], W,
                                               (gc._quantized_cdf, gc._cdf_length, gc._offset))
        packed, header = ops.rans_lanes_pack(out, result)
        head = header.cpu().numpy()
        total = int(head[B * W])
        words = packed[:total].cpu().numpy() if (head[:B * W] >= 0).all() else np.zeros(0, np.int32)
        return coding.lanes_strings(head, words, B, W)

    @torch.no_grad()
    def _decompress_lanes_eager(self, strings, shape, ref_frames, W, device_coder, check):
        subs = coding.lanes_parse(strings[0], W)   # the headers, before any device work
        if len(subs) != len(strings[1]):
            raise ValueError(f"decompress: {len(subs)} y streams for {len(strings[1])} z streams")
        ref_features = self._ref(ref_frames)
        z_hat = self.entropy_bottleneck.decompress(strings[1], shape)
        latent_scales = self.h_scale_s(z_hat)
        latent_means = self.h_mean_s(z_hat)
        B, dev = z_hat.shape[0], z_hat.device
        y_shape = [z_hat.shape[2] * 4, z_hat.shape[3] * 4]
        Cs = self.M // self.num_slices
        n = y_shape[0] * y_shape[1] * Cs
        gc = self.gaussian_conditional
        if device_coder:
            tables = (gc._quantized_cdf, gc._cdf_length, gc._offset)
            state, spans, words = coding.upload_streams(subs, 2 * ans.LANES, dev)
        else:
            state = [ans.LanesDecoder(img) for img in subs]
            decode = coding.table_decode([d.decode for d in state], gc.host_tables())
            hop = coding.HostHop(B * n, B * n, dev)
        y_hat_slices = []
        for i in range(self.num_slices):
            mean_support, mu, scale = self._slice_params(i, latent_means, latent_scales, y_hat_slices, ref_features, y_shape)
            if device_coder:
                y_hat_slice = ops.rans_lanes_decode_gauss(scale, mu, gc.scale_table, tables, words, spans, state)
            else:
                down, up = hop.step(B * n, B * n)
                down.copy_(gc.build_indexes(scale).permute(0, 2, 3, 1).reshape(-1))   # NHWC: the segment's order
                hop.run(decode)
                y_hat_slice = up.view(B, y_shape[0], y_shape[1], Cs).permute(0, 3, 1, 2).float() + mu
            y_hat_slices.append(self._refine(i, mean_support, y_hat_slice, ref_features))
        x_hat = self.g_s(torch.cat(y_hat_slices, dim=1)).clamp_(0, 1)
        if check:
            coding.lanes_check(state, subs)
        return {"x_hat": x_hat}

    @torch.no_grad()
    def _decompress_eager(self, strings, shape, ref_frames=None, lanes=None, device_coder=True, check=True):
        Wn = coding.lanes_count(lanes, f"{type(self).__name__}.decompress")
        if Wn is not None:
            return self._decompress_lanes_eager(strings, shape, ref_frames, Wn, device_coder, check)
        ref_features = self._ref(ref_frames)
        z_hat = self.entropy_bottleneck.decompress(strings[1], shape)
        latent_scales = self.h_scale_s(z_hat)
        latent_means = self.h_mean_s(z_hat)
        y_shape = [z_hat.shape[2] * 4, z_hat.shape[3] * 4]
        gc = self.gaussian_conditional
        cdf, cdf_len, off = gc.host_tables()
        dec = ans.RansDecoder()
        dec.set_stream(strings[0][0])
        y_hat_slices = []
        for i in range(self.num_slices):
            mean_support, mu, scale = self._slice_params(i, latent_means, latent_scales, y_hat_slices, ref_features, y_shape)
            index = gc.build_indexes(scale)
            rv = dec.decode_stream(index.contiguous().cpu().numpy().reshape(-1), cdf, cdf_len, off)
            rv = torch.from_numpy(rv.astype(np.float32)).reshape(1, -1, y_shape[0], y_shape[1]).to(mu.device).contiguous(memory_format=CL)
            y_hat_slice = rv + mu
            y_hat_slices.append(self._refine(i, mean_support, y_hat_slice, ref_features))
        x_hat = self.g_s(torch.cat(y_hat_slices, dim=1)).clamp_(0, 1)
        return {"x_hat": x_hat}


class CLC(_SliceCodec):
    def __init__(self, config=[2, 2, 2, 2, 2, 2], head_dim=[8, 16, 32, 32, 16, 8], drop_path_rate=0, N=128, M=320,
                 num_slices=5, max_support_slices=5, num_ref_frames=3, use_ref=True, **kwargs):
        refuse_rate_levels("CLC", kwargs)
        refuse_integer_hyper("CLC", kwargs)
        super().__init__(entropy_bottleneck_channels=N)
        if list(config) != [2] * 6 or drop_path_rate != 0 or M != 320 or num_slices != 5:
            raise ValueError("clc_amd.CLC supports the reference configuration: config=[2]*6, drop_path_rate=0, M=320, num_slices=5")
        self.config, self.head_dim, self.window_size = config, head_dim, 8
        self.num_slices, self.max_support_slices = num_slices, max_support_slices
        self.num_ref_frames, self.use_ref, self.M = num_ref_frames, use_ref, M
        S = 320 // num_slices
        self._build_backbone(N, M, head_dim)
        self.ref_encoder = ReferenceEncoder(N, M)
        self.feature_alignment = nn.ModuleList([CLM(192, head_dim=32, window_size=4) for _ in range(num_ref_frames)])
        self.multi_ref_fusion = PointwiseMLP(192 * (num_ref_frames + 1), 256, 192)
        self._build_hyper(N)
        self.atten_mean = nn.ModuleList(self._swatten(i) for i in range(num_slices))
        self.atten_scale = nn.ModuleList(self._swatten(i) for i in range(num_slices))
        self.ref_cc_mean_transforms = nn.ModuleList(SliceTransform(self._w(i) + 64, S) for i in range(num_slices))
        self.ref_cc_scale_transforms = nn.ModuleList(SliceTransform(self._w(i) + 64, S) for i in range(num_slices))
        self.cc_mean_transforms = nn.ModuleList(SliceTransform(self._w(i), S) for i in range(num_slices))
        self.cc_scale_transforms = nn.ModuleList(SliceTransform(self._w(i), S) for i in range(num_slices))
        self.lrp_transforms = nn.ModuleList(SliceTransform(self._w(i, 1), S) for i in range(num_slices))
        self.ref_lrp_transforms = nn.ModuleList(SliceTransform(self._w(i, 1) + 64, S) for i in range(num_slices))
        self.ref_feature_adapter = PointwiseMLP(M * num_ref_frames, 128, 64)
        self.entropy_bottleneck = EntropyBottleneck(192)
        self.gaussian_conditional = GaussianConditional(None)

    def _ref(self, ref_frames):
        if ref_frames is None or not self.use_ref:
            return None
        R = len(ref_frames)
        if R != self.num_ref_frames:
            raise ValueError(f"expected {self.num_ref_frames} reference frames, got {R}")
        return self._ref_from_latents(self._ref_encode(ref_frames), R)

    def _ref_encode(self, ref_frames):
        """R reference frames [B, 3, H, W] -> their latents [R*B, M, H/16, W/16], reference-major: one batched ref_encoder pass."""
        R = len(ref_frames)
        refs = self._prep(torch.cat(list(ref_frames), dim=0)) if R > 1 else self._prep(ref_frames[0])
        return self.ref_encoder(refs)

    def _ref_from_latents(self, feats, R):
        """reference latents [R*B, M, h, w] (reference-major, from _ref_encode or gathered from a clc_amd.refbank.ReferenceBank) -> the
        reference features every slice reads."""
        if R != self.num_ref_frames:
            raise ValueError(f"expected {self.num_ref_frames} reference frames, got {R}")
        self._ref_latents = feats if self.wire_clm else None   # [R*B, M, h, w], reference-major
        if R > 1:
            feats = torch.cat(feats.chunk(R, dim=0), dim=1)  # [B, R*M, h, w] in reference order
        return self.ref_feature_adapter(feats)

    # SURVEY §8(f)-4 — NOT reference behaviour: the reference constructs feature_alignment / multi_ref_fusion (CLC_run.py:359-369) and
    # never calls them.  wire_clm = True applies them the one way their constructor shapes admit: CLM(192) pairs the hyper-latent z with
    # a 192-channel feature of each reference at z's resolution — h_a of that reference's latent, one batched pass — and
    # multi_ref_fusion (192 * (R + 1) -> 256 -> 192) fuses z with the R aligned features.  Encoder side only (forward / compress):
    # the decoder receives the fused z_hat.  The CPU checker restates the same definition; the modules themselves are pinned against
    # the genuine classes (tests/golden/dormant.npz).
    wire_clm = False

    def _fuse_z(self, z):
        lat = getattr(self, "_ref_latents", None)
        if not self.wire_clm or lat is None:
            return z
        R = self.num_ref_frames
        zr = self.h_a(lat).chunk(R, dim=0)
        aligned = [self.feature_alignment[r](z, zr[r]) for r in range(R)]
        return self.multi_ref_fusion(torch.cat([z] + aligned, dim=1))

    extract_ref_features = _ref

    def update(self, scale_table=None, force=False):
        if scale_table is None:
            scale_table = get_scale_table()
        updated = self.gaussian_conditional.update_scale_table(scale_table, force=force)
        updated |= self.entropy_bottleneck.update(force=force)
        return updated

    def load_state_dict(self, state_dict, strict=False):
        own = self.state_dict()
        filtered = {k: v for k, v in state_dict.items() if k in own}
        _resize_registered_buffers(self.gaussian_conditional, "gaussian_conditional",
                                   ["_quantized_cdf", "_offset", "_cdf_length", "scale_table"], state_dict)
        _resize_registered_buffers(self.entropy_bottleneck, "entropy_bottleneck", ["_quantized_cdf", "_offset", "_cdf_length"], state_dict)
        return nn.Module.load_state_dict(self, filtered, strict=False)


class TCM(_SliceCodec):
    def __init__(self, config=[2, 2, 2, 2, 2, 2], head_dim=[8, 16, 32, 32, 16, 8], drop_path_rate=0, N=128, M=320,
                 num_slices=5, max_support_slices=5, **kwargs):
        refuse_rate_levels("TCM", kwargs)
        refuse_integer_hyper("TCM", kwargs)
        super().__init__(entropy_bottleneck_channels=N)
        if list(config) != [2] * 6 or drop_path_rate != 0 or M != 320 or num_slices != 5:
            raise ValueError("clc_amd.TCM supports the reference configuration: config=[2]*6, drop_path_rate=0, M=320, num_slices=5")
        self.config, self.head_dim, self.window_size = config, head_dim, 8
        self.num_slices, self.max_support_slices, self.M = num_slices, max_support_slices, M
        S = 320 // num_slices
        self._build_backbone(N, M, head_dim)
        self._build_hyper(N)
        self.atten_mean = nn.ModuleList(self._swatten(i) for i in range(num_slices))
        self.atten_scale = nn.ModuleList(self._swatten(i) for i in range(num_slices))
        self.cc_mean_transforms = nn.ModuleList(SliceTransform(self._w(i), S) for i in range(num_slices))
        self.cc_scale_transforms = nn.ModuleList(SliceTransform(self._w(i), S) for i in range(num_slices))
        self.lrp_transforms = nn.ModuleList(SliceTransform(self._w(i, 1), S) for i in range(num_slices))
        self.entropy_bottleneck = EntropyBottleneck(192)
        self.gaussian_conditional = GaussianConditional(None)

    def forward(self, x, ref_frames=None):
        return super().forward(x, None)

    def compress(self, x, ref_frames=None, lanes=None):
        return super().compress(x, None, lanes=lanes)

    def decompress(self, strings, shape, ref_frames=None, lanes=None, device_coder=True, check=True):
        return super().decompress(strings, shape, None, lanes=lanes, device_coder=device_coder, check=check)

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
