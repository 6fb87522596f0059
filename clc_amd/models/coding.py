"""What the context-model coders (hyperprior.py, elic.py, cheng.py) share on the host side of their kernels — each decision has one
owner here:

* THE HOP of a host-decoded step: ``HostHop`` (buffers allocated once; per step one download, one synchronize, the caller's decode, one
  upload), ``open_decoders`` and ``table_decode``.
* WHERE A TABLE-CODED STEP'S SYMBOLS COME FROM, between the finish kernel and the commit kernel: ``HostSymbols`` (a hop to host
  decoders) and ``DeviceLanesSymbols`` (the device's lanes decoder, no hop), one interface: ``views``, ``decode``, ``state``.
* THE START of a decoder's pass loop: ``decoder_start`` (parameters channels-last, the batch refusal, the zeroed y_hat).
* THE UPLOAD IMAGE of a device-decoded batch, ``[states | spans | words]`` in one pinned int32 buffer: ``stream_image`` (numpy),
  ``stream_views``, ``upload_streams`` (a buffer per call; an engine plan keeps its own image at a fixed address and hands its
  ``stream_views`` to the model's pass, codec._Engine._lanes_decoder_buffers); and the end-state rule of a whole stream, ``check_stream_ends`` / ``device_ends``.
* THE MULTI-STREAM STRINGS of a batch, for either container of ans.py: ``stream_parse`` and ``stream_check``; for the lanes stream
  (elic2022, CLC, TCM; model and CodecEngine) also ``lanes_count``, ``lanes_parse``, ``refuse_lanes_strings``, ``lanes_strings``,
  ``lanes_check``.
* Small pieces: ``linear_filters``, ``CodeInputs._code_inputs``, ``coded_item``.

The kernels, their order and their arguments stay with the models; the multi-stream container is ans.py's.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import ans, ops
from ..ops import CL


class HostHop:
    """The buffers and the protocol of one host-decoded step.  ``step(n, m)`` hands out the device views ``down`` (n int32, for the
    finish kernel to write) and ``up`` (m int32, for the commit kernel to read); between the two kernels ``run(decode)`` takes down to
    the host, lets the caller decode it into m int32 and brings those to up.  Device staging buffers, their pinned twins and the numpy
    views of the twins are allocated once, for the largest step."""

    def __init__(self, down_elems, up_elems, dev):
        self._down_dev = torch.empty((down_elems,), device=dev, dtype=torch.int32)
        self._up_dev = torch.empty((up_elems,), device=dev, dtype=torch.int32)
        self._down_host = torch.empty((down_elems,), dtype=torch.int32).pin_memory()
        self._up_host = torch.empty((up_elems,), dtype=torch.int32).pin_memory()
        self._down_np, self._up_np = self._down_host.numpy(), self._up_host.numpy()
        self._stream = torch.cuda.current_stream(dev)
        self._sizes = self._cut = None

    def step(self, n_down, n_up):
        """-> (down, up) of the next run.  The views are kept while the sizes repeat: a tensor slice costs microseconds, mbt2018 hops
        once per pixel at one size and a wavefront repeats each step size three times."""
        if self._sizes != (n_down, n_up):
            self._sizes = (n_down, n_up)
            self._cut = (self._down_dev[:n_down], self._up_dev[:n_up], self._down_host[:n_down], self._up_host[:n_up],
                         self._down_np[:n_down], self._up_np[:n_up])
        return self._cut[0], self._cut[1]

    def run(self, decode):
        """one device -> host copy, one synchronize, ``decode(down, up)`` on numpy views of the pinned pages, one host -> device copy"""
        down_dev, up_dev, down_host, up_host, down_np, up_np = self._cut
        down_host.copy_(down_dev, non_blocking=True)
        self._stream.synchronize()   # (also: the previous step's upload has left the pinned page that decode is about to overwrite)
        decode(down_np, up_np)
        up_dev.copy_(up_host, non_blocking=True)


def open_decoders(strings):
    """one incremental ans.RansDecoder per stream, opened once"""
    decoders = []
    for s in strings:
        d = ans.RansDecoder()
        d.set_stream(s)
        decoders.append(d)
    return decoders


def table_decode(decode_fns, tables):
    """The ``HostHop.run`` callback of a step coded through table indexes.  The step's rows are B equal blocks, image b's pixels in list
    order with channels inner, which is the order of its stream: block b goes through decode_fns[b](indexes, cdf, sizes, offsets)."""
    cdf, ln, off = tables

    def decode(idx_np, sym_np):
        e = idx_np.size // len(decode_fns)
        for b, fn in enumerate(decode_fns):
            sym_np[b * e:(b + 1) * e] = fn(idx_np[b * e:(b + 1) * e], cdf, ln, off)
    return decode


class HostSymbols:
    """A table-coded step's symbols from the host: one hop to ``decode_fns`` (table_decode's, one per image).  ``state`` is what
    stream_check takes when the last step is done: the caller's decoders."""

    def __init__(self, decode_fns, tables, most, dev, state=None):
        self._decode, self.state = table_decode(decode_fns, tables), state
        self._hop = HostHop(most, most, dev)   # most: the elements of the largest step

    def views(self, n, c):
        """-> (indexes, symbols) int32 [n, c] of a step of n rows x c channels: the finish kernel writes the first, commit reads the second"""
        idx, sym = self._hop.step(n * c, n * c)
        return idx.view(n, c), sym.view(n, c)

    def decode(self, idx, sym, per_image):
        """the step whose views were cut last: its indexes down, its symbols up (HostHop.run)"""
        self._hop.run(self._decode)


class DeviceLanesSymbols:
    """A table-coded step's symbols from the device's lanes decoder: every wave stream's states, spans and words uploaded once, then one
    clc_rans_lanes_decode_step per step — no download, no synchronize.  ``state`` is the device's int32 [B, W, 130] (64 x (x low, x
    high), pos, pad) as the last step left it.  tables: the DEVICE's (cdf, lengths, offsets)."""

    def __init__(self, subs, tables, most, dev):
        self._tables = tables
        self.state, self._spans, self._words = upload_streams(subs, 2 * ans.LANES, dev)   # a wave stream starts with its 64 lane states
        self._idx = torch.empty((most,), device=dev, dtype=torch.int32)
        self._sym = torch.empty((most,), device=dev, dtype=torch.int32)

    def views(self, n, c):
        return self._idx[:n * c].view(n, c), self._sym[:n * c].view(n, c)

    def decode(self, idx, sym, per_image):
        ops.rans_lanes_decode_step(idx, per_image, self._tables, self._words, self._spans, self.state, sym)


def decoder_start(params, n_streams, M):
    """What a decoder's pass loop opens with -> (the hyper parameters channels-last, y_hat [B, M, H, W] zeroed and channels-last); a
    batch of y streams that is not the z streams' is refused."""
    params = params.contiguous(memory_format=CL)
    B, (H, W) = params.shape[0], params.shape[2:]
    if n_streams != B:
        raise ValueError(f"decompress: {n_streams} y streams for {B} z streams")
    return params, torch.zeros((B, M, H, W), device=params.device, dtype=torch.float32).contiguous(memory_format=CL)


def stream_spans(counts):
    """word counts of a batch's streams -> int64 [n, 2] (first word, word count): back to back from word 0"""
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    n_words = int(counts.sum())
    if n_words >= 1 << 31:
        raise ValueError(f"decompress: {n_words} stream words in one batch; the spans are int32")
    return np.stack((np.concatenate(([0], np.cumsum(counts)[:-1])), counts), axis=1)


def stream_image(subs, n_state):
    """The upload image of a device-decoded batch, subs[b][s] the bytes of image b's stream s -> int32 [(n_state + 4) B S + words]:

        B S states of n_state + 2 words | B S spans (first word, word count) | every stream's 32-bit words, back to back

    A state is the stream's first n_state words (its coder's initial state: 2 for a split sub-stream, 128 for a lanes wave stream), then
    pos = n_state, the next word to read, and a pad word 0."""
    flat = [np.frombuffer(s, dtype="<u4") for img in subs for s in img]
    spans = stream_spans([w.size for w in flat])
    image = np.empty(((n_state + 4) * len(flat) + int(spans[:, 1].sum()),), dtype=np.uint32)
    state, sp, words = stream_views(image, 1, len(flat), n_state)
    for i, w in enumerate(flat):
        state[0, i, :n_state] = w[:n_state]
    state[0, :, n_state], state[0, :, n_state + 1] = n_state, 0
    sp[0] = spans
    np.concatenate(flat, out=words)
    return image.view(np.int32)


def stream_views(image, B, S, n_state):
    """a stream_image (numpy array or tensor) -> its (state [B, S, n_state + 2], spans [B, S, 2], words) views"""
    SW, n = n_state + 2, B * S
    return image[:SW * n].reshape(B, S, SW), image[SW * n:(SW + 2) * n].reshape(B, S, 2), image[(SW + 2) * n:]


def upload_streams(subs, n_state, dev):
    """stream_image through one pinned buffer and one non-blocking copy -> the device's (state, spans, words)"""
    host = torch.from_numpy(stream_image(subs, n_state)).pin_memory()
    image = torch.empty((host.numel(),), device=dev, dtype=torch.int32)
    image.copy_(host, non_blocking=True)
    # (host's pages stay pinned until the copy has run: the caching host allocator holds them back until then)
    return stream_views(image, len(subs), len(subs[0]), n_state)


def device_ends(state):
    """the device coder's state tensor int32 [B, S, n_state + 2] -> (x uint64 [B, S, n_state / 2], pos [B, S]): ONE download"""
    st = state.cpu().numpy().view(np.uint32)
    n = st.shape[2] - 2
    return st[..., 0:n:2].astype(np.uint64) | (st[..., 1:n:2].astype(np.uint64) << np.uint64(32)), st[..., n]


def check_stream_ends(x, pos, counts, noun):
    """A stream decoded to its end leaves every coder state at 2^31 and pos == its word count (the coder's end-state property); anything
    else raises, naming per image every stream that did not.  (A wrong symbol enters the context of what is decoded after it, so a damaged
    stream usually takes the image's others out of step with it: the list holds the damaged one, it cannot single it out.)
    x: final states [B, S, states per stream]; pos, counts: words consumed and words held [B, S]; noun: what a stream is called."""
    x, pos, counts = np.asarray(x, dtype=np.uint64), np.asarray(pos), np.asarray(counts)
    astray = (x != np.uint64(1 << 31)).sum(axis=2)
    bad = []
    for b in range(x.shape[0]):
        off = [s for s in range(x.shape[1]) if astray[b, s] or pos[b, s] != counts[b, s]]
        if off:
            s = off[0]
            bad.append(f"image {b}: {noun}s {off} did not decode to their end ({noun} {s}: {int(astray[b, s])} of {x.shape[2]} states not at "
                       f"2^31, {int(pos[b, s])} of {int(counts[b, s])} words consumed)")
    if bad:
        raise ValueError("decompress: " + "; ".join(bad) + ": the stream is corrupt, truncated or belongs to other parameters")


def lanes_count(lanes, who):
    """lanes=None: the one-stream format; else the number W of wave streams per image, refused by name outside 1 .. 16"""
    return None if lanes is None else ans.stream_count(ans.LANES_STREAM, lanes, who, "lanes")


def stream_parse(fmt, y_strings, n, keyword):
    """-> per image the n streams of its string in container fmt (ans.SPLIT_STREAM, ans.LANES_STREAM); a header that disagrees with the
    caller's ``keyword=n`` is refused.  Host only."""
    subs = []
    for b, blob in enumerate(y_strings):
        got = ans._unpack(fmt, blob)
        if len(got) != n:
            raise ValueError(f"decompress: {keyword} = {n}, but the header of image {b} says {len(got)} {fmt.noun}s")
        subs.append(got)
    return subs


def lanes_parse(y_strings, W):
    """stream_parse of lanes strings under ``lanes=W``"""
    return stream_parse(ans.LANES_STREAM, y_strings, W, "lanes")


def refuse_lanes_strings(y_strings):
    """the one-stream decoder was handed a lanes string: refused by name before any device work"""
    for b, blob in enumerate(y_strings):
        if bytes(blob[:4]) == ans.LANES_MAGIC:
            raise ValueError(f"decompress: the y string of image {b} is a lanes stream ({ans.LANES_MAGIC!r}); pass lanes= (its header "
                             f"says {blob[4] if len(blob) > 4 else '?'} wave streams)")


def lanes_strings(header, words, B, W):
    """What ops.rans_lanes_pack left, on the host — header int32 [B W + 1] (counts or negative codes, total) and the packed words — ->
    per image its lanes string.  A negative code raises by name."""
    from .. import lib

    counts = np.asarray(header[:B * W]).reshape(B, W)
    for b, w in zip(*np.nonzero(counts < 0)):
        why = "a zero-frequency symbol" if counts[b, w] == lib.RANS_LANES_ZERO_FREQ else "its region overflowed"
        raise ValueError(f"compress: image {b}, wave stream {w}: {why} (clc_rans_lanes_encode code {int(counts[b, w])})")
    words = np.asarray(words).view(np.uint32)
    if int(counts.sum()) != int(header[B * W]) or words.size < int(counts.sum()):
        raise ValueError(f"compress: the packed wave streams hold {words.size} words, their header counts {int(counts.sum())} (total {int(header[B * W])})")
    ends = np.cumsum(counts.reshape(-1))
    streams = [words[e - n:e].astype("<u4").tobytes() for e, n in zip(ends, counts.reshape(-1))]
    return [ans.lanes_pack(streams[b * W:(b + 1) * W]) for b in range(B)]


def stream_check(fmt, state, subs):
    """check_stream_ends over every state of every stream of container fmt.  state: the device coder's [B, S, n_state + 2] tensor — ONE
    download — or the host coder's list of ans.LanesDecoder."""
    if isinstance(state, torch.Tensor):
        x, pos = device_ends(state)
    else:
        ends = [[d.state(w) for w in range(len(img))] for d, img in zip(state, subs)]
        x, pos = [[e[0] for e in img] for img in ends], [[e[1] for e in img] for img in ends]
    check_stream_ends(x, pos, [[len(blob) // 4 for blob in img] for img in subs], fmt.noun)


def lanes_check(state, subs):
    """stream_check over every wave stream's 64 lanes"""
    stream_check(ans.LANES_STREAM, state, subs)


def linear_filters(layers):
    """[(filter [N, K] row-major, bias)] of layers 0, 2 and 4 of a Sequential of three 1x1 convolutions and their activations"""
    out = []
    for i in (0, 2, 4):
        w = layers[i].weight.detach()
        out.append((w.reshape(w.shape[0], w.shape[1]).contiguous(), layers[i].bias.detach().contiguous()))
    return out


def coded_item(y_strings, z_strings, z_size, **extra):
    """what compress returns"""
    from ..codec import kernel_config

    return {"strings": [y_strings, z_strings], "shape": z_size, "kernel_config": kernel_config(), **extra}


class CodeInputs:
    """for models with _prep, _analysis, _hyper_analysis, _hyper_synthesis and an entropy_bottleneck"""

    @torch.no_grad()
    def _code_inputs(self, x):
        """(y, hyper parameters from the coded z, z streams, z's map size): what the context model's passes start from"""
        x = self._prep(x)
        y = self._analysis(x)
        z = self._hyper_analysis(y)
        z_strings = self.entropy_bottleneck.compress(z)
        z_hat = self.entropy_bottleneck.decompress(z_strings, z.size()[-2:])
        return y, self._hyper_synthesis(z_hat), z_strings, z.size()[-2:]
