"""``compressai.ans``-compatible entropy coder backed by the C++ rANS of libclc_hip.so.

Same class / method names as the pybind11 module the reference imports
(/root/reference/models/CLC_run.py:2,658,712-713,762-763,793): ``BufferedRansEncoder``
(``encode_with_indexes``, ``flush``), ``RansEncoder`` (``encode_with_indexes``) and
``RansDecoder`` (``set_stream``, ``decode_stream``, ``decode_with_indexes``).  Arguments may be
Python lists (reference style) or int32 numpy arrays (zero-copy fast path used by clc_amd.models).
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np

from . import lib as _lib


def _i32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.int32))


def _tables(cdfs, cdfs_sizes, offsets):
    if isinstance(cdfs, np.ndarray) and cdfs.dtype == np.int32 and cdfs.ndim == 2 and cdfs.flags.c_contiguous:
        cdf = cdfs
    else:  # ragged python lists are allowed by the reference API: pad to a rectangle
        rows = [np.asarray(r, dtype=np.int32) for r in cdfs]
        width = max(len(r) for r in rows)
        cdf = np.zeros((len(rows), width), dtype=np.int32)
        for i, r in enumerate(rows):
            cdf[i, : len(r)] = r
    return cdf, _i32(cdfs_sizes).reshape(-1), _i32(offsets).reshape(-1)


def encode(symbols, indexes, cdfs, cdfs_sizes, offsets) -> bytes:
    L = _lib.load()
    sym, idx = _i32(symbols).reshape(-1), _i32(indexes).reshape(-1)
    if sym.size != idx.size:
        raise ValueError("symbols and indexes must have the same length")
    cdf, ln, off = _tables(cdfs, cdfs_sizes, offsets)
    if idx.size and (idx.min() < 0 or idx.max() >= cdf.shape[0]):
        raise ValueError("index out of range of the CDF table")
    cap = L.clc_rans_encode_bound(sym.size)
    buf = np.empty(cap, dtype=np.uint8)
    n = L.clc_rans_encode(sym.ctypes.data, idx.ctypes.data, sym.size, cdf.ctypes.data, cdf.shape[1], ln.ctypes.data, off.ctypes.data,
                          buf.ctypes.data, cap)
    _lib.check(n, "clc_rans_encode")
    return buf[:n].tobytes()


def encode_direct(triples) -> bytes:
    """One stream from per-symbol (start, freq, esc) int32 triples ([n, 3], or flat 3 n) read from each symbol's own CDF row
    (clc_rans_encode_direct): the bytes ``encode`` gives for the same symbols coded through their full rows."""
    L = _lib.load()
    t = _i32(triples).reshape(-1)
    if t.size % 3:
        raise ValueError(f"encode_direct: the triples must be 3 n int32 values (got {t.size})")
    n = t.size // 3
    cap = L.clc_rans_encode_bound(n)
    buf = np.empty(cap, dtype=np.uint8)
    nb = L.clc_rans_encode_direct(t.ctypes.data, n, buf.ctypes.data, cap)
    _lib.check(nb, "clc_rans_encode_direct")
    return buf[:nb].tobytes()


class _Container(NamedTuple):
    """A multi-stream container: one image's independently decodable rANS streams as one string, little endian:

        magic | u8 count | u8 lane byte | 2 x u8 0 | count x u32 byte length | the streams, back to back

    Every stream is whole 32-bit words and at least ``least`` bytes, the coder state it starts with."""
    name: str       # of the public pair: name_pack / name_unpack
    magic: bytes
    letter: str     # the count, in messages
    noun: str       # one stream, in messages
    most: int       # streams per image
    least: int      # bytes of a stream
    lanes: int      # what header byte 5 must be: the rANS lanes of a stream, or 0 for a third pad byte


def stream_count(fmt, n, who, name=None):
    """-> the int n, the number of streams of one image in container fmt; refused by name (the caller's, or the format's letter)"""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= int(n) <= fmt.most:
        raise ValueError(f"{who}: {name or fmt.letter} must be between 1 and {fmt.most} {fmt.noun}s (got {n!r})")
    return int(n)


def _pack(fmt, streams) -> bytes:
    who = fmt.name + "_pack"
    streams = [bytes(s) for s in streams]
    stream_count(fmt, len(streams), who)
    for i, s in enumerate(streams):
        if len(s) < fmt.least or len(s) % 4:
            raise ValueError(f"{who}: {fmt.noun} {i} has {len(s)} bytes; a length must be a multiple of 4 and at least {fmt.least}")
    head = fmt.magic + bytes([len(streams), fmt.lanes, 0, 0]) + np.array([len(s) for s in streams], dtype="<u4").tobytes()
    return head + b"".join(streams)


def _unpack(fmt, blob) -> list:
    who = fmt.name + "_unpack"
    blob = bytes(blob)
    if len(blob) < 8 or blob[:4] != fmt.magic:
        raise ValueError(f"{who}: bad magic {blob[:4]!r} (a {fmt.name} stream starts with {fmt.magic!r})")
    n = stream_count(fmt, blob[4], who)
    pad = 6 if fmt.lanes else 5   # the first pad byte
    if fmt.lanes and blob[5] != fmt.lanes:
        raise ValueError(f"{who}: the lane byte must be {fmt.lanes} (got {blob[5]})")
    if blob[pad:8] != bytes(8 - pad):
        raise ValueError(f"{who}: non-zero pad byte in the header ({blob[pad:8].hex()})")
    if len(blob) < 8 + 4 * n:
        raise ValueError(f"{who}: the lengths do not add up to the blob ({len(blob)} bytes end inside the header of {fmt.letter} = {n})")
    lengths = [int(m) for m in np.frombuffer(blob, dtype="<u4", count=n, offset=8)]
    for i, m in enumerate(lengths):
        if m < fmt.least or m % 4:
            raise ValueError(f"{who}: {fmt.noun} {i} has length {m}; a length must be a multiple of 4 and at least {fmt.least}")
    if 8 + 4 * n + sum(lengths) != len(blob):
        raise ValueError(f"{who}: the lengths do not add up to the blob (header {8 + 4 * n} + {sum(lengths)} != {len(blob)} bytes)")
    out, at = [], 8 + 4 * n
    for m in lengths:
        out.append(blob[at:at + m])
        at += m
    return out


SPLIT_MAGIC = b"CGS1"
SPLIT_MAX = 64   # sub-streams per image: one wave each on the device decoder (clc_gmm_decode_step)
SPLIT_STREAM = _Container("split", SPLIT_MAGIC, "S", "sub-stream", SPLIT_MAX, 8, 0)


def split_pack(streams) -> bytes:
    """S independent rANS sub-streams of one image as one string, little endian:

        b"CGS1" | u8 S | 3 x u8 0 | S x u32 byte length | the S sub-streams, back to back

    Every sub-stream is a whole stream of ``encode_direct`` (32-bit words, at least the two of its final state).  Overhead: 8 + 4 S
    bytes of header plus the 8-byte final state of each sub-stream, 8 + 12 S bytes — 200 per image at S = 16 (the one stream it
    replaces carried one such state)."""
    return _pack(SPLIT_STREAM, streams)


def split_unpack(blob) -> list:
    """-> the S sub-streams of a ``split_pack`` string; anything malformed is refused by name."""
    return _unpack(SPLIT_STREAM, blob)


LANES_MAGIC = b"CLN1"
LANES = 64          # rANS lanes of a wave stream: one per GPU lane
LANES_MAX_W = 16    # wave streams per image: one wave each on the device coder (clc_rans_lanes_decode_step / clc_rans_lanes_encode)
LANES_STREAM = _Container("lanes", LANES_MAGIC, "W", "wave stream", LANES_MAX_W, 8 * LANES, LANES)


def lanes_pack(streams) -> bytes:
    """The W wave streams of one image's lane-interleaved stream (include/clc_hip.h: the "lanes" stream) as one string, little endian:

        b"CLN1" | u8 W | u8 64 | 2 x u8 0 | W x u32 byte length | the W wave streams, back to back

    A wave stream is 32-bit words and starts with its 64 lane states (512 bytes).  Overhead against the one stream of ``encode``:
    8 + 4 W bytes of header plus 512 W bytes of lane states.

    What the SEGMENTS of an image are is the model's: elic2022's 2 K passes, the slices of CLC / TCM in NHWC order, and for the two
    context models of models/hyperprior.py the dependent steps of their schedule — mbt2018: the non-empty steps of
    ar_schedule(H, W, "wavefront") in ascending t = w + 3 h, inside a step its pixels in ascending h, channels inner (ar_lanes_order;
    W + 3 (H - 1) segments at most, so its device encoder reads the lengths from memory: clc_rans_lanes_encode_list);
    mbt2018-checkerboard: the anchors, then the non-anchors, each in raster order with channels inner.  The container does not record
    the segments; encoder and decoder derive them from the latent's size."""
    return _pack(LANES_STREAM, streams)


def lanes_unpack(blob) -> list:
    """-> the W wave streams of a ``lanes_pack`` string; anything malformed is refused by name."""
    return _unpack(LANES_STREAM, blob)


def lanes_wave_symbols(segments, W):
    """-> per wave stream the number of symbols it carries: chunk q (64 symbols) of every segment belongs to wave q % W"""
    n_w = [0] * W
    for n in segments:
        n = int(n)
        for q in range((n + LANES - 1) // LANES):
            n_w[q % W] += min(LANES, n - q * LANES)
    return n_w


def lanes_encode(symbols, indexes, segments, W, cdfs, cdfs_sizes, offsets) -> list:
    """One image's symbols / indexes in stream order (the segments back to back) -> its W wave streams (bytes), by the host coder
    (clc_rans_lanes_encode_host): the bytes the device encoder writes."""
    L = _lib.load()
    W = stream_count(LANES_STREAM, W, "lanes_encode")
    sym, idx = _i32(symbols).reshape(-1), _i32(indexes).reshape(-1)
    seg = _i32(segments).reshape(-1)
    if sym.size != idx.size:
        raise ValueError("lanes_encode: symbols and indexes must have the same length")
    if (seg < 0).any() or int(seg.sum()) != sym.size:
        raise ValueError(f"lanes_encode: the segment lengths must be non-negative and add up to the {sym.size} symbols (got {seg.tolist()})")
    cdf, ln, off = _tables(cdfs, cdfs_sizes, offsets)
    cap = sum(L.clc_rans_lanes_bound(n) for n in lanes_wave_symbols(seg, W))
    buf = np.empty(cap, dtype=np.uint8)
    lengths = np.zeros(W, dtype=np.int32)
    n = L.clc_rans_lanes_encode_host(sym.ctypes.data, idx.ctypes.data, seg.ctypes.data, seg.size, W, cdf.ctypes.data, cdf.shape[1], cdf.shape[0],
                                     ln.ctypes.data, off.ctypes.data, buf.ctypes.data, cap, lengths.ctypes.data)
    _lib.check(n, "clc_rans_lanes_encode_host")
    ends = np.cumsum(lengths)
    return [buf[e - m:e].tobytes() for e, m in zip(ends, lengths)]


class LanesDecoder:
    """Incremental host decoder of one image's W wave streams (clc_rans_lanes_decoder_*): ``decode`` takes the next segment's indexes."""

    def __init__(self, streams):
        L = _lib.load()
        streams = [bytes(s) for s in streams]
        self.W = len(streams)
        self._h = None
        self.lengths = np.array([len(s) for s in streams], dtype=np.int32)
        b = np.frombuffer(b"".join(streams) or b"\0", dtype=np.uint8)
        self._h = L.clc_rans_lanes_decoder_create(b.ctypes.data, self.lengths.ctypes.data, self.W)
        if not self._h:
            raise _lib.ClcError(f"clc_rans_lanes_decoder_create failed: {L.clc_last_error().decode()}")

    def decode(self, indexes, cdfs, cdfs_sizes, offsets):
        L = _lib.load()
        idx = _i32(indexes).reshape(-1)
        cdf, ln, off = _tables(cdfs, cdfs_sizes, offsets)
        out = np.empty(idx.size, dtype=np.int32)
        n = L.clc_rans_lanes_decoder_decode(self._h, idx.ctypes.data, idx.size, cdf.ctypes.data, cdf.shape[1], cdf.shape[0], ln.ctypes.data,
                                            off.ctypes.data, out.ctypes.data)
        _lib.check(n, "clc_rans_lanes_decoder_decode")
        return out

    def state(self, w):
        """-> (the 64 lane states of wave stream w as uint64, the words consumed so far)"""
        L = _lib.load()
        x = np.empty(LANES, dtype=np.uint64)
        pos = C.c_long(0)
        _lib.check(L.clc_rans_lanes_decoder_state(self._h, int(w), x.ctypes.data, C.byref(pos)), "clc_rans_lanes_decoder_state")
        return x, int(pos.value)

    def at_end(self):
        """every wave stream decoded to its end: all lanes at 2^31 and pos == its word count"""
        for w in range(self.W):
            x, pos = self.state(w)
            if not (x == np.uint64(1 << 31)).all() or pos != int(self.lengths[w]) // 4:
                return False
        return True

    def close(self):
        if self._h:
            _lib.load().clc_rans_lanes_decoder_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_ROW_INDEX = {}   # n -> (arange(n), full(n, size)) int32: the index / size arrays of a decode over per-symbol rows


class _Decoder:
    def __init__(self, stream: bytes):
        L = _lib.load()
        b = np.frombuffer(stream, dtype=np.uint8)
        self._h = L.clc_rans_decoder_create(b.ctypes.data, b.size)
        if not self._h:
            raise _lib.ClcError(f"clc_rans_decoder_create failed: {L.clc_last_error().decode()}")
        self.words = 2

    def decode(self, indexes, cdfs, cdfs_sizes, offsets):
        L = _lib.load()
        idx = _i32(indexes).reshape(-1)
        cdf, ln, off = _tables(cdfs, cdfs_sizes, offsets)
        if idx.size and (idx.min() < 0 or idx.max() >= cdf.shape[0]):
            raise ValueError("index out of range of the CDF table")
        out = np.empty(idx.size, dtype=np.int32)
        n = L.clc_rans_decoder_decode(self._h, idx.ctypes.data, idx.size, cdf.ctypes.data, cdf.shape[1], ln.ctypes.data, off.ctypes.data,
                                      out.ctypes.data)
        _lib.check(n, "clc_rans_decoder_decode")
        self.words = n
        return out

    def decode_rows(self, rows, offsets):
        """The next n symbols, symbol i through its own row rows[i] (int32 [n, size], every entry used) at offsets[i]: numpy arrays
        (views of pinned buffers as they are), nothing goes through a Python list."""
        L = _lib.load()
        for a, what in ((rows, "rows"), (offsets, "offsets")):
            if not (isinstance(a, np.ndarray) and a.dtype == np.int32 and a.flags.c_contiguous):
                raise ValueError(f"decode_rows: {what} must be a C-contiguous int32 numpy array")
        if rows.ndim != 2 or offsets.size != rows.shape[0]:
            raise ValueError(f"decode_rows: rows [n, size] and n offsets (got {rows.shape}, {offsets.shape})")
        n, size = rows.shape
        key = (n, size)
        if key not in _ROW_INDEX:
            _ROW_INDEX[key] = (np.arange(n, dtype=np.int32), np.full(n, size, dtype=np.int32))
        idx, ln = _ROW_INDEX[key]
        out = np.empty(n, dtype=np.int32)
        w = L.clc_rans_decoder_decode(self._h, idx.ctypes.data, n, rows.ctypes.data, size, ln.ctypes.data, offsets.ctypes.data, out.ctypes.data)
        _lib.check(w, "clc_rans_decoder_decode")
        self.words = w
        return out

    def close(self):
        if self._h:
            _lib.load().clc_rans_decoder_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def decode(stream: bytes, indexes, cdfs, cdfs_sizes, offsets) -> np.ndarray:
    d = _Decoder(stream)
    try:
        return d.decode(indexes, cdfs, cdfs_sizes, offsets)
    finally:
        d.close()


class BufferedRansEncoder:
    """Buffers (symbols, indexes) chunks; flush() encodes them as ONE stream (same bytes as the reference coder)."""

    def __init__(self):
        self._sym, self._idx, self._tables = [], [], None

    def encode_with_indexes(self, symbols, indexes, cdfs, cdfs_sizes, offsets):
        self._sym.append(_i32(symbols).reshape(-1))
        self._idx.append(_i32(indexes).reshape(-1))
        self._tables = (cdfs, cdfs_sizes, offsets)

    def flush(self) -> bytes:
        if self._tables is None:
            out = encode(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((1, 2), np.int32), [2], [0])
        else:
            out = encode(np.concatenate(self._sym), np.concatenate(self._idx), *self._tables)
        self._sym, self._idx, self._tables = [], [], None
        return out


class RansEncoder:
    def encode_with_indexes(self, symbols, indexes, cdfs, cdfs_sizes, offsets) -> bytes:
        return encode(symbols, indexes, cdfs, cdfs_sizes, offsets)


class RansDecoder:
    def __init__(self):
        self._d = None

    def set_stream(self, stream: bytes):
        if self._d is not None:
            self._d.close()
        self._d = _Decoder(stream)

    def decode_stream(self, indexes, cdfs, cdfs_sizes, offsets):
        if self._d is None:
            raise ValueError("set_stream() must be called first")
        out = self._d.decode(indexes, cdfs, cdfs_sizes, offsets)
        return out if isinstance(indexes, np.ndarray) else out.tolist()

    def decode_rows(self, rows, offsets):
        """decode_stream over per-symbol CDF rows (see _Decoder.decode_rows)"""
        if self._d is None:
            raise ValueError("set_stream() must be called first")
        return self._d.decode_rows(rows, offsets)

    def decode_with_indexes(self, stream, indexes, cdfs, cdfs_sizes, offsets):
        self.set_stream(stream)
        return self.decode_stream(indexes, cdfs, cdfs_sizes, offsets)
