"""The lane-interleaved ("lanes") rANS stream without a GPU: the host coder (rans_host.cpp: clc_rans_lanes_encode_host,
clc_rans_lanes_decoder_*) against a restatement of the format in Python integers, the container (ans.lanes_pack / lanes_unpack), every
refusal by name — the host coder's, the container's, the model's (on stubbed device halves), and the argument refusals of the two device
entries, which return before any launch — and the default compress / decompress of elic2022, which must not notice any of it.

THE RESTATEMENT (include/clc_hip.h, "the lanes stream").  A segment's symbol j lies in chunk q = j // 64, lane j % 64; chunk q belongs
to wave q % W; a wave takes its chunks one per round.  Per round the decoder runs sub-steps t = 0, 1, ...: operation 0 is the symbol,
operations 1 .. exist only for a lane whose symbol was the row's tail (the count nibble, then the payload nibbles LSB first), every
operation ends with the renorm, and within a sub-step the renormalising lanes take the next words in ascending lane order.  The encoder
is the exact reverse.  Every comparison here is exact.

Inputs: W in {1, 3, 4}; the segment lists (1), (63, 64, 65), (64 W, 64 W + 1, 0, 200); the table of a GaussianConditional over 8 scales
from 0.11 to 64 (rows of 5 to 785 entries); symbols drawn from each row's own Gaussian, and planted: max_value - 1 (the last symbol
inside), max_value (the empty payload), -1 below the offset, +-10^6, one round in which seven lanes escape with 0, 1, 2, 3, 5, 6 and 8
payload nibbles, and an escape as the last symbol of every partial chunk.
"""
import ctypes

import numpy as np
import pytest
import torch

L31 = 1 << 31
M32 = 0xFFFFFFFF
LANES = 64
SEGMENT_LISTS = [lambda W: (1,), lambda W: (63, 64, 65), lambda W: (64 * W, 64 * W + 1, 0, 200)]
CASES = [(W, s) for W in (1, 3, 4) for s in range(len(SEGMENT_LISTS))]

_TABLE = []


def lanes_table():
    """(cdfs int32 [8, stride], cdf sizes, offsets) of a GaussianConditional over 8 scales from 0.11 to 64, built once"""
    if not _TABLE:
        from clc_amd.entropy_models import GaussianConditional

        gc = GaussianConditional([float(s) for s in np.geomspace(0.11, 64.0, 8)])
        gc.update()
        cdf, ln, off = gc.host_tables()
        assert cdf.shape[0] == 8 and int(ln.min()) <= 8 and int(ln.max()) >= 300   # a handful of entries to several hundred
        _TABLE.append((cdf, ln, off, np.geomspace(0.11, 64.0, 8)))
    return _TABLE[0][:3]


def lanes_case(W, which, seed=0):
    """-> (symbols, indexes, segments) of one image: int32 arrays in stream order and the tuple of segment lengths"""
    cdf, ln, off = lanes_table()
    scales = _TABLE[0][3]
    seg = SEGMENT_LISTS[which](W)
    g = np.random.default_rng(1000 * seed + 10 * W + which)
    T = sum(seg)
    idx = g.integers(0, 8, T).astype(np.int32)
    maxv = ln[idx] - 2
    val = np.clip(np.rint(g.normal(0.0, 1.0, T) * scales[idx]).astype(np.int64) - off[idx], 0, maxv - 1)   # inside the rows
    i = np.arange(T)
    val = np.where(i % 17 == 3, maxv - 1, val)
    val = np.where(i % 23 == 5, maxv, val)            # the tail itself: an escape with the empty payload
    val = np.where(i % 29 == 7, -1, val)              # -1 below the offset
    sym = val + off[idx]
    sym = np.where(i % 31 == 11, 10**6, sym)
    sym = np.where(i % 37 == 13, -10**6, sym)
    at = 0
    for p, n in enumerate(seg):
        if n >= LANES:   # one round with several lanes escaping, every one with another nibble count: 0, 1, 2, 3, 5, 6, 8
            for lane, raw in ((1, 0), (2, 1), (5, 0x10), (9, 0x400), (30, 0x12345), (31, 0x1E8480), (63, 0x80000000)):
                k = at + lane
                sym[k] = off[idx[k]] + (-(raw >> 1) - 1 if raw & 1 else (raw >> 1) + maxv[k])
        if n % LANES and not (n == 1 and W == 1):   # an escape in the last, partial chunk
            k = at + n - 1
            sym[k] = off[idx[k]] + (maxv[k] + 300, -2, 10**6)[(W + p) % 3]
        at += n
    return sym.astype(np.int32), idx, seg


# ---------------------------------------------------------------------------------------------- the format, restated in Python integers
def _ops_of(sym, ci, cdf, ln, off):
    """the operations of one symbol in the DECODER's order: (start, freq) of the symbol, then (nibble, 0) per escape nibble"""
    maxv = int(ln[ci]) - 2
    v = int(sym) - int(off[ci])
    raw = None
    if v < 0:
        raw, v = -2 * v - 1, maxv
    elif v >= maxv:
        raw, v = 2 * (v - maxv), maxv
    row = cdf[ci]
    ops = [(int(row[v]), int(row[v + 1]) - int(row[v]))]
    if raw is not None:
        assert raw < 1 << 32
        nb = 0
        while nb < 8 and raw >> (4 * nb):
            nb += 1
        ops.append((nb, 0))
        ops += [((raw >> (4 * k)) & 15, 0) for k in range(nb)]
    return ops


def _rounds(seg, W, w):
    """wave w's rounds: (first symbol of the chunk in stream order, active lanes)"""
    out, at = [], 0
    for n in seg:
        for q in range(w, (n + LANES - 1) // LANES, W):
            out.append((at + q * LANES, min(LANES, n - q * LANES)))
        at += n
    return out


def restated_encode(sym, idx, seg, W, cdf, ln, off):
    """-> per wave its list of 32-bit words"""
    streams = []
    for w in range(W):
        x, out = [L31] * LANES, []   # out is written backward: appended here, reversed at the end
        for first, active in reversed(_rounds(seg, W, w)):
            ops = [_ops_of(sym[first + l], idx[first + l], cdf, ln, off) for l in range(active)]
            for t in range(max(len(o) for o in ops) - 1, -1, -1):
                for l in range(active - 1, -1, -1):
                    if t >= len(ops[l]):
                        continue
                    start, freq = ops[l][t]
                    if freq:   # enc_put
                        if x[l] >= ((L31 >> 16) << 32) * freq:
                            out.append(x[l] & M32)
                            x[l] >>= 32
                        x[l] = ((x[l] // freq) << 16) + (x[l] % freq) + start
                    else:      # enc_put_bits
                        if x[l] >= ((L31 >> 16) << 32) * (1 << 12):
                            out.append(x[l] & M32)
                            x[l] >>= 32
                        x[l] = (x[l] << 4) | start
        for l in range(LANES - 1, -1, -1):
            out.append(x[l] >> 32)
            out.append(x[l] & M32)
        streams.append(out[::-1])
    return streams


class RestatedDecoder:
    def __init__(self, streams):
        self.words = [list(s) for s in streams]
        self.x = [[s[2 * l] | (s[2 * l + 1] << 32) for l in range(LANES)] for s in self.words]
        self.pos = [2 * LANES] * len(streams)

    def segment(self, idx, cdf, ln, off):
        W, n = len(self.words), len(idx)
        out = [0] * n
        for q in range((n + LANES - 1) // LANES):
            w = q % W
            x, words = self.x[w], self.words[w]
            active = min(LANES, n - q * LANES)
            tail, nb, base, raw = [False] * active, [0] * active, [2] * active, [0] * active

            def renorm(l):
                if x[l] < L31:
                    x[l] = (x[l] << 32) | (words[self.pos[w]] if self.pos[w] < len(words) else 0)
                    self.pos[w] += 1

            def nibble(l):
                v = x[l] & 15
                x[l] >>= 4
                renorm(l)
                return v

            for t in range(1 + 2 + 16):
                did = False
                for l in range(active):
                    ci = int(idx[q * LANES + l])
                    maxv = int(ln[ci]) - 2
                    if t == 0:
                        row, cf = cdf[ci], x[l] & 0xFFFF
                        s = max(j for j in range(maxv + 1) if int(row[j]) <= cf)
                        x[l] = (int(row[s + 1]) - int(row[s])) * (x[l] >> 16) + cf - int(row[s])
                        renorm(l)
                        out[q * LANES + l], tail[l], did = s, s == maxv, True
                    elif tail[l] and (t == 1 or (t == 2 and nb[l] == 15)):
                        nb[l] += nibble(l)
                        base[l] = 3 if t == 2 else 2
                        did = True
                    elif tail[l] and t - base[l] < min(nb[l], 16):
                        v = nibble(l)
                        if t - base[l] < 8:
                            raw[l] |= v << (4 * (t - base[l]))
                        did = True
                if not did:
                    break
            for l in range(active):
                ci = int(idx[q * LANES + l])
                if tail[l]:
                    out[q * LANES + l] = -(raw[l] >> 1) - 1 if raw[l] & 1 else (raw[l] >> 1) + int(ln[ci]) - 2
                out[q * LANES + l] += int(off[ci])
        return out

    def at_end(self):
        return all(all(v == L31 for v in x) for x in self.x) and self.pos == [len(w) for w in self.words]


# ------------------------------------------------------------------------------------------------------------------- the host coder
@pytest.mark.parametrize("W,which", CASES)
def test_host_coder_is_the_restatement(W, which):
    from clc_amd import ans

    cdf, ln, off = lanes_table()
    sym, idx, seg = lanes_case(W, which)
    streams = ans.lanes_encode(sym, idx, seg, W, cdf, ln, off)
    want = restated_encode(sym, idx, seg, W, cdf, ln, off)
    assert len(streams) == W
    assert [np.frombuffer(s, "<u4").tolist() for s in streams] == want
    n_w = ans.lanes_wave_symbols(seg, W)
    assert sum(n_w) == sum(seg) and all(len(s) <= 4 * (128 + 10 * n) for s, n in zip(streams, n_w))   # the capacity bound
    # both decoders return the symbols and end at (2^31 in every lane, the word count)
    r, d = RestatedDecoder(want), ans.LanesDecoder(streams)
    at = 0
    for n in seg:
        got = d.decode(idx[at:at + n], cdf, ln, off)
        assert got.tolist() == sym[at:at + n].tolist() == r.segment(idx[at:at + n], cdf, ln, off)
        at += n
    assert r.at_end() and d.at_end()
    for w in range(W):
        x, pos = d.state(w)
        assert x.tolist() == [L31] * LANES and pos == len(want[w])
    # the container
    blob = ans.lanes_pack(streams)
    assert blob[:8] == b"CLN1" + bytes([W, 64, 0, 0]) and np.frombuffer(blob, "<u4", W, 8).tolist() == [len(s) for s in streams]
    assert len(blob) == 8 + 4 * W + sum(len(s) for s in streams) and ans.lanes_unpack(blob) == streams == ans.lanes_unpack(bytearray(blob))
    # the size bound: 8 bytes of state per lane plus one slack word per lane over the one stream
    one = ans.encode(sym, idx, cdf, ln, off)
    print(f"W = {W}, segments {seg}: {len(blob)} bytes as lanes, {len(one)} as one stream, bound {len(one) + 8 + 4 * W + 64 * W * 12}")
    assert len(blob) <= len(one) + 8 + 4 * W + 64 * W * 12


def test_the_planted_symbols_are_there():
    cdf, ln, off = lanes_table()
    seen = set()
    for W, which in CASES:
        sym, idx, seg = lanes_case(W, which)
        v = sym.astype(np.int64) - off[idx]
        maxv = ln[idx] - 2
        seen |= {"inside"} if ((v >= 0) & (v < maxv - 1)).any() else set()
        seen |= {"last"} if (v == maxv - 1).any() else set()
        seen |= {"tail"} if (v == maxv).any() else set()
        seen |= {"below"} if (v == -1).any() else set()
        seen |= {"+1e6"} if (sym == 10**6).any() else set()
        seen |= {"-1e6"} if (sym == -10**6).any() else set()
        at = 0
        for n in seg:
            if n >= LANES:   # the round of many escapes: nibble counts 0, 1, 2, 3, 5, 6, 8 among its lanes
                counts = {len(_ops_of(sym[at + l], idx[at + l], cdf, ln, off)) - 2 for l in (1, 2, 5, 9, 30, 31, 63)}
                assert counts == {0, 1, 2, 3, 5, 6, 8}
                seen.add("round")
            if n % LANES and not (n == 1 and W == 1):
                assert len(_ops_of(sym[at + n - 1], idx[at + n - 1], cdf, ln, off)) > 1
                seen.add("partial")
            at += n
    assert seen == {"inside", "last", "tail", "below", "+1e6", "-1e6", "round", "partial"}


def test_one_lane_is_the_one_stream():
    """W = 1 and one symbol per segment: only lane 0 ever works, and its words are ans.encode's of the same symbols"""
    from clc_amd import ans

    cdf, ln, off = lanes_table()
    sym, idx, _ = lanes_case(3, 1)
    sym, idx = sym[:80], idx[:80]
    assert len({len(_ops_of(s, c, cdf, ln, off)) for s, c in zip(sym, idx)}) >= 4   # escapes of several lengths among them
    (stream,) = ans.lanes_encode(sym, idx, [1] * 80, 1, cdf, ln, off)
    words = np.frombuffer(stream, "<u4").tolist()
    one = np.frombuffer(ans.encode(sym, idx, cdf, ln, off), "<u4").tolist()
    assert words[:2] == one[:2] and words[2:128] == [L31, 0] * 63 and words[128:] == one[2:]


def test_truncated_and_foreign_words():
    """a truncated stream feeds zeros; other words give wrong symbols and nothing worse; neither ends where a whole stream ends"""
    from clc_amd import ans

    cdf, ln, off = lanes_table()
    sym, idx, seg = lanes_case(3, 2)
    streams = ans.lanes_encode(sym, idx, seg, 3, cdf, ln, off)
    assert len(streams[1]) > 4 * 140
    cut = [streams[0], streams[1][:4 * 130], streams[2]]
    g = np.random.default_rng(5)
    noise = [g.integers(0, 256, len(s), dtype=np.uint8).tobytes() for s in streams]
    for bad in (cut, noise):
        d = ans.LanesDecoder(bad)
        r = RestatedDecoder([np.frombuffer(s, "<u4").tolist() for s in bad])
        at = 0
        for n in seg:
            assert d.decode(idx[at:at + n], cdf, ln, off).tolist() == [((v + L31) & M32) - L31 for v in r.segment(idx[at:at + n], cdf, ln, off)]
            at += n
        assert not d.at_end() and not r.at_end()
        for w in range(3):
            x, pos = d.state(w)
            assert x.tolist() == r.x[w] and pos == r.pos[w]
    d = ans.LanesDecoder(cut)
    for n, at in zip(seg, np.cumsum((0,) + seg[:-1])):
        d.decode(idx[at:at + n], cdf, ln, off)
    assert d.state(1)[1] > 130 and d.state(0)[1] == len(streams[0]) // 4   # pos runs past the cut stream's end; wave 0 is its own stream


# ------------------------------------------------------------------------------------------------------------------------- refusals
def test_host_coder_refusals_by_name():
    from clc_amd import ans, lib

    cdf, ln, off = lanes_table()
    sym, idx, seg = lanes_case(3, 1)
    for W in (0, 17, -1, True, 2.0):
        with pytest.raises(ValueError, match="W must be between 1 and 16"):
            ans.lanes_encode(sym, idx, seg, W, cdf, ln, off)
    with pytest.raises(lib.ClcError, match="clc_rans_lanes_encode_host: index 8 outside the table of 8 rows"):
        ans.lanes_encode(sym, np.where(np.arange(idx.size) == 70, 8, idx), seg, 3, cdf, ln, off)
    with pytest.raises(lib.ClcError, match="clc_rans_lanes_encode_host: index -1 outside the table"):
        ans.lanes_encode(sym, np.where(np.arange(idx.size) == 3, -1, idx), seg, 3, cdf, ln, off)
    for size in (1, cdf.shape[1] + 1):
        bad_ln = ln.copy()
        bad_ln[int(idx[10])] = size
        with pytest.raises(lib.ClcError, match=f"clc_rans_lanes_encode_host: bad cdf size {size} at index {int(idx[10])}"):
            ans.lanes_encode(sym, idx, seg, 3, cdf, bad_ln, off)
    flat = np.array([[0, 5, 5, 65536]], dtype=np.int32)   # symbol 1 has frequency 0
    with pytest.raises(lib.ClcError, match="clc_rans_lanes_encode_host: zero-frequency symbol"):
        ans.lanes_encode([0, 1, 0], [0, 0, 0], [3], 2, flat, [4], [0])
    with pytest.raises(ValueError, match="add up to the 192 symbols"):
        ans.lanes_encode(sym, idx, (63, 64), 3, cdf, ln, off)
    with pytest.raises(ValueError, match="same length"):
        ans.lanes_encode(sym, idx[:-1], seg, 3, cdf, ln, off)
    # the C entries themselves: W, and the streams' lengths
    L = lib.load()
    buf = (ctypes.c_int32 * 4096)()
    p = ctypes.addressof(buf)
    for W in (0, 17):
        assert L.clc_rans_lanes_encode_host(p, p, p, 1, W, p, 4, 1, p, p, p, 4096, p) == -1
        assert "clc_rans_lanes_encode_host: W must be between 1 and 16" in L.clc_last_error().decode()
        assert not L.clc_rans_lanes_decoder_create(p, p, W)
        assert "clc_rans_lanes_decoder_create: W must be between 1 and 16" in L.clc_last_error().decode()
    streams = ans.lanes_encode(sym, idx, seg, 3, cdf, ln, off)
    for bad in (streams[1][:508], streams[1][:-2], b""):
        with pytest.raises(lib.ClcError, match=rf"wave stream 1 has {len(bad)} bytes; a stream must be >= 512 bytes, multiple of 4"):
            ans.LanesDecoder([streams[0], bad, streams[2]])
    with pytest.raises(lib.ClcError, match="W must be between 1 and 16"):
        ans.LanesDecoder([streams[0]] * 17)
    d = ans.LanesDecoder(streams)
    before = [d.state(w) for w in range(3)]
    with pytest.raises(lib.ClcError, match="clc_rans_lanes_decoder_decode: index 8 outside the table"):
        d.decode(np.where(np.arange(63) == 62, 8, idx[:63]), cdf, ln, off)
    bad_ln = ln.copy()
    bad_ln[int(idx[5])] = 0
    with pytest.raises(lib.ClcError, match="clc_rans_lanes_decoder_decode: bad cdf size 0"):
        d.decode(idx[:63], cdf, bad_ln, off)
    for w in range(3):   # a refused call changed no state
        assert d.state(w)[0].tolist() == before[w][0].tolist() and d.state(w)[1] == before[w][1] == 128
    assert d.decode(idx[:63], cdf, ln, off).tolist() == sym[:63].tolist()


def test_container_refusals_by_name():
    from clc_amd import ans

    g = np.random.default_rng(0)
    subs = [g.integers(0, 256, 512 + 4 * int(g.integers(0, 40)), dtype=np.uint8).tobytes() for _ in range(4)]
    blob = ans.lanes_pack(subs)
    assert ans.lanes_unpack(blob) == subs
    with pytest.raises(ValueError, match="bad magic"):
        ans.lanes_unpack(b"CLN2" + blob[4:])
    with pytest.raises(ValueError, match="bad magic"):
        ans.lanes_unpack(b"CGS1" + blob[4:])   # a cheng2020 split string is not a lanes string
    with pytest.raises(ValueError, match="bad magic"):
        ans.lanes_unpack(subs[0])
    for W in (0, 17, 255):
        with pytest.raises(ValueError, match=rf"W must be between 1 and 16.*got {W}"):
            ans.lanes_unpack(blob[:4] + bytes([W]) + blob[5:])
    for lanes in (0, 32, 65):
        with pytest.raises(ValueError, match=rf"lane byte must be 64 \(got {lanes}\)"):
            ans.lanes_unpack(blob[:5] + bytes([lanes]) + blob[6:])
    for at in (6, 7):
        with pytest.raises(ValueError, match="non-zero pad byte"):
            ans.lanes_unpack(blob[:at] + b"\x01" + blob[at + 1:])
    lens = lambda *v: blob[:8] + np.array(v, dtype="<u4").tobytes() + blob[24:]
    n = [len(s) for s in subs]
    with pytest.raises(ValueError, match="wave stream 1 has length .* multiple of 4 and at least 512"):
        ans.lanes_unpack(lens(n[0], n[1] + 2, n[2], n[3]))
    with pytest.raises(ValueError, match="wave stream 2 has length 508; .* multiple of 4 and at least 512"):
        ans.lanes_unpack(lens(n[0], n[1], 508, n[3]))
    with pytest.raises(ValueError, match="do not add up"):
        ans.lanes_unpack(lens(n[0], n[1], n[2], n[3] + 4))
    with pytest.raises(ValueError, match="do not add up"):
        ans.lanes_unpack(blob + b"\0\0\0\0")
    with pytest.raises(ValueError, match="do not add up"):
        ans.lanes_unpack(blob[:-4])
    with pytest.raises(ValueError, match="do not add up"):
        ans.lanes_unpack(blob[:12])   # ends inside the header
    with pytest.raises(ValueError, match="W must be between 1 and 16"):
        ans.lanes_pack([])
    with pytest.raises(ValueError, match="W must be between 1 and 16"):
        ans.lanes_pack(subs * 5)
    with pytest.raises(ValueError, match="wave stream 1 has 510 bytes"):
        ans.lanes_pack([subs[0], subs[1][:510]])
    with pytest.raises(ValueError, match="wave stream 0 has 8 bytes"):
        ans.lanes_pack([b"12345678"])


def _small_model():
    from clc_amd import models

    return models.Elic2022(N=8, M=32, groups=(4, 4, 8, 16), ch_widths=(12, 8), agg_widths=(40, 24))


def test_model_refusals_by_name():
    from clc_amd import ans

    p = _small_model()
    x = torch.zeros(1, 3, 64, 64)
    for lanes in (0, 17, -1, True, 4.0, "4"):
        with pytest.raises(ValueError, match=r"Elic2022.compress: lanes must be between 1 and 16"):
            p.compress(x, lanes=lanes)
        with pytest.raises(ValueError, match=r"Elic2022.decompress: lanes must be between 1 and 16"):
            p.decompress([[b""], [b""]], (1, 1), lanes=lanes)
    g = np.random.default_rng(1)
    wave = lambda: g.integers(0, 256, 520, dtype=np.uint8).tobytes()
    two, four = ans.lanes_pack([wave(), wave()]), ans.lanes_pack([wave() for _ in range(4)])
    # the headers are parsed before any device work: nothing below reaches a kernel or an upload
    with pytest.raises(ValueError, match=r"lanes = 2, but the header of image 1 says 4 wave streams"):
        p.decompress([[two, four], [b"", b""]], (1, 1), lanes=2)
    with pytest.raises(ValueError, match="bad magic"):   # a default-format string handed to the lanes decoder
        p.decompress([[wave()], [b""]], (1, 1), lanes=4)
    with pytest.raises(ValueError, match=r"image 1 is a lanes stream \(b'CLN1'\); pass lanes= \(its header says 4 wave streams\)"):
        p.decompress([[wave(), four], [b"", b""]], (1, 1))
    with pytest.raises(ValueError, match="non-zero pad byte"):
        p.decompress([[two[:7] + b"\x02" + two[8:]], [b""]], (1, 1), lanes=2)


def test_device_entries_refuse_their_arguments_before_any_launch():
    """Each call hands the library host buffers where device pointers belong: a launch would fault, a refusal returns -1 first."""
    from clc_amd import lib

    Lb = lib.load()
    ibuf = (ctypes.c_int32 * 4096)()
    ip = ctypes.addressof(ibuf)

    def refused(rc, who, what):
        assert rc == -1
        msg = Lb.clc_last_error().decode()
        assert who + ":" in msg and what in msg, msg

    names = ("idx", "ld_idx", "n", "B", "cdfs", "stride", "rows", "sizes", "offs", "words", "spans", "state", "W", "sym", "ld_sym", "st")
    base = dict(idx=ip, ld_idx=100, n=100, B=2, cdfs=ip, stride=8, rows=4, sizes=ip, offs=ip, words=ip, spans=ip, state=ip, W=4, sym=ip, ld_sym=100,
                st=None)
    call = lambda **k: Lb.clc_rans_lanes_decode_step(*[{**base, **k}[n] for n in names])
    who = "clc_rans_lanes_decode_step"
    for name in ("idx", "words", "spans", "state", "sym"):
        refused(call(**{name: None}), who, "null pointer")
    for name in ("cdfs", "sizes", "offs"):
        refused(call(**{name: None}), who, "null table pointer")
    refused(call(stride=1), who, "cdf_stride >= 2")
    refused(call(rows=0), who, "n_rows >= 1")
    refused(call(W=0), who, "W must be between 1 and 16")
    refused(call(W=17), who, "W must be between 1 and 16")
    refused(call(n=-1), who, "n must not be negative")
    refused(call(B=0), who, "B must be positive")
    refused(call(ld_idx=99), who, "ld_idx or ld_sym < n")
    refused(call(ld_sym=99), who, "ld_idx or ld_sym < n")
    refused(call(B=1 << 23), who, "B * W must be below 2^24")
    assert call(n=0, ld_idx=0, ld_sym=0) == 0   # an empty segment: nothing to do, nothing launched

    segs = lib.LanesSegments()
    segs.P, segs.n[0], segs.n[1] = 2, 60, 40
    names = ("sym", "idx", "ld", "B", "segs", "W", "cdfs", "stride", "rows", "sizes", "offs", "out", "regions", "result", "st")
    base = dict(sym=ip, idx=ip, ld=100, B=2, segs=segs, W=4, cdfs=ip, stride=8, rows=4, sizes=ip, offs=ip, out=ip, regions=ip, result=ip, st=None)
    call = lambda **k: Lb.clc_rans_lanes_encode(*[{**base, **k}[n] for n in names])
    who = "clc_rans_lanes_encode"
    for name in ("sym", "idx", "out", "regions", "result"):
        refused(call(**{name: None}), who, "null pointer")
    for name in ("cdfs", "sizes", "offs"):
        refused(call(**{name: None}), who, "null table pointer")
    refused(call(stride=1), who, "cdf_stride >= 2")
    refused(call(rows=0), who, "n_rows >= 1")
    refused(call(W=0), who, "W must be between 1 and 16")
    refused(call(W=17), who, "W must be between 1 and 16")
    refused(call(B=0), who, "B must be positive")
    refused(call(ld=99), who, "ld < the segments' total")
    bad = lib.LanesSegments()
    bad.P = 33
    refused(call(segs=bad), who, "P must be between 0 and 32")
    bad.P, bad.n[0] = 1, -5
    refused(call(segs=bad), who, "segment 0 has a negative length")
    bad.n[0] = 1 << 27
    refused(call(segs=bad, ld=1 << 27), who, "symbols per image")
    refused(call(B=1 << 23), who, "B * W must be below 2^24")


def test_wrapper_refusals_without_a_device():
    """the Python wrappers refuse host tensors by name before they touch the library"""
    from clc_amd import ops

    t = torch.zeros(64, dtype=torch.int32)
    with pytest.raises(ValueError, match="rans_lanes_decode_step: indexes must be a contiguous int32 device tensor"):
        ops.rans_lanes_decode_step(t, 64, (t, t, t), t, t, t, t)
    with pytest.raises(ValueError, match="rans_lanes_encode: symbols must be a contiguous int32 \\[B, T\\] device tensor"):
        ops.rans_lanes_encode(t.view(1, 64), t.view(1, 64), [64], 2, (t, t, t))
    with pytest.raises(ValueError, match="rans_lanes_encode: W must be between 1 and 16"):
        ops.rans_lanes_encode(t.view(1, 64), t.view(1, 64), [64], 0, (t, t, t))
    r = ops.rans_lanes_regions([130, 1], 2, 3)   # waves 0 and 1 carry 64 + 2 + 1 and 64 symbols
    assert r.shape == (3, 2, 2) and r[0].tolist() == [[0, 128 + 670], [798, 128 + 640]] and r[2, 1].tolist() == [2 * 1566 + 798, 768]


# ---------------------------------------------------------------------------------------------------------------- the default stays put
def test_defaults_are_todays_code_path(monkeypatch):
    """the device halves stubbed (fixed symbols on the CPU), so the host halves of compress / decompress run without a GPU"""
    from clc_amd import ans

    p = _small_model()
    p.update(force=True)
    cdf, ln, off = p.gaussian_conditional.host_tables()
    B, H, W = 2, 2, 3
    g = np.random.default_rng(7)
    syms = [torch.from_numpy(g.integers(-40, 40, (B, H * W, c)).astype(np.int32)) for c in p.groups]
    idxs = [torch.from_numpy(g.integers(0, cdf.shape[0], (B, H * W, c)).astype(np.int32)) for c in p.groups]
    monkeypatch.setattr(p, "_code_inputs", lambda x: (torch.zeros(B, p.M, H, W), "params", [b"z0", b"z1"], (1, 2)))
    monkeypatch.setattr(p, "_scctx_encode", lambda y, params: (syms, idxs, None))
    from clc_amd.models import scctx_order

    order = scctx_order(H, W, p.groups)
    sym_s = [np.ascontiguousarray(torch.cat(syms, 2)[b].numpy()[order[:, 0], order[:, 1]]) for b in range(B)]
    idx_s = [np.ascontiguousarray(torch.cat(idxs, 2)[b].numpy()[order[:, 0], order[:, 1]]) for b in range(B)]
    for item in (p.compress(None), p.compress(None, lanes=None)):
        assert sorted(item) == ["kernel_config", "shape", "strings"]   # no "lanes"
        assert item["strings"] == [[ans.encode(sym_s[b], idx_s[b], cdf, ln, off) for b in range(B)], [b"z0", b"z1"]]
    # compress(lanes=): the flat stream-order buffers and the 2 K segments reach the device half as they are
    seen = {}

    def fake(sym, idx, segments, Wn):
        seen.update(sym=sym, idx=idx, segments=segments, W=Wn)
        return [ans.lanes_pack(ans.lanes_encode(sym[b].numpy(), idx[b].numpy(), segments, Wn, cdf, ln, off)) for b in range(B)]

    monkeypatch.setattr(p, "_lanes_encode_device", fake)
    lanes = p.compress(None, lanes=3)
    assert sorted(lanes) == ["kernel_config", "lanes", "shape", "strings"] and lanes["lanes"] == 3
    assert lanes["kernel_config"] == item["kernel_config"] and lanes["strings"][1] == item["strings"][1]
    assert seen["W"] == 3 and seen["segments"] == [3 * 4, 3 * 4, 3 * 4, 3 * 4, 3 * 8, 3 * 8, 3 * 16, 3 * 16]   # 3 anchors, 3 non-anchors
    assert [seen["sym"][b].numpy().tolist() for b in range(B)] == [s.tolist() for s in sym_s]
    assert [seen["idx"][b].numpy().tolist() for b in range(B)] == [s.tolist() for s in idx_s]
    for b in range(B):   # ... and decode on the host coder, segment by segment, to the symbols
        d = ans.LanesDecoder(ans.lanes_unpack(lanes["strings"][0][b]))
        got = np.concatenate([d.decode(idx_s[b][a:a + n], cdf, ln, off) for a, n in zip(np.cumsum([0] + seen["segments"][:-1]), seen["segments"])])
        assert got.tolist() == sym_s[b].tolist() and d.at_end()

    # decompress: the default goes through _scctx_decode and nothing else
    calls = []
    monkeypatch.setattr(p.entropy_bottleneck, "decompress", lambda s, shape: "z_hat")
    monkeypatch.setattr(p, "_hyper_synthesis", lambda z: "params")
    monkeypatch.setattr(p, "_scctx_decode", lambda s, params: calls.append(("one", s, params)) or torch.zeros(1))
    monkeypatch.setattr(p, "_scctx_decode_lanes", lambda subs, params, dc: calls.append(("lanes", len(subs), len(subs[0]), dc)) or (torch.zeros(1), []))
    monkeypatch.setattr(p, "_synthesis", lambda y: y + 2.0)
    for out in (p.decompress(item["strings"], (1, 2)), p.decompress(item["strings"], (1, 2), lanes=None)):
        assert sorted(out) == ["x_hat"] and float(out["x_hat"]) == 1.0
    assert calls == [("one", item["strings"][0], "params")] * 2
    p.decompress(lanes["strings"], (1, 2), lanes=3, device_coder=False, check=False)
    assert calls[-1] == ("lanes", 2, 3, False)
