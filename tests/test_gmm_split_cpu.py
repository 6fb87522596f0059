"""The split stream of cheng2020 (K > 1) without a GPU: ans.split_pack / split_unpack with their refusals, the model's refusals, the
coder's END-STATE PROPERTY that decompress(..., check=True) rests on, the argument refusals of clc_gmm_decode_step (which return before
any launch), and the default compress / decompress, which must not notice any of it.

END-STATE PROPERTY.  The coder's integer arithmetic (rans_host.cpp: enc_put, enc_put_bits, the escape, renorm) is restated here in
Python integers.  Over random strictly increasing rows ending in 65536, symbols inside, below and above the window and escape payloads
0, 1, 300, 2 * 10^6, 2^31 - 1 and 2^32 - 1, the restated encoder's words are the library's, and the restated decoder returns the symbols
and ends at x == 2^31 with pos == the word count.  (A triple's esc is an int32, so ans.encode_direct carries payloads up to 2^31 - 1;
the payload 2^32 - 1 — the symbol offset - 2^31 — goes through ans.encode on the full rows, which produces the same stream format.)
"""
import ctypes

import numpy as np
import pytest
import torch

STRIDE = 67          # lib.GMM_ROW_STRIDE: L + 2 entries, L = 65
L = STRIDE - 2
L31 = 1 << 31
M32 = 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------------------ the container of S streams
def _streams(S, seed=0):
    g = np.random.default_rng(seed)
    return [g.integers(0, 256, 4 * int(g.integers(2, 40)), dtype=np.uint8).tobytes() for _ in range(S)]


@pytest.mark.parametrize("S", [1, 4, 64])
def test_split_round_trip(S):
    from clc_amd import ans

    subs = _streams(S, S)
    blob = ans.split_pack(subs)
    assert blob[:4] == b"CGS1" and blob[4] == S and blob[5:8] == b"\0\0\0"
    assert np.frombuffer(blob, "<u4", S, 8).tolist() == [len(s) for s in subs]
    assert len(blob) == 8 + 4 * S + sum(len(s) for s in subs)   # the overhead: 8 + 4 S bytes of header
    assert blob[8 + 4 * S:] == b"".join(subs)
    assert ans.split_unpack(blob) == subs
    assert ans.split_unpack(bytearray(blob)) == subs


def test_split_refusals_by_name():
    from clc_amd import ans

    subs = _streams(4)
    blob = ans.split_pack(subs)
    with pytest.raises(ValueError, match="bad magic"):
        ans.split_unpack(b"CGS2" + blob[4:])
    with pytest.raises(ValueError, match="bad magic"):
        ans.split_unpack(subs[0])   # a one-stream string is not a split string
    for S in (0, 65, 255):
        with pytest.raises(ValueError, match=rf"S must be between 1 and 64.*got {S}"):
            ans.split_unpack(blob[:4] + bytes([S]) + blob[5:])
    for at in (5, 6, 7):
        with pytest.raises(ValueError, match="non-zero pad byte"):
            ans.split_unpack(blob[:at] + b"\x01" + blob[at + 1:])
    lens = lambda *v: blob[:8] + np.array(v, dtype="<u4").tobytes() + blob[24:]
    n = [len(s) for s in subs]
    with pytest.raises(ValueError, match="sub-stream 1 has length .* multiple of 4 and at least 8"):
        ans.split_unpack(lens(n[0], n[1] + 2, n[2], n[3]))
    with pytest.raises(ValueError, match="sub-stream 2 has length 4; .* multiple of 4 and at least 8"):
        ans.split_unpack(lens(n[0], n[1], 4, n[3]))
    with pytest.raises(ValueError, match="do not add up"):
        ans.split_unpack(lens(n[0], n[1], n[2], n[3] + 4))
    with pytest.raises(ValueError, match="do not add up"):
        ans.split_unpack(blob + b"\0\0\0\0")
    with pytest.raises(ValueError, match="do not add up"):
        ans.split_unpack(blob[:-4])
    with pytest.raises(ValueError, match="do not add up"):
        ans.split_unpack(blob[:12])   # ends inside the header
    with pytest.raises(ValueError, match="S must be between 1 and 64"):
        ans.split_pack([])
    with pytest.raises(ValueError, match="S must be between 1 and 64"):
        ans.split_pack(_streams(65))
    with pytest.raises(ValueError, match="sub-stream 1 has 6 bytes"):
        ans.split_pack([subs[0], b"123456"])
    with pytest.raises(ValueError, match="sub-stream 0 has 4 bytes"):
        ans.split_pack([b"1234"])


def test_model_refusals_by_name():
    from clc_amd import ans, models

    p = models.Cheng2020Anchor(24, 3)
    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(ValueError, match=r"substreams = 25 > N = 24"):
        p.compress(x, substreams=25)
    with pytest.raises(ValueError, match=r"substreams must be between 1 and 64"):
        p.compress(x, substreams=0)
    with pytest.raises(ValueError, match=r"substreams must be between 1 and 64"):
        models.Cheng2020Anchor(96, 2).compress(x, substreams=65)
    with pytest.raises(ValueError, match=r"substreams = 25 > N = 24"):
        p.decompress([[b""], [b""]], (1, 1), substreams=25)
    one = models.Cheng2020Attention(24, 1)
    with pytest.raises(ValueError, match=r"K = 1 stream is CompressAI's"):
        one.compress(x, substreams=4)
    with pytest.raises(ValueError, match=r"K = 1 stream is CompressAI's"):
        one.decompress([[b""], [b""]], (1, 1), substreams=4)
    blob = ans.split_pack(_streams(4))
    with pytest.raises(ValueError, match=r"substreams = 2, but the header of image 1 says 4"):
        p.decompress([[ans.split_pack(_streams(2)), blob], [b"", b""]], (1, 1), substreams=2)
    with pytest.raises(ValueError, match="bad magic"):   # a default-format string handed to the split decoder
        p.decompress([[_streams(1)[0]], [b""]], (1, 1), substreams=4)


# ------------------------------------------------------------------------------------------------------ the coder, restated in integers
def _enc_put(x, out, start, freq):
    if x >= ((L31 >> 16) << 32) * freq:
        out.append(x & M32)
        x >>= 32
    return ((x // freq) << 16) + (x % freq) + start


def _enc_put_bits(x, out, val):
    if x >= ((L31 >> 16) << 32) * (1 << 12):
        out.append(x & M32)
        x >>= 32
    return (x << 4) | val


def _enc_escape(x, out, raw):
    nb = 0
    while nb < 8 and (raw >> (4 * nb)) != 0:
        nb += 1
    for j in range(nb - 1, -1, -1):
        x = _enc_put_bits(x, out, (raw >> (4 * j)) & 15)
    full, rem = divmod(nb, 15)
    x = _enc_put_bits(x, out, rem)
    for _ in range(full):
        x = _enc_put_bits(x, out, 15)
    return x


def _encode(triples):
    """(start, freq, raw or -1) per symbol -> the stream's 32-bit words"""
    x, out = L31, []
    for start, freq, raw in reversed(triples):
        if raw >= 0:
            x = _enc_escape(x, out, raw)
        x = _enc_put(x, out, start, freq)
    out.append(x >> 32)
    out.append(x & M32)
    return out[::-1]


class _Dec:
    def __init__(self, words):
        self.words, self.pos, self.x = words, 2, words[0] | (words[1] << 32)

    def renorm(self):
        if self.x < L31:
            w = self.words[self.pos] if self.pos < len(self.words) else 0
            self.pos += 1
            self.x = (self.x << 32) | w

    def bits(self):
        v = self.x & 15
        self.x >>= 4
        self.renorm()
        return v

    def symbol(self, row):
        """-> the value relative to the row's offset"""
        cf = self.x & 0xFFFF
        s = max(j for j in range(len(row) - 1) if row[j] <= cf)
        self.x = (row[s + 1] - row[s]) * (self.x >> 16) + cf - row[s]
        self.renorm()
        if s != len(row) - 2:
            return s
        v = self.bits()
        nb = v
        while v == 15:
            v = self.bits()
            nb += v
        raw = 0
        for j in range(nb):
            b = self.bits()
            if j < 8:
                raw |= b << (4 * j)
        return -(raw >> 1) - 1 if raw & 1 else (raw >> 1) + len(row) - 2


def _random_rows(n, g):
    rows = np.zeros((n, STRIDE), dtype=np.int32)
    for r in rows:
        r[1:L + 1] = np.sort(g.choice(np.arange(1, 65536), L, replace=False))
        r[L + 1] = 65536
    rows[0, 1:L + 1] = np.arange(1, L + 1)            # every regular frequency 1, the tail's 65471
    rows[1, 1:L + 1] = 65536 - L + np.arange(L)       # the first symbol takes almost everything, the tail's frequency is 1
    return rows


def _value_of(raw):
    return -(raw >> 1) - 1 if raw & 1 else (raw >> 1) + L


def _triple(row, v):
    if v < 0:
        return int(row[L]), 65536 - int(row[L]), -2 * v - 1
    if v >= L:
        return int(row[L]), 65536 - int(row[L]), 2 * (v - L)
    return int(row[v]), int(row[v + 1] - row[v]), -1


PAYLOADS = [0, 1, 300, 2_000_000, (1 << 31) - 1]


@pytest.mark.parametrize("seed", range(6))
def test_end_state_property(seed):
    from clc_amd import ans

    g = np.random.default_rng(seed)
    n = 50 + 40 * seed
    rows = _random_rows(n, g)
    values = g.integers(0, L, n)
    values[::5] = -1 - g.integers(0, 50, len(values[::5]))                 # below the window
    values[2::5] = L + g.integers(0, 50, len(values[2::5]))                # above it (L itself: the empty payload)
    for i, raw in enumerate(PAYLOADS + [2 * 10**6 + 1, 15, 16, 0x1234, 0x12345, 0xFFFFFFF, 0x10000000]):   # every nibble count 0 .. 8 is in here
        values[3 + 4 * i] = _value_of(raw)
    values[0], values[1], values[n - 1] = 0, L - 1, L                      # the window's first and last; the stream ENDS on an empty payload
    triples = [_triple(rows[i], int(values[i])) for i in range(n)]
    assert {t[2] for t in triples} >= set(PAYLOADS)
    assert {len(f"{t[2]:x}") for t in triples if t[2] > 0} == set(range(1, 9))
    words = _encode(triples)
    direct = ans.encode_direct(np.array(triples, dtype=np.int64).astype(np.int32))
    assert np.frombuffer(direct, "<u4").tolist() == words
    for cut in (n, n // 3):   # the property holds for every stream the encoder can produce: a prefix of the symbols is one too
        w = words if cut == n else _encode(triples[:cut])
        d = _Dec(w)
        assert [d.symbol(rows[i].tolist()) for i in range(cut)] == [int(v) for v in values[:cut]]
        assert d.x == L31 and d.pos == len(w), (d.x, d.pos, len(w))
    # ... and the library's decoder agrees on symbols and on the words consumed
    dd = ans.RansDecoder()
    dd.set_stream(direct)
    assert dd.decode_rows(rows, np.zeros(n, np.int32)).tolist() == [int(v) for v in values]
    assert dd._d.words == len(words)
    # a flipped word does not end there (what check= sees), and a truncated stream runs past its end.  (The end state is no checksum:
    # the escape's payload nibbles are raw bits, so a changed bit inside one decodes to another symbol and still ends clean.)
    bad = list(words)
    bad[len(bad) // 2] ^= M32
    d = _Dec(bad)
    for i in range(n):
        d.symbol(rows[i].tolist())
    assert (d.x, d.pos) != (L31, len(bad))
    d = _Dec(words[:2])
    for i in range(n):
        d.symbol(rows[i].tolist())
    assert d.pos > 2 or n < 3


def test_end_state_with_the_full_32_bit_payload():
    """raw = 2^32 - 1 is the symbol offset - 2^31: beyond an int32 esc, so it is coded through ans.encode on the full rows"""
    from clc_amd import ans

    g = np.random.default_rng(99)
    n = 12
    rows = _random_rows(n, g)
    values = [int(v) for v in g.integers(0, L, n)]
    values[4], values[n - 1] = -(1 << 31), -(1 << 31)
    trip = []
    for i, v in enumerate(values):
        t = _triple(rows[i], v)
        trip.append(t)
    assert trip[4][2] == trip[n - 1][2] == (1 << 32) - 1
    words = _encode(trip)
    full = ans.encode(np.array(values, dtype=np.int64).astype(np.int32), np.arange(n, dtype=np.int32), rows, np.full(n, STRIDE, np.int32),
                      np.zeros(n, np.int32))
    assert np.frombuffer(full, "<u4").tolist() == words
    d = _Dec(words)
    assert [d.symbol(rows[i].tolist()) for i in range(n)] == values
    assert d.x == L31 and d.pos == len(words)


# ------------------------------------------------------------------------------------------------------------------------- the C entry
def test_decode_step_argument_refusals_return_before_any_launch():
    """Each call hands the library host buffers where device pointers belong: a launch would fault, a refusal returns -1 first."""
    from clc_amd import lib

    assert "clc_gmm_decode_step" in lib.SIGNATURES
    Lb = lib.load()
    buf = (ctypes.c_float * 4096)()
    ibuf = (ctypes.c_int32 * 4096)()
    p, ip = ctypes.addressof(buf), ctypes.addressof(ibuf)
    names = ("gp", "ldg", "N", "K", "pix", "P", "B", "H", "W", "words", "spans", "state", "S", "yh", "ldh", "st")
    base = dict(gp=p, ldg=72, N=8, K=3, pix=ip, P=2, B=1, H=2, W=2, words=ip, spans=ip, state=ip, S=4, yh=p, ldh=8, st=None)
    call = lambda **k: Lb.clc_gmm_decode_step(*[{**base, **k}[n] for n in names])

    def refused(rc, what):
        assert rc == -1
        msg = Lb.clc_last_error().decode()
        assert "clc_gmm_decode_step" in msg and what in msg, msg

    for name in ("gp", "pix", "words", "spans", "state", "yh"):
        refused(call(**{name: None}), "null pointer")
    refused(call(K=0), "K must be between 1 and 4")
    refused(call(K=5), "K must be between 1 and 4")
    refused(call(S=0), "S must be between 1 and 64")
    refused(call(S=65, N=96, ldg=864, ldh=96), "S must be between 1 and 64")
    refused(call(S=9), "S > N")
    refused(call(ldg=71), "ldg < 3 K N")
    refused(call(ldh=7), "ldh < N")
    for name in ("P", "B", "H", "W", "N"):
        refused(call(**{name: 0}), "must be positive")
    refused(call(B=1 << 20, H=1 << 10, W=1 << 10), "below 2^31")


# ---------------------------------------------------------------------------------------------------------------- the default stays put
def _fake_codec_inputs(p, monkeypatch, B=2, HW=6):
    """the device half of compress replaced by fixed triples (valid ones, from random rows), so the host half runs without a GPU"""
    g = np.random.default_rng(4)
    N = p.N
    rows = _random_rows(B * HW * N, g)
    vals = g.integers(-3, L + 3, B * HW * N)
    t = torch.tensor([_triple(rows[i], int(vals[i])) for i in range(len(vals))], dtype=torch.int32).reshape(B, HW, N, 3)
    monkeypatch.setattr(p, "_code_inputs", lambda x: ("y", "params", [b"z0", b"z1"][:B], (1, 2)))
    monkeypatch.setattr(p, "_gmm_encode", lambda y, params: (t, None))
    return t.numpy()


def test_defaults_are_todays_code_path(monkeypatch):
    from clc_amd import ans, models

    p = models.Cheng2020Anchor(24, 3)
    t = _fake_codec_inputs(p, monkeypatch)
    for item in (p.compress(None), p.compress(None, "wavefront"), p.compress(None, substreams=None)):
        assert sorted(item) == ["kernel_config", "shape", "strings"]   # no "substreams"
        assert item["strings"][0] == [ans.encode_direct(t[0]), ans.encode_direct(t[1])] and item["strings"][1] == [b"z0", b"z1"]
    split = p.compress(None, substreams=4)
    assert sorted(split) == ["kernel_config", "shape", "strings", "substreams"] and split["substreams"] == 4
    assert split["kernel_config"] == item["kernel_config"] and split["strings"][1] == item["strings"][1]
    for b in range(2):
        subs = ans.split_unpack(split["strings"][0][b])
        assert subs == [ans.encode_direct(np.ascontiguousarray(t[b][:, s::4])) for s in range(4)]
        # the overhead against the one stream: 8 + 4 S of header and S - 1 more 8-byte final states; a final state holds 31 .. 63 bits
        # of the payload, so each of the S - 1 may also save up to one 32-bit word (and the coder's rounding may cost one overall)
        extra = len(split["strings"][0][b]) - len(item["strings"][0][b])
        assert 8 + 4 * 4 + (8 - 4) * 3 - 4 <= extra <= 8 + 4 * 4 + 8 * 3 + 4, extra

    # decompress: the default goes through _gmm_decode and nothing else
    calls = []
    monkeypatch.setattr(p.entropy_bottleneck, "decompress", lambda s, shape: "z_hat")
    monkeypatch.setattr(p, "_hyper_synthesis", lambda z: "params")
    monkeypatch.setattr(p, "_gmm_decode", lambda s, params: calls.append(("one", s, params)) or torch.zeros(1))
    monkeypatch.setattr(p, "_gmm_decode_split", lambda *a, **k: calls.append(("split",)) or (torch.zeros(1), None))
    monkeypatch.setattr(p, "_synthesis", lambda y: y + 2.0)
    for out in (p.decompress(item["strings"], (1, 2)), p.decompress(item["strings"], (1, 2), substreams=None)):
        assert sorted(out) == ["x_hat"] and float(out["x_hat"]) == 1.0
    assert calls == [("one", item["strings"][0], "params")] * 2
    p.decompress(split["strings"], (1, 2), substreams=4, device_decoder=False)
    assert calls[-1] == ("split",)
