"""The device coder of the lanes stream (csrc/rans_lanes.hip: clc_rans_lanes_encode, clc_rans_lanes_decode_step) against the host coder
(rans_host.cpp), on the inputs of tests/test_rans_lanes_cpu.py at B = 2: W in {1, 3, 4}, the segment lists (1), (63, 64, 65),
(64 W, 64 W + 1, 0, 200), symbols inside, at the edges of and far outside their rows.  Every comparison is exact.

The device encoder's wave streams are byte-equal to the host encoder's; the device decoder, one call per segment with the state carried
on the device, returns the symbols and ends at (2^31 in all 64 lanes, the word count).  Every buffer a kernel writes or reads through a
span is allocated with 256 spare words on both sides and sentinel words between its parts, and is compared whole afterwards: nothing
outside a stream's own words changes.  A span cut to 130 words ends with pos beyond the count and leaves the other wave streams alone;
a region one word too small returns the overflow code and writes nothing outside itself.
"""
import numpy as np
import pytest
import torch

from test_rans_lanes_cpu import CASES, LANES, lanes_case, lanes_table

pytestmark = pytest.mark.gpu

L31 = 1 << 31
SENT = 0x5A5A5A5A
PAD, GAP = 256, 8


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def tables(dev):
    return tuple(torch.from_numpy(t).to(dev) for t in lanes_table())


def _batch(W, which):
    """B = 2 images of one segment list -> (symbols [2, T], indexes [2, T], segments, per image the host encoder's wave streams)"""
    from clc_amd import ans

    cdf, ln, off = lanes_table()
    imgs = [lanes_case(W, which, seed) for seed in (0, 1)]
    seg = imgs[0][2]
    assert imgs[1][2] == seg and not np.array_equal(imgs[0][0], imgs[1][0])
    sym, idx = np.stack([i[0] for i in imgs]), np.stack([i[1] for i in imgs])
    return sym, idx, seg, [ans.lanes_encode(sym[b], idx[b], seg, W, cdf, ln, off) for b in range(2)]


def _regions(seg, W, B, shrink=None):
    """regions of 128 + 10 n_w words behind PAD spare words and GAP sentinel words apart -> (int32 [B, W, 2], the buffer's size)"""
    from clc_amd import ans

    caps = [128 + 10 * n for n in ans.lanes_wave_symbols(seg, W)]
    reg, at = np.zeros((B, W, 2), dtype=np.int32), PAD
    for b in range(B):
        for w in range(W):
            cap = caps[w] if shrink is None or (b, w) not in shrink else shrink[(b, w)]
            reg[b, w] = (at, cap)
            at += cap + GAP
    return reg, at - GAP + PAD


def _lay_out(streams, dev, cut=None):
    """every wave stream's words behind PAD spare words and GAP sentinel words apart -> (words, spans [B, W, 2], state [B, W, 130])"""
    B, W = len(streams), len(streams[0])
    flat = [np.frombuffer(s, "<u4") for img in streams for s in img]
    total = PAD + sum(w.size + GAP for w in flat) - GAP + PAD
    words = np.full(total, SENT, dtype=np.uint32)
    spans, state, at = np.zeros((B * W, 2), np.int32), np.zeros((B * W, 130), np.uint32), PAD
    for i, w in enumerate(flat):
        words[at:at + w.size] = w
        spans[i] = (at, w.size if cut is None or i not in cut else cut[i])
        state[i, :128], state[i, 128] = w[:128], 128
        at += w.size + GAP
    to = lambda a: torch.from_numpy(a.view(np.int32)).to(dev)
    return to(words), to(spans).view(B, W, 2), to(state).view(B, W, 130)


def _decode(idx, seg, tables, words, spans, state, dev):
    """one decode_step per segment, the state carried on the device -> symbols [B, T]; the spare words behind every image's block stay"""
    from clc_amd import ops

    B, out, at = idx.shape[0], [], 0
    for n in seg:
        ib = torch.from_numpy(np.ascontiguousarray(idx[:, at:at + n])).to(dev)
        sb = torch.full((B, n + 16), -SENT, device=dev, dtype=torch.int32)
        ops.rans_lanes_decode_step(ib, n, tables, words, spans, state, sb)
        assert torch.equal(sb[:, n:], torch.full((B, 16), -SENT, device=dev, dtype=torch.int32))
        out.append(sb[:, :n].cpu().numpy())
        at += n
    return np.concatenate(out, axis=1)


def _final(state):
    st = state.cpu().numpy().view(np.uint32)
    x = st[..., 0:128:2].astype(np.uint64) | (st[..., 1:128:2].astype(np.uint64) << np.uint64(32))
    return x, st[..., 128].astype(np.int64)


@pytest.mark.parametrize("W,which", CASES)
def test_device_coder_is_the_host_coder(dev, tables, W, which):
    from clc_amd import lib, ops

    sym, idx, seg, host = _batch(W, which)
    B = 2
    # the encoder
    reg, size = _regions(seg, W, B)
    buf = torch.full((size,), SENT, device=dev, dtype=torch.int32)
    _, _, result = ops.rans_lanes_encode(torch.from_numpy(sym).to(dev), torch.from_numpy(idx).to(dev), seg, W, tables, out=buf, regions=reg)
    res, got = result.cpu().numpy(), buf.cpu().numpy().view(np.uint32)
    want = np.full(size, SENT, dtype=np.uint32)
    for b in range(B):
        for w in range(W):
            first, count = int(res[b, w, 0]), int(res[b, w, 1])
            assert first >= 0, (b, w, first)
            assert count == len(host[b][w]) // 4 and first + count == int(reg[b, w, 0]) + int(reg[b, w, 1])   # written backward from the region's end
            assert got[first:first + count].tobytes() == host[b][w], (b, w)
            want[first:first + count] = got[first:first + count]
    assert np.array_equal(got, want)   # every other word of the buffer is still the sentinel
    # the default regions (back to back, no spare words) give the same streams
    out2, reg2, res2 = ops.rans_lanes_encode(torch.from_numpy(sym).to(dev), torch.from_numpy(idx).to(dev), seg, W, tables)
    assert np.array_equal(reg2, ops.rans_lanes_regions(seg, W, B)) and out2.numel() == int(reg2[-1, -1].sum())
    r2, o2 = res2.cpu().numpy(), out2.cpu().numpy().view(np.uint32)
    assert all(o2[r2[b, w, 0]:r2[b, w, 0] + r2[b, w, 1]].tobytes() == host[b][w] for b in range(B) for w in range(W))

    # the decoder: one call per segment, the state carried on the device
    words, spans, state = _lay_out(host, dev)
    before = words.clone()
    assert np.array_equal(_decode(idx, seg, tables, words, spans, state, dev), sym)
    x, pos = _final(state)
    assert (x == np.uint64(L31)).all() and pos.tolist() == [[len(s) // 4 for s in img] for img in host]
    assert torch.equal(words, before) and int(state[..., 129].abs().max()) == 0
    assert lib.load().clc_kernel_config_tag() == 6   # (the codec's tag does not notice the new entries)


def test_truncated_span(dev, tables):
    from clc_amd import ans

    W, which = 3, 2
    cdf, ln, off = lanes_table()
    sym, idx, seg, host = _batch(W, which)
    assert len(host[0][1]) > 4 * 140
    words, spans, state = _lay_out(host, dev, cut={1: 130})   # image 0, wave stream 1
    before = words.clone()
    got = _decode(idx, seg, tables, words, spans, state, dev)
    x, pos = _final(state)
    assert int(pos[0, 1]) > 130 and torch.equal(words, before)
    # the other wave streams: their symbols and final states are untouched; the cut one is the host decoder's on the same words
    d = ans.LanesDecoder([host[0][0], host[0][1][:4 * 130], host[0][2]])
    at = 0
    for n in seg:
        assert d.decode(idx[0, at:at + n], cdf, ln, off).tolist() == got[0, at:at + n].tolist()
        chunk_wave = (np.arange(n) // LANES) % W
        assert np.array_equal(got[0, at:at + n][chunk_wave != 1], sym[0, at:at + n][chunk_wave != 1])
        at += n
    assert not np.array_equal(got[0], sym[0]) and np.array_equal(got[1], sym[1])
    for w in range(W):
        hx, hpos = d.state(w)
        assert np.array_equal(hx, x[0, w]) and hpos == int(pos[0, w])
    for b, w in ((0, 0), (0, 2), (1, 0), (1, 1), (1, 2)):
        assert (x[b, w] == np.uint64(L31)).all() and int(pos[b, w]) == len(host[b][w]) // 4


def test_random_words_decode_like_the_host(dev, tables):
    """other words than an encoder's: wrong symbols, the host decoder's, and nothing outside the spans is read or written"""
    from clc_amd import ans

    W, which = 4, 1
    cdf, ln, off = lanes_table()
    sym, idx, seg, host = _batch(W, which)
    g = np.random.default_rng(11)
    noise = [[g.integers(0, 256, len(s), dtype=np.uint8).tobytes() for s in img] for img in host]
    words, spans, state = _lay_out(noise, dev)
    before = words.clone()
    got = _decode(idx, seg, tables, words, spans, state, dev)
    x, pos = _final(state)
    assert torch.equal(words, before)
    for b in range(2):
        d = ans.LanesDecoder(noise[b])
        want = np.concatenate([d.decode(idx[b, at:at + n], cdf, ln, off) for at, n in zip(np.cumsum((0,) + seg[:-1]), seg)])
        assert np.array_equal(got[b], want)
        for w in range(W):
            hx, hpos = d.state(w)
            assert np.array_equal(hx, x[b, w]) and hpos == int(pos[b, w])


def test_encoder_overflow_and_zero_frequency(dev, tables):
    from clc_amd import lib, ops

    W, which = 3, 1
    sym, idx, seg, host = _batch(W, which)
    short = len(host[1][0]) // 4 - 1   # image 1, wave stream 0: one word less than its stream needs
    reg, size = _regions(seg, W, 2, shrink={(1, 0): short, (0, 2): 100})   # ... and a region that cannot even hold the states
    buf = torch.full((size,), SENT, device=dev, dtype=torch.int32)
    _, _, result = ops.rans_lanes_encode(torch.from_numpy(sym).to(dev), torch.from_numpy(idx).to(dev), seg, W, tables, out=buf, regions=reg)
    res, got = result.cpu().numpy(), buf.cpu().numpy().view(np.uint32)
    assert res[1, 0].tolist() == [lib.RANS_LANES_OVERFLOW, 0] and res[0, 2].tolist() == [lib.RANS_LANES_OVERFLOW, 0]
    want = np.full(size, SENT, dtype=np.uint32)
    for b in range(2):
        for w in range(W):
            first, cap = int(reg[b, w, 0]), int(reg[b, w, 1])
            if (b, w) in ((1, 0), (0, 2)):
                want[first:first + cap] = got[first:first + cap]   # inside its own region an overflowing wave may have written
                continue
            assert res[b, w].tolist() == [first + cap - len(host[b][w]) // 4, len(host[b][w]) // 4]
            assert got[res[b, w, 0]:first + cap].tobytes() == host[b][w]
            want[res[b, w, 0]:first + cap] = got[res[b, w, 0]:first + cap]
    assert np.array_equal(got, want)   # nothing outside the regions, nothing below a stream inside its region
    assert (got[reg[0, 2, 0]:reg[0, 2, 0] + 100] == SENT).all()   # (the region too small for the states: not touched at all)
    # what the overflowing wave did write is its stream behind the states, at the region's end; the 128 state words no longer fit
    first = int(reg[1, 0, 0])
    assert got[first + 127:first + short].tobytes() == host[1][0][4 * 128:] and (got[first:first + 127] == SENT).all()

    # a zero-frequency symbol: the code, and the other image's stream is whole
    flat = torch.tensor([[0, 5, 5, 65536]], dtype=torch.int32, device=dev)
    t2 = (flat, torch.tensor([4], dtype=torch.int32, device=dev), torch.tensor([0], dtype=torch.int32, device=dev))
    s2 = torch.tensor([[0, 1, 0], [0, 0, 7]], dtype=torch.int32, device=dev)
    out, reg2, res2 = ops.rans_lanes_encode(s2, torch.zeros_like(s2), [3], 1, t2)
    r = res2.cpu().numpy()
    assert r[0, 0].tolist() == [lib.RANS_LANES_ZERO_FREQ, 0] and r[1, 0, 1] >= 128
    from clc_amd import ans

    (want1,) = ans.lanes_encode([0, 0, 7], [0, 0, 0], [3], 1, flat.cpu().numpy(), [4], [0])
    assert out.cpu().numpy().view(np.uint32)[r[1, 0, 0]:r[1, 0, 0] + r[1, 0, 1]].tobytes() == want1


def test_wrapper_refusals(dev, tables):
    from clc_amd import ops

    sym, idx, seg, host = _batch(3, 1)
    words, spans, state = _lay_out(host, dev)
    ib = torch.from_numpy(np.ascontiguousarray(idx[:, :63])).to(dev)
    sb = torch.zeros_like(ib)
    with pytest.raises(ValueError, match="indexes must be a contiguous int32 device tensor"):
        ops.rans_lanes_decode_step(ib.long(), 63, tables, words, spans, state, sb)
    with pytest.raises(ValueError, match="symbols must be a contiguous int32 device tensor"):
        ops.rans_lanes_decode_step(ib, 63, tables, words, spans, state, sb.cpu())
    with pytest.raises(ValueError, match=r"spans int32 \[B, W, 2\]"):
        ops.rans_lanes_decode_step(ib, 63, tables, words, spans.view(-1, 2), state, sb)
    with pytest.raises(ValueError, match=r"state must be int32 \[B, W, 130\]"):
        ops.rans_lanes_decode_step(ib, 63, tables, words, spans, state[..., :128].contiguous(), sb)
    with pytest.raises(ValueError, match="at least n = 64 elements"):
        ops.rans_lanes_decode_step(ib, 64, tables, words, spans, state, sb)
    with pytest.raises(ValueError, match="W must be between 1 and 16"):
        ops.rans_lanes_decode_step(ib, 63, tables, words, torch.zeros((2, 17, 2), device=dev, dtype=torch.int32),
                                   torch.zeros((2, 17, 130), device=dev, dtype=torch.int32), sb)
    with pytest.raises(ValueError, match="cdfs must be a contiguous int32 device tensor"):
        ops.rans_lanes_decode_step(ib, 63, (tables[0].cpu(), tables[1], tables[2]), words, spans, state, sb)
    with pytest.raises(ValueError, match="one cdf size and one offset per row"):
        ops.rans_lanes_decode_step(ib, 63, (tables[0], tables[1][:4].contiguous(), tables[2]), words, spans, state, sb)
    s, i = torch.from_numpy(sym).to(dev), torch.from_numpy(idx).to(dev)
    with pytest.raises(ValueError, match="W must be between 1 and 16"):
        ops.rans_lanes_encode(s, i, seg, 17, tables)
    with pytest.raises(ValueError, match="one shape"):
        ops.rans_lanes_encode(s, i[:, :100].contiguous(), seg, 3, tables)
    with pytest.raises(ValueError, match="at most 32 segments"):
        ops.rans_lanes_encode(s, i, [1] * 33, 3, tables)
    with pytest.raises(ValueError, match="adding up to at most T = 192"):
        ops.rans_lanes_encode(s, i, (63, 64, 66), 3, tables)
    reg, size = _regions(seg, 3, 2)
    with pytest.raises(ValueError, match="every region must lie inside out"):
        ops.rans_lanes_encode(s, i, seg, 3, tables, out=torch.zeros(size - PAD - 1, device=dev, dtype=torch.int32), regions=reg)
    neg = reg.copy()
    neg[0, 0, 0] = -4
    with pytest.raises(ValueError, match="every region must lie inside out"):
        ops.rans_lanes_encode(s, i, seg, 3, tables, out=torch.zeros(size, device=dev, dtype=torch.int32), regions=neg)
    with pytest.raises(ValueError, match=r"regions must be int32 \[B, W, 2\]"):
        ops.rans_lanes_encode(s, i, seg, 3, tables, out=torch.zeros(size, device=dev, dtype=torch.int32), regions=reg[:1])
