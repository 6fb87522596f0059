"""clc_gmm_decode_step (csrc/gmm.hip), the split stream's device decoder, against the host coder.  Every comparison is exact.

Per case: B = 2 images of a 3x5 map, seeded hostile parameter rows (scales under the 0.11 bound, means +-1000, logits +-50, NaN and +-Inf
entries), symbols inside each element's window, at its first and last place, just below and just above it and +-10^6 away.  The triples
come from ops.gmm_finish_encode, sub-stream s of an image is ans.encode_direct(triples[:, s::S]), and the device decodes them in three
calls over pixel lists of 8, 1 and 6 pixels with the coder states carried in device memory between the calls.  Expected: y_hat is the
symbols, every state ends at (2^31, word count), and RansDecoder.decode_rows over the rows of ops.gmm_finish_decode returns the same
symbols from the same bytes.

The word buffer of every run keeps sentinel words before, between and after the sub-streams, inside the allocation: a second run with
other sentinels must give identical results (words outside a span are never used), and a span cut to 2 words ends the call with that
sub-stream's pos beyond its count — what decompress(check=True) sees — while every other sub-stream is untouched.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
CL = torch.channels_last
H_, W_, B_ = 3, 5, 2
CASES = [(3, 4, 24), (2, 4, 6), (1, 1, 24), (4, 24, 24)]   # K, S, N
LISTS = (8, 1, 6)
GAP = 5
_REF = {}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _gp_rows(rows, K, N, seed):
    """[rows, 3 K N]: part, k, c"""
    g = torch.Generator().manual_seed(seed)
    sc = torch.rand((rows, K, N), generator=g) * 3.0 - 0.5          # a fifth under the 0.11 bound, some negative
    mu = torch.randn((rows, K, N), generator=g) * 4.0
    lg = torch.randn((rows, K, N), generator=g) * 2.0
    pick = lambda p: torch.rand((rows, K, N), generator=g) < p
    sc[pick(0.2)] = 0.05
    far = pick(0.1)
    mu[far] = torch.where(torch.rand((int(far.sum()),), generator=g) < 0.5, 1000.0, -1000.0)
    steep = pick(0.1)
    lg[steep] = torch.where(torch.rand((int(steep.sum()),), generator=g) < 0.5, 50.0, -50.0)
    bad = torch.tensor([float("nan"), float("inf"), -float("inf")])
    for t in (sc, mu, lg):
        hit = pick(0.03)
        t[hit] = bad[torch.randint(0, 3, (int(hit.sum()),), generator=g)]
    return torch.cat((sc.reshape(rows, -1), mu.reshape(rows, -1), lg.reshape(rows, -1)), 1).contiguous()


def _reference(dev, K, S, N):
    """once per case: parameter rows, symbols, triples, the sub-streams' bytes and the host decoder's answer"""
    key = (K, S, N)
    if key in _REF:
        return _REF[key]
    from clc_amd import ans, lib, ops
    from clc_amd.models import ar_wavefront_order

    R, L, stride = lib.GMM_R, 2 * lib.GMM_R + 1, lib.GMM_ROW_STRIDE
    order = ar_wavefront_order(H_, W_)
    P = len(order)
    pix = torch.tensor(order, dtype=torch.int32).reshape(-1, 2).to(dev)
    gp = _gp_rows(B_ * P, K, N, 40 + 7 * K + S).to(dev)
    rows = torch.empty((B_ * P, N, stride), device=dev, dtype=torch.int32)
    offs = torch.empty((B_ * P, N), device=dev, dtype=torch.int32)
    ops.gmm_finish_decode(gp, N, K, pix, B_, H_, W_, rows, offs)
    rows, offs = rows.cpu().numpy().reshape(B_, P, N, stride), offs.cpu().numpy().reshape(B_, P, N)
    g = np.random.default_rng(3 + K)
    val = g.integers(0, L, (B_, P, N))                                  # inside the window
    e = np.arange(B_ * P * N).reshape(B_, P, N)
    for m, v in ((0, 0), (1, L - 1), (2, -1), (3, L), (4, -2), (5, L + 1), (6, 1_000_000), (7, -1_000_000), (8, -R - 5), (9, L + R)):
        val[e % 23 == m] = v                                            # first, last, just below, just above (the empty payload), far outside
    sym = (offs + val).astype(np.float32)                               # |offset| <= 2^20 + R: exact
    y = torch.zeros(B_, N, H_, W_)
    for p, (h, w) in enumerate(order):
        y[:, :, h, w] = torch.from_numpy(sym[:, p])
    yd = y.to(dev).contiguous(memory_format=CL)
    y_hat = torch.full_like(yd, -5.0)
    triples = torch.zeros((B_, P, N, 3), device=dev, dtype=torch.int32)
    ops.gmm_finish_encode(gp, N, K, pix, yd, y_hat, triples)
    assert torch.equal(y_hat.cpu(), y)
    t = triples.cpu().numpy()
    assert int((t[..., 2] >= 0).sum()) >= 8 and int((t[..., 2] < 0).sum()) > t[..., 2].size // 2
    streams = [[ans.encode_direct(t[b][:, s::S, :]) for s in range(S)] for b in range(B_)]
    host = np.zeros((B_, P, N), dtype=np.int32)                         # the same bytes through the host decoder
    for b in range(B_):
        for s in range(S):
            d = ans.RansDecoder()
            d.set_stream(streams[b][s])
            back = d.decode_rows(np.ascontiguousarray(rows[b][:, s::S]).reshape(-1, stride), np.ascontiguousarray(offs[b][:, s::S]).reshape(-1))
            host[b][:, s::S] = back.reshape(P, -1)
    assert np.array_equal(host, sym.astype(np.int32))
    _REF[key] = dict(order=order, gp=gp, y=y, streams=streams)
    return _REF[key]


def _buffers(streams, sentinel, dev, cut=None):
    """words with GAP sentinel words before, between and after the sub-streams; spans; fresh states.  cut = (b, s): that span's count
    becomes 2 (its words stay where they are, so the reads that a wrong decoder would make still land inside the allocation)."""
    S = len(streams[0])
    words, spans, state = [], np.zeros((B_, S, 2), np.int32), np.zeros((B_, S, 4), np.uint32)
    at = 0
    for b in range(B_):
        for s in range(S):
            w = np.frombuffer(streams[b][s], dtype="<u4")
            words += [np.full(GAP, sentinel, np.uint32), w]
            at += GAP
            spans[b, s] = (at, 2 if cut == (b, s) else w.size)
            state[b, s] = (w[0], w[1], 2, 0)
            at += w.size
    words.append(np.full(GAP + 40, sentinel, np.uint32))
    to = lambda a: torch.from_numpy(a.view(np.int32).copy()).to(dev)
    return to(np.concatenate(words)), to(spans), to(state)


def _decode(dev, ref, K, S, N, words, spans, state, lists=LISTS, stray=None):
    """the device decoder over consecutive pixel lists of the order; stray = (list index, place, (h, w)): a pixel outside the map put
    into that list, with a parameter row of its own"""
    from clc_amd import ops

    order, P = ref["order"], len(ref["order"])
    gp = ref["gp"].reshape(B_, P, -1)
    y_hat = torch.full((B_, N, H_, W_), -5.0, device=dev).contiguous(memory_format=CL)
    lo = 0
    for i, n in enumerate(lists):
        px, g = list(order[lo:lo + n]), gp[:, lo:lo + n]
        if stray is not None and stray[0] == i:
            px.insert(stray[1], stray[2])
            g = torch.cat((g[:, :stray[1]], torch.full_like(g[:, :1], float("nan")), g[:, stray[1]:]), 1)
        ops.gmm_decode_step(g.reshape(-1, g.shape[-1]).contiguous(), N, K, torch.tensor(px, dtype=torch.int32).reshape(-1, 2).to(dev),
                            words, spans, state, y_hat)
        lo += n
    assert lo == P
    return y_hat.cpu(), state.cpu().numpy().view(np.uint32)


def _final(streams):
    return np.array([[(0x80000000, 0, len(s) // 4, 0) for s in img] for img in streams], dtype=np.uint32)


@pytest.mark.parametrize("K,S,N", CASES)
def test_device_decoder_against_the_host_coder(dev, K, S, N):
    ref = _reference(dev, K, S, N)
    y_hat, state = _decode(dev, ref, K, S, N, *_buffers(ref["streams"], 0xDEADBEEF, dev))
    assert torch.equal(y_hat, ref["y"])
    assert np.array_equal(state, _final(ref["streams"]))   # x == 2^31, pos == the word count, the pad untouched
    # other words around the spans: nothing changes
    y2, state2 = _decode(dev, ref, K, S, N, *_buffers(ref["streams"], 0x12345678, dev))
    assert torch.equal(y2, y_hat) and np.array_equal(state2, state)
    # one call over the whole order: the state carried across calls is the state of one call
    y3, state3 = _decode(dev, ref, K, S, N, *_buffers(ref["streams"], 0, dev), lists=(H_ * W_,))
    assert torch.equal(y3, y_hat) and np.array_equal(state3, state)


@pytest.mark.parametrize("K,S,N", [(3, 4, 24), (4, 24, 24)])
def test_truncated_span(dev, K, S, N):
    ref = _reference(dev, K, S, N)
    b, s = 1, S - 1
    assert len(ref["streams"][b][s]) // 4 > 3
    y_hat, state = _decode(dev, ref, K, S, N, *_buffers(ref["streams"], 0xDEADBEEF, dev, cut=(b, s)))
    mine = torch.zeros((B_, N, 1, 1), dtype=torch.bool)
    mine[b, s::S] = True
    mine = mine.expand(B_, N, H_, W_)
    assert torch.equal(y_hat[~mine], ref["y"][~mine])                  # every other sub-stream's symbols
    assert not torch.equal(y_hat[mine], ref["y"][mine])                # zeros were fed behind word 2, not the stream's words
    want = _final(ref["streams"])
    keep = np.ones((B_, S), bool)
    keep[b, s] = False
    assert np.array_equal(state[keep], want[keep])
    assert int(state[b, s, 2]) > 2                                     # pos beyond the count: what check= detects
    assert bool(torch.isfinite(y_hat).all())


@pytest.mark.parametrize("stray", [(0, 3, (-1, 2)), (1, 0, (H_, 0)), (2, 6, (1, W_)), (0, 0, (0, -1))])
def test_pixel_outside_the_map_is_skipped(dev, stray):
    K, S, N = 3, 4, 24
    ref = _reference(dev, K, S, N)
    y_hat, state = _decode(dev, ref, K, S, N, *_buffers(ref["streams"], 0xDEADBEEF, dev), stray=stray)
    assert torch.equal(y_hat, ref["y"])
    assert np.array_equal(state, _final(ref["streams"]))


def test_wrapper_refusals(dev):
    from clc_amd import lib, ops

    K, S, N = 3, 4, 24
    ref = _reference(dev, K, S, N)
    words, spans, state = _buffers(ref["streams"], 0, dev)
    pix = torch.tensor(ref["order"][:2], dtype=torch.int32).reshape(-1, 2).to(dev)
    gp = ref["gp"][:2 * B_]
    y_hat = torch.zeros((B_, N, H_, W_), device=dev).contiguous(memory_format=CL)
    with pytest.raises(ValueError, match="state must be"):
        ops.gmm_decode_step(gp, N, K, pix, words, spans, state[:, :3], y_hat)
    with pytest.raises(ValueError, match="spans must be"):
        ops.gmm_decode_step(gp, N, K, pix, words, spans.float(), state, y_hat)
    with pytest.raises(ValueError, match="words must be int32"):
        ops.gmm_decode_step(gp, N, K, pix, words.reshape(1, -1), spans, state, y_hat)
    with pytest.raises(ValueError, match="needs 3 K N"):
        ops.gmm_decode_step(gp[:, :-4], N, K, pix, words, spans, state, y_hat)
    with pytest.raises(ValueError, match="N = 24 channels"):
        ops.gmm_decode_step(gp, N, K, pix, words, spans, state, y_hat[:, :20])
    wide = torch.zeros((B_, 30, 2), device=dev, dtype=torch.int32)
    with pytest.raises(lib.ClcError, match="S > N"):
        ops.gmm_decode_step(gp, N, K, pix, words, wide, torch.zeros((B_, 30, 4), device=dev, dtype=torch.int32), y_hat)
