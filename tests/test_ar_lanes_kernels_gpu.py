"""The two kernels of the context models' lanes stream (csrc/rans_lanes.hip: clc_ar_lanes_decode, clc_rans_lanes_encode_list) against the
host coder and against the launches they replace, at B = 2.  Every comparison is exact.

clc_ar_lanes_decode.  A SEQUENCE is a list of steps over one 4 x 5 latent, each step a pixel list of P pairs x M channels, n = P M
symbols per image, decoded by one call per step with the state carried on the device.
    M = 24, P = 1, 2, 3, 4, 1   n = 24 .. 96: a partial chunk or one chunk and a partial one; at W = 3 wave 1 has no round in the first
                                two steps and wave 2 none at all (its state must come back as it went in)
    M = 72, P = 5, 2, 3, 4      n = 360, 144, 216, 288: rows straddle chunks; 6, 3, 4 and 5 rounds per step at W = 1, one or two at W = 3
so a wave's rounds per step pass through 0, 1, 2, 3, 4, 5 and 6: the group look-ahead (four rounds) is short, exact and overfull.
gp has ldg = 2 M + 5 and y_hat ldh = M + 3; every sequence lists one pair outside the map (decoded, nothing written).  Scales exactly
on the entries of the table, one ulp either side, below the 0.11 bound (zero, negative) and above the last entry (huge, infinite);
fractional means; symbols inside their rows, at max_value - 1, and escaping with 0 to 8 payload nibbles.  Compared with (a)
ar_finish_decode + rans_lanes_decode_step + ar_commit on the same inputs and a state of their own: y_hat whole, symbols, state; (b)
ans.LanesDecoder on indexes restated in numpy float32: symbols and the states after every step.  Every buffer lies between 256
sentinel words, has sentinel padding columns and is compared whole.

clc_rans_lanes_encode_list.  P in {0, 1, 32, 33, 40} segments with empty ones among them, W in {1, 3}: the bytes of ans.lanes_encode, of
clc_rans_lanes_encode where it takes the list, nothing outside the streams; overflow and zero frequency as codes.
"""
import numpy as np
import pytest
import torch

from test_rans_lanes_cpu import lanes_table
from test_rans_lanes_kernels_gpu import GAP, PAD, SENT, _final, _lay_out, _regions

pytestmark = pytest.mark.gpu

B, H, WM = 2, 4, 5
FSENT = -777.25
OUTSIDE = {(H, 0), (-1, 2), (1, WM), (2, -1)}
# (M, per step the pixel list): every in-map pixel at most once per sequence
SEQUENCES = {
    24: [[(0, 0)], [(0, 1), (1, 4)], [(3, 3), (H, 0), (2, 2)], [(1, 0), (1, 1), (0, 4), (3, 4)], [(2, 0)]],
    72: [[(0, 3), (1, 0), (-1, 2), (2, 1), (3, 4)], [(0, 0), (3, 0)], [(2, 2), (1, WM), (0, 4)], [(1, 1), (1, 2), (2, -1), (3, 3)]],
}
RAWS = (0, 1, 0x10, 0x400, 0x1000, 0x12345, 0x1E8480, 0x1000000, 0x80000000)   # 0 .. 8 payload nibbles


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gauss():
    """the table of tests/test_rans_lanes_cpu.py -> (host tables, its 8 scales as float32)"""
    cdf, ln, off = lanes_table()
    return (cdf, ln, off), np.geomspace(0.11, 64.0, 8).astype(np.float32)


@pytest.fixture(scope="module")
def cases(gauss):
    """per M the steps: (pixel list, gp float32 [B, P, 2 M], indexes restated in numpy float32 and planted symbols, int32 [B, P M])"""
    (cdf, ln, off), table = gauss
    up, down = np.nextafter(table, np.float32(np.inf)), np.nextafter(table, np.float32(-np.inf))
    special = np.concatenate([table, up, down, np.float32([0.05, 0.0, -3.0, 0.10999999, 1e30, np.inf, 65.0, 3.4e38])]).astype(np.float32)
    out = {}
    for M, steps in SEQUENCES.items():
        g = np.random.default_rng(M)
        seq = []
        for k, px in enumerate(steps):
            P = len(px)
            n = P * M
            scale = np.exp(g.uniform(np.log(0.05), np.log(100.0), B * n)).astype(np.float32)
            take = min(special.size, B * n // 2)
            scale[g.permutation(B * n)[:take]] = np.roll(special, 7 * k)[:take]
            scale = scale.reshape(B, P, M)
            mean = (g.uniform(-4.0, 4.0, (B, P, M)) + 0.37).astype(np.float32)
            sg = np.maximum(scale.reshape(B, n), np.float32(0.11))
            idx = (7 - (sg[..., None] <= table[None, None, :7]).sum(-1)).astype(np.int32)
            maxv = ln[idx] - 2
            val = np.clip(np.rint(g.normal(0.0, 1.0, (B, n)) * table[idx]).astype(np.int64) - off[idx], 0, maxv - 1)   # inside the rows
            i = np.arange(n)[None, :] + np.arange(B)[:, None]
            val = np.where(i % 7 == 1, maxv - 1, val)
            sym = val + off[idx]
            for r, raw in enumerate(RAWS):   # escapes of every payload length, spread over the step (and its last symbol)
                j = (5 + 11 * r + 3 * k) % n if r else n - 1
                b = (r + k) % B
                sym[b, j] = off[idx[b, j]] + (-(raw >> 1) - 1 if raw & 1 else (raw >> 1) + maxv[b, j])
            seq.append((px, np.concatenate((scale, mean), axis=2), idx, sym.astype(np.int32)))
        out[M] = seq
    _check_inputs(gauss, out)
    return out


def _host_streams(seq, W, gauss):
    from clc_amd import ans

    cdf, ln, off = gauss[0]
    sym, idx = np.concatenate([s[3] for s in seq], axis=1), np.concatenate([s[2] for s in seq], axis=1)
    return [ans.lanes_encode(sym[b], idx[b], [s[3].shape[1] for s in seq], W, cdf, ln, off) for b in range(B)]


def _latent(M, dev):
    """-> (the whole flat buffer PAD | [B, H, WM, ldh = M + 3] | PAD of sentinels, its [B, M, H, WM] pixel-major view)"""
    ldh = M + 3
    flat = torch.full((2 * PAD + B * H * WM * ldh,), FSENT, device=dev, dtype=torch.float32)
    return flat, flat[PAD:PAD + B * H * WM * ldh].view(B, H, WM, ldh).permute(0, 3, 1, 2)[:, :M]


def _rows(gp, dev):
    """gp float32 [B, P, 2 M] -> (the flat buffer PAD | [B P, ldg = 2 M + 5] with sentinel padding columns | PAD, its [B P, 2 M] view)"""
    rows, C = gp.shape[0] * gp.shape[1], gp.shape[2]
    flat = torch.full((2 * PAD + rows * (C + 5),), FSENT, dtype=torch.float32)
    flat[PAD:PAD + rows * (C + 5)].view(rows, C + 5)[:, :C] = torch.from_numpy(gp).view(rows, C)
    flat = flat.to(dev)
    return flat, flat[PAD:PAD + rows * (C + 5)].view(rows, C + 5)[:, :C]


def _expected_latent(M, seq, upto, syms):
    """what the latent's flat buffer holds after steps 0 .. upto: sentinels but for (float)symbol + mean at the listed in-map pixels"""
    ldh = M + 3
    want = np.full((B, H, WM, ldh), FSENT, dtype=np.float32)
    for k in range(upto + 1):
        px, gp = seq[k][0], seq[k][1]
        for p, (h, w) in enumerate(px):
            if 0 <= h < H and 0 <= w < WM:
                want[:, h, w, :M] = syms[k].reshape(B, len(px), M)[:, p].astype(np.float32) + gp[:, p, M:]
    return np.concatenate((np.full(PAD, FSENT, np.float32), want.reshape(-1), np.full(PAD, FSENT, np.float32)))


def _fused_step(step, M, tdev, tables, words, spans, state, latent, dev, with_symbols=True):
    """one ar_lanes_decode over sentinel-framed buffers -> the decoded symbols [B, n] (or None); its inputs are asserted unchanged"""
    from clc_amd import ops

    px, gp = step[0], step[1]
    n = len(px) * M
    pix = torch.tensor(px, dtype=torch.int32, device=dev).reshape(-1, 2)
    gp_flat, gp_v = _rows(gp, dev)
    sb = torch.full((B, n + 16), -SENT, device=dev, dtype=torch.int32) if with_symbols else None
    keep = (gp_flat.clone(), words.clone(), spans.clone(), pix.clone())
    out = ops.ar_lanes_decode(gp_v, M, pix, B, H, WM, tdev, tables, words, spans, state, latent, symbols=sb)
    assert out is latent
    assert torch.equal(gp_flat, keep[0]) and torch.equal(words, keep[1]) and torch.equal(spans, keep[2]) and torch.equal(pix, keep[3])
    if not with_symbols:
        return None
    assert torch.equal(sb[:, n:], torch.full((B, 16), -SENT, device=dev, dtype=torch.int32))
    return sb[:, :n].cpu().numpy()


def _three_launches(step, M, tdev, tables, words, spans, state, latent, dev):
    """ar_finish_decode + rans_lanes_decode_step + ar_commit on the same inputs -> the decoded symbols [B, n]"""
    from clc_amd import ops

    px, gp = step[0], step[1]
    P = len(px)
    pix = torch.tensor(px, dtype=torch.int32, device=dev).reshape(-1, 2)
    _, gp_v = _rows(gp, dev)
    ib = torch.zeros((B * P, M), device=dev, dtype=torch.int32)
    sb = torch.zeros((B * P, M), device=dev, dtype=torch.int32)
    ops.ar_finish_decode(gp_v, M, pix, B, H, WM, tdev, ib)
    ops.rans_lanes_decode_step(ib, P * M, tables, words, spans, state, sb)
    ops.ar_commit(sb, gp_v, M, pix, latent)
    return sb.view(B, P * M).cpu().numpy(), ib.view(B, P * M).cpu().numpy()


@pytest.mark.parametrize("W", [1, 3])
@pytest.mark.parametrize("M", [24, 72])
def test_fused_step_is_the_three_launches_and_the_host_coder(dev, gauss, cases, M, W):
    from clc_amd import ans, lib

    (cdf, ln, off), table = gauss
    seq = cases[M]
    tdev = torch.from_numpy(table).to(dev)
    tables = tuple(torch.from_numpy(t).to(dev) for t in (cdf, ln, off))
    host = _host_streams(seq, W, gauss)
    words, spans, state = _lay_out(host, dev)
    words2, spans2, state2 = _lay_out(host, dev)   # the three launches the kernel replaces, on a state and a latent of their own
    flat, latent = _latent(M, dev)
    flat2, latent2 = _latent(M, dev)
    decoders = [ans.LanesDecoder(img) for img in host]
    rounds = set()
    for k, step in enumerate(seq):
        px, gp, idx, sym = step
        n = len(px) * M
        rounds |= {len(range(w, (n + 63) // 64, W)) for w in range(W)}
        fresh = state.clone()
        got = _fused_step(step, M, tdev, tables, words, spans, state, latent, dev, with_symbols=(k != 1))
        if got is not None:
            assert np.array_equal(got, sym), k
        assert np.array_equal(flat.cpu().numpy().view(np.uint32), _expected_latent(M, seq, k, [s[3] for s in seq]).view(np.uint32)), k   # bit for bit, whole
        for w in range((n + 63) // 64, W):   # a wave with no round in the step: its state is as it was
            assert torch.equal(state[:, w], fresh[:, w])
        # the host decoder on the restated indexes: the symbols and the states after this step
        x, pos = _final(state)
        for b in range(B):
            assert np.array_equal(decoders[b].decode(idx[b], cdf, ln, off), sym[b])
            for w in range(W):
                hx, hpos = decoders[b].state(w)
                assert np.array_equal(hx, x[b, w]) and hpos == int(pos[b, w]), (k, b, w)
        # the composition
        sym3, idx3 = _three_launches(step, M, tdev, tables, words2, spans2, state2, latent2, dev)
        assert np.array_equal(idx3, idx) and np.array_equal(sym3, sym)   # (clc_ar_finish's index is the restated one)
        assert torch.equal(flat.view(torch.int32), flat2.view(torch.int32)) and torch.equal(state, state2), k
    assert rounds == ({3, 4, 5, 6} if (M, W) == (72, 1) else {1, 2} if W == 1 else {0, 1} if M == 24 else {1, 2})
    x, pos = _final(state)
    assert (x == np.uint64(1 << 31)).all() and pos.tolist() == [[len(s) // 4 for s in img] for img in host]
    assert int(state[..., 129].abs().max()) == 0
    assert lib.load().clc_kernel_config_tag() == 6   # (the codec's tag does not notice the new entries)


def _check_inputs(gauss, cases):
    """the inputs are what the docstring says: asserted once, where they are made"""
    (cdf, ln, off), table = gauss
    for M, seq in cases.items():
        sc = np.concatenate([s[1][..., :M].reshape(-1) for s in seq])
        idx = np.concatenate([s[2].reshape(-1) for s in seq])
        assert (sc < 0.11).any() and (sc > table[-1]).any() and all((sc == t).any() for t in table) and set(idx.tolist()) == set(range(8))
        nibbles = set()
        for _, _, ix, sy in seq:
            v = sy.astype(np.int64) - off[ix]
            maxv = ln[ix] - 2
            raw = np.where(v < 0, -2 * v - 1, 2 * (v - maxv))[(v < 0) | (v >= maxv)]
            nibbles |= {(int(r).bit_length() + 3) // 4 for r in raw}
        assert nibbles == set(range(9)), nibbles
        assert sum((h, w) in OUTSIDE for s in seq for h, w in s[0]) >= 1


def test_cut_span_decodes_like_the_host_and_leaves_the_others(dev, gauss, cases):
    """image 0's wave stream 0 cut to 130 words: the host decoder's symbols and states on the same words; image 1 untouched"""
    from clc_amd import ans

    M, W = 72, 3
    (cdf, ln, off), table = gauss
    seq = cases[M]
    tdev = torch.from_numpy(table).to(dev)
    tables = tuple(torch.from_numpy(t).to(dev) for t in (cdf, ln, off))
    host = _host_streams(seq, W, gauss)
    assert len(host[0][0]) > 4 * 140
    words, spans, state = _lay_out(host, dev, cut={0: 130})
    decoders = [ans.LanesDecoder([host[0][0][:4 * 130], host[0][1], host[0][2]]), ans.LanesDecoder(host[1])]
    flat, latent = _latent(M, dev)
    differs, syms = False, []
    for k, step in enumerate(seq):
        _, _, idx, sym = step
        got = _fused_step(step, M, tdev, tables, words, spans, state, latent, dev)
        for b in range(B):
            assert np.array_equal(decoders[b].decode(idx[b], cdf, ln, off), got[b]), (k, b)
        assert np.array_equal(got[1], sym[1])
        differs |= not np.array_equal(got[0], sym[0])
        syms.append(got)
        assert np.array_equal(flat.cpu().numpy().view(np.uint32), _expected_latent(M, seq, k, syms).view(np.uint32)), k
    assert differs
    x, pos = _final(state)
    for b in range(B):
        for w in range(W):
            hx, hpos = decoders[b].state(w)
            assert np.array_equal(hx, x[b, w]) and hpos == int(pos[b, w])
    assert int(pos[0, 0]) > 130 and (x[1] == np.uint64(1 << 31)).all()


def test_ar_lanes_decode_wrapper_refusals(dev, gauss, cases):
    from clc_amd import ops

    M = 24
    (cdf, ln, off), table = gauss
    tdev = torch.from_numpy(table).to(dev)
    tables = tuple(torch.from_numpy(t).to(dev) for t in (cdf, ln, off))
    words, spans, state = _lay_out(_host_streams(cases[M], 3, gauss), dev)
    px, gp = cases[M][1][0], cases[M][1][1]
    pix = torch.tensor(px, dtype=torch.int32, device=dev).reshape(-1, 2)
    _, gp_v = _rows(gp, dev)
    _, latent = _latent(M, dev)
    base = dict(gp=gp_v, M=M, pix=pix, B=B, H=H, W=WM, scale_table=tdev, tables=tables, words=words, spans=spans, state=state, y_hat=latent)
    call = lambda **k: ops.ar_lanes_decode(**{**base, **k})
    with pytest.raises(ValueError, match="the pixel list must be a contiguous int32"):
        call(pix=pix.long())
    with pytest.raises(ValueError, match="ar_lanes_decode gp: needs a row-major"):
        call(gp=gp_v[:3])
    with pytest.raises(ValueError, match=r"gp needs 2 M = 48 columns and y_hat must be a \[B, M, H, W\]"):
        call(gp=gp_v[:, :40])
    with pytest.raises(ValueError, match=r"y_hat must be a \[B, M, H, W\] = \(2, 24, 4, 5\) map"):
        call(y_hat=latent[:, :20])
    with pytest.raises(ValueError, match="the map must be a channels_last"):
        call(y_hat=torch.zeros((B, M, H, WM), device=dev))
    with pytest.raises(ValueError, match="scale_table must be a contiguous float32 device tensor of 2 .. 256 entries"):
        call(scale_table=torch.zeros(257, device=dev))
    with pytest.raises(ValueError, match=r"state must be int32 \[B, W, 130\]"):
        call(state=state[..., :128].contiguous())
    with pytest.raises(ValueError, match=r"spans must be int32 \[B = 2, W, 2\]"):
        call(spans=spans[:1].contiguous(), state=state[:1].contiguous())
    with pytest.raises(ValueError, match="at least n = 48 elements"):
        call(symbols=torch.zeros((B, 47), device=dev, dtype=torch.int32))
    with pytest.raises(ValueError, match="cdfs must be a contiguous int32 device tensor"):
        call(tables=(tables[0].cpu(), tables[1], tables[2]))


# ------------------------------------------------------------------------------------------------------------------- the list encoder
def _segments(P):
    """P segment lengths with empty ones among them: partial chunks, whole chunks, one lane over"""
    return [(1, 63, 0, 64, 65, 130, 0, 24, 200, 7)[(p * 3 + P) % 10] for p in range(P)]


def _list_case(P, seed):
    """-> (symbols, indexes) int32 [T] of one image over _segments(P): inside the rows, at their edges and escaping"""
    cdf, ln, off = lanes_table()
    T = max(sum(_segments(P)), 64)   # (P = 0: buffers of 64 unused symbols — an empty tensor has no pointer to hand over)
    g = np.random.default_rng(1000 * P + seed)
    idx = g.integers(0, 8, T).astype(np.int32)
    maxv = ln[idx] - 2
    val = g.integers(0, 1 << 30, T) % maxv
    i = np.arange(T)
    val = np.where(i % 17 == 3, maxv - 1, val)
    val = np.where(i % 23 == 5, maxv, val)
    val = np.where(i % 29 == 7, -1, val)
    sym = val + off[idx]
    sym = np.where(i % 31 == 11, 10**6, sym)
    sym = np.where(i % 37 == 13, -10**6, sym)
    return sym.astype(np.int32), idx


@pytest.mark.parametrize("W", [1, 3])
@pytest.mark.parametrize("P", [0, 1, 32, 33, 40])
def test_list_encoder_is_the_host_encoder(dev, P, W):
    from clc_amd import ans, ops

    cdf, ln, off = lanes_table()
    tables = tuple(torch.from_numpy(t).to(dev) for t in (cdf, ln, off))
    seg = _segments(P)
    assert P < 3 or (0 in seg and any(n % 64 for n in seg))
    imgs = [_list_case(P, seed) for seed in (0, 1)]
    sym, idx = np.stack([i[0] for i in imgs]), np.stack([i[1] for i in imgs])
    T = sum(seg)
    host = [ans.lanes_encode(sym[b, :T], idx[b, :T], seg, W, cdf, ln, off) for b in range(B)]
    reg, size = _regions(seg, W, B)
    buf = torch.full((size,), SENT, device=dev, dtype=torch.int32)
    s, i = torch.from_numpy(sym).to(dev), torch.from_numpy(idx).to(dev)
    out, reg_back, result = ops.rans_lanes_encode_list(s, i, seg, W, tables, out=buf, regions=reg)
    assert out is buf and np.array_equal(reg_back, reg)
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
    # the default regions give the same streams
    out2, reg2, res2 = ops.rans_lanes_encode_list(s, i, seg, W, tables)
    assert np.array_equal(reg2, ops.rans_lanes_regions(seg, W, B))
    r2, o2 = res2.cpu().numpy(), out2.cpu().numpy().view(np.uint32)
    assert all(o2[r2[b, w, 0]:r2[b, w, 0] + r2[b, w, 1]].tobytes() == host[b][w] for b in range(B) for w in range(W))
    if P <= 32:   # the by-value encoder on the same list: the same words at the same places
        buf3 = torch.full((size,), SENT, device=dev, dtype=torch.int32)
        _, _, res3 = ops.rans_lanes_encode(s, i, seg, W, tables, out=buf3, regions=reg)
        assert torch.equal(res3, result) and torch.equal(buf3, buf)
    else:
        with pytest.raises(ValueError, match="rans_lanes_encode: at most 32 segments"):
            ops.rans_lanes_encode(s, i, seg, W, tables)


def test_list_encoder_overflow_and_zero_frequency(dev):
    from clc_amd import ans, lib, ops

    P, W = 33, 3
    cdf, ln, off = lanes_table()
    tables = tuple(torch.from_numpy(t).to(dev) for t in (cdf, ln, off))
    seg = _segments(P)
    imgs = [_list_case(P, seed) for seed in (0, 1)]
    sym, idx = np.stack([i[0] for i in imgs]), np.stack([i[1] for i in imgs])
    host = [ans.lanes_encode(sym[b], idx[b], seg, W, cdf, ln, off) for b in range(B)]
    short = len(host[1][0]) // 4 - 1   # image 1, wave stream 0: one word less than its stream needs
    reg, size = _regions(seg, W, B, shrink={(1, 0): short, (0, 2): 100})   # ... and a region that cannot even hold the states
    buf = torch.full((size,), SENT, device=dev, dtype=torch.int32)
    _, _, result = ops.rans_lanes_encode_list(torch.from_numpy(sym).to(dev), torch.from_numpy(idx).to(dev), seg, W, tables, out=buf, regions=reg)
    res, got = result.cpu().numpy(), buf.cpu().numpy().view(np.uint32)
    assert res[1, 0].tolist() == [lib.RANS_LANES_OVERFLOW, 0] and res[0, 2].tolist() == [lib.RANS_LANES_OVERFLOW, 0]
    want = np.full(size, SENT, dtype=np.uint32)
    for b in range(B):
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
    first = int(reg[1, 0, 0])
    assert got[first + 127:first + short].tobytes() == host[1][0][4 * 128:] and (got[first:first + 127] == SENT).all()

    # a zero-frequency symbol: the code, and the other image's stream is whole
    flat = torch.tensor([[0, 5, 5, 65536]], dtype=torch.int32, device=dev)
    t2 = (flat, torch.tensor([4], dtype=torch.int32, device=dev), torch.tensor([0], dtype=torch.int32, device=dev))
    s2 = torch.tensor([[0, 1, 0], [0, 0, 7]], dtype=torch.int32, device=dev)
    out, _, res2 = ops.rans_lanes_encode_list(s2, torch.zeros_like(s2), [1, 0, 2], 1, t2)
    r = res2.cpu().numpy()
    assert r[0, 0].tolist() == [lib.RANS_LANES_ZERO_FREQ, 0] and r[1, 0, 1] >= 128
    (want1,) = ans.lanes_encode([0, 0, 7], [0, 0, 0], [1, 0, 2], 1, flat.cpu().numpy(), [4], [0])
    assert out.cpu().numpy().view(np.uint32)[r[1, 0, 0]:r[1, 0, 0] + r[1, 0, 1]].tobytes() == want1


def test_list_encoder_wrapper_refusals(dev):
    from clc_amd import ops

    tables = tuple(torch.from_numpy(t).to(dev) for t in lanes_table())
    s = torch.zeros((2, 192), device=dev, dtype=torch.int32)
    with pytest.raises(ValueError, match="rans_lanes_encode_list: W must be between 1 and 16"):
        ops.rans_lanes_encode_list(s, s, [64] * 3, 17, tables)
    with pytest.raises(ValueError, match="one shape"):
        ops.rans_lanes_encode_list(s, s[:, :100].contiguous(), [64], 3, tables)
    with pytest.raises(ValueError, match="rans_lanes_encode_list: segments of non-negative length adding up to at most T = 192"):
        ops.rans_lanes_encode_list(s, s, [1] * 193, 3, tables)
    with pytest.raises(ValueError, match="segments of non-negative length"):
        ops.rans_lanes_encode_list(s, s, [64, -1], 3, tables)
    reg, size = _regions([64] * 3, 3, 2)
    with pytest.raises(ValueError, match="every region must lie inside out"):
        ops.rans_lanes_encode_list(s, s, [64] * 3, 3, tables, out=torch.zeros(size - PAD - 1, device=dev, dtype=torch.int32), regions=reg)
    with pytest.raises(ValueError, match=r"regions must be int32 \[B, W, 2\]"):
        ops.rans_lanes_encode_list(s, s, [64] * 3, 3, tables, out=torch.zeros(size, device=dev, dtype=torch.int32), regions=reg[:1])
    with pytest.raises(ValueError, match="at most 32 segments"):   # the by-value entry keeps its limit
        ops.rans_lanes_encode(s, s, [1] * 33, 3, tables)
