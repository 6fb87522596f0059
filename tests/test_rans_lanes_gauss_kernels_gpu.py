"""The slice step's fused coder and the pack kernel of the lanes stream (csrc/rans_lanes.hip: clc_rans_lanes_decode_gauss,
clc_rans_lanes_pack) against the host coder and against the launches they replace.  Every comparison is exact.

decode_gauss: B = 2 images of 13 pixels x C = 5 channels (n = 65: one full chunk and one lane of the next), scale, mu and y_hat with a
leading dimension of 7, W in {1, 3}, three consecutive segments with the state carried on the device.  Scales exactly on the entries of
the table, one ulp either side of them, below the 0.11 bound (and zero, negative) and huge (and infinite); fractional means; symbols
inside their rows, at max_value - 1, at max_value, below the offset and +-10^6 (several payload nibbles, one of them in the partial
chunk).  The indexes are ops.quantize_build_indexes', the words the host encoder's.  Every buffer lies between 256 sentinel words and
is compared whole, padding columns included.

pack: B = 2, W = 3 regions with sentinel words between them from a real rans_lanes_encode.
"""
import numpy as np
import pytest
import torch

from test_rans_lanes_kernels_gpu import GAP, PAD, SENT, _batch, _final, _lay_out, _regions

pytestmark = pytest.mark.gpu

B, C, PIX, LD, SEGS = 2, 5, 13, 7, 3
N = PIX * C
FSENT = -777.25


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gauss():
    """a GaussianConditional over 8 scales from 0.11 to 64 -> (host tables, scale table float32)"""
    from clc_amd.entropy_models import GaussianConditional

    gc = GaussianConditional([float(s) for s in np.geomspace(0.11, 64.0, 8)])
    gc.update()
    return gc.host_tables(), gc.scale_table.detach().float().cpu().numpy().copy()


def _padded(vals, dev):
    """float [B, PIX, C] -> (the whole flat buffer: PAD sentinels | [B, PIX, LD] with sentinel padding columns | PAD sentinels,
    its logical [B, C, PIX, 1] pixel-major view with leading dimension LD)"""
    flat = torch.full((2 * PAD + B * PIX * LD,), FSENT, dtype=torch.float32)
    body = flat[PAD:PAD + B * PIX * LD].view(B, PIX, 1, LD)
    if vals is not None:
        body[..., :C] = torch.from_numpy(vals).view(B, PIX, 1, C)
    flat = flat.to(dev)
    return flat, flat[PAD:PAD + B * PIX * LD].view(B, PIX, 1, LD).permute(0, 3, 1, 2)[:, :C]


@pytest.fixture(scope="module")
def case(dev, gauss):
    """three segments: (scale, mu) float32 [B, PIX, C], the indexes of quantize_build_indexes and the planted symbols, int32 [B, N]"""
    from clc_amd import ops

    (cdf, ln, off), table = gauss
    g = np.random.default_rng(5)
    up, down = np.nextafter(table, np.float32(np.inf)), np.nextafter(table, np.float32(-np.inf))
    special = np.concatenate([table, up, down, np.float32([0.05, 0.0, -3.0, 0.10999999, 1e30, np.inf, 65.0, 3.4e38])]).astype(np.float32)
    tdev = torch.from_numpy(table).to(dev)
    segs = []
    for p in range(SEGS):
        scale = np.exp(g.uniform(np.log(0.05), np.log(100.0), B * N)).astype(np.float32)
        where = g.permutation(B * N)[:3 * special.size]
        scale[where] = np.tile(special, 3)
        scale = scale.reshape(B, PIX, C)
        mu = (g.uniform(-4.0, 4.0, (B, PIX, C)) + 0.37).astype(np.float32)
        _, sc_v = _padded(scale, dev)
        _, mu_v = _padded(mu, dev)
        _, idx, _ = ops.quantize_build_indexes(torch.zeros_like(mu_v), mu_v, sc_v, tdev)
        idx = idx.permute(0, 2, 3, 1).reshape(B, N).cpu().numpy()   # NHWC: the segment's order
        # the restated index: n_scales - 1 - #{k < n_scales - 1: max(scale, 0.11) <= table[k]}
        sg = np.maximum(scale.reshape(B, N), np.float32(0.11))
        assert np.array_equal(idx, 7 - (sg[..., None] <= table[None, None, :7]).sum(-1))
        assert set(idx.reshape(-1).tolist()) == set(range(8))
        maxv = ln[idx] - 2
        val = np.clip(np.rint(g.normal(0.0, 1.0, (B, N)) * table[idx]).astype(np.int64) - off[idx], 0, maxv - 1)   # inside the rows
        i = np.arange(N)[None, :] + np.arange(B)[:, None]
        val = np.where(i % 7 == 1, maxv - 1, val)
        val = np.where(i % 11 == 2, maxv, val)
        val = np.where(i % 13 == 3, -1, val)
        sym = val + off[idx]
        sym = np.where(i % 17 == 4, 10**6, sym)
        sym = np.where(i % 19 == 5, -10**6, sym)
        sym[:, N - 1] = (10**6, -10**6)[p % 2]   # an escape with several payload nibbles in the partial chunk
        segs.append((scale, mu, idx.astype(np.int32), sym.astype(np.int32)))
    return segs


def _host_streams(case, W, gauss):
    from clc_amd import ans

    cdf, ln, off = gauss[0]
    sym = np.concatenate([s[3] for s in case], axis=1)
    idx = np.concatenate([s[2] for s in case], axis=1)
    return [ans.lanes_encode(sym[b], idx[b], [N] * SEGS, W, cdf, ln, off) for b in range(B)]


def _run_segment(seg, tdev, tables, words, spans, state, dev, with_symbols=True):
    """one decode_gauss over sentinel-framed buffers -> (y_hat [B, N] in segment order, symbols or None); everything else is asserted whole"""
    from clc_amd import ops

    scale, mu, _, _ = seg
    sc_flat, sc_v = _padded(scale, dev)
    mu_flat, mu_v = _padded(mu, dev)
    yh_flat, yh_v = _padded(None, dev)
    sb = torch.full((B, N + 16), -SENT, device=dev, dtype=torch.int32) if with_symbols else None
    keep = (sc_flat.clone(), mu_flat.clone(), words.clone(), spans.clone())
    out = ops.rans_lanes_decode_gauss(sc_v, mu_v, tdev, tables, words, spans, state, y_hat=yh_v, symbols=sb)
    assert out.data_ptr() == yh_v.data_ptr()
    assert torch.equal(sc_flat, keep[0]) and torch.equal(mu_flat, keep[1]) and torch.equal(words, keep[2]) and torch.equal(spans, keep[3])
    got = yh_flat.cpu()
    body = got[PAD:PAD + B * PIX * LD].view(B, PIX, LD)
    assert (got[:PAD] == FSENT).all() and (got[PAD + B * PIX * LD:] == FSENT).all() and (body[..., C:] == FSENT).all()
    if with_symbols:
        assert torch.equal(sb[:, N:], torch.full((B, 16), -SENT, device=dev, dtype=torch.int32))
        sb = sb[:, :N].cpu().numpy()
    return body[..., :C].reshape(B, N).clone(), sb


@pytest.mark.parametrize("W", [1, 3])
def test_fused_slice_coder_is_the_host_coder_and_the_composition(dev, gauss, case, W):
    from clc_amd import ans, lib, ops

    (cdf, ln, off), table = gauss
    tdev = torch.from_numpy(table).to(dev)
    tables = tuple(torch.from_numpy(t).to(dev) for t in (cdf, ln, off))
    host = _host_streams(case, W, gauss)
    words, spans, state = _lay_out(host, dev)
    words2, spans2, state2 = _lay_out(host, dev)   # the three launches the kernel replaces, on a state of their own
    decoders = [ans.LanesDecoder(img) for img in host]
    for p, seg in enumerate(case):
        scale, mu, idx, sym = seg
        y_hat, got_sym = _run_segment(seg, tdev, tables, words, spans, state, dev, with_symbols=(p != 1))
        want = torch.from_numpy(sym).float() + torch.from_numpy(mu).reshape(B, N)
        assert torch.equal(y_hat.view(torch.int32), want.view(torch.int32)), p   # bit for bit
        if got_sym is not None:
            assert np.array_equal(got_sym, sym)
        # the states after this segment are the host decoder's
        x, pos = _final(state)
        for b in range(B):
            assert np.array_equal(decoders[b].decode(idx[b], cdf, ln, off), sym[b])
            for w in range(W):
                hx, hpos = decoders[b].state(w)
                assert np.array_equal(hx, x[b, w]) and hpos == int(pos[b, w]), (p, b, w)
        # quantize_build_indexes + rans_lanes_decode_step + add on the same inputs
        _, sc_v = _padded(scale, dev)
        _, mu_v = _padded(mu, dev)
        _, ib, _ = ops.quantize_build_indexes(torch.zeros_like(mu_v), mu_v, sc_v, tdev)
        ib = ib.permute(0, 2, 3, 1).reshape(B, N).contiguous()
        sb = torch.zeros((B, N), device=dev, dtype=torch.int32)
        ops.rans_lanes_decode_step(ib, N, tables, words2, spans2, state2, sb)
        comp = sb.view(B, PIX, 1, C).permute(0, 3, 1, 2).float() + mu_v
        assert torch.equal(comp.permute(0, 2, 3, 1).reshape(B, N).cpu().view(torch.int32), y_hat.view(torch.int32))
        assert torch.equal(state, state2)
    x, pos = _final(state)
    assert (x == np.uint64(1 << 31)).all() and pos.tolist() == [[len(s) // 4 for s in img] for img in host]
    assert int(state[..., 129].abs().max()) == 0
    assert lib.load().clc_kernel_config_tag() == 6   # (the codec's tag does not notice the new entries)


@pytest.mark.parametrize("noise", [False, True])
def test_cut_span_and_random_words_decode_like_the_host(dev, gauss, case, noise):
    """a span cut short / other words than an encoder's: the host decoder's symbols and states on the kernel's own indexes"""
    from clc_amd import ans

    W = 3
    (cdf, ln, off), table = gauss
    tdev = torch.from_numpy(table).to(dev)
    tables = tuple(torch.from_numpy(t).to(dev) for t in (cdf, ln, off))
    host = _host_streams(case, W, gauss)
    if noise:
        g = np.random.default_rng(11)
        streams = [[g.integers(0, 256, len(s), dtype=np.uint8).tobytes() for s in img] for img in host]
        words, spans, state = _lay_out(streams, dev)
    else:
        assert len(host[0][0]) > 4 * 140
        streams = [[host[0][0][:4 * 130], host[0][1], host[0][2]], host[1]]
        words, spans, state = _lay_out(host, dev, cut={0: 130})   # image 0, wave stream 0
    decoders = [ans.LanesDecoder(img) for img in streams]
    differs = False
    for seg in case:
        _, mu, idx, sym = seg
        y_hat, got = _run_segment(seg, tdev, tables, words, spans, state, dev)
        for b in range(B):
            assert np.array_equal(decoders[b].decode(idx[b], cdf, ln, off), got[b])
        assert torch.equal(y_hat.view(torch.int32), (torch.from_numpy(got).float() + torch.from_numpy(mu).reshape(B, N)).view(torch.int32))
        differs |= not np.array_equal(got, sym)
        if not noise:
            assert np.array_equal(got[1], sym[1])   # the other image is untouched
    assert differs
    x, pos = _final(state)
    for b in range(B):
        for w in range(W):
            hx, hpos = decoders[b].state(w)
            assert np.array_equal(hx, x[b, w]) and hpos == int(pos[b, w])
    if not noise:
        assert int(pos[0, 0]) > 130


def test_decode_gauss_wrapper_refusals(dev, gauss, case):
    from clc_amd import ops

    (cdf, ln, off), table = gauss
    tdev = torch.from_numpy(table).to(dev)
    tables = tuple(torch.from_numpy(t).to(dev) for t in (cdf, ln, off))
    words, spans, state = _lay_out(_host_streams(case, 3, gauss), dev)
    _, sc = _padded(case[0][0], dev)
    _, mu = _padded(case[0][1], dev)
    call = lambda **k: ops.rans_lanes_decode_gauss(**{**dict(scale=sc, mu=mu, scale_table=tdev, tables=tables, words=words, spans=spans, state=state), **k})
    with pytest.raises(ValueError, match="scale must be a float32"):
        call(scale=sc.double())
    with pytest.raises(ValueError, match="scale and mu must have one shape"):
        call(mu=mu[:, :4])
    with pytest.raises(ValueError, match="scale_table must be a contiguous float32 device tensor of 2 .. 256 entries"):
        call(scale_table=torch.zeros(257, device=dev))
    with pytest.raises(ValueError, match=r"state must be int32 \[B, W, 130\]"):
        call(state=state[..., :128].contiguous())
    with pytest.raises(ValueError, match=r"spans must be int32 \[B = 2, W, 2\]"):
        call(spans=spans[:1].contiguous(), state=state[:1].contiguous())
    with pytest.raises(ValueError, match="y_hat must be stored pixel-major"):
        call(y_hat=torch.zeros((B, C, PIX, 1), device=dev))
    with pytest.raises(ValueError, match="at least n = 65 elements"):
        call(symbols=torch.zeros((B, 64), device=dev, dtype=torch.int32))
    with pytest.raises(ValueError, match="cdfs must be a contiguous int32 device tensor"):
        call(tables=(tables[0].cpu(), tables[1], tables[2]))


# ------------------------------------------------------------------------------------------------------------------------------- pack
def _encoded(dev, shrink=None):
    from clc_amd import ops

    from test_rans_lanes_cpu import lanes_table

    W, which = 3, 2
    tables = tuple(torch.from_numpy(t).to(dev) for t in lanes_table())
    sym, idx, seg, host = _batch(W, which)
    reg, size = _regions(seg, W, 2, shrink=shrink)
    buf = torch.full((size,), SENT, device=dev, dtype=torch.int32)
    _, _, result = ops.rans_lanes_encode(torch.from_numpy(sym).to(dev), torch.from_numpy(idx).to(dev), seg, W, tables, out=buf, regions=reg)
    return buf, result, host


def _pack(buf, result, capacity, dev):
    """-> (the packed words [capacity], header) with everything around them asserted to be sentinels still"""
    from clc_amd import ops

    n = int(result.shape[0] * result.shape[1])
    frame = torch.full((2 * PAD + capacity,), SENT, device=dev, dtype=torch.int32)
    hframe = torch.full((2 * PAD + n + 1,), SENT, device=dev, dtype=torch.int32)
    before = buf.clone()
    packed, header = ops.rans_lanes_pack(buf, result, capacity, packed=frame[PAD:PAD + capacity], header=hframe[PAD:PAD + n + 1])
    assert torch.equal(buf, before)
    for f, m in ((frame, capacity), (hframe, n + 1)):
        f = f.cpu().numpy()
        assert (f[:PAD] == SENT).all() and (f[PAD + m:] == SENT).all()
    return packed.cpu().numpy().view(np.uint32), header.cpu().numpy()


def test_pack_is_the_concatenation_of_the_spans(dev):
    buf, result, host = _encoded(dev)
    flat = b"".join(s for img in host for s in img)
    counts = [len(s) // 4 for img in host for s in img]
    total = sum(counts)
    packed, header = _pack(buf, result, total + GAP, dev)
    assert header.tolist() == counts + [total]
    assert packed[:total].tobytes() == flat and (packed[total:] == SENT).all()
    # a capacity one word short: the total is reported, the copy stops at the capacity
    packed, header = _pack(buf, result, total - 1, dev)
    assert header.tolist() == counts + [total] and packed.tobytes() == flat[:-4]
    # the default buffers
    from clc_amd import ops

    p2, h2 = ops.rans_lanes_pack(buf, result)
    assert h2.cpu().numpy().tolist() == counts + [total] and p2.cpu().numpy().view(np.uint32)[:total].tobytes() == flat


def test_pack_passes_codes_through_and_copies_nothing_for_them(dev):
    from clc_amd import lib

    probe, _, host = _encoded(dev)
    short = len(host[1][0]) // 4 - 1   # image 1, wave stream 0: one word less than its stream needs
    buf, result, host = _encoded(dev, shrink={(1, 0): short})
    res = result.cpu().numpy()
    assert res[1, 0].tolist() == [lib.RANS_LANES_OVERFLOW, 0]
    result = result.clone()
    result[0, 2] = torch.tensor([lib.RANS_LANES_ZERO_FREQ, 5], device=dev, dtype=torch.int32)   # a code with a count behind it: still no words
    streams = [host[0][0], host[0][1], b"", b"", host[1][1], host[1][2]]
    counts = [len(s) // 4 for s in streams]
    total = sum(counts)
    packed, header = _pack(buf, result, total + GAP, dev)
    want = list(counts) + [total]
    want[2], want[3] = lib.RANS_LANES_ZERO_FREQ, lib.RANS_LANES_OVERFLOW
    assert header.tolist() == want
    assert packed[:total].tobytes() == b"".join(streams) and (packed[total:] == SENT).all()


def test_pack_wrapper_refusals(dev):
    from clc_amd import ops

    buf, result, _ = _encoded(dev)
    with pytest.raises(ValueError, match="out must be a contiguous int32 device tensor"):
        ops.rans_lanes_pack(buf.cpu(), result)
    with pytest.raises(ValueError, match=r"result int32 \[B, W, 2\]"):
        ops.rans_lanes_pack(buf, result.view(-1, 2))
    with pytest.raises(ValueError, match="W must be between 1 and 16"):
        ops.rans_lanes_pack(buf, torch.zeros((1, 17, 2), device=dev, dtype=torch.int32))
    with pytest.raises(ValueError, match="capacity must lie inside packed"):
        ops.rans_lanes_pack(buf, result, 100, packed=torch.zeros(99, device=dev, dtype=torch.int32))
    with pytest.raises(ValueError, match="header hold B W \\+ 1 = 7"):
        ops.rans_lanes_pack(buf, result, header=torch.zeros(6, device=dev, dtype=torch.int32))
