"""The row kernels of the autoregressive coder (csrc/ar_context.hip: clc_ar_linear, clc_ar_finish, clc_ar_commit) at the smallest shapes
at which each thing can go wrong: maps 1x1, 2x3, 5x7 (smaller and larger than the 5x5 window), C in {4, 12, 36}, N in {4, 24, 52} (tails
of the four-channel workgroup), B in {1, 3}, pixel lists of one pixel, one wavefront step, every pixel (all corners and edges) and a list
of 315 rows (more than grid.y = 32 blocks of 8 rows: the row-block loop is walked).

  exact    integer operands, |x| <= 3, |w| <= 2: every partial sum is below 2^24, so any order is exact in f32 and the three source kinds
           and the two-range form must equal float64 masked F.conv2d / cat + matmul element for element.
  bounded  normal operands, none / LeakyReLU: |got - ref64| <= (K + 2) 2^-24 S (S the same sum on absolute values; tests/conv5_ref.py).
  bits     a row's output is bit-identical alone (P = 1), inside a wavefront step, inside the full list, at B = 1 and as image 1 of 3,
           and run to run: the order rule the decoder's sync rests on.
  finish / commit  symbols, indexes, y_hat bit-equal to ops.quantize_build_indexes on the same rows; decode mode + commit give the same
           y_hat bits; raster placement.
"""
import itertools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CL = torch.channels_last
EPS = 2.0 ** -24
MAPS = [(1, 1), (2, 3), (5, 7)]
CS, NS, BS = (4, 12, 36), (4, 24, 52), (1, 3)
LIVE = [(0, kw) for kw in range(5)] + [(1, kw) for kw in range(5)] + [(2, 0), (2, 1)]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _lists(H, W):
    """name -> list of (h, w)"""
    from clc_amd.models import ar_schedule

    every = [(h, w) for h in range(H) for w in range(W)]
    wave = max(ar_schedule(H, W, "wavefront"), key=len)
    long = (every * (105 // len(every) + 1))[:105] if len(every) > 1 else every * 105   # x B = 3: 315 rows
    return {"one": [every[-1]], "step": wave, "every": every, "long": long}


def _pix(lst, dev):
    return torch.tensor(lst, dtype=torch.int32).reshape(-1, 2).to(dev)


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _dense_filter(w, N, C):
    """[N, 12 C] live-tap filter -> the masked [N, C, 5, 5] filter of F.conv2d"""
    full = torch.zeros(N, C, 5, 5, dtype=torch.float64)
    w3 = w.double().reshape(N, 12, C)
    for t, (kh, kw) in enumerate(LIVE):
        full[:, :, kh, kw] = w3[:, t]
    return full


def _rows_of(t_map, lst):
    """[B, C, H, W] -> [B * P, C], rows r = b * P + p"""
    hs, ws = torch.tensor([p[0] for p in lst]), torch.tensor([p[1] for p in lst])
    return t_map[:, :, hs, ws].permute(0, 2, 1).reshape(-1, t_map.shape[1])


def _act(v, act):
    return torch.where(v > 0, v, 0.01 * v) if act else v


def _run(srcs, lst, B, H, W, w, b, act, dev, ldo_pad=0):
    from clc_amd import ops

    rows, N = B * len(lst), w.shape[0]
    out = torch.full((rows, N + ldo_pad), float("nan"), device=dev)
    ops.ar_linear(srcs, _pix(lst, dev), B, H, W, w.to(dev), b.to(dev) if b is not None else None, out, act=act)
    return out[:, :N].cpu()


def _to_map(t, dev):
    return t.to(dev).contiguous(memory_format=CL)


def _dense_buf(t, dev, pad=4):
    """[rows, C] values inside a wider [rows, C + pad] buffer: ld != C"""
    buf = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), device=dev)
    buf[:, :t.shape[1]] = t.to(dev)
    return buf[:, :t.shape[1]]


@pytest.mark.parametrize("H,W", MAPS)
def test_exact_every_source_kind(dev, H, W):
    g = torch.Generator().manual_seed(H * 16 + W)
    lists = _lists(H, W)
    for C, N, B in itertools.product(CS, NS, BS):
        x, x2 = _ints(g, -3, 3, B, C, H, W), _ints(g, -3, 3, B, 8, H, W)
        wt, wp, w2 = _ints(g, -2, 2, N, 12 * C), _ints(g, -2, 2, N, C), _ints(g, -2, 2, N, 8 + C)
        bias = _ints(g, -3, 3, N)
        conv = F.conv2d(x.double(), _dense_filter(wt, N, C), bias.double(), padding=2)
        for name, lst in lists.items():
            if name == "long" and B != 3:
                continue
            tag = f"{H}x{W} C{C} N{N} B{B} {name}"
            got = _run([("taps", _to_map(x, dev))], lst, B, H, W, wt, bias, 0, dev, ldo_pad=3)
            assert torch.equal(got.double(), _rows_of(conv, lst)), f"taps {tag}"
            xr = _rows_of(x, lst)
            got = _run([("pixel", _to_map(x, dev))], lst, B, H, W, wp, bias, 0, dev)
            assert torch.equal(got.double(), xr.double() @ wp.double().T + bias.double()), f"pixel {tag}"
            got = _run([("dense", _dense_buf(xr, dev))], lst, B, H, W, wp, None, 0, dev)
            assert torch.equal(got.double(), xr.double() @ wp.double().T), f"dense {tag}"
            # cat((pixel of an 8-channel map, dense rows), 1) @ w2.T — the first layer of entropy_parameters without the copy
            ref = torch.cat((_rows_of(x2, lst), xr), 1).double() @ w2.double().T + bias.double()
            got = _run([("pixel", _to_map(x2, dev)), ("dense", _dense_buf(xr, dev))], lst, B, H, W, w2, bias, 1, dev)
            assert torch.equal(got, _act(ref.float(), 1)), f"two ranges {tag}"   # (0.01f * v is one f32 rounding of an exact v)


@pytest.mark.parametrize("H,W", MAPS)
def test_bounded_against_float64(dev, H, W):
    g = torch.Generator().manual_seed(100 + H * 16 + W)
    lists = _lists(H, W)
    worst = 0.0
    for C, N, B in itertools.product(CS, NS, BS):
        x, x2 = torch.randn(B, C, H, W, generator=g), torch.randn(B, 8, H, W, generator=g)
        wt, w2, bias = torch.randn(N, 12 * C, generator=g), torch.randn(N, 8 + C, generator=g), torch.randn(N, generator=g)
        full = _dense_filter(wt, N, C)
        conv = F.conv2d(x.double(), full, bias.double(), padding=2)
        conv_s = F.conv2d(x.double().abs(), full.abs(), bias.double().abs(), padding=2)
        for (name, lst), act in itertools.product(lists.items(), (0, 1)):
            if name == "long" and B != 3:
                continue
            got = _run([("taps", _to_map(x, dev))], lst, B, H, W, wt, bias, act, dev).double()
            err, bound = (got - _act(_rows_of(conv, lst), act)).abs(), (12 * C + 2) * EPS * _rows_of(conv_s, lst)
            worst = max(worst, (err / bound).max().item())
            assert (err <= bound).all(), f"taps {H}x{W} C{C} N{N} B{B} {name} act{act}: {(err / bound).max().item():.3f} of the bound"
            xr = _rows_of(x, lst)
            cat = torch.cat((_rows_of(x2, lst), xr), 1).double()
            got = _run([("pixel", _to_map(x2, dev)), ("dense", _dense_buf(xr, dev))], lst, B, H, W, w2, bias, act, dev).double()
            err = (got - _act(cat @ w2.double().T + bias.double(), act)).abs()
            bound = (8 + C + 2) * EPS * (cat.abs() @ w2.double().abs().T + bias.double().abs())
            worst = max(worst, (err / bound).max().item())
            assert (err <= bound).all(), f"two ranges {H}x{W} C{C} N{N} B{B} {name} act{act}: {(err / bound).max().item():.3f} of the bound"
    print(f"{H}x{W}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("H,W", MAPS)
def test_a_rows_bits_do_not_depend_on_its_company(dev, H, W):
    g = torch.Generator().manual_seed(200 + H * 16 + W)
    lists = _lists(H, W)
    every = lists["every"]
    for C, N in ((4, 24), (12, 52), (36, 4), (36, 52)):
        x3, p3 = torch.randn(3, C, H, W, generator=g), torch.randn(3, 8, H, W, generator=g)
        wt, w2, bias = torch.randn(N, 12 * C, generator=g), torch.randn(N, 8 + N, generator=g), torch.randn(N, generator=g)

        def chain(x, p, lst):
            """taps -> N, then (pixel, dense) -> N with LeakyReLU: both launches of one list"""
            from clc_amd import ops

            B, rows = x.shape[0], x.shape[0] * len(lst)
            px = _pix(lst, dev)
            ctx = torch.empty((rows, N), device=dev)
            out = torch.empty((rows, N), device=dev)
            ops.ar_linear([("taps", _to_map(x, dev))], px, B, H, W, wt.to(dev), bias.to(dev), ctx)
            ops.ar_linear([("pixel", _to_map(p, dev)), ("dense", ctx)], px, B, H, W, w2.to(dev), bias.to(dev), out, act=1)
            return torch.cat((ctx, out), 1).cpu().reshape(B, len(lst), 2 * N)

        full = chain(x3, p3, every)                          # [3, HW, 2N]
        assert torch.equal(full, chain(x3, p3, every)), "run to run"
        alone_b1 = chain(x3[1:2], p3[1:2], every)            # image 1 of 3 on its own, B = 1
        assert torch.equal(alone_b1[0], full[1]), "B = 1 against image 1 of 3"
        long = chain(x3, p3, lists["long"])                  # 315 rows: the row-block loop
        for j, px in enumerate(lists["long"]):
            assert torch.equal(long[:, j], full[:, every.index(px)]), f"long list entry {j}"
        step = chain(x3, p3, lists["step"])
        for j, px in enumerate(lists["step"]):
            assert torch.equal(step[:, j], full[:, every.index(px)]), f"wavefront step entry {j}"
        for i, px in enumerate(every):                       # P = 1: the decoder's step
            one = chain(x3[1:2], p3[1:2], [px])
            assert torch.equal(one[0, 0], full[1, i]), f"pixel {px} alone"


@pytest.mark.parametrize("H,W", MAPS)
def test_finish_and_commit(dev, H, W):
    from clc_amd import ops
    from clc_amd.models.clc import get_scale_table

    g = torch.Generator().manual_seed(300 + H * 16 + W)
    table = get_scale_table().to(dev)
    lists = _lists(H, W)
    for M, B in itertools.product((4, 12, 36), BS):
        y = (4.0 * torch.randn(B, M, H, W, generator=g))
        scales = torch.exp(torch.empty(B, M, H, W).uniform_(-3.0, 5.0, generator=g))
        scales[:, :, 0, 0] = table.cpu()[:M]               # exactly on table entries: the <= of build_indexes
        means = torch.randn(B, M, H, W, generator=g)
        yd, sd, md = _to_map(y, dev), _to_map(scales, dev), _to_map(means, dev)
        sym_ref, idx_ref, yhat_ref = ops.quantize_build_indexes(yd, md, sd, table)   # logical [B, M, H, W]
        sym_ref = sym_ref.permute(0, 2, 3, 1).reshape(B, H * W, M)
        idx_ref = idx_ref.permute(0, 2, 3, 1).reshape(B, H * W, M)
        for name in ("one", "step", "every"):
            lst = lists[name]
            P, rows = len(lst), B * len(lst)
            px = _pix(lst, dev)
            gp = torch.full((rows, 2 * M + 4), float("nan"), device=dev)
            gp[:, :M] = _rows_of(scales, lst).to(dev)
            gp[:, M:2 * M] = _rows_of(means, lst).to(dev)
            y_hat = torch.full_like(yd, 777.0)
            sym = torch.full((B, H * W, M), -99, dtype=torch.int32, device=dev)
            idx = torch.full((B, H * W, M), -99, dtype=torch.int32, device=dev)
            ops.ar_finish_encode(gp, M, px, yd, y_hat, table, sym, idx)
            touched = torch.zeros(H * W, dtype=torch.bool)
            touched[[h * W + w for h, w in lst]] = True
            tag = f"{H}x{W} M{M} B{B} {name}"
            assert torch.equal(sym[:, touched], sym_ref[:, touched]) and torch.equal(idx[:, touched], idx_ref[:, touched]), tag
            assert (sym[:, ~touched] == -99).all() and (idx[:, ~touched] == -99).all(), f"{tag}: wrote outside the list"
            yh = y_hat.permute(0, 2, 3, 1).reshape(B, H * W, M)
            assert torch.equal(yh[:, touched], yhat_ref.permute(0, 2, 3, 1).reshape(B, H * W, M)[:, touched]), tag
            assert (yh[:, ~touched] == 777.0).all(), f"{tag}: y_hat written outside the list"
            # decode mode + commit from the encoder's symbols: the same indexes and the same y_hat bits
            idx_d = torch.full((rows, M), -99, dtype=torch.int32, device=dev)
            ops.ar_finish_decode(gp, M, px, B, H, W, table, idx_d)
            rows_of_idx = _rows_of(idx_ref.reshape(B, H, W, M).permute(0, 3, 1, 2), lst)
            assert torch.equal(idx_d, rows_of_idx.to(dev)), f"{tag}: decode-mode indexes"
            sym_rows = _rows_of(sym_ref.reshape(B, H, W, M).permute(0, 3, 1, 2), lst).contiguous().to(dev)
            y_hat2 = torch.full_like(yd, 777.0)
            ops.ar_commit(sym_rows, gp, M, px, y_hat2)
            assert torch.equal(y_hat2, y_hat), f"{tag}: commit"
        # in place: y_hat may be the y map itself
        lst = lists["every"]
        gp = torch.cat((_rows_of(scales, lst), _rows_of(means, lst)), 1).to(dev).contiguous()
        inplace = yd.clone(memory_format=torch.preserve_format)
        sym = torch.empty((B, H * W, M), dtype=torch.int32, device=dev)
        idx = torch.empty((B, H * W, M), dtype=torch.int32, device=dev)
        ops.ar_finish_encode(gp, M, _pix(lst, dev), inplace, inplace, table, sym, idx)
        assert torch.equal(inplace, yhat_ref) and torch.equal(sym, sym_ref) and torch.equal(idx, idx_ref)


def test_named_refusals(dev):
    from clc_amd import lib, ops

    px = _pix([(0, 0)], dev)
    m = lambda c: torch.zeros(1, c, 2, 3, device=dev).contiguous(memory_format=CL)
    out = torch.zeros(1, 8, device=dev)
    w = lambda n, k: torch.zeros(n, k, device=dev)
    with pytest.raises(lib.ClcError, match=r"C % 4"):
        ops.ar_linear([("taps", m(6))], px, 1, 2, 3, w(8, 72), None, out)
    with pytest.raises(lib.ClcError, match=r"C % 4"):
        ops.ar_linear([("dense", torch.zeros(1, 6, device=dev))], px, 1, 2, 3, w(8, 6), None, out)
    with pytest.raises(lib.ClcError, match=r"ld % 4"):
        ops.ar_linear([("dense", torch.zeros(1, 6, device=dev)[:, :4])], px, 1, 2, 3, w(8, 4), None, out)
    with pytest.raises(lib.ClcError, match="act must be"):
        ops.ar_linear([("pixel", m(4))], px, 1, 2, 3, w(8, 4), None, out, act=2)
    with pytest.raises(ValueError, match="one or two"):
        ops.ar_linear([("pixel", m(4))] * 3, px, 1, 2, 3, w(8, 12), None, out)
    with pytest.raises(ValueError, match="unknown source kind"):
        ops.ar_linear([("window", m(4))], px, 1, 2, 3, w(8, 4), None, out)
    with pytest.raises(ValueError, match=r"\[N, K = 48\]"):
        ops.ar_linear([("taps", m(4))], px, 1, 2, 3, w(8, 100), None, out)
    with pytest.raises(ValueError, match="does not match"):
        ops.ar_linear([("taps", m(4))], px, 1, 5, 7, w(8, 48), None, out)
    with pytest.raises(ValueError, match="channels_last"):
        ops.ar_linear([("taps", torch.zeros(1, 4, 2, 3, device=dev))], px, 1, 2, 3, w(8, 48), None, out)
    with pytest.raises(ValueError, match="pixel list"):
        ops.ar_linear([("taps", m(4))], px.long(), 1, 2, 3, w(8, 48), None, out)
    with pytest.raises(ValueError, match="rows"):
        ops.ar_linear([("taps", m(4))], _pix([(0, 0), (0, 1)], dev), 1, 2, 3, w(8, 48), None, out)
    with pytest.raises(lib.ClcError, match="GPU only"):
        ops.ar_linear([("taps", m(4).cpu().contiguous(memory_format=CL))], px, 1, 2, 3, w(8, 48), None, out)
