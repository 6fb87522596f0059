"""clc_row_gemm (csrc/row_gemm.hip; ops.row_gemm) at the smallest shapes at which it can go wrong: a 3 x 5 map, B in {1, 3}, lists of 1, 5,
127, 128, 129 and 300 rows (one row, less than a tile, one short of / exactly / one over the 128-row tile, three tiles), per-range C in
{4, 32, 36, 68} (a sub-chunk range, exactly one 32-channel chunk, chunk + 4, two chunks + 4), 1 to 4 ranges mixing pixel and dense
sources with ld > C, N in {1, 3, 64, 66} (scalar stores, one full 64-channel tile, a second tile of two channels), output pitches that
do and do not allow 16-byte stores, all three activations.  One list holds a pixel outside the map: its output row keeps the sentinel
and its neighbours are right.

Every shape is checked three ways:
  1. EXACT on small-integer operands (|x| <= 4, |w| <= 3, integer bias: every partial sum is far below 2^24, so any summation order is
     exact and one misplaced term shows);
  2. within (K + 2) 2^-24 S of float64 on normal operands, S = the sum of the absolute products of the element (K fused
     multiply-adds, the bias addition and the activation each round once, each by at most 2^-24 of a magnitude S bounds; the bias is
     kept small against S);
  3. the ORDER RULE (test_order_rule): one row's bits are identical alone (P = 1), inside lists of 5, 129 and 300 at several places
     (other tiles), at B = 1 and as image 1 of 3, and run to run.
Also: on operands where both kernels are exact the result equals ops.ar_linear's; refusals name the offending field.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

H, W = 3, 5
CL = torch.channels_last
SENTINEL = -777.0
# (kind, C, ld - C or extra map channels, channel offset of the slice inside its map)
RANGES = {
    "1": [("pixel", 4, 4, 4)],
    "2": [("pixel", 32, 8, 0), ("dense", 36, 4, 0)],
    "3": [("dense", 68, 0, 0), ("pixel", 4, 0, 0), ("pixel", 36, 12, 8)],
    "4": [("pixel", 36, 4, 0), ("dense", 32, 8, 0), ("pixel", 68, 4, 4), ("dense", 4, 0, 0)],
}
# (P, B, index of a list entry that lies outside the map or None)
LISTS = [(1, 1, None), (5, 1, 3), (127, 1, None), (128, 1, 127), (43, 3, None), (300, 1, 128), (100, 3, 99)]
NS = [(1, 0), (3, 1), (64, 0), (64, 2), (64, 4), (66, 0)]   # (N, ldo - N)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _pixels(P, bad, g):
    pix = torch.stack((torch.randint(0, H, (P,), generator=g), torch.randint(0, W, (P,), generator=g)), 1).to(torch.int32)
    if bad is not None:
        pix[bad] = torch.tensor([(H, 0), (0, -1), (-1, 2), (1, W)][bad % 4], dtype=torch.int32)
    return pix


def _operands(cfg, P, B, g, integer):
    """CPU operands: per range the map / buffer, the filter and the bias"""
    rows = B * P
    draw = (lambda shape, a: torch.randint(-a, a + 1, shape, generator=g).float()) if integer else (lambda shape, a: torch.randn(shape, generator=g))
    srcs = []
    for kind, Cc, extra, off in cfg:
        if kind == "pixel":
            srcs.append(draw((B, Cc + extra + off, H, W), 4).contiguous(memory_format=CL))
        else:
            srcs.append(draw((rows + 3, Cc + extra), 4))
    K = sum(c[1] for c in cfg)
    return srcs, K


def _gather(cfg, srcs, pix, B):
    """float64 [rows, K]: what the kernel's rows read"""
    P = pix.shape[0]
    cols = []
    for (kind, Cc, extra, off), t in zip(cfg, srcs):
        if kind == "pixel":
            hh, ww = pix[:, 0].long().clamp(0, H - 1), pix[:, 1].long().clamp(0, W - 1)
            cols.append(torch.cat([t[b, off:off + Cc][:, hh, ww].t() for b in range(B)], 0))
        else:
            cols.append(t[:B * P, :Cc])
    return torch.cat(cols, 1).double()


def _device_srcs(cfg, srcs, dev):
    out = []
    for (kind, Cc, extra, off), t in zip(cfg, srcs):
        d = t.to(dev)
        out.append((kind, d[:, off:off + Cc] if kind == "pixel" else d[:, :Cc]))
    return out


def _inside(pix):
    return (pix[:, 0] >= 0) & (pix[:, 0] < H) & (pix[:, 1] >= 0) & (pix[:, 1] < W)


def _act64(v, act):
    from clc_amd.ops import ACT_LRELU, ACT_RELU

    if act == ACT_RELU:
        return v.clamp_min(0)
    if act == ACT_LRELU:
        return torch.where(v > 0, v, 0.01 * v)
    return v


@pytest.mark.parametrize("P,B,bad", LISTS, ids=[f"rows{p * b}-B{b}" for p, b, _ in LISTS])
@pytest.mark.parametrize("name", list(RANGES))
def test_exact_and_float64(dev, name, P, B, bad):
    from clc_amd import ops
    from clc_amd.ops import ACT_LRELU, ACT_NONE, ACT_RELU

    cfg = RANGES[name]
    rows = B * P
    g = torch.Generator().manual_seed(1000 * len(cfg) + rows + B)
    pix = _pixels(P, bad, g)
    live = _inside(pix).repeat(B)
    assert (bad is None) == bool(live.all())
    pd = pix.to(dev)
    for integer in (True, False):
        srcs, K = _operands(cfg, P, B, g, integer)
        X = _gather(cfg, srcs, pix, B)
        dsrcs = _device_srcs(cfg, srcs, dev)
        for i, (N, pad) in enumerate(NS):
            if integer:
                w = torch.randint(-3, 4, (N, K), generator=g).float()
                bias = torch.randint(-5, 6, (N,), generator=g).float()
            else:
                w = torch.randn((N, K), generator=g)
                bias = 0.1 * torch.randn((N,), generator=g)
            wd, bd = w.to(dev), (bias.to(dev) if i != 2 else None)   # one case without a bias
            pre = X @ w.double().t() + (bias.double() if bd is not None else 0.0)
            S = X.abs() @ w.double().abs().t()
            for act in (ACT_NONE, ACT_LRELU, ACT_RELU):
                buf = torch.full((rows + 2, N + pad), SENTINEL, device=dev)
                ops.row_gemm(dsrcs, pd, B, H, W, wd, bd, buf[:, :N], act=act)
                got = buf.cpu()
                tag = (name, rows, B, N, pad, act, integer)
                assert torch.all(got[rows:] == SENTINEL) and torch.all(got[:, N:] == SENTINEL), tag   # nothing past the rows / the N columns
                assert torch.all(got[:rows, :N][~live] == SENTINEL), tag                                # an outside pixel's row is never stored
                if integer:
                    v = pre.float()   # exact: integers below 2^24
                    want = v if act == ACT_NONE else (v.clamp_min(0) if act == ACT_RELU else torch.where(v > 0, v, torch.tensor(0.01) * v))
                    assert torch.equal(got[:rows, :N][live], want[live]), tag
                else:
                    err = (got[:rows, :N].double() - _act64(pre, act)).abs()
                    bound = (K + 2) * 2.0 ** -24 * S
                    worst = (err / bound)[live].max().item()
                    print(f"{tag}: largest error / bound {worst:.3f}")
                    assert worst <= 1.0, (tag, worst)


def _target_case(cfg, P, B, place, image, vec, g, dev):
    """operands in which row (image, place) reads exactly `vec` (per range) and everything else is random"""
    srcs, K = _operands(cfg, P, B, g, False)
    pix = _pixels(P, None, g)
    h0, w0 = 1, 3
    pix[place] = torch.tensor([h0, w0], dtype=torch.int32)
    r = image * P + place
    for (kind, Cc, extra, off), t, v in zip(cfg, srcs, vec):
        if kind == "pixel":
            t[image, off:off + Cc, h0, w0] = v
        else:
            t[r, :Cc] = v
    return _device_srcs(cfg, srcs, dev), pix.to(dev), r


@pytest.mark.parametrize("name", list(RANGES))
def test_order_rule(dev, name):
    from clc_amd import ops
    from clc_amd.ops import ACT_RELU

    cfg = RANGES[name]
    g = torch.Generator().manual_seed(77 + len(cfg))
    K = sum(c[1] for c in cfg)
    vec = [torch.randn(c[1], generator=g) for c in cfg]
    N = 66
    wd, bd = torch.randn((N, K), generator=g).to(dev), torch.randn((N,), generator=g).to(dev)

    def run(P, B, place, image):
        dsrcs, pd, r = _target_case(cfg, P, B, place, image, vec, g, dev)
        out = torch.empty((B * P, N), device=dev)
        ops.row_gemm(dsrcs, pd, B, H, W, wd, bd, out, act=ACT_RELU)
        again = torch.empty_like(out)
        ops.row_gemm(dsrcs, pd, B, H, W, wd, bd, again, act=ACT_RELU)
        assert torch.equal(out, again), (P, B, "run to run")
        return out[r].clone()

    base = run(1, 1, 0, 0)   # the row alone
    assert float(base.abs().max()) > 0.0
    for P, B, place, image in [(5, 1, 2, 0), (129, 1, 0, 0), (129, 1, 128, 0), (300, 1, 37, 0), (300, 1, 299, 0),
                               (1, 3, 0, 1), (5, 3, 4, 1), (129, 3, 70, 1), (300, 3, 161, 1)]:
        assert torch.equal(run(P, B, place, image), base), (name, P, B, place, image)


@pytest.mark.parametrize("name", ["1", "2"])
def test_equals_ar_linear_where_both_are_exact(dev, name):
    from clc_amd import ops
    from clc_amd.ops import ACT_LRELU, ACT_NONE

    cfg = RANGES[name]
    P, B = 43, 3
    g = torch.Generator().manual_seed(5)
    pix = _pixels(P, 7, g)
    srcs, K = _operands(cfg, P, B, g, True)
    dsrcs, pd = _device_srcs(cfg, srcs, dev), pix.to(dev)
    for N in (3, 64):
        wd = torch.randint(-3, 4, (N, K), generator=g).float().to(dev)
        bd = torch.randint(-5, 6, (N,), generator=g).float().to(dev)
        for act in (ACT_NONE, ACT_LRELU):
            a = torch.full((B * P, N), SENTINEL, device=dev)
            b = torch.full((B * P, N), SENTINEL, device=dev)
            ops.row_gemm(dsrcs, pd, B, H, W, wd, bd, a, act=act)
            ops.ar_linear(dsrcs, pd, B, H, W, wd, bd, b, act=act)
            assert torch.equal(a, b), (name, N, act)
            assert int((a == SENTINEL).all(1).sum()) == B   # the outside pixel's row of every image


def test_refusals_name_the_field(dev):
    from clc_amd import lib, ops
    from clc_amd.ops import ACT_GELU

    pd = torch.tensor([(0, 0), (2, 4)], dtype=torch.int32, device=dev)
    m = torch.zeros((1, 16, H, W), device=dev).contiguous(memory_format=CL)
    w8, out = torch.zeros((4, 8), device=dev), torch.zeros((2, 4), device=dev)
    ok = lambda: ops.row_gemm([("pixel", m[:, :8])], pd, 1, H, W, w8, None, out)
    ok()
    with pytest.raises(ValueError, match="taps.*ar_linear"):
        ops.row_gemm([("taps", m[:, :8])], pd, 1, H, W, w8, None, out)
    with pytest.raises(ValueError, match="one to four K ranges"):
        ops.row_gemm([("pixel", m[:, :4])] * 5, pd, 1, H, W, torch.zeros((4, 20), device=dev), None, out)
    with pytest.raises(ValueError, match=r"filter must be a contiguous float32 \[N, K = 8\]"):
        ops.row_gemm([("pixel", m[:, :8])], pd, 1, H, W, torch.zeros((4, 12), device=dev), None, out)
    with pytest.raises(ValueError, match="does not match B, H, W"):
        ops.row_gemm([("pixel", m[:, :8])], pd, 2, H, W, w8, None, torch.zeros((4, 4), device=dev))
    with pytest.raises(lib.ClcError, match=r"clc_row_gemm: act must be .* \(got 3\)"):
        ops.row_gemm([("pixel", m[:, :8])], pd, 1, H, W, w8, None, out, act=ACT_GELU)
    with pytest.raises(lib.ClcError, match=r"clc_row_gemm: range 0 is not 16-byte aligned"):
        ops.row_gemm([("pixel", m[:, 2:10])], pd, 1, H, W, w8, None, out)
    with pytest.raises(lib.ClcError, match=r"clc_row_gemm: C % 4 != 0 \(range 1 has C = 6\)"):
        ops.row_gemm([("pixel", m[:, :4]), ("pixel", m[:, 4:10])], pd, 1, H, W, torch.zeros((4, 10), device=dev), None, out)
    with pytest.raises(lib.ClcError, match=r"clc_row_gemm: ld % 4 != 0 or ld < C \(range 0 has ld = 10, C = 8\)"):
        ops.row_gemm([("dense", torch.zeros((2, 10), device=dev)[:, :8])], pd, 1, H, W, w8, None, out)
    ok()
