"""The six patch-matching kernels (csrc/patch_match.hip) one by one against the float64 references of tests/patch_matching_ref.py,
at the shapes where each kernel takes another path: partly filled patch / position / k tiles of the MFMA Pearson kernel, a 1x1 map,
a window next to the LDS budget, non-square patches, ties / NaN / inf in the top-k search, extreme positions in the gather.

Bars.  Pearson map: 2e-5 absolute (correlations are bounded by 1; the project's bar for this map); a case that misses may take 4x
the error of the float32 oracle against float64 on the same input, both figures printed (as tests/test_clm_train_gpu.py does).
Prep: 1e-5 (about six float32 operations on magnitudes up to 255 / 73: rounding bound about 3e-6).  Gaussian mask: 1e-6.  Gather:
1e-5 weighted, exact for the unweighted copy.  Top-k: indices and values equal the ordering rule's.  Measured errors: DESIGN.md §24.
"""
import numpy as np
import pytest
import torch

import patch_matching_ref as ref

pytestmark = pytest.mark.gpu
PEARSON_BAR, PREP_BAR, MASK_BAR, GATHER_BAR = 2e-5, 1e-5, 1e-6, 1e-5

# (P, C, H, W, ph, pw)
PEARSON_CASES = [
    (70, 3, 10, 72, 8, 8),      # map 3x65: a second, partly filled patch tile; one full and one 1-column position segment
    (64, 3, 9, 71, 8, 8),       # exact tiles: 64 patches, map 2x64
    (5, 3, 9, 40, 5, 4),        # K = 60: the second k-tile is partial, half of one 8-group invalid; map narrower than 64
    (7, 1, 9, 30, 6, 12),       # C = 1, ph != pw
    (4, 3, 6, 30, 4, 12),
    (1, 3, 16, 16, 16, 16),     # 1x1 map
    (3, 3, 41, 70, 40, 64),     # window of 60 960 B against the 65 536 B budget, K = 7680
]
_IDS = ["-".join(map(str, c)) for c in PEARSON_CASES]
_inputs = {}


def _pearson_inputs(case, shift):
    """seeded randn patches and image, patch 0 cut from the image at the LAST map position; `shift` added to both operands.
    Computed once per (case, shift) with the float64 map, shared and left unchanged."""
    key = (case, shift)
    if key not in _inputs:
        P, C, H, W, ph, pw = case
        g = torch.Generator().manual_seed(1000 + PEARSON_CASES.index(case))
        y = torch.randn(1, C, H, W, generator=g)
        q = torch.randn(P, C, ph, pw, generator=g)
        q[0] = y[0, :, H - ph:, W - pw:]
        q, y = (q + shift).contiguous(), (y + shift).contiguous()
        _inputs[key] = (q, y, ref.pearson_map(q, y))
    return _inputs[key]


def _corr(q, y, ph, pw, dev, mask=None):
    from clc_amd import patch_matching as pm

    return pm.L2_or_pearson_corr(q.to(dev), y.to(dev), ph, pw, mask=None if mask is None else mask.to(dev))


# ------------------------------------------------------------------------------------------------------------------------ Pearson


@pytest.mark.parametrize("shift", [0.0, 3.0], ids=["zero-mean", "mean3"])
@pytest.mark.parametrize("case", PEARSON_CASES, ids=_IDS)
def test_pearson_against_float64(dev, case, shift):
    from oracle import patch_matching as opm

    P, C, H, W, ph, pw = case
    q, y, want = _pearson_inputs(case, shift)
    out = _corr(q, y, ph, pw, dev)
    assert out.shape == want.shape and out.dtype == torch.float32
    got = out.cpu()
    err = (got.double() - want).abs().max().item()
    print(f"\n  pearson {case} shift {shift}: HIP {err:.3e}")
    bar = PEARSON_BAR
    if not err <= bar:
        own = (opm.L2_or_pearson_corr(q, y, ph, pw).double() - want).abs().max().item()
        bar = max(bar, 4.0 * own)
        print(f"  pearson {case} shift {shift}: HIP {err:.3e}, float32 oracle {own:.3e} -> bar {bar:.3e}")
    assert err <= bar, (case, shift, err, bar)
    # the planted match: patch 0 IS the window at the last position
    npos = want.shape[2] * want.shape[3]
    row, row64 = got.reshape(P, npos)[0], want.reshape(P, npos)[0]
    if npos > 1:
        runner_up = row64[:-1].max().item()
        print(f"  planted match: float64 runner-up {runner_up:.3f}")
        assert runner_up < 0.4, runner_up
    assert abs(row[-1].item() - 1.0) <= bar, row[-1].item()
    assert int(torch.argmax(row)) == npos - 1


@pytest.mark.parametrize("case", PEARSON_CASES, ids=_IDS)
def test_pearson_mask_is_one_multiply(dev, case):
    """the fused mask is the same float32 multiply as corr * mask: bit for bit, with a mask no index slip could hide behind"""
    P, C, H, W, ph, pw = case
    q, y, want = _pearson_inputs(case, 0.0)
    mask = torch.rand(want.shape, generator=torch.Generator().manual_seed(7)) + 0.5
    plain = _corr(q, y, ph, pw, dev)
    masked = _corr(q, y, ph, pw, dev, mask=mask)
    assert torch.equal(masked.cpu(), plain.cpu() * mask)
    assert torch.equal(masked, plain * mask.to(dev))


@pytest.mark.parametrize("case", PEARSON_CASES, ids=_IDS)
def test_pearson_repeatable(dev, case):
    P, C, H, W, ph, pw = case
    q, y, _ = _pearson_inputs(case, 3.0)
    assert torch.equal(_corr(q, y, ph, pw, dev), _corr(q, y, ph, pw, dev))


def test_pearson_row_independent_of_batch(dev):
    """the row of one patch computed alone is the row it has inside the 70-patch batch (first tile, second tile, planted patch)"""
    case = PEARSON_CASES[0]
    P, C, H, W, ph, pw = case
    q, y, _ = _pearson_inputs(case, 3.0)
    full = _corr(q, y, ph, pw, dev)
    for n in (0, 37, 63, 64, 69):
        alone = _corr(q[n:n + 1].contiguous(), y, ph, pw, dev)
        assert torch.equal(alone[0, 0], full[0, n]), n


def test_pearson_named_refusals(dev):
    """refused on the host, before any launch"""
    from clc_amd import lib
    from clc_amd import patch_matching as pm

    with pytest.raises(lib.ClcError, match="multiple of 4"):
        pm.L2_or_pearson_corr(torch.randn(2, 3, 4, 6, device=dev), torch.randn(1, 3, 8, 20, device=dev), 4, 6)
    with pytest.raises(lib.ClcError, match="exceeds the 64 KiB LDS budget"):
        pm.L2_or_pearson_corr(torch.randn(1, 3, 64, 64, device=dev), torch.randn(1, 3, 70, 130, device=dev), 64, 64)
    L = lib.load()
    P, C, H, W, ph, pw = 5, 3, 9, 40, 5, 4
    q, y = torch.randn(P, C, ph, pw, device=dev), torch.randn(1, C, H, W, device=dev)
    out = torch.empty(1, P, H - ph + 1, W - pw + 1, device=dev)
    nbytes = L.clc_pm_pearson_workspace_bytes(P, C, H, W, ph, pw)
    ws = torch.empty((nbytes + 3) // 4, device=dev, dtype=torch.float32)
    stream = torch.cuda.current_stream().cuda_stream
    with pytest.raises(lib.ClcError, match="workspace too small"):
        lib.check(L.clc_pm_pearson(q.data_ptr(), P, y.data_ptr(), C, H, W, ph, pw, None, out.data_ptr(), ws.data_ptr(), nbytes - 1, stream),
                  "clc_pm_pearson")
    lib.check(L.clc_pm_pearson(q.data_ptr(), P, y.data_ptr(), C, H, W, ph, pw, None, out.data_ptr(), ws.data_ptr(), nbytes, stream), "clc_pm_pearson")
    assert (out.cpu().double() - ref.pearson_map(q.cpu(), y.cpu())).abs().max().item() <= PEARSON_BAR


# ------------------------------------------------------------------------------------------------------------------ prep and mask


@pytest.mark.parametrize("in_scale", [255.0, 1.0])
@pytest.mark.parametrize("shape", [(2, 7, 9), (1, 16, 17)])
def test_prep_against_float64(dev, shape, in_scale):
    from clc_amd import patch_matching as pm

    N, H, W = shape
    x = torch.rand(N, 3, H, W, generator=torch.Generator().manual_seed(11)) * (255.0 / in_scale)
    got = pm.rgb_transform_normalized(x.to(dev), in_scale).cpu()
    err = (got.double() - ref.prep(x, in_scale)).abs().max().item()
    print(f"\n  prep {shape} in_scale {in_scale}: {err:.3e}")
    assert got.shape == x.shape and err <= PREP_BAR, err


@pytest.mark.parametrize("size", [(16, 24, 8, 8), (15, 21, 5, 7), (8, 8, 8, 8), (12, 8, 4, 8)])
def test_gaussian_mask_against_oracle(dev, size):
    from clc_amd import patch_matching as pm
    from oracle import patch_matching as opm

    want = opm.create_gaussian_masks(*size)
    got = pm.create_gaussian_masks(*size, device=dev).cpu()
    assert got.shape == want.shape
    err = (got.double() - want.double()).abs().max().item()
    print(f"\n  gaussian mask {size}: {err:.3e}")
    assert err <= MASK_BAR, err


# -------------------------------------------------------------------------------------------------------------------------- top-k


def _topk_rows(kind, P, npos, k, rng):
    """[P, npos] float32 rows of one kind"""
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    if kind == "tie-free":
        return np.stack([rng.permutation(npos) for _ in range(P)]).astype(np.float32) / np.float32(npos) - np.float32(0.5)
    if kind == "heavy-ties":
        return rng.choice(np.array([0.0, 0.5, 1.0], dtype=np.float32), size=(P, npos))
    if kind == "all-equal":
        return np.full((P, npos), 0.25, dtype=np.float32)
    if kind == "equal-maxima":          # twice the maximum, at i, i+1 (even rows) or at i, i+256: the same thread's next element (odd rows)
        a = rng.random((P, npos), dtype=np.float32) * np.float32(0.5)
        for p in range(P):
            gap = 256 if (p % 2 and npos > 256) else 1
            if npos > gap:
                i = int(rng.integers(0, npos - gap))
                a[p, i] = a[p, i + gap] = 2.0
        return a
    if kind == "all-neg-inf":
        return np.full((P, npos), -inf, dtype=np.float32)
    if kind == "scattered-nan-inf":
        a = rng.standard_normal((P, npos)).astype(np.float32)
        pick = rng.random((P, npos))
        a[pick < 0.10] = nan
        a[(pick >= 0.10) & (pick < 0.15)] = inf
        a[(pick >= 0.15) & (pick < 0.20)] = -inf
        return a
    if kind == "all-nan":
        return np.full((P, npos), nan, dtype=np.float32)
    if kind == "few-non-nan":           # fewer than k entries that are not NaN
        a = np.full((P, npos), nan, dtype=np.float32)
        for p in range(P):
            keep = rng.permutation(npos)[:k - 1]
            a[p, keep] = rng.standard_normal(len(keep)).astype(np.float32)
        return a
    raise AssertionError(kind)


_TOPK_KINDS = ["tie-free", "heavy-ties", "all-equal", "equal-maxima", "all-neg-inf", "scattered-nan-inf", "all-nan", "few-non-nan"]


@pytest.mark.parametrize("kind", _TOPK_KINDS)
@pytest.mark.parametrize("P,npos,k", [(3, 1, 1), (2, 8, 8), (5, 255, 3), (5, 256, 8), (5, 257, 8), (4, 1000, 8)])
def test_topk_ordering_rule(dev, P, npos, k, kind):
    """ties -> lowest index, NaN above +inf: indices and values are the reference rule's; every index in range, none twice.
    (the kernel reads row[i], i < npos, only: whatever the floats hold)"""
    from clc_amd import patch_matching as pm

    rows = _topk_rows(kind, P, npos, k, np.random.default_rng(npos * 10 + k))
    val, idx = pm._topk(torch.from_numpy(rows).reshape(1, P, 1, npos).to(dev), k)
    val, idx = val.cpu().numpy(), idx.cpu().numpy()
    assert val.shape == (P, k) and idx.shape == (P, k)
    assert idx.min() >= 0 and idx.max() < npos, idx
    for p in range(P):
        assert len(set(idx[p].tolist())) == k, idx[p]
    want_val, want_idx = ref.topk(rows, k)
    assert np.array_equal(idx, want_idx), (kind, idx, want_idx)
    assert np.array_equal(val, want_val, equal_nan=True), (kind, val, want_val)
    if kind == "all-equal":
        assert np.array_equal(idx, np.tile(np.arange(k), (P, 1)))


# ------------------------------------------------------------------------------------------------------------------------- gather


def _hip_gather(dev, y, idx, val, k, temperature, ph, pw):
    from clc_amd import lib

    yd = y.to(dev).contiguous()
    _, C, H, W = yd.shape
    idx_d = torch.as_tensor(np.asarray(idx), dtype=torch.int32).reshape(-1, k).contiguous().to(dev)
    val_d = None if val is None else torch.as_tensor(np.asarray(val), dtype=torch.float32).reshape(-1, k).contiguous().to(dev)
    out = torch.empty_like(yd)
    lib.check(lib.load().clc_pm_gather(yd.data_ptr(), C, H, W, ph, pw, None if val_d is None else val_d.data_ptr(), idx_d.data_ptr(), k,
                                       float(temperature), out.data_ptr(), torch.cuda.current_stream().cuda_stream), "clc_pm_gather")
    return out.cpu()


def _gather_indices(rng, P, k, npos):
    """drawn over the whole map (every one checked in range here, on the host); position 0 and the last one appear"""
    idx = rng.integers(0, npos, size=(P, k))
    idx[0, 0], idx[-1, -1] = 0, npos - 1
    assert idx.min() >= 0 and idx.max() < npos
    return idx


@pytest.mark.parametrize("C,H,W,ph,pw", [(3, 16, 24, 8, 8), (1, 8, 36, 4, 12), (3, 16, 16, 16, 16)])
def test_gather_against_float64(dev, C, H, W, ph, pw):
    rng = np.random.default_rng(H * W + pw)
    y = torch.rand(1, C, H, W, generator=torch.Generator().manual_seed(5))
    P, npos = (H // ph) * (W // pw), (H - ph + 1) * (W - pw + 1)
    # k = 1, no weights: a copy
    for last_first in (False, True):
        idx = _gather_indices(rng, P, 1, npos)
        if last_first:
            idx[0, 0] = npos - 1
        got = _hip_gather(dev, y, idx, None, 1, -1.0, ph, pw)
        assert torch.equal(got.double(), ref.gather(y, idx, None, 1, -1.0, ph, pw))
    # softmax(val * 15)-weighted sums
    for k in (3, 8):
        idx = _gather_indices(rng, P, k, npos)
        val = rng.uniform(-1.0, 1.0, size=(P, k)).astype(np.float32)
        got = _hip_gather(dev, y, idx, val, k, 15.0, ph, pw)
        err = (got.double() - ref.gather(y, idx, val, k, 15.0, ph, pw)).abs().max().item()
        print(f"\n  gather {(C, H, W, ph, pw)} k={k} T=15: {err:.3e}")
        assert err <= GATHER_BAR, (k, err)
    # a large temperature, the winner ahead by >= 0.1: the other weights are exp(-100) -> the top-1 patch
    idx = _gather_indices(rng, P, 3, npos)
    val = rng.uniform(-1.0, 0.8, size=(P, 3)).astype(np.float32)
    val[:, 0] = 0.9
    got = _hip_gather(dev, y, idx, val, 3, 1000.0, ph, pw)
    err = (got.double() - ref.gather(y, idx[:, :1], None, 1, -1.0, ph, pw)).abs().max().item()
    print(f"  gather {(C, H, W, ph, pw)} k=3 T=1000 vs top-1 patch: {err:.3e}")
    assert err <= 1e-6, err


def test_si_wraper_stack_on_nan_rows(dev):
    """a map with an all-NaN row and a row of fewer than k numbers: the top-k indices are checked in range ON THE HOST before any
    gather sees them; the stacked candidates then equal the reference's exactly"""
    from clc_amd import patch_matching as pm

    C, H, W, ph, pw, k = 3, 16, 24, 8, 8, 3
    P, ch, cw = 6, 9, 17
    g = torch.Generator().manual_seed(21)
    y = torch.rand(1, C, H, W, generator=g)
    cc = torch.randn(1, P, ch, cw, generator=g)
    cc[0, 1] = float("nan")
    cc[0, 3] = float("nan")
    cc[0, 3, 4, 5], cc[0, 3, 8, 16] = 0.25, 0.75
    cc[0, 4, 0, 0] = float("nan")
    cc[0, 5, 2, 2] = float("inf")
    val, idx = pm._topk(cc.to(dev), k)
    idx_h = idx.cpu().numpy()
    assert idx_h.min() >= 0 and idx_h.max() < ch * cw, idx_h
    want_val, want_idx = ref.topk(cc.reshape(P, -1), k)
    assert np.array_equal(idx_h, want_idx) and np.array_equal(val.cpu().numpy(), want_val, equal_nan=True)
    assert idx_h[1].tolist() == [0, 1, 2] and idx_h[3].tolist() == [0, 1, 2] and idx_h[4, 0] == 0 and idx_h[5, 0] == 2 * cw + 2
    out = pm.SI_Wraper(cc.to(dev), ph, pw, P, y.to(dev), k=k, temperature=15, is_stack=True)
    want = torch.cat([ref.gather(y, want_idx[:, j:j + 1], None, 1, -1.0, ph, pw) for j in range(k)], dim=1)
    assert out.shape == (1, k * C, H, W) and torch.equal(out.cpu().double(), want)


def test_si_wraper_refuses_a_map_of_another_size(dev):
    """in-range indices of a map that is not y's would point outside y: refused by name before the top-k runs"""
    from clc_amd import lib
    from clc_amd import patch_matching as pm

    y = torch.rand(1, 3, 16, 24, device=dev)
    for shape in [(1, 6, 9, 18), (1, 6, 10, 17), (1, 6, 17, 9)]:
        with pytest.raises(lib.ClcError, match="cross_corr map"):
            pm.SI_Wraper(torch.zeros(shape, device=dev), 8, 8, 6, y, k=1)
    assert pm.SI_Wraper(torch.zeros(1, 6, 9, 17, device=dev), 8, 8, 6, y, k=1).shape == (1, 3, 16, 24)


# --------------------------------------------------------------------------------------------------------------------- end to end


def test_finder_end_to_end_planted(dev):
    """every patch of x_dec is cut from y_dec at its own known position: the finder must copy exactly the patches of y_imgs at
    those positions.  (a planted window correlates at 1, any other window of the white-noise image at about 1 / sqrt(192) = 0.07.)"""
    from clc_amd import patch_matching as pm

    N, C, H, W, ph, pw = 2, 3, 32, 48, 8, 8
    g = torch.Generator().manual_seed(31)
    y_dec, y_imgs = torch.rand(N, C, H, W, generator=g), torch.rand(N, C, H, W, generator=g)
    ch, cw, bw = H - ph + 1, W - pw + 1, W // pw
    P = (H // ph) * bw
    x_dec, want = torch.empty(N, C, H, W), torch.empty(N, C, H, W)
    for n in range(N):
        pos = torch.randperm(ch * cw - 2, generator=g)[:P] + 1      # all different; the first and the last position among them
        pos[0], pos[-1] = 0, ch * cw - 1
        for p in range(P):
            iy, ix, by, bx = int(pos[p]) // cw, int(pos[p]) % cw, p // bw, p % bw
            x_dec[n, :, by * ph:(by + 1) * ph, bx * pw:(bx + 1) * pw] = y_dec[n, :, iy:iy + ph, ix:ix + pw]
            want[n, :, by * ph:(by + 1) * ph, bx * pw:(bx + 1) * pw] = y_imgs[n, :, iy:iy + ph, ix:ix + pw]
    out = pm.SI_Finder_at_Image_Domain(x_dec.to(dev), y_imgs.to(dev), ph, pw, y_dec.to(dev))
    assert out.shape == want.shape and torch.equal(out.cpu(), want)
