"""Pins the float64 references of tests/patch_matching_ref.py, without a GPU: the Pearson map and the gather to the golden file of
the genuine functions (tests/golden/patch_matching.npz), the ordering rule to torch.topk / torch.argmax, the colour transform to the
oracle."""
import os

import numpy as np
import pytest
import torch

import patch_matching_ref as ref

GOLD = os.path.join(os.path.dirname(__file__), "golden", "patch_matching.npz")


@pytest.fixture(scope="module")
def gold():
    return {k: torch.from_numpy(v) for k, v in np.load(GOLD).items()}


def test_pearson_map_matches_golden(gold):
    """the golden map is the genuine float32 function's output: its own rounding is what separates the two (4.4e-6 measured)."""
    err = (ref.pearson_map(gold["q"], gold["r"]) - gold["corr"].double()).abs().max().item()
    print(f"\n  float64 pearson_map vs golden corr: {err:.3e}")
    assert err <= 1e-5, err


_PALETTE = np.array([0.0, 0.5, 1.0, np.nan, np.inf, -np.inf], dtype=np.float32)


@pytest.mark.parametrize("n", [1, 8, 255, 257, 1000])
def test_topk_rule_is_torchs(n):
    """rows drawn from {0, 0.5, 1, NaN, +inf, -inf}: the values are torch.topk's (NaN included), for k = 1 the index is
    torch.argmax's; indices are distinct, in range, and point at the values."""
    rng = np.random.default_rng(n)
    for trial in range(20):
        row = _PALETTE[rng.integers(0, len(_PALETTE), size=n)]
        if trial == 0:
            row[:] = np.nan
        if trial == 1:
            row[:] = -np.inf
        t = torch.from_numpy(row)
        for k in sorted({1, min(3, n), min(8, n)}):
            val, idx = ref.topk(row, k)
            want = torch.topk(t, k).values.numpy()
            assert np.array_equal(val, want, equal_nan=True), (n, trial, k, val, want)
            assert len(set(idx.tolist())) == k and idx.min() >= 0 and idx.max() < n
            assert np.array_equal(row[idx], val, equal_nan=True)
            if k == 1:
                assert idx[0] == int(torch.argmax(t)), (n, trial, idx, int(torch.argmax(t)))
            # ties (NaNs among themselves included) come out lowest index first
            for a in range(k - 1):
                same = (np.isnan(val[a]) and np.isnan(val[a + 1])) or val[a] == val[a + 1]
                assert not same or idx[a] < idx[a + 1], (n, trial, k, val, idx)


def test_topk_rows_and_all_equal():
    val, idx = ref.topk(np.full((3, 40), 0.25, dtype=np.float32), 8)
    assert np.array_equal(idx, np.tile(np.arange(8), (3, 1))) and np.all(val == 0.25)
    val, idx = ref.topk(np.array([1.0, np.inf, np.nan, 1.0, np.nan, -np.inf], dtype=np.float32), 6)
    assert idx.tolist() == [2, 4, 1, 0, 3, 5]


def test_prep_matches_oracle(gold):
    """float32 oracle against the float64 chain: about six float32 operations on magnitudes up to 255 / 73 -> rounding bound about 3e-6"""
    from oracle import patch_matching as opm

    x = gold["x_dec"]
    for scale in (255.0, 1.0):
        xin = x if scale == 255.0 else x * 255.0
        want = opm.rgb_transform(opm.reduce_mean_and_std_normalize_images(xin * scale))
        err = (ref.prep(xin, scale) - want.double()).abs().max().item()
        print(f"\n  float64 prep vs oracle, in_scale {scale}: {err:.3e}")
        assert err <= 1e-5, err


def test_gather_matches_oracle(gold):
    """SI_Wraper of the oracle == topk + gather here on the golden map: the stacked candidates exactly (copies), the weighted sum to
    the rounding of the oracle's float32 softmax (weights within 15 * 2^-23 ~ 2e-6 relative, image in [0, 1])."""
    from oracle import patch_matching as opm

    cc, y = gold["corr"] * gold["mask"], gold["y_img"][0:1]
    val, idx = ref.topk(cc.reshape(24, -1), 3)
    tv, ti = torch.topk(cc.reshape(24, -1), 3, dim=1)
    assert np.array_equal(idx, ti.numpy()) and np.array_equal(val, tv.numpy())
    wr = ref.gather(y, idx, val, 3, 15, 16, 16)
    assert wr.shape == gold["wraper_k3"].shape
    err = (wr - gold["wraper_k3"].double()).abs().max().item()
    err_o = (wr - opm.SI_Wraper(cc, 16, 16, 24, y, k=3, temperature=15).double()).abs().max().item()
    print(f"\n  float64 gather vs golden wraper_k3: {err:.3e}, vs oracle: {err_o:.3e}")
    assert err <= 1e-5 and err_o <= 1e-5, (err, err_o)
    stack = torch.cat([ref.gather(y, idx[:, j:j + 1], None, 1, -1.0, 16, 16) for j in range(3)], dim=1)
    assert torch.equal(stack.float(), gold["wraper_k3_stack"])
    assert torch.equal(stack.float(), opm.SI_Wraper(cc, 16, 16, 24, y, k=3, temperature=15, is_stack=True))
    # the finder's copy: the arg-max of the float32 map, candidate 0 as it is
    for n in range(gold["x_dec"].shape[0]):
        q = opm.rgb_transform(opm.reduce_mean_and_std_normalize_images(
            gold["x_dec"][n:n + 1].reshape(1, 3, 4, 16, 6, 16).permute(0, 2, 4, 1, 3, 5).reshape(-1, 3, 16, 16) * 255))
        r = opm.rgb_transform(opm.reduce_mean_and_std_normalize_images(gold["y_dec"][n:n + 1] * 255))
        m = opm.L2_or_pearson_corr(q, r, 16, 16) * gold["mask"]
        _, i1 = ref.topk(m.reshape(24, -1), 1)
        assert torch.equal(ref.gather(gold["y_img"][n:n + 1], i1, None, 1, -1.0, 16, 16).float(), gold["finder"][n:n + 1])
