"""cheng2020 (models.Cheng2020Anchor / Cheng2020Attention) without a GPU: the state_dict surface against the plain-torch restatement
(tests/cheng_ref.py) at K = 1 and K = 3, the constructor's refusals, the compat and zoo names, the stream order, the integer CDF-row
rule of the restatement on hostile parameters, ans.encode_direct against ans.encode, and the argument refusals of the clc_gmm_* entries
(which return before any launch, so they run on a machine without a GPU)."""
import ctypes
import sys

import numpy as np
import pytest
import torch

import cheng_ref

PAIRS = [("Cheng2020Anchor", 1), ("Cheng2020Anchor", 3), ("Cheng2020Attention", 1), ("Cheng2020Attention", 3)]


def _both(name, K, N=24):
    from clc_amd import models

    return getattr(models, name)(N, K), getattr(cheng_ref, name)(N, K)


@pytest.mark.parametrize("name,K", PAIRS)
def test_state_dict_matches_the_restatement_and_loads_both_ways(name, K):
    p, r = _both(name, K)
    sp, sr = p.state_dict(), r.state_dict()
    assert sorted(sp.keys()) == sorted(sr.keys())
    for k in sp:
        assert tuple(sp[k].shape) == tuple(sr[k].shape), k
        assert sp[k].dtype == sr[k].dtype, k
    P = 48 if K == 1 else 3 * K * 24
    assert tuple(sp["entropy_parameters.4.weight"].shape) == (P, 64, 1, 1)
    assert tuple(sp["entropy_parameters.0.weight"].shape) == (80, 96, 1, 1)
    assert tuple(sp["context_prediction.weight"].shape) == (48, 24, 5, 5)
    assert tuple(sp["h_s.8.weight"].shape) == (48, 36, 3, 3) and tuple(sp["h_s.6.0.weight"].shape) == (144, 36, 3, 3)
    assert tuple(sp["g_a.0.conv1.weight"].shape) == (24, 3, 3, 3) and tuple(sp[f"g_s.{9 if 'Att' in name else 7}.0.weight"].shape) == (12, 24, 3, 3)
    assert ("g_a.3.conv_a.0.conv.0.weight" in sp) == ("Att" in name)
    res = p.load_state_dict(sr, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in sr.items():
        assert torch.equal(p.state_dict()[k], v), k
    res = r.load_state_dict(_both(name, K)[0].state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    r.update(force=True)   # a checkpoint saved after update(): the empty CDF buffers are resized
    res = _both(name, K)[0].load_state_dict(r.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys


def test_mixture_adds_no_state_and_has_no_table():
    from clc_amd import entropy_models, models

    p = models.Cheng2020Anchor(24, 3)
    assert not [k for k in p.state_dict() if k.startswith("gaussian_conditional")]
    assert isinstance(p.gaussian_conditional, entropy_models.GaussianMixtureConditional) and p.gaussian_conditional.K == 3
    assert p.gaussian_conditional.update() is False
    assert [k for k in models.Cheng2020Anchor(24, 1).state_dict() if k.startswith("gaussian_conditional")]
    for K in (0, 5):
        with pytest.raises(ValueError, match="between 1 and 4"):
            entropy_models.GaussianMixtureConditional(K)
    with pytest.raises(ValueError, match="0.11"):
        entropy_models.GaussianMixtureConditional(2, scale_bound=0.2)


@pytest.mark.parametrize("name", ["Cheng2020Anchor", "Cheng2020Attention"])
def test_refusals_by_name(name):
    from clc_amd import models

    cls = getattr(models, name)
    with pytest.raises(ValueError, match="cheng2020 qualities 1–3 are not built"):
        cls(128)
    with pytest.raises(ValueError, match=r"N % 12 == 0.*N = 20"):
        cls(20)
    for K in (0, 5):
        with pytest.raises(ValueError, match=rf"K must be between 1 and 4.*K = {K}"):
            cls(24, K)


def test_compat_zoo_and_signatures():
    from clc_amd import compat, lib, models

    for n in ("Cheng2020Anchor", "Cheng2020Attention", "ar_wavefront_order"):
        assert n in models.__all__
    assert issubclass(models.Cheng2020Attention, models.Cheng2020Anchor)
    assert issubclass(models.Cheng2020Anchor, models.JointAutoregressiveHierarchicalPriors)
    saved = {k: v for k, v in sys.modules.items() if k == "models" or k.split(".")[0] in ("compressai", "timm", "pytorch_msssim")}
    try:
        compat.install(force=True)
        import compressai.models as cm
        import compressai.zoo as cz

        assert cm.Cheng2020Anchor is models.Cheng2020Anchor and cm.Cheng2020Attention is models.Cheng2020Attention
        assert cz.models["cheng2020-anchor"] is models.Cheng2020Anchor and cz.models["cheng2020-attn"] is models.Cheng2020Attention
    finally:
        for k in [k for k in sys.modules if k == "models" or k.split(".")[0] in ("compressai", "timm", "pytorch_msssim")]:
            del sys.modules[k]
        sys.modules.update(saved)
    for n in ("clc_gmm_finish", "clc_gmm_commit", "clc_gmm_likelihood_fwd", "clc_gmm_likelihood_bwd", "clc_rans_encode_direct"):
        assert n in lib.SIGNATURES
    assert lib.GMM_R == cheng_ref.R and lib.GMM_ROW_STRIDE == cheng_ref.STRIDE <= 256 and lib.load().clc_gmm_half_width() == cheng_ref.R


LIVE = [(dh, dw) for dh in (-2, -1) for dw in (-2, -1, 0, 1, 2)] + [(0, -2), (0, -1)]


@pytest.mark.parametrize("H,W", [(1, 1), (1, 5), (4, 8), (7, 3), (8, 12)])
def test_ar_wavefront_order(H, W):
    from clc_amd.models import ar_schedule, ar_wavefront_order

    order = ar_wavefront_order(H, W)
    assert order == cheng_ref.ar_wavefront_order(H, W)
    assert sorted(order) == [(h, w) for h in range(H) for w in range(W)]   # every pixel exactly once
    step = {p: p[1] + 3 * p[0] for p in order}
    for (h, w), t in step.items():
        for dh, dw in LIVE:
            q = (h + dh, w + dw)
            if 0 <= q[0] < H and 0 <= q[1] < W:
                assert step[q] < t, ((h, w), q)
    sizes, at = [len(s) for s in ar_schedule(H, W, "wavefront")], 0
    for t, n in enumerate(sizes):   # the step sizes are those of ar_schedule, and inside a step the order is raster
        chunk = order[at:at + n]
        assert all(step[p] == t for p in chunk) and chunk == sorted(chunk)
        at += n
    assert at == H * W


def _hostile_parameters(n=400, K=3, seed=11):
    g = torch.Generator().manual_seed(seed)
    sc = torch.rand((n, K), generator=g) * 3.0 - 0.5            # a fifth under the 0.11 bound, some negative
    mu = torch.randn((n, K), generator=g) * 4.0
    lg = torch.randn((n, K), generator=g) * 2.0
    mu[:40] = torch.where(torch.rand((40, K), generator=g) < 0.5, torch.tensor(1000.0), torch.tensor(-1000.0))
    lg[40:80] = torch.where(torch.rand((40, K), generator=g) < 0.5, torch.tensor(50.0), torch.tensor(-50.0))
    sc[80:90] = 1e-30
    sc[90:100] = 300.0
    bad = [float("nan"), float("inf"), -float("inf")]
    for i in range(100, 190):   # one non-finite entry per row, every (tensor, value, component) combination
        t = (sc, mu, lg)[(i // 3) % 3]
        t[i, i % K] = bad[i % 3]
    sc[190:200], mu[190:200], lg[190:200] = float("nan"), float("inf"), float("nan")
    return sc, mu, lg


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_row_rule_of_the_restatement(dtype):
    sc, mu, lg = _hostile_parameters()
    rows, offsets = cheng_ref.cdf_rows(sc, mu, lg, dtype)
    L = cheng_ref.L
    assert rows.shape == (400, L + 2) and offsets.shape == (400,)
    cheng_ref.check_row_structure(rows)
    assert int((65536 - rows[:, L]).min()) >= 1                         # the tail symbol's frequency
    assert int(offsets.abs().max()) <= (1 << 20) + cheng_ref.R
    # a plain row: the regular symbols carry almost everything when the mixture sits inside the window
    r, o = cheng_ref.cdf_rows(torch.tensor([[1.0, 2.0]]), torch.tensor([[0.2, -3.0]]), torch.tensor([[0.0, 1.0]]), dtype)
    assert int(o[0]) == -2 - cheng_ref.R and int(r[0, L]) >= 65535 - 2 and int(r[0, L // 2 + 4] - r[0, L // 2 - 4]) > 30000


def _symbols_for(rows, offsets, seed=3):
    g = np.random.default_rng(seed)
    n, L = len(offsets), cheng_ref.L
    sym = offsets + g.integers(0, L, n)                                  # inside the window
    sym[::7] = offsets[::7] - 1 - g.integers(0, 40, len(sym[::7]))       # below it
    sym[3::7] = offsets[3::7] + L + g.integers(0, 40, len(sym[3::7]))    # at or above max_value
    sym[5::31] = 1_000_000
    sym[6::31] = -1_000_000
    sym[0], sym[1], sym[2] = offsets[0], offsets[1] + L - 1, offsets[2] + L
    return sym.astype(np.int32)


def test_encode_direct_equals_encode_through_the_full_rows():
    from clc_amd import ans

    sc, mu, lg = _hostile_parameters()
    rows, offsets = cheng_ref.cdf_rows(sc, mu, lg, torch.float64)
    rows, offsets = rows.numpy().astype(np.int32), offsets.numpy().astype(np.int32)
    n, L = len(offsets), cheng_ref.L
    sym = _symbols_for(rows, offsets)
    triples = np.array([cheng_ref.triple_of(rows[i], offsets[i], sym[i]) for i in range(n)], dtype=np.int32)
    assert (triples[:, 2] >= 0).sum() > n // 5 and (triples[:, 2] < 0).sum() > n // 3
    direct = ans.encode_direct(triples)
    full = ans.encode(sym, np.arange(n, dtype=np.int32), rows, np.full(n, L + 2, dtype=np.int32), offsets)
    assert direct == full and len(direct) > 8
    assert ans.encode_direct(triples.reshape(-1)) == full
    d = ans.RansDecoder()
    d.set_stream(direct)
    half = n // 2   # incrementally, on one decoder, through the numpy rows as they are
    got = np.concatenate((d.decode_rows(rows[:half], offsets[:half]), d.decode_rows(rows[half:], offsets[half:])))
    assert np.array_equal(got, sym)
    assert np.array_equal(ans.decode(full, np.arange(n, dtype=np.int32), rows, np.full(n, L + 2, dtype=np.int32), offsets), sym)
    assert ans.encode_direct(np.zeros((0, 3), np.int32)) == ans.encode(np.zeros(0, np.int32), np.zeros(0, np.int32), rows, [L + 2] * n, offsets)
    # a truncated stream ends as it does today: zeros are fed, nothing is read outside the buffer, n symbols come back
    d.set_stream(direct[:8])
    assert d.decode_rows(rows, offsets).shape == (n,)


def test_encode_direct_refusals():
    from clc_amd import ans, lib

    for bad in ([0, 0, -1], [-1, 5, -1], [65530, 10, -1], [0, 65536, -1]):
        with pytest.raises(lib.ClcError, match="clc_rans_encode_direct"):
            ans.encode_direct(np.array([bad], dtype=np.int32))
    with pytest.raises(ValueError, match="3 n"):
        ans.encode_direct(np.zeros(4, np.int32))
    d = ans.RansDecoder()
    d.set_stream(ans.encode_direct(np.array([[0, 10, -1]], dtype=np.int32)))
    with pytest.raises(ValueError, match="int32"):
        d.decode_rows(np.zeros((1, 67), np.int64), np.zeros(1, np.int32))


def test_gmm_argument_refusals_return_before_any_launch():
    """Each call hands the library a host buffer where a device pointer belongs: a launch would fault, a refusal returns -1 first."""
    from clc_amd import lib

    L = lib.load()
    buf = (ctypes.c_float * 4096)()
    ibuf = (ctypes.c_int32 * 4096)()
    p, ip = ctypes.addressof(buf), ctypes.addressof(ibuf)

    def refused(rc, what):
        assert rc == -1
        msg = L.clc_last_error().decode()
        assert what in msg, msg

    fwd = lambda **k: L.clc_gmm_likelihood_fwd(*[{**dict(y=p, ldy=8, noise=p, ldn=8, sc=p, mu=p, wt=p, ldp=24, lik=p, ldl=8, rows=4, C=8, K=3, mode=0,
                                                         st=None), **k}[n] for n in ("y", "ldy", "noise", "ldn", "sc", "mu", "wt", "ldp", "lik", "ldl",
                                                                                     "rows", "C", "K", "mode", "st")])
    refused(fwd(K=0), "K must be between 1 and 4")
    refused(fwd(K=5), "K must be between 1 and 4")
    refused(fwd(y=None), "null pointer")
    refused(fwd(noise=None), "mode 0 needs the noise map")
    refused(fwd(ldp=23), "ldp < K C")
    refused(fwd(ldy=7), "< C")
    refused(fwd(mode=2), "mode must be 0")
    refused(fwd(rows=0), "must be positive")
    bwd = lambda **k: L.clc_gmm_likelihood_bwd(*[{**dict(dlik=p, lddl=8, y=p, ldy=8, noise=p, ldn=8, sc=p, mu=p, wt=p, ldp=24, dy=p, lddy=8, dsc=p, dmu=p,
                                                         dwt=p, lddp=24, rows=4, C=8, K=3, mode=0, st=None), **k}[n]
                                                 for n in ("dlik", "lddl", "y", "ldy", "noise", "ldn", "sc", "mu", "wt", "ldp", "dy", "lddy", "dsc", "dmu",
                                                           "dwt", "lddp", "rows", "C", "K", "mode", "st")])
    refused(bwd(K=7), "K must be between 1 and 4")
    refused(bwd(dwt=None), "null pointer")
    refused(bwd(lddp=20), "lddp < K C")
    refused(bwd(mode=1), "mode 1 has no gradient of y")
    fin = lambda **k: L.clc_gmm_finish(*[{**dict(gp=p, ldg=72, N=8, K=3, pix=ip, P=2, B=1, H=2, W=2, y=p, ldy=8, yh=p, ldh=8, tr=ip, rows=ip, offs=ip,
                                                 mode=lib.AR_ENCODE, st=None), **k}[n]
                                         for n in ("gp", "ldg", "N", "K", "pix", "P", "B", "H", "W", "y", "ldy", "yh", "ldh", "tr", "rows", "offs", "mode", "st")])
    refused(fin(K=0), "K must be between 1 and 4")
    refused(fin(ldg=71), "ldg < 3 K N")
    refused(fin(gp=None), "null pointer")
    refused(fin(mode=2), "mode must be CLC_AR_ENCODE or CLC_AR_DECODE")
    refused(fin(tr=None), "encode mode needs")
    refused(fin(mode=lib.AR_DECODE, offs=None), "decode mode needs")
    refused(fin(B=1 << 20, H=1 << 10, W=1 << 10), "below 2^31")
    refused(fin(P=0), "must be positive")
    com = lambda **k: L.clc_gmm_commit(*[{**dict(sym=ip, N=8, pix=ip, P=2, B=1, H=2, W=2, yh=p, ldh=8, st=None), **k}[n]
                                         for n in ("sym", "N", "pix", "P", "B", "H", "W", "yh", "ldh", "st")])
    refused(com(sym=None), "null pointer")
    refused(com(ldh=7), "ldh < N")
    refused(com(N=0), "must be positive")


def test_wrappers_refuse_the_cpu_by_name():
    from clc_amd import entropy_models, lib, models

    gm = entropy_models.GaussianMixtureConditional(2)
    y, g = torch.zeros(1, 4, 2, 2), torch.zeros(1, 8, 2, 2)
    with pytest.raises(lib.ClcError, match="gmm_likelihood"):
        gm(y, g, g, g, training=False)
    with pytest.raises(lib.ClcError):
        models.Cheng2020Anchor(24, 3)(torch.zeros(1, 3, 64, 64))
