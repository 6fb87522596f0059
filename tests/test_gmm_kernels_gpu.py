"""csrc/gmm.hip against float64 (tests/cheng_ref.py): the mixture likelihood forward and backward (both LowerBound gradient rules, with
mixed-sign upstream gradients), the per-symbol integer CDF rows of clc_gmm_finish in both modes, clc_gmm_commit, and the named refusals.

Bars.  The likelihood's arithmetic is GaussianConditional's per component, so the bars are those of
tests/test_kernels_gpu.py::test_gaussian_likelihood: likelihood 1e-5 of the largest value, 2e-3 in the log domain, gradients 2e-4.
A CDF-row entry is j + floor((G_j - G_0) S) with S < 2^16: an f32 mixture CDF is good to a few 2^-24, so against the same rule in float64
ON THE GPU'S OWN PARAMETER FLOATS an entry can move by one count, and only when the exact value sits next to an integer (measured:
about 15 % of the entries do, all of them by one — the flat upper tail of a row, where the exact value lies just under the integer S
and the f32 CDF has rounded to 1).  The centre
round(sum pi mu) can flip only next to a half-integer: elements whose float64 mixture mean lies within 1e-4 of one are left out of that
comparison (a condition on the inputs, at most 1 % of them), never out of the structural checks.
"""
import numpy as np
import pytest
import torch

import cheng_ref

pytestmark = pytest.mark.gpu
CL = torch.channels_last
R, L, S = cheng_ref.R, cheng_ref.L, cheng_ref.STRIDE


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _close(a, b, tol, what=""):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    scale = max(b.abs().max().item(), 1e-6)
    err = (a - b).abs().max().item() / scale
    print(f"{what}: rel err {err:.3e} (scale {scale:.3e})")
    assert err <= tol, f"{what}: rel err {err:.3e} > {tol:.1e} (scale {scale:.3e})"


def _lik_inputs(shape, K, seed):
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(s, generator=g)
    y = rn(B, C, H, W) * 3.0
    sc = rn(B, K * C, H, W) + 0.5          # some below the 0.11 bound, some negative
    mu = rn(B, K * C, H, W) * 2.0
    wt = rn(B, K * C, H, W) * 1.5
    noise = torch.rand((B, C, H, W), generator=g) - 0.5
    up = torch.rand((B, C, H, W), generator=g) - 0.7   # mixed-sign upstream gradients (the LowerBound rule)
    return y, sc, mu, wt, noise, up


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("training", [False, True])
@pytest.mark.parametrize("shape,K", [((2, 8, 5, 7), 3), ((1, 6, 3, 3), 2)])
def test_gmm_likelihood_against_float64(dev, shape, K, training, packed):
    from clc_amd import entropy_models
    from oracle.leaves import LowerBound

    y, sc, mu, wt, noise, up = _lik_inputs(shape, K, 7)
    y64, sc64, mu64, wt64 = (t.double().requires_grad_() for t in (y, sc, mu, wt))
    v = y64 + noise.double() if training else torch.round(y64)
    ref = cheng_ref.mixture_likelihood(v, sc64, mu64, wt64, K, (LowerBound(0.11).double(), LowerBound(1e-9).double()))
    (ref * up.double()).sum().backward()
    assert float((sc < 0.11).float().mean()) > 0.2 and float(ref.min()) < 1e-6 < float(ref.max())

    gm = entropy_models.GaussianMixtureConditional(K).to(dev)
    yd = y.to(dev).contiguous(memory_format=CL).requires_grad_()
    orig = torch.Tensor.uniform_
    torch.Tensor.uniform_ = lambda t, a=0.0, b=1.0, generator=None: t.copy_(noise.to(t.device))
    try:
        if packed:
            gp = torch.cat((sc, mu, wt), 1).to(dev).contiguous(memory_format=CL).requires_grad_()
            out, lik = gm.forward_packed(yd, gp, training=training)
        else:
            scd, mud, wtd = (t.to(dev).contiguous(memory_format=CL).requires_grad_() for t in (sc, mu, wt))
            out, lik = gm(yd, scd, mud, wtd, training=training)
    finally:
        torch.Tensor.uniform_ = orig
    assert torch.equal(out.detach().cpu(), (y + noise) if training else torch.round(y))
    _close(lik, ref, 1e-5, "gmm lik")
    gap = (torch.log(lik.detach().cpu().double()) - torch.log(ref.detach())).abs().max().item()
    print(f"log-domain gap {gap:.3e}")
    assert gap < 2e-3
    (lik * up.to(dev)).sum().backward()
    KC = K * shape[1]
    got = (gp.grad[:, :KC], gp.grad[:, KC:2 * KC], gp.grad[:, 2 * KC:]) if packed else (scd.grad, mud.grad, wtd.grad)
    for name, a, b in zip(("dscales", "dmeans", "dweights"), got, (sc64.grad, mu64.grad, wt64.grad)):
        assert float(b.abs().max()) > 0
        _close(a, b, 2e-4, "gmm " + name)
    if training:
        _close(yd.grad, y64.grad, 2e-4, "gmm dy")
    else:
        assert yd.grad is None or float(yd.grad.abs().max()) == 0.0


def test_one_component_with_zero_logits_is_the_gaussian_kernel(dev):
    from clc_amd import ops

    y, sc, mu, wt, noise, _ = _lik_inputs((2, 8, 5, 7), 1, 9)
    yd, scd, mud, nd = (t.to(dev).contiguous(memory_format=CL) for t in (y, sc, mu, noise))
    for training in (False, True):
        ref, _ = ops.gaussian_likelihood(yd, scd, mud, nd if training else None, training)
        if not training:   # the Gaussian kernel rounds y - mu, the mixture rounds y: compare at integer means
            ref, _ = ops.gaussian_likelihood(yd, scd, torch.round(mud), None, False)
        got = ops.gmm_likelihood(yd, scd, mud if training else torch.round(mud), torch.zeros_like(scd), nd if training else None, training, 1)
        _close(got, ref, 1e-5, f"K = 1 against gaussian_likelihood (training={training})")
        assert (torch.log(got) - torch.log(ref)).abs().max().item() < 2e-3


# ---------------------------------------------------------------------------------------------------------------- the coder kernels
H_, W_, N_, K_ = 3, 5, 8, 3


def _gp_rows(rows, seed, hostile=False):
    g = torch.Generator().manual_seed(seed)
    sc = torch.rand((rows, K_, N_), generator=g) * 3.0 - 0.3
    mu = torch.randn((rows, K_, N_), generator=g) * 5.0
    lg = torch.randn((rows, K_, N_), generator=g) * 2.0
    if hostile:
        bad = torch.tensor([float("nan"), float("inf"), -float("inf")])
        for t in (sc, mu, lg):
            hit = torch.rand(t.shape, generator=g) < 0.15
            t[hit] = bad[torch.randint(0, 3, (int(hit.sum()),), generator=g)]
    return torch.cat((sc.reshape(rows, -1), mu.reshape(rows, -1), lg.reshape(rows, -1)), 1).contiguous()   # [rows, 3 K N]: part, k, c


def _split(gp):
    """[rows, 3 K N] -> scales, means, logits as [rows * N, K] in element order (row, channel)"""
    rows = gp.shape[0]
    return tuple(gp.reshape(rows, 3, K_, N_)[:, i].permute(0, 2, 1).reshape(rows * N_, K_) for i in range(3))


def _pix(dev, P=None):
    from clc_amd.models import ar_wavefront_order

    order = ar_wavefront_order(H_, W_)
    if P is not None:
        order = [order[(7 * i + 3) % len(order)] for i in range(P)]
    return order, torch.tensor(order, dtype=torch.int32).reshape(-1, 2).to(dev)


def _decode_rows(gp, pix, B, dev):
    from clc_amd import ops

    rows = B * pix.shape[0]
    out = torch.full((rows, N_, S), -7, device=dev, dtype=torch.int32)
    offs = torch.full((rows, N_), -7, device=dev, dtype=torch.int32)
    ops.gmm_finish_decode(gp, N_, K_, pix, B, H_, W_, out, offs)
    return out.cpu(), offs.cpu()


@pytest.mark.parametrize("B", [1, 3])
def test_gmm_finish_rows_and_triples(dev, B):
    from clc_amd import ops

    order, pix = _pix(dev)
    P = len(order)
    gp = _gp_rows(B * P, 20 + B)
    gpd = gp.to(dev)
    rows, offs = _decode_rows(gpd, pix, B, dev)
    cheng_ref.check_row_structure(rows.reshape(-1, S))
    assert int((65536 - rows[..., L]).min()) >= 1
    # float64, from the same parameter floats
    sc, mu, lg = _split(gp)
    rows64, offs64 = cheng_ref.cdf_rows(sc, mu, lg, torch.float64)
    m64 = (torch.softmax(lg.double(), 1) * mu.double()).sum(1)
    safe = ((m64 - torch.floor(m64)) - 0.5).abs() > 1e-4
    assert 1.0 - safe.double().mean().item() <= 0.01
    assert torch.equal(offs.reshape(-1).long()[safe], offs64[safe])
    diff = (rows.reshape(-1, S).long() - rows64)[safe].abs()
    print(f"B = {B}: {100.0 * (diff > 0).double().mean().item():.3f} % of the row entries differ from float64 (by at most {int(diff.max())})")
    assert int(diff.max()) <= 1
    assert int((rows64[:, L] - rows64[:, 0]).max()) > 60000   # informative rows, not all-tail

    # encode mode: y around the centres, some outside the window and far outside
    ctr = (offs.reshape(B, P, N_) + R).float()
    g = torch.Generator().manual_seed(5)
    yv = ctr + torch.randn(ctr.shape, generator=g) * 2.0
    yv[:, 0, 0], yv[:, 1, 1], yv[:, 2, 2], yv[:, 3, 3] = ctr[:, 0, 0] + (R + 5), ctr[:, 1, 1] - (R + 5), 1000.0, -1000.0
    yv[:, 4, 4], yv[:, 5, 5], yv[:, 6, 6] = ctr[:, 4, 4] - R, ctr[:, 5, 5] + R, ctr[:, 6, 6] + R + 1   # the window's first, last, first outside
    y = torch.zeros(B, N_, H_, W_)
    for p, (h, w) in enumerate(order):
        y[:, :, h, w] = yv[:, p]
    yd = y.to(dev).contiguous(memory_format=CL)
    y_hat = torch.full_like(yd, -5.0)
    triples = torch.full((B, P, N_, 3), -9, device=dev, dtype=torch.int32)
    ops.gmm_finish_encode(gpd, N_, K_, pix, yd, y_hat, triples)
    assert torch.equal(y_hat.cpu(), torch.round(y))
    t = triples.cpu().reshape(-1, 3)
    sym = torch.round(yv).reshape(-1)
    want = torch.tensor([cheng_ref.triple_of(rows.reshape(-1, S)[i], offs.reshape(-1)[i], sym[i]) for i in range(t.shape[0])], dtype=torch.int32)
    assert torch.equal(t, want)
    assert int((t[:, 2] >= 0).sum()) >= 5 * B and int((t[:, 2] < 0).sum()) > t.shape[0] // 2
    # and the streams: the triples through encode_direct decode through the decode-mode rows
    from clc_amd import ans

    per = P * N_
    for b in range(B):
        s = ans.encode_direct(t[b * per:(b + 1) * per].numpy())
        d = ans.RansDecoder()
        d.set_stream(s)
        back = d.decode_rows(np.ascontiguousarray(rows.reshape(-1, S)[b * per:(b + 1) * per].numpy()),
                             np.ascontiguousarray(offs.reshape(-1)[b * per:(b + 1) * per].numpy()))
        assert np.array_equal(back, sym[b * per:(b + 1) * per].numpy().astype(np.int32))


def test_gmm_finish_row_does_not_depend_on_its_surroundings(dev):
    from clc_amd import ops

    one = _gp_rows(1, 77)
    y = (torch.randn(3, N_, H_, W_, generator=torch.Generator().manual_seed(8)) * 6.0).to(dev).contiguous(memory_format=CL)
    results = []
    for P, B, b, at in ((1, 1, 0, 0), (5, 1, 0, 3), (40, 1, 0, 29), (5, 3, 1, 2), (1, 1, 0, 0)):
        order, pix = _pix(dev, P)
        order1, _ = _pix(dev, 1)
        # the pixel of the row under test is always the same one
        lst = list(order)
        lst[at] = order1[0]
        pix = torch.tensor(lst, dtype=torch.int32).reshape(-1, 2).to(dev)
        gp = _gp_rows(B * P, 100 + P + B)
        gp[b * P + at] = one[0]
        gpd = gp.to(dev)
        rows, offs = _decode_rows(gpd, pix, B, dev)
        yb = y[:B].clone()
        yb[b] = y[0]
        y_hat = torch.zeros_like(yb)
        triples = torch.zeros((B, P, N_, 3), device=dev, dtype=torch.int32)
        ops.gmm_finish_encode(gpd, N_, K_, pix, yb, y_hat, triples)
        results.append((rows[b * P + at].clone(), offs[b * P + at].clone(), triples[b, at].cpu().clone()))
    for r in results[1:]:
        for a, b_ in zip(results[0], r):
            assert torch.equal(a, b_)


def test_gmm_finish_hostile_parameters_still_give_valid_rows(dev):
    order, pix = _pix(dev)
    gp = _gp_rows(len(order), 31, hostile=True)
    assert int(torch.isnan(gp).sum()) > 20 and int(torch.isinf(gp).sum()) > 40
    gp[0], gp[1, :K_ * N_], gp[2, 2 * K_ * N_:] = float("nan"), float("inf"), -float("inf")
    rows, offs = _decode_rows(gp.to(dev), pix, 1, dev)
    cheng_ref.check_row_structure(rows.reshape(-1, S))
    assert int((65536 - rows[..., L]).min()) >= 1
    assert int(offs.abs().max()) <= (1 << 20) + R


def test_gmm_commit_writes_the_listed_pixels_only(dev):
    from clc_amd import ops

    order, _ = _pix(dev)
    some = order[2:9]
    pix = torch.tensor(some, dtype=torch.int32).reshape(-1, 2).to(dev)
    B = 2
    sym = torch.randint(-3000, 3000, (B * len(some), N_), generator=torch.Generator().manual_seed(2), dtype=torch.int32)
    wide = torch.full((B, N_ + 4, H_, W_), 123.5, device=dev).contiguous(memory_format=CL)
    y_hat = wide[:, :N_]   # a channel range of a wider map: ldh > N
    ops.gmm_commit(sym.to(dev), N_, pix, y_hat)
    want = torch.full((B, N_ + 4, H_, W_), 123.5)
    for b in range(B):
        for p, (h, w) in enumerate(some):
            want[b, :N_, h, w] = sym[b * len(some) + p].float()
    assert torch.equal(wide.cpu(), want)


def test_named_refusals(dev):
    from clc_amd import lib, ops

    order, pix = _pix(dev)
    P = len(order)
    gp = _gp_rows(P, 1).to(dev)
    y = torch.zeros(1, N_, H_, W_, device=dev).contiguous(memory_format=CL)
    tr = torch.zeros((1, P, N_, 3), device=dev, dtype=torch.int32)
    with pytest.raises(ValueError, match="triples must be"):
        ops.gmm_finish_encode(gp, N_, K_, pix, y, torch.zeros_like(y), tr[:, :-1])
    with pytest.raises(ValueError, match="needs 3 K N"):
        ops.gmm_finish_encode(gp[:, :-4], N_, K_, pix, y, torch.zeros_like(y), tr)
    with pytest.raises(ValueError, match="cdf_rows must be"):
        ops.gmm_finish_decode(gp, N_, K_, pix, 1, H_, W_, torch.zeros((P, N_, S - 1), device=dev, dtype=torch.int32),
                              torch.zeros((P, N_), device=dev, dtype=torch.int32))
    with pytest.raises(ValueError, match="offsets"):
        ops.gmm_finish_decode(gp, N_, K_, pix, 1, H_, W_, torch.zeros((P, N_, S), device=dev, dtype=torch.int32),
                              torch.zeros((P, N_ + 1), device=dev, dtype=torch.int32))
    with pytest.raises(lib.ClcError, match="K must be between 1 and 4"):
        ops.gmm_finish_encode(torch.zeros((P, 3 * 5 * N_), device=dev), N_, 5, pix, y, torch.zeros_like(y), tr)
    with pytest.raises(ValueError, match="gmm_commit"):
        ops.gmm_commit(torch.zeros((P, N_ + 1), device=dev, dtype=torch.int32), N_, pix, y)
    g = torch.zeros(1, 2 * N_, H_, W_, device=dev).contiguous(memory_format=CL)
    with pytest.raises(ValueError, match="parameter group"):
        ops.gmm_likelihood(y, g, g, g, None, False, 3)
    with pytest.raises(lib.ClcError, match="K must be between 1 and 4"):
        ops.gmm_likelihood(y, torch.cat([g] * 3, 1)[:, :5 * N_], torch.cat([g] * 3, 1)[:, :5 * N_], torch.cat([g] * 3, 1)[:, :5 * N_], None, False, 5)
    with pytest.raises(ValueError, match="3 K C"):
        ops.gmm_likelihood_packed(y, g, None, False, 3)
