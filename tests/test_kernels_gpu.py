"""GPU parity of every HIP kernel (through the C ABI via clc_amd.ops) against plain-PyTorch CPU references.

Tolerances (fp32 kernels on f32 MFMA == exact fmaf chains; the only difference to the CPU
reference is summation order): rel 2e-5 of the output scale for forward, 1e-4 for gradients
(long split-K reductions).  Integer outputs (symbols / indexes) must be bit-exact.
"""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CL = torch.channels_last


def _close(a, b, tol, what=""):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    scale = max(b.abs().max().item(), 1e-6)
    err = (a - b).abs().max().item() / scale
    assert err <= tol, f"{what}: rel err {err:.3e} > {tol:.1e} (scale {scale:.3e})"


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def _dev(t, dev, cl=True, grad=False):
    t = t.to(dev)
    if cl and t.dim() == 4:
        t = t.contiguous(memory_format=CL)
    return t.requires_grad_(grad)


CONV_CASES = [
    # N, Cin, H, W, Cout, ks, stride
    (2, 64, 32, 32, 64, 3, 1),
    (1, 128, 16, 16, 128, 3, 1),
    (2, 128, 32, 32, 128, 3, 2),
    (2, 128, 32, 32, 128, 1, 2),
    (1, 448, 16, 16, 224, 3, 1),
    (1, 224, 16, 16, 128, 3, 1),
    (2, 64, 16, 16, 192, 1, 1),
    (1, 3, 64, 64, 128, 3, 2),
    (8, 320, 16, 16, 128, 3, 2),
    (1, 192, 4, 4, 512, 3, 1),
    (3, 128, 24, 40, 96, 3, 1),  # ragged: non power-of-two map, Cout not a tile multiple
    (2, 64, 8, 8, 96, 3, 1),     # all-taps filter gradient, 4x8 pixel tiles
    (1, 64, 64, 128, 64, 3, 1),  # all-taps filter gradient, 1x32 pixel tiles, non-square map
    (2, 96, 32, 16, 160, 3, 1),  # all-taps filter gradient, 2x16 tiles, channel counts that are not tile multiples
    # the tiles that dominate the timed step (selection rules at the end of clc_conv2d, csrc/conv_igemm.hip): per-image map
    # > 1024 pixels and Cout % 128 == 0 -> conv_igemm_dma2_kernel<128,128,4,2,*>; 64 channels -> <128,64,...>; with the fused
    # activation derivative (act 1 / 3) the data gradients run on the register-staged conv_igemm_kernel<...,true>; the 3x3
    # filter gradients of these maps run on conv_wgrad_taps(_grouped)_kernel<32>
    (8, 128, 128, 128, 128, 3, 1),
    (8, 128, 64, 64, 512, 3, 1),
    (8, 128, 128, 128, 128, 1, 1),
    (8, 64, 128, 128, 64, 3, 1),
]


def test_wgrad_batched_matches_single_launches(dev):
    """clc_conv2d_wgrad_batched == the same problems launched one by one, bit for bit: mixed tile shapes, the RGB
    small path, K-splits, fused activation derivative, more problems than one group holds, and a filter that is
    written twice (accumulation order preserved)."""
    from clc_amd import ops

    shapes = [(8, 64, 16, 16, 64, 3, 1), (8, 224, 16, 16, 128, 3, 1), (8, 128, 16, 16, 32, 3, 1), (8, 64, 16, 16, 128, 1, 1),
              (2, 128, 64, 64, 128, 3, 1), (2, 128, 32, 32, 256, 3, 2), (1, 3, 64, 64, 128, 3, 2), (3, 128, 24, 40, 96, 3, 1),
              (8, 448, 16, 16, 224, 3, 1), (1, 192, 4, 4, 512, 3, 1)] * 2 + [(8, 64, 16, 16, 64, 3, 1)] * 3
    probs = []
    for i, (N, Cin, H, W, Cout, ks, stride) in enumerate(shapes):
        pad = ks // 2
        OH, OW = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
        x = _dev(_rand((N, Cin, H, W), 100 + i), dev).contiguous(memory_format=torch.channels_last)
        dy = _dev(_rand((N, Cout, OH, OW), 200 + i), dev).contiguous(memory_format=torch.channels_last)
        pre = _dev(_rand((N, Cout, OH, OW), 300 + i), dev).contiguous(memory_format=torch.channels_last)
        kw = dict(x=x, dy=dy, ks=ks, stride=stride, pad=pad, Cout=Cout, Cin=Cin, want_bias=True)
        if i % 3 == 1:
            kw.update(dys=pre, dys_act=1, dys_pre=True)
        probs.append(kw)

    def buffers():
        out = []
        for i, kw in enumerate(probs):
            if i >= len(probs) - 2:   # the last two problems accumulate into the buffers of the third-last one
                out.append(out[len(probs) - 3])
            else:
                n = kw["Cout"] * kw["ks"] ** 2 * kw["Cin"]
                out.append((torch.full((n,), 0.25, device=dev), torch.full((kw["Cout"],), -0.5, device=dev)))
        return out

    from clc_amd import lib as _lib

    single = buffers()
    for kw, (dw, db) in zip(probs, single):
        ops.wgrad_raw(**kw, dw_out=dw, db_out=db)

    def run_batched():
        out = buffers()
        keep = ops.wgrad_batched([dict(kw, dw_out=dw, db_out=db) for kw, (dw, db) in zip(probs, out)])
        torch.cuda.synchronize()
        del keep
        return out

    # (a) split-K grouped form (tuning key 1 = 0): the same launches as the single calls, bit for bit
    prev = _lib.load().clc_set_tuning(1, 0)
    try:
        batched = run_batched()
    finally:
        _lib.load().clc_set_tuning(1, prev)
    for i, ((dw1, db1), (dw2, db2)) in enumerate(zip(single, batched)):
        assert torch.equal(dw1, dw2), f"problem {i}: dW differs"
        assert torch.equal(db1, db2), f"problem {i}: dbias differs"
    # (b) stream-K grouped form (default): another split of the K range -> equal up to fp32 summation order, and run-to-run
    #     reproducible bit for bit (the ranges are a function of the group's shapes only)
    sk1, sk2 = run_batched(), run_batched()
    for i, ((dw1, db1), (dw2, db2), (dw3, db3)) in enumerate(zip(single, sk1, sk2)):
        assert torch.equal(dw2, dw3) and torch.equal(db2, db3), f"problem {i}: stream-K result is not reproducible"
        _close(dw2, dw1, 1e-5, f"problem {i}: stream-K dW vs split-K")
        _close(db2, db1, 1e-5, f"problem {i}: stream-K dbias vs split-K")
    batched = sk1
    # and against the fp32 reference for one grouped problem
    kw = probs[0]
    wref = torch.zeros(64, 64, 3, 3, requires_grad=True)
    F.conv2d(kw["x"].cpu(), wref, None, padding=1).backward(kw["dy"].cpu())
    got = (batched[0][0] - 0.25).view(64, 3, 3, 64).permute(0, 3, 1, 2).cpu()
    _close(got, wref.grad, 1e-4, "grouped wgrad vs torch")


@pytest.mark.parametrize("case", CONV_CASES)
@pytest.mark.parametrize("act", [0, 1, 3])
def test_conv_fwd_bwd(dev, case, act):
    from clc_amd import ops

    N, Cin, H, W, Cout, ks, stride = case
    if N * H * W >= 8 * 64 * 64 and act == 3:
        pytest.skip("large-map cases: GELU adds nothing over act 0 / 1 (same kernels as act 1's fused-derivative path)")
    x = _rand((N, Cin, H, W), 1)
    w = _rand((Cout, Cin, ks, ks), 2, (1.0 / (Cin * ks * ks)) ** 0.5)
    b = _rand((Cout,), 3, 0.1)
    xr, wr, br = x.clone().requires_grad_(Cin != 3), w.clone().requires_grad_(), b.clone().requires_grad_()
    xd, wd, bd = _dev(x, dev, grad=Cin != 3), _dev(w, dev, grad=True), _dev(b, dev, grad=True)
    y = ops.conv2d(xd, wd, bd, stride=stride, act=act)
    ref = F.conv2d(xr, wr, br, stride=stride, padding=ks // 2)
    if act == 1:
        # LeakyReLU's derivative jumps at 0: a pre-activation of ~1e-8 can round to either side in two fp32 summation
        # orders, which moves dW by |dy*x| ~ 1e-2 of its scale.  Take the branch from the kernel's own output so the
        # comparison tests arithmetic, not the coin flip (the forward check still pins y to 2e-5).
        ref = torch.where(y.detach().cpu() > 0, ref, 0.01 * ref)
    else:
        ref = {0: ref, 3: F.gelu(ref)}[act]
    gy = _rand(ref.shape, 4)
    ref.backward(gy)
    assert y.shape == ref.shape
    _close(y, ref, 2e-5, "conv fwd")
    y.backward(_dev(gy, dev))
    _close(wd.grad, wr.grad, 1e-4, "conv wgrad")
    _close(bd.grad, br.grad, 1e-4, "conv bgrad")
    if Cin != 3:
        _close(xd.grad, xr.grad, 1e-4, "conv dgrad")


# (4, 320, 24, 24, 224, 3): the first layer of the paired slice nets of a 384x384 image at batch 2 (1152-row halves on the 64x64 tiles)
@pytest.mark.parametrize("case", [(8, 64, 16, 16, 64, 3), (8, 128, 16, 16, 64, 1), (2, 448, 16, 16, 224, 3), (2, 64, 64, 64, 128, 3), (4, 64, 32, 32, 64, 1),
                                  (4, 320, 24, 24, 224, 3)])
def test_conv_paired_filters(dev, case, request):
    """w2/bias2: the second half of the batch on a second filter set in the same launch == two separate launches, bit
    for bit (forward, data gradient, both filter gradients), for both kernel families."""
    from clc_amd import ops

    N, Cin, H, W, Cout, ks = case
    h = N // 2
    # (the paired launch has no Winograd form: compare with separate launches on the same, direct kernels — key 23 off for this test)
    request.addfinalizer(lambda old=ops._L().clc_set_tuning(23, 0): ops._L().clc_set_tuning(23, old))
    x = _rand((N, Cin, H, W), 1)
    w1, w2 = _rand((Cout, Cin, ks, ks), 2, 0.05), _rand((Cout, Cin, ks, ks), 3, 0.05)
    b1, b2 = _rand((Cout,), 4, 0.1), _rand((Cout,), 5, 0.1)
    gy = _rand((N, Cout, H, W), 6)
    for act in (0, 1, 3):
        xs, ws = _dev(x, dev, grad=True), [_dev(t, dev, grad=True) for t in (w1, b1, w2, b2)]
        ya = ops.conv2d(xs[:h], ws[0], ws[1], act=act)
        yb = ops.conv2d(xs[h:], ws[2], ws[3], act=act)
        torch.cat((ya, yb), 0).backward(_dev(gy, dev))
        xp, wp = _dev(x, dev, grad=True), [_dev(t, dev, grad=True) for t in (w1, b1, w2, b2)]
        yp = ops.conv2d(xp, wp[0], wp[1], act=act, w2=wp[2], b2=wp[3])
        yp.backward(_dev(gy, dev))
        assert torch.equal(yp[:h], ya) and torch.equal(yp[h:], yb), f"act {act}: paired forward differs"
        assert torch.equal(xp.grad, xs.grad), f"act {act}: paired data gradient differs"
        for a, b, name in zip(wp, ws, ("w", "b", "w2", "b2")):
            assert torch.equal(a.grad, b.grad), f"act {act}: paired {name} gradient differs"


@pytest.mark.parametrize("case", [(8, 64, 16, 16, 64, 3), (8, 128, 16, 16, 64, 1), (16, 64, 16, 16, 128, 1), (4, 64, 32, 32, 64, 3), (4, 128, 64, 64, 128, 1)])
def test_conv_four_filter_sets(dev, case):
    """w3 / w4: the four quarters of the batch on four filter sets in one launch == four separate launches, bit for bit (forward,
    data gradient, all filter / bias gradients) — the ResidualUnit chains of a paired attention block (layers.SWAtten)."""
    from clc_amd import ops

    N, Cin, H, W, Cout, ks = case
    q = N // 4
    x = _rand((N, Cin, H, W), 1)
    wb = [t for k in range(4) for t in (_rand((Cout, Cin, ks, ks), 2 + 2 * k, 0.05), _rand((Cout,), 3 + 2 * k, 0.1))]
    gy = _rand((N, Cout, H, W), 11)
    for act in (0, 2):
        xs, ws = _dev(x, dev, grad=True), [_dev(t, dev, grad=True) for t in wb]
        ys = [ops.conv2d(xs[k * q:(k + 1) * q], ws[2 * k], ws[2 * k + 1], act=act) for k in range(4)]
        torch.cat(ys, 0).backward(_dev(gy, dev))
        xp, wp = _dev(x, dev, grad=True), [_dev(t, dev, grad=True) for t in wb]
        yp = ops.conv2d(xp, wp[0], wp[1], act=act, w2=wp[2], b2=wp[3], wx=((wp[4], wp[5]), (wp[6], wp[7])))
        yp.backward(_dev(gy, dev))
        for k in range(4):
            assert torch.equal(yp[k * q:(k + 1) * q], ys[k]), f"act {act}: forward of set {k} differs"
        assert torch.equal(xp.grad, xs.grad), f"act {act}: data gradient differs"
        for i, (a, b) in enumerate(zip(wp, ws)):
            assert torch.equal(a.grad, b.grad), f"act {act}: gradient of {'wb'[i % 2]}{i // 2 + 1} differs"


@pytest.mark.parametrize("inverse", [False, True])
def test_gdn_raw_parameters(dev, inverse):
    """layers.GDN on the raw gamma / beta (fused NonNegativeParametrizer forward + LowerBound-rule backward) against the
    oracle's CompressAI GDN, with parameters on both sides of the bound and gradients of both signs."""
    from clc_amd import layers
    from oracle import leaves

    C = 64
    torch.manual_seed(5)
    ref = leaves.GDN(C, inverse=inverse)
    with torch.no_grad():
        ref.gamma.add_(torch.randn(C, C) * 0.02)            # many entries end up below the bound (2^-18) and negative
        ref.beta.add_(torch.randn(C) * 0.5).clamp_(min=-0.5)
    mod = layers.GDN(C, inverse=inverse)
    mod.load_state_dict(ref.state_dict())
    mod = mod.to(dev)
    x = _rand((2, C, 16, 16), 1)
    gy = _rand((2, C, 16, 16), 2)
    xr = x.clone().requires_grad_()
    ref(xr).backward(gy)
    xd = _dev(x, dev, grad=True)
    y = mod(xd)
    _close(y, ref(x).detach(), 2e-5, "gdn(raw) fwd")
    y.backward(_dev(gy, dev))
    _close(xd.grad, xr.grad, 1e-4, "gdn(raw) dx")
    _close(mod.gamma.grad, ref.gamma.grad, 1e-4, "gdn(raw) dgamma")
    _close(mod.beta.grad, ref.beta.grad, 1e-4, "gdn(raw) dbeta")


def test_conv_residual_slice_shuffle(dev):
    from clc_amd import ops

    # channel-slice input (split view), residual with scale, lrelu + residual (needs saved pre-activation)
    N, C, H, W = 2, 128, 32, 32
    u = _rand((N, C, H, W), 1)
    w = _rand((64, 64, 3, 3), 2, 0.05)
    b = _rand((64,), 3, 0.1)
    ur, wr, br = u.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
    cr = ur[:, :64]
    ref = F.leaky_relu(F.conv2d(cr, wr, br, padding=1), 0.01) + 2.0 * cr
    gy = _rand(ref.shape, 4)
    ref.backward(gy)
    ud, wd, bd = _dev(u, dev, grad=True), _dev(w, dev, grad=True), _dev(b, dev, grad=True)
    cd = ud[:, :64]
    y = ops.conv2d(cd, wd, bd, act=1, res=cd, res_scale=2.0)
    _close(y, ref, 2e-5, "slice+res fwd")
    y.backward(_dev(gy, dev))
    _close(ud.grad, ur.grad, 1e-4, "slice+res dgrad")
    _close(wd.grad, wr.grad, 1e-4, "slice+res wgrad")

    # subpel conv: 3x3 conv + PixelShuffle(2) fused in the store
    w2 = _rand((4 * 32, 128, 3, 3), 5, 0.03)
    b2 = _rand((4 * 32,), 6, 0.1)
    x2 = _rand((2, 128, 16, 16), 7)
    xr2, wr2, br2 = x2.clone().requires_grad_(), w2.clone().requires_grad_(), b2.clone().requires_grad_()
    ref2 = F.pixel_shuffle(F.conv2d(xr2, wr2, br2, padding=1), 2)
    gy2 = _rand(ref2.shape, 8)
    ref2.backward(gy2)
    xd2, wd2, bd2 = _dev(x2, dev, grad=True), _dev(w2, dev, grad=True), _dev(b2, dev, grad=True)
    y2 = ops.conv2d(xd2, wd2, bd2, shuffle=True)
    _close(y2, ref2, 2e-5, "subpel fwd")
    y2.backward(_dev(gy2, dev))
    _close(xd2.grad, xr2.grad, 1e-4, "subpel dgrad")
    _close(wd2.grad, wr2.grad, 1e-4, "subpel wgrad")
    _close(bd2.grad, br2.grad, 1e-4, "subpel bgrad")


def test_conv_batch_invariance_and_determinism(dev):
    """Encoder/decoder agreement needs bitwise identical results for an image regardless of batch size / tile config."""
    from clc_amd import ops

    x = _rand((8, 448, 16, 16), 1)
    w = _rand((224, 448, 3, 3), 2, 0.02)
    xd, wd = _dev(x, dev), _dev(w, dev)
    with torch.no_grad():
        y8 = ops.conv2d(xd, wd, None)
        y1 = ops.conv2d(xd[3:4].contiguous(memory_format=CL), wd, None)
        y8b = ops.conv2d(xd, wd, None)
    assert torch.equal(y8[3:4], y1), "result depends on the batch size"
    assert torch.equal(y8, y8b), "not run-to-run deterministic"


@pytest.mark.parametrize("inverse", [False, True])
def test_gdn(dev, inverse):
    from clc_amd import ops
    from oracle.leaves import GDN

    C = 128
    m = GDN(C, inverse=inverse)
    with torch.no_grad():
        m.gamma.add_(0.02 * torch.rand(C, C, generator=torch.Generator().manual_seed(1)))
    x = _rand((2, C, 16, 16), 2).requires_grad_()
    res = _rand((2, C, 16, 16), 5)
    ref = m(x) + res
    gy = _rand(ref.shape, 3)
    ref.backward(gy)
    beta_eff = m.beta_reparam(m.beta).detach()
    gamma_eff = m.gamma_reparam(m.gamma).detach()
    # reference grads w.r.t. the effective (re-parametrised) tensors
    be, ge = beta_eff.clone().requires_grad_(), gamma_eff.clone().requires_grad_()
    x2 = x.detach().clone().requires_grad_()
    norm = F.conv2d(x2 ** 2, ge.reshape(C, C, 1, 1), be)
    r2 = x2 * (torch.sqrt(norm) if inverse else torch.rsqrt(norm)) + res
    r2.backward(gy)
    xd = _dev(x.detach(), dev, grad=True)
    gd, bd = _dev(gamma_eff, dev, grad=True), _dev(beta_eff, dev, grad=True)
    y = ops.gdn(xd, gd, bd, inverse=inverse, res=_dev(res, dev))
    _close(y, ref, 2e-5, "gdn fwd")
    y.backward(_dev(gy, dev))
    _close(xd.grad, x2.grad, 1e-4, "gdn dx")
    _close(gd.grad, ge.grad, 1e-4, "gdn dgamma")
    _close(bd.grad, be.grad, 1e-4, "gdn dbeta")


@pytest.mark.parametrize("C", [64, 128])
def test_layernorm(dev, C):
    from clc_amd import ops

    x = _rand((2, C, 16, 24), 1, 2.0).requires_grad_()
    g = (1 + 0.1 * _rand((C,), 2)).requires_grad_()
    b = (0.1 * _rand((C,), 3)).requires_grad_()
    ref = F.layer_norm(x.permute(0, 2, 3, 1), (C,), g, b).permute(0, 3, 1, 2)
    gy = _rand(ref.shape, 4)
    ref.backward(gy)
    xd, gd, bd = _dev(x.detach(), dev, grad=True), _dev(g.detach(), dev, grad=True), _dev(b.detach(), dev, grad=True)
    y = ops.layernorm(xd, gd, bd)
    _close(y, ref, 2e-5, "ln fwd")
    y.backward(_dev(gy, dev))
    _close(xd.grad, x.grad, 1e-4, "ln dx")
    _close(gd.grad, g.grad, 1e-4, "ln dgamma")
    _close(bd.grad, b.grad, 1e-4, "ln dbeta")


def _ref_wmsa_core(qkv_nchw, relbias, heads, ws, shift):
    """attention core of the oracle WMSA (no projections) on [N,3C,H,W]."""
    from oracle.graph import WMSA

    N, C3, H, W = qkv_nchw.shape
    C = C3 // 3
    m = WMSA(C, C, C // heads, ws, "SW" if shift else "W")
    del m.relative_position_params
    m.relative_position_params = relbias  # plain tensor so that autograd reaches the caller's leaf
    x = qkv_nchw.permute(0, 2, 3, 1)
    sh = ws // 2
    if shift:
        x = torch.roll(x, shifts=(-sh, -sh), dims=(1, 2))
    hw, ww = H // ws, W // ws
    xw = x.reshape(N, hw, ws, ww, ws, C3).permute(0, 1, 3, 2, 4, 5).reshape(N, hw * ww, ws * ws, C3)
    hd = C // heads
    qkv = xw.reshape(N, hw * ww, ws * ws, 3 * heads, hd).permute(3, 0, 1, 2, 4)
    q, k, v = qkv[:heads], qkv[heads:2 * heads], qkv[2 * heads:]
    sim = torch.matmul(q, k.transpose(-1, -2)) * hd ** -0.5 + m.rel_bias()[:, None, None]
    if shift:
        sim = sim.masked_fill(m.shift_mask(hw, ww)[None, None], float("-inf"))
    out = torch.matmul(torch.softmax(sim, -1), v).permute(1, 2, 3, 0, 4).reshape(N, hw * ww, ws * ws, C)
    out = out.reshape(N, hw, ww, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(N, H, W, C)
    if shift:
        out = torch.roll(out, shifts=(sh, sh), dims=(1, 2))
    return out.permute(0, 3, 1, 2)


@pytest.mark.parametrize("cfg", [(64, 8, 8, 32, 32), (64, 4, 8, 16, 24), (64, 2, 8, 16, 16), (128, 8, 8, 16, 16), (64, 2, 4, 8, 8), (64, 2, 4, 8, 16), (64, 2, 4, 8, 12)])
@pytest.mark.parametrize("shift", [False, True])
def test_window_attention(dev, cfg, shift):
    from clc_amd import ops

    C, heads, ws, H, W = cfg
    N = 2
    qkv = _rand((N, 3 * C, H, W), 1).requires_grad_()
    rb = _rand((heads, 2 * ws - 1, 2 * ws - 1), 2, 0.5).requires_grad_()
    ref = _ref_wmsa_core(qkv, rb, heads, ws, shift)
    gy = _rand(ref.shape, 3)
    ref.backward(gy)
    qd, rd = _dev(qkv.detach(), dev, grad=True), _dev(rb.detach(), dev, grad=True)
    y = ops.window_attention(qd, rd, heads, ws, shift)
    _close(y, ref, 2e-5, "attn fwd")
    y.backward(_dev(gy, dev))
    _close(qd.grad, qkv.grad, 1e-4, "attn dqkv")
    _close(rd.grad, rb.grad, 1e-4, "attn drelbias")



# 3x3 window grids (the per-image maps of a 384x384 / 384x640 image, which a 128-multiple pad with an odd block count gives) at batch 1 and 3:
# (C, heads, ws, H, W) = slice SWAtten (inter_dim 128, head_dim 16; the NH-per-workgroup forward kernel), the hyper ConvTransBlocks at N = 64
# and N = 128, and the 24x40 latent of 384x640
@pytest.mark.parametrize("cfg", [(128, 8, 8, 24, 24), (64, 2, 4, 12, 12), (128, 4, 4, 12, 12), (128, 8, 8, 24, 40)])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("shift", [False, True])
def test_window_attention_odd_grids_vs_fp64(dev, cfg, N, shift):
    from clc_amd import ops

    C, heads, ws, H, W = cfg
    qkv = _rand((N, 3 * C, H, W), 21 + N)
    rb = _rand((heads, 2 * ws - 1, 2 * ws - 1), 22, 0.5)
    gy = _rand((N, C, H, W), 23)
    qr, rr = qkv.double().requires_grad_(), rb.double().requires_grad_()
    ref = _ref_wmsa_core(qr, rr, heads, ws, shift)
    ref.backward(gy.double())
    qd, rd = _dev(qkv, dev, grad=True), _dev(rb, dev, grad=True)
    y = ops.window_attention(qd, rd, heads, ws, shift)
    _close(y, ref, 2e-5, "attn fwd")
    y.backward(_dev(gy, dev))
    _close(qd.grad, qr.grad, 1e-4, "attn dqkv")
    _close(rd.grad, rr.grad, 1e-4, "attn drelbias")


def _is_64x64_tile(v):
    """kernel-variant id of clc_conv2d's 64x64 tiles on 4 waves (conv_igemm_kernel / conv_igemm_dma2_kernel<64, 64, 2, 2, ...>)"""
    return (v >> 20) in (1, 4) and (v & 0xFFFFF) == (2 << 16) | (2 << 12) | (64 << 3) | (64 >> 5)


@pytest.mark.parametrize("cin", [320, 576])
@pytest.mark.parametrize("act", [0, 3])
def test_unpaired_slice_net_convs_at_24x24_vs_fp64(dev, cin, act):
    """The slice nets' 3x3 layers (cin -> 224 -> 128 -> 64) as the unpaired route launches them for one 384x384 image: a 24x24 map, 576 rows
    (not a multiple of 128, so no filter-set pairing), above the split-K family's 256-pixel threshold.  Forward, data and filter gradients
    against fp64.  An eval (no_grad) forward must take the 64x64 tiles — or, for the few-channel layers that tuning keys 4 / 5 route there
    by the per-image map, the split-K family; a recorded one may take the Winograd kernel only where wino_ok says so, and otherwise gives
    the eval forward's bits."""
    from clc_amd import ops

    H = W = 24
    L = ops._L()
    splitk_pix, splitk_maxc = max(L.clc_get_tuning(4), 256), L.clc_get_tuning(5)

    def family_ok(v, cout):   # clc_conv2d's rule for a per-image map of 257..1024 pixels (csrc/conv_igemm.hip)
        if H * W <= splitk_pix and cout <= splitk_maxc:
            return v >> 20 == 3
        return _is_64x64_tile(v)

    for li, (ci, co) in enumerate(((cin, 224), (224, 128), (128, 64))):
        seed = 100 * li + cin + act
        x = _rand((1, ci, H, W), seed)
        w = _rand((co, ci, 3, 3), seed + 1, (1.0 / (ci * 9)) ** 0.5)
        b = _rand((co,), seed + 2, 0.1)
        gy = _rand((1, co, H, W), seed + 3)
        xr, wr, br = (t.double().requires_grad_() for t in (x, w, b))
        ref = F.conv2d(xr, wr, br, padding=1)
        ref = F.gelu(ref) if act == 3 else ref
        ref.backward(gy.double())
        xd, wd, bd = _dev(x, dev, grad=True), _dev(w, dev, grad=True), _dev(b, dev, grad=True)
        ops.PROFILE = []
        try:
            with torch.no_grad():
                y_eval = ops.conv2d(xd, wd, bd, act=act)
            y = ops.conv2d(xd, wd, bd, act=act)
            n_fwd = len(ops.PROFILE)
            y.backward(_dev(gy, dev))
            ops.flush_wgrads()
            torch.cuda.synchronize()
            recs = list(ops.PROFILE)
        finally:
            ops.PROFILE = None
        what = f"{ci}->{co} act {act}"
        fwd = [r.variant for r in recs[:n_fwd] if r.fam == "conv_igemm"]
        dgrad = [r.variant for r in recs[n_fwd:] if r.fam == "conv_igemm"]
        assert len(fwd) == 2 and len(dgrad) == 1, (what, [(r.fam, hex(r.variant)) for r in recs])
        assert family_ok(fwd[0], co), (what, "eval forward", hex(fwd[0]))
        if ops.wino_ok(1, H, W, ci, co, 3, 1):
            assert fwd[1] >> 20 == 13, (what, "recorded forward", hex(fwd[1]))
        else:
            assert family_ok(fwd[1], co), (what, "recorded forward", hex(fwd[1]))
            assert torch.equal(y.detach(), y_eval), what
        assert family_ok(dgrad[0], ci), (what, "data gradient", hex(dgrad[0]))
        _close(y_eval, ref, 2e-5, f"{what} eval fwd")
        _close(y, ref, 2e-5, f"{what} fwd")
        _close(xd.grad, xr.grad, 1e-4, f"{what} dgrad")
        _close(wd.grad, wr.grad, 1e-4, f"{what} wgrad")
        _close(bd.grad, br.grad, 1e-4, f"{what} bgrad")


def test_gate(dev):
    from clc_amd import ops

    a, b, i = (_rand((2, 128, 16, 16), s).requires_grad_() for s in (1, 2, 3))
    ref = a * torch.sigmoid(b) + i
    gy = _rand(ref.shape, 4)
    ref.backward(gy)
    ad, bd, idd = (_dev(t.detach(), dev, grad=True) for t in (a, b, i))
    y = ops.gate(ad, bd, idd)
    _close(y, ref, 1e-6, "gate fwd")
    y.backward(_dev(gy, dev))
    _close(ad.grad, a.grad, 1e-5, "gate da")
    _close(bd.grad, b.grad, 1e-5, "gate db")
    _close(idd.grad, i.grad, 1e-6, "gate didn")


@pytest.mark.parametrize("training", [False, True])
def test_gaussian_likelihood(dev, training):
    from clc_amd import ops
    from oracle.leaves import GaussianConditional

    gc = GaussianConditional(None)
    y = _rand((2, 64, 16, 16), 1, 3.0).requires_grad_()
    mu = _rand((2, 64, 16, 16), 2, 1.0).requires_grad_()
    sc = (_rand((2, 64, 16, 16), 3, 1.0) + 0.5).requires_grad_()  # some below the 0.11 bound, some negative
    noise = torch.rand((2, 64, 16, 16), generator=torch.Generator().manual_seed(4)) - 0.5
    if training:
        lik = gc._likelihood(y + noise, sc, mu)
    else:
        lik = gc._likelihood(torch.round(y - mu) + mu, sc, mu)
    lik = gc.likelihood_lower_bound(lik)
    w = torch.rand(lik.shape, generator=torch.Generator().manual_seed(5)) - 0.7  # mixed-sign upstream grads (LowerBound rule)
    (lik * w).sum().backward()
    yd, md, sd = (_dev(t.detach(), dev, grad=True) for t in (y, mu, sc))
    l2, y_hat = ops.gaussian_likelihood(yd, sd, md, _dev(noise, dev) if training else None, training)
    _close(l2, lik, 1e-5, "gauss lik")
    assert torch.equal(y_hat.cpu(), (torch.round(y - mu) + mu).detach()), "ste-rounded y_hat"
    # relative check in log domain for the tails
    assert (torch.log(l2.cpu()) - torch.log(lik.detach())).abs().max() < 2e-3
    (l2 * _dev(w, dev)).sum().backward()
    _close(sd.grad, sc.grad, 2e-4, "gauss dscale")
    if training:
        _close(yd.grad, y.grad, 2e-4, "gauss dy")
        _close(md.grad, mu.grad, 2e-4, "gauss dmu")
    else:
        assert yd.grad is None or float(yd.grad.abs().max()) == 0.0


@pytest.mark.parametrize("training", [False, True])
def test_entropy_bottleneck_likelihood(dev, training):
    from clc_amd import ops
    from oracle.leaves import EntropyBottleneck
    from oracle.recipe import apply_weight_recipe

    C = 192
    eb = EntropyBottleneck(C)
    apply_weight_recipe(eb, 3)
    eb.train(training)
    z = _rand((8, C, 4, 4), 1, 2.0).requires_grad_()
    noise = torch.rand(z.shape, generator=torch.Generator().manual_seed(4)) - 0.5
    med = eb._get_medians().reshape(1, C, 1, 1)
    v = z + noise if training else torch.round(z - med) + med
    vv = v.permute(1, 0, 2, 3).reshape(C, 1, -1)
    lik = eb.likelihood_lower_bound(eb._likelihood(vv)).reshape(C, 8, 4, 4).permute(1, 0, 2, 3)
    w = torch.rand(lik.shape, generator=torch.Generator().manual_seed(5)) - 0.3
    (lik * w).sum().backward()
    mats = [getattr(eb, f"_matrix{k}") for k in range(5)]
    biases = [getattr(eb, f"_bias{k}") for k in range(5)]
    factors = [getattr(eb, f"_factor{k}") for k in range(4)]
    md, bd, fd = ([_dev(t.detach(), dev, cl=False, grad=True) for t in ts] for ts in (mats, biases, factors))
    zd = _dev(z.detach(), dev, grad=True)
    qd = _dev(eb.quantiles.detach(), dev, cl=False)
    l2, z_hat = ops.eb_likelihood(zd, _dev(noise, dev) if training else None, qd, training, md, bd, fd)
    _close(l2, lik, 1e-5, "eb lik")
    assert torch.equal(z_hat.cpu(), (torch.round(z - med) + med).detach()), "ste-rounded z_hat"
    (l2 * _dev(w, dev)).sum().backward()
    for k in range(5):
        _close(md[k].grad, mats[k].grad, 2e-4, f"eb dmatrix{k}")
        _close(bd[k].grad, biases[k].grad, 2e-4, f"eb dbias{k}")
    for k in range(4):
        _close(fd[k].grad, factors[k].grad, 2e-4, f"eb dfactor{k}")
    if training:
        _close(zd.grad, z.grad, 2e-4, "eb dz")
    # aux loss
    eb.zero_grad()
    aux = eb.loss()
    aux.backward()
    qg = _dev(eb.quantiles.detach(), dev, cl=False, grad=True)
    a2 = ops.eb_aux_loss(qg, _dev(eb.target, dev, cl=False), md, bd, fd)
    _close(a2, aux, 1e-5, "eb aux")
    a2.backward()
    _close(qg.grad, eb.quantiles.grad, 1e-4, "eb dquantiles")


def test_quantize_build_indexes_bit_exact(dev):
    from clc_amd import ops
    from oracle.leaves import GaussianConditional, get_scale_table

    gc = GaussianConditional(None)
    gc.scale_table = get_scale_table()
    y = _rand((1, 64, 16, 16), 1, 4.0)
    mu = _rand((1, 64, 16, 16), 2, 1.0)
    sc = torch.exp(_rand((1, 64, 16, 16), 3, 2.0))
    sc.view(-1)[:64] = gc.scale_table  # exactly on the thresholds
    sc.view(-1)[64:70] = torch.tensor([0.0, -1.0, 0.11, 0.10999, 256.0, 1e4])
    sym_ref = gc.quantize(y, "symbols", mu)
    idx_ref = gc.build_indexes(sc)
    sym, idx, y_hat = ops.quantize_build_indexes(_dev(y, dev), _dev(mu, dev), _dev(sc, dev), gc.scale_table.to(dev))
    assert torch.equal(sym.cpu(), sym_ref), "symbols differ"
    assert torch.equal(idx.cpu(), idx_ref), "indexes differ"
    assert torch.equal(y_hat.cpu(), sym_ref.float() + mu)


@pytest.mark.parametrize("shape", [(2, 3, 256, 256), (1, 3, 256, 384)])
def test_ms_ssim_fwd_bwd(dev, shape):
    """HIP MS-SSIM (5 scales, 11-tap Gaussian) vs the oracle's plain-PyTorch restatement of pytorch_msssim.ms_ssim."""
    from clc_amd import ops
    from oracle.loss import ms_ssim as ms_ssim_ref
    from oracle.recipe import synthetic_image

    B, C, H, W = shape
    y = synthetic_image(B, H, W, 5, smooth=True)
    x = (y + 0.05 * _rand(shape, 6)).clamp(0, 1).requires_grad_()
    ref = ms_ssim_ref(x, y, data_range=1.0)
    ref.backward()
    xd = _dev(x.detach(), dev, grad=True)
    out = ops.ms_ssim(xd, _dev(y, dev), data_range=1.0)
    assert abs(out.item() - ref.item()) < 2e-5, (out.item(), ref.item())
    out.backward()
    _close(xd.grad, x.grad, 2e-3, "ms-ssim dx")


@pytest.mark.parametrize("cout", [64, 128])
def test_rgb_head_block_patch_rows(dev, cout):
    """ResidualBlockWithStride(3, C) — the RGB heads g_a.0 / ref_encoder.encoder.0 — runs conv1 (3x3/s2) and the skip conv
    (1x1/s2) as 1x1 convolutions over zero-padded 27->32 patch rows (clc_im2col_small): forward and every parameter
    gradient against the plain-PyTorch block (oracle leaves)."""
    from clc_amd import layers
    from oracle import leaves as ol

    torch.manual_seed(3)
    ref = ol.ResidualBlockWithStride(3, cout, stride=2)
    blk = layers.ResidualBlockWithStride(3, cout, stride=2)
    blk.load_state_dict(ref.state_dict())
    blk = blk.to(dev)
    x = torch.rand(2, 3, 64, 96, generator=torch.Generator().manual_seed(5))
    y_ref = ref(x)
    g = _rand(y_ref.shape, 7)
    y_ref.backward(g)
    y = blk(_dev(x, dev))
    y.backward(_dev(g, dev))
    _close(y, y_ref, 2e-5, "rgb head fwd")
    for (n, p), (_, q) in zip(blk.named_parameters(), ref.named_parameters()):
        _close(p.grad, q.grad, 1e-4, f"rgb head grad {n}")
    # the no-grad path (compress / decompress) gives the same bits
    with torch.no_grad():
        assert torch.equal(blk(_dev(x, dev)), y.detach())


def test_layernorm_and_attention_paired_modules(dev):
    """Paired form (second half of the batch on a second module's parameters, one launch): LayerNorm and window attention,
    forward and every gradient, against the two single-module launches — bit for bit forward, 1e-6 on parameter gradients
    (different partial-sum grouping)."""
    from clc_amd import ops

    C, heads, ws = 128, 8, 8
    x = _dev(_rand((4, C, 16, 16), 1), dev, grad=True)
    g1, b1, g2, b2 = (_dev(_rand((C,), s) * 0.3 + (1.0 if s % 2 else 0.0), dev, grad=True) for s in (2, 3, 4, 5))
    gy = _dev(_rand((4, C, 16, 16), 6), dev)
    y = ops.layernorm(x, g1, b1, None, None, g2, b2)
    y.backward(gy)
    got = [t.grad.clone() for t in (x, g1, b1, g2, b2)]
    for t in (x, g1, b1, g2, b2):
        t.grad = None
    ya, yb = ops.layernorm(x[:2], g1, b1), ops.layernorm(x[2:], g2, b2)
    assert torch.equal(y, torch.cat((ya, yb), 0))
    torch.cat((ya, yb), 0).backward(gy)
    for a, t, n in zip(got, (x, g1, b1, g2, b2), ("dx", "dgamma", "dbeta", "dgamma2", "dbeta2")):
        _close(a, t.grad, 1e-6, f"paired LN {n}")

    qkv = _dev(_rand((4, 3 * C, 16, 16), 7, 0.5), dev, grad=True)
    r1, r2 = (_dev(_rand((heads, 2 * ws - 1, 2 * ws - 1), s, 0.2), dev, grad=True) for s in (8, 9))
    go = _dev(_rand((4, C, 16, 16), 10), dev)
    for shift in (False, True):
        for t in (qkv, r1, r2):
            t.grad = None
        o = ops.window_attention(qkv, r1, heads, ws, shift, relbias2=r2)
        o.backward(go)
        got = [t.grad.clone() for t in (qkv, r1, r2)]
        for t in (qkv, r1, r2):
            t.grad = None
        oa, ob = ops.window_attention(qkv[:2], r1, heads, ws, shift), ops.window_attention(qkv[2:], r2, heads, ws, shift)
        assert torch.equal(o, torch.cat((oa, ob), 0))
        torch.cat((oa, ob), 0).backward(go)
        for a, t, n in zip(got, (qkv, r1, r2), ("dqkv", "drelbias", "drelbias2")):
            _close(a, t.grad, 1e-6, f"paired attention {n} shift={shift}")


# ------------------------------------------------------------------------- blocks against the GENUINE reference classes
# tests/golden/blocks.npz holds outputs of the reference's own WMSA / Block / ConvTransBlock / SWAtten classes
# (/root/reference/models/CLC_run.py:108-244, generated by tools/make_golden.py through tools/ref_shim.py): here the HIP
# modules meet them directly, not via the oracle.


def _golden_blocks():
    import os

    import numpy as np

    return np.load(os.path.join(os.path.dirname(__file__), "golden", "blocks.npz"))


@pytest.mark.parametrize("typ", ["W", "SW"])
@pytest.mark.parametrize("cfg", [(64, 8, 8, 16, 24), (64, 32, 4, 8, 8), (128, 16, 8, 16, 16)])
def test_wmsa_and_block_vs_reference_golden(dev, typ, cfg):
    from clc_amd import layers
    from clc_amd.recipe import apply_weight_recipe

    g = _golden_blocks()
    C, hd, ws, H, W = cfg
    tag = f"{typ}_{C}_{hd}_{ws}_{H}x{W}"
    x = torch.from_numpy(g[f"wmsa_{tag}_x"])                     # [2, H, W, C] tokens (the reference's b h w c layout)
    xd = _dev(x.permute(0, 3, 1, 2), dev)                         # logical NCHW, channels_last = the same bytes
    msa = layers.WMSA(C, C, hd, ws, typ)
    apply_weight_recipe(msa, 1)
    blk = layers.Block(C, C, hd, ws, 0, typ)
    apply_weight_recipe(blk, 2)
    with torch.no_grad():
        ym = msa.to(dev)(xd).permute(0, 2, 3, 1).cpu()
        yb = blk.to(dev)(xd).permute(0, 2, 3, 1).cpu()
    _close(ym, torch.from_numpy(g[f"wmsa_{tag}_y"]), 2e-5, f"WMSA {tag} vs reference class")
    _close(yb, torch.from_numpy(g[f"block_{tag}_y"]), 2e-5, f"Block {tag} vs reference class")


@pytest.mark.parametrize("typ", ["W", "SW"])
def test_block_fused_large_map_path_vs_reference_class(dev, typ):
    """The launches that carry the Swin blocks of the 128 x 128 maps — ln1 + qkv (`clc_lnlin_*`), MFMA window attention, the wave-private
    1x1 kernel (projection), LayerNorm + MLP in one launch (`clc_mlp_*`) — against numbers produced by the reference's OWN Block class
    (CLC_run.py:172-193) at M = 2 x 128 x 128 = 32 768 tokens, the size from which they switch on (tests/golden/block_large.npz,
    tools/make_golden.py block_large): output, input gradient and all 13 parameter gradients under a seeded dy."""
    import hashlib

    from clc_amd import layers, ops
    from clc_amd.recipe import apply_weight_recipe

    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "block_large.npz"))
    shape = g["shape"].tolist()
    x0 = torch.randn(*shape, generator=torch.Generator().manual_seed(int(g["seed_x"])))
    dy0 = torch.randn(*shape, generator=torch.Generator().manual_seed(int(g["seed_dy"])))
    assert hashlib.sha256(x0.numpy().tobytes()).hexdigest() == str(g["x_sha256"]) and hashlib.sha256(dy0.numpy().tobytes()).hexdigest() == str(g["dy_sha256"])
    blk = layers.Block(64, 64, 8, 8, 0, typ)
    apply_weight_recipe(blk, 2)
    blk = blk.to(dev).train()
    x = _dev(x0.permute(0, 3, 1, 2), dev, grad=True)              # tokens [b, h, w, c] = the bytes of a channels_last NCHW tensor
    dy = _dev(dy0.permute(0, 3, 1, 2), dev)
    assert ops.lnlin_fusable(x, blk.msa.embedding_layer.weight) and ops.mlp_ln_fusable(x, blk.mlp[0].weight, blk.mlp[2].weight)
    ops.PROFILE = []
    try:
        y = blk(x)
        y.backward(dy)
        ops.join_side_streams()
        torch.cuda.synchronize()
        launched = {r.fam for r in ops.PROFILE}
    finally:
        ops.PROFILE = None
    for name in ("clc_lnlin_fwd", "clc_lnlin_bwd", "clc_mlp_fwd", "clc_mlp_bwd"):
        assert name in launched, (name, sorted(launched))        # the fused launches are what ran
    yt, dxt = y.detach().permute(0, 2, 3, 1).cpu(), x.grad.permute(0, 2, 3, 1).cpu()
    for k, (b, r, c) in enumerate(g["patch_origins"].tolist()):
        _close(yt[b, r:r + 8, c:c + 8], torch.from_numpy(g[f"{typ}_y_patch{k}"]), 2e-5, f"Block {typ} y patch {k} vs reference class")
        _close(dxt[b, r:r + 8, c:c + 8], torch.from_numpy(g[f"{typ}_dx_patch{k}"]), 1e-4, f"Block {typ} dx patch {k} vs reference class")
    for nm, t, tol in (("y", yt, 2e-5), ("dx", dxt, 1e-4)):
        _close(t.double().sum(dim=(1, 2)), torch.from_numpy(g[f"{typ}_{nm}_row_sums"]), tol, f"Block {typ} {nm} per-channel sums")
        assert abs(t.double().abs().sum().item() - float(g[f"{typ}_{nm}_abs_sum"])) <= tol * float(g[f"{typ}_{nm}_abs_sum"])
    for n, q in blk.named_parameters():
        assert q.grad is not None, n
        _close(q.grad.cpu(), torch.from_numpy(g[f"{typ}_grad_{n}"]), 1e-4, f"Block {typ} d{n} vs reference class")


def test_convtransblock_large_map_path_vs_reference_class(dev):
    """A whole ConvTransBlock on a [2, 128, 128, 128] input (32 768 pixels: conv1_1 / conv1_2 on the wave-private 1x1 kernel, the ResidualBlock's
    64-channel 3x3 layers on the LDS-tiled kernels with their activation gates and gradient folds, the Swin Block on its fused launches, the two
    branches written / differentiated in place through channel halves) against numbers produced by the reference's OWN ConvTransBlock class
    (CLC_run.py:195-220; tests/golden/block_large.npz ctb_*, tools/make_golden.py block_large): output, input gradient, 21 parameter gradients."""
    import hashlib

    from clc_amd import layers, ops
    from clc_amd.recipe import apply_weight_recipe

    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "block_large.npz"))
    x0 = torch.randn(2, 128, 128, 128, generator=torch.Generator().manual_seed(int(g["ctb_seed_x"])))
    dy0 = torch.randn(2, 128, 128, 128, generator=torch.Generator().manual_seed(int(g["ctb_seed_dy"])))
    assert hashlib.sha256(x0.numpy().tobytes()).hexdigest() == str(g["ctb_x_sha256"])
    ctb = layers.ConvTransBlock(64, 64, 8, 8, 0, "SW")
    apply_weight_recipe(ctb, 3)
    ctb = ctb.to(dev).train()
    x, dy = _dev(x0, dev, grad=True), _dev(dy0, dev)
    ops.PROFILE = []
    try:
        y = ctb(x)
        y.backward(dy)
        ops.join_side_streams()
        torch.cuda.synchronize()
        fams = {(r.fam, r.variant >> 20) for r in ops.PROFILE}
    finally:
        ops.PROFILE = None
    assert ("conv_igemm", 11) in fams, sorted(fams)                                   # conv1_1 / conv1_2: lin_kernel (family 11)
    assert {"clc_lnlin_fwd", "clc_mlp_bwd"} <= {f for f, _ in fams}                   # the Swin Block's fused launches
    yt, dxt = y.detach().cpu(), x.grad.cpu()
    for k, (b, r, c) in enumerate(g["patch_origins"].tolist()):
        _close(yt[b, :, r:r + 8, c:c + 8], torch.from_numpy(g[f"ctb_y_patch{k}"]), 2e-5, f"ConvTransBlock y patch {k} vs reference class")
        _close(dxt[b, :, r:r + 8, c:c + 8], torch.from_numpy(g[f"ctb_dx_patch{k}"]), 1e-4, f"ConvTransBlock dx patch {k} vs reference class")
    for nm, t, tol in (("y", yt, 2e-5), ("dx", dxt, 1e-4)):
        _close(t.double().sum(dim=(2, 3)), torch.from_numpy(g[f"ctb_{nm}_chan_sums"]), tol, f"ConvTransBlock {nm} per-channel sums")
        assert abs(t.double().abs().sum().item() - float(g[f"ctb_{nm}_abs_sum"])) <= tol * float(g[f"ctb_{nm}_abs_sum"])
    for n, q in ctb.named_parameters():
        assert q.grad is not None, n
        _close(q.grad.cpu(), torch.from_numpy(g[f"ctb_grad_{n}"]), 1e-4, f"ConvTransBlock d{n} vs reference class")


def test_convtransblock_and_swatten_vs_reference_golden(dev):
    from clc_amd import layers
    from clc_amd.recipe import apply_weight_recipe

    g = _golden_blocks()
    ctb = layers.ConvTransBlock(64, 64, 16, 8, 0, "SW")
    apply_weight_recipe(ctb, 3)
    swa = layers.SWAtten(384, 384, 16, 8, 0, inter_dim=128)
    apply_weight_recipe(swa, 4)
    with torch.no_grad():
        yc = ctb.to(dev)(_dev(torch.from_numpy(g["ctb_x"]), dev)).cpu()
        ys = swa.to(dev)(_dev(torch.from_numpy(g["swatten_x"]), dev)).cpu()
    _close(yc, torch.from_numpy(g["ctb_y"]), 2e-5, "ConvTransBlock vs reference class")
    _close(ys, torch.from_numpy(g["swatten_y"]), 2e-5, "SWAtten vs reference class")


def test_dormant_clm_and_fusion_vs_reference_golden(dev):
    """the modules the reference constructs and never calls (in-file CLM, multi_ref_fusion; CLC_run.py:284-313,
    359-369) on the HIP path against outputs of the genuine classes (tests/golden/dormant.npz)."""
    import os

    import numpy as np

    from clc_amd.models import clc as pm
    from clc_amd.recipe import apply_weight_recipe

    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "dormant.npz"))
    clm = pm.CLM(192, head_dim=32, window_size=4)
    apply_weight_recipe(clm, 5)
    fus = pm.PointwiseMLP(384, 256, 192)
    apply_weight_recipe(fus, 6)
    x, r = _dev(torch.from_numpy(g["x"]), dev), _dev(torch.from_numpy(g["ref"]), dev)
    with torch.no_grad():
        a = clm.to(dev)(x, r)
        f = fus.to(dev)(torch.cat([x, a], dim=1))
    _close(a.cpu(), torch.from_numpy(g["clm_y"]), 2e-5, "CLM vs reference class")
    _close(f.cpu(), torch.from_numpy(g["fusion_y"]), 2e-5, "multi_ref_fusion vs reference class")


@pytest.mark.parametrize("kind", ["lrelu3x3", "relu1x1", "gelu_linear", "subpel_lrelu", "big_lrelu"])
def test_activation_gate_in_consumer_dgrad(dev, kind):
    """ops.ActGate: z = conv_b(act(conv_a(x))) — conv_b's data-gradient epilogue multiplies by act'(.), conv_a's gradient kernels then
    run without an operand prologue.  Every gradient against plain torch autograd, and bit-identical forward with / without gates."""
    from clc_amd import ops

    if kind == "big_lrelu":
        N, C, H, W = 4, 64, 128, 128     # conv_a's data gradient on the 128-row LDS-DMA tile
    else:
        N, C, H, W = 2, 64, 32, 32
    act = {"lrelu3x3": 1, "relu1x1": 2, "gelu_linear": 3, "subpel_lrelu": 1, "big_lrelu": 1}[kind]
    ks = 1 if kind in ("relu1x1", "gelu_linear") else 3
    shuffle = kind == "subpel_lrelu"
    Ca = 4 * C if shuffle else C
    x = _rand((N, C, H, W), 1)
    wa = _rand((Ca, C, ks, ks), 2, (1.0 / (C * ks * ks)) ** 0.5)
    ba = _rand((Ca,), 3, 0.1)
    wb = _rand((96, C, 3, 3), 4, (1.0 / (C * 9)) ** 0.5)
    bb = _rand((96,), 5, 0.1)
    # the kernel's own activated output decides which side of 0 a pre-activation of ~1e-8 falls on (see test_conv_fwd_bwd) — of a RECORDED
    # forward like the ones below (a no_grad forward may run another kernel: the Winograd forms serve recorded passes only)
    ya_gpu = ops.conv2d(_dev(x, dev, grad=True), _dev(wa, dev, grad=True), _dev(ba, dev, grad=True), act=act, shuffle=shuffle).detach().cpu()
    ref_in = [t.clone().requires_grad_() for t in (x, wa, ba, wb, bb)]
    t = F.conv2d(ref_in[0], ref_in[1], ref_in[2], padding=ks // 2)
    if shuffle:
        t = F.pixel_shuffle(t, 2)
    a = {1: lambda v: torch.where(ya_gpu > 0, v, 0.01 * v), 2: lambda v: torch.where(ya_gpu > 0, v, 0.0 * v), 3: F.gelu}[act](t)
    ref = F.conv2d(a, ref_in[3], ref_in[4], padding=1)
    gy = _rand(ref.shape, 6)
    ref.backward(gy)
    outs = {}
    for gated in (True, False):
        d = [_dev(t_, dev, grad=True) for t_ in (x, wa, ba, wb, bb)]
        g = ops.ActGate() if gated else None
        ya = ops.conv2d(d[0], d[1], d[2], act=act, shuffle=shuffle, gate_out=g)
        y = ops.conv2d(ya, d[3], d[4], gate_in=g)
        y.backward(_dev(gy, dev))
        assert (g.done if gated else True)
        outs[gated] = (y.detach(), [t_.grad for t_ in d])
        _close(y, ref, 3e-5, f"{kind} fwd")
        for name, got, want in zip(("dx", "dwa", "dba", "dwb", "dbb"), outs[gated][1], [r.grad for r in ref_in]):
            _close(got, want, 2e-4, f"{kind} gated={gated} {name}")
    assert torch.equal(outs[True][0], outs[False][0])


@pytest.mark.parametrize("case", [(8, 128, 32, 32, 512, True), (8, 320, 16, 16, 512, False), (2, 128, 32, 32, 512, True)])
def test_dgrad_k_split_matches_unsplit(dev, case):
    """Round 3: a 3x3 data gradient whose 64x64-tile grid would leave most CUs with one workgroup (few output channels, long K) splits
    its K range over 2-4 workgroups per tile (partials to a scratch buffer, fixed-order finish launch with the ordinary epilogue).
    Same values as the unsplit launch up to fp32 summation order, with the epilogue operands (folded residual gradient + the producer's
    activation-derivative gate) applied once; run-to-run bit-identical; and a torch reference of the plain transposed convolution."""
    from clc_amd import lib as _clib
    from clc_amd import ops

    N, Cin, H, W, Cout, with_epi = case
    g = torch.Generator().manual_seed(3)
    dy = torch.randn(N, Cout, H, W, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) * 0.05).to(dev).contiguous(memory_format=torch.channels_last)
    res = torch.randn(N, Cin, H, W, generator=g).to(dev).contiguous(memory_format=torch.channels_last) if with_epi else None
    gate = torch.randn(N, Cin, H, W, generator=g).to(dev).contiguous(memory_format=torch.channels_last) if with_epi else None
    wt = ops.filter_transpose(w, Cout, 9, Cin).view(Cin, -1)
    L = _clib.load()

    def run():
        return ops.conv_raw(dy, wt, None, ks=3, pad=1, transposed=True, out_hw=(H, W), res=res, res_scale=0.5,
                            out_gate=((gate, ops.ACT_LRELU, False) if with_epi else None))

    old = L.clc_set_tuning(11, 0)
    try:
        ref = run().clone()
        L.clc_set_tuning(11, 1)
        got, again = run().clone(), run().clone()
    finally:
        L.clc_set_tuning(11, old)
    assert torch.equal(got, again), "K-split data gradient is not reproducible"
    scale = ref.abs().max().item()
    assert (got - ref).abs().max().item() <= 2e-5 * scale
    want = torch.nn.functional.conv_transpose2d(dy.cpu().double(), w.cpu().double(), padding=1)
    if with_epi:
        want = (want + 0.5 * res.cpu().double()) * torch.where(gate.cpu().double() > 0, 1.0, 0.01)
    assert (got.cpu().double() - want).abs().max().item() <= 3e-5 * want.abs().max().item()


@pytest.mark.parametrize("sets,n", [(1, 1), (1, 3), (2, 4), (4, 8), (4, 32)])
def test_fused_residual_unit_matches_three_layers(dev, sets, n):
    """clc_residual_unit_fwd / clc_residual_unit_dgrad (csrc/fused_ru.hip: 1x1 -> 3x3 -> 1x1 + identity on 16x16 maps in one launch, and the
    whole data gradient in one more) vs torch fp32 layer by layer.  The gradient reference applies the ReLU masks of the kernel's OWN
    activations (a pre-activation within rounding of 0 may land on either side of the kink; the forward check bounds how far)."""
    import torch.nn.functional as F
    from torch.nn.grad import conv2d_weight
    from clc_amd import layers, ops

    torch.manual_seed(40 + sets)
    units = [layers.ResidualUnit(128).to(dev) for _ in range(sets)]
    x = torch.randn(n, 128, 16, 16, device=dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    pair = None if sets == 1 else (units[1] if sets == 2 else tuple(units[1:]))
    assert ops.residual_unit_fusable(x, units)
    y = units[0](x, pair=pair)
    gy = torch.randn_like(y)
    y.backward(gy)
    per = n // sets
    with torch.no_grad():
        t1, t2, y_again = ops.residual_unit_fwd_raw(x.detach(), [(u.conv[0].weight, u.conv[0].bias, u.conv[2].weight, u.conv[2].bias,
                                                                  u.conv[4].weight, u.conv[4].bias) for u in units])
        assert torch.equal(y_again, y)
        for k, u in enumerate(units):
            sl = slice(k * per, (k + 1) * per)
            c, xs = u.conv, x.detach()[sl]
            r1 = F.relu(F.conv2d(xs, c[0].weight, c[0].bias))
            r2 = F.relu(F.conv2d(r1, c[2].weight, c[2].bias, padding=1))
            ry = F.relu(F.conv2d(r2, c[4].weight, c[4].bias) + xs)
            for got, want in ((t1[sl], r1), (t2[sl], r2), (y[sl], ry)):
                assert (got - want).abs().max().item() <= 2e-5 * max(1.0, want.abs().max().item())
            g3 = gy[sl] * (y[sl] > 0)
            g2 = F.conv_transpose2d(g3, c[4].weight) * (t2[sl] > 0)
            g1 = F.conv_transpose2d(g2, c[2].weight, padding=1) * (t1[sl] > 0)
            dx = F.conv_transpose2d(g1, c[0].weight) + g3
            want = (conv2d_weight(xs, c[0].weight.shape, g1), g1.sum((0, 2, 3)), conv2d_weight(t1[sl], c[2].weight.shape, g2, padding=1), g2.sum((0, 2, 3)),
                    conv2d_weight(t2[sl], c[4].weight.shape, g3), g3.sum((0, 2, 3)))
            assert (x.grad[sl] - dx).abs().max().item() <= 1e-4 * max(1.0, dx.abs().max().item())
            for prm, w in zip(u.parameters(), want):
                assert (prm.grad - w).abs().max().item() <= 2e-4 * max(1.0, w.abs().max().item()), (k, tuple(prm.shape))
    # the unfused path gives the same result to rounding, and a result does not depend on the rest of the batch
    old = ops.FUSED_RU
    try:
        ops.FUSED_RU = 0
        with torch.no_grad():
            yu = units[0](x.detach(), pair=pair)
    finally:
        ops.FUSED_RU = old
    assert (y - yu).abs().max().item() <= 2e-5 * max(1.0, yu.abs().max().item())
    with torch.no_grad():
        y1 = units[0](x.detach()[:1].contiguous(memory_format=torch.channels_last))
    assert torch.equal(y1, y[:1].detach())


def test_window_attention_kernel_variants_agree(dev):
    """The round-3 variants of the 8x8-window kernels — 4-block MFMAs for the N = head_dim products (tuning key 16, bit mask) and the
    two-workgroups-per-window backward of small grids (key 18) — against the plain variants on the same inputs: same values to fp32
    summation order, forward, dqkv and the relative-bias gradient, for head_dim 8 and 16, shifted windows."""
    from clc_amd import lib as _clib
    from clc_amd import ops

    L = _clib.load()
    for C, heads in ((64, 8), (64, 4)):
        qkv = _dev(_rand((2, 3 * C, 32, 32), 11), dev, grad=True)
        rb = _dev(_rand((heads, 15, 15), 12, 0.5), dev, grad=True)
        gy = _dev(_rand((2, C, 32, 32), 13), dev)
        res = {}
        old16, old18 = L.clc_set_tuning(16, 0), L.clc_set_tuning(18, 0)
        try:
            for k16, k18 in ((0, 0), (7, 0), (7, 1), (0, 1)):
                L.clc_set_tuning(16, k16)
                L.clc_set_tuning(18, k18)
                y = ops.window_attention(qkv, rb, heads, 8, True)
                gq, gb = torch.autograd.grad(y, [qkv, rb], gy)
                res[(k16, k18)] = (y.detach().clone(), gq.clone(), gb.clone())
        finally:
            L.clc_set_tuning(16, old16)
            L.clc_set_tuning(18, old18)
        base = res[(0, 0)]
        for key, r in res.items():
            for name, a, b in zip(("fwd", "dqkv", "drelbias"), r, base):
                assert (a - b).abs().max().item() <= 2e-5 * max(1e-6, b.abs().max().item()), (C, heads, key, name)


def test_training_forward_long_k_layers_on_128x128_tiles(dev):
    """clc_conv_desc.batch_variant_ok (set for forward passes that record an autograd graph): the slice-parameter nets' long-K 3x3 layers
    leave the split-K family for 128x128 LDS tiles with a grid-sized K split (fixed-order finish launch: bias, activation, saved
    pre-activation, two filter sets).  Same values as the inference path to fp32 summation order and as torch; run-to-run bit-identical;
    the inference path (no grad) is untouched, so an image's bits there do not depend on the batch."""
    import torch.nn.functional as F
    from clc_amd import ops

    g = torch.Generator().manual_seed(21)
    x = (torch.randn(16, 640, 16, 16, generator=g) * 0.5).to(dev).contiguous(memory_format=torch.channels_last)
    w1 = (torch.randn(224, 640, 3, 3, generator=g) * 0.02).to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    w2 = (torch.randn(224, 640, 3, 3, generator=g) * 0.02).to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    b1, b2 = torch.randn(224, generator=g).to(dev).requires_grad_(True), torch.randn(224, generator=g).to(dev).requires_grad_(True)
    xg = x.clone().requires_grad_(True)
    y_train = ops.conv2d(xg, w1, b1, act=ops.ACT_LRELU, w2=w2, b2=b2)          # records a graph -> batch_variant_ok
    y_again = ops.conv2d(xg, w1, b1, act=ops.ACT_LRELU, w2=w2, b2=b2)
    with torch.no_grad():
        y_eval = ops.conv2d(x, w1, b1, act=ops.ACT_LRELU, w2=w2, b2=b2)         # the codec / eval path
        y_one = ops.conv2d(x[:2].contiguous(memory_format=torch.channels_last), w1, b1, act=ops.ACT_LRELU)
        want = torch.cat((F.leaky_relu(F.conv2d(x[:8], w1, b1, padding=1), 0.01), F.leaky_relu(F.conv2d(x[8:], w2, b2, padding=1), 0.01)))
    assert torch.equal(y_train, y_again)
    scale = want.abs().max().item()
    assert (y_train - want).abs().max().item() <= 3e-5 * scale and (y_eval - want).abs().max().item() <= 3e-5 * scale
    assert torch.equal(y_one, y_eval[:2])                                       # inference: batch-independent bits
    (y_train.square().sum()).backward()                                         # and the ordinary backward still runs on its outputs
    assert torch.isfinite(w1.grad).all() and torch.isfinite(xg.grad).all()


@pytest.mark.parametrize("save_h", [1, 0])
@pytest.mark.parametrize("N,H,W,strided", [(8, 64, 64, False), (2, 128, 128, True), (8, 128, 128, False), (1, 64, 96, True)])
def test_fused_mlp_same_bits_as_two_launches(dev, N, H, W, strided, save_h):
    """clc_mlp_fwd / clc_mlp_bwd (csrc/fused_mlp.hip: `x + fc2(gelu(fc1(LN x)))` of a Swin block in one launch, its data gradient with the
    hidden tensor recomputed in one more) against (a) the two-launch chain of 1x1 convolutions it replaces — THE SAME BITS forward, for
    dx, d(res) and all four parameter gradients — and (b) plain torch fp32.  2 / 4 / 8 waves per workgroup (6 144 .. 131 072 pixels), a
    destination and an incoming gradient that are channel ranges of wider buffers (ConvTransBlock's conv1_2 input)."""
    from clc_amd import layers, ops

    torch.manual_seed(7)
    fc1, fc2 = layers.Linear(64, 256).to(dev), layers.Linear(256, 64).to(dev)
    with torch.no_grad():
        fc1.bias.normal_(0, 0.3)
        fc2.bias.normal_(0, 0.3)
    x0 = (torch.randn(N, 64, H, W, device=dev) * 1.5).contiguous(memory_format=CL)
    r0 = torch.randn(N, 64, H, W, device=dev).contiguous(memory_format=CL)
    gy = torch.randn(N, 64, H, W, device=dev).contiguous(memory_format=CL)
    wide = torch.randn(N, 128, H, W, device=dev).contiguous(memory_format=CL)
    old_min, old_save = ops.FUSED_MLP_MIN_PIX, ops.MLP_SAVE_H
    ops.FUSED_MLP_MIN_PIX, ops.MLP_SAVE_H = 1024, save_h   # (save_h: fc1's pre-activation stored forward / recomputed backward)
    try:
        assert ops.mlp_fusable(x0, fc1.weight, fc2.weight)
        res = {}
        for mode in ("fused", "chain"):
            for prm in list(fc1.parameters()) + list(fc2.parameters()):
                prm.grad = None
            x, r = x0.clone().requires_grad_(True), r0.clone().requires_grad_(True)
            out = ops.new_act(N, 128, H, W, x0)[:, 64:] if strided else None
            if mode == "fused":
                y = ops.mlp(x, fc1.weight, fc1.bias, fc2.weight, fc2.bias, res=r, out=out)
            else:
                g = ops.ActGate()
                y = fc2(fc1(x, act=ops.ACT_GELU, gate_out=g), res=r, out=out, gate_in=g)
            dy = (wide[:, 64:] if strided else gy)
            y.backward(dy)
            torch.cuda.synchronize()
            res[mode] = (y.detach().clone(), x.grad.clone(), r.grad.clone(), [prm.grad.clone() for prm in list(fc1.parameters()) + list(fc2.parameters())])
    finally:
        ops.FUSED_MLP_MIN_PIX, ops.MLP_SAVE_H = old_min, old_save
    (yf, dxf, drf, pf), (yc, dxc, drc, pc) = res["fused"], res["chain"]
    assert torch.equal(yf, yc), f"forward differs from the two-launch chain: max {(yf - yc).abs().max().item():.3e}"
    assert torch.equal(dxf, dxc), f"dx differs: max {(dxf - dxc).abs().max().item():.3e}"
    assert torch.equal(drf, drc)
    for a, b, name in zip(pf, pc, ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias")):
        assert torch.equal(a, b), f"{name} gradient differs: max {(a - b).abs().max().item():.3e}"
    # plain torch fp32 on the same values
    with torch.no_grad():
        hp = F.conv2d(x0, fc1.weight[:, :, None, None], fc1.bias)
        want = F.conv2d(F.gelu(hp), fc2.weight[:, :, None, None], fc2.bias) + r0
    _close(yf, want, 2e-5, "fused mlp forward vs torch")
    xt = x0.clone().requires_grad_(True)
    yt = F.conv2d(F.gelu(F.conv2d(xt, fc1.weight.detach()[:, :, None, None], fc1.bias.detach())), fc2.weight.detach()[:, :, None, None], fc2.bias.detach())
    yt.backward(wide[:, 64:] if strided else gy)
    _close(dxf, xt.grad, 1e-4, "fused mlp dx vs torch")


@pytest.mark.parametrize("N,H,W,strided", [(8, 64, 64, False), (2, 128, 128, True), (8, 128, 128, False), (1, 64, 96, True), (3, 40, 56, False)])
def test_fused_mlp_with_layernorm_same_bits_as_separate_launches(dev, N, H, W, strided):
    """The LayerNorm form of clc_mlp_fwd / clc_mlp_bwd (`x + mlp(ln2(x))` from the block's raw input, /root/reference/models/CLC_run.py:183,192):
    LN in registers forward, its backward pass (+ the residual's gradient) in the data-gradient launch — against clc_layernorm_fwd / _bwd around
    the plain fused form: THE SAME BITS for y, dx and the four filter / bias gradients (the row sums follow the LayerNorm kernel's butterfly);
    dgamma / dbeta sum the same products over the pixels in another order -> fp32 accuracy.  And plain torch fp32."""
    from clc_amd import layers, ops

    torch.manual_seed(11)
    fc1, fc2, ln = layers.Linear(64, 256).to(dev), layers.Linear(256, 64).to(dev), layers.LayerNorm(64).to(dev)
    with torch.no_grad():
        fc1.bias.normal_(0, 0.3)
        fc2.bias.normal_(0, 0.3)
        ln.weight.normal_(1.0, 0.2)
        ln.bias.normal_(0, 0.2)
    prms = list(fc1.parameters()) + list(fc2.parameters()) + list(ln.parameters())
    x0 = (torch.randn(N, 64, H, W, device=dev) * 1.5 + 0.3).contiguous(memory_format=CL)
    gy = torch.randn(N, 64, H, W, device=dev).contiguous(memory_format=CL)
    wide = torch.randn(N, 128, H, W, device=dev).contiguous(memory_format=CL)
    old_min = ops.FUSED_MLP_MIN_PIX
    ops.FUSED_MLP_MIN_PIX = 1024
    try:
        assert ops.mlp_ln_fusable(x0, fc1.weight, fc2.weight)
        res = {}
        for mode in ("ln_fused", "separate"):
            for prm in prms:
                prm.grad = None
            x = x0.clone().requires_grad_(True)
            out = ops.new_act(N, 128, H, W, x0)[:, 64:] if strided else None
            if mode == "ln_fused":
                y = ops.mlp_ln(x, ln.weight, ln.bias, fc1.weight, fc1.bias, fc2.weight, fc2.bias, out=out)
            else:
                f2 = ops.GradFold()
                y = ops.mlp(ln(x, fold_in=f2), fc1.weight, fc1.bias, fc2.weight, fc2.bias, res=x, fold_out=f2, out=out)
            y.backward(wide[:, 64:] if strided else gy)
            torch.cuda.synchronize()
            res[mode] = (y.detach().clone(), x.grad.clone(), [prm.grad.clone() for prm in prms])
    finally:
        ops.FUSED_MLP_MIN_PIX = old_min
    (yf, dxf, pf), (yc, dxc, pc) = res["ln_fused"], res["separate"]
    assert torch.equal(yf, yc), f"forward differs from LayerNorm + fused MLP: max {(yf - yc).abs().max().item():.3e}"
    assert torch.equal(dxf, dxc), f"dx differs: max {(dxf - dxc).abs().max().item():.3e}"
    for a, b, name in zip(pf[:4], pc[:4], ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias")):
        assert torch.equal(a, b), f"{name} gradient differs: max {(a - b).abs().max().item():.3e}"
    _close(pf[4], pc[4], 2e-5, "ln.weight gradient vs the LayerNorm kernel")
    _close(pf[5], pc[5], 2e-5, "ln.bias gradient vs the LayerNorm kernel")
    xt = x0.clone().requires_grad_(True)
    lw, lb = ln.weight.detach().clone().requires_grad_(True), ln.bias.detach().clone().requires_grad_(True)
    t = F.layer_norm(xt.permute(0, 2, 3, 1), (64,), lw, lb, 1e-5).permute(0, 3, 1, 2)
    yt = xt + F.conv2d(F.gelu(F.conv2d(t, fc1.weight.detach()[:, :, None, None], fc1.bias.detach())), fc2.weight.detach()[:, :, None, None], fc2.bias.detach())
    yt.backward(wide[:, 64:] if strided else gy)
    _close(yf, yt.detach(), 2e-5, "ln-fused mlp forward vs torch")
    _close(dxf, xt.grad, 1e-4, "ln-fused mlp dx vs torch")
    _close(pf[4], lw.grad, 1e-4, "ln.weight gradient vs torch")
    _close(pf[5], lb.grad, 1e-4, "ln.bias gradient vs torch")


@pytest.mark.parametrize("N,H,W,typ,strided", [(8, 64, 64, "W", True), (2, 128, 128, "SW", True), (8, 128, 128, "W", False), (1, 64, 96, "SW", False)])
def test_swin_block_fused_launches_same_bits_as_separate(dev, N, H, W, typ, strided):
    """A whole Swin Block (/root/reference/models/CLC_run.py:172-193) on a large map with its fused launches — ln1 + qkv embedding
    (clc_lnlin_fwd / _bwd: LayerNorm, Linear(64 -> 192); backward: the embedding's data gradient, ln1's backward pass and the residual
    gradient) and ln2 + MLP (clc_mlp_*) — against the same Block on separate LayerNorm / 1x1 launches: THE SAME BITS for the output, the input
    gradient and every filter / bias / relative-position gradient; the LayerNorm parameter gradients (another summation order over the pixels)
    to fp32 accuracy.  Input and output as channel ranges of wider buffers (ConvTransBlock's layout)."""
    from clc_amd import layers, ops

    torch.manual_seed(5)
    blk = layers.Block(64, 64, 8, 8, 0.0, typ).to(dev)
    with torch.no_grad():
        for prm in blk.parameters():
            if prm.dim() == 1:
                prm.add_(torch.randn_like(prm) * 0.2)
    wide_x = (torch.randn(N, 128, H, W, device=dev) * 1.3).contiguous(memory_format=CL)
    x0 = wide_x[:, 64:] if strided else wide_x[:, :64].contiguous(memory_format=CL)
    gy = torch.randn(N, 64, H, W, device=dev).contiguous(memory_format=CL)
    names = [n for n, _ in blk.named_parameters()]
    old = (ops.FUSED_MLP_MIN_PIX, ops.FUSED_LNLIN, ops.FUSED_MLP_LN, ops.FUSED_MLP)
    ops.FUSED_MLP_MIN_PIX = 1024
    res = {}
    try:
        for mode in ("fused", "separate"):
            ops.FUSED_LNLIN = ops.FUSED_MLP_LN = ops.FUSED_MLP = 1 if mode == "fused" else 0
            if mode == "fused":
                assert ops.lnlin_fusable(x0, blk.msa.embedding_layer.weight)
            for prm in blk.parameters():
                prm.grad = None
            x = x0.detach().clone().requires_grad_(True) if not strided else wide_x.detach().clone().requires_grad_(True)
            xin = x[:, 64:] if strided else x
            out = ops.new_act(N, 128, H, W, x0)[:, 64:] if strided else None
            y = blk(xin, out=out)
            y.backward(gy)
            torch.cuda.synchronize()
            res[mode] = (y.detach().clone(), x.grad.clone(), [prm.grad.clone() for prm in blk.parameters()])
    finally:
        ops.FUSED_MLP_MIN_PIX, ops.FUSED_LNLIN, ops.FUSED_MLP_LN, ops.FUSED_MLP = old
    (yf, dxf, pf), (yc, dxc, pc) = res["fused"], res["separate"]
    assert torch.equal(yf, yc), f"block output differs: max {(yf - yc).abs().max().item():.3e}"
    assert torch.equal(dxf, dxc), f"input gradient differs: max {(dxf - dxc).abs().max().item():.3e}"
    for a, b, name in zip(pf, pc, names):
        if name.startswith("ln"):
            _close(a, b, 2e-5, f"{name} gradient vs the LayerNorm kernel")
        else:
            assert torch.equal(a, b), f"{name} gradient differs: max {(a - b).abs().max().item():.3e}"


@pytest.mark.parametrize("N,C,H,W,strided", [(8, 128, 64, 64, False), (2, 128, 128, 128, True), (8, 64, 64, 64, True), (2, 64, 128, 192, False), (8, 128, 128, 128, False)])
def test_wave_private_1x1_same_bits_as_tiled(dev, N, C, H, W, strided):
    """lin_kernel (csrc/fused_mlp.hip; tuning key 21): the 128 -> 128 / 64 -> 64 1x1 layers of the ConvTransBlocks (conv1_1, conv1_2, the
    attention's projection: /root/reference/models/CLC_run.py:205-206, 121) on >= 32 768 rows, forward with bias + residual and the data
    gradient with a folded residual gradient — THE SAME BITS as the tiled kernels it replaces (clc_conv2d may pick by the row count), and
    plain torch fp32.  Source / destination as channel ranges of wider buffers."""
    from clc_amd import layers, ops
    from clc_amd import lib as _clib

    L = _clib.load()
    torch.manual_seed(C + H)
    lin = layers.Linear(C, C).to(dev)
    with torch.no_grad():
        lin.bias.normal_(0, 0.3)
    wide = (torch.randn(N, 2 * C, H, W, device=dev)).contiguous(memory_format=CL)
    x0 = wide[:, C:] if strided else wide[:, :C].contiguous(memory_format=CL)
    r0 = torch.randn(N, C, H, W, device=dev).contiguous(memory_format=CL)
    gy = torch.randn(N, C, H, W, device=dev).contiguous(memory_format=CL)
    res = {}
    for key in (1, 0):
        prev = L.clc_set_tuning(21, key)
        try:
            for prm in lin.parameters():
                prm.grad = None
            x, r = x0.detach().clone().requires_grad_(True), r0.clone().requires_grad_(True)
            out = ops.new_act(N, 2 * C, H, W, x0)[:, C:] if strided else None
            y = lin(x, res=r, out=out)
            y.backward(gy)
            torch.cuda.synchronize()
            res[key] = (y.detach().clone(), x.grad.clone(), r.grad.clone(), lin.weight.grad.clone(), lin.bias.grad.clone())
        finally:
            L.clc_set_tuning(21, prev)
    for a, b, name in zip(res[1], res[0], ("y", "dx", "dres", "dW", "db")):
        assert torch.equal(a, b), f"{name} differs from the tiled kernels: max {(a - b).abs().max().item():.3e}"
    xt = x0.detach().clone().requires_grad_(True)
    yt = F.conv2d(xt, lin.weight.detach()[:, :, None, None], lin.bias.detach()) + r0
    yt.backward(gy)
    _close(res[1][0], yt.detach(), 2e-5, "1x1 forward vs torch")
    _close(res[1][1], xt.grad, 1e-4, "1x1 dx vs torch")


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("N,H,W", [(8, 64, 64), (2, 128, 128), (3, 96, 128)])
def test_gdn_backward_in_one_launch_same_bits(dev, N, H, W, inverse):
    """clc_gdn_bwd_fused (csrc/fused_mlp.hip: gdn_bwd_kernel): the data gradient of a 128-channel GDN / IGDN on a large map — the elementwise part,
    gamma^T dv and the combination in one launch, dx_direct never written — against clc_gdn_bwd_elem + the transposed 1x1 convolution with the
    MUL2 epilogue: THE SAME BITS for dx and for the gamma / beta gradients (whose filter gradient reads the dv it stores); and torch autograd on
    the CompressAI formula."""
    from clc_amd import layers, ops

    torch.manual_seed(17 + int(inverse))
    gdn = layers.GDN(128, inverse=inverse).to(dev)
    with torch.no_grad():
        gdn.gamma.add_(torch.rand_like(gdn.gamma) * 0.02)
        gdn.beta.add_(torch.rand_like(gdn.beta) * 0.3)
    x0 = torch.randn(N, 128, H, W, device=dev).contiguous(memory_format=CL)
    r0 = torch.randn(N, 128, H, W, device=dev).contiguous(memory_format=CL)
    gy = torch.randn(N, 128, H, W, device=dev).contiguous(memory_format=CL)
    res, old = {}, ops.FUSED_GDN_BWD
    try:
        for mode in (1, 0):
            ops.FUSED_GDN_BWD = mode
            gdn.gamma.grad = gdn.beta.grad = None
            x, r = x0.clone().requires_grad_(True), r0.clone().requires_grad_(True)
            y = gdn(x, res=r)
            y.backward(gy)
            torch.cuda.synchronize()
            res[mode] = (y.detach().clone(), x.grad.clone(), r.grad.clone(), gdn.gamma.grad.clone(), gdn.beta.grad.clone())
    finally:
        ops.FUSED_GDN_BWD = old
    for a, b, name in zip(res[1], res[0], ("y", "dx", "dres", "dgamma", "dbeta")):
        assert torch.equal(a, b), f"{name} differs from the two-launch path: max {(a - b).abs().max().item():.3e}"
    # the CompressAI formula in torch
    gb, bb, ped = gdn._consts()
    xt = x0.clone().requires_grad_(True)
    gam = (torch.clamp(gdn.gamma.detach(), min=gb) ** 2 - ped)
    bet = (torch.clamp(gdn.beta.detach(), min=bb) ** 2 - ped)
    norm = F.conv2d(xt * xt, gam[:, :, None, None], bet)
    yt = (xt * torch.sqrt(norm) if inverse else xt * torch.rsqrt(norm)) + r0
    yt.backward(gy)
    _close(res[1][0], yt.detach(), 2e-5, "gdn forward vs torch")
    _close(res[1][1], xt.grad, 1e-4, "gdn dx vs torch")


@pytest.mark.parametrize("N,Cin,H,W,Cout,shuffle", [(2, 128, 64, 64, 12, True), (1, 128, 40, 72, 12, True), (2, 64, 64, 48, 16, False), (3, 256, 48, 48, 12, True)])
def test_16_column_kernel_for_the_few_channel_tail(dev, N, Cin, H, W, Cout, shuffle):
    """conv_igemm_n16_kernel (v_mfma_f32_16x16x4_f32, 256 x 16 tiles; tuning key 20): the synthesis transform's subpel tail, 128 -> 12 with the
    PixelShuffle(2) store (CLC_run.py:351) — vs torch fp32, vs the 32-column kernel it replaces (another summation order: fp32 accuracy,
    not bits), ragged row counts, and batch-independence of an image's bits (the kernel is chosen by the layer's shape alone)."""
    from clc_amd import lib as _clib
    from clc_amd import ops

    L = _clib.load()
    g = torch.Generator().manual_seed(Cin + Cout + H)
    x = _dev(torch.randn(N, Cin, H, W, generator=g), dev)
    w = _dev(torch.randn(Cout, Cin, 3, 3, generator=g) * 0.05, dev)
    b = torch.randn(Cout, generator=g).to(dev)
    outs = {}
    for key in (0, 1):
        prev = L.clc_set_tuning(20, key)
        try:
            outs[key] = ops.conv_raw(x, ops.to_kernel_weight(w), b, ks=3, shuffle=shuffle).clone()
            if key == 1:
                one = ops.conv_raw(x[:1].contiguous(memory_format=CL), ops.to_kernel_weight(w), b, ks=3, shuffle=shuffle).clone()
        finally:
            L.clc_set_tuning(20, prev)
    with torch.no_grad():
        want = F.conv2d(x, w, b, padding=1)
        if shuffle:
            want = F.pixel_shuffle(want, 2)
    assert outs[1].shape == want.shape
    _close(outs[1], want, 2e-5, "n16 kernel vs torch")
    _close(outs[1], outs[0], 4e-6, "n16 kernel vs the 32-column kernel")
    assert torch.equal(one, outs[1][:1]), "an image's bits depend on the batch"


@pytest.mark.parametrize("N,H,W,Cin,Cout,mode", [
    (8, 64, 64, 128, 128, "plain"), (2, 128, 128, 128, 128, "lrelu_res"), (8, 32, 32, 128, 512, "shuffle_lrelu"), (2, 64, 64, 128, 512, "shuffle"),
    (8, 64, 64, 128, 128, "dgrad_gate"), (12, 40, 48, 128, 128, "plain"), (1, 256, 256, 128, 128, "pre"), (8, 128, 128, 128, 128, "plain"),
    (8, 128, 128, 64, 64, "plain"), (2, 128, 128, 64, 64, "lrelu_res"), (8, 128, 128, 64, 64, "dgrad_gate"), (3, 72, 80, 64, 128, "pre"), (8, 64, 64, 64, 64, "strided")])
def test_halo_conv_same_bits_as_tiled(dev, N, H, W, Cin, Cout, mode):
    """conv_halo3x3_kernel (csrc/conv_halo.hip: 3x3 / stride 1 / 128 or 64 input channels; input halo resident in LDS, filter streamed from L2 in
    fragment order, no barrier in the K loop) against the LDS-tiled kernels on the same launch: THE SAME BITS — forward with bias /
    LeakyReLU / residual / saved pre-activation epilogues, the PixelShuffle store of the sub-pixel convolutions
    (/root/reference/models/CLC_run.py:28-30 via compressai.layers.subpel_conv3x3), the data gradient with the consumer-side activation
    gate, input and output as channel ranges of wider buffers (ConvTransBlock's halves); image borders, maps that are not powers of
    two, a workgroup that walks several tiles."""
    from clc_amd import lib, ops
    from clc_amd.ops import ACT_LRELU, ACT_NONE

    L = lib.load()
    restore = L.clc_set_tuning(22, 3)     # (the 64-channel instantiation is off by default: slower inside the step)
    try:
        _halo_case(dev, L, ops, N, H, W, Cin, Cout, mode, ACT_LRELU)
    finally:
        L.clc_set_tuning(22, restore)


def _halo_case(dev, L, ops, N, H, W, Cin, Cout, mode, ACT_LRELU):
    g = torch.Generator().manual_seed(N * 1000 + H + Cout)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) * 0.05).to(dev).contiguous(memory_format=CL)
    b = (torch.randn(Cout, generator=g) * 0.1).to(dev)
    wk = ops.to_kernel_weight(w)
    kw = dict(ks=3, stride=1)
    tr = mode.startswith("dgrad")
    if tr:   # "x" is dY [N, Cout, H, W]; the launch's K channels = Cout, its rows = Cin
        x = _dev(torch.randn(N, Cout, H, W, generator=g), dev)
        assert ops.halo_ok(N, H, W, Cout, Cin, 3, 1) == Cout
        wt = ops.filter_transpose(wk, Cout, 9, Cin).view(Cin, -1)
        pk = ops.halo_pack(wt, Cin, Cout)
        gate = _dev(torch.randn(N, Cin, H, W, generator=g), dev)
        run = lambda wpk: ops.conv_raw(x, wt, None, ks=3, stride=1, pad=1, transposed=True, out_hw=(H, W), out_gate=(gate, ACT_LRELU, False),
                                       res=_dev(torch.ones(N, Cin, H, W), dev), res_scale=0.25, wpk=wpk)
    else:
        wide = _dev(torch.randn(N, 2 * Cin, H, W, generator=g), dev)
        x = wide[:, Cin:] if mode == "strided" else _dev(torch.randn(N, Cin, H, W, generator=g), dev)
        assert ops.halo_ok(N, H, W, Cin, Cout, 3, 1) == Cin
        if mode in ("plain", "strided"):
            kw.update(bias=b)
        elif mode == "lrelu_res":
            kw.update(bias=b, act=ACT_LRELU, res=_dev(torch.randn(N, Cout, H, W, generator=g), dev), res_scale=0.5)
        elif mode == "pre":
            kw.update(bias=b, act=ACT_LRELU, res=_dev(torch.randn(N, Cout, H, W, generator=g), dev), y_pre=ops.new_act(N, Cout, H, W, x))
        elif mode == "shuffle_lrelu":
            kw.update(bias=b, act=ACT_LRELU, shuffle=True)
        elif mode == "shuffle":
            kw.update(bias=b, shuffle=True)
        outw = ops.new_act(N, 2 * Cout, H, W, wide) if mode == "strided" else None
        run = lambda wpk: ops.conv_raw(x, wk, kw.get("bias"), **{k: v for k, v in kw.items() if k != "bias"}, wpk=wpk,
                                       out=(outw[:, :Cout] if outw is not None else None))
        pk = ops.halo_pack(wk, Cout, Cin)
    ops.PROFILE = []
    try:
        y_halo = run(pk).clone()
        pre_halo = kw["y_pre"].clone() if "y_pre" in kw else None
        y_tiled = run(None).clone()
        torch.cuda.synchronize()
        variants = [r.variant >> 20 for r in ops.PROFILE if r.fam == "conv_igemm"]
    finally:
        ops.PROFILE = None
    assert variants[0] == 12 and variants[1] != 12, variants          # the halo kernel ran, then a tiled one
    assert torch.equal(y_halo, y_tiled), f"max diff {(y_halo - y_tiled).abs().max().item():.3e}"
    if pre_halo is not None:
        assert torch.equal(pre_halo, kw["y_pre"])
    # ... and against torch for the plain forward (the tiled kernels are held to torch by test_conv_fwd_bwd)
    if mode == "plain":
        ref = F.conv2d(x.cpu(), w.cpu(), b.cpu(), padding=1)
        _close(y_halo, ref, 2e-5, f"halo conv {N}x{H}x{W} {Cin} -> {Cout}")
    # the tuning key switches it off
    old = L.clc_set_tuning(22, 0)
    try:
        ops.PROFILE = []
        run(pk)
        assert (ops.PROFILE[0].variant >> 20) != 12
    finally:
        ops.PROFILE = None
        L.clc_set_tuning(22, old)
    assert L.clc_set_tuning(22, 1) == 3     # the default mask: 128-channel layers only
    assert ops.halo_ok(8, 64, 64, 64, 64, 3, 1) == 0 and ops.halo_ok(8, 64, 64, 128, 128, 3, 1) == 128
    L.clc_set_tuning(22, 3)


@pytest.mark.parametrize("rows,K", [(128, 128), (512, 128), (64, 64), (192, 64)])
def test_halo_filter_pack_is_the_documented_fragment_order(dev, rows, K):
    """clc_filter_pack_halo against its layout statement (include/clc_hip.h, csrc/conv_halo.hip): element (n-tile, wave column wc, K step kt, block j,
    quarter t8, lane) x 4 floats = filter row nt * 64 NWC + wc * 64 + j * 32 + (lane & 31), tap kt / (K / 32), channels (kt % (K / 32)) * 32 + 8 t8 +
    4 (lane >> 5) .. + 3 — i.e. what lane (n, k-half) of a v_mfma_f32_32x32x2_f32 B operand needs for MFMA steps ss = 0..3 of that quarter."""
    from clc_amd import ops

    w = torch.arange(rows * 9 * K, dtype=torch.float32).reshape(rows, 9 * K).to(dev)      # every element its own value: a pure permutation check
    pk = ops.halo_pack(w, rows, K).cpu().numpy().reshape(-1, 4)
    KCN, NWC = K // 32, K // 64
    KST = 9 * KCN
    e = np.arange(pk.shape[0])
    lane, r = e & 63, e >> 6
    t8, r = r & 3, r >> 2
    j, r = r & 1, r >> 1
    kt, r = r % KST, r // KST
    wc, nt = r % NWC, r // NWC
    row = nt * 64 * NWC + wc * 64 + j * 32 + (lane & 31)
    k0 = (kt % KCN) * 32 + 8 * t8 + 4 * (lane >> 5)
    src = (row * 9 + kt // KCN) * K + k0
    want = src[:, None] + np.arange(4)[None, :]
    assert pk.shape[0] == rows * 9 * K // 4 and np.array_equal(pk, want.astype(np.float32))
    assert np.array_equal(np.sort(pk.reshape(-1)), np.arange(rows * 9 * K, dtype=np.float32))    # a permutation: nothing dropped, nothing twice


@pytest.mark.parametrize("N,H,W,Cin,Cout,mode", [
    (8, 64, 64, 128, 128, "plain"), (2, 128, 128, 128, 128, "lrelu_res"), (8, 32, 32, 128, 512, "shuffle_lrelu"), (2, 64, 64, 128, 512, "shuffle"),
    (8, 64, 64, 128, 128, "dgrad_gate"), (3, 48, 96, 128, 128, "plain"), (1, 256, 256, 128, 128, "pre"), (2, 64, 64, 256, 128, "plain"),
    (2, 64, 64, 128, 512, "dgrad_gate"), (3, 72, 80, 128, 128, "strided"), (1, 64, 128, 128, 128, "plain"),
    (8, 128, 128, 64, 64, "plain"), (2, 128, 128, 64, 64, "lrelu_res"), (2, 128, 128, 64, 64, "dgrad_gate"), (2, 64, 64, 64, 256, "shuffle_lrelu"),
    (1, 128, 128, 64, 64, "pre"), (3, 72, 80, 64, 128, "strided"), (2, 64, 128, 192, 64, "plain"), (2, 64, 128, 64, 192, "dgrad_gate"),
    (8, 32, 32, 320, 320, "plain"), (8, 32, 32, 320, 320, "dgrad_gate"), (8, 64, 64, 64, 64, "lrelu_res")])
def test_wino_conv_vs_direct_and_fp64(dev, N, H, W, Cin, Cout, mode):
    """conv_wino_kernel (csrc/conv_wino.hip: Winograd F(2x2, 3x3) for 3x3 / stride-1 layers with 128 k channels; input transform B^T d B from an
    LDS-resident halo, 16 batched MFMA GEMMs against the pre-transformed filter U = G g G^T, output transform A^T M A through LDS into the
    shared epilogues) on the launches the training step gives it — forward with bias / LeakyReLU / residual / saved pre-activation, the
    PixelShuffle store of the sub-pixel convolutions (/root/reference/models/CLC_run.py:28-30), the data gradient with the consumer-side
    activation gate and a 512-channel K range, channel ranges of wider buffers, image borders, non-power-of-two maps.  ANOTHER summation
    order than the direct kernels, so not their bits: held to an fp64 convolution at least as tightly as the direct kernel is (both errors
    printed), and to the direct kernel within 4e-6 of the largest output."""
    from clc_amd import lib, ops
    from clc_amd.ops import ACT_LRELU

    L = lib.load()
    restore = L.clc_set_tuning(23, 7)     # (bit 2: the 64-wide instantiation for layers of 64 k channels)
    try:
        g = torch.Generator().manual_seed(N * 1000 + H + Cout)
        w = (torch.randn(Cout, Cin, 3, 3, generator=g) * 0.05).to(dev).contiguous(memory_format=CL)
        b = (torch.randn(Cout, generator=g) * 0.1).to(dev)
        wk = ops.to_kernel_weight(w)
        kw = dict(ks=3, stride=1)
        tr = mode.startswith("dgrad")
        if tr:   # "x" is dY [N, Cout, H, W]; the launch's K channels = Cout, its rows = Cin
            x = _dev(torch.randn(N, Cout, H, W, generator=g), dev)
            assert ops.wino_ok(N, H, W, Cout, Cin, 3, 1, transposed=True)
            wt = ops.filter_transpose(wk, Cout, 9, Cin).view(Cin, -1)
            u = ops.wino_pack(wt, Cin, Cout, flip=True)
            gate = _dev(torch.randn(N, Cin, H, W, generator=g), dev)
            res = _dev(torch.randn(N, Cin, H, W, generator=g), dev)
            run = lambda wwino: ops.conv_raw(x, wt, None, ks=3, stride=1, pad=1, transposed=True, out_hw=(H, W), out_gate=(gate, ACT_LRELU, False),
                                             res=res, res_scale=0.25, wwino=wwino)
            ref = F.conv_transpose2d(x.double().cpu(), w.double().cpu(), padding=1)
            gc = gate.double().cpu()
            ref = (ref + 0.25 * res.double().cpu()) * torch.where(gc > 0, 1.0, 0.01)     # out_gate: the WHOLE result times act'(saved)
        else:
            wide = _dev(torch.randn(N, 2 * Cin, H, W, generator=g), dev)
            x = wide[:, Cin:] if mode == "strided" else _dev(torch.randn(N, Cin, H, W, generator=g), dev)
            assert ops.wino_ok(N, H, W, Cin, Cout, 3, 1)
            ref = F.conv2d(x.double().cpu(), w.double().cpu(), b.double().cpu(), padding=1)
            if mode in ("plain", "strided"):
                kw.update(bias=b)
            elif mode in ("lrelu_res", "pre"):
                r = _dev(torch.randn(N, Cout, H, W, generator=g), dev)
                kw.update(bias=b, act=ACT_LRELU, res=r, res_scale=0.5)
                if mode == "pre":
                    kw.update(y_pre=ops.new_act(N, Cout, H, W, x))
                pre_ref = ref
                ref = F.leaky_relu(ref, 0.01) + 0.5 * r.double().cpu()
            elif mode == "shuffle_lrelu":
                kw.update(bias=b, act=ACT_LRELU, shuffle=True)
                ref = F.pixel_shuffle(F.leaky_relu(ref, 0.01), 2)
            elif mode == "shuffle":
                kw.update(bias=b, shuffle=True)
                ref = F.pixel_shuffle(ref, 2)
            outw = ops.new_act(N, 2 * Cout, H, W, wide) if mode == "strided" else None
            run = lambda wwino: ops.conv_raw(x, wk, kw.get("bias"), **{k: v for k, v in kw.items() if k != "bias"}, wwino=wwino,
                                             out=(outw[:, :Cout] if outw is not None else None))
            u = ops.wino_pack(wk, Cout, Cin)
        ops.PROFILE = []
        try:
            y_w = run(u).clone()
            pre_w = kw["y_pre"].clone() if "y_pre" in kw else None
            y_d = run(None).clone()
            torch.cuda.synchronize()
            full = [r.variant for r in ops.PROFILE if r.fam == "conv_igemm"]
            variants = [v >> 20 for v in full]
        finally:
            ops.PROFILE = None
        assert variants[0] == 13 and variants[1] != 13, variants          # the Winograd kernel ran, then a direct one
        rows_out = Cin if tr else Cout          # the launch's output channels
        wide = Cin % 128 == 0 and Cout % 128 == 0 and N * (H // 8) * (W // 16) * (rows_out // 128) >= 192
        assert ((full[0] >> 12) & 1) == (0 if wide else 1), hex(full[0])   # which instantiation: 128-wide from 192 items up, else the 64-wide one
        scale = ref.abs().max().item()
        e_w = (y_w.double().cpu() - ref).abs().max().item() / scale
        e_d = (y_d.double().cpu() - ref).abs().max().item() / scale
        print(f"wino {N}x{H}x{W} {Cin}->{Cout} {mode}: err vs fp64 winograd {e_w:.2e} direct {e_d:.2e}")
        assert e_w < 3e-6 and e_w < 1.5 * e_d + 2e-7, (e_w, e_d)
        assert (y_w - y_d).abs().max().item() / scale < 4e-6
        if pre_w is not None:
            assert (pre_w.double().cpu() - pre_ref).abs().max().item() / pre_ref.abs().max().item() < 3e-6
        # (which kernel a launch takes depends on its item count, i.e. on the batch: allowed, because these kernels serve recorded — training —
        #  passes only; test_wino_forward_is_training_only holds that line)
        # the tuning key switches it off (bit 0: forward launches, bit 1: data gradients)
        L.clc_set_tuning(23, 1 if tr else 2)
        ops.PROFILE = []
        try:
            y_off = run(u).clone()
            assert (ops.PROFILE[0].variant >> 20) != 13
        finally:
            ops.PROFILE = None
        assert torch.equal(y_off, y_d)
    finally:
        L.clc_set_tuning(23, restore)


def test_wino_forward_is_training_only(dev):
    """The Winograd kernel's bits are not the direct kernels': it may serve a recorded (training) forward and the data gradients, never an eval /
    no_grad forward — the parity measurement, the codec and `model.forward` under no_grad keep their bits whatever tuning key 23 says."""
    from clc_amd import lib, ops

    L = lib.load()
    g = torch.Generator().manual_seed(5)
    x = _dev(torch.randn(2, 128, 64, 64, generator=g), dev).requires_grad_(True)
    w = torch.nn.Parameter((torch.randn(128, 128, 3, 3, generator=g) * 0.05).to(dev).contiguous(memory_format=CL))
    b = torch.nn.Parameter(torch.zeros(128, device=dev))

    def fams(fn):
        ops.PROFILE = []
        try:
            y = fn()
            torch.cuda.synchronize()
            return y, [r.variant >> 20 for r in ops.PROFILE if r.fam == "conv_igemm"]
        finally:
            ops.PROFILE = None

    restore = L.clc_set_tuning(23, 7)
    try:
        with torch.no_grad():
            y_eval, v = fams(lambda: ops.conv2d(x, w, b))
        assert 13 not in v, v
        y_tr, v = fams(lambda: ops.conv2d(x, w, b))
        assert v == [13], v
        L.clc_set_tuning(23, 0)
        with torch.no_grad():
            y_off, _ = fams(lambda: ops.conv2d(x, w, b))
        assert torch.equal(y_eval, y_off)
        assert (y_tr - y_eval).abs().max().item() / y_eval.abs().max().item() < 4e-6
        L.clc_set_tuning(23, 7)
        _, v = fams(lambda: y_tr.square().sum().backward())
        ops.flush_wgrads()
        assert 13 in v, v       # the data gradient took it too
        assert x.grad is not None and torch.isfinite(x.grad).all()
    finally:
        L.clc_set_tuning(23, restore)


@pytest.mark.parametrize("N,H,W,Cin,Cout,ks,bias", [(2, 64, 64, 128, 128, 3, True), (2, 128, 128, 64, 64, 3, False), (4, 32, 32, 128, 512, 3, True),
                                                    (8, 128, 128, 128, 128, 1, True), (8, 32, 32, 320, 320, 3, False), (8, 16, 16, 640, 224, 3, True), (2, 64, 64, 96, 160, 3, True)])
def test_split_wgrad_has_the_f32_kernels_accuracy(dev, N, H, W, Cin, Cout, ks, bias):
    """Tuning key 24: the LDS-DMA-staged filter-gradient kernels form their f32 products from three-way bf16 splits (v = h + m + l exactly; the six
    largest of the nine piece products, six v_mfma_f32_32x32x16_bf16, f32 accumulate: csrc/conv_wgrad.hip split3) instead of v_mfma_f32_32x32x2_f32 —
    the bf16 matrix cores run at 16x the f32 rate.  NOT a reduced-precision mode: held here to an fp64 filter gradient as tightly as the native f32
    kernels (error <= 1.25x theirs + 5e-8 of the largest element; measured 0.8x .. 1.15x), all-taps and tiled kernels (the 64 x 64 tiles keep the f32 MFMAs:
    VALU-bound in this form), bias sums, ragged channel counts."""
    from clc_amd import lib, ops

    L = lib.load()
    g = torch.Generator().manual_seed(N + H + Cin + ks)
    x = _dev(torch.randn(N, Cin, H, W, generator=g), dev)
    dy = _dev(torch.randn(N, Cout, H, W, generator=g), dev)
    ref = torch.nn.grad.conv2d_weight(x.double().cpu(), (Cout, Cin, ks, ks), dy.double().cpu(), padding=ks // 2).permute(0, 2, 3, 1).reshape(Cout, -1)
    ref_b = dy.double().cpu().sum((0, 2, 3))
    out = {}
    for mode in (0, 3):
        old = L.clc_set_tuning(24, mode)
        try:
            dw = torch.zeros(Cout * ks * ks * Cin, device=dev)
            db = torch.zeros(Cout, device=dev) if bias else None
            keep = ops.wgrad_batched([dict(x=x, dy=dy, ks=ks, stride=1, pad=ks // 2, Cout=Cout, Cin=Cin, want_bias=bias, dw_out=dw, db_out=db, accumulate=0)])
            torch.cuda.synchronize()
            out[mode] = (dw.double().cpu().view(Cout, -1), db.double().cpu() if bias else None)
        finally:
            L.clc_set_tuning(24, old)
    scale = ref.abs().max().item()
    e_native = (out[0][0] - ref).abs().max().item() / scale
    e_split = (out[3][0] - ref).abs().max().item() / scale
    print(f"wgrad {Cin}->{Cout} k{ks} {N}x{H}x{W}: err vs fp64 native {e_native:.2e} split {e_split:.2e}")
    assert e_split <= 1.25 * e_native + 5e-8, (e_split, e_native)
    assert e_split < 2e-6
    assert not torch.equal(out[0][0], out[3][0])       # (the split kernels did run: another summation path)
    if bias:
        assert torch.equal(out[0][1], out[3][1])       # the bias sums are untouched by the mode
        assert (out[3][1] - ref_b).abs().max().item() / ref_b.abs().max().item() < 1e-5
