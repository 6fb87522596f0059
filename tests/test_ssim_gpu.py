"""HIP SSIM / MS-SSIM on any image size, window and input gradient (clc_amd.ssim, clc_amd.ops.ms_ssim, clc_ssim_desc_*).

References: the oracle's plain-PyTorch restatement of pytorch_msssim.ms_ssim (default window, any side) and, for what it does not
cover (other windows, `K`, `weights`, `ssim`, `nonnegative_ssim`, `size_average=False`, gradients of both inputs), the float64
restatement below."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CL = torch.channels_last
WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


# ----------------------------------------------------------------------------- float64 restatement of pytorch_msssim (2-D)


def _win64(ws, sigma):
    c = torch.arange(ws, dtype=torch.float64) - ws // 2
    g = torch.exp(-(c ** 2) / (2 * sigma ** 2))
    return g / g.sum()


def _filt64(x, w):
    C_ = x.shape[1]
    x = F.conv2d(x, w.view(1, 1, -1, 1).repeat(C_, 1, 1, 1), groups=C_)
    return F.conv2d(x, w.view(1, 1, 1, -1).repeat(C_, 1, 1, 1), groups=C_)


def _ssim64(X, Y, w, data_range, K):
    C1, C2 = (K[0] * data_range) ** 2, (K[1] * data_range) ** 2
    mu1, mu2 = _filt64(X, w), _filt64(Y, w)
    s11 = _filt64(X * X, w) - mu1 * mu1
    s22 = _filt64(Y * Y, w) - mu2 * mu2
    s12 = _filt64(X * Y, w) - mu1 * mu2
    cs_map = (2 * s12 + C2) / (s11 + s22 + C2)
    ssim_map = ((2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1)) * cs_map
    return ssim_map.flatten(2).mean(-1), cs_map.flatten(2).mean(-1)


def ref_ssim(X, Y, data_range=255, size_average=True, w=None, K=(0.01, 0.03), nonnegative_ssim=False):
    s, _ = _ssim64(X.double(), Y.double(), _win64(11, 1.5) if w is None else w.double(), data_range, K)
    if nonnegative_ssim:
        s = torch.relu(s)
    return s.mean() if size_average else s.mean(1)


def ref_ms_ssim(X, Y, data_range=255, size_average=True, w=None, weights=WEIGHTS, K=(0.01, 0.03)):
    X, Y = X.double(), Y.double()
    w = _win64(11, 1.5) if w is None else w.double()
    mcs = []
    for i in range(len(weights)):
        s, cs = _ssim64(X, Y, w, data_range, K)
        if i < len(weights) - 1:
            mcs.append(torch.relu(cs))
            pad = [v % 2 for v in X.shape[2:]]
            X = F.avg_pool2d(X, kernel_size=2, padding=pad)
            Y = F.avg_pool2d(Y, kernel_size=2, padding=pad)
    vals = torch.stack(mcs + [torch.relu(s)], dim=0)
    out = torch.prod(vals ** torch.tensor(weights, dtype=torch.float64).view(-1, 1, 1), dim=0)
    return out.mean() if size_average else out.mean(1)


# ----------------------------------------------------------------------------- helpers


def _pair(shape, seed, noise=0.05):
    """y: smooth test image in [0, 1] (channel count of `shape`), x: y plus noise, clamped."""
    from clc_amd.recipe import synthetic_image

    B, Cc, H, W = shape
    y = synthetic_image(B, H, W, seed, smooth=True)
    y = y.repeat(1, (Cc + 2) // 3, 1, 1)[:, :Cc].contiguous()
    g = torch.Generator().manual_seed(seed + 1)
    x = (y + noise * torch.randn(y.shape, generator=g)).clamp(0, 1)
    return x, y


def _close(a, b, tol, what=""):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    scale = max(b.abs().max().item(), 1e-12)
    err = (a - b).abs().max().item() / scale
    assert err <= tol, f"{what}: rel err {err:.3e} > {tol:.1e} (scale {scale:.3e})"


def _leaf(t, dev, grad=True):
    return t.to(dev).contiguous(memory_format=CL).requires_grad_(grad)


# ----------------------------------------------------------------------------- odd sides against the oracle


@pytest.mark.parametrize("shape", [(1, 3, 333, 517), (2, 3, 257, 256), (1, 1, 161, 200), (1, 3, 2040, 1356)])
def test_odd_sides_match_oracle(dev, shape):
    from clc_amd import ssim
    from oracle.loss import ms_ssim as oracle_ms_ssim

    x, y = _pair(shape, 11)
    xr = x.clone().requires_grad_()
    ref = oracle_ms_ssim(xr, y, data_range=1.0)
    ref.backward()
    xd = _leaf(x, dev)
    out = ssim.ms_ssim(xd, y.to(dev), data_range=1.0)
    assert abs(out.item() - ref.item()) < 2e-5, (out.item(), ref.item())
    out.backward()
    _close(xd.grad, xr.grad, 2e-3, "ms-ssim dx")


# ----------------------------------------------------------------------------- gradients of both inputs


def test_both_gradients_match_float64(dev):
    from clc_amd import ops

    x, y = _pair((2, 3, 193, 250), 21, noise=0.1)
    x64, y64 = x.double().requires_grad_(), y.double().requires_grad_()
    ref = ref_ms_ssim(x64, y64, data_range=1.0)
    ref.backward()
    xd, yd = _leaf(x, dev), _leaf(y, dev)
    out = ops.ms_ssim(xd, yd, data_range=1.0)
    assert abs(out.item() - ref.item()) < 2e-5
    out.backward()
    assert yd.grad is not None
    _close(xd.grad, x64.grad, 2e-3, "dx")
    _close(yd.grad, y64.grad, 2e-3, "dy")
    # one input at a time: dx alone is the dx of the pair bit for bit; dy alone (x and y exchanged in the kernels) matches float64
    xa = _leaf(x, dev)
    ops.ms_ssim(xa, y.to(dev), data_range=1.0).backward()
    assert torch.equal(xa.grad, xd.grad)
    yb = _leaf(y, dev)
    ops.ms_ssim(x.to(dev), yb, data_range=1.0).backward()
    _close(yb.grad, y64.grad, 2e-3, "dy alone")


# ----------------------------------------------------------------------------- the parameters of pytorch_msssim


@pytest.mark.parametrize("kw", [dict(win_size=7), dict(win_size=15), dict(win_sigma=1.0), dict(K=(0.02, 0.04)),
                                dict(weights=(0.2, 0.3, 0.5)), dict(size_average=False), dict(win="custom")])
def test_ms_ssim_parameters(dev, kw):
    from clc_amd import ssim

    x, y = _pair((2, 3, 241, 270), 31, noise=0.08)
    x, y = x * 255, y * 255                  # pytorch_msssim's default data_range = 255
    kw = dict(kw)
    w64 = _win64(kw.get("win_size", 11), kw.get("win_sigma", 1.5))
    if kw.get("win") == "custom":
        taps = torch.tensor([1.0, 2.0, 4.0, 2.0, 1.0]) / 10
        kw["win"] = taps.view(1, 1, 1, 5).repeat(3, 1, 1, 1)
        w64 = taps.double()
    x64 = x.double().requires_grad_()
    ref = ref_ms_ssim(x64, y.double(), w=w64, **{k: v for k, v in kw.items() if k in ("size_average", "weights", "K")})
    ref.sum().backward()
    xd = _leaf(x, dev)
    out = ssim.ms_ssim(xd, y.to(dev), **kw)
    assert out.shape == ref.shape
    assert (out.detach().cpu().double() - ref.detach()).abs().max().item() < 2e-5, (out, ref)
    out.sum().backward()
    _close(xd.grad, x64.grad, 2e-3, f"dx {kw}")


@pytest.mark.parametrize("kw", [dict(), dict(win_size=3), dict(size_average=False), dict(nonnegative_ssim=True)])
def test_ssim_single_scale(dev, kw):
    from clc_amd import ssim

    x, y = _pair((2, 2, 40, 57), 41, noise=0.1)
    if kw.get("nonnegative_ssim"):
        y = 1 - x                             # anti-correlated: negative SSIM in every channel
    w64 = _win64(kw.get("win_size", 11), 1.5)
    x64, y64 = x.double().requires_grad_(), y.double().requires_grad_()
    ref = ref_ssim(x64, y64, data_range=1.0, w=w64, **{k: v for k, v in kw.items() if k != "win_size"})
    ref.sum().backward()
    xd, yd = _leaf(x, dev), _leaf(y, dev)
    out = ssim.ssim(xd, yd, data_range=1.0, **kw)
    assert out.shape == ref.shape
    assert (out.detach().cpu().double() - ref.detach()).abs().max().item() < 2e-5, (out, ref)
    if kw.get("nonnegative_ssim"):
        assert ref_ssim(x, y, data_range=1.0).item() < 0 and out.item() == 0.0
        return
    out.sum().backward()
    _close(xd.grad, x64.grad, 2e-3, "dx")
    _close(yd.grad, y64.grad, 2e-3, "dy")


def test_modules(dev):
    from clc_amd.ssim import MS_SSIM, SSIM

    x, y = _pair((2, 3, 200, 211), 51, noise=0.08)
    m = SSIM(data_range=1.0, win_size=7, channel=3)
    assert tuple(m.win.shape) == (3, 1, 1, 7)
    assert abs(m(x.to(dev), y.to(dev)).item() - ref_ssim(x, y, data_range=1.0, w=_win64(7, 1.5)).item()) < 2e-5
    mm = MS_SSIM(data_range=1.0, size_average=False, weights=[0.5, 0.5])
    out = mm(x.to(dev), y.to(dev))
    ref = ref_ms_ssim(x, y, data_range=1.0, size_average=False, weights=(0.5, 0.5))
    assert out.shape == (2,) and (out.cpu().double() - ref).abs().max().item() < 2e-5


def test_keywords_reach_ops_and_train(dev):
    """ops.ms_ssim / train.ms_ssim take pytorch_msssim's keywords; their data_range stays 1.0 by default."""
    from clc_amd import ops, ssim, train

    x, y = _pair((2, 3, 176, 180), 61)
    xd, yd = x.to(dev), y.to(dev)
    a = ssim.ms_ssim(xd, yd, data_range=1.0, size_average=False, win_size=9, K=(0.02, 0.03))
    b = ops.ms_ssim(xd, yd, size_average=False, win_size=9, K=(0.02, 0.03))
    c = train.ms_ssim(xd, yd, size_average=False, win_size=9, K=(0.02, 0.03))
    assert a.shape == (2,) and torch.equal(a, b) and torch.equal(a, c)


# ----------------------------------------------------------------------------- the default path, bit for bit


class _OldMsSsimMeans(torch.autograd.Function):
    """The previous ops path: clc_ssim_init + clc_ssim_scale_fwd / clc_ssim_scale_bwd + clc_avgpool2 (even sides, dx only)."""

    @staticmethod
    def forward(ctx, x, y, levels):
        from clc_amd import lib

        L = lib.load()
        st = torch.cuda.current_stream().cuda_stream
        lib.check(L.clc_ssim_init(), "clc_ssim_init")
        B, Cc = x.shape[0], x.shape[1]
        xs, ys = [x], [y]
        means = torch.empty((levels, B * Cc, 2), device=x.device)
        for s in range(levels):
            xc, yc = xs[-1], ys[-1]
            h, w = xc.shape[2], xc.shape[3]
            nbytes = L.clc_ssim_workspace_bytes(B, h, w, Cc)
            ws = torch.empty((nbytes + 3) // 4, device=x.device)
            lib.check(L.clc_ssim_scale_fwd(xc.data_ptr(), Cc, yc.data_ptr(), Cc, B, h, w, Cc, 1.0, means[s].data_ptr(), ws.data_ptr(), nbytes, st))
            if s + 1 < levels:
                xn = torch.empty((B, Cc, h // 2, w // 2), device=x.device, memory_format=CL)
                yn = torch.empty((B, Cc, h // 2, w // 2), device=x.device, memory_format=CL)
                lib.check(L.clc_avgpool2(xc.data_ptr(), Cc, xn.data_ptr(), B, h, w, Cc, st))
                lib.check(L.clc_avgpool2(yc.data_ptr(), Cc, yn.data_ptr(), B, h, w, Cc, st))
                xs.append(xn)
                ys.append(yn)
        ctx.save_for_backward(*xs, *ys)
        return means

    @staticmethod
    def backward(ctx, g):
        from clc_amd import lib

        L = lib.load()
        st = torch.cuda.current_stream().cuda_stream
        saved = ctx.saved_tensors
        levels = len(saved) // 2
        g = g.contiguous()
        dnext = None
        for s in reversed(range(levels)):
            xc, yc = saved[s], saved[levels + s]
            B, Cc, h, w = xc.shape
            nbytes = L.clc_ssim_workspace_bytes(B, h, w, Cc)
            ws = torch.empty((nbytes + 3) // 4, device=xc.device)
            dx = torch.empty((B, Cc, h, w), device=xc.device, memory_format=CL)
            lib.check(L.clc_ssim_scale_bwd(xc.data_ptr(), Cc, yc.data_ptr(), Cc, B, h, w, Cc, 1.0, g[s].data_ptr(),
                                           dnext.data_ptr() if dnext is not None else None, dx.data_ptr(), Cc, ws.data_ptr(), nbytes, st))
            dnext = dx
        return dnext, None, None


def _old_ms_ssim(x, y):
    B, Cc = x.shape[0], x.shape[1]
    means = _OldMsSsimMeans.apply(x, y, 5).view(5, B, Cc, 2)
    out = None
    for s in range(5):
        v = torch.relu(means[s, :, :, 0 if s + 1 < 5 else 1]) ** float(WEIGHTS[s])
        out = v if out is None else out * v
    return out.mean()


@pytest.mark.parametrize("shape", [(2, 3, 256, 256), (1, 3, 256, 384)])
def test_default_path_bit_identical_to_previous_kernels(dev, shape):
    from clc_amd import ops, train

    x, y = _pair(shape, 71)
    xo = _leaf(x, dev)
    old = _old_ms_ssim(xo, y.to(dev).contiguous(memory_format=CL))
    old.backward()
    for fn in (ops.ms_ssim, train.ms_ssim):
        xn = _leaf(x, dev)
        new = fn(xn, y.to(dev).contiguous(memory_format=CL), data_range=1.0)
        new.backward()
        assert torch.equal(new, old), (new.item(), old.item())
        assert torch.equal(xn.grad, xo.grad)


# ----------------------------------------------------------------------------- batch independence, graph capture


def test_per_image_values_do_not_depend_on_the_batch(dev):
    from clc_amd import ssim

    x, y = _pair((3, 3, 193, 250), 81)
    xd, yd = x.to(dev), y.to(dev)
    batch = ssim.ms_ssim(xd, yd, data_range=1.0, size_average=False)
    batch_s = ssim.ssim(xd, yd, data_range=1.0, size_average=False)
    for i in range(3):
        assert torch.equal(batch[i:i + 1], ssim.ms_ssim(xd[i:i + 1], yd[i:i + 1], data_range=1.0, size_average=False))
        assert torch.equal(batch_s[i:i + 1], ssim.ssim(xd[i:i + 1], yd[i:i + 1], data_range=1.0, size_average=False))


def test_graph_capture_odd_sides_both_gradients(dev):
    from clc_amd import ops

    x, y = _pair((1, 3, 177, 250), 91)
    xs, ys = x.to(dev).contiguous(memory_format=CL), y.to(dev).contiguous(memory_format=CL)

    def step():
        xl, yl = xs.detach().requires_grad_(), ys.detach().requires_grad_()
        loss = ops.ms_ssim(xl, yl, data_range=1.0)
        gx, gy = torch.autograd.grad(loss, (xl, yl))
        return loss.detach(), gx, gy

    eager = step()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static = step()
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(static, eager):
        assert torch.equal(a, b)


# ----------------------------------------------------------------------------- argument checks


def test_value_errors_on_gpu(dev):
    from clc_amd import ssim

    x, y = _pair((1, 3, 200, 200), 101)
    xd, yd = x.to(dev), y.to(dev)
    with pytest.raises(ValueError):
        ssim.ms_ssim(xd, yd, win_size=10)
    with pytest.raises(ValueError):
        ssim.ssim(xd, yd, win_size=4)
    with pytest.raises(ValueError):
        ssim.ms_ssim(xd[..., :160], yd[..., :160])
    with pytest.raises(ValueError):
        ssim.ssim(xd[..., :9, :], yd[..., :9, :])
    with pytest.raises(ValueError):
        ssim.ms_ssim(xd, yd[..., :199])


# ----------------------------------------------------------------------------- evaluation


def test_compute_msssim_db_matches_oracle(dev):
    from clc_amd import eval as pe
    from oracle.loss import ms_ssim as oracle_ms_ssim

    x, y = _pair((1, 3, 333, 517), 111, noise=0.15)
    ref = -10 * math.log10(1 - oracle_ms_ssim(x.double(), y.double(), data_range=1.0).item())
    assert abs(pe.compute_msssim(x.to(dev), y.to(dev)) - ref) < 1e-4


def test_evaluate_ms_ssim_rows(dev):
    from clc_amd import eval as pe
    from clc_amd import models as pm
    from clc_amd import ssim
    from clc_amd.recipe import apply_weight_recipe, synthetic_image

    m = pm.CLC(N=64, num_ref_frames=1)
    apply_weight_recipe(m, 0)
    m = m.to(dev).eval()
    samples = [(synthetic_image(1, h, w, 120 + i, smooth=True)[0], [synthetic_image(1, h, w, 130 + i, smooth=True)[0]])
               for i, (h, w) in enumerate([(200, 300), (177, 190)])]
    plain = pe.evaluate(m, samples, device=dev)
    assert sorted(plain) == ["avg_bpp", "avg_psnr", "avg_time_s", "rows"]
    assert all(sorted(r) == ["bpp", "psnr"] for r in plain["rows"])
    res = pe.evaluate(m, samples, device=dev, ms_ssim=True)
    dbs = []
    for (x, refs), row, row0 in zip(samples, res["rows"], plain["rows"]):
        assert row["bpp"] == row0["bpp"] and row["psnr"] == row0["psnr"]
        xd = x.unsqueeze(0).to(dev)
        xp, padding = pe.pad(xd, 128)
        rp = [pe.pad(refs[0].unsqueeze(0).to(dev), 128)[0]]
        with torch.no_grad():
            enc = m.compress(xp, rp)
            x_hat = pe.crop(m.decompress(enc["strings"], enc["shape"], rp)["x_hat"], padding)
            v = ssim.ms_ssim(xd, x_hat, data_range=1.0).item()
        assert row["ms_ssim"] == v and row["ms_ssim_db"] == -10 * math.log10(1 - v)
        dbs.append(row["ms_ssim_db"])
    assert res["avg_ms_ssim_db"] == sum(dbs) / 2
