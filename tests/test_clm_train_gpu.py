"""Trainable Conditional Latent Matching: the recorded forward and the HIP backward of the CLM ops against autograd through the
oracle (oracle/clm.py, or a plain-torch restatement of one op) in float64 on the CPU.

Error measure: max|a - b| / max|b| per tensor, b the float64 reference.  Bars: 2e-5 forward, 1e-4 gradients.  A gradient
tensor that misses 1e-4 may take 4x the error of the FLOAT32 ORACLE against the float64 one on the same input (the reference's own
rounding; the factor covers another summation order at the same precision); both figures are printed when that happens.
"""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
CL = torch.channels_last
GOLD = os.path.join(os.path.dirname(__file__), "golden", "clm.npz")
FWD_BAR, GRAD_BAR = 2e-5, 1e-4


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-300)


def _check_grads(named, ref32=None):
    """named: [(name, got, float64 reference)]; ref32: callable -> {name: float32-oracle tensor}, evaluated only if a tensor misses the bar"""
    r32 = None
    for name, got, ref in named:
        assert got is not None, f"{name}: no gradient"
        assert tuple(got.shape) == tuple(ref.shape), (name, got.shape, ref.shape)
        err = _rel(got, ref)
        print(f"  grad {name}: {err:.3e}")
        bar = GRAD_BAR
        if err >= bar and ref32 is not None:
            r32 = ref32() if r32 is None else r32
            own = _rel(r32[name], ref)
            bar = max(bar, 4.0 * own)
            print(f"  grad {name}: HIP {err:.3e}, float32 oracle {own:.3e} -> bar {bar:.3e}")
        assert err < bar, (name, err, bar)


def _to_dev(t, dev, grad=True):
    return t.float().to(dev).contiguous(memory_format=CL).requires_grad_(grad)


# ------------------------------------------------------------------------------------------------------------------ 1. similarity op


def _sim_ref(yt, yr, tau, g):
    """(w, dyt, dyr) of w = softmax(yt yr^T / tau, -1).sum(1) in the dtype of the inputs; yt / yr [B,C,H,W]"""
    yt, yr = yt.clone().requires_grad_(True), yr.clone().requires_grad_(True)
    B, C = yt.shape[:2]
    S = F.softmax(torch.bmm(yt.reshape(B, C, -1).transpose(1, 2), yr.reshape(B, C, -1)) / tau, dim=-1)
    w = S.sum(1)
    dyt, dyr = torch.autograd.grad(w, (yt, yr), g.to(w.dtype))
    return w.detach(), dyt, dyr, S.max().item()


SIM_SHAPES = [(2, 16, 16, 64), (3, 32, 24, 128), (2, 32, 32, 320), (1, 64, 64, 192), (2, 20, 12, 64), (1, 17, 19, 96)]


@pytest.mark.parametrize("B,H,W,C", SIM_SHAPES)
def test_sim_colsum_forward_backward(dev, B, H, W, C):
    from clc_amd import clm, lib, ops

    tau = 0.5
    gen = torch.Generator().manual_seed(100 + H * W + C)
    a = (3.0 * tau / C ** 0.5) ** 0.5    # logits yt.yr / tau get a standard deviation of about 3
    yt = torch.randn(B, C, H, W, generator=gen, dtype=torch.float64) * a
    yr = torch.randn(B, C, H, W, generator=gen, dtype=torch.float64) * a
    g = torch.randn(B, H * W, generator=gen, dtype=torch.float64)
    yt, yr, g = yt.float().double(), yr.float().double(), g.float().double()   # the float32 inputs, exactly
    w64, dyt64, dyr64, smax = _sim_ref(yt, yr, tau, g)
    print(f"\n  sim ({B}, {H}x{W}, {C}): max S = {smax:.3f}")
    ytg, yrg = _to_dev(yt, dev), _to_dev(yr, dev)
    w = clm.sim_colsum(ytg, yrg, tau)
    w.backward(g.float().to(dev))
    err = _rel(w, w64)
    print(f"  forward: {err:.3e}")
    assert err < FWD_BAR, err
    # the inference kernel on the same input
    L = lib.load()
    nbytes = L.clc_clm_sim_colsum_workspace_bytes(B, H * W)
    ws = torch.empty((nbytes + 3) // 4, device=dev)
    w_old = torch.empty(B, H * W, device=dev)
    lib.check(L.clc_clm_sim_colsum(ytg.data_ptr(), C, yrg.data_ptr(), C, B, H * W, C, tau, w_old.data_ptr(), ws.data_ptr(), nbytes, ops._stream()))
    err_old = _rel(w, w_old)
    print(f"  recorded forward vs clc_clm_sim_colsum: {err_old:.3e}")
    assert err_old < FWD_BAR, err_old

    def ref32():
        _w, a32, b32, _s = _sim_ref(yt.float(), yr.float(), tau, g.float())
        return {"dyt": a32, "dyr": b32}

    _check_grads([("dyt", ytg.grad, dyt64), ("dyr", yrg.grad, dyr64)], ref32)


def test_sim_colsum_limits(dev):
    from clc_amd import clm, lib

    with pytest.raises(lib.ClcError, match="4097"):
        clm.sim_colsum(torch.zeros(1, 8, 4097, 1, device=dev).contiguous(memory_format=CL).requires_grad_(),
                       torch.zeros(1, 8, 4097, 1, device=dev).contiguous(memory_format=CL), 0.5)
    with pytest.raises(lib.ClcError):   # C % 4
        clm.sim_colsum(torch.zeros(1, 6, 4, 4, device=dev).requires_grad_(), torch.zeros(1, 6, 4, 4, device=dev), 0.5)


def test_sim_colsum_one_sided(dev):
    """needs_input_grad: a reference side that wants no gradient gets none, and the dyr sweep does not run"""
    from clc_amd import clm

    gen = torch.Generator().manual_seed(5)
    yt, yr = torch.randn(1, 64, 8, 8, generator=gen) * 0.4, torch.randn(1, 64, 8, 8, generator=gen) * 0.4
    g = torch.randn(1, 64, generator=gen)
    _w, dyt64, _d, _s = _sim_ref(yt.double(), yr.double(), 0.5, g.double())
    ytg, yrg = _to_dev(yt, dev), _to_dev(yr, dev, grad=False)
    clm.TRACE = []
    try:
        clm.sim_colsum(ytg, yrg, 0.5).backward(g.to(dev))
        assert clm.TRACE == [("sim_colsum_bwd", {"dyt": True, "dyr": False})], clm.TRACE
    finally:
        clm.TRACE = None
    assert yrg.grad is None
    _check_grads([("dyt", ytg.grad, dyt64)])


# ---------------------------------------------------------------------------------------------------------------------- 2. deform op


def _deform_ref(x, off, logit):
    """oracle/clm.py's sampling (DeformableAlignment.forward from `offset` on) with the offsets / modulation logits as inputs"""
    B, C, H, W = x.shape
    offset = off.reshape(B, 9, 2, H, W)
    modulation = torch.sigmoid(logit).reshape(B, 9, 1, H, W)
    hh = torch.arange(H, dtype=x.dtype).view(1, 1, H, 1)
    ww = torch.arange(W, dtype=x.dtype).view(1, 1, 1, W)
    off_h, off_w = hh + offset[:, :, 0], ww + offset[:, :, 1]
    valid = (off_h >= 0) & (off_h <= H - 1) & (off_w >= 0) & (off_w <= W - 1)
    h0 = off_h.clamp(0, H - 1).long()
    w0 = off_w.clamp(0, W - 1).long()
    h1, w1 = (h0 + 1).clamp(max=H - 1), (w0 + 1).clamp(max=W - 1)
    lh, lw = off_h - h0.to(x.dtype), off_w - w0.to(x.dtype)
    flat = x.reshape(B, C, H * W)

    def gather(hi, wi):
        idx = (hi * W + wi).reshape(B, 1, -1).expand(B, C, -1)
        return torch.gather(flat, 2, idx).reshape(B, C, 9, H, W)

    val = ((1 - lh) * (1 - lw)).unsqueeze(1) * gather(h0, w0) + (lh * (1 - lw)).unsqueeze(1) * gather(h1, w0) + \
          ((1 - lh) * lw).unsqueeze(1) * gather(h0, w1) + (lh * lw).unsqueeze(1) * gather(h1, w1)
    val = val * (valid.to(x.dtype) * modulation[:, :, 0]).unsqueeze(1)
    return val.sum(dim=2)


def test_deform_restatement_matches_oracle():
    """zero convolution weights, chosen biases -> constant offsets / modulation: the restatement equals oracle.clm.DeformableAlignment"""
    from oracle import clm as oc

    gen = torch.Generator().manual_seed(1)
    B, C, H, W = 2, 8, 9, 7
    o = oc.DeformableAlignment(C).double()
    with torch.no_grad():
        o.offset_conv.weight.zero_()
        o.modulation_conv.weight.zero_()
        o.offset_conv.bias.copy_((torch.rand(18, generator=gen, dtype=torch.float64) - 0.5) * 9.0)
        o.modulation_conv.bias.copy_(torch.randn(9, generator=gen, dtype=torch.float64))
    x = torch.randn(B, C, H, W, generator=gen, dtype=torch.float64)
    sim = torch.rand(B, H * W, H * W, generator=gen, dtype=torch.float64)
    with torch.no_grad():
        ref = o(x, sim)
        got = _deform_ref(x, o.offset_conv.bias.view(1, 18, 1, 1).expand(B, 18, H, W), o.modulation_conv.bias.view(1, 9, 1, 1).expand(B, 9, H, W))
    assert ref.abs().max() > 0.1
    assert (got - ref).abs().max().item() <= 1e-6 * ref.abs().max().item()


def _constructed_offsets(B, H, W, gen):
    """sampling positions with fractions in [0.05, 0.95]: about half the taps outside the map (at least 0.05 beyond the validity edge), the
    rest inside, at least 0.05 from every grid line — except a few taps put EXACTLY on the last row / column (offset an integer, so float32
    and float64 agree to the bit), the only place where h1 == h0 / w1 == w0."""
    def axis(n):
        frac = 0.05 + 0.9 * torch.rand(B, 9, H, W, generator=gen, dtype=torch.float64)
        cell = torch.floor(torch.rand(B, 9, H, W, generator=gen, dtype=torch.float64) * (n - 1))   # 0 .. n-2
        inside = cell + frac
        outside = torch.where(torch.rand(B, 9, H, W, generator=gen) < 0.5, -0.05 - 2.5 * frac, n - 1 + 0.05 + 2.5 * frac)
        pick = torch.rand(B, 9, H, W, generator=gen)
        pos = torch.where(pick < 0.7, inside, outside)            # 0.7^2 ~ half the taps valid
        return torch.where(pick < 0.04, torch.full_like(pos, n - 1), pos)
    ph, pw = axis(H), axis(W)
    hh = torch.arange(H, dtype=torch.float64).view(1, 1, H, 1)
    ww = torch.arange(W, dtype=torch.float64).view(1, 1, 1, W)
    off = torch.stack([ph - hh, pw - ww], dim=2).reshape(B, 18, H, W)
    return off.float().double()


def _deform_case(dev, x, off, logit, dout, pad):
    from clc_amd import clm

    B, C, H, W = x.shape
    xr, offr, lr = (t.clone().requires_grad_(True) for t in (x, off, logit))
    out64 = _deform_ref(xr, offr, lr)
    gx, go, gl = torch.autograd.grad(out64, (xr, offr, lr), dout)
    pos = (offr.detach().reshape(B, 9, 2, H, W)[:, :, 0] + torch.arange(H, dtype=torch.float64).view(1, 1, H, 1))
    print(f"\n  deform {tuple(x.shape)}: {((pos >= 0) & (pos <= H - 1)).float().mean().item():.2f} of the taps inside in h")
    xg = _to_dev(x, dev)
    if pad:   # the padded rows the modules use
        offg = _to_dev(torch.cat([off, torch.zeros(B, 2, H, W, dtype=off.dtype)], 1), dev)
        lg = _to_dev(torch.cat([logit, torch.zeros(B, 3, H, W, dtype=off.dtype)], 1), dev)
    else:
        offg, lg = _to_dev(off, dev), _to_dev(logit, dev)
    out = clm.deform(xg, offg, lg)
    err = _rel(out, out64)
    print(f"  forward: {err:.3e}")
    assert err < FWD_BAR, err
    out.backward(dout.float().to(dev).contiguous(memory_format=CL))
    if pad:
        assert float(offg.grad[:, 18:].abs().max()) == 0.0 and float(lg.grad[:, 9:].abs().max()) == 0.0

    def ref32():
        a, b, c = (t.float().clone().requires_grad_(True) for t in (x, off, logit))
        r = torch.autograd.grad(_deform_ref(a, b, c), (a, b, c), dout.float())
        return dict(zip(("dx", "d_off", "d_logit"), r))

    _check_grads([("dx", xg.grad, gx), ("d_off", offg.grad[:, :18], go), ("d_logit", lg.grad[:, :9], gl)], ref32)
    return xg, offg, lg


@pytest.mark.parametrize("B,H,W,C,pad", [(2, 16, 16, 64, True), (1, 32, 24, 320, False), (1, 17, 19, 96, True)])
def test_deform_backward_constructed_offsets(dev, B, H, W, C, pad):
    gen = torch.Generator().manual_seed(7 + C)
    x = torch.randn(B, C, H, W, generator=gen).double()
    off = _constructed_offsets(B, H, W, gen)
    logit = torch.randn(B, 9, H, W, generator=gen).double()
    dout = torch.randn(B, C, H, W, generator=gen).double()
    _deform_case(dev, x, off, logit, dout, pad)


def test_deform_backward_degenerate_and_deterministic(dev):
    """every tap of every pixel aimed at (3.5, 4.5): four destination pixels take all 9 * H * W contributions; two passes give the same bits"""
    from clc_amd import clm

    gen = torch.Generator().manual_seed(11)
    B, C, H, W = 2, 64, 16, 16
    x = torch.randn(B, C, H, W, generator=gen).double()
    hh = torch.arange(H, dtype=torch.float64).view(1, 1, H, 1)
    ww = torch.arange(W, dtype=torch.float64).view(1, 1, 1, W)
    off = torch.stack([(3.5 - hh).expand(B, 9, H, W), (4.5 - ww).expand(B, 9, H, W)], dim=2).reshape(B, 18, H, W)
    logit = torch.randn(B, 9, H, W, generator=gen).double()
    dout = torch.randn(B, C, H, W, generator=gen).double()
    xg, offg, lg = _deform_case(dev, x, off, logit, dout, False)
    first = [t.grad.clone() for t in (xg, offg, lg)]
    assert int((first[0].abs().amax(dim=1) > 0).sum()) == 4 * B
    for t in (xg, offg, lg):
        t.grad = None
    clm.deform(xg, offg, lg).backward(dout.float().to(dev).contiguous(memory_format=CL))
    for a, t in zip(first, (xg, offg, lg)):
        assert torch.equal(a, t.grad)


# ------------------------------------------------------------------------------------------------------------------------ 3. fuse op


@pytest.mark.parametrize("gate", [False, True])
@pytest.mark.parametrize("M", [1, 2, 3, 8])
@pytest.mark.parametrize("C", [64, 320])
def test_fuse_backward(dev, gate, M, C):
    from clc_amd import clm

    gen = torch.Generator().manual_seed(13 * M + C + int(gate))
    B, H, W = 2, 8, 6
    feats = [torch.randn(B, C, H, W, generator=gen).double() for _ in range(M)]
    atts = [torch.randn(B, 1, H, W, generator=gen).double() * 2.0 for _ in range(M)]
    y = torch.randn(B, C, H, W, generator=gen).double()
    dout = torch.randn(B, C, H, W, generator=gen).double()

    def ref(dtype):
        f = [t.to(dtype).clone().requires_grad_(True) for t in feats]
        a = [t.to(dtype).clone().requires_grad_(True) for t in atts]
        yy = y.to(dtype).clone().requires_grad_(True)
        wts = F.softmax(torch.stack(a, dim=1), dim=1)
        fused = [fi * torch.sigmoid(ai) for fi, ai in zip(f, a)] if gate else f
        out = (torch.stack(fused, dim=1) * wts).sum(dim=1) + yy
        grads = torch.autograd.grad(out, f + a + [yy], dout.to(dtype))
        return out.detach(), grads

    out64, g64 = ref(torch.float64)
    fg, ag, yg = [_to_dev(t, dev) for t in feats], [_to_dev(t, dev) for t in atts], _to_dev(y, dev)
    out = clm.fuse(fg, ag, yg, gate)
    err = _rel(out, out64)
    print(f"\n  fuse M={M} C={C} gate={gate}: forward {err:.3e}")
    assert err < FWD_BAR, err
    out.backward(dout.float().to(dev).contiguous(memory_format=CL))
    names = [f"dfeat{i}" for i in range(M)] + [f"datt{i}" for i in range(M)] + ["dy"]
    _check_grads(list(zip(names, [t.grad for t in fg + ag + [yg]], g64)), lambda: dict(zip(names, ref(torch.float32)[1])))


# ------------------------------------------------------------------------------------------------------------------- 4. whole modules


def _oracle(kind, C=64, temperature=0.5, recipe=11):
    from oracle import clm as oc
    from oracle.recipe import apply_weight_recipe

    m = (oc.CLM if kind == "clm" else oc.SimpleCLM)(C, temperature=temperature).eval()
    apply_weight_recipe(m, recipe)
    if kind == "clm":   # (the set-up of tests/test_clm.py)
        with torch.no_grad():
            m.alignment.offset_conv.weight.mul_(6.0)
            m.alignment.offset_conv.bias.mul_(20.0)
    return m


def _hip(kind, o, dev, C=64, temperature=0.5):
    from clc_amd import clm as pc

    p = (pc.CLM if kind == "clm" else pc.SimpleCLM)(C, temperature=temperature)
    p.load_state_dict(o.state_dict())
    return p.to(dev).eval()


def _draw(seed, B, n_refs, C=64, H=16, W=16):
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(B, C, H, W, generator=g)
    refs = [torch.randn(B, C, H, W, generator=g) for _ in range(n_refs)]
    dout = torch.randn(B, C, H, W, generator=g)
    return y, refs, dout


def _oracle_run(o, y, refs, dout, dtype, refs_grad=True):
    """forward + backward through the oracle in `dtype`: (out, {name: gradient}, [offsets per reference])"""
    m = copy.deepcopy(o).to(dtype)
    offsets = []
    hook = m.alignment.offset_conv.register_forward_hook(lambda _m, _i, out: offsets.append(out.detach())) if hasattr(m, "alignment") else None
    yy = y.to(dtype).clone().requires_grad_(True)
    rr = [r.to(dtype).clone().requires_grad_(refs_grad) for r in refs]
    out = m(yy, rr)
    out.backward(dout.to(dtype))
    if hook is not None:
        hook.remove()
    grads = {n: p.grad for n, p in m.named_parameters()}
    grads["y"] = yy.grad
    for i, r in enumerate(rr):
        grads[f"y_ref{i}"] = r.grad
    return out.detach(), grads, offsets


def _coords(offset, dtype):
    B, _c, H, W = offset.shape
    o = offset.to(dtype).reshape(B, 9, 2, H, W)
    return torch.arange(H, dtype=dtype).view(1, 1, H, 1) + o[:, :, 0].cpu(), torch.arange(W, dtype=dtype).view(1, 1, 1, W) + o[:, :, 1].cpu()


def _min_grid_distance(offsets):
    d = 1.0
    for off in offsets:
        for c, n in zip(_coords(off, torch.float64), off.shape[2:]):
            c = c[(c > -0.5) & (c < n - 0.5)]
            d = min(d, (c - c.round()).abs().min().item())
    return d


def _flipped_taps(hip_offsets, ref_offsets):
    """taps whose validity or cell index differs between the HIP module's float32 offsets and the float64 oracle's"""
    n = 0
    for a, b in zip(hip_offsets, ref_offsets):
        H, W = a.shape[2:]
        (ah, aw), (bh, bw) = _coords(a.float(), torch.float32), _coords(b, torch.float64)
        va = (ah >= 0) & (ah <= H - 1) & (aw >= 0) & (aw <= W - 1)
        vb = (bh >= 0) & (bh <= H - 1) & (bw >= 0) & (bw <= W - 1)
        cell = (ah.clamp(0, H - 1).long() != bh.clamp(0, H - 1).long()) | (aw.clamp(0, W - 1).long() != bw.clamp(0, W - 1).long())
        n += int(((va != vb) | (va & vb & cell)).sum())
    return n


def _module_grads(p, yg, rg):
    grads = {n: q.grad for n, q in p.named_parameters()}
    grads["y"] = yg.grad
    for i, r in enumerate(rg):
        grads[f"y_ref{i}"] = r.grad
    return grads


def _compare_module(p, o, grads, g64, y, refs, dout, refs_grad=True):
    named = []
    for name, ref in g64.items():
        if ref is None:
            assert grads[name] is None, name
            continue
        if name == "attention_conv.bias" and hasattr(o, "alignment"):
            # analytically zero (the softmax over the references ignores a common shift): an absolute bound, not a relative error
            lim = GRAD_BAR * g64["attention_conv.weight"].abs().max().item()
            print(f"  grad attention_conv.bias: |g| = {grads[name].abs().max().item():.3e} (bound {lim:.3e})")
            assert grads[name].abs().max().item() <= lim
            continue
        named.append((name, grads[name], ref))
    _check_grads(named, lambda: _oracle_run(o, y, refs, dout, torch.float32, refs_grad)[1])


@pytest.mark.parametrize("seed", [2689, 792])
def test_clm_module_gradients(dev, seed):
    o = _oracle("clm")
    y, refs, dout = _draw(seed, 1, 2)
    out64, g64, off64 = _oracle_run(o, y, refs, dout, torch.float64)
    dist = _min_grid_distance(off64)
    print(f"\n  seed {seed}: smallest distance of a sampling coordinate to a grid line = {dist:.2e}")
    assert dist >= 5e-4, f"seed {seed} draws a sampling coordinate {dist:.2e} from a grid line with this torch build: pick seeds with tools/scan_clm_seeds.py"
    assert len(g64) == 17
    p = _hip("clm", o, dev)
    with torch.no_grad():
        before = p(y.to(dev), [r.to(dev) for r in refs])
    yg, rg = _to_dev(y, dev), [_to_dev(r, dev) for r in refs]
    out = p(yg, rg)
    err = _rel(out, out64)
    print(f"  recorded forward vs float64 oracle: {err:.3e}")
    assert err < FWD_BAR, err
    flips = _flipped_taps(p.last_offsets, off64)
    print(f"  flipped taps: {flips}")
    assert flips == 0
    out.backward(dout.to(dev))
    first = _module_grads(p, yg, rg)
    _compare_module(p, o, first, g64, y, refs, dout)
    # a second pass on the same inputs: the same bits
    first = {k: v.clone() for k, v in first.items()}
    p.zero_grad(set_to_none=True)
    yg.grad = None
    for r in rg:
        r.grad = None
    p(yg, rg).backward(dout.to(dev))
    for k, v in _module_grads(p, yg, rg).items():
        assert torch.equal(v, first[k]), k
    # recording leaves no state behind
    with torch.no_grad():
        after = p(y.to(dev), [r.to(dev) for r in refs])
    assert torch.equal(before, after)


@pytest.mark.parametrize("kind", ["clm", "simple"])
def test_recorded_forward_matches_reference_golden(dev, kind):
    g = np.load(GOLD)
    o = _oracle(kind)
    p = _hip(kind, o, dev)
    y = torch.from_numpy(g[f"{kind}_y"]).to(dev)
    refs = [torch.from_numpy(r).to(dev) for r in g[f"{kind}_refs"]]
    with torch.no_grad():
        before = p(y, refs)
    out = p(y, refs)
    assert out.requires_grad and out.grad_fn is not None
    ref = torch.from_numpy(g[f"{kind}_out"])
    err = _rel(out, ref)
    print(f"\n  {kind}: recorded forward vs golden {err:.3e}")
    assert err < 1e-4, err
    out.sum().backward()
    with torch.no_grad():
        after = p(y, refs)
    assert torch.equal(before, after)


def test_clm_module_detached_references(dev):
    """references from a no_grad encoder: no gradient for them and no deform input scatter; y and every parameter as before.  (The
    similarity's reference side still gets its gradient while feature_transform is trained: it reaches those parameters through
    f(y_ref).  With feature_transform frozen as well, that sweep is skipped too.)"""
    from clc_amd import clm as pc

    o = _oracle("clm")
    y, refs, dout = _draw(792, 1, 2)
    _out, g64, off64 = _oracle_run(o, y, refs, dout, torch.float64, refs_grad=False)
    assert _min_grid_distance(off64) >= 5e-4
    p = _hip("clm", o, dev)
    yg, rg = _to_dev(y, dev), [_to_dev(r, dev, grad=False) for r in refs]
    pc.TRACE = []
    try:
        out = p(yg, rg)
        assert _flipped_taps(p.last_offsets, off64) == 0
        out.backward(dout.to(dev))
        trace = list(pc.TRACE)
    finally:
        pc.TRACE = None
    assert all(r.grad is None for r in rg)
    deform = [ran for name, ran in trace if name == "deform_bwd"]
    assert len(deform) == 2 and all(not ran["dx"] and ran["doff"] for ran in deform), trace
    scale = [ran for name, ran in trace if name == "scale_rows_bwd"]
    assert len(scale) == 2 and all(not ran["dx"] and ran["dw"] for ran in scale), trace
    _compare_module(p, o, _module_grads(p, yg, rg), g64, y, refs, dout, refs_grad=False)
    # feature_transform frozen too: nothing behind f(y_ref) wants a gradient
    for q in p.feature_transform.parameters():
        q.requires_grad_(False)
    pc.TRACE = []
    try:
        p(yg, rg).backward(dout.to(dev))
        sim = [ran for name, ran in pc.TRACE if name == "sim_colsum_bwd"]
    finally:
        pc.TRACE = None
    assert len(sim) == 2 and all(ran["dyt"] and not ran["dyr"] for ran in sim), sim


def test_simple_clm_module_gradients(dev):
    o = _oracle("simple")
    y, refs, dout = _draw(3, 2, 2)
    out64, g64, _ = _oracle_run(o, y, refs, dout, torch.float64)
    p = _hip("simple", o, dev)
    yg, rg = _to_dev(y, dev), [_to_dev(r, dev) for r in refs]
    out = p(yg, rg)
    err = _rel(out, out64)
    print(f"\n  SimpleCLM recorded forward: {err:.3e}")
    assert err < FWD_BAR, err
    out.backward(dout.to(dev))
    _compare_module(p, o, _module_grads(p, yg, rg), g64, y, refs, dout)


def test_clm_module_larger_shape_forward_and_finite_gradients(dev):
    """32x24 latents, C = 128, batch 3 (the set-up of test_hip_matches_oracle_other_shape): forward against the float64 oracle, gradients
    finite.  (No gradient comparison at this size: with 41 000 taps no seed keeps every sampling coordinate away from the grid lines;
    the ops are compared at these sizes with constructed positions above.)"""
    from oracle import clm as oc
    from oracle.recipe import apply_weight_recipe

    o = oc.CLM(128, temperature=0.7).eval()
    apply_weight_recipe(o, 5)
    with torch.no_grad():
        o.alignment.offset_conv.weight.mul_(8.0)
    p = _hip("clm", o, dev, C=128, temperature=0.7)
    g = torch.Generator().manual_seed(3)
    y = torch.randn(3, 128, 32, 24, generator=g)
    refs = [torch.randn(3, 128, 32, 24, generator=g) for _ in range(2)]
    with torch.no_grad():
        ref = copy.deepcopy(o).double()(y.double(), [r.double() for r in refs])
    yg, rg = _to_dev(y, dev), [_to_dev(r, dev) for r in refs]
    out = p(yg, rg)
    err = _rel(out, ref)
    print(f"\n  C=128 32x24 B=3 recorded forward: {err:.3e}")
    assert err < FWD_BAR, err
    out.backward(torch.randn(out.shape, generator=g).to(dev))
    for name, v in _module_grads(p, yg, rg).items():
        assert v is not None and bool(torch.isfinite(v).all()), name


# ---------------------------------------------------------------------------------------------------------- 5. capture


def test_sim_colsum_forward_backward_captured(dev):
    """forward + backward of the similarity op in one captured graph on one stream; two replays equal the eager bits.
    Every run differentiates with respect to leaves of its own on the shared storage: a leaf that an earlier autograd graph used keeps
    the stream of that graph, autograd.grad inside a capture would then join the capturing stream with it, and ending such a capture
    crashes in the runtime (clc_amd/graphed.py, _StandIns, met the same thing)."""
    from clc_amd import clm, ops

    gen = torch.Generator().manual_seed(21)
    B, C, H, W = 2, 96, 20, 12
    yt = _to_dev(torch.randn(B, C, H, W, generator=gen) * 0.3, dev, grad=False)
    yr = _to_dev(torch.randn(B, C, H, W, generator=gen) * 0.3, dev, grad=False)
    g = torch.randn(B, H * W, generator=gen).to(dev)

    def run():
        a, b = yt.detach().requires_grad_(True), yr.detach().requires_grad_(True)
        w = clm.sim_colsum(a, b, 0.5)
        da, db = torch.autograd.grad(w, (a, b), g)
        return w.detach(), da, db

    w0, a0, b0 = run()
    assert float(a0.abs().max()) > 0 and float(b0.abs().max()) > 0
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):   # warm-up on a side stream, as torch.cuda.graph asks
        run()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with ops.capture_guard(), torch.cuda.graph(graph, capture_error_mode=ops.graph_capture_mode()):
        w, da, db = run()
    for _ in range(2):
        for t in (w, da, db):
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(w, w0) and torch.equal(da, a0) and torch.equal(db, b0)
