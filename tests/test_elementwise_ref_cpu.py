"""The float64 references of tests/elementwise_ref.py against independent float64 formulations (torch.nn.functional, double autograd,
oracle.leaves, oracle.loss), so that a wrong reference fails here before it misjudges a kernel — and the one place where the libm budgets
of elementwise_ref.BUDGET are measured: the kernels' formulas in float32 torch on the CPU, on the operands of the GPU cases."""
import math

import pytest
import torch
import torch.nn.functional as F

import elementwise_ref as R

F64 = torch.float64


def _close(a, b, tol=1e-12):
    assert a.shape == b.shape, (a.shape, b.shape)
    scale = max(1.0, float(b.abs().max()))
    assert float((a - b).abs().max()) <= tol * scale, float((a - b).abs().max())


# ------------------------------------------------------------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("C,rows", [(3, 5), (64, 17), (96, 35), (256, 5)])
@pytest.mark.parametrize("paired", [False, True])
def test_layernorm_reference_is_double_autograd(C, rows, paired):
    t = {k: v.double() for k, v in R.ln_inputs(C, rows).items()}
    half = rows // 3 if paired else 0
    x = t["x"].clone().requires_grad_()
    ps = [t[k].clone().requires_grad_() for k in ("gamma", "beta", "gamma2", "beta2")]
    if paired:
        y = torch.cat((F.layer_norm(x[:half], (C,), ps[0], ps[1], R.LN_EPS), F.layer_norm(x[half:], (C,), ps[2], ps[3], R.LN_EPS)))
    else:
        y = F.layer_norm(x, (C,), ps[0], ps[1], R.LN_EPS)
    y.backward(t["dy"])
    g2, b2 = (t["gamma2"], t["beta2"]) if paired else (None, None)
    f = R.ln_fwd_ref(t["x"], t["gamma"], t["beta"], g2, b2, half)
    _close(f["y"], y.detach())
    _close(f["mean"], t["x"].mean(1))
    _close(f["rstd"], 1 / torch.sqrt(t["x"].var(1, unbiased=False) + R.LN_EPS))
    b = R.ln_bwd_ref(t["x"], t["gamma"], t["dy"], t["dadd"], g2, half)
    _close(b["dx"], x.grad + t["dadd"])
    _close(b["params"][0]["dgamma"], ps[0].grad)
    _close(b["params"][0]["dbeta"], ps[1].grad)
    if paired:
        _close(b["params"][1]["dgamma"], ps[2].grad)
        _close(b["params"][1]["dbeta"], ps[3].grad)
    assert (f["by"] > 0).all() and (b["bdx"] > 0).all()


def test_partial_reduce_and_colsum_references():
    p = R.rand(1, 9, 33).double()
    init = R.rand(2, 33).double()
    out, bound = R.partial_reduce_ref(p, init)
    _close(out, torch.einsum("bn->n", p) + init)
    out, bound = R.colsum_ref(p, None)
    _close(out, torch.ones(1, 9, dtype=F64).matmul(p)[0])
    assert R.colsum_terms(1) == 3 and R.colsum_terms(257) == 129 + 2 + 1 and R.colsum_terms(512 * 256 + 3) == 257 + 512 + 1


# ------------------------------------------------------------------------------------------------------------------- activations
def _act_fn(act):
    return {R.ACT_NONE: lambda v: v, R.ACT_LRELU: lambda v: F.leaky_relu(v, R.SLOPE32), R.ACT_RELU: F.relu,
            R.ACT_GELU: lambda v: F.gelu(v), R.ACT_HALFTANH: lambda v: 0.5 * torch.tanh(v)}[act]


@pytest.mark.parametrize("act", [R.ACT_NONE, R.ACT_LRELU, R.ACT_RELU, R.ACT_GELU, R.ACT_HALFTANH])
def test_activation_derivatives_are_autograd(act):
    dy, saved = (t.double() for t in R.act_inputs(35, 22))
    v = saved.clone().requires_grad_()
    out = _act_fn(act)(v)
    out.backward(dy)
    keep = saved != 0 if act in (R.ACT_LRELU, R.ACT_RELU) else torch.ones_like(saved, dtype=torch.bool)   # (autograd's choice at the kink is not the kernels')
    dz, bound = R.act_bwd_ref(dy, saved, act, 1)
    _close(dz[keep], v.grad[keep])
    assert (bound > 0).all()
    if act in (R.ACT_LRELU, R.ACT_RELU):
        # at +-0 the kernels' rule is `s > 0 ? 1 : slope`
        z = torch.tensor([0.0, -0.0], dtype=F64)
        d, _ = R.act_deriv_ref(z, act, 1)
        assert d.tolist() == [R.SLOPE32 if act == R.ACT_LRELU else 0.0] * 2
    if act != R.ACT_GELU:
        # from the OUTPUT: the same derivative (GELU has no such form)
        dz_out, _ = R.act_bwd_ref(dy, out.detach(), act, 0)
        _close(dz_out[keep], v.grad[keep], 1e-9)
    d, S = R.act_deriv_ref(saved, R.ACT_SAVED_DERIV, 0)
    assert torch.equal(d, saved)


@pytest.mark.parametrize("shape", R.UNSHUFFLE_SHAPES)
def test_unshuffle_is_pixel_unshuffle(shape):
    N, H, W, C = shape
    t = R.rand(3, N, 2 * H, 2 * W, C // 4).double()
    want = F.pixel_unshuffle(t.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    assert torch.equal(R.unshuffle_ref(t), want)


def test_gate_and_axpby_references():
    a, b, idn, g = (t.double().requires_grad_() for t in R.gate_inputs(1023))
    out = a * torch.sigmoid(b) + idn
    out.backward(g.detach())
    y, by = R.gate_fwd_ref(a.detach(), b.detach(), idn.detach())
    _close(y, out.detach())
    da, bda, db, bdb = R.gate_bwd_ref(g.detach(), a.detach(), b.detach())
    _close(da, a.grad)
    _close(db, b.grad)
    assert torch.isfinite(y).all() and torch.isfinite(db).all()
    o, bo = R.axpby_ref(a.detach(), 0.75, b.detach(), -1.5)
    _close(o, torch.add(0.75 * a.detach(), b.detach(), alpha=-1.5))
    o, bo = R.axpby_ref(a.detach(), 0.75, None, -1.5)
    _close(o, 0.75 * a.detach())


# ------------------------------------------------------------------------------------------------------------------- GDN parameters
@pytest.mark.parametrize("C", [3, 64])
def test_gdn_reparam_is_the_oracle_parametrizer(C):
    from oracle.leaves import GDN

    m = GDN(C).double()
    gb, bb = float(m.gamma_reparam.lower_bound.bound), float(m.beta_reparam.lower_bound.bound)
    ped = float(m.gamma_reparam.pedestal)
    assert ped == 2.0 ** -36 and gb == 2.0 ** -18 and float(m.beta_reparam.pedestal) == ped
    gamma, beta, dge, dbe = (t.double() for t in R.gdn_inputs(C, gb, bb))
    with torch.no_grad():
        m.gamma.copy_(gamma)
        m.beta.copy_(beta)
    ge, be = m.gamma_reparam(m.gamma), m.beta_reparam(m.beta)
    (ge * dge).sum().backward()
    (be * dbe).sum().backward()
    (rg, rgt, rb), _ = R.gdn_reparam_fwd_ref(gamma, beta, gb, bb, ped)
    _close(rg, ge.detach(), 0)
    _close(rgt, ge.detach().t(), 0)
    _close(rb, be.detach(), 0)
    dg, _, keep = R.gdn_reparam_bwd_ref(gamma, gb, dge)
    _close(dg, m.gamma.grad, 0)
    db, _, _ = R.gdn_reparam_bwd_ref(beta, bb, dbe)
    _close(db, m.beta.grad, 0)
    # the planted entries: at the bound everything passes; below it only negative gradients do
    flat, fk, fg = gamma.view(-1), keep.view(-1), dge.view(-1)
    assert bool(fk[flat == gb].all()) and int((flat == gb).sum()) >= 3
    below = flat < gb
    assert torch.equal(fk[below], fg[below] < 0) and int((below & (fg < 0)).sum()) and int((below & (fg > 0)).sum()) and int((below & (fg == 0)).sum())


# ------------------------------------------------------------------------------------------------------------------- loss
@pytest.mark.parametrize("grads", [(1.0, None, None), (None, 0.5, None), (None, None, 2.0), (1.0, -0.5, None), (0.25, None, 2.0),
                                   (None, 0.5, -2.0), (1.0, 0.5, 2.0)])
def test_rd_loss_is_the_oracle_loss(grads):
    from oracle.loss import RateDistortionLoss

    ly, lz = R.lik_inputs("small").double().requires_grad_(), R.lik_inputs("wide").double().requires_grad_()
    xh, tg = (t.double() for t in R.img_inputs())
    xh.requires_grad_()
    lmbda = 0.0067
    N, H, W, C = tg.shape
    c32 = float(torch.tensor(lmbda * 255 ** 2, dtype=torch.float32).double())
    nchw = lambda t: t.permute(0, 3, 1, 2)
    out = RateDistortionLoss(lmbda=c32 / 255 ** 2)({"x_hat": nchw(xh), "likelihoods": {"y": nchw(ly), "z": nchw(lz)}}, nchw(tg))
    bpp, mse, loss = R.rd_loss_ref(ly.detach(), lz.detach(), xh.detach(), tg, lmbda, N * H * W)
    _close(bpp, out["bpp_loss"].detach())
    _close(mse, out["mse_loss"].detach())
    _close(loss, out["loss"].detach())
    total = sum(g * out[k] for g, k in zip(grads, ("bpp_loss", "mse_loss", "loss")) if g is not None)
    total.backward()
    r = R.rd_grads_ref(ly.detach(), lz.detach(), xh.detach(), tg, lmbda, N * H * W, *grads)
    # (the kernels' 1 / ln 2 is a float32 argument: 3e-8 relative from the exact constant)
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    _close(r["dy"], zero(ly), 1e-7)
    _close(r["dz"], zero(lz), 1e-7)
    _close(r["dx"], zero(xh), 1e-12)
    s, b = R.sum_log2_ref(ly.detach())
    _close(s, (torch.log(ly.detach()) / math.log(2.0)).sum())
    s, b = R.sqdiff_sum_ref(xh.detach(), tg)
    _close(s, F.mse_loss(xh.detach(), tg, reduction="sum"))
    assert float(R.lik_inputs("small").min()) == float(torch.tensor(1e-9, dtype=torch.float32)) and float(R.lik_inputs("wide").max()) == 1.0


# ------------------------------------------------------------------------------------------------------------------- stem, patch rows, pooling
@pytest.mark.parametrize("co,cin", [(22, 3), (128, 3), (5, 1)])
def test_stem_pack_is_the_patch_row_filter(co, cin):
    """a 3x3 / stride-2 convolution and its 1x1 / stride-2 skip ARE the products of the 32-column patch rows with w1 and ws"""
    w3, w1x1 = R.rand(1, co, cin, 3, 3).double(), R.rand(2, co, cin, 1, 1).double()
    x = R.rand(3, 2, 9, 11, cin).double()
    w1, ws = R.stem_pack_ref(w3, w1x1)
    col = R.im2col_ref(x, 3, 2, 1, 32)
    _close(col @ w1.t(), F.conv2d(x.permute(0, 3, 1, 2), w3, stride=2, padding=1).permute(0, 2, 3, 1).reshape(-1, co))
    _close(col @ ws.t(), F.conv2d(x.permute(0, 3, 1, 2), w1x1, stride=2).permute(0, 2, 3, 1).reshape(-1, co))
    # the backward is the transpose
    dw1, dws = R.rand(4, co, 32).double(), R.rand(5, co, 32).double()
    g3, g1 = R.stem_unpack_ref(dw1, dws, cin)
    assert abs(float((g3 * w3).sum() + (g1 * w1x1).sum() - (dw1 * w1).sum() - (dws * ws).sum())) < 1e-9


@pytest.mark.parametrize("hw", [(9, 11), (1, 1)])
@pytest.mark.parametrize("case", R.IM2COL_CASES)
def test_im2col_is_unfold(case, hw):
    ks, stride, pad, C, ldc = case
    x = R.rand(6, 2, hw[0], hw[1], C).double()
    col = R.im2col_ref(x, ks, stride, pad, ldc)
    un = F.unfold(x.permute(0, 3, 1, 2), ks, padding=pad, stride=stride)      # [N, C ks ks, L] in (c, kh, kw) order
    N, L = un.shape[0], un.shape[2]
    un = un.reshape(N, C, ks * ks, L).permute(0, 3, 2, 1).reshape(N * L, ks * ks * C)
    assert torch.equal(col[:, : ks * ks * C], un) and float(col[:, ks * ks * C:].abs().sum()) == 0.0


@pytest.mark.parametrize("hw", [(7, 9), (1, 1)])
@pytest.mark.parametrize("case", R.POOL_CASES)
def test_maxpool_is_max_pool2d(case, hw):
    ks, stride, pad = case
    x = -R.uniform(7, 2, hw[0], hw[1], 4, lo=0.5, hi=2.0).double()
    if R.out_size(hw[0], ks, stride, pad) is None:
        with pytest.raises(RuntimeError):
            F.max_pool2d(x.permute(0, 3, 1, 2), ks, stride, pad)
        return
    want = F.max_pool2d(x.permute(0, 3, 1, 2), ks, stride, pad).permute(0, 2, 3, 1)
    assert torch.equal(R.maxpool_ref(x, ks, stride, pad), want)


@pytest.mark.parametrize("case", R.ADAPTIVE_CASES)
def test_adaptive_pool_is_torch(case):
    H, W, L = case
    x = -R.uniform(8, 2, H, W, 3, lo=0.5, hi=2.0).double()
    mx, _ = R.adaptive_pool_ref(x, L, True)
    av, bound = R.adaptive_pool_ref(x, L, False)
    assert torch.equal(mx, F.adaptive_max_pool2d(x.permute(0, 3, 1, 2), L))
    _close(av, F.adaptive_avg_pool2d(x.permute(0, 3, 1, 2), L))
    assert (bound > 0).all()


# ------------------------------------------------------------------------------------------------------------------- libm budgets
def _ratio(got32, ref, bound):
    return float(((got32.double() - ref).abs() / bound).max())


def _measure():
    """worst error / bound of each libm formula in float32 torch on the CPU, over the operands of the GPU cases"""
    m = {k: 0.0 for k in R.BUDGET}
    for C, rows in R.LN_FWD_SHAPES:
        t = R.ln_inputs(C, rows)
        f = R.ln_fwd_ref(t["x"].double(), t["gamma"].double(), t["beta"].double())
        y, mu, rs = R.ln_fwd_f32(t["x"], t["gamma"], t["beta"])
        m["ln_y"] = max(m["ln_y"], _ratio(y, f["y"], f["by"]))
        m["ln_rstd"] = max(m["ln_rstd"], _ratio(rs, f["rstd"], f["brstd"]))
    for rows, C in R.ACT_SHAPES + [(s[0] * 2 * s[1] * 2 * s[2], s[3] // 4) for s in R.UNSHUFFLE_SHAPES]:
        dy, saved = R.act_inputs(rows, C)
        dz, b = R.act_bwd_ref(dy.double(), saved.double(), R.ACT_HALFTANH, 1)
        m["halftanh_pre"] = max(m["halftanh_pre"], _ratio(R.halftanh_pre_f32(dy, saved), dz, b))
        dz, b = R.act_bwd_ref(dy.double(), saved.double(), R.ACT_GELU, 1)
        m["gelu"] = max(m["gelu"], _ratio(R.gelu_grad_f32(dy, saved), dz, b))
    for inputs in [R.gate_inputs(n) for n in R.GATE_N] + [R.gate_inputs_neg()]:
        a, b, idn, g = inputs
        y, by = R.gate_fwd_ref(a.double(), b.double(), idn.double())
        da, bda, db, bdb = R.gate_bwd_ref(g.double(), a.double(), b.double())
        m["gate_fwd"] = max(m["gate_fwd"], _ratio(R.gate_fwd_f32(a, b, idn), y, by))
        da32, db32 = R.gate_bwd_f32(g, a, b)
        m["gate_da"] = max(m["gate_da"], _ratio(da32, da, bda))
        m["gate_db"] = max(m["gate_db"], _ratio(db32, db, bdb))
    for k in R.LIK_SHAPES:
        lik = R.lik_inputs(k)
        t, b = R.log2_term_ref(lik.double())
        m["log2"] = max(m["log2"], _ratio(torch.log2(lik), t, b))
    return m


def test_libm_budgets_are_eight_times_the_float32_cpu_error():
    m = _measure()
    for k, v in sorted(m.items()):
        print(f"libm budget {k}: float32 CPU error / bound = {v:.4f}, 8 x = {8 * v:.4f}, BUDGET = {R.BUDGET[k]}")
    for k, v in m.items():
        assert 8 * v <= R.BUDGET[k], (k, v, R.BUDGET[k])
        assert R.BUDGET[k] <= 16 * v, f"{k}: the budget {R.BUDGET[k]} is more than 16 x the measurement {v}"
