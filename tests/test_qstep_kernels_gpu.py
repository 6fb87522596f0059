"""The quantisation-step kernels (csrc/qstep.hip) through the C ABI, on [rows, C] maps:

    (1, 1), (3, 5), (257, 4) — crosses a 256-thread block —, (64, 192), and (130, 192) read and written through channel slices of wider
    buffers (ld = C + 64; the bytes around every slice are sentinels and must survive),

steps mixed per channel from {0.25, 1.0, 3.7}.  With step == 1 every output equals the unit-step kernel's bit for bit; likelihood and
gradients are held to the float64 specification (tests/qstep_ref.py) at the tolerances of tests/test_kernels_gpu.py::
test_gaussian_likelihood — 1e-5 of the largest likelihood, 2e-3 in the log domain, 2e-4 of the largest gradient; dstep to the float64
per-channel sum within 2e-4 of the float64 sum of the absolute per-element contributions (rows terms, each within the per-element
tolerance of its own size); the integer path to an f32 numpy restatement of its one expression, every element; the rate sweep to its
two identities bit for bit and to n x 2e-3 bits of the float64 sum.

The float64 reference and the f32 kernel must agree on the symbol round((y - mu) / step), so the random latents keep (y - mu) / step at
least 1e-3 away from a tie; exact ties are the integer-path test's subject, where both sides are f32.
The lanes decoder with a step (clc_rans_lanes_decode_gauss_step) follows tests/test_rans_lanes_gauss_kernels_gpu.py: host-encoded words,
sentinel words around every buffer; B = 2, W in {1, 4}, n = 64 W - 1 and 64 W + 1 symbols per image as whole rows of C channels
(63 = 9 x 7, 65 = 13 x 5, 255 = 51 x 5, 257 = 1 x 257).
"""
import numpy as np
import pytest
import torch

import qstep_ref as R

pytestmark = pytest.mark.gpu

CASES = [(1, 1, False), (3, 5, False), (257, 4, False), (64, 192, False), (130, 192, True)]
IDS = ["1x1", "3x5", "257x4", "64x192", "130x192-sliced"]
STEPS = (0.25, 1.0, 3.7)
PAD, SENTINEL = 32, -777.25


def _api():
    from clc_amd import lib, ops

    return lib.load(), lib, ops._stream()


class _Map:
    """a [rows, C] device map, dense or a channel slice of a [rows, C + 2 PAD] buffer of sentinels"""

    def __init__(self, rows, C, wide, dev, src=None, dtype=torch.float32):
        self.wide, self.C = wide, C
        self.buf = torch.full((rows, C + 2 * PAD if wide else C), SENTINEL, device=dev, dtype=dtype)
        self.view = self.buf[:, PAD:PAD + C] if wide else self.buf
        if src is not None:
            self.view.copy_(src.to(dev))
        self.ptr, self.ld = self.view.data_ptr(), self.buf.shape[1]

    def get(self):
        if self.wide:
            assert bool((self.buf[:, :PAD] == SENTINEL).all()) and bool((self.buf[:, PAD + self.C:] == SENTINEL).all()), "wrote outside the slice"
        return self.view.cpu().clone()


def _steps(C, unit=False):
    return torch.tensor([1.0 if unit else STEPS[c % 3] for c in range(C)], dtype=torch.float32)


def _latent(rows, C, seed):
    g = torch.Generator().manual_seed(seed)
    step = _steps(C)
    mu = torch.randn((rows, C), generator=g)
    scale = torch.randn((rows, C), generator=g) + 0.5      # some below the bound 0.11, some negative
    t = torch.randn((rows, C), generator=g) * 3
    frac = t - torch.floor(t)
    t = torch.where((frac - 0.5).abs() < 1e-3, t + 0.01, t)   # away from the ties (see the module docstring)
    y = mu + t * step
    noise = torch.rand((rows, C), generator=g) - 0.5
    w = torch.rand((rows, C), generator=g) - 0.7           # mixed-sign upstream gradients (the LowerBound rule)
    gh = torch.randn((rows, C), generator=g)
    return {"y": y, "mu": mu, "scale": scale, "noise": noise, "w": w, "gh": gh, "step": step}


def _fwd(dev, d, step, rows, C, wide, training, with_step=True, partials=False):
    L, lib, st = _api()
    m = {k: _Map(rows, C, wide, dev, d[k]) for k in ("y", "mu", "scale", "noise")}
    lik, yh = _Map(rows, C, wide, dev), _Map(rows, C, wide, dev)
    nb = L.clc_gauss_lik_partials(rows, C)
    part = torch.zeros(nb, device=dev)
    sd = step.to(dev)
    npn, ldn = (m["noise"].ptr, m["noise"].ld) if training else (None, 0)
    pp, pn = (part.data_ptr(), nb) if partials else (None, 0)
    if with_step:
        lib.check(L.clc_gauss_lik_step_fwd(m["y"].ptr, m["y"].ld, m["mu"].ptr, m["mu"].ld, m["scale"].ptr, m["scale"].ld, npn, ldn, sd.data_ptr(),
                                           lik.ptr, lik.ld, yh.ptr, yh.ld, rows, C, 0 if training else 1, pp, pn, st), "clc_gauss_lik_step_fwd")
    else:
        lib.check(L.clc_gauss_lik_fwd(m["y"].ptr, m["y"].ld, m["mu"].ptr, m["mu"].ld, m["scale"].ptr, m["scale"].ld, npn, ldn,
                                      lik.ptr, lik.ld, yh.ptr, yh.ld, rows, C, 0 if training else 1, pp, pn, st), "clc_gauss_lik_fwd")
    return lik.get(), yh.get(), part.cpu()


def _bwd(dev, d, step, rows, C, wide, training, with_step=True, hat=True):
    L, lib, st = _api()
    m = {k: _Map(rows, C, wide, dev, d[k]) for k in ("y", "mu", "scale", "noise", "w", "gh")}
    dy, dmu, dsc = (_Map(rows, C, wide, dev) for _ in range(3))
    npn, ldn = (m["noise"].ptr, m["noise"].ld) if training else (None, 0)
    hp, ldh = (m["gh"].ptr, m["gh"].ld) if hat else (None, 0)
    dyp, dmp = (dy.ptr, dmu.ptr) if training else (None, None)
    dstep = torch.full((C,), SENTINEL, device=dev)
    if with_step:
        sd = step.to(dev)
        nbytes = L.clc_gauss_lik_step_bwd_workspace_bytes(rows, C)
        assert nbytes > 0 and nbytes % 4 == 0
        ws = torch.full((nbytes // 4 + 8,), SENTINEL, device=dev)
        lib.check(L.clc_gauss_lik_step_bwd(m["w"].ptr, m["w"].ld, m["y"].ptr, m["y"].ld, m["mu"].ptr, m["mu"].ld, m["scale"].ptr, m["scale"].ld, npn, ldn,
                                           sd.data_ptr(), dyp, dy.ld, dmp, dmu.ld, dsc.ptr, dsc.ld, dstep.data_ptr(), rows, C, 0 if training else 1,
                                           hp, ldh, ws.data_ptr(), nbytes, st), "clc_gauss_lik_step_bwd")
        assert bool((ws[nbytes // 4:] == SENTINEL).all()), "wrote past the workspace"
    else:
        lib.check(L.clc_gauss_lik_bwd(m["w"].ptr, m["w"].ld, m["y"].ptr, m["y"].ld, m["mu"].ptr, m["mu"].ld, m["scale"].ptr, m["scale"].ld, npn, ldn,
                                      dyp, dy.ld, dmp, dmu.ld, dsc.ptr, dsc.ld, rows, C, 0 if training else 1, hp, ldh, st), "clc_gauss_lik_bwd")
    return dy.get(), dmu.get(), dsc.get(), dstep.cpu()


def _table(dev):
    from clc_amd.models.clc import get_scale_table

    return torch.tensor([float(s) for s in get_scale_table()], dtype=torch.float32, device=dev)


def _qbi(dev, y, mu, scale, step, rows, C, wide, with_step=True):
    L, lib, st = _api()
    table = _table(dev)
    my, mm, ms = (_Map(rows, C, wide, dev, t) for t in (y, mu, scale))
    yh = _Map(rows, C, wide, dev)
    sym = torch.full((rows, C), -12345, device=dev, dtype=torch.int32)
    idx = torch.full((rows, C), -12345, device=dev, dtype=torch.int32)
    if with_step:
        sd = step.to(dev)
        lib.check(L.clc_quantize_build_indexes_step(my.ptr, my.ld, mm.ptr, mm.ld, ms.ptr, ms.ld, sd.data_ptr(), table.data_ptr(), table.numel(),
                                                    sym.data_ptr(), idx.data_ptr(), yh.ptr, yh.ld, rows, C, st), "clc_quantize_build_indexes_step")
    else:
        lib.check(L.clc_quantize_build_indexes(my.ptr, my.ld, mm.ptr, mm.ld, ms.ptr, ms.ld, table.data_ptr(), table.numel(),
                                               sym.data_ptr(), idx.data_ptr(), yh.ptr, yh.ld, rows, C, st), "clc_quantize_build_indexes")
    return sym.cpu().numpy(), idx.cpu().numpy(), yh.get().numpy()


def _bits(a):
    return a.contiguous().view(torch.int32)


# ---- step == 1: the unit-step kernels' bits ----

@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_unit_step_is_bit_equal_to_the_unit_step_kernels(dev, case):
    rows, C, wide = case
    d = _latent(rows, C, 11)
    one = _steps(C, unit=True)
    for training in (False, True):
        a = _fwd(dev, d, one, rows, C, wide, training, True, partials=True)
        b = _fwd(dev, d, one, rows, C, wide, training, False, partials=True)
        for x, y_, what in zip(a, b, ("lik", "y_hat", "bits_partial")):
            assert torch.equal(_bits(x), _bits(y_)), (what, training)
        a = _bwd(dev, d, one, rows, C, wide, training, True)
        b = _bwd(dev, d, one, rows, C, wide, training, False)
        for x, y_, what in zip(a[:3], b[:3], ("dy", "dmu", "dscale")):
            assert torch.equal(_bits(x), _bits(y_)), (what, training)
    y = d["y"].clone()
    y[0, 0] = d["mu"][0, 0] + 0.5     # a tie, and a -0 symbol
    if rows > 2:
        y[1, 0] = d["mu"][1, 0] - 0.25
    a = _qbi(dev, y, d["mu"], d["scale"].abs() * 40, one, rows, C, wide, True)
    b = _qbi(dev, y, d["mu"], d["scale"].abs() * 40, one, rows, C, wide, False)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))


# ---- against the float64 specification ----

def _reference(d, training):
    """float64: (lik, y_hat, dy, dmu, dscale, dstep, sum of |per-element dstep contributions| per channel)"""
    y, mu, sc = (d[k].double().requires_grad_() for k in ("y", "mu", "scale"))
    step = d["step"].double().requires_grad_()
    noise = d["noise"].double() if training else None
    lik, yh = R.forward(y, mu, sc, step, noise)
    ((lik * d["w"].double()).sum() + (yh * d["gh"].double()).sum()).backward()
    # the per-element contributions to dstep: the gradient of each element's own terms with respect to a step of its own
    se = d["step"].double().expand_as(y).clone().requires_grad_()
    lik_e, yh_e = R.forward(y.detach(), mu.detach(), sc.detach(), se, noise)
    ((lik_e * d["w"].double()).sum() + (yh_e * d["gh"].double()).sum()).backward()
    assert torch.allclose(se.grad.sum(0), step.grad, rtol=1e-10, atol=1e-12)
    return lik.detach(), yh.detach(), y.grad, mu.grad, sc.grad, step.grad, se.grad.abs().sum(0)


def _rel(a, b):
    return (a.double() - b).abs().max().item() / max(b.abs().max().item(), 1e-6)


@pytest.mark.parametrize("training", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_likelihood_and_gradients_against_float64(dev, case, training):
    rows, C, wide = case
    d = _latent(rows, C, 5)
    lik64, yh64, dy64, dmu64, dsc64, dstep64, abs64 = _reference(d, training)
    lik, yh, _ = _fwd(dev, d, d["step"], rows, C, wide, training)
    e_lik, e_log = _rel(lik, lik64), (torch.log(lik.double()) - torch.log(lik64)).abs().max().item()
    print(f"lik rel {e_lik:.3e}  log {e_log:.3e}")
    assert e_lik <= 1e-5 and e_log < 2e-3
    # y_hat: the f32 expression, bit for bit (the float64 value only to its rounding)
    want = R.dequantise(np.rint(((d["y"] - d["mu"]) / d["step"]).numpy()), d["mu"].numpy(), d["step"].numpy())
    assert np.array_equal(yh.numpy().view(np.uint32), want.view(np.uint32))
    assert (yh.double() - yh64).abs().max().item() <= 1e-5
    dy, dmu, dsc, dstep = _bwd(dev, d, d["step"], rows, C, wide, training)
    e = {"dscale": _rel(dsc, dsc64)}
    if training:
        e["dy"], e["dmu"] = _rel(dy, dy64), _rel(dmu, dmu64)   # (dy includes the straight-through gradient of y_hat, as the reference's)
    else:
        # eval: y reaches the loss through y_hat only (the reference's step * (g / step) is g to a rounding)
        assert torch.allclose(dy64, d["gh"].double(), rtol=1e-12, atol=0) and float(dmu64.abs().max()) <= 1e-12
    print("gradients rel", {k: f"{v:.3e}" for k, v in e.items()})
    assert all(v <= 2e-4 for v in e.values()), e
    tol = 2e-4 * abs64
    err = (dstep.double() - dstep64).abs()
    worst = float((err / abs64.clamp(min=1e-300)).max())
    print(f"dstep: worst |error| / sum |contributions| = {worst:.3e} (bound 2e-4)")
    assert bool((err <= tol).all()), (err, tol)
    again = _bwd(dev, d, d["step"], rows, C, wide, training)[3]
    assert torch.equal(_bits(again), _bits(dstep)), "dstep differs run to run"
    # without the upstream gradient of y_hat its path is absent
    no_hat = _bwd(dev, d, d["step"], rows, C, wide, training, hat=False)[3]
    d0 = dict(d, gh=torch.zeros_like(d["gh"]))
    assert torch.equal(_bits(no_hat), _bits(_bwd(dev, d0, d["step"], rows, C, wide, training)[3]))


# ---- the integer path ----

@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_integer_path_every_element(dev, case):
    rows, C, wide = case
    g = torch.Generator().manual_seed(9)
    step = _steps(C)
    table = _table(dev).cpu().numpy()
    mu = torch.randn((rows, C), generator=g)
    mu[::3] = 0.0      # with a zero mean (y - mu) / step is exact: the ties below are exact ties
    mu[1::6] = -0.0
    scale = torch.rand((rows, C), generator=g) * 8
    y = mu + torch.randn((rows, C), generator=g) * 6
    # even rows: y at an edge offset from mu, in units of the channel's step (-0.25: the symbol is negative zero); odd rows: an edge scale.
    # Every edge meets every step where the map is large enough; small maps take what fits.
    edge_y = torch.tensor([0.5, -0.5, -0.25, 1.5, 2.5, -1.5, 0.49999997, 1e-30, -1e-30, 300.0, -0.0, 0.25])
    edge_s = torch.tensor([0.05, -3.0, 0.11, 0.02, 0.0275, 1e-4, 250.0, 1000.0, float("inf"), float("nan"), 0.1100001, 64.0])
    n = rows * C
    r = torch.arange(rows).reshape(rows, 1).expand(rows, C)
    c = torch.arange(C).reshape(1, C).expand(rows, C)
    even = r % 2 == 0
    y = torch.where(even, mu + edge_y[(r // 2 + c) % len(edge_y)] * step, y)
    scale = torch.where(~even, edge_s[(r // 2 + c) % len(edge_s)], scale)
    sym, idx, yh = _qbi(dev, y, mu, scale, step, rows, C, wide)
    w_sym, w_idx, w_yh = R.integer_path(y.numpy(), mu.numpy(), scale.numpy(), step.numpy(), table)
    assert np.array_equal(sym, w_sym)
    assert np.array_equal(idx, w_idx)
    assert np.array_equal(yh.view(np.uint32), w_yh.view(np.uint32)), "y_hat bits (negative zero included)"
    if n >= 600:   # the rows the text names are all there
        q = np.fmax(scale.numpy(), np.float32(0.11)) / step.numpy()
        assert (idx[q < table[0]] == 0).all() and (q < table[0]).any()
        assert (idx[q > table[-1]] == len(table) - 1).all() and (q > table[-1]).any()
        nan = np.isnan(scale.numpy())
        assert nan.any() and np.array_equal(idx[nan], R.scale_index(np.float32(0.11) / np.broadcast_to(step.numpy(), scale.shape)[nan], table))


# ---- the rate sweep ----

def _sweep(dev, y, mu, scale, steps, B, n_rows, C, wide):
    L, lib, st = _api()
    my, mm, ms = (_Map(B * n_rows, C, wide, dev, t) for t in (y, mu, scale))
    K = steps.shape[0]
    sd = steps.contiguous().to(dev)
    bits = torch.full((B, K), SENTINEL, device=dev)
    nbytes = L.clc_gauss_rate_sweep_workspace_bytes(B, n_rows, C, K)
    assert nbytes > 0 and nbytes % 4 == 0
    ws = torch.full((nbytes // 4 + 8,), SENTINEL, device=dev)
    lib.check(L.clc_gauss_rate_sweep(my.ptr, my.ld, mm.ptr, mm.ld, ms.ptr, ms.ld, sd.data_ptr(), K, B, n_rows, C, bits.data_ptr(), ws.data_ptr(),
                                     nbytes, st), "clc_gauss_rate_sweep")
    assert bool((ws[nbytes // 4:] == SENTINEL).all()), "wrote past the workspace"
    return bits.cpu()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_rate_sweep_identities_and_float64(dev, case):
    n_rows, C, wide = case
    B, K = 3, 16
    d = _latent(B * n_rows, C, 21)
    g = torch.Generator().manual_seed(22)
    steps = torch.stack([_steps(C)] + [torch.exp((torch.rand(C, generator=g) - 0.5) * 3.0) for _ in range(K - 2)] + [_steps(C, unit=True)])
    for _ in range(20):   # no candidate's (y - mu) / step within 1e-4 of a tie (the module docstring): such an element moves on
        t = (d["y"] - d["mu"]).unsqueeze(0) / steps.unsqueeze(1)
        near = (((t - torch.floor(t)) - 0.5).abs() < 1e-4).any(0)
        if not bool(near.any()):
            break
        d["y"] = torch.where(near, d["y"] + 0.0137, d["y"])
    assert not bool(near.any())
    bits = _sweep(dev, d["y"], d["mu"], d["scale"], steps, B, n_rows, C, wide)
    for k in (0, 7, K - 1):   # column k of the K-wide call = the K = 1 call with that candidate
        one = _sweep(dev, d["y"], d["mu"], d["scale"], steps[k:k + 1], B, n_rows, C, wide)
        assert torch.equal(_bits(one[:, 0]), _bits(bits[:, k])), k
    assert torch.equal(_bits(_sweep(dev, d["y"], d["mu"], d["scale"], steps[:5], B, n_rows, C, wide)), _bits(bits[:, :5]))
    for b in range(B):        # image b alone = image b of the batch
        rows = slice(b * n_rows, (b + 1) * n_rows)
        alone = _sweep(dev, d["y"][rows], d["mu"][rows], d["scale"][rows], steps, 1, n_rows, C, wide)
        assert torch.equal(_bits(alone[0]), _bits(bits[b])), b
    shape = (B, n_rows, C)
    want = R.rate_bits(d["y"].double().reshape(shape), d["mu"].double().reshape(shape), d["scale"].double().reshape(shape), steps.double())
    err = (bits.double() - want).abs().max().item()
    print(f"rate sweep: worst |bits - float64| = {err:.3e} of a bound {n_rows * C * 2e-3:.3e} (n = {n_rows * C})")
    assert err <= n_rows * C * 2e-3
    # the last column is the unit step: the sum of the eval forward's log2 likelihoods, within the same tolerance
    lik, _, _ = _fwd(dev, {k: v[:n_rows] for k, v in d.items() if k != "step"}, steps[K - 1], n_rows, C, wide, False)
    assert abs(float(-torch.log2(lik.double()).sum()) - float(bits[0, K - 1])) <= n_rows * C * 2e-3


# ---- the wrappers and the refusals ----

def test_autograd_wrapper_matches_the_raw_kernels(dev):
    from clc_amd import ops

    rows, C = 130, 192
    d = _latent(rows, C, 5)
    to4 = lambda t: t.reshape(1, rows, 1, C).permute(0, 3, 1, 2).to(dev)
    for training in (False, True):
        y, mu, sc = (to4(d[k]).requires_grad_() for k in ("y", "mu", "scale"))
        step = d["step"].to(dev).requires_grad_()
        lik, yh = ops.gaussian_likelihood_step(y, sc, mu, step, to4(d["noise"]) if training else None, training)
        ((lik * to4(d["w"])).sum() + (yh * to4(d["gh"])).sum()).backward()
        raw_f = _fwd(dev, d, d["step"], rows, C, False, training)
        raw_b = _bwd(dev, d, d["step"], rows, C, False, training)
        back = lambda t: t.detach().permute(0, 2, 3, 1).reshape(rows, C).cpu()
        assert torch.equal(back(lik), raw_f[0]) and torch.equal(back(yh), raw_f[1])
        assert torch.equal(step.grad.cpu(), raw_b[3]) and torch.equal(back(sc.grad), raw_b[2])
        if training:
            assert torch.equal(back(y.grad), raw_b[0]) and torch.equal(back(mu.grad), raw_b[1])
        else:
            assert torch.equal(back(y.grad), d["gh"]) and (mu.grad is None or float(mu.grad.abs().max()) == 0.0)
    sym, idx, yh = ops.quantize_build_indexes_step(to4(d["y"]), to4(d["mu"]), to4(d["scale"]), _table(dev), d["step"].to(dev))
    raw = _qbi(dev, d["y"], d["mu"], d["scale"], d["step"], rows, C, False)
    assert np.array_equal(sym.permute(0, 2, 3, 1).reshape(rows, C).cpu().numpy(), raw[0])
    assert np.array_equal(idx.permute(0, 2, 3, 1).reshape(rows, C).cpu().numpy(), raw[1])
    steps = torch.stack([d["step"], _steps(C, unit=True)]).to(dev)
    to4b = lambda t: t.reshape(2, 65, 1, C).permute(0, 3, 1, 2).to(dev)
    got = ops.gauss_rate_sweep(to4b(d["y"]), to4b(d["mu"]), to4b(d["scale"]), steps)
    assert torch.equal(got.cpu(), _sweep(dev, d["y"], d["mu"], d["scale"], steps.cpu(), 2, 65, C, False))


def test_c_abi_refuses_bad_arguments_by_name(dev):
    L, lib, st = _api()
    t = torch.zeros(64, device=dev)
    i32 = torch.zeros(64, device=dev, dtype=torch.int32)
    p = t.data_ptr()

    def refused(rc, text):
        assert rc < 0 and text in L.clc_last_error().decode(), (rc, L.clc_last_error())

    refused(L.clc_gauss_lik_step_fwd(p, 4, p, 4, p, 4, None, 0, None, p, 4, p, 4, 4, 4, 1, None, 0, st), "clc_gauss_lik_step_fwd: step is NULL")
    refused(L.clc_gauss_lik_step_fwd(p, 4, p, 4, p, 4, None, 0, p, p, 4, p, 4, 4, 4, 0, None, 0, st), "training mode needs noise")
    refused(L.clc_gauss_lik_step_fwd(p, 4, p, 3, p, 4, None, 0, p, p, 4, p, 4, 4, 4, 1, None, 0, st), "a leading dimension is below C = 4")
    refused(L.clc_gauss_lik_step_fwd(p, 4, p, 4, p, 4, None, 0, p, p, 4, p, 4, 4, 4, 2, None, 0, st), "mode must be 0 (training) or 1 (eval)")
    refused(L.clc_gauss_lik_step_fwd(p, 4, p, 4, p, 4, None, 0, p, p, 4, p, 4, 4, 4, 1, p, 7, st), "n_partials must be clc_gauss_lik_partials() = 1")
    need = L.clc_gauss_lik_step_bwd_workspace_bytes(4, 4)
    assert need == 16 and L.clc_gauss_lik_step_bwd_workspace_bytes(0, 4) == 0 and "rows and C must be positive" in L.clc_last_error().decode()
    refused(L.clc_gauss_lik_step_bwd(p, 4, p, 4, p, 4, p, 4, None, 0, p, None, 0, None, 0, p, 4, None, 4, 4, 1, None, 0, p, need, st), "step or dstep is NULL")
    refused(L.clc_gauss_lik_step_bwd(p, 4, p, 4, p, 4, p, 4, None, 0, p, None, 0, None, 0, p, 4, p, 4, 4, 1, None, 0, p, need - 1, st), "ws_bytes >= clc_gauss_lik_step_bwd_workspace_bytes() = 16")
    refused(L.clc_gauss_lik_step_bwd(p, 4, p, 4, p, 4, p, 4, None, 0, p, None, 0, None, 0, p, 4, p, 4, 4, 1, p, 2, p, need, st), "a leading dimension is below C = 4")
    refused(L.clc_quantize_build_indexes_step(p, 4, p, 4, p, 4, None, p, 8, i32.data_ptr(), i32.data_ptr(), p, 4, 4, 4, st), "clc_quantize_build_indexes_step: step is NULL")
    refused(L.clc_quantize_build_indexes_step(p, 4, p, 4, p, 4, p, p, 257, i32.data_ptr(), i32.data_ptr(), p, 4, 4, 4, st), "n_scales must be between 2 and 256 (got 257)")
    assert L.clc_gauss_rate_sweep_workspace_bytes(1, 4, 4, 17) == 0 and "K 1 .. 16" in L.clc_last_error().decode()
    ws_need = L.clc_gauss_rate_sweep_workspace_bytes(1, 4, 4, 2)
    assert ws_need == 8
    refused(L.clc_gauss_rate_sweep(p, 4, p, 4, p, 4, p, 17, 1, 4, 4, p, p, 256, st), "K must be 1 .. 16 candidates (got 17)")
    refused(L.clc_gauss_rate_sweep(p, 4, p, 4, p, 4, p, 0, 1, 4, 4, p, p, 256, st), "K must be 1 .. 16 candidates (got 0)")
    refused(L.clc_gauss_rate_sweep(p, 4, p, 4, p, 4, None, 2, 1, 4, 4, p, p, 256, st), "steps or bits is NULL")
    refused(L.clc_gauss_rate_sweep(p, 4, p, 4, p, 2, p, 2, 1, 4, 4, p, p, 256, st), "a leading dimension is below C = 4")
    refused(L.clc_gauss_rate_sweep(p, 4, p, 4, p, 4, p, 2, 1, 4, 4, p, p, ws_need - 4, st), "ws_bytes >= clc_gauss_rate_sweep_workspace_bytes() = 8")
    refused(L.clc_gauss_rate_sweep(p, 4, p, 4, p, 4, p, 2, 0, 4, 4, p, p, 256, st), "B must be 1 .. 65535")


# ---- the lanes decoder with a step ----

LANES_CASES = [(1, 9, 7), (1, 13, 5), (4, 51, 5), (4, 1, 257)]   # (W, pixels, C): n = pixels x C = 64 W -+ 1


def _framed(vals, B, pix, C, dev):
    """float [B, pix, C] (or None) -> (the flat buffer: 256 sentinels | [B, pix, C + 2] with sentinel padding columns | 256 sentinels,
    its logical [B, C, pix, 1] pixel-major view of leading dimension C + 2)"""
    ld, pad = C + 2, 256
    flat = torch.full((2 * pad + B * pix * ld,), SENTINEL, dtype=torch.float32)
    if vals is not None:
        flat[pad:pad + B * pix * ld].view(B, pix, ld)[..., :C] = torch.from_numpy(vals)
    flat = flat.to(dev)
    return flat, flat[pad:pad + B * pix * ld].view(B, pix, 1, ld).permute(0, 3, 1, 2)[:, :C]


def _unframed(flat, B, pix, C):
    ld, pad = C + 2, 256
    got = flat.cpu()
    body = got[pad:pad + B * pix * ld].view(B, pix, ld)
    assert (got[:pad] == SENTINEL).all() and (got[pad + B * pix * ld:] == SENTINEL).all() and (body[..., C:] == SENTINEL).all()
    return body[..., :C].reshape(B, pix * C).clone()


@pytest.mark.parametrize("W,pix,C", LANES_CASES, ids=[f"W{w}-n{p * c}" for w, p, c in LANES_CASES])
def test_lanes_decoder_with_a_step(dev, W, pix, C):
    from clc_amd import ans, ops
    from clc_amd.entropy_models import GaussianConditional
    from test_rans_lanes_kernels_gpu import SENT, _final, _lay_out

    B, n = 2, pix * C
    assert n in (64 * W - 1, 64 * W + 1)
    gc = GaussianConditional([float(s) for s in np.geomspace(0.11, 64.0, 8)])
    gc.update()
    (cdf, ln, off), table = gc.host_tables(), gc.scale_table.detach().float().cpu().numpy().copy()
    tdev = torch.from_numpy(table).to(dev)
    tables = tuple(torch.from_numpy(t).to(dev) for t in (cdf, ln, off))
    g = np.random.default_rng(100 + n)
    scale = np.exp(g.uniform(np.log(0.03), np.log(300.0), (B, pix, C))).astype(np.float32)
    scale.reshape(-1)[::9] = np.resize(np.float32([0.05, 0.0, -3.0, 0.11, 1e30, np.inf, 0.0275, 64.0]), scale.reshape(-1)[::9].size)
    mu = (g.uniform(-4.0, 4.0, (B, pix, C)) + 0.37).astype(np.float32)
    y = (mu + g.normal(0.0, 1.0, (B, pix, C)) * np.minimum(np.abs(scale) + 0.1, 50.0)).astype(np.float32)
    y.reshape(-1)[3::17] += 1e5       # escapes with several payload nibbles
    y.reshape(-1)[5::19] -= 1e5
    y[:, -1, -1] = mu[:, -1, -1] + np.float32([1e6, -1e6])   # one in the partial chunk
    step = _steps(C).to(dev)
    _, sc_v = _framed(scale, B, pix, C, dev)
    _, mu_v = _framed(mu, B, pix, C, dev)
    _, y_v = _framed(y, B, pix, C, dev)
    nhwc = lambda t: t.permute(0, 2, 3, 1).reshape(B, n)
    sym, idx, want = (nhwc(t) for t in ops.quantize_build_indexes_step(y_v, mu_v, sc_v, tdev, step))
    sym, idx = sym.cpu().numpy(), idx.cpu().numpy()
    w_sym, w_idx, w_yh = R.integer_path(y.reshape(B * pix, C), mu.reshape(B * pix, C), scale.reshape(B * pix, C), step.cpu().numpy(), table)
    assert np.array_equal(sym.reshape(-1), w_sym.reshape(-1)) and np.array_equal(idx.reshape(-1), w_idx.reshape(-1))
    assert len(set(idx.reshape(-1).tolist())) >= 6
    host = [ans.lanes_encode(sym[b], idx[b], [n], W, cdf, ln, off) for b in range(B)]

    def run(step_arg):
        words, spans, state = _lay_out(host, dev)
        yh_flat, yh_v = _framed(None, B, pix, C, dev)
        sb = torch.full((B, n + 16), -SENT, device=dev, dtype=torch.int32)
        keep = (words.clone(), spans.clone())
        out = ops.rans_lanes_decode_gauss(sc_v, mu_v, tdev, tables, words, spans, state, y_hat=yh_v, symbols=sb, step=step_arg)
        assert out.data_ptr() == yh_v.data_ptr() and torch.equal(words, keep[0]) and torch.equal(spans, keep[1])
        assert torch.equal(sb[:, n:], torch.full((B, 16), -SENT, device=dev, dtype=torch.int32))
        return _unframed(yh_flat, B, pix, C), sb[:, :n].cpu().numpy(), state

    y_hat, got_sym, state = run(step)
    assert np.array_equal(got_sym, sym)
    assert torch.equal(_bits(y_hat), _bits(want.cpu())), "the decoder's y_hat is not the encoder's"
    assert np.array_equal(y_hat.numpy().view(np.uint32).reshape(-1), w_yh.view(np.uint32).reshape(-1))
    x, pos = _final(state)
    for b in range(B):
        d = ans.LanesDecoder(host[b])
        assert np.array_equal(d.decode(idx[b], cdf, ln, off), sym[b])
        for w in range(W):
            hx, hpos = d.state(w)
            assert np.array_equal(hx, x[b, w]) and hpos == int(pos[b, w]), (b, w)
    assert (x == np.uint64(1 << 31)).all() and pos.tolist() == [[len(s) // 4 for s in img] for img in host]
    # step == 1: the unit-step kernel's bits, on the same (now mismatched) words — whatever they decode to
    one = run(torch.ones(C, device=dev))
    unit = run(None)
    assert torch.equal(_bits(one[0]), _bits(unit[0])) and np.array_equal(one[1], unit[1]) and torch.equal(one[2], unit[2])
    with pytest.raises(ValueError, match=rf"rans_lanes_decode_gauss: step must have shape \[{C}\]"):
        run(torch.ones(C + 1, device=dev))


def test_lanes_stream_grows_with_a_finer_step(dev):
    """A latent large enough for the lanes to shed words (B = 2, W = 4, n = 128 x 48 = 6144: 24 symbols per lane of 2.6 bits at step 2 and
    4.6 bits at step 0.5, scales around 3): the host-encoded lanes stream of the step-0.5 symbols is strictly longer than that of the
    step-2 symbols, image by image, and the device decoder returns each encoder's y_hat under its own step."""
    from clc_amd import ans, ops
    from clc_amd.entropy_models import GaussianConditional
    from test_rans_lanes_kernels_gpu import _final, _lay_out

    B, W, pix, C = 2, 4, 128, 48
    n = pix * C
    gc = GaussianConditional([float(s) for s in np.geomspace(0.11, 64.0, 8)])
    gc.update()
    (cdf, ln, off), table = gc.host_tables(), gc.scale_table.detach().float().cpu().numpy().copy()
    tdev = torch.from_numpy(table).to(dev)
    tables = tuple(torch.from_numpy(t).to(dev) for t in (cdf, ln, off))
    g = np.random.default_rng(4)
    scale = np.exp(g.uniform(np.log(2.0), np.log(4.5), (B, pix, C))).astype(np.float32)
    mu = g.uniform(-4.0, 4.0, (B, pix, C)).astype(np.float32)
    y = (mu + g.normal(0.0, 1.0, (B, pix, C)) * scale).astype(np.float32)
    _, sc_v = _framed(scale, B, pix, C, dev)
    _, mu_v = _framed(mu, B, pix, C, dev)
    _, y_v = _framed(y, B, pix, C, dev)
    nhwc = lambda t: t.permute(0, 2, 3, 1).reshape(B, n)
    sizes = {}
    for s in (2.0, 0.5):
        step = torch.full((C,), s, device=dev)
        sym, idx, want = (nhwc(t) for t in ops.quantize_build_indexes_step(y_v, mu_v, sc_v, tdev, step))
        sym, idx = sym.cpu().numpy(), idx.cpu().numpy()
        host = [ans.lanes_encode(sym[b], idx[b], [n], W, cdf, ln, off) for b in range(B)]
        sizes[s] = [sum(len(w) for w in img) for img in host]
        words, spans, state = _lay_out(host, dev)
        yh_flat, yh_v = _framed(None, B, pix, C, dev)
        ops.rans_lanes_decode_gauss(sc_v, mu_v, tdev, tables, words, spans, state, y_hat=yh_v, step=step)
        assert torch.equal(_bits(_unframed(yh_flat, B, pix, C)), _bits(want.cpu())), s
        x, pos = _final(state)
        assert (x == np.uint64(1 << 31)).all() and pos.tolist() == [[len(w) // 4 for w in img] for img in host]
    print(f"lanes bytes per image at step 2 / 0.5: {sizes[2.0]} / {sizes[0.5]} (of which {W * 512} are lane states)")
    assert all(c > W * 512 for c in sizes[2.0]), "the coarse stream must shed words too: the comparison is between two real payloads"
    assert all(f > c for f, c in zip(sizes[0.5], sizes[2.0])), sizes
