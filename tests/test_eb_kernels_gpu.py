"""The factorised-density kernels (csrc/entropy.hip: clc_eb_lik_fwd, clc_eb_lik_bwd, clc_eb_aux) through the C ABI, every element against
the float64 specification tests/eb_ref.py, on [rows, C] maps (one 256-thread workgroup per channel walks the rows in trips of 256):

    (1, 1)      single element, single channel            (256, 2)    exactly one trip through the row loop
    (3, 5)      fewer rows than one wave                   (257, 3)    one thread takes a second trip
    (255, 2)    one row short of the workgroup             (600, 4)    two full trips and a partial third; read and written through
    (128, 192)  the shape of test_kernels_gpu.py's test                channel slices of wider buffers (ld = C + 64) of sentinels

each in training and in inference mode; parameter set A (the weight recipe, heavy tails) on every shape, B (the density falls through
the likelihood bound inside a ramp of latents) and C (zero factors, softplus beyond 20, a vanishing sigmoid, exact rounding ties) on
(257, 3) and the sliced (600, 4).  clc_eb_aux runs at C = 1, 63, 64, 65, 192 around its 64-thread block.

Bars (tests/test_kernels_gpu.py::test_gaussian_likelihood / test_entropy_bottleneck_likelihood): likelihood 1e-5 of the largest value,
2e-3 in the log domain over all elements, gradients 2e-4 — dz on its own maximum, each parameter gradient per channel on the larger of
that channel's largest magnitude and the element's float64 sum of absolute per-row contributions —, aux loss 1e-5 and dquantiles 1e-4
per channel.  Exact: z_hat is numpy float32's rint(z - med) + med bit for bit; an element whose float64 likelihood is below 1e-9 is
1e-9f; below the bound a positive upstream gradient gives dz = 0; dz in inference is 0; the NaN the gradient buffers are filled with is
gone; two calls give the same bits; the sentinels around every slice and behind every buffer survive.

Worst figure per quantity over all cases and modes, as one run of this module on an MI355X printed them: the float32 oracle
(oracle.leaves.EntropyBottleneck in float32 on the host; tests/test_eb_ref_cpu.py prints the same column without a GPU) and the
kernels, both against the float64 specification.  Every exact property held for both.

    quantity                         float32 oracle    kernels    bar
    likelihood                       3.6e-06           3.3e-06    1e-05
    log likelihood                   2.4e-05           1.6e-05    2e-03
    dz                               5.2e-05           2.8e-05    2e-04     (both at the single element of the 1 x 1 map)
    dz passed below the bound        7.8e-06           4.9e-06    2e-04
    parameter gradients              2.0e-05           2.1e-05    2e-04
    aux loss                         1.4e-07           1.4e-07    1e-05
    dquantiles                       2.3e-07           2.5e-07    1e-04

No kernel figure is far from the oracle's: the kernels are as good as float32 allows, and nothing in entropy.hip needed changing.
"""
import functools

import numpy as np
import pytest
import torch

import eb_ref as R

pytestmark = pytest.mark.gpu

PAD, SENTINEL = 32, -777.25
TAIL = 8
IDS = [R.case_id(c) for c in R.CASES]


def _api():
    from clc_amd import lib, ops

    return lib.load(), lib, ops._stream()


class _Map:
    """a [rows, C] device map, dense or a channel slice of a [rows, C + 2 PAD] buffer of sentinels"""

    def __init__(self, rows, C, wide, dev, src=None):
        self.wide, self.C = wide, C
        self.buf = torch.full((rows, C + 2 * PAD if wide else C), SENTINEL, device=dev, dtype=torch.float32)
        self.view = self.buf[:, PAD:PAD + C] if wide else self.buf
        if src is not None:
            self.view.copy_(src.to(dev))
        self.ptr, self.ld = self.view.data_ptr(), self.buf.shape[1]

    def get(self):
        if self.wide:
            assert bool((self.buf[:, :PAD] == SENTINEL).all()) and bool((self.buf[:, PAD + self.C:] == SENTINEL).all()), "wrote outside the slice"
        return self.view.cpu().clone()


class _Flat:
    """n floats on the device followed by TAIL sentinels that must survive"""

    def __init__(self, n, dev, fill):
        self.n = n
        self.buf = torch.full((n + TAIL,), SENTINEL, device=dev, dtype=torch.float32)
        self.buf[:n] = fill
        self.ptr = self.buf.data_ptr()

    def get(self):
        assert bool((self.buf[self.n:] == SENTINEL).all()), "wrote past the buffer"
        return self.buf[:self.n].cpu().clone()


class _Params:
    """the 14 parameter tensors and the quantiles on the device, as the pointer arrays of the ABI"""

    def __init__(self, P, dev):
        from clc_amd import lib

        self.t = [t.contiguous().to(dev) for t in R.param_list(P)]
        self.q = P["q"].reshape(-1, 3).contiguous().to(dev)
        self.target = P["target"].contiguous().to(dev)
        self.m, self.b, self.f = (lib.ptr_array([t.data_ptr() for t in ts]) for ts in (self.t[0:5], self.t[5:10], self.t[10:14]))


def _fwd(dev, P, d, rows, C, wide, training, z_hat=True):
    L, lib, st = _api()
    p = _Params(P, dev)
    z, noise = _Map(rows, C, wide, dev, d["z"]), _Map(rows, C, wide, dev, d["noise"])
    lik, zh = _Map(rows, C, wide, dev), _Map(rows, C, wide, dev)
    npn, ldn = (noise.ptr, noise.ld) if training else (None, 0)
    zp, ldh = (zh.ptr, zh.ld) if z_hat else (None, 0)
    lib.check(L.clc_eb_lik_fwd(z.ptr, z.ld, npn, ldn, p.q.data_ptr(), p.m, p.b, p.f, lik.ptr, lik.ld, zp, ldh, rows, C, 0 if training else 1, st),
              "clc_eb_lik_fwd")
    return lik.get(), zh.get()


def _bwd(dev, P, d, rows, C, wide, training):
    L, lib, st = _api()
    p = _Params(P, dev)
    z, noise, w = (_Map(rows, C, wide, dev, d[k]) for k in ("z", "noise", "w"))
    dz = _Map(rows, C, wide, dev)
    g = [_Flat(t.numel(), dev, float("nan")) for t in p.t]
    gm, gb, gf = (lib.ptr_array([x.ptr for x in xs]) for xs in (g[0:5], g[5:10], g[10:14]))
    npn, ldn = (noise.ptr, noise.ld) if training else (None, 0)
    lib.check(L.clc_eb_lik_bwd(w.ptr, w.ld, z.ptr, z.ld, npn, ldn, p.q.data_ptr(), p.m, p.b, p.f, gm, gb, gf, dz.ptr, dz.ld, rows, C,
                               0 if training else 1, st), "clc_eb_lik_bwd")
    return dz.get(), [x.get().reshape(t.shape) for x, t in zip(g, p.t)]


def _aux(dev, P, C, with_dq=True):
    L, lib, st = _api()
    p = _Params(P, dev)
    loss, dq = _Flat(C, dev, float("nan")), _Flat(3 * C, dev, float("nan"))
    lib.check(L.clc_eb_aux(p.q.data_ptr(), p.m, p.b, p.f, p.target.data_ptr(), loss.ptr, dq.ptr if with_dq else None, C, st), "clc_eb_aux")
    return loss.get(), dq.get().reshape(C, 3)


def _bits(a):
    return a.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _ref(case, training):
    """float64, computed once, shared, never modified"""
    ps, rows, C, _ = case
    return R.reference(R.params(ps, C), R.latents(ps, rows, C), training)


@functools.lru_cache(maxsize=None)
def _oracle(case, training):
    ps, rows, C, _ = case
    return R.oracle_result(R.params(ps, C), R.latents(ps, rows, C), training, R.F32)


def _report(tag, kernel, oracle):
    """the kernel's figure next to the float32 oracle's, for every quantity"""
    for k, (v, bar) in kernel.items():
        print(f"{tag:26s} {k:28s} kernel {v:10.3e}   float32 oracle {oracle[k][0]:10.3e}   bar {bar:.0e}")
    assert not R.failures(kernel), R.failures(kernel)


@pytest.mark.parametrize("training", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_forward_every_element(dev, case, training):
    ps, rows, C, wide = case
    P, d, ref = R.params(ps, C), R.latents(ps, rows, C), _ref(case, training)
    lik, zh = _fwd(dev, P, d, rows, C, wide, training)
    _report(R.case_id(case), R.compare_forward({"lik": lik, "z_hat": zh}, ref), R.compare_forward(_oracle(case, training), ref))
    # z_hat is optional: without it the likelihood is the same
    assert torch.equal(_bits(_fwd(dev, P, d, rows, C, wide, training, z_hat=False)[0]), _bits(lik))


@pytest.mark.parametrize("training", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_backward_every_element(dev, case, training):
    ps, rows, C, wide = case
    P, d, ref = R.params(ps, C), R.latents(ps, rows, C), _ref(case, training)
    dz, grads = _bwd(dev, P, d, rows, C, wide, training)
    _report(R.case_id(case), R.compare_backward({"dz": dz, "grads": grads}, ref, training), R.compare_backward(_oracle(case, training), ref, training))
    dz2, grads2 = _bwd(dev, P, d, rows, C, wide, training)      # the reduction is a fixed tree
    assert torch.equal(_bits(dz2), _bits(dz)) and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(grads2, grads)), "differs run to run"


@pytest.mark.parametrize("training", [False, True], ids=["eval", "train"])
def test_sign_trick_at_zero(dev, training):
    """an odd logits function (set C with zero biases: its factors are zero, so every layer is a bias-free fused multiply-add and
    logits(-x) = -logits(x) exactly in float32 as in float64) with median 0: at v = 0 lower + upper is exactly zero, the sign is 0, the
    raw likelihood is 0, the stored one is the bound and every gradient of that element is zero; the other rows are ordinary"""
    C = 2
    P = dict(R.params("C", C))
    P["b"] = tuple(torch.zeros_like(t) for t in P["b"])
    P["q"] = torch.tensor([[[-4.0, 0.0, 5.0]]]).repeat(C, 1, 1)
    z = torch.tensor([[0.0, 0.0], [1.0, -1.0], [0.3, -0.2], [0.0, 2.0]])
    d = {"z": z, "noise": torch.zeros_like(z), "w": torch.tensor([[1.0, -1.0], [0.5, -0.5], [1.0, 1.0], [-2.0, 1.0]])}
    ref, oracle = R.reference(P, d, training), R.oracle_result(P, d, training, R.F32)
    assert float(ref["raw"][0].abs().max()) == 0.0 and float(ref["raw"][3, 0]) == 0.0 and float(ref["raw"][1].min()) > 1e-3
    lik, zh = _fwd(dev, P, d, 4, C, False, training)
    dz, grads = _bwd(dev, P, d, 4, C, False, training)
    fig = R.compare_forward({"lik": lik, "z_hat": zh}, ref)
    fig.update(R.compare_backward({"dz": dz, "grads": grads}, ref, training))
    want = R.compare_forward(oracle, ref)
    want.update(R.compare_backward(oracle, ref, training))
    _report("sign 0", fig, want)


@pytest.mark.parametrize("training", [False, True], ids=["eval", "train"])
def test_a_nan_latent_stays_nan(dev, training):
    """one NaN in z on (257, 3), set A: the likelihood of that element is NaN (LowerBound's forward is torch.max, which keeps a NaN;
    fmaxf returned the bound), and so are its dz in training and its channel's parameter gradients, exactly where the float32 oracle's
    are; every other element and every other channel has the bits of a run without the NaN"""
    ps, rows, C = "A", 257, 3
    P, clean = R.params(ps, C), R.latents(ps, rows, C)
    d = dict(clean, z=clean["z"].clone())
    d["z"][100, 1] = float("nan")
    oracle = R.oracle_result(P, d, training, R.F32)
    assert bool(torch.isnan(oracle["lik"][100, 1])) and int(torch.isnan(oracle["lik"]).sum()) == 1
    lik, zh = _fwd(dev, P, d, rows, C, False, training)
    lik0, _ = _fwd(dev, P, clean, rows, C, False, training)
    dz, grads = _bwd(dev, P, d, rows, C, False, training)
    dz0, grads0 = _bwd(dev, P, clean, rows, C, False, training)
    keep = torch.ones(rows, C, dtype=torch.bool)
    keep[100, 1] = False
    assert torch.equal(torch.isnan(lik), torch.isnan(oracle["lik"])) and torch.equal(_bits(lik[keep]), _bits(lik0[keep]))
    assert torch.equal(torch.isnan(dz), torch.isnan(oracle["dz"])) and torch.equal(_bits(dz[keep]), _bits(dz0[keep]))
    for name, g, g0, go in zip(R.GRAD_NAMES, grads, grads0, oracle["grads"]):
        assert torch.equal(torch.isnan(g), torch.isnan(go)), name
        assert bool(torch.isnan(g[1]).all()) and torch.equal(_bits(g[[0, 2]]), _bits(g0[[0, 2]])), name


@pytest.mark.parametrize("ps", ["A", "B", "C"])
@pytest.mark.parametrize("C", R.AUX_CS)
def test_aux_loss_and_dquantiles(dev, C, ps):
    P = R.params(ps, C)
    ref, oracle = R.aux(P), R.compare_aux(R.oracle_aux(P, R.F32), R.aux(P))
    loss, dq = _aux(dev, P, C)
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(dq).all())
    _report(f"aux {ps} C={C}", R.compare_aux({"loss": loss, "dq": dq}, ref), oracle)
    loss0, dq0 = _aux(dev, P, C, with_dq=False)                 # dquantiles is optional: the same loss, nothing written
    assert torch.equal(_bits(loss0), _bits(loss)) and bool(torch.isnan(dq0).all())


def test_wrappers_give_the_raw_kernels_bits(dev):
    """ops.eb_likelihood / ops.eb_aux_loss on (257, 3), set B: the raw kernels' bits; an upstream gradient on z_hat adds straight through
    in training mode and is the whole of dz in inference mode; with persistent gradient buffers (the optimizer's arena) the parameter
    gradients are added into them"""
    from clc_amd import ops

    ps, rows, C = "B", 257, 3
    P, d = R.params(ps, C), R.latents(ps, rows, C)
    to4 = lambda t: t.reshape(1, rows, 1, C).permute(0, 3, 1, 2).to(dev)
    back = lambda t: t.detach().permute(0, 2, 3, 1).reshape(rows, C).cpu()
    q = P["q"].to(dev)
    for training in (False, True):
        raw_lik, raw_zh = _fwd(dev, P, d, rows, C, False, training)
        raw_dz, raw_g = _bwd(dev, P, d, rows, C, False, training)
        for direct in (False, True):
            prm = [t.to(dev).requires_grad_() for t in R.param_list(P)]
            init = [torch.full_like(t, 0.5) for t in R.param_list(P)]
            if direct:
                for t, i in zip(prm, init):
                    t.grad = i.to(dev)
                    t._clc_direct = True
                    assert ops._direct_grad(t) is t.grad
            held = [t.grad for t in prm]
            z = to4(d["z"]).requires_grad_()
            lik, zh = ops.eb_likelihood(z, to4(d["noise"]) if training else None, q, training, prm[0:5], prm[5:10], prm[10:14])
            assert torch.equal(_bits(back(lik)), _bits(raw_lik)) and torch.equal(_bits(back(zh)), _bits(raw_zh))
            ((lik * to4(d["w"])).sum() + (zh * to4(d["gh"])).sum()).backward()
            want_dz = raw_dz + d["gh"] if training else d["gh"]          # float32: one IEEE add per element
            assert torch.equal(_bits(back(z.grad)), _bits(want_dz)), (training, direct)
            for t, g, i, h in zip(prm, raw_g, init, held):
                assert torch.equal(_bits(t.grad.cpu()), _bits(i + g if direct else g)), (training, direct)
                assert not direct or t.grad is h, "the gradient buffer was replaced, not added into"
        # without an upstream gradient on z_hat: dz alone in training, no gradient at all in inference
        z = to4(d["z"]).requires_grad_()
        prm = [t.to(dev).requires_grad_() for t in R.param_list(P)]
        lik, _ = ops.eb_likelihood(z, to4(d["noise"]) if training else None, q, training, prm[0:5], prm[5:10], prm[10:14])
        (lik * to4(d["w"])).sum().backward()
        if training:
            assert torch.equal(_bits(back(z.grad)), _bits(raw_dz))
        else:
            assert z.grad is None or float(z.grad.abs().max()) == 0.0
    prm = [t.to(dev).requires_grad_() for t in R.param_list(P)]
    qg = P["q"].to(dev).requires_grad_()
    total = ops.eb_aux_loss(qg, P["target"].to(dev), prm[0:5], prm[5:10], prm[10:14])
    total.backward()
    loss, dq = _aux(dev, P, C)
    ref = R.aux(P)
    assert abs(float(total.detach()) - float(ref["loss"].sum())) <= R.BARS["aux"] * float(ref["loss"].sum())
    assert torch.equal(_bits(qg.grad.reshape(C, 3).cpu()), _bits(dq))
    fig = R.compare_aux({"loss": loss, "dq": qg.grad.reshape(C, 3).cpu(), "dparams": [t.grad.cpu() for t in prm if t.grad is not None]}, ref)
    assert not R.failures(fig), fig


def test_c_abi_refuses_bad_arguments_by_message(dev):
    """every CLC_CHECK of the three entry points, one argument at a time; none of these calls launches a kernel"""
    L, lib, st = _api()
    rows, C = 4, 2
    P = R.params("A", C)
    p = _Params(P, dev)
    t = torch.zeros(rows * C, device=dev)
    x = t.data_ptr()
    g = [torch.zeros(a.numel(), device=dev) for a in p.t]
    gm, gb, gf = (lib.ptr_array([a.data_ptr() for a in xs]) for xs in (g[0:5], g[5:10], g[10:14]))

    def refused(rc, text):
        assert rc < 0 and text in L.clc_last_error().decode(), (rc, L.clc_last_error())

    def swap(args, i, v):
        return args[:i] + (v,) + args[i + 1:]

    fwd = (x, C, x, C, p.q.data_ptr(), p.m, p.b, p.f, x, C, x, C, rows, C, 0, st)
    for i in (0, 4, 5, 6, 7, 8):                   # z, quantiles, matrices, biases, factors, lik
        refused(L.clc_eb_lik_fwd(*swap(fwd, i, None)), "clc_eb_lik_fwd: bad args")
    refused(L.clc_eb_lik_fwd(*swap(fwd, 12, 0)), "clc_eb_lik_fwd: bad args")
    refused(L.clc_eb_lik_fwd(*swap(fwd, 13, 0)), "clc_eb_lik_fwd: bad args")
    refused(L.clc_eb_lik_fwd(*swap(fwd, 2, None)), "clc_eb_lik_fwd: training mode needs noise")
    bwd = (x, C, x, C, x, C, p.q.data_ptr(), p.m, p.b, p.f, gm, gb, gf, x, C, rows, C, 0, st)
    for i in (0, 2, 6, 7, 8, 9, 10, 11, 12):       # dlik, z, quantiles, matrices, biases, factors, dmatrices, dbiases, dfactors
        refused(L.clc_eb_lik_bwd(*swap(bwd, i, None)), "clc_eb_lik_bwd: bad args")
    refused(L.clc_eb_lik_bwd(*swap(bwd, 15, 0)), "clc_eb_lik_bwd: bad args")
    refused(L.clc_eb_lik_bwd(*swap(bwd, 16, 0)), "clc_eb_lik_bwd: bad args")
    refused(L.clc_eb_lik_bwd(*swap(bwd, 4, None)), "clc_eb_lik_bwd: training mode needs noise")
    aux = (p.q.data_ptr(), p.m, p.b, p.f, p.target.data_ptr(), x, x, C, st)
    for i in (0, 1, 2, 3, 4, 5):                   # quantiles, matrices, biases, factors, target, loss_partial
        refused(L.clc_eb_aux(*swap(aux, i, None)), "clc_eb_aux: bad args")
    refused(L.clc_eb_aux(*swap(aux, 7, 0)), "clc_eb_aux: bad args")
    torch.cuda.synchronize()
    assert float(t.abs().max()) == 0.0 and all(float(a.abs().max()) == 0.0 for a in g), "a refused call wrote something"
