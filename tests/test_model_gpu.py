"""GPU parity of the product models (HIP path through the C ABI) against the CPU oracle on identical weights/inputs.

Bars (BASELINE.json north_star): |d bpp| <= 1e-4, |d PSNR| <= 0.01 dB for the float transforms; bit-identical
bitstreams for the integer CDF / quantise / rANS path.  Weights come from the by-name recipe (oracle/recipe.py).
"""
import contextlib
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _psnr(a, b):
    return -10 * math.log10(torch.mean((a.double() - b.double()) ** 2).item())


def _pair(kind, R, dev, seed=0):
    from clc_amd import models as pm
    from oracle import graph as og
    from oracle.recipe import apply_weight_recipe

    if kind == "clc":
        o, p = og.CLC(N=64, num_ref_frames=R), pm.CLC(N=64, num_ref_frames=R)
    else:
        o, p = og.TCM(N=64), pm.TCM(N=64)
    apply_weight_recipe(o, seed)
    p.load_state_dict(o.state_dict())
    return o.eval(), p.to(dev).eval()


def _inputs(B, R, smooth=True, size=256, seed=100):
    """size: the side of a square image, or (h, w)"""
    from oracle.recipe import synthetic_image

    h, w = (size, size) if isinstance(size, int) else size
    return synthetic_image(B, h, w, seed, smooth=smooth), [synthetic_image(B, h, w, seed + 1 + i, smooth=smooth) for i in range(R)]


def _count_paired_slices(monkeypatch):
    """-> a one-element list counting the calls of ops.whole_and_first_half, which only the paired slice route of
    models/clc.py `_slice_params` makes (once per slice): 0 on the unpaired route, 5 per forward on the paired one"""
    from clc_amd import ops

    n = [0]
    real = ops.whole_and_first_half

    def counted(x):
        n[0] += 1
        return real(x)

    monkeypatch.setattr(ops, "whole_and_first_half", counted)
    return n


@pytest.mark.parametrize("kind,R", [("clc", 1), ("clc", 3), ("tcm", 0)])
def test_forward_parity(dev, kind, R):
    from oracle.loss import RateDistortionLoss as ORD, compute_bpp

    o, p = _pair(kind, R, dev)
    x, refs = _inputs(1, R)
    with torch.no_grad():
        a = o(x, refs) if kind == "clc" else o(x)
        b = p(x.to(dev), [r.to(dev) for r in refs]) if kind == "clc" else p(x.to(dev))
    assert b["x_hat"].shape == a["x_hat"].shape and b["likelihoods"]["y"].shape == (1, 320, 16, 16) and b["likelihoods"]["z"].shape == (1, 192, 4, 4)
    # pre-quantisation tensors agree to fp32 summation-order accuracy
    y_err = (b["para"]["y"].cpu() - a["para"]["y"]).abs().max().item() / a["para"]["y"].abs().max().item()
    assert y_err < 5e-5, f"y rel err {y_err}"
    bpp_o, bpp_p = compute_bpp(a), compute_bpp({"x_hat": b["x_hat"].cpu(), "likelihoods": {k: v.cpu() for k, v in b["likelihoods"].items()}})
    assert abs(bpp_o - bpp_p) <= 1e-4, (bpp_o, bpp_p)
    psnr_o, psnr_p = _psnr(a["x_hat"], x), _psnr(b["x_hat"].cpu(), x)
    assert abs(psnr_o - psnr_p) <= 0.01, (psnr_o, psnr_p)
    # elementwise: everything except (rare) rounding-boundary flips must agree (bar 0.5 % of the pixels; measured: none)
    d = (b["x_hat"].cpu() - a["x_hat"]).abs()
    frac_bad = (d > 1e-3 * a["x_hat"].abs().max()).float().mean().item()
    assert frac_bad < 5e-3, frac_bad


def test_forward_parity_over_a_sample_of_images(dev):
    """north_star's bars (|d bpp| <= 1e-4, |d PSNR| <= 0.01 dB) on a SAMPLE of seeded images, as bench.py's `parity` object states them: the
    mean is held against the bar, and no single image may be off by more than the footprint of one hyper-latent rounding flip (1e-3 bpp) —
    so that one latent within float error of a rounding boundary on one image neither hides a real error nor dictates a kernel choice."""
    from oracle.loss import compute_bpp
    from oracle.recipe import synthetic_image

    o, p = _pair("clc", 1, dev)
    dbpp, dpsnr = [], []
    for sd in (100, 110, 120, 130):
        x, r = synthetic_image(1, 256, 256, sd, smooth=True), [synthetic_image(1, 256, 256, sd + 1, smooth=True)]
        with torch.no_grad():
            a = o(x, r)
            b = p(x.to(dev), [r[0].to(dev)])
        dbpp.append(abs(compute_bpp(a) - compute_bpp({"x_hat": b["x_hat"].cpu(), "likelihoods": {k: v.cpu() for k, v in b["likelihoods"].items()}})))
        dpsnr.append(abs(_psnr(a["x_hat"], x) - _psnr(b["x_hat"].cpu(), x)))
    assert sum(dbpp) / len(dbpp) <= 1e-4 and max(dbpp) <= 1e-3, dbpp
    assert sum(dpsnr) / len(dpsnr) <= 0.01 and max(dpsnr) <= 0.02, dpsnr


def test_forward_parity_other_shapes(dev):
    """Shape-generic kernels: the wide model (N=128, train_CLC.py's default width) and a non-square 256x384 input."""
    from clc_amd import models as pm
    from oracle import graph as og
    from oracle.loss import compute_bpp
    from oracle.recipe import apply_weight_recipe, synthetic_image

    for N, (h, w) in ((128, (256, 256)), (64, (256, 384))):
        o = og.CLC(N=N, num_ref_frames=1).eval()
        apply_weight_recipe(o, 2)
        p = pm.CLC(N=N, num_ref_frames=1)
        p.load_state_dict(o.state_dict())
        p = p.to(dev).eval()
        x, r = synthetic_image(1, h, w, 50, smooth=True), [synthetic_image(1, h, w, 51, smooth=True)]
        with torch.no_grad():
            a = o(x, r)
            b = p(x.to(dev), [r[0].to(dev)])
        assert b["x_hat"].shape == (1, 3, h, w)
        y_err = (b["para"]["y"].cpu() - a["para"]["y"]).abs().max().item() / a["para"]["y"].abs().max().item()
        assert y_err < 5e-5, (N, h, w, y_err)
        bo = compute_bpp(a)
        bp = compute_bpp({"x_hat": b["x_hat"].cpu(), "likelihoods": {k: v.cpu() for k, v in b["likelihoods"].items()}})
        assert abs(bo - bp) <= 1e-4, (N, h, w, bo, bp)
        assert abs(_psnr(a["x_hat"], x) - _psnr(b["x_hat"].cpu(), x)) <= 0.01


def _grad_parity(o, p, tol=1e-3, min_checked=600, flips=0, flip_tol=5e-2):
    """every parameter gradient of the product vs the oracle's, relative to the gradient's largest element (bar 1e-3; measured worst
    1.6e-4 — a 10x regression fails).
    flips: number of latent elements whose STE-rounded symbol differs between the two runs (round(y - mu) is discontinuous: an
    argument within float error of .5 lands on either side, and that y_hat element then differs by 1.0).  Each flip perturbs the
    gradients of the layers downstream of it; with flips > 0 at most 4 * flips parameters may exceed `tol`, none `flip_tol`."""
    og = dict(o.named_parameters())
    checked, worst, over = 0, 0.0, []
    for n, prm in p.named_parameters():
        go = og[n].grad
        if go is None:
            assert prm.grad is None or float(prm.grad.abs().max()) == 0.0, f"{n}: oracle has no grad"
            continue
        assert prm.grad is not None, f"{n}: missing grad"
        gp = prm.grad.cpu()
        denom = go.abs().max().item()
        if denom < 1e-12:
            continue
        err = (gp - go).abs().max().item() / denom
        worst = max(worst, err)
        checked += 1
        if err >= tol:
            over.append((n, err))
        assert err < (flip_tol if flips else tol), f"{n}: grad rel err {err:.3e} (symbol flips: {flips})"
    assert len(over) <= 4 * flips, (flips, over)
    assert checked > min_checked, checked
    return checked, worst


@contextlib.contextmanager
def _direct_forward():
    """Pin a recorded forward to the direct kernels (tuning key 23 bit 0 off; the data gradients keep the Winograd kernel).
    The gradient comparison below is conditioned on both sides quantizing to the SAME symbols.  These two seeded inputs have a latent within
    float error of a rounding boundary: the direct kernels land on the oracle's side of it, the Winograd forward's summation order (y moves by
    9e-7 of its largest element) does not, and the flip cascades through the autoregressive slices (tools/wino_flip_check.py: 70 / 30 differing
    symbols, scales moved by up to 0.04) and moves every gradient by ~1e-3.  The Winograd forward itself is held to the direct kernels and to
    fp64 by tests/test_kernels_gpu.py::test_wino_conv_vs_direct_and_fp64, and rides in the flip-aware batch-8 steps below
    (test_config1_bs8_..., test_config2_bs8_...) and in the 3-reference and TCM cases of test_backward_parity, which run on the defaults."""
    from clc_amd import lib
    L = lib.load()
    old = L.clc_get_tuning(23)
    L.clc_set_tuning(23, old & 2)
    try:
        yield
    finally:
        L.clc_set_tuning(23, old)


def _symbol_flips(a, b):
    """positions where round(y - mu) differs between the oracle's and the product's forward (see _grad_parity)"""
    so = torch.round(a["para"]["y"] - a["para"]["means"])
    sp = torch.round(b["para"]["y"].cpu() - b["para"]["means"].cpu())
    return int((so != sp).sum())


@pytest.mark.parametrize("kind,R,B", [("clc", 1, 2), ("clc", 3, 2), ("tcm", 0, 2)])
def test_backward_parity(dev, kind, R, B):
    """Eval-mode (deterministic rounding) forward with autograd on: loss terms and every parameter gradient vs the oracle,
    for CLC with 1 and 3 references and for TCM (the no-reference slice nets)."""
    from clc_amd.train import RateDistortionLoss as PRD
    from oracle.loss import RateDistortionLoss as ORD

    o, p = _pair(kind, R, dev)
    x, refs = _inputs(B, R)
    lo = ORD(0.0067)(o(x, refs) if kind == "clc" else o(x), x)
    lo["loss"].backward()
    xd, rd = x.to(dev), [r.to(dev) for r in refs]
    with (_direct_forward() if (kind, R) == ("clc", 1) else contextlib.nullcontext()):
        lp = PRD(0.0067)(p(xd, rd) if kind == "clc" else p(xd), xd)
    lp["loss"].backward()
    for k in ("loss", "bpp_loss", "mse_loss"):
        assert abs(lo[k].item() - lp[k].item()) <= 2e-4 * max(1.0, abs(lo[k].item())), (k, lo[k].item(), lp[k].item())
    checked, worst = _grad_parity(o, p)
    print(kind, R, "checked", checked, "worst rel err", worst)


# 384x384: a 24x24 latent, 576 rows per image.  The slice nets pair only when B * 576 is a multiple of 128, so one image takes the
# unpaired route (models/clc.py `_slice_params`, the `else` body) — the route of every odd-block image that eval.py pads at batch 1.
@pytest.mark.parametrize("kind,R", [("clc", 1), ("tcm", 0)])
def test_forward_parity_unpaired_slices_384(dev, kind, R, monkeypatch):
    from oracle.loss import compute_bpp

    paired = _count_paired_slices(monkeypatch)
    o, p = _pair(kind, R, dev)
    x, refs = _inputs(1, R, size=384)
    with torch.no_grad():
        a = o(x, refs) if kind == "clc" else o(x)
        b = p(x.to(dev), [r.to(dev) for r in refs]) if kind == "clc" else p(x.to(dev))
    assert paired[0] == 0, "expected the unpaired slice route"
    assert b["likelihoods"]["y"].shape == (1, 320, 24, 24) and b["likelihoods"]["z"].shape == (1, 192, 6, 6)
    y_err = (b["para"]["y"].cpu() - a["para"]["y"]).abs().max().item() / a["para"]["y"].abs().max().item()
    assert y_err < 5e-5, f"y rel err {y_err}"
    bpp_o, bpp_p = compute_bpp(a), compute_bpp({"x_hat": b["x_hat"].cpu(), "likelihoods": {k: v.cpu() for k, v in b["likelihoods"].items()}})
    assert abs(bpp_o - bpp_p) <= 1e-4, (bpp_o, bpp_p)
    psnr_o, psnr_p = _psnr(a["x_hat"], x), _psnr(b["x_hat"].cpu(), x)
    assert abs(psnr_o - psnr_p) <= 0.01, (psnr_o, psnr_p)
    d = (b["x_hat"].cpu() - a["x_hat"]).abs()
    frac_bad = (d > 1e-3 * a["x_hat"].abs().max()).float().mean().item()
    assert frac_bad < 5e-3, frac_bad


@pytest.mark.parametrize("B", [1, 2])
def test_backward_parity_384(dev, B, monkeypatch):
    """CLC R = 1 at 384x384, loss terms and every parameter gradient vs the oracle.  B = 1: the unpaired slice nets; B = 2: the paired
    ones with 1152-row halves on the 64x64 tiles (the 16x16-map cases of test_backward_parity run on the split-K family)."""
    from clc_amd.train import RateDistortionLoss as PRD
    from oracle.loss import RateDistortionLoss as ORD

    paired = _count_paired_slices(monkeypatch)
    o, p = _pair("clc", 1, dev)
    x, refs = _inputs(B, 1, size=384)
    oo = o(x, refs)
    lo = ORD(0.0067)(oo, x)
    lo["loss"].backward()
    xd, rd = x.to(dev), [r.to(dev) for r in refs]
    po = p(xd, rd)
    assert paired[0] == (5 if B == 2 else 0), (B, paired[0])
    lp = PRD(0.0067)(po, xd)
    lp["loss"].backward()
    assert _symbol_flips(oo, po) == 0
    for k in ("loss", "bpp_loss", "mse_loss"):
        assert abs(lo[k].item() - lp[k].item()) <= 2e-4 * max(1.0, abs(lo[k].item())), (k, lo[k].item(), lp[k].item())
    checked, worst = _grad_parity(o, p)
    print("384x384 B", B, "checked", checked, "worst rel err", worst)


def test_unpaired_slices_stay_on_one_stream_after_a_train_engine(dev, monkeypatch):
    """A TrainEngine in the process leaves other models' launches alone: a plain forward and backward at 384x384, batch 1 (the unpaired
    slice route), issues every C-ABI launch on one stream — the scale-parameter net is not moved to a stream of its own."""
    from clc_amd import models as pm
    from clc_amd import ops
    from clc_amd.recipe import apply_weight_recipe
    from clc_amd.train import RateDistortionLoss, TrainEngine

    x, refs = _inputs(2, 1)
    m = pm.CLC(N=64, num_ref_frames=1).to(dev)
    apply_weight_recipe(m, 0)
    TrainEngine(m, lmbda=0.0067, use_graph=False, train_mode=False).step(x.to(dev), [r.to(dev) for r in refs])
    torch.cuda.synchronize()

    paired = _count_paired_slices(monkeypatch)
    p = pm.CLC(N=64, num_ref_frames=1).to(dev).eval()
    apply_weight_recipe(p, 0)
    x, refs = _inputs(1, 1, size=384)
    xd, rd = x.to(dev), [r.to(dev) for r in refs]
    streams, real = [], ops._stream

    def recorded():
        s = real()
        streams.append(s)
        return s

    monkeypatch.setattr(ops, "_stream", recorded)
    out = p(xd, rd)
    n_fwd = len(streams)
    RateDistortionLoss(0.0067)(out, xd)["loss"].backward()
    torch.cuda.synchronize()
    assert paired[0] == 0, "expected the unpaired slice route"
    assert 0 < n_fwd < len(streams)
    assert set(streams[:n_fwd]) == {torch.cuda.current_stream().cuda_stream}, "forward"
    assert set(streams[n_fwd:]) == {torch.cuda.current_stream().cuda_stream}, "backward"


def test_paired_and_unpaired_slices_agree(dev, monkeypatch):
    """The same 256x256 batch of 2 through the paired slice nets and, with ops.PAIR_SLICES = 0, the unpaired ones.  A filter-set launch gives
    each half the bits of a separate launch (test_conv_paired_filters), so the eval forward is bit-identical; the gradients agree up to fp32
    accumulation order (the bar of test_slice_loop_launch_merging_keeps_the_bits)."""
    from clc_amd import ops
    from clc_amd.train import RateDistortionLoss as PRD

    paired = _count_paired_slices(monkeypatch)
    _, p = _pair("clc", 1, dev)
    x, refs = _inputs(2, 1)
    xd, rd = x.to(dev), [r.to(dev) for r in refs]

    def run():
        paired[0] = 0
        with torch.no_grad():
            ev = p(xd, rd)
        n_eval = paired[0]
        p.zero_grad(set_to_none=True)
        PRD(0.0067)(p(xd, rd), xd)["loss"].backward()
        ops.flush_wgrads()
        torch.cuda.synchronize()
        return ev, {n: q.grad.clone() for n, q in p.named_parameters() if q.grad is not None}, (n_eval, paired[0] - n_eval)

    ev1, g1, n1 = run()
    monkeypatch.setattr(ops, "PAIR_SLICES", 0)
    ev0, g0, n0 = run()
    assert n1 == (5, 5) and n0 == (0, 0), (n1, n0)
    assert torch.equal(ev1["x_hat"], ev0["x_hat"]), "x_hat"
    for k in ("y", "z"):
        assert torch.equal(ev1["likelihoods"][k], ev0["likelihoods"][k]), k
    for k in ("means", "scales", "y"):
        assert torch.equal(ev1["para"][k], ev0["para"][k]), k
    assert g1.keys() == g0.keys()
    worst = 0.0
    for n in g1:
        d = g0[n].abs().max().item()
        if d > 1e-12:
            worst = max(worst, (g1[n] - g0[n]).abs().max().item() / d)
    assert worst < 2e-4, worst


def test_slice_loop_launch_merging_keeps_the_bits(dev, monkeypatch):
    """The slice loop's launch-count reductions — four filter sets per launch (ops.QUAD_UNITS), the support / gradient buffers
    (ops.SUPPORT_BUFFER), the separate activation-backward pass of large 3x3 layers (ops.MATERIALIZE_DZ) — only regroup work: the
    forward results are bit-identical with and without them, the gradients equal up to fp32 accumulation order."""
    from clc_amd import ops
    from clc_amd.train import RateDistortionLoss as PRD

    _, p = _pair("clc", 1, dev)
    x, refs = _inputs(2, 1)
    xd, rd = x.to(dev), [r.to(dev) for r in refs]

    def run():
        p.zero_grad(set_to_none=True)
        out = p(xd, rd)
        PRD(0.0067)(out, xd)["loss"].backward()
        ops.flush_wgrads()
        torch.cuda.synchronize()
        return out, {n: q.grad.clone() for n, q in p.named_parameters() if q.grad is not None}

    out1, g1 = run()
    monkeypatch.setattr(ops, "QUAD_UNITS", 0)
    monkeypatch.setattr(ops, "SUPPORT_BUFFER", 0)
    monkeypatch.setattr(ops, "MATERIALIZE_DZ", 0)
    out0, g0 = run()
    for k in ("x_hat",):
        assert torch.equal(out1[k], out0[k]), k
    for k in ("y", "z"):
        assert torch.equal(out1["likelihoods"][k], out0["likelihoods"][k]), k
    assert g1.keys() == g0.keys()
    worst = 0.0
    for n in g1:
        d = g0[n].abs().max().item()
        if d > 1e-12:
            worst = max(worst, (g1[n] - g0[n]).abs().max().item() / d)
    assert worst < 2e-4, worst


@pytest.mark.parametrize("R", [1])
def test_wire_clm_forward_backward_vs_oracle(dev, R):
    """SURVEY 8(f)-4 (an extension, not reference behaviour): wire_clm = True routes the hyper-latent through feature_alignment /
    multi_ref_fusion (clc_amd/models/clc.py `_fuse_z`; the same definition restated in oracle/graph.py).  Loss terms, every parameter
    gradient — the dormant modules' included — and the codec round trip against the oracle."""
    from clc_amd.train import RateDistortionLoss as PRD
    from oracle.loss import RateDistortionLoss as ORD

    o, p = _pair("clc", R, dev)
    o.wire_clm = p.wire_clm = True
    x, refs = _inputs(1, R, size=512)   # (CLM's Swin block has 4x4 windows: the hyper-latent must be larger, i.e. the image >= 512)
    lo = ORD(0.0067)(o(x, refs), x)
    lo["loss"].backward()
    xd, rd = x.to(dev), [r.to(dev) for r in refs]
    with _direct_forward():
        lp = PRD(0.0067)(p(xd, rd), xd)
    lp["loss"].backward()
    for k in ("loss", "bpp_loss", "mse_loss"):
        assert abs(lo[k].item() - lp[k].item()) <= 2e-4 * max(1.0, abs(lo[k].item())), (k, lo[k].item(), lp[k].item())
    _grad_parity(o, p)
    names = [n for n, q in p.named_parameters() if n.startswith(("feature_alignment", "multi_ref_fusion")) and q.grad is not None and float(q.grad.abs().max()) > 0]
    assert len(names) > 50, "the wired modules received no gradient"
    # with the wiring off the same weights give the reference graph (other z, other loss)
    o.wire_clm = p.wire_clm = False
    with torch.no_grad():
        assert abs(PRD(0.0067)(p(xd, rd), xd)["loss"].item() - lp["loss"].item()) > 1e-6
    # codec: encoder-side only — the decoder needs no change
    p.wire_clm = True
    p.update(force=True)
    with torch.no_grad():
        out = p.compress(xd[:1], [r[:1] for r in rd])
        rec = p.decompress(out["strings"], out["shape"], [r[:1] for r in rd])
    assert rec["x_hat"].shape == (1, 3, 512, 512) and torch.isfinite(rec["x_hat"]).all()


@pytest.mark.parametrize("fwd", ["direct", "default"])
def test_config1_bs8_train_mode_step_vs_oracle(dev, fwd):
    """BASELINE configs[1] at its quoted size (CLC lambda 0.0067 MSE, 256x256, batch 8, 1 reference), TRAIN mode: the additive-noise
    proxy is injected identically on both sides (one U(-1/2,1/2) tensor for y, one for z), so the loss terms (<= 2e-4) and the
    gradients are comparable element for element (train mode consumes RNG).
    fwd = "direct": the recorded forward pinned to the direct kernels (_direct_forward) — at most 8 of the 655 360 STE-rounded symbols may
    differ from the oracle's.  fwd = "default": the step as the engine runs it, Winograd forward included — its other summation order moves
    more knife-edge symbols (each flip cascades through the autoregressive slices; measured 39): at most 1e-4 of the elements, gradients
    held flip-aware like the first case."""
    from clc_amd.train import RateDistortionLoss as PRD
    from oracle.loss import RateDistortionLoss as ORD

    o, p = _pair("clc", 1, dev)
    o.train()
    p.train()
    x, refs = _inputs(8, 1, smooth=False)   # uint8 noise / 255: the bench's synthetic batch
    g = torch.Generator().manual_seed(77)
    ny = torch.rand((8, 320, 16, 16), generator=g) - 0.5
    nz = torch.rand((8, 192, 4, 4), generator=g) - 0.5
    with _injected_noise(ny, nz, dev):
        oo = o(x, refs)
        lo = ORD(0.0067)(oo, x)
        lo["loss"].backward()
        xd, rd = x.to(dev), [r.to(dev) for r in refs]
        with (_direct_forward() if fwd == "direct" else contextlib.nullcontext()):
            po = p(xd, rd)
        lp = PRD(0.0067)(po, xd)
        lp["loss"].backward()
    flips = _symbol_flips(oo, po)
    for k in ("loss", "bpp_loss", "mse_loss"):
        assert abs(lo[k].item() - lp[k].item()) <= 2e-4 * max(1.0, abs(lo[k].item())), (k, lo[k].item(), lp[k].item())
    assert flips <= (8 if fwd == "direct" else 65), flips   # of 655 360 latent elements
    checked, worst = _grad_parity(o, p, tol=4e-3, flips=flips)   # (8-image / 512x512 / N=128 reductions: measured worst 1.1e-3 .. 3.2e-3 of a tensor's largest element, fp32 summation order)
    print("bs8 train-mode: checked", checked, "worst rel err", worst, "symbol flips", flips)


class _injected_noise:
    """Both models draw their quantisation noise with Tensor.uniform_(-0.5, 0.5) on a fresh tensor (CompressAI quantize("noise"),
    SURVEY.md A.2/A.3; product: entropy_models / models.clc).  Replace those draws by slices of fixed tensors, matched by shape."""

    def __init__(self, ny, nz, dev):
        self.ny, self.nz, self.dev = ny, nz, dev
        self.cursor = {}

    def __enter__(self):
        self.orig = torch.Tensor.uniform_
        me = self

        def fake(t, a=0.0, b=1.0, generator=None):
            if (a, b) != (-0.5, 0.5):
                return me.orig(t, a, b, generator=generator)
            shp = tuple(t.shape)
            if shp == tuple(me.nz.shape) or (len(shp) == 3 and t.numel() == me.nz.numel()):
                if len(shp) == 3:   # CompressAI's EntropyBottleneck works on [C, 1, B*H*W]
                    C = shp[0]
                    src = me.nz.permute(1, 0, 2, 3).reshape(C, 1, -1)
                else:
                    src = me.nz
            elif shp == tuple(me.ny.shape):
                src = me.ny
            elif len(shp) == 4 and shp[1] * 5 == me.ny.shape[1]:   # per-slice draw (oracle): slices in order
                k = me.cursor.get("y", 0)
                me.cursor["y"] = (k + 1) % 5
                src = me.ny[:, k * shp[1]:(k + 1) * shp[1]]
            else:
                return me.orig(t, a, b, generator=generator)
            with torch.no_grad():
                t.copy_(src.to(t.device))
            return t

        torch.Tensor.uniform_ = fake
        return self

    def __exit__(self, *exc):
        torch.Tensor.uniform_ = self.orig
        return False


def test_config4_512_bs4_r3_msssim_step_and_codec(dev):
    """BASELINE configs[4]: CLC lambda 0.05 MS-SSIM, 512x512, batch 4, 3 references.
    (1) one MS-SSIM-loss training step (eval-mode rounding): loss terms and every gradient vs the oracle (train_CLC.py:56-57);
    (2) per-image compress -> decompress: y / z bytes identical across the product's C++ coder, the plain-C oracle and the
        pure-Python oracle; decoded x_hat == encoder-side reconstruction bit for bit; an image's stream does not depend on
        which batch it was encoded in."""
    from clc_amd.train import RateDistortionLoss as PRD
    from oracle import rans_c, rans_py
    from oracle.loss import RateDistortionLoss as ORD

    o, p = _pair("clc", 3, dev)
    x, refs = _inputs(4, 3, size=512)
    lo = ORD(0.05, "ms_ssim")(o(x, refs), x)
    lo["loss"].backward()
    xd, rd = x.to(dev), [r.to(dev) for r in refs]
    lp = PRD(0.05, "ms_ssim")(p(xd, rd), xd)
    lp["loss"].backward()
    for k in ("loss", "bpp_loss", "ms_ssim_loss"):
        assert abs(lo[k].item() - lp[k].item()) <= 2e-4 * max(1.0, abs(lo[k].item())), (k, lo[k].item(), lp[k].item())
    checked, worst = _grad_parity(o, p, tol=4e-3)   # (8-image / 512x512 / N=128 reductions: measured worst 1.1e-3 .. 3.2e-3 of a tensor's largest element, fp32 summation order)
    print("configs[4] step: checked", checked, "worst rel err", worst)
    for q in p.parameters():
        q.grad = None
    p.update(force=True)
    gc = p.gaussian_conditional
    cdf, ln, off = gc.host_tables()
    ecdf, eln, eoff = p.entropy_bottleneck.host_tables()
    with torch.no_grad():
        fwd_all = p(xd, rd)
    for i in range(4):
        xi, ri = xd[i:i + 1], [r[i:i + 1] for r in rd]
        enc = p.compress(xi, ri)
        assert tuple(enc["shape"]) == (8, 8) and len(enc["strings"][0]) == 1 and len(enc["strings"][1]) == 1
        dec = p.decompress(enc["strings"], enc["shape"], ri)
        with torch.no_grad():
            fwd = p(xi, ri)
        assert torch.equal(dec["x_hat"], fwd["x_hat"].clamp(0, 1)), f"image {i}: decoder reconstruction != encoder-side reconstruction"
        # batch invariance: the same image inside the batch-4 forward has the same latents and parameters, bit for bit
        assert torch.equal(fwd["para"]["y"], fwd_all["para"]["y"][i:i + 1]) and torch.equal(fwd["para"]["means"], fwd_all["para"]["means"][i:i + 1])
        scales, means, y = fwd["para"]["scales"], fwd["para"]["means"], fwd["para"]["y"]
        idx = torch.cat([gc.build_indexes(s_).contiguous().reshape(-1) for s_ in scales.chunk(5, 1)]).cpu().numpy()
        sym = torch.cat([torch.round(a - m).int().contiguous().reshape(-1) for a, m in zip(y.chunk(5, 1), means.chunk(5, 1))]).cpu().numpy()
        ys = enc["strings"][0][0]
        assert rans_c.encode(sym, idx, cdf, ln, off) == ys, f"image {i}: y bitstream differs from the C oracle coder"
        if i == 0:   # the pure-Python coder takes ~10 s per 327 680-symbol image: once is enough
            assert rans_py.RansEncoder().encode_with_indexes(sym.tolist(), idx.tolist(), cdf.tolist(), ln.tolist(), off.tolist()) == ys
        out, words = rans_c.decode(ys, idx, cdf, ln, off)
        assert (out == sym).all() and words * 4 == len(ys)
        # z stream: EntropyBottleneck.compress on the analysis output
        z = p.h_a(fwd["para"]["y"])
        zsym = torch.round(z - p.entropy_bottleneck._get_medians().reshape(1, -1, 1, 1)).int().contiguous().reshape(-1).cpu().numpy()
        zidx = np.repeat(np.arange(192, dtype=np.int32), 64)
        zs = enc["strings"][1][0]
        assert rans_c.encode(zsym, zidx, ecdf, eln, eoff) == zs, f"image {i}: z bitstream differs from the C oracle coder"
        assert rans_py.RansEncoder().encode_with_indexes(zsym.tolist(), zidx.tolist(), ecdf.tolist(), eln.tolist(), eoff.tolist()) == zs


def test_codec_roundtrip_and_bitstream(dev):
    from oracle import rans_c, rans_py

    o, p = _pair("clc", 1, dev)
    o.update(force=True)
    p.update(force=True)
    # integer CDF tables: bit-identical to the oracle's
    for name in ("_quantized_cdf", "_cdf_length", "_offset"):
        assert torch.equal(getattr(p.gaussian_conditional, name).cpu(), getattr(o.gaussian_conditional, name)), name
        assert torch.equal(getattr(p.entropy_bottleneck, name).cpu(), getattr(o.entropy_bottleneck, name)), name
    x, refs = _inputs(1, 1)
    xd, rd = x.to(dev), [r.to(dev) for r in refs]
    enc = p.compress(xd, rd)
    assert isinstance(enc["strings"][0][0], bytes) and len(enc["strings"][1]) == 1 and tuple(enc["shape"]) == (4, 4)
    dec = p.decompress(enc["strings"], enc["shape"], rd)
    assert dec["x_hat"].shape == (1, 3, 256, 256) and float(dec["x_hat"].min()) >= 0 and float(dec["x_hat"].max()) <= 1
    # determinism: encoding twice gives the same bytes; decoding reproduces the encoder-side reconstruction bit for bit
    enc2 = p.compress(xd, rd)
    assert enc2["strings"] == enc["strings"]
    with torch.no_grad():
        fwd = p(xd, rd)
    assert torch.equal(dec["x_hat"], fwd["x_hat"].clamp(0, 1)), "decoder reconstruction != encoder-side reconstruction"
    # the y stream decodes (with the oracle's C coder) to symbols that re-encode to the same bytes with the oracle coders
    gc = p.gaussian_conditional
    cdf, ln, off = gc.host_tables()
    scales, means, y = fwd["para"]["scales"], fwd["para"]["means"], fwd["para"]["y"]
    idx = torch.cat([gc.build_indexes(s).contiguous().reshape(-1) for s in scales.chunk(5, 1)]).cpu().numpy()
    sym = torch.cat([torch.round(a - m).int().contiguous().reshape(-1) for a, m in zip(y.chunk(5, 1), means.chunk(5, 1))]).cpu().numpy()
    assert rans_c.encode(sym, idx, cdf, ln, off) == enc["strings"][0][0], "y bitstream differs from the C oracle coder"
    assert rans_py.RansEncoder().encode_with_indexes(sym.tolist(), idx.tolist(), cdf.tolist(), ln.tolist(), off.tolist()) == enc["strings"][0][0]
    out, words = rans_c.decode(enc["strings"][0][0], idx, cdf, ln, off)
    assert (out == sym).all() and words * 4 == len(enc["strings"][0][0])
    # bitrate sanity vs the likelihood estimate
    bits = 8 * (len(enc["strings"][0][0]) + len(enc["strings"][1][0]))
    est = -(torch.log2(fwd["likelihoods"]["y"]).sum() + torch.log2(fwd["likelihoods"]["z"]).sum()).item()
    # (random-weight model: ~5 % of the elements sit at the 1e-9 likelihood floor = 30 "estimated" bits each, while the
    # coder's bypass escape spends fewer, so the real stream is shorter than the estimate; only a sanity band here)
    assert 0.6 * est < bits < 1.1 * est, (bits, est)


def test_train_engine_steps(dev):
    """Fused step (flat arenas, direct gradient writes, batched transposes, fused AdamW): first-step gradients equal plain
    autograd's; eager and hipGraph replay give bit-identical loss sequences (deterministic eval-mode rounding); loss falls."""
    from clc_amd import models as pm
    from clc_amd.train import RateDistortionLoss, TrainEngine
    from clc_amd.recipe import apply_weight_recipe

    x, refs = _inputs(2, 1)
    xd, rd = x.to(dev), [r.to(dev) for r in refs]
    # reference gradients: plain autograd, no engine
    m0 = pm.CLC(N=64, num_ref_frames=1).to(dev).eval()
    apply_weight_recipe(m0, 0)
    RateDistortionLoss(0.0067)(m0(xd, rd), xd)["loss"].backward()
    ref_grads = {n: p.grad.clone() for n, p in m0.named_parameters() if p.grad is not None}
    losses = {}
    for use_graph in (False, True):
        m = pm.CLC(N=64, num_ref_frames=1).to(dev)
        apply_weight_recipe(m, 0)
        eng = TrainEngine(m, lmbda=0.0067, use_graph=use_graph, train_mode=False)
        if not use_graph:
            eng._discover(xd, rd)
            eng._fwd_bwd(xd, rd)
            worst = 0.0
            for n, p in m.named_parameters():
                if n in ref_grads and not n.endswith(".quantiles"):
                    d = ref_grads[n].abs().max().item()
                    if d > 1e-12:
                        worst = max(worst, (p.grad - ref_grads[n]).abs().max().item() / d)
            assert worst < 1e-5, f"direct-write gradients differ from autograd: {worst}"
        seq = [eng.step(xd, rd)["loss"].item() for _ in range(8 if not use_graph else 6)]
        assert all(math.isfinite(v) for v in seq), seq
        losses[use_graph] = seq
    # the graph warm-up steps are rolled back before capture: the i-th replay IS the i-th training step
    assert losses[False][0:6] == losses[True][0:6], (losses[False], losses[True])
    assert min(losses[False][3:]) < losses[False][0], losses[False]


@pytest.mark.parametrize("fwd", ["direct", "default"])
def test_config2_bs8_r3_train_mode_step_vs_oracle(dev, fwd):
    """BASELINE configs[2] at its quoted size (CLC lambda 0.025 MSE, 256x256, batch 8, 3 references), TRAIN mode with the noise
    injected identically on both sides: loss terms and every gradient vs the oracle (bs2 only before)."""
    from clc_amd.train import RateDistortionLoss as PRD
    from oracle.loss import RateDistortionLoss as ORD

    o, p = _pair("clc", 3, dev)
    o.train()
    p.train()
    x, refs = _inputs(8, 3, smooth=False)
    g = torch.Generator().manual_seed(78)
    ny = torch.rand((8, 320, 16, 16), generator=g) - 0.5
    nz = torch.rand((8, 192, 4, 4), generator=g) - 0.5
    with _injected_noise(ny, nz, dev):
        oo = o(x, refs)
        lo = ORD(0.025)(oo, x)
        lo["loss"].backward()
        xd, rd = x.to(dev), [r.to(dev) for r in refs]
        with (_direct_forward() if fwd == "direct" else contextlib.nullcontext()):
            po = p(xd, rd)
        lp = PRD(0.025)(po, xd)
        lp["loss"].backward()
    flips = _symbol_flips(oo, po)
    for k in ("loss", "bpp_loss", "mse_loss"):
        assert abs(lo[k].item() - lp[k].item()) <= 2e-4 * max(1.0, abs(lo[k].item())), (k, lo[k].item(), lp[k].item())
    assert flips <= (8 if fwd == "direct" else 65), flips   # of 655 360 latent elements (see test_config1_bs8_train_mode_step_vs_oracle)
    checked, worst = _grad_parity(o, p, tol=4e-3, flips=flips)   # (8-image / 512x512 / N=128 reductions: measured worst 1.1e-3 .. 3.2e-3 of a tensor's largest element, fp32 summation order)
    print("configs[2] bs8 R=3 train-mode: checked", checked, "worst rel err", worst, "symbol flips", flips)


def test_backward_parity_wide_model(dev):
    """N=128 (train_CLC.py:356's default width): loss terms and every gradient vs the oracle (forward-only before)."""
    from clc_amd import models as pm
    from clc_amd.train import RateDistortionLoss as PRD
    from oracle import graph as og
    from oracle.loss import RateDistortionLoss as ORD
    from oracle.recipe import apply_weight_recipe

    o = og.CLC(N=128, num_ref_frames=1).eval()
    apply_weight_recipe(o, 2)
    p = pm.CLC(N=128, num_ref_frames=1)
    p.load_state_dict(o.state_dict())
    p = p.to(dev).eval()
    x, refs = _inputs(1, 1)
    lo = ORD(0.0067)(o(x, refs), x)
    lo["loss"].backward()
    xd, rd = x.to(dev), [r.to(dev) for r in refs]
    lp = PRD(0.0067)(p(xd, rd), xd)
    lp["loss"].backward()
    for k in ("loss", "bpp_loss", "mse_loss"):
        assert abs(lo[k].item() - lp[k].item()) <= 2e-4 * max(1.0, abs(lo[k].item())), (k, lo[k].item(), lp[k].item())
    checked, worst = _grad_parity(o, p, tol=4e-3)   # (8-image / 512x512 / N=128 reductions: measured worst 1.1e-3 .. 3.2e-3 of a tensor's largest element, fp32 summation order)
    print("N=128: checked", checked, "worst rel err", worst)


def test_max_support_slices_variants(dev):
    """max_support_slices: the reference sizes every slice net for min(i, 5) support slices (CLC_run.py:402-474), so only 4 and 5
    (and -1 = all) give consistent channel counts — 4 reads exactly what 5 reads — and anything smaller fails on a channel mismatch
    in the reference too.  The shared support / gradient buffers (ops.SliceSupport) need every slice to read its predecessor
    (ADVICE r2): they are enabled for 4 and 5 only; a smaller value raises instead of walking off a filter."""
    from clc_amd import lib, models as pm
    from clc_amd.recipe import apply_weight_recipe
    from clc_amd.train import RateDistortionLoss as PRD

    x, refs = _inputs(2, 1)
    xd, rd = x.to(dev), [r.to(dev) for r in refs]
    res = {}
    for ms in (5, 4, -1):
        p = pm.CLC(N=64, num_ref_frames=1, max_support_slices=ms)
        apply_weight_recipe(p, 0)
        p = p.to(dev).eval()
        out = PRD(0.0067)(p(xd, rd), xd)
        out["loss"].backward()
        torch.cuda.synchronize()
        res[ms] = (out["loss"].item(), {n: q.grad.clone() for n, q in p.named_parameters() if q.grad is not None})
    assert res[5][0] == res[4][0]
    for n in res[5][1]:
        assert torch.equal(res[5][1][n], res[4][1][n]), n
    # -1 takes the concatenation path (no shared buffers): same forward bits, gradients equal up to accumulation order
    assert abs(res[5][0] - res[-1][0]) <= 1e-6 * abs(res[5][0])
    worst = max((res[5][1][n] - res[-1][1][n]).abs().max().item() / max(res[5][1][n].abs().max().item(), 1e-12) for n in res[5][1])
    assert worst < 2e-4, worst
    p = pm.CLC(N=64, num_ref_frames=1, max_support_slices=2).to(dev).eval()
    with pytest.raises(lib.ClcError, match="does not match the filter"):
        with torch.no_grad():
            p(xd, rd)
