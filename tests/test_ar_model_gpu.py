"""JointAutoregressiveHierarchicalPriors (mbt2018; clc_amd/models/hyperprior.py) at N = 12, M = 24 against the float64 plain-torch
restatement (tests/ar_ref.py): a seeded 2x3x64x128 batch (latent 4x8) and a 1x3x128x192 image (latent 8x12).  Weights: the recipe with
the scalings of tests/test_hyperprior_gpu.py, plus entropy_parameters.4.weight x 8 and + 0.6 on the first M entries of its bias, so that
the predicted scales reach about 1.6 and the means +-1.4 instead of sitting under the 0.11 bound.

Training step: both uniform draws of y's shape (the context model's noisy y_hat and the likelihood's) are replaced by one fixed tensor on
both sides (the technique of tests/test_hyperprior_gpu.py::_injected_noise); |d bpp| <= 1e-4, |d PSNR| <= 0.01 dB, per-parameter
gradient error <= 5e-3 of the gradient's largest element, every parameter with a non-zero reference gradient.

Codec: the wavefront and the raster schedule give equal symbols, indexes, y_hat bits and stream bytes; decompress returns exactly
g_s(encoder y_hat).clamp(0, 1); an image's streams do not depend on the batch; the container round-trips.

Causal consistency: the sequential coder cannot be compared with float64 step by step (one flipped rounding changes everything after
it), so the encoder's final y_hat is taken from the GPU and every pixel's (scale, mean) is recomputed in ONE teacher-forced parallel
pass of the float64 restatement (masked conv of the whole y_hat, then entropy_parameters).  That pass equals the restatement's own
sequential loop to 1e-15 (checked here on the CPU; evaluated in patch-row form it is bit-identical to the loop, as one whole-map
convolution it sits 0.9e-15 .. 1.2e-15 away, a few float64 ulps of another BLAS summation order: see tests/ar_ref.py).  GPU scales and
means within 2e-5 of the tensor's largest magnitude; sym == round(y - mean64) wherever the fractional part of y - mean64 is farther
than 1e-4 from 1/2; idx == build_indexes(scale64) wherever the scale is farther than 1e-4 (relative) from every table entry; at most
1 % of each tensor may be excluded (a condition, not a tolerance: the float64 restatement alone excludes at most 0.02 % of symbols and
0.11 % of indexes on these inputs).
"""
import copy
import math

import pytest
import torch

import ar_ref

pytestmark = pytest.mark.gpu

N_, M_ = 12, 24
CL = torch.channels_last


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pair(dev):
    """(float64 restatement, product model on the GPU) with the same weights; tables built"""
    from clc_amd import models
    from clc_amd.recipe import apply_weight_recipe

    r = ar_ref.JointAutoregressiveHierarchicalPriors(N_, M_)
    apply_weight_recipe(r, 3)
    with torch.no_grad():
        r.g_a[6].weight.mul_(20.0)
        r.h_s[4].weight.mul_(4.0)
        r.h_s[4].bias.add_(0.6)
        r.entropy_parameters[4].weight.mul_(8.0)
        r.entropy_parameters[4].bias[:M_].add_(0.6)
    p = models.JointAutoregressiveHierarchicalPriors(N_, M_)
    p.load_state_dict(r.state_dict())
    o = copy.deepcopy(r).double()
    o.update(force=True)
    p = p.to(dev)
    p.update(force=True)
    return o, p


def _images(B, h, w):
    from clc_amd.recipe import synthetic_image

    return synthetic_image(B, h, w, 321, smooth=True)


class _injected_noise:
    """Both sides draw their quantisation noise with Tensor.uniform_(-0.5, 0.5) on a fresh tensor: replace those draws by fixed
    tensors, matched by shape (the restatement's EntropyBottleneck works on [C, 1, B*H*W]).  Every draw of y's shape takes ny."""

    def __init__(self, ny, nz):
        self.ny, self.nz = ny, nz

    def __enter__(self):
        self.orig = torch.Tensor.uniform_
        me = self

        def fake(t, a=0.0, b=1.0, generator=None):
            if (a, b) != (-0.5, 0.5):
                return me.orig(t, a, b, generator=generator)
            shp = tuple(t.shape)
            if shp == tuple(me.nz.shape):
                src = me.nz
            elif len(shp) == 3 and t.numel() == me.nz.numel():
                src = me.nz.permute(1, 0, 2, 3).reshape(shp[0], 1, -1)
            elif shp == tuple(me.ny.shape):
                src = me.ny
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


def test_training_step_against_float64(dev, pair):
    from clc_amd.train import RateDistortionLoss as PRD
    from oracle.loss import RateDistortionLoss as ORD

    o, p = copy.deepcopy(pair[0]), copy.deepcopy(pair[1])
    o.train()
    p.train()
    x = _images(2, 64, 128)
    g = torch.Generator().manual_seed(5)
    ny = torch.rand((2, M_, 4, 8), generator=g) - 0.5
    nz = torch.rand((2, N_, 1, 2), generator=g) - 0.5
    with _injected_noise(ny, nz):
        oo = o(x.double())
        lo = ORD(0.0067)(oo, x.double())
        lo["loss"].backward()
        xd = x.to(dev)
        po = p(xd)
        lp = PRD(0.0067)(po, xd)
        lp["loss"].backward()
    assert po["x_hat"].shape == (2, 3, 64, 128) and po["likelihoods"]["y"].shape == (2, M_, 4, 8) and po["likelihoods"]["z"].shape == (2, N_, 1, 2)
    d_bpp = abs(lo["bpp_loss"].item() - lp["bpp_loss"].item())
    psnr = lambda m: -10 * math.log10(m)
    d_psnr = abs(psnr(lo["mse_loss"].item()) - psnr(lp["mse_loss"].item()))
    print(f"bpp {lo['bpp_loss'].item():.6f} / {lp['bpp_loss'].item():.6f}  psnr {psnr(lo['mse_loss'].item()):.4f} / {psnr(lp['mse_loss'].item()):.4f}")
    assert d_bpp <= 1e-4, d_bpp
    assert d_psnr <= 0.01, d_psnr
    og = dict(o.named_parameters())
    checked, worst = 0, (0.0, "")
    for n, prm in p.named_parameters():
        go = og[n].grad
        if go is None:
            assert prm.grad is None or float(prm.grad.abs().max()) == 0.0, f"{n}: the restatement has no grad"
            continue
        assert prm.grad is not None, f"{n}: missing grad"
        denom = go.abs().max().item()
        if denom < 1e-12:
            continue
        err = (prm.grad.double().cpu() - go).abs().max().item() / denom
        worst = max(worst, (err, n))
        checked += 1
        assert err <= 5e-3, f"{n}: grad rel err {err:.3e}"
    print(f"checked {checked} gradients, worst {worst}")
    for n in ("context_prediction.weight", "context_prediction.bias", "entropy_parameters.0.weight", "entropy_parameters.4.bias"):
        assert og[n].grad is not None and og[n].grad.abs().max().item() > 1e-12, n
    assert checked >= 48, checked
    # the masked taps were zeroed in place by the forward, on both sides
    mask = p.context_prediction.mask
    assert float((p.context_prediction.weight.detach() * (1 - mask)).abs().max()) == 0.0


def test_codec_schedules_round_trip_and_container(dev, pair):
    from clc_amd import codec

    _, p = pair
    p.eval()
    x = _images(1, 128, 192).to(dev)
    y, params, z_strings, z_size = p._code_inputs(x)
    assert tuple(y.shape) == (1, M_, 8, 12) and tuple(z_size) == (2, 3)
    sym_w, idx_w, yhat_w = p._ar_encode(y, params, "wavefront")
    sym_r, idx_r, yhat_r = p._ar_encode(y, params, "raster")
    assert sym_w.shape == (1, 96, M_) and sym_w.dtype == torch.int32
    assert torch.equal(sym_w, sym_r) and torch.equal(idx_w, idx_r) and torch.equal(yhat_w, yhat_r)
    assert int(sym_w.abs().max()) >= 2 and int(idx_w.max()) > int(idx_w.min())   # not a degenerate stream
    item = p.compress(x)
    item_r = p.compress(x, order="raster")
    assert item["strings"][0] == item_r["strings"][0] and item["strings"][1] == item_r["strings"][1] == z_strings
    assert len(item["strings"]) == 2 and len(item["strings"][0]) == 1 and tuple(item["shape"]) == (2, 3)
    dec = p.decompress(item["strings"], item["shape"])
    assert torch.equal(dec["x_hat"], p._synthesis(yhat_w).clamp(0, 1))
    # an image's streams do not depend on the batch around it
    xb = _images(2, 64, 128).to(dev)
    both, one = p.compress(xb), p.compress(xb[:1])
    assert len(both["strings"][0]) == 2 and tuple(both["shape"]) == (1, 2)
    assert one["strings"][0][0] == both["strings"][0][0] and one["strings"][1][0] == both["strings"][1][0]
    dec_b = p.decompress(both["strings"], both["shape"])
    yb, pb, _, _ = p._code_inputs(xb)
    assert torch.equal(dec_b["x_hat"], p._synthesis(p._ar_encode(yb, pb)[2]).clamp(0, 1))
    # the container
    blob = codec.pack_item(one, image_hw=(64, 128))
    strings, shape, meta = codec.unpack(blob)
    assert strings[0][0] == one["strings"][0][0] and strings[1][0] == one["strings"][1][0] and tuple(shape) == (1, 2)
    assert meta["image_hw"] == (64, 128)
    assert torch.equal(p.decompress(strings, shape)["x_hat"], dec_b["x_hat"][:1])
    with pytest.raises(ValueError, match="multiples of 64"):
        p.compress(torch.zeros(1, 3, 64, 100, device=dev))
    with pytest.raises(ValueError, match="multiples of 64"):
        p(torch.zeros(1, 3, 64, 100, device=dev))


@pytest.mark.parametrize("B,h,w", [(2, 64, 128), (1, 128, 192)])
def test_causal_consistency_against_float64(dev, pair, B, h, w):
    from clc_amd import ops

    o, p = pair
    o.eval()
    p.eval()
    x = _images(B, h, w).to(dev)
    y, params, _, _ = p._code_inputs(x)
    sym, idx, y_hat = p._ar_encode(y, params)
    _, _, H, W = y.shape
    # the GPU's (scales | means) of every pixel from the finished y_hat: the chain on the full list (bit-identical to the coder's steps)
    steps, pix = p._ar_pixels([[(hh, ww) for hh in range(H) for ww in range(W)]], dev)
    ws = p._ar_workspace(B * H * W, dev)
    p._ar_chain(pix, B, H, W, y_hat, params.contiguous(memory_format=CL), ws, p._ar_filters())
    gp = ws["gp"].reshape(B, H * W, 2 * M_).double().cpu()
    sc_gpu, mu_gpu = gp[..., :M_], gp[..., M_:]
    yh_rows = y_hat.permute(0, 2, 3, 1).reshape(B, H * W, M_)
    assert torch.equal(yh_rows, sym.float() + ws["gp"].reshape(B, H * W, 2 * M_)[..., M_:]), "y_hat is sym + mean of the same chain"

    y64, p64, yh64 = y.double().cpu(), params.double().cpu(), y_hat.double().cpu()
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(B, H * W, M_)
    sc64, mu64 = (rows(t) for t in o.teacher_forced(yh64, p64))
    # the restatement with itself: its sequential loop against the teacher-forced pass on the loop's own y_hat
    # (one BLAS thread for the two sides: a threaded BLAS may split K differently for a batch of 2 and a batch of 64 samples)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        _, _, yh_loop, sc_loop, mu_loop = o.compress_ar(y64, p64)
        sc_tf, mu_tf = o.teacher_forced(yh_loop, p64)
    finally:
        torch.set_num_threads(threads)
    for name, a, b in (("scales", sc_tf, sc_loop), ("means", mu_tf, mu_loop)):
        gap = (a - b).abs().max().item()
        print(f"{H}x{W} float64 teacher-forced against loop, {name}: {gap:.2e}")
        assert gap <= 1e-15, (name, gap)
    for name, a, b in zip(("scales", "means"), o.teacher_forced(yh_loop, p64, whole_map=True), (sc_loop, mu_loop)):
        print(f"{H}x{W} (for information) the whole map as one convolution against the loop, {name}: {(a - b).abs().max().item():.2e}")

    for name, got, ref in (("scales", sc_gpu, sc64), ("means", mu_gpu, mu64)):
        err = (got - ref).abs().max().item() / ref.abs().max().item()
        print(f"{H}x{W} {name}: GPU against float64 {err:.2e} of the largest magnitude {ref.abs().max().item():.3f}")
        assert err <= 2e-5, (name, err)
    assert sc64.max().item() > 1.0 and mu64.abs().max().item() > 1.0   # the predictions are informative, not clamped

    d = rows(y64) - mu64
    frac = d - torch.floor(d)
    safe = (frac - 0.5).abs() > 1e-4
    excluded = 1.0 - safe.double().mean().item()
    print(f"{H}x{W} symbols: {100 * excluded:.3f} % excluded")
    assert excluded <= 0.01
    assert torch.equal(sym.cpu()[safe], torch.round(d).int()[safe])

    table = o.gaussian_conditional.scale_table.double()
    # (the raw scale: table[0] is the 0.11 bound itself, so a scale clamped from well below it is safe, one near it is not)
    safe = ((sc64.unsqueeze(-1) - table).abs() > 1e-4 * table).all(-1)
    excluded = 1.0 - safe.double().mean().item()
    print(f"{H}x{W} indexes: {100 * excluded:.3f} % excluded")
    assert excluded <= 0.01
    assert torch.equal(idx.cpu()[safe], rows(o.gaussian_conditional.build_indexes(sc64.reshape(B, H, W, M_).permute(0, 3, 1, 2)))[safe])
