"""ScaleHyperprior / MeanScaleHyperprior (clc_amd/models/hyperprior.py) at N = 12, M = 24 on a seeded 2x3x64x128 batch — y is 4x8,
z is 1x2, so the 5x5 kernels run on maps down to 1x2 — against the float64 plain-torch restatement (tests/hyperprior_ref.py).

Training mode: the quantisation noise is injected identically on both sides (shape-matched replacement of Tensor.uniform_(-0.5, 0.5), the
technique of tests/test_model_gpu.py::_injected_noise), so the forward has no rounding and loss terms and gradients are comparable:
|d bpp| <= 1e-4, |d PSNR| <= 0.01 dB, per-parameter gradient error <= 5e-3 of the gradient's largest element.
Codec: compress -> decompress reproduces the eval forward's x_hat bit for bit, an image's streams do not depend on the batch around it,
and the container round-trips them.
"""
import copy
import math

import pytest
import torch

import hyperprior_ref

pytestmark = pytest.mark.gpu

N_, M_ = 12, 24


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _pair(kind, dev):
    from clc_amd import models
    from clc_amd.recipe import apply_weight_recipe

    r = hyperprior_ref.MODELS[kind](N_, M_)
    apply_weight_recipe(r, 3)
    with torch.no_grad():
        r.g_a[6].weight.mul_(20.0)    # a latent with a few quantisation bins of spread
        r.h_s[4].weight.mul_(4.0)    # predicted scales (and means) of order one: informative likelihoods
        r.h_s[4].bias.add_(0.6)
    p = {"scale": models.ScaleHyperprior, "mean_scale": models.MeanScaleHyperprior}[kind](N_, M_)
    p.load_state_dict(r.state_dict())
    return copy.deepcopy(r).double(), p.to(dev)


def _images(B=2, h=64, w=128):
    from clc_amd.recipe import synthetic_image

    return synthetic_image(B, h, w, 321, smooth=True)


class _injected_noise:
    """Both sides draw their quantisation noise with Tensor.uniform_(-0.5, 0.5) on a fresh tensor: replace those draws by fixed
    tensors, matched by shape (the restatement's EntropyBottleneck works on [C, 1, B*H*W])."""

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


@pytest.mark.parametrize("kind", ["scale", "mean_scale"])
def test_training_step_against_float64(dev, kind):
    from clc_amd.train import RateDistortionLoss as PRD
    from oracle.loss import RateDistortionLoss as ORD

    o, p = _pair(kind, dev)
    o.train()
    p.train()
    x = _images()
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
    print(f"{kind}: bpp {lo['bpp_loss'].item():.6f} / {lp['bpp_loss'].item():.6f}  psnr {psnr(lo['mse_loss'].item()):.4f} / {psnr(lp['mse_loss'].item()):.4f}")
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
    print(f"{kind}: checked {checked} gradients, worst {worst}")
    assert checked >= 40, checked


@pytest.mark.parametrize("kind", ["scale", "mean_scale"])
def test_codec_round_trip(dev, kind):
    from clc_amd import codec

    _, p = _pair(kind, dev)
    p.eval()
    p.update(force=True)
    x = _images().to(dev)
    with torch.no_grad():
        fwd = p(x)
    item = p.compress(x)
    assert len(item["strings"]) == 2 and len(item["strings"][0]) == 2 and len(item["strings"][1]) == 2
    assert tuple(item["shape"]) == (1, 2)
    dec = p.decompress(item["strings"], item["shape"])
    assert torch.equal(dec["x_hat"], fwd["x_hat"].clamp(0, 1))
    # image 0 alone: the same two streams, byte for byte
    one = p.compress(x[:1])
    assert one["strings"][0][0] == item["strings"][0][0] and one["strings"][1][0] == item["strings"][1][0]
    # the container
    blob = codec.pack_item(one, image_hw=(64, 128))
    strings, shape, meta = codec.unpack(blob)
    assert strings[0][0] == one["strings"][0][0] and strings[1][0] == one["strings"][1][0] and tuple(shape) == (1, 2)
    assert meta["image_hw"] == (64, 128)
    assert torch.equal(p.decompress(strings, shape)["x_hat"], dec["x_hat"][:1])
    with pytest.raises(ValueError, match="multiples of 64"):
        p.compress(torch.zeros(1, 3, 64, 100, device=dev))
    with pytest.raises(ValueError, match="multiples of 64"):
        p(torch.zeros(1, 3, 64, 100, device=dev))
