"""cheng2020 (clc_amd/models/cheng.py) at N = 24 against the float64 plain-torch restatement (tests/cheng_ref.py): a seeded 2x3x64x128
batch (latent 4x8) and a 1x3x128x192 image (latent 8x12).  Weights: the recipe with the scalings of tests/test_ar_model_gpu.py moved to
this model's layers (the last convolution of g_a x 20, the last layer of h_s x 4 and + 0.6, entropy_parameters.4.weight x 8 and + 0.6 on
the scale entries of its bias), so that the predicted scales leave the 0.11 bound.

Training step (both classes at K = 3, the attention class at K = 1): every uniform draw of y's shape is replaced by one fixed tensor on
both sides; |d bpp| <= 1e-4, |d PSNR| <= 0.01 dB, per-parameter gradient error <= 5e-3 of the gradient's largest element, every parameter
with a non-zero reference gradient.

K = 3 codec: decompress returns exactly g_s(round(y)).clamp(0, 1); the decoder's y_hat is the encoder's bit for bit; H W N symbols in
ar_wavefront_order; an image's bytes do not depend on the batch; the container round-trips; decompress makes one device -> host copy per
wavefront step, W + 3 (H - 1), and with the one upload of the decoded z that is W + 3 (H - 1) + 1 host hops per batch (counted).

Causal consistency: the GPU's parameter rows against ONE teacher-forced float64 pass from the GPU's y_hat, within 2e-5 of the tensor's
largest magnitude; the symbols are round(y) exactly, with no exclusion, because no mean is involved.
"""
import copy
import math

import numpy as np
import pytest
import torch

import cheng_ref
from test_ar_model_gpu import _images, _injected_noise

pytestmark = pytest.mark.gpu

N_ = 24
CL = torch.channels_last
_PAIRS = {}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _pair(name, K, dev):
    """(float64 restatement, product model on the GPU) with the same weights; tables built"""
    if (name, K) in _PAIRS:
        return _PAIRS[(name, K)]
    from clc_amd import models
    from clc_amd.recipe import apply_weight_recipe

    r = getattr(cheng_ref, name)(N_, K)
    apply_weight_recipe(r, 3)
    last = 7 if name == "Cheng2020Attention" else 6
    with torch.no_grad():
        r.g_a[last].weight.mul_(20.0)
        r.h_s[8].weight.mul_(4.0)
        r.h_s[8].bias.add_(0.6)
        r.entropy_parameters[4].weight.mul_(8.0)
        r.entropy_parameters[4].bias[:K * N_].add_(0.6)
    p = getattr(models, name)(N_, K)
    p.load_state_dict(r.state_dict())
    o = copy.deepcopy(r).double()
    o.update(force=True)
    p = p.to(dev)
    p.update(force=True)
    _PAIRS[(name, K)] = (o, p)
    return o, p


@pytest.mark.parametrize("name,K", [("Cheng2020Anchor", 3), ("Cheng2020Attention", 3), ("Cheng2020Attention", 1)])
def test_training_step_against_float64(dev, name, K):
    from clc_amd.train import RateDistortionLoss as PRD
    from oracle.loss import RateDistortionLoss as ORD

    o, p = (copy.deepcopy(m) for m in _pair(name, K, dev))
    o.train()
    p.train()
    x = _images(2, 64, 128)
    g = torch.Generator().manual_seed(5)
    ny = torch.rand((2, N_, 4, 8), generator=g) - 0.5
    nz = torch.rand((2, N_, 1, 2), generator=g) - 0.5
    with _injected_noise(ny, nz):
        oo = o(x.double())
        lo = ORD(0.0067)(oo, x.double())
        lo["loss"].backward()
        xd = x.to(dev)
        po = p(xd)
        lp = PRD(0.0067)(po, xd)
        lp["loss"].backward()
    assert po["x_hat"].shape == (2, 3, 64, 128) and po["likelihoods"]["y"].shape == (2, N_, 4, 8) and po["likelihoods"]["z"].shape == (2, N_, 1, 2)
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
    for n in ("context_prediction.weight", "context_prediction.bias", "entropy_parameters.0.weight", "entropy_parameters.4.bias", "h_s.8.weight"):
        assert og[n].grad is not None and og[n].grad.abs().max().item() > 1e-12, n
    if K > 1:   # all three parameter groups of the mixture carry gradient
        gb = og["entropy_parameters.4.bias"].grad.reshape(3, K * N_)
        assert all(float(gb[i].abs().max()) > 1e-12 for i in range(3))
    assert checked >= 60, checked


class _count_d2h:
    """counts device -> host copies (Tensor.copy_ into a CPU tensor from a GPU tensor, Tensor.cpu() of a GPU tensor)"""

    def __enter__(self):
        self.n = 0
        self.copy_, self.cpu = torch.Tensor.copy_, torch.Tensor.cpu
        me = self

        def copy_(t, src, *a, **k):
            if not t.is_cuda and isinstance(src, torch.Tensor) and src.is_cuda:
                me.n += 1
            return me.copy_(t, src, *a, **k)

        def cpu(t, *a, **k):
            if t.is_cuda:
                me.n += 1
            return me.cpu(t, *a, **k)

        torch.Tensor.copy_, torch.Tensor.cpu = copy_, cpu
        return self

    def __exit__(self, *exc):
        torch.Tensor.copy_, torch.Tensor.cpu = self.copy_, self.cpu
        return False


def test_host_hop_is_one_download_and_one_upload(dev):
    from clc_amd.models.coding import HostHop

    hop = HostHop(16, 16, dev)
    wrote = torch.arange(16, dtype=torch.int32).reshape(2, 8) * 3 - 7
    down, up = hop.step(16, 16)
    down.view(2, 8).copy_(wrote.to(dev))   # what a finish kernel leaves
    up.fill_(-1)
    seen = []

    def decode(down_np, up_np):
        seen.append(down_np.copy())
        up_np[:] = down_np[::-1] + 100

    with _count_d2h() as c:
        hop.run(decode)
    assert c.n == 1 and len(seen) == 1
    assert seen[0].dtype == np.int32 and seen[0].tolist() == wrote.reshape(-1).tolist()   # the callback saw what the device wrote
    assert up.cpu().tolist() == (wrote.reshape(-1).flip(0) + 100).tolist()               # the upload region holds what it wrote
    short_down, short_up = hop.step(8, 4)   # a shorter step moves its own elements only
    assert short_down.data_ptr() == down.data_ptr() and short_up.data_ptr() == up.data_ptr() and (short_down.numel(), short_up.numel()) == (8, 4)
    with _count_d2h() as c:
        hop.run(lambda down_np, up_np: up_np.fill(len(down_np)))
    assert c.n == 1 and up.cpu().tolist()[:5] == [8, 8, 8, 8, int(wrote.reshape(-1)[11]) + 100]


def test_mixture_codec(dev):
    from clc_amd import ans, codec, lib, models
    from clc_amd.models import ar_wavefront_order

    _, p = _pair("Cheng2020Attention", 3, dev)
    p.eval()
    x = _images(1, 128, 192).to(dev)
    y, params, z_strings, z_size = p._code_inputs(x)
    B, N, H, W = y.shape
    assert (B, N, H, W) == (1, N_, 8, 12) and tuple(z_size) == (2, 3)
    triples, y_hat = p._gmm_encode(y, params)
    assert torch.equal(y_hat, torch.round(y)) and int(y_hat.abs().max()) >= 2
    assert tuple(triples.shape) == (1, H * W, N_, 3)   # H W N symbols, in ar_wavefront_order:
    # the triples of pixel i of the order are those of a one-pixel call on that pixel
    order = ar_wavefront_order(H, W)
    for i in (0, 1, 17, H * W - 1):
        px = torch.tensor([order[i]], dtype=torch.int32, device=dev)
        ws = p._gmm_workspace(1, dev)
        p._ar_chain(px, 1, H, W, y_hat, params.contiguous(memory_format=CL), ws, p._ar_filters())
        one = torch.zeros((1, 1, N_, 3), device=dev, dtype=torch.int32)
        from clc_amd import ops

        ops.gmm_finish_encode(ws["gp"], N_, 3, px, y.contiguous(memory_format=CL), y_hat.clone(), one)
        assert torch.equal(one[0, 0], triples[0, i]), i
    esc = float((triples[..., 2] >= 0).float().mean())
    print(f"escaped symbols: {100 * esc:.2f} %")
    assert esc < 0.5 and int((triples[..., 1] < 60000).sum()) > 0   # not a degenerate stream

    item = p.compress(x)
    assert item["strings"][1] == z_strings and len(item["strings"][0]) == 1
    assert item["strings"][0][0] == ans.encode_direct(triples[0].cpu().numpy())
    with _count_d2h() as c:
        z_calls, orig = [], p.entropy_bottleneck.decompress
        p.entropy_bottleneck.decompress = lambda *a, **k: (z_calls.append(1), orig(*a, **k))[1]
        try:
            dec = p.decompress(item["strings"], item["shape"])
        finally:
            del p.entropy_bottleneck.decompress
    steps = W + 3 * (H - 1)
    print(f"decompress: {c.n} device -> host copies, {len(z_calls)} z upload")
    assert c.n == steps and c.n + len(z_calls) == steps + 1
    assert torch.equal(dec["x_hat"], p._synthesis(torch.round(y)).clamp(0, 1))
    assert torch.equal(p._gmm_decode(item["strings"][0], params), y_hat)   # the decoder's y_hat is the encoder's, bit for bit

    # an image's streams do not depend on the batch around it, and decode at batch 1
    xb = _images(3, 64, 128).to(dev)
    both, one = p.compress(xb), p.compress(xb[1:2])
    assert len(both["strings"][0]) == 3 and tuple(both["shape"]) == (1, 2)
    assert one["strings"][0][0] == both["strings"][0][1] and one["strings"][1][0] == both["strings"][1][1]
    dec_b = p.decompress(both["strings"], both["shape"])
    dec_1 = p.decompress([[both["strings"][0][1]], [both["strings"][1][1]]], both["shape"])
    yb = p._code_inputs(xb)[0]
    assert torch.equal(dec_b["x_hat"], p._synthesis(torch.round(yb)).clamp(0, 1))
    assert torch.equal(dec_1["x_hat"], dec_b["x_hat"][1:2])
    # the container
    blob = codec.pack_item(one, image_hw=(64, 128))
    strings, shape, meta = codec.unpack(blob)
    assert strings[0][0] == one["strings"][0][0] and strings[1][0] == one["strings"][1][0] and tuple(shape) == (1, 2)
    assert meta["image_hw"] == (64, 128)
    assert torch.equal(p.decompress(strings, shape)["x_hat"], dec_1["x_hat"])
    with pytest.raises(ValueError, match="multiples of 64"):
        p.compress(torch.zeros(1, 3, 64, 100, device=dev))

    # another model class beside it keeps its bytes, and the kernel_config tag is that of a default build
    from clc_amd.recipe import apply_weight_recipe

    m = models.JointAutoregressiveHierarchicalPriors(12, 24)
    apply_weight_recipe(m, 3)
    m = m.to(dev).eval()
    m.update(force=True)
    before = m.compress(xb[:1])
    p.decompress(one["strings"], one["shape"])
    after = m.compress(xb[:1])
    assert before["strings"] == after["strings"] and before["kernel_config"] == after["kernel_config"] == one["kernel_config"]
    assert lib.load().clc_kernel_config_tag() == 6


@pytest.mark.parametrize("B,h,w", [(2, 64, 128), (1, 128, 192)])
def test_causal_consistency_against_float64(dev, B, h, w):
    o, p = _pair("Cheng2020Anchor", 3, dev)
    o.eval()
    p.eval()
    K = 3
    x = _images(B, h, w).to(dev)
    y, params, _, _ = p._code_inputs(x)
    triples, y_hat = p._gmm_encode(y, params)
    _, _, H, W = y.shape
    # the GPU's parameter rows of every pixel from the finished y_hat: the chain on the raster list (bit-identical to the coder's steps)
    _, pix = p._ar_pixels([[(hh, ww) for hh in range(H) for ww in range(W)]], dev)
    ws = p._gmm_workspace(B * H * W, dev)
    p._ar_chain(pix, B, H, W, y_hat, params.contiguous(memory_format=CL), ws, p._ar_filters())
    gp = ws["gp"].reshape(B, H * W, 3 * K * N_).double().cpu()
    gp64 = o.teacher_forced_params(y_hat.double().cpu(), params.double().cpu()).permute(0, 2, 3, 1).reshape(B, H * W, 3 * K * N_)
    KN = K * N_
    for name, lo in (("scales", 0), ("means", KN), ("weights", 2 * KN)):
        got, ref = gp[..., lo:lo + KN], gp64[..., lo:lo + KN]
        err = (got - ref).abs().max().item() / ref.abs().max().item()
        print(f"{H}x{W} {name}: GPU against float64 {err:.2e} of the largest magnitude {ref.abs().max().item():.3f}")
        assert err <= 2e-5, (name, err)
    assert gp64[..., :KN].max().item() > 1.0 and gp64[..., KN:2 * KN].abs().max().item() > 1.0   # informative, not clamped
    assert torch.equal(y_hat.cpu(), torch.round(y).cpu())   # the symbols are round(y): no mean is involved, nothing is excluded
    # and the coded triples are those of the float64 rule on the GPU's rows wherever the centre is not next to a half-integer
    from clc_amd.models import ar_wavefront_order

    order = torch.tensor([hh * W + ww for hh, ww in ar_wavefront_order(H, W)])
    g = ws["gp"].reshape(B, H * W, 3, K, N_)[:, order].cpu()   # stream order
    sc, mu, lg = (g[:, :, i].permute(0, 1, 3, 2).reshape(-1, K) for i in range(3))
    rows64, offs64 = cheng_ref.cdf_rows(sc, mu, lg, torch.float64)
    sym = torch.round(y).permute(0, 2, 3, 1).reshape(B, H * W, N_)[:, order].reshape(-1).cpu()
    t = triples.reshape(-1, 3).cpu()
    inside = (sym.long() - offs64 >= 0) & (sym.long() - offs64 < cheng_ref.L)
    m64 = (torch.softmax(lg.double(), 1) * mu.double()).sum(1)
    safe = ((m64 - torch.floor(m64)) - 0.5).abs() > 1e-4
    assert 1.0 - safe.double().mean().item() <= 0.01
    assert torch.equal((t[:, 2] < 0)[safe], inside[safe])
    v = (sym.long() - offs64).clamp(0, cheng_ref.L - 1)
    start64 = rows64.gather(1, v[:, None])[:, 0]
    pick = safe & inside
    assert int((t[:, 0].long() - start64)[pick].abs().max()) <= 1


def test_single_gaussian_codec(dev):
    """K = 1 on the attention class: the parent's round-trip and schedule checks"""
    from clc_amd import models

    _, p = _pair("Cheng2020Attention", 1, dev)
    p.eval()
    assert isinstance(p, models.JointAutoregressiveHierarchicalPriors)
    x = _images(1, 128, 192).to(dev)
    y, params, z_strings, z_size = p._code_inputs(x)
    assert tuple(y.shape) == (1, N_, 8, 12) and tuple(z_size) == (2, 3)
    sym_w, idx_w, yhat_w = p._ar_encode(y, params, "wavefront")
    sym_r, idx_r, yhat_r = p._ar_encode(y, params, "raster")
    assert torch.equal(sym_w, sym_r) and torch.equal(idx_w, idx_r) and torch.equal(yhat_w, yhat_r)
    assert int(sym_w.abs().max()) >= 2 and int(idx_w.max()) > int(idx_w.min())   # not a degenerate stream
    item = p.compress(x)
    item_r = p.compress(x, order="raster")
    assert item["strings"][0] == item_r["strings"][0] and item["strings"][1] == item_r["strings"][1] == z_strings
    dec = p.decompress(item["strings"], item["shape"])
    assert torch.equal(dec["x_hat"], p._synthesis(yhat_w).clamp(0, 1))
    xb = _images(2, 64, 128).to(dev)
    both, one = p.compress(xb), p.compress(xb[:1])
    assert one["strings"][0][0] == both["strings"][0][0] and one["strings"][1][0] == both["strings"][1][0]
