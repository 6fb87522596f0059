"""models.Elic2022 (clc_amd/models/elic.py) at scctx_ref.SMALL (N = 8, M = 32, groups (4, 4, 8, 16), ch_widths (12, 8), agg_widths
(40, 24)) against the float64 plain-torch restatement (tests/scctx_ref.py): a seeded 2x3x64x64 batch (latent 4x4) and a 1x3x64x128
image (latent 4x8), the weights of scctx_ref.small_reference().

Training step: both uniform draws of y's shape are replaced by one fixed tensor on both sides (tests/test_ar_model_gpu.py::
_injected_noise); |d bpp| <= 1e-4, |d PSNR| <= 0.01 dB, per-parameter gradient error <= 5e-3 of the gradient's largest element for
every parameter with a non-zero reference gradient.

Codec: decompress(compress(x)) returns exactly g_s(encoder y_hat).clamp(0, 1) of the same batch and the decoder's y_hat equals the
encoder's bit for bit; image 1 of a batch of 3 gives the bytes it gives alone and its stream decodes at batch 1 to the same y_hat
bits; a stream decodes with the symbol count H W M in scctx_order; a model of another class built beside it gives the bytes it gave
before and the kernel_config tag is unchanged.

Causal consistency, as for mbt2018 and mbt2018-checkerboard: from the GPU's final y_hat the restatement's teacher-forced pass gives
every element's (scale, mean) in float64: GPU scales and means within 2e-5 of the tensor's largest magnitude; sym == round(y - mean64)
wherever the fractional part of y - mean64 is farther than 1e-4 from 1/2; idx == build_indexes(scale64) wherever the scale is farther
than 1e-4 (relative) from every table entry; at most 1 % of each tensor may be excluded (a condition, not a tolerance: the restatement
alone excludes at most 0.20 %, tests/test_scctx_cpu.py).
"""
import copy
import math

import numpy as np
import pytest
import torch

import scctx_ref
from test_ar_model_gpu import _images, _injected_noise

pytestmark = pytest.mark.gpu

SMALL = scctx_ref.SMALL
N_, M_ = SMALL["N"], SMALL["M"]
CL = torch.channels_last


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pair(dev):
    """(float64 restatement, product model on the GPU) with the same weights; tables built"""
    from clc_amd import models

    r = scctx_ref.small_reference()
    p = models.Elic2022(**SMALL)
    p.load_state_dict(r.state_dict())
    o = copy.deepcopy(r).double()
    o.update(force=True)
    p = p.to(dev)
    p.update(force=True)
    return o, p


def _rows(t):
    B, C, H, W = t.shape
    return t.permute(0, 2, 3, 1).reshape(B, H * W, C)


def test_training_step_against_float64(dev, pair):
    from clc_amd.train import RateDistortionLoss as PRD
    from oracle.loss import RateDistortionLoss as ORD

    o, p = copy.deepcopy(pair[0]), copy.deepcopy(pair[1])
    o.train()
    p.train()
    x = _images(2, 64, 64)
    g = torch.Generator().manual_seed(5)
    ny = torch.rand((2, M_, 4, 4), generator=g) - 0.5
    nz = torch.rand((2, N_, 1, 1), generator=g) - 0.5
    with _injected_noise(ny, nz):
        oo = o(x.double())
        lo = ORD(0.0067)(oo, x.double())
        lo["loss"].backward()
        xd = x.to(dev)
        po = p(xd)
        lp = PRD(0.0067)(po, xd)
        lp["loss"].backward()
    assert po["x_hat"].shape == (2, 3, 64, 64) and po["likelihoods"]["y"].shape == (2, M_, 4, 4) and po["likelihoods"]["z"].shape == (2, N_, 1, 1)
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
    for n in ("channel_context.1.0.weight", "channel_context.3.4.bias", "spatial_context.0.weight", "spatial_context.3.bias",
              "aggregation.0.0.weight", "aggregation.3.4.bias", "g_a.14.conv_b.3.weight", "g_s.0.conv_a.0.conv.2.weight", "h_s.4.weight"):
        assert og[n].grad is not None and og[n].grad.abs().max().item() > 1e-12, n
    assert checked >= 300, checked
    for k in range(len(SMALL["groups"])):   # exactly 0 on the masked taps
        m = p.spatial_context[k]
        assert float((m.weight.grad * (1 - m.mask)).abs().max()) == 0.0


def test_round_trip_batch_independence_and_symbol_count(dev, pair):
    from clc_amd import ans
    from clc_amd.models import scctx_order

    _, p = pair
    p.eval()
    groups = SMALL["groups"]
    x1 = _images(1, 64, 128).to(dev)
    y, params, z_strings, z_size = p._code_inputs(x1)
    assert tuple(y.shape) == (1, M_, 4, 8) and tuple(z_size) == (1, 2)
    syms, idxs, y_hat = p._scctx_encode(y, params)
    assert [tuple(s.shape) for s in syms] == [(1, 32, c) for c in groups] and all(s.dtype == torch.int32 for s in syms + idxs)
    sym, idx = torch.cat(syms, 2), torch.cat(idxs, 2)
    assert int(sym.abs().max()) >= 2 and int(idx.max()) > int(idx.min())   # not a degenerate stream
    item = p.compress(x1)
    again = p.compress(x1)
    assert item["strings"][0] == again["strings"][0] and item["strings"][1] == again["strings"][1] == z_strings   # run to run
    assert len(item["strings"]) == 2 and len(item["strings"][0]) == 1 and tuple(item["shape"]) == (1, 2) and "kernel_config" in item
    dec = p.decompress(item["strings"], item["shape"])
    assert torch.equal(dec["x_hat"], p._synthesis(y_hat).clamp(0, 1))
    assert torch.equal(p._scctx_decode(item["strings"][0], params), y_hat)   # the decoder's y_hat, bit for bit

    # the stream decodes with the symbol count H W M, in scctx_order, to the encoder's symbols
    order = scctx_order(4, 8, groups)
    assert order.shape == (4 * 8 * M_, 2)
    cdf, ln, off = p.gaussian_conditional.host_tables()
    idx_s = np.ascontiguousarray(idx[0].cpu().numpy()[order[:, 0], order[:, 1]])
    sym_s = sym[0].cpu().numpy()[order[:, 0], order[:, 1]]
    assert item["strings"][0][0] == ans.encode(np.ascontiguousarray(sym_s), idx_s, cdf, ln, off)
    assert np.array_equal(np.asarray(ans.decode(item["strings"][0][0], idx_s, cdf, ln, off)).astype(np.int64), sym_s.astype(np.int64))

    # image 1 of a batch of 3 gives the bytes it gives alone; its stream decodes at batch 1 to the same y_hat bits
    xb = torch.cat((_images(2, 64, 64), _images(1, 64, 64).flip(3)), 0).to(dev)
    xb = xb[[2, 0, 1]].contiguous()
    both = p.compress(xb)
    assert len(both["strings"][0]) == 3 and tuple(both["shape"]) == (1, 1)
    for i in range(3):
        one = p.compress(xb[i:i + 1])
        assert one["strings"][0][0] == both["strings"][0][i] and one["strings"][1][0] == both["strings"][1][i], i
    assert len({s for s in both["strings"][0]}) == 3   # three different images
    yb, pb, _, _ = p._code_inputs(xb)
    _, _, yhat_b = p._scctx_encode(yb, pb)
    dec_b = p.decompress(both["strings"], both["shape"])
    assert torch.equal(dec_b["x_hat"], p._synthesis(yhat_b).clamp(0, 1))
    assert torch.equal(p._scctx_decode(both["strings"][0], pb), yhat_b)
    y1, p1, _, _ = p._code_inputs(xb[1:2])
    assert torch.equal(p._scctx_decode([both["strings"][0][1]], p1), yhat_b[1:2])
    dec_1 = p.decompress([[both["strings"][0][1]], [both["strings"][1][1]]], both["shape"])
    assert torch.equal(dec_1["x_hat"], dec_b["x_hat"][1:2])

    with pytest.raises(ValueError, match="multiples of 64"):
        p.compress(torch.zeros(1, 3, 64, 100, device=dev))
    with pytest.raises(ValueError, match="multiples of 64"):
        p(torch.zeros(1, 3, 64, 100, device=dev))


def test_no_disturbance(dev, pair):
    """a model of another class built beside it gives the bytes it gave before; the kernel_config tag is unchanged"""
    from clc_amd import codec, lib, models
    from clc_amd.recipe import apply_weight_recipe

    _, p = pair
    p.eval()
    tag, hsh = lib.load().clc_kernel_config_tag(), lib.load().clc_kernel_config_hash()
    cfg = codec.kernel_config()
    torch.manual_seed(0)
    other = models.JointCheckerboardHierarchicalPriors(12, 24)
    apply_weight_recipe(other, 3)
    other = other.to(dev).eval()
    other.update(force=True)
    x = _images(1, 64, 128).to(dev)
    before = other.compress(x)
    item = p.compress(x)
    p.decompress(item["strings"], item["shape"])
    after = other.compress(x)
    assert before["strings"] == after["strings"]
    assert item["kernel_config"] == cfg == codec.kernel_config() == before["kernel_config"]
    assert lib.load().clc_kernel_config_tag() == tag and lib.load().clc_kernel_config_hash() == hsh


@pytest.mark.parametrize("B,h,w", [(2, 64, 64), (1, 64, 128)])
def test_consistency_against_float64(dev, pair, B, h, w):
    o, p = pair
    o.eval()
    p.eval()
    groups, starts = SMALL["groups"], p.starts
    x = _images(B, h, w).to(dev)
    y, params, _, _ = p._code_inputs(x)
    syms, idxs, y_hat = p._scctx_encode(y, params)
    sym, idx = torch.cat(syms, 2), torch.cat(idxs, 2)
    _, _, H, W = y.shape
    # the GPU's (scales | means) of every element from the finished y_hat: per group the chain on the full raster list with the contexts of
    # y_hat (at the anchors the spatial context is 0 either way)
    pix = torch.tensor([(hh, ww) for hh in range(H) for ww in range(W)], dtype=torch.int32).to(dev)
    ws = p._scctx_workspace(B * H * W, dev)
    filt = p._scctx_filters()
    pc = params.contiguous(memory_format=CL)
    sc_gpu, mu_gpu = [], []
    with torch.no_grad():
        for k, (s, c) in enumerate(zip(starts, groups)):
            sp = p.spatial_context[k](y_hat[:, s:s + c])
            p._scctx_chain(pix, B, H, W, pc, sp, p._channel_ctx(k, y_hat), ws, filt[k])
            gp = ws["gp"][:, :2 * c].reshape(B, H * W, 2 * c)
            assert torch.equal(_rows(y_hat[:, s:s + c]), syms[k].float() + gp[..., c:]), "y_hat is sym + mean of the same chain"
            sc_gpu.append(gp[..., :c].double().cpu())
            mu_gpu.append(gp[..., c:].double().cpu())
    sc_gpu, mu_gpu = torch.cat(sc_gpu, 2), torch.cat(mu_gpu, 2)

    y64, p64, yh64 = y.double().cpu(), params.double().cpu(), y_hat.double().cpu()
    with torch.no_grad():
        sc64, mu64 = (_rows(t) for t in o.teacher_forced(yh64, p64))
    for name, got, ref in (("scales", sc_gpu, sc64), ("means", mu_gpu, mu64)):
        err = (got - ref).abs().max().item() / ref.abs().max().item()
        print(f"{H}x{W} {name}: GPU against float64 {err:.2e} of the largest magnitude {ref.abs().max().item():.3f}")
        assert err <= 2e-5, (name, err)
    assert sc64.max().item() > 1.0 and mu64.abs().max().item() > 1.0   # the predictions are informative, not clamped

    d = _rows(y64) - mu64
    frac = d - torch.floor(d)
    safe = (frac - 0.5).abs() > 1e-4
    excluded = 1.0 - safe.double().mean().item()
    print(f"{H}x{W} symbols: {100 * excluded:.3f} % excluded")
    assert excluded <= 0.01
    assert torch.equal(sym.cpu()[safe], torch.round(d).int()[safe])

    table = o.gaussian_conditional.scale_table.double()
    safe = ((sc64.unsqueeze(-1) - table).abs() > 1e-4 * table).all(-1)
    excluded = 1.0 - safe.double().mean().item()
    print(f"{H}x{W} indexes: {100 * excluded:.3f} % excluded")
    assert excluded <= 0.01
    assert torch.equal(idx.cpu()[safe], _rows(o.gaussian_conditional.build_indexes(sc64.reshape(B, H, W, M_).permute(0, 3, 1, 2)))[safe].int())
