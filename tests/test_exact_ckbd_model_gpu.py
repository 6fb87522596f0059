"""Build-independent streams for mbt2018-checkerboard: ``integer_context=True`` and ``exact=True``.  N = 32, M = 192, seeded
recipe weights rescaled as tests/test_ckbd_model_gpu.py does, ``integerize`` on two seeded 128x192 images; coded: a 64x64 image (a 4x4
latent) and a batch of two 128x192 images.  Every comparison is bit for bit: integer sums have no tolerance.  The
bytes-against-estimate figure is recorded only — tests/test_hyperprior_gpu.py gates no such bound."""
import numpy as np
import pytest
import torch

import intctx_ref as X
import intnet_ref as R

pytestmark = pytest.mark.gpu

N_, M_ = 32, 192


def _build(dev, **kw):
    from clc_amd import models
    from clc_amd.recipe import apply_weight_recipe

    base = models.JointCheckerboardHierarchicalPriors(N_, M_)   # (the weight recipe knows the plain model's parameters)
    apply_weight_recipe(base, 3)
    with torch.no_grad():
        base.g_a[6].weight.mul_(20.0)   # a latent with a few quantisation bins of spread
        base.h_s[4].weight.mul_(4.0)
        base.h_s[4].bias.add_(0.6)
        base.entropy_parameters[4].weight.mul_(8.0)   # predicted scales (and means) of order one
        base.entropy_parameters[4].bias[:M_].add_(0.6)
    m = models.JointCheckerboardHierarchicalPriors(N_, M_, **kw)
    m.load_state_dict(base.state_dict(), strict=False)   # the integer buffers stay zero
    m = m.to(dev).eval()
    m.update(force=True)
    return m


def _images(B, h, w, seed):
    from clc_amd.recipe import synthetic_image

    return synthetic_image(B, h, w, seed, smooth=True)


def _encoder_side(m, x):
    """what compress(x, exact=True) codes: symbols, indexes, y_hat, the (scales | means) rows of both passes as a map, psi, z"""
    with torch.no_grad():
        y, psi, z_strings, z_size = m._exact_inputs(x)
        B, M, H, W = y.shape
        gp_map = torch.full((B, H, W, 2 * M), float("nan"), device=y.device)
        launches = []

        def passes(params, y_hat):
            for cnt, px, gp in m._ckbd_passes(params, y_hat):
                gp_map[:, px[:, 0].long(), px[:, 1].long()] = gp[:B * cnt].view(B, cnt, 2 * M)
                launches.append(cnt)
                yield cnt, px, gp

        sym, idx, y_hat = m._encode_passes("test", y, psi, passes)
    return {"sym": sym.cpu().numpy(), "idx": idx.cpu().numpy(), "y_hat": y_hat, "gp": gp_map.cpu().numpy(), "psi": psi.permute(0, 2, 3, 1).cpu().numpy(),
            "z_strings": z_strings, "passes": launches}


@pytest.fixture(scope="module")
def coded(dev):
    m = _build(dev, integer_context=True)
    assert not m.ctx_int.ready
    h = m.integerize(_images(2, 128, 192, 11).to(dev))
    assert h == m.spec_hash() and m.ctx_int.ready and m.h_s_int.ready
    xs = {"small": _images(1, 64, 64, 21).to(dev), "batch": _images(2, 128, 192, 22).to(dev)}
    items = {k: m.compress(x, exact=True) for k, x in xs.items()}
    lanes = {k: m.compress(x, lanes=4, exact=True) for k, x in xs.items()}
    enc = {k: _encoder_side(m, x) for k, x in xs.items()}
    return m, xs, items, lanes, enc


def _net_of(m):
    """the integer entropy model as tests/intctx_ref.py takes it, from the state_dict alone"""
    return X.net_of_state_dict({k: v.cpu().numpy() for k, v in m.state_dict().items() if k.startswith(("h_s_int.", "ctx_int."))})


@pytest.mark.parametrize("which", ["small", "batch"])
def test_round_trip_on_both_streams(coded, which):
    m, xs, items, lanes, enc = coded
    item, litem, e = items[which], lanes[which], enc[which]
    assert item["exact"] == litem["exact"] == m.spec_hash() == X.spec_hash(_net_of(m))
    assert item["strings"][1] == litem["strings"][1] == e["z_strings"] and litem["lanes"] == 4 and "lanes" not in item
    assert tuple(item["shape"]) == ((1, 1) if which == "small" else (2, 3))
    assert e["passes"] == ([8, 8] if which == "small" else [48, 48]) and not np.isnan(e["gp"]).any()
    for exact in (True, item["exact"]):
        assert torch.equal(m._decode_y_hat(item["strings"], item["shape"], exact=exact), e["y_hat"])
    # the lanes stream: the device coder against the host coder, both the encoder's y_hat
    assert torch.equal(m._decode_y_hat(litem["strings"], litem["shape"], lanes=4, exact=litem["exact"]), e["y_hat"])
    assert torch.equal(m._decode_y_hat(litem["strings"], litem["shape"], lanes=4, exact=True, device_coder=False), e["y_hat"])
    with torch.no_grad():
        want = m._synthesis(e["y_hat"]).clamp_(0, 1)
    assert torch.equal(m.decompress(item["strings"], item["shape"], exact=item["exact"])["x_hat"], want)
    assert torch.equal(m.decompress(litem["strings"], litem["shape"], lanes=4, exact=litem["exact"])["x_hat"], want)
    # the float parameters are another entropy model: the default stream differs, and each decodes under its own
    plain = m.compress(xs[which])
    assert "exact" not in plain and plain["strings"][1] == item["strings"][1] and plain["strings"][0] != item["strings"][0]
    assert torch.equal(m.decompress(plain["strings"], plain["shape"])["x_hat"], m.decompress(plain["strings"], plain["shape"], exact=None)["x_hat"])


@pytest.mark.parametrize("which", ["small", "batch"])
def test_decodes_on_the_cpu_from_the_strings_alone(coded, which):
    """THE CLAIM: no float kernel of the GPU takes part — host rANS for z, the numpy h_s, per pass the numpy chain, a numpy scale index,
    an incremental host rANS decoder, y_hat = symbol + mean, the numpy quantiser and tap layer; symbols, indexes and y_hat are the
    encoder's on every element"""
    from clc_amd import ans

    m, xs, items, lanes, enc = coded
    item, e = items[which], enc[which]
    zh, zw = (int(v) for v in item["shape"])
    eb, gc = m.entropy_bottleneck, m.gaussian_conditional
    cdf, ln, off = eb.host_tables()
    zidx = np.ascontiguousarray(np.broadcast_to(np.arange(N_, dtype=np.int32).reshape(N_, 1, 1), (N_, zh, zw))).reshape(-1)
    med = eb.quantiles[:, 0, 1].detach().cpu().numpy().astype(np.float32).reshape(1, N_, 1, 1)
    z_hat = np.stack([ans.decode(s, zidx, cdf, ln, off).reshape(N_, zh, zw) for s in item["strings"][1]]).astype(np.float32) + med
    net = _net_of(m)
    psi = X.psi_map(net, z_hat)
    assert np.array_equal(psi, e["psi"])                                       # the kernels' bits are the reference's
    B, H, W = psi.shape[:3]
    table = gc.scale_table.cpu().numpy()
    ycdf, yln, yoff = gc.host_tables()
    decoders = []
    for s in item["strings"][0]:
        d = ans.RansDecoder()
        d.set_stream(s)
        decoders.append(d)
    y_hat = np.zeros((B, M_, H, W), np.float32)
    sym_map, idx_map = np.zeros((B, H * W, M_), np.int32), np.zeros((B, H * W, M_), np.int32)
    kinds = []
    for pixels in X.passes(H, W):
        anchor = X.is_anchor(pixels)
        kinds.append(anchor)
        gp = X.chain(net, pixels, psi, None if anchor else X.quantize_y(y_hat, net["f_y"]))["gp"]   # [B, P, 2M]
        scales, means = gp[..., :M_], gp[..., M_:]
        idx = R.scale_indexes(scales, table)
        for b in range(B):
            sym = np.asarray(decoders[b].decode_stream(np.ascontiguousarray(idx[b]).reshape(-1), ycdf, yln, yoff), dtype=np.int32).reshape(len(pixels), M_)
            for p, (h, w) in enumerate(pixels):
                y_hat[b, :, h, w] = sym[p].astype(np.float32) + means[b, p]   # one rounded add
                sym_map[b, h * W + w], idx_map[b, h * W + w] = sym[p], idx[b, p]
                assert np.array_equal(gp[b, p], e["gp"][b, h, w])
    assert kinds == [True, False]
    assert np.array_equal(sym_map, e["sym"]) and np.array_equal(idx_map, e["idx"])
    assert np.array_equal(y_hat, e["y_hat"].cpu().numpy())
    assert len(np.unique(sym_map)) > 3 and len(np.unique(idx_map)) > 3         # (a latent of a few bins, scales that vary)


def test_survives_a_kernel_state_change(coded):
    import clc_amd
    from clc_amd import codec

    m, xs, items, lanes, enc = coded
    x = xs["batch"][:1]
    item = m.compress(x, exact=True)
    assert item["strings"][0][0] == items["batch"]["strings"][0][0]          # an image's exact stream does not depend on the batch around it
    assert m.compress(xs["batch"][1:], lanes=4, exact=True)["strings"][0][0] == lanes["batch"]["strings"][0][1]
    blob4 = codec.pack_item(item, image_hw=(128, 192))
    blob1 = codec.pack_item(m.compress(x), image_hw=(128, 192))
    assert blob4[4] == 4 and blob1[4] in (1, 2)
    old = clc_amd.set_precision("bf16")
    try:
        got = codec.unpack_item(blob4, strict=True)
        assert got["meta"]["exact_hash"] == item["exact"] and got["meta"]["same_kernel_config"] is True
        y_hat = m._decode_y_hat(got["strings"], got["shape"], exact=got["exact"])
        assert torch.equal(y_hat, enc["batch"]["y_hat"][:1])
        with pytest.raises(codec.KernelConfigMismatch):
            codec.unpack(blob1, strict=True)
    finally:
        clc_amd.set_precision(old)
    assert clc_amd.get_precision() == old


def test_one_by_one_latent_takes_the_single_non_anchor_pass(coded, dev):
    """the model's smallest image gives a 4x4 latent, so the 1x1 latent is driven at the pass level: one non-anchor pass, four
    launches' worth of chain, the context row = the requantised bias (every tap is off the map)"""
    m, xs, items, lanes, enc = coded
    net = _net_of(m)
    rng = np.random.default_rng(3)
    psi = rng.integers(-128, 128, (2, 1, 1, 2 * M_)).astype(np.int8)
    y = torch.from_numpy(rng.normal(0, 3, (2, M_, 1, 1)).astype(np.float32)).to(dev)
    params = torch.from_numpy(psi).to(dev).permute(0, 3, 1, 2)
    got = []
    with torch.no_grad():
        def passes(p, y_hat):
            for cnt, px, gp in m._ckbd_passes(p, y_hat):
                got.append((cnt, px.cpu().numpy().tolist(), gp[:2 * cnt].cpu().numpy().copy()))
                yield cnt, px, gp

        sym, idx, y_hat = m._encode_passes("test", y, params, passes)
    assert len(got) == 1 and got[0][0] == 1 and got[0][1] == [[0, 0]]
    ref = X.chain(net, [(0, 0)], psi, X.quantize_y(np.zeros((2, M_, 1, 1), np.float32), net["f_y"]))
    bias_row = X.rows_int8(np.zeros((1, 12 * M_), np.int64), net["ctx"][0])
    assert np.array_equal(ref["ctx"][0], bias_row) and np.array_equal(ref["ctx"][1], bias_row)
    assert np.array_equal(got[0][2], ref["gp"].reshape(2, 2 * M_))
    scales, means = ref["gp"][..., :M_], ref["gp"][..., M_:]
    assert np.array_equal(idx.cpu().numpy(), R.scale_indexes(scales, m.gaussian_conditional.scale_table.cpu().numpy()))
    s = np.rint(y.cpu().numpy().reshape(2, 1, M_) - means)
    assert np.array_equal(sym.cpu().numpy(), s.astype(np.int32))
    assert np.array_equal(y_hat.cpu().numpy().reshape(2, 1, M_), (s + means).astype(np.float32))


def test_eval_forward_and_the_rate_actually_written(coded):
    m, xs, items, lanes, enc = coded
    x, e = xs["batch"], enc["batch"]
    with torch.no_grad():
        out = m(x, exact=True)
        plain = m(x)
        gp = torch.from_numpy(e["gp"]).to(x.device).permute(0, 3, 1, 2)
        y = m._analysis(m._prep(x))
        _, lik = m.gaussian_conditional(y, gp[:, :M_], means=gp[:, M_:])
        assert torch.equal(out["likelihoods"]["y"], lik) and torch.equal(out["x_hat"], m._synthesis(e["y_hat"]))
    assert torch.equal(out["likelihoods"]["z"], plain["likelihoods"]["z"]) and not torch.equal(out["likelihoods"]["y"], plain["likelihoods"]["y"])
    est = float(-torch.log2(out["likelihoods"]["y"]).sum()) / 8.0
    actual = sum(len(s) for s in items["batch"]["strings"][0])
    actual_lanes = sum(len(s) for s in lanes["batch"]["strings"][0])
    est_plain = float(-torch.log2(plain["likelihoods"]["y"]).sum()) / 8.0
    print(f"mbt2018-checkerboard exact: y bytes {actual} (lanes=4: {actual_lanes}) / estimate {est:.1f} = {actual / est:.4f} (recorded, not gated); "
          f"estimate of the float eval forward {est_plain:.1f}")


def test_state_dict_round_trip_and_the_plain_model_is_unchanged(coded, dev):
    m, xs, items, lanes, enc = coded
    from clc_amd import models

    fresh = models.JointCheckerboardHierarchicalPriors(N_, M_, integer_context=True)
    fresh.load_state_dict(m.state_dict())
    fresh = fresh.to(dev).eval()
    assert fresh.spec_hash() == m.spec_hash()
    again = fresh.compress(xs["batch"], exact=True)
    assert again["strings"] == items["batch"]["strings"] and again["exact"] == items["batch"]["exact"]
    # without the flag: no new module, no new key, and the default bytes of the same weights are the flagged model's default bytes
    plain = _build(dev)
    assert not hasattr(plain, "ctx_int") and not hasattr(plain, "h_s_int")
    assert set(m.state_dict()) - set(plain.state_dict()) == {k for k in m.state_dict() if k.startswith(("h_s_int.", "ctx_int."))}
    for kw in ({}, {"lanes": 4}):
        assert plain.compress(xs["batch"], **kw)["strings"] == m.compress(xs["batch"], **kw)["strings"]


def test_refusals_on_the_device(coded, dev):
    m, xs, items, lanes, enc = coded
    item = items["small"]
    plain = _build(dev)
    with pytest.raises(ValueError, match="integer_context=True"):
        plain.compress(xs["small"], exact=True)
    with pytest.raises(ValueError, match="integer_context=True"):
        plain.decompress(item["strings"], item["shape"], exact=item["exact"])
    h = item["exact"]
    with pytest.raises(ValueError, match=f"0x{h ^ 0x10:08x}.*0x{h:08x}"):
        m.decompress(item["strings"], item["shape"], exact=h ^ 0x10)
    with pytest.raises(ValueError, match="lanes"):   # a lanes string is not taken for a one-stream string
        m.decompress(lanes["small"]["strings"], item["shape"], exact=h)
