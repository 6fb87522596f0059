"""Build-independent streams: ScaleHyperprior / MeanScaleHyperprior with ``integer_hyper=True`` and ``exact=True``.
N = 32, M = 64, seeded weights, ``integerize`` on two seeded 128x192 images; coded: a 64x64 image (a 1x1 z) and a batch of two 128x192
images.  Every comparison is bit for bit: integer sums have no tolerance.  The bytes-against-estimate figure is recorded only —
tests/test_hyperprior_gpu.py gates no such bound."""
import numpy as np
import pytest
import torch

import hyperprior_ref
import intnet_ref as R

pytestmark = pytest.mark.gpu

N_, M_ = 32, 64
KINDS = ["scale", "mean_scale"]


def _cls(kind):
    from clc_amd import models

    return {"scale": models.ScaleHyperprior, "mean_scale": models.MeanScaleHyperprior}[kind]


def _build(kind, dev, **kw):
    from clc_amd.recipe import apply_weight_recipe

    base = _cls(kind)(N_, M_)   # (the weight recipe knows the plain model's parameters)
    apply_weight_recipe(base, 3)
    with torch.no_grad():
        base.g_a[6].weight.mul_(20.0)   # a latent with a few quantisation bins of spread
        base.h_s[4].weight.mul_(4.0)    # predicted scales (and means) of order one
        base.h_s[4].bias.add_(0.6)
    m = _cls(kind)(N_, M_, integer_hyper=True, **kw)
    m.load_state_dict(base.state_dict(), strict=False)   # the integer buffers stay zero, a step table keeps its default ladder
    m = m.to(dev).eval()
    m.update(force=True)
    return m


def _images(B, h, w, seed):
    from clc_amd.recipe import synthetic_image

    return synthetic_image(B, h, w, seed, smooth=True)


def _encoder_side(m, x, q=None):
    """what compress(x, exact=True) codes: (symbols, indexes, y_hat, y, scales, means, z strings) from the integer net's parameters"""
    with torch.no_grad():
        y = m._analysis(m._prep(x))
        z = m._hyper_analysis(y)
        z_strings = m.entropy_bottleneck.compress(z)
        z_hat = m.entropy_bottleneck.decompress(z_strings, z.size()[-2:])
        scales, means = m.h_s_int(z_hat)
        mu = means if means is not None else torch.zeros_like(y, memory_format=torch.channels_last)
        step = m._step(q, "test")
        gc = m.gaussian_conditional
        sym, idx, y_hat = gc.quantize_and_index(y, mu, scales) if step is None else gc.quantize_and_index(y, mu, scales, step=step)
    return {"sym": sym, "idx": idx, "y_hat": y_hat, "y": y, "scales": scales, "means": means, "z_strings": z_strings, "z_hat": z_hat}


@pytest.fixture(scope="module", params=KINDS)
def coded(request, dev):
    m = _build(request.param, dev)
    h = m.integerize(_images(2, 128, 192, 11).to(dev))
    assert h == m.h_s_int.spec_hash() and m.h_s_int.ready
    xs = {"1x1": _images(1, 64, 64, 21).to(dev), "batch": _images(2, 128, 192, 22).to(dev)}
    items = {k: m.compress(x, exact=True) for k, x in xs.items()}
    enc = {k: _encoder_side(m, x) for k, x in xs.items()}
    return request.param, m, xs, items, enc


def _net_of(m):
    """the integer net as tests/intnet_ref.py takes it, from the state_dict alone"""
    sd = {k[len("h_s_int."):]: v.cpu().numpy() for k, v in m.state_dict().items() if k.startswith("h_s_int.")}
    layers = [{k: sd[f"{k}{i}"] for k in ("w", "bias", "mult_pos", "mult_neg", "shift")} for i in range(3)]
    return {"f0": int(sd["fixed_point"][0]), "f_out": int(sd["fixed_point"][1]), "layers": layers}


@pytest.mark.parametrize("which", ["1x1", "batch"])
def test_round_trip(coded, which):
    kind, m, xs, items, enc = coded
    item, e = items[which], enc[which]
    assert item["exact"] == m.h_s_int.spec_hash() and item["strings"][1] == e["z_strings"]
    assert tuple(item["shape"]) == ((1, 1) if which == "1x1" else (2, 3))
    for exact in (True, item["exact"]):
        y_hat = m._decode_y_hat(item["strings"], item["shape"], exact=exact)
        assert torch.equal(y_hat, e["y_hat"])
    x_hat = m.decompress(item["strings"], item["shape"], exact=item["exact"])["x_hat"]
    with torch.no_grad():
        assert torch.equal(x_hat, m._synthesis(e["y_hat"]).clamp_(0, 1))
    # the float parameters are another entropy model: the default stream differs, and each decodes under its own
    plain = m.compress(xs[which])
    assert "exact" not in plain and plain["strings"][1] == item["strings"][1]
    if which == "batch":   # (12 288 symbols: the two parameter sets do not index alike)
        assert plain["strings"][0] != item["strings"][0]


@pytest.mark.parametrize("which", ["1x1", "batch"])
def test_decodes_on_the_cpu_from_the_strings_alone(coded, which):
    """THE CLAIM: no float kernel of the GPU takes part — the host rANS decoder, the numpy integer net on the host-decoded z symbols,
    a numpy restatement of the scale index; the decoded symbols are the encoder's on every element"""
    from clc_amd import ans

    kind, m, xs, items, enc = coded
    item, e = items[which], enc[which]
    zh, zw = (int(v) for v in item["shape"])
    eb, gc = m.entropy_bottleneck, m.gaussian_conditional
    cdf, ln, off = eb.host_tables()
    zidx = np.ascontiguousarray(np.broadcast_to(np.arange(N_, dtype=np.int32).reshape(N_, 1, 1), (N_, zh, zw))).reshape(-1)
    med = eb.quantiles[:, 0, 1].detach().cpu().numpy().astype(np.float32).reshape(1, N_, 1, 1)
    z_sym = np.stack([ans.decode(s, zidx, cdf, ln, off).reshape(N_, zh, zw) for s in item["strings"][1]])
    z_hat = z_sym.astype(np.float32) + med                                   # one rounded add
    assert np.array_equal(z_hat, e["z_hat"].cpu().numpy())
    params = R.forward(_net_of(m), z_hat)
    scales, means = (params[:, :M_], params[:, M_:]) if kind == "mean_scale" else (params, None)
    assert np.array_equal(scales, e["scales"].cpu().numpy())                  # the kernels' bits are the reference's
    if means is not None:
        assert np.array_equal(means, e["means"].cpu().numpy())
    idx = R.scale_indexes(scales, gc.scale_table.cpu().numpy())
    assert np.array_equal(idx, e["idx"].cpu().numpy())
    ycdf, yln, yoff = gc.host_tables()
    sym = np.stack([ans.decode(s, np.ascontiguousarray(idx[i]).reshape(-1), ycdf, yln, yoff).reshape(idx.shape[1:]) for i, s in enumerate(item["strings"][0])])
    assert np.array_equal(sym, e["sym"].cpu().numpy())
    y_hat = sym.astype(np.float32) + (means if means is not None else np.float32(0))
    assert np.array_equal(y_hat, e["y_hat"].cpu().numpy())


def test_survives_a_kernel_state_change(coded):
    import clc_amd
    from clc_amd import codec

    kind, m, xs, items, enc = coded
    x = xs["batch"][:1]
    item = m.compress(x, exact=True)
    assert item["strings"][0][0] == items["batch"]["strings"][0][0]          # an image's stream does not depend on the batch around it
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


def test_eval_forward(coded):
    kind, m, xs, items, enc = coded
    x, e = xs["batch"], enc["batch"]
    with torch.no_grad():
        out = m(x, exact=True)
        mu = e["means"] if e["means"] is not None else None
        y_hat, lik = m.gaussian_conditional(e["y"], e["scales"], means=mu)
        plain = m(x)
    assert torch.equal(out["likelihoods"]["y"], lik) and torch.equal(out["x_hat"], m._synthesis(y_hat))
    assert torch.equal(out["likelihoods"]["z"], plain["likelihoods"]["z"]) and not torch.equal(out["likelihoods"]["y"], plain["likelihoods"]["y"])
    est = float(-torch.log2(out["likelihoods"]["y"]).sum()) / 8.0
    actual = sum(len(s) for s in items["batch"]["strings"][0])
    est_plain = float(-torch.log2(plain["likelihoods"]["y"]).sum()) / 8.0
    print(f"{kind}: y bytes {actual} / estimate {est:.1f} = {actual / est:.4f} (recorded, not gated); estimate with float parameters {est_plain:.1f}")


def test_composes_with_the_quantisation_step(dev):
    m = _build("mean_scale", dev, rate_levels=5)
    m.integerize(_images(2, 128, 192, 11).to(dev))
    x = _images(1, 128, 192, 23).to(dev)
    item = m.compress(x, q=2.5, exact=True)
    assert item["q"] == 2.5 and item["exact"] == m.h_s_int.spec_hash()
    e = _encoder_side(m, x, q=2.5)
    y_hat = m._decode_y_hat(item["strings"], item["shape"], q=item["q"], exact=item["exact"])
    assert torch.equal(y_hat, e["y_hat"])
    assert m.compress(x, q=0.5, exact=True)["strings"][0] != item["strings"][0]
    idx = R.scale_indexes(e["scales"].cpu().numpy(), m.gaussian_conditional.scale_table.cpu().numpy(), step=m._step(2.5, "test").detach().cpu().numpy())
    assert np.array_equal(idx, e["idx"].cpu().numpy())


def test_state_dict_round_trip_and_keys(coded, dev):
    kind, m, xs, items, enc = coded
    fresh = _cls(kind)(N_, M_, integer_hyper=True)
    assert not fresh.h_s_int.ready
    fresh.load_state_dict(m.state_dict())
    fresh = fresh.to(dev).eval()
    assert fresh.h_s_int.spec_hash() == m.h_s_int.spec_hash()
    again = fresh.compress(xs["batch"], exact=True)
    assert again["strings"] == items["batch"]["strings"] and again["exact"] == items["batch"]["exact"]
    # without the flag: no new module, the keys of the model as it was
    plain = _cls(kind)(N_, M_)
    assert not hasattr(plain, "h_s_int")
    assert set(plain.state_dict()) == set(hyperprior_ref.MODELS[kind](N_, M_).state_dict())
    assert set(m.state_dict()) - set(plain.state_dict()) == {k for k in m.state_dict() if k.startswith("h_s_int.")}


def test_refusals_by_name(coded, dev):
    from clc_amd import models
    from clc_amd.models.hyperprior import JointAutoregressiveHierarchicalPriors

    kind, m, xs, items, enc = coded
    item = items["1x1"]
    plain = _cls(kind)(N_, M_).to(dev).eval()
    plain.update(force=True)
    with pytest.raises(ValueError, match="integer_hyper=True"):
        plain.compress(xs["1x1"], exact=True)
    with pytest.raises(ValueError, match="integer_hyper=True"):
        plain.decompress(item["strings"], item["shape"], exact=item["exact"])
    h = item["exact"]
    with pytest.raises(ValueError, match=f"0x{h ^ 0x10:08x}.*0x{h:08x}"):
        m.decompress(item["strings"], item["shape"], exact=h ^ 0x10)
    m.train()
    try:
        with pytest.raises(ValueError, match="training mode"):
            m(xs["1x1"], exact=True)
    finally:
        m.eval()
    with pytest.raises(ValueError, match="multiple of 32"):
        _cls(kind)(48, 64, integer_hyper=True)
    with pytest.raises(ValueError, match="no integer hyper-synthesis net"):
        JointAutoregressiveHierarchicalPriors(integer_hyper=True)
    with pytest.raises(ValueError, match="no integer hyper-synthesis net"):
        models.CLC(integer_hyper=True)
    with pytest.raises(ValueError, match="z_hat must be"):
        m.h_s_int(torch.zeros(1, 64, 1, 1, device=dev))
