"""The hyperprior baselines without a GPU: construction, the CompressAI state_dict surface against the plain-torch restatement
(tests/hyperprior_ref.py), the compat names, and the two identities the 5x5 transposed kernel rests on (tests/conv5_ref.py)."""
import sys

import pytest
import torch

import conv5_ref
import hyperprior_ref


def _product(kind, N=12, M=24):
    from clc_amd import models

    return {"scale": models.ScaleHyperprior, "mean_scale": models.MeanScaleHyperprior}[kind](N, M)


@pytest.mark.parametrize("kind", ["scale", "mean_scale"])
def test_state_dict_matches_the_restatement(kind):
    p, r = _product(kind), hyperprior_ref.MODELS[kind](12, 24)
    sp, sr = p.state_dict(), r.state_dict()
    assert list(sp.keys()) == list(sr.keys())
    for k in sp:
        assert tuple(sp[k].shape) == tuple(sr[k].shape), k
        assert sp[k].dtype == sr[k].dtype, k
    # the 5x5 layers are where they should be, with torch's parameter shapes
    assert tuple(sp["g_a.0.weight"].shape) == (12, 3, 5, 5) and tuple(sp["g_s.6.weight"].shape) == (12, 3, 5, 5)
    assert tuple(sp["h_s.0.weight"].shape) == ((12, 12, 5, 5) if kind == "scale" else (12, 24, 5, 5))
    assert tuple(sp["h_a.0.weight"].shape) == (12, 24, 3, 3)


@pytest.mark.parametrize("kind", ["scale", "mean_scale"])
def test_load_state_dict_is_strict_clean_both_ways(kind):
    p, r = _product(kind), hyperprior_ref.MODELS[kind](12, 24)
    res = p.load_state_dict(r.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in r.state_dict().items():
        assert torch.equal(p.state_dict()[k], v), k
    p2 = _product(kind)
    res = r.load_state_dict(p2.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    # ... and with the CDF tables present (a checkpoint saved after update()): the empty buffers are resized
    r.update(force=True)
    res = _product(kind).load_state_dict(r.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys


def test_constructor_and_layer_geometry_errors():
    from clc_amd import layers, models

    with pytest.raises(ValueError, match="multiples of 4"):
        models.ScaleHyperprior(10, 24)
    with pytest.raises(ValueError, match="multiples of 4"):
        models.MeanScaleHyperprior(12, 20)   # M * 3 / 2 = 30
    with pytest.raises(ValueError, match="kernel_size"):
        layers.Conv2d(8, 8, 7)
    with pytest.raises(ValueError, match="output_padding"):
        layers.ConvTranspose2d(8, 8, 5, stride=2, padding=2, output_padding=0)
    assert isinstance(layers.conv(8, 8), layers.Conv2d) and layers.conv(8, 8).kernel_size == (5, 5) and layers.conv(8, 8).stride == (2, 2)
    assert isinstance(layers.deconv(8, 8), layers.ConvTranspose2d)
    assert isinstance(layers.deconv(8, 8, kernel_size=3, stride=1), layers.Conv2d)
    assert isinstance(layers.conv(8, 8, kernel_size=3, stride=1), layers.Conv2d)


def test_compat_names():
    from clc_amd import compat, models

    saved = {k: v for k, v in sys.modules.items() if k == "models" or k.split(".")[0] in ("compressai", "timm", "pytorch_msssim")}
    try:
        compat.install(force=True)
        import compressai.models as cm
        import compressai.zoo as cz

        assert cm.ScaleHyperprior is models.ScaleHyperprior and cm.MeanScaleHyperprior is models.MeanScaleHyperprior
        assert cz.models["bmshj2018-hyperprior"] is models.ScaleHyperprior and cz.models["mbt2018-mean"] is models.MeanScaleHyperprior
        assert cz.models["clc"] is models.CLC and cz.models["tcm"] is models.TCM
    finally:
        for k in [k for k in sys.modules if k == "models" or k.split(".")[0] in ("compressai", "timm", "pytorch_msssim")]:
            del sys.modules[k]
        sys.modules.update(saved)


def test_deconv_is_the_data_gradient_and_tap_table():
    assert conv5_ref.deconv_identity_gap() == 0.0
    assert conv5_ref.tap_table() == {(0, 0): 9, (0, 1): 6, (1, 0): 6, (1, 1): 4}
    assert conv5_ref.live_taps(0) == [0, 2, 4] and conv5_ref.live_taps(1) == [1, 3]
