"""ssf2020 (clc_amd/models/video.py, clc_amd/scale_space.py) without a GPU: the CompressAI state_dict surface against the plain-torch
restatement (tests/ssf_ref.py), the compat and zoo names, the refusals, the loud failure on CPU tensors, and two identities of the
restatement's own operators in float64 that pin the definition the kernels are held to."""
import sys

import pytest
import torch

import ssf_ref

WIDTHS = [(128, 192), (12, 24)]


def _product(mid, planes, **kw):
    from clc_amd import models

    return models.ScaleSpaceFlow(mid_planes=mid, planes=planes, **kw)


@pytest.mark.parametrize("mid,planes", WIDTHS)
def test_state_dict_matches_the_restatement(mid, planes):
    p, r = _product(mid, planes), ssf_ref.ScaleSpaceFlow(mid_planes=mid, planes=planes)
    sp, sr = p.state_dict(), r.state_dict()
    assert list(sp.keys()) == list(sr.keys())
    for k in sp:
        assert tuple(sp[k].shape) == tuple(sr[k].shape), k
        assert sp[k].dtype == sr[k].dtype, k
    assert "motion_hyperprior.hyper_decoder_scale.deconv2.weight" in sp
    assert tuple(sp["res_decoder.0.weight"].shape) == (2 * planes, mid, 5, 5)      # ConvTranspose2d: [in, out, 5, 5]
    assert tuple(sp["motion_encoder.0.weight"].shape) == (mid, 6, 5, 5)
    assert tuple(sp["res_encoder.0.weight"].shape) == (mid, 3, 5, 5) and tuple(sp["motion_decoder.6.weight"].shape) == (mid, 3, 5, 5)
    assert tuple(sp["img_hyperprior.hyper_encoder.4.weight"].shape) == (planes, planes, 5, 5)
    tops = []
    for k in sp:
        if k.split(".")[0] not in tops:
            tops.append(k.split(".")[0])
    assert tops == ["img_encoder", "img_decoder", "img_hyperprior", "res_encoder", "res_decoder", "res_hyperprior", "motion_encoder",
                    "motion_decoder", "motion_hyperprior"]


@pytest.mark.parametrize("mid,planes", WIDTHS)
def test_load_state_dict_is_strict_clean_both_ways(mid, planes):
    p, r = _product(mid, planes), ssf_ref.ScaleSpaceFlow(mid_planes=mid, planes=planes)
    res = p.load_state_dict(r.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in r.state_dict().items():
        assert torch.equal(p.state_dict()[k], v), k
    res = r.load_state_dict(_product(mid, planes).state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    if planes > 24:
        return   # (the table build below is the slow part; the small width covers it)
    # ... and with the CDF tables present (a checkpoint saved after update()): the empty buffers of all three hyperpriors are resized
    r.update(force=True)
    q = _product(mid, planes)
    res = q.load_state_dict(r.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for h in ("img_hyperprior", "res_hyperprior", "motion_hyperprior"):
        assert getattr(q, h).gaussian_conditional._quantized_cdf.numel() > 0 and getattr(q, h).entropy_bottleneck._offset.numel() == planes


def test_constructor_keeps_compressai_arguments():
    m = _product(12, 24, num_levels=3, sigma0=2.0, scale_field_shift=0.5)
    assert (m.num_levels, m.sigma0, m.scale_field_shift) == (3, 2.0, 0.5)
    from clc_amd.entropy_models import EntropyBottleneck

    assert sum(isinstance(s, EntropyBottleneck) for s in m.modules()) == 3   # what aux_loss() and update() walk
    with pytest.raises(ValueError, match="multiples of 4"):
        _product(10, 24)


def test_compat_and_zoo_names():
    from clc_amd import compat, models

    saved = {k: v for k, v in sys.modules.items() if k == "models" or k.split(".")[0] in ("compressai", "timm", "pytorch_msssim")}
    try:
        compat.install(force=True)
        import compressai.models as cm
        import compressai.models.video as cmv
        import compressai.zoo as cz
        from compressai.models.video import ScaleSpaceFlow

        assert cm.ScaleSpaceFlow is models.ScaleSpaceFlow and cmv.ScaleSpaceFlow is models.ScaleSpaceFlow and ScaleSpaceFlow is models.ScaleSpaceFlow
        assert cm.video is cmv
        assert cz.video_models == {"ssf2020": models.ScaleSpaceFlow}
        assert sorted(cz.models) == sorted(["clc", "tcm", "bmshj2018-hyperprior", "mbt2018-mean", "mbt2018", "mbt2018-checkerboard", "elic2022",
                                            "cheng2020-anchor", "cheng2020-attn"])
    finally:
        for k in [k for k in sys.modules if k == "models" or k.split(".")[0] in ("compressai", "timm", "pytorch_msssim")]:
            del sys.modules[k]
        sys.modules.update(saved)


def test_refusals_by_name():
    from clc_amd import models
    from clc_amd.scale_space import scale_space_volume, scale_space_warp

    with pytest.raises(ValueError, match="num_levels"):
        models.ScaleSpaceFlow(num_levels=0, mid_planes=12, planes=24)
    with pytest.raises(ValueError, match="sigma0"):
        models.ScaleSpaceFlow(sigma0=0.0, mid_planes=12, planes=24)
    with pytest.raises(ValueError, match="sigma0"):
        models.ScaleSpaceFlow(sigma0=-1.5, mid_planes=12, planes=24)
    m = _product(12, 24)
    f = torch.zeros(1, 3, 128, 128)
    with pytest.raises(ValueError, match="fewer than one frame"):
        m([])
    with pytest.raises(ValueError, match="fewer than one frame"):
        m.compress([])
    with pytest.raises(ValueError, match="differing shapes"):
        m([f, torch.zeros(1, 3, 128, 256)])
    with pytest.raises(ValueError, match="multiples of 128"):
        m([torch.zeros(1, 3, 128, 192)])
    with pytest.raises(ValueError, match="multiples of 128"):
        m.compress([torch.zeros(1, 3, 64, 128)])
    # the operators
    with pytest.raises(ValueError, match="num_levels"):
        scale_space_volume(f, num_levels=0)
    with pytest.raises(ValueError, match="sigma0"):
        scale_space_volume(f, sigma0=0.0)
    with pytest.raises(ValueError, match="divisible"):
        scale_space_volume(torch.zeros(1, 3, 24, 16), num_levels=5)
    with pytest.raises(ValueError, match="flow"):
        scale_space_warp(torch.zeros(1, 3, 6, 16, 16), torch.zeros(1, 2, 16, 8), torch.zeros(1, 1, 16, 16))


def test_the_product_fails_loudly_without_a_gpu():
    from clc_amd.lib import ClcError
    from clc_amd.scale_space import scale_space_volume, scale_space_warp

    m = _product(12, 24)
    f = torch.zeros(1, 3, 128, 128)
    with pytest.raises(ClcError, match="GPU only"):
        m([f, f])
    with pytest.raises(ClcError, match="GPU only"):
        m.compress([f])
    with pytest.raises(ClcError, match="GPU only"):
        scale_space_volume(f)
    with pytest.raises(ClcError, match="GPU only"):
        scale_space_warp(torch.zeros(1, 3, 6, 16, 16), torch.zeros(1, 2, 16, 16), torch.zeros(1, 1, 16, 16))


def test_taps_are_the_restatements():
    from clc_amd.scale_space import gaussian_taps

    for s in (0.5, 1.5, 2.0, 3.3):
        g = ssf_ref.gaussian_kernel1d(s)
        t = torch.tensor(gaussian_taps(s), dtype=torch.float64)
        assert t.numel() == g.numel() and (t - g).abs().max().item() <= 1e-15
    assert len(gaussian_taps(1.5)) == 11


# ---- the restatement's own operators, float64: two identities that pin the definition ----
@pytest.mark.parametrize("shape,levels", [((1, 3, 4, 4), 1), ((2, 3, 8, 16), 3), ((1, 3, 16, 48), 5)])
def test_a_constant_frame_gives_a_constant_volume(shape, levels):
    x = torch.full(shape, 0.3725, dtype=torch.float64)
    v = ssf_ref.volume(x, 1.5, levels)
    assert tuple(v.shape) == (shape[0], 3, levels + 1, shape[2], shape[3])
    assert (v - 0.3725).abs().max().item() <= 1e-14


@pytest.mark.parametrize("shape,levels", [((2, 3, 8, 16), 3), ((1, 3, 16, 48), 5)])
def test_zero_flow_at_a_slice_coordinate_returns_the_slice(shape, levels):
    g = torch.Generator().manual_seed(11)
    x = torch.rand(shape, generator=g, dtype=torch.float64)
    v = ssf_ref.volume(x, 1.5, levels)
    N, _, H, W = shape
    D = levels + 1
    zero = torch.zeros(N, 2, H, W, dtype=torch.float64)
    for d in range(D):
        gz = torch.full((N, 1, H, W), (2 * d + 1) / D - 1, dtype=torch.float64)
        assert (ssf_ref.warp(v, zero, gz) - v[:, :, d]).abs().max().item() <= 1e-14, d
    # slice 0 is the frame itself, slice 1 its blur
    assert torch.equal(v[:, :, 0], x)
    assert (v[:, :, 1] - ssf_ref.blur(x, ssf_ref.gaussian_kernel1d(1.5))).abs().max().item() == 0.0
