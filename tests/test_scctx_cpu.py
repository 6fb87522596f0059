"""The space-channel context model (models.Elic2022, csrc/row_gemm.hip) without a GPU: the state_dict surface against the plain-torch
restatement (tests/scctx_ref.py) and strict loading both ways, the constructor's refusals, the compat and zoo names, the stream order,
clc_row_gemm's argument refusals (all of which return before any launch) — and the restatement against itself in float64 at
scctx_ref.SMALL (N = 8, M = 32, groups (4, 4, 8, 16)) with the weights and images of tests/test_scctx_model_gpu.py: its 2 K-pass loop
against its teacher-forced pass on the loop's own y_hat (the gap is exactly 0.0 here; held to 1e-15), informative predictions, and the
exclusion shares of the GPU consistency test measured on the reference alone.  Measured on the CPU with these inputs:

    quantity                  (2, 64, 64)    (1, 64, 128)
    symbols excluded              0.00 %         0.10 %
    indexes excluded              0.20 %         0.20 %
    largest scale                 2.12           2.44
    largest mean magnitude        3.23           3.97
"""
import ctypes
import sys

import numpy as np
import pytest
import torch

import scctx_ref

SMALL = scctx_ref.SMALL


def _product(**kw):
    from clc_amd import models

    return models.Elic2022(**{**SMALL, **kw})


def test_state_dict_matches_the_restatement():
    p, r = _product(), scctx_ref.Elic2022(**SMALL)
    sp, sr = p.state_dict(), r.state_dict()
    assert list(sp.keys()) == list(sr.keys())
    for k in sp:
        assert tuple(sp[k].shape) == tuple(sr[k].shape), k
        assert sp[k].dtype == sr[k].dtype, k
    M, groups = SMALL["M"], SMALL["groups"]
    assert len(p.channel_context) == len(p.spatial_context) == len(p.aggregation) == len(groups)
    assert len(p.channel_context[0]) == 0 and not any(k.startswith("channel_context.0.") for k in sp)   # list indexes equal group numbers
    assert tuple(sp["channel_context.3.0.weight"].shape) == (12, 16, 5, 5) and tuple(sp["channel_context.3.4.weight"].shape) == (32, 8, 5, 5)
    assert tuple(sp["spatial_context.2.weight"].shape) == (16, 8, 5, 5) and tuple(sp["spatial_context.2.mask"].shape) == (16, 8, 5, 5)
    assert tuple(sp["aggregation.0.0.weight"].shape) == (40, 2 * M + 2 * 4, 1, 1)
    assert tuple(sp["aggregation.3.0.weight"].shape) == (40, 2 * M + 4 * 16, 1, 1) and tuple(sp["aggregation.3.4.weight"].shape) == (32, 24, 1, 1)
    assert tuple(sp["h_s.4.weight"].shape) == (2 * M, 12, 3, 3) and tuple(sp["entropy_bottleneck.quantiles"].shape) == (8, 1, 3)
    # the default model: the layer widths the aggregation kernel is measured at
    d = _product(N=192, M=320, groups=(16, 16, 32, 64, 192), ch_widths=(224, 128), agg_widths=(640, 512))
    assert [a[0].in_channels for a in d.aggregation] == [672, 704, 768, 896, 1408]
    assert [a[4].out_channels for a in d.aggregation] == [32, 32, 64, 128, 384] and d.starts == (0, 16, 32, 64, 128)


def test_load_state_dict_is_strict_clean_both_ways():
    p, r = _product(), scctx_ref.small_reference()
    res = p.load_state_dict(r.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in r.state_dict().items():
        assert torch.equal(p.state_dict()[k], v), k
    res = r.load_state_dict(_product().state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    r.update(force=True)   # a checkpoint saved after update(): the empty CDF buffers are resized
    res = _product().load_state_dict(r.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys


def test_constructor_refusals():
    with pytest.raises(ValueError, match=r"Elic2022: sum\(groups\) must equal M"):
        _product(groups=(4, 4, 8, 12))
    with pytest.raises(ValueError, match=r"Elic2022: groups\[1\] must be a positive multiple of 4"):
        _product(groups=(4, 6, 6, 16))
    with pytest.raises(ValueError, match=r"Elic2022: ch_widths\[0\] must be a positive multiple of 4"):
        _product(ch_widths=(10, 8))
    with pytest.raises(ValueError, match=r"Elic2022: agg_widths\[1\] must be a positive multiple of 4"):
        _product(agg_widths=(40, 22))
    with pytest.raises(ValueError, match=r"Elic2022: N must be a positive multiple of 4"):
        _product(N=10)
    with pytest.raises(ValueError, match=r"Elic2022: N//2 must be a positive multiple of 4"):
        _product(N=12)
    # (N*3//2 is checked by name too, but no N passes the two checks before it and fails that one: N % 8 == 0 implies it)
    with pytest.raises(ValueError, match=r"Elic2022: M//2 must be a multiple of 4"):
        _product(M=36, groups=(4, 4, 8, 20))
    with pytest.raises(ValueError, match=r"Elic2022: ch_widths and agg_widths take two widths"):
        _product(agg_widths=(40, 24, 8))


def test_compat_and_zoo_names():
    from clc_amd import compat, lib, models

    assert "Elic2022" in models.__all__ and "scctx_order" in models.__all__
    saved = {k: v for k, v in sys.modules.items() if k == "models" or k.split(".")[0] in ("compressai", "timm", "pytorch_msssim")}
    try:
        compat.install(force=True)
        import compressai.models as cm
        import compressai.zoo as cz

        assert cm.Elic2022 is models.Elic2022
        assert cz.models["elic2022"] is models.Elic2022
        assert cz.models["mbt2018-checkerboard"] is models.JointCheckerboardHierarchicalPriors
    finally:
        for k in [k for k in sys.modules if k == "models" or k.split(".")[0] in ("compressai", "timm", "pytorch_msssim")]:
            del sys.modules[k]
        sys.modules.update(saved)
    assert "clc_row_gemm" in lib.SIGNATURES
    assert "written from the paper" in models.Elic2022.__doc__.lower()
    if not torch.cuda.is_available():   # no CPU fallback
        from clc_amd import ops

        with pytest.raises(lib.ClcError):
            _product()(torch.rand(1, 3, 64, 64))
        with pytest.raises((lib.ClcError, ValueError)):
            ops.row_gemm([("dense", torch.zeros(2, 4))], torch.zeros(1, 2, dtype=torch.int32), 1, 1, 1, torch.zeros(4, 4), None, torch.zeros(2, 4))


@pytest.mark.parametrize("H,W", [(1, 1), (2, 3), (4, 4), (4, 8), (5, 7)])
def test_stream_order(H, W):
    from clc_amd.models import ckbd_pixels, scctx_order

    groups = SMALL["groups"]
    M = sum(groups)
    order = scctx_order(H, W, groups)
    assert order.dtype == np.int64 and order.shape == (H * W * M, 2)
    pairs = [tuple(int(v) for v in row) for row in order]
    assert pairs == scctx_ref.scctx_order(H, W, groups)
    assert sorted(pairs) == [(p, c) for p in range(H * W) for c in range(M)]   # every (pixel, channel) exactly once
    anchors, others = ckbd_pixels(H, W)
    pos, start = 0, 0
    for c in groups:   # groups ascending; inside a group anchors before non-anchors, raster inside, channels inner
        for lst in (anchors, others):
            assert lst == sorted(lst)
            for h, w in lst:
                assert pairs[pos:pos + c] == [(h * W + w, ch) for ch in range(start, start + c)]
                pos += c
        start += c
    assert pos == len(pairs)


@pytest.fixture(scope="module")
def reference():
    o = scctx_ref.small_reference().double().eval()
    o.update(force=True)
    return o


@pytest.mark.parametrize("B,h,w", [(2, 64, 64), (1, 64, 128)])
def test_restatement_passes_against_teacher_forced(reference, B, h, w):
    from clc_amd.recipe import synthetic_image

    o = reference
    M = SMALL["M"]
    x = synthetic_image(B, h, w, 321, smooth=True).double()
    with torch.no_grad():
        y = o.g_a(x)
        z_hat, _ = o.entropy_bottleneck(o.h_a(y))   # eval mode: the dequantised z
        params = o.h_s(z_hat)
        sym, idx, y_hat, scales, means = o.compress_scctx(y, params)
        sc_tf, mu_tf = o.teacher_forced(y_hat, params)
    _, _, H, W = y.shape
    for name, a, b in (("scales", sc_tf, scales), ("means", mu_tf, means)):
        gap = (a - b).abs().max().item()
        print(f"{H}x{W} float64 teacher-forced against the {2 * len(o.groups)} passes, {name}: {gap:.2e}")
        assert gap <= 1e-15, (name, gap)
    print(f"{H}x{W} largest scale {scales.max().item():.3f}, largest |mean| {means.abs().max().item():.3f}")
    assert scales.max().item() > 1.0 and means.abs().max().item() > 1.0
    # the loop is self-consistent: y_hat = sym + mean, idx = build_indexes(scale)
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(B, H * W, M)
    assert torch.equal(rows(y_hat), sym.double() + rows(means))
    assert int(sym.abs().max()) >= 2 and int(idx.max()) > int(idx.min())
    # the exclusion shares of the GPU consistency test, on the reference alone
    d = rows(y) - rows(mu_tf)
    frac = d - torch.floor(d)
    safe = (frac - 0.5).abs() > 1e-4
    excluded = 1.0 - safe.double().mean().item()
    print(f"{H}x{W} symbols: {100 * excluded:.3f} % excluded")
    assert excluded <= 0.01
    assert torch.equal(sym[safe], torch.round(d).int()[safe])
    table = o.gaussian_conditional.scale_table.double()
    safe = ((rows(sc_tf).unsqueeze(-1) - table).abs() > 1e-4 * table).all(-1)
    excluded = 1.0 - safe.double().mean().item()
    print(f"{H}x{W} indexes: {100 * excluded:.3f} % excluded")
    assert excluded <= 0.01
    assert torch.equal(idx[safe], rows(o.gaussian_conditional.build_indexes(sc_tf)).int()[safe])


def test_row_gemm_refusals_before_any_launch():
    """every refusal of clc_row_gemm is decided on the host from the arguments alone: fake (never dereferenced) device addresses"""
    from clc_amd import lib

    L = lib.load()
    A = 0x10000   # a 16-byte aligned address that nothing reads

    def call(srcs=((A, 8, 8, lib.AR_SRC_PIXEL),), nsrc=None, pix=A, P=5, B=1, H=3, W=5, w=A, bias=None, N=4, act=lib.ACT_RELU, out=A, ldo=4):
        arr = (lib.ArSrc * 5)()
        for i, (p, ld, Cc, kind) in enumerate(srcs):
            arr[i] = lib.ArSrc(p, ld, Cc, kind)
        return L.clc_row_gemm(arr if srcs is not None else None, len(srcs) if nsrc is None else nsrc, pix, P, B, H, W, w, bias, N, act, out, ldo, None)

    def refused(pattern, **kw):
        assert call(**kw) < 0, kw
        msg = L.clc_last_error().decode()
        assert msg.startswith("clc_row_gemm: ") and pattern in msg, msg

    for field in ("pix", "w", "out"):
        refused("null pointer", **{field: None})
    refused("nsrc must be 1 to 4 (got 0)", nsrc=0)
    refused("nsrc must be 1 to 4 (got 5)", srcs=((A, 8, 8, lib.AR_SRC_PIXEL),) * 5)
    for field in ("P", "B", "H", "W", "N"):
        refused("P, B, H, W and N must be positive", **{field: 0})
    for act in (lib.ACT_GELU, lib.ACT_SIGMOID, -1):
        refused(f"act must be CLC_ACT_NONE, CLC_ACT_LRELU or CLC_ACT_RELU (got {act})", act=act)
    refused("ldo < N (ldo=3 N=4)", ldo=3)
    refused("B * H * W must be below 2^31", B=1 << 11, H=1 << 10, W=1 << 10)
    refused("B * P must be below 2^31", B=1 << 11, P=1 << 20)
    refused("range 0 is CLC_AR_SRC_TAPS: the gather stays with clc_ar_linear", srcs=((A, 8, 8, lib.AR_SRC_TAPS),))
    refused("range 1 is CLC_AR_SRC_TAPS", srcs=((A, 8, 8, lib.AR_SRC_DENSE), (A, 8, 8, lib.AR_SRC_TAPS)))
    refused("range 1 has unknown kind 7", srcs=((A, 8, 8, lib.AR_SRC_DENSE), (A, 8, 8, 7)))
    refused("range 0 has a null pointer", srcs=((None, 8, 8, lib.AR_SRC_PIXEL),))
    refused("C % 4 != 0 (range 2 has C = 6)", srcs=((A, 8, 8, 0), (A, 8, 8, 1), (A, 8, 6, 1)))
    refused("C % 4 != 0 (range 0 has C = 0)", srcs=((A, 8, 0, 0),))
    refused("ld % 4 != 0 or ld < C (range 0 has ld = 10, C = 8)", srcs=((A, 10, 8, 0),))
    refused("ld % 4 != 0 or ld < C (range 3 has ld = 4, C = 8)", srcs=((A, 8, 8, 0),) * 3 + ((A, 4, 8, 1),))
    refused("range 1 is not 16-byte aligned", srcs=((A, 8, 8, 0), (A + 4, 8, 8, 1)))
    refused("the filter w is not 16-byte aligned", w=A + 8)
    assert ctypes.sizeof(lib.ArSrc) == 24
