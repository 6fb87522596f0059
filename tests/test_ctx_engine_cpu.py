"""clc_amd.codec.ContextCodecEngine without a GPU: every refusal by name and before any device work (the models are on the
CPU, where no kernel, upload or capture can run), the schedule object the plans and the models' own calls share
(clc_amd.models.hyperprior.PassSchedule) against the functions that own each order, and the new keywords of
ops.rans_lanes_encode_list.  Every comparison is exact.
"""
import numpy as np
import pytest
import torch

from scctx_ref import SMALL

N_, M_ = 12, 24
CPU = torch.device("cpu")


def _served():
    from clc_amd import models

    return [models.JointAutoregressiveHierarchicalPriors(N_, M_), models.JointCheckerboardHierarchicalPriors(N_, M_)]


# ---------------------------------------------------------------------------------------------------------------------- refusals
def test_other_models_are_refused_by_name():
    from clc_amd import models
    from clc_amd.codec import ContextCodecEngine

    others = [models.ScaleHyperprior(N_, M_), models.MeanScaleHyperprior(N_, M_), models.Elic2022(**SMALL)]
    others += [cls(24, K) for name, cls in sorted(vars(models).items()) if name.startswith("Cheng2020") and isinstance(cls, type) for K in (1, 3)]
    assert len(others) == 7
    for p in others:
        with pytest.raises(ValueError, match=f"ContextCodecEngine: {type(p).__name__} is not served") as e:
            ContextCodecEngine(p, lanes=4)
        assert "JointAutoregressiveHierarchicalPriors and JointCheckerboardHierarchicalPriors" in str(e.value)
        if type(p).__name__.startswith("Cheng2020"):
            assert "takes no lanes=" in str(e.value)


@pytest.mark.parametrize("which", [0, 1])
def test_lanes_outside_the_format_are_refused(which):
    from clc_amd.codec import ContextCodecEngine

    p = _served()[which]
    with pytest.raises(ValueError, match="ContextCodecEngine: lanes=None .* is not served"):
        ContextCodecEngine(p, lanes=None)
    for W in (0, 17):
        with pytest.raises(ValueError, match="ContextCodecEngine: lanes must be between 1 and 16"):
            ContextCodecEngine(p, lanes=W)
    with ContextCodecEngine(p, lanes=16) as eng:
        assert eng.lanes == 16 and eng.use_graph and eng.max_plans == 0 and eng.last == {}
    assert eng.pool is None   # closed by the context manager


def test_items_are_refused_before_any_device_work():
    from clc_amd import ans
    from clc_amd.codec import ContextCodecEngine, kernel_config

    p = _served()[0]
    y = ans.lanes_pack([np.full(128, 1 << 31, "<u4").view("<u4").tobytes()] * 2)
    item = lambda shape, lanes: {"strings": [[y], [b"z"]], "shape": shape, "kernel_config": kernel_config(), "lanes": lanes}
    with ContextCodecEngine(p, lanes=2) as eng:
        with pytest.raises(ValueError, match="ContextCodecEngine.decompress: no items"):
            eng.decompress([])
        with pytest.raises(ValueError, match="decompress: item 1 was coded with lanes = 3, the call says lanes = 2"):
            eng.decompress([item((1, 1), 2), item((1, 1), 3)])
        with pytest.raises(ValueError, match=r"the items of one call share one shape, got \[\(1, 1\), \(1, 2\)\]"):
            eng.decompress([item((1, 1), 2), item((1, 2), 2)])
        one_stream = {"strings": [[b"\x00" * 8], [b"z"]], "shape": (1, 1)}
        with pytest.raises(ValueError, match="lanes_unpack: bad magic"):   # a one-stream string: the engine serves the lanes format only
            eng.decompress([one_stream])
        assert eng._dec == {} and eng._enc == {}


# ------------------------------------------------------------------------------------------------------------- the schedule object
@pytest.mark.parametrize("H,W", [(4, 8), (8, 12)])
def test_wavefront_schedule(H, W):
    from clc_amd.models import ar_schedule

    p, B = _served()[0], 2
    s = p._lanes_schedule(B, H, W, CPU)
    steps = [st for st in ar_schedule(H, W, "wavefront") if st]
    assert s.shape == (B, H, W, CPU) and s.steps == steps and s.ctx0 is None
    assert s.pix.dtype == torch.int32 and s.pix.tolist() == [list(px) for st in steps for px in st]
    assert s.segments == p._lanes_segments(H, W) == [len(st) * M_ for st in steps]
    assert s.order.dtype == torch.int64 and s.order.tolist() == p._lanes_order(H, W).tolist()
    assert s.seg_dev.dtype == torch.int32 and s.seg_dev.tolist() == s.segments
    rows = B * max(len(st) for st in steps)
    assert {k: tuple(v.shape) for k, v in s.ws.items()} == {"ctx": (rows, 2 * M_), "h1": (rows, M_ * 10 // 3), "h2": (rows, M_ * 8 // 3),
                                                            "gp": (rows, 2 * M_)}
    if (H, W) == (8, 12):
        assert len(s.segments) == 33 and sorted(set(s.segments)) == [M_, 2 * M_, 3 * M_, 4 * M_]
    # a schedule of another order: what the default decoder's call makes for itself
    r = p._pass_schedule(B, H, W, CPU, "raster")
    assert r.steps == [[(h, w)] for h in range(H) for w in range(W)] and r.segments is None and r.order is None
    assert tuple(r.ws["gp"].shape) == (B, 2 * M_)


@pytest.mark.parametrize("H,W", [(4, 8), (8, 12), (1, 1)])
def test_checkerboard_schedule(H, W):
    from clc_amd.models import ckbd_pixels

    p, B = _served()[1], 2
    s = p._lanes_schedule(B, H, W, CPU)
    anchors, others = ckbd_pixels(H, W)
    assert s.steps == [st for st in (anchors, others) if st]
    assert s.pix.tolist() == [list(px) for px in anchors + others]
    assert s.segments == p._lanes_segments(H, W) == [len(anchors) * M_, len(others) * M_]
    assert s.order.tolist() == p._lanes_order(H, W).tolist() == [h * W + w for h, w in anchors + others]
    assert tuple(s.ctx0.shape) == (B, 2 * M_, H, W) and not bool(s.ctx0.any()) and s.ctx0.is_contiguous(memory_format=torch.channels_last)
    assert tuple(s.ws["gp"].shape) == (B * max(len(anchors), len(others)), 2 * M_) and "ctx" not in s.ws
    assert p._lanes_encoder_keywords(s) == {} and list(_served()[0]._lanes_encoder_keywords(s)) == ["segments_dev"]


def test_a_schedule_refuses_another_latent():
    p = _served()[0]
    s = p._lanes_schedule(2, 4, 8, CPU)
    assert s.check(torch.zeros(2, M_, 4, 8)) is s
    for shape in ((1, M_, 4, 8), (2, M_, 8, 4)):
        with pytest.raises(ValueError, match="the schedule was made for"):
            s.check(torch.zeros(shape))


# ------------------------------------------------------------------------------------------ the keywords of rans_lanes_encode_list
def test_encode_list_keywords_are_checked_by_name():
    from clc_amd import ops

    t = torch.zeros(64, dtype=torch.int32)
    args = (t.view(1, 64), t.view(1, 64), [32, 32], 2, (t, t, t))
    for bad in ([32, 32], t[:2], t[:2].float(), np.zeros(2, np.int32)):   # not a tensor, on the host, not int32
        with pytest.raises(ValueError, match=r"rans_lanes_encode_list: segments_dev must be a contiguous int32 \[len\(segments\)\] device tensor"):
            ops.rans_lanes_encode_list(*args, segments_dev=bad)
    for bad in (np.zeros((1, 2, 2), np.int32), torch.zeros((1, 2, 2), dtype=torch.int32), torch.zeros((1, 2, 2))):
        with pytest.raises(ValueError, match=r"rans_lanes_encode_list: regions_dev must be a contiguous int32 \[B, W, 2\] device tensor"):
            ops.rans_lanes_encode_list(*args, regions_dev=bad)
    # without the keywords: today's first refusal, under today's name
    with pytest.raises(ValueError, match=r"rans_lanes_encode_list: symbols must be a contiguous int32 \[B, T\] device tensor"):
        ops.rans_lanes_encode_list(*args)
