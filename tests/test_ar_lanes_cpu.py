"""The lanes stream of mbt2018 and mbt2018-checkerboard without a GPU (clc_amd/models/hyperprior.py): the two orders and
their segments, a numpy restatement of the stream through the host coder, every refusal of both models by name and before any device
work (the models are on the CPU, where no kernel and no upload can run; device halves stubbed as in tests/test_codec_lanes_cpu.py), the
argument refusals of the two new C entries, which return before any launch, and the default compress / decompress, which must not
notice any of it.  Every comparison is exact.
"""
import ctypes

import numpy as np
import pytest
import torch

from test_rans_lanes_cpu import lanes_table

N_, M_ = 12, 24
SIZES = [(1, 1), (1, 5), (4, 2), (4, 8), (8, 12)]


def _models():
    from clc_amd import models

    return [models.JointAutoregressiveHierarchicalPriors(N_, M_), models.JointCheckerboardHierarchicalPriors(N_, M_)]


# ------------------------------------------------------------------------------------------------------------------------- the orders
@pytest.mark.parametrize("H,W", SIZES)
def test_wavefront_order_and_segments(H, W):
    from clc_amd.models import ar_lanes_order, ar_schedule

    p = _models()[0]
    order = ar_lanes_order(H, W)
    assert order.dtype == np.int64 and sorted(order.tolist()) == list(range(H * W))   # every pixel once
    steps = [s for s in ar_schedule(H, W, "wavefront") if s]
    segs = p._lanes_segments(H, W)
    assert segs == [len(s) * M_ for s in steps] and sum(segs) == H * W * M_ and all(n > 0 for n in segs)
    assert order.tolist() == [h * W + w for s in steps for h, w in s]
    at = 0
    for t, s in enumerate(steps):   # inside a step: one t = w + 3 h, ascending h
        hw = [(int(r) // W, int(r) % W) for r in order[at:at + len(s)]]
        assert len({w + 3 * h for h, w in hw}) == 1 and [h for h, _ in hw] == sorted(h for h, _ in hw)
        at += len(s)
    assert p._lanes_most(H, W) == max(len(s) for s in steps)
    assert type(p)._lanes_order is ar_lanes_order


def test_a_wavefront_has_more_segments_than_the_by_value_encoder_takes():
    from clc_amd import lib

    p = _models()[0]
    assert len(p._lanes_segments(8, 12)) == 33 == lib.RANS_LANES_MAX_SEGMENTS + 1
    assert len(p._lanes_segments(16, 16)) == 61 and len(p._lanes_segments(32, 48)) == 141   # W + 3 (H - 1)


@pytest.mark.parametrize("H,W", SIZES)
def test_checkerboard_order_and_segments(H, W):
    from clc_amd.models import ckbd_pixels

    p = _models()[1]
    anchors, others = ckbd_pixels(H, W)
    assert p._lanes_segments(H, W) == [len(anchors) * M_, len(others) * M_]
    assert p._lanes_order(H, W).tolist() == [h * W + w for h, w in anchors + others] == p._ckbd_order(H, W).tolist()
    assert p._lanes_most(H, W) == max(len(anchors), len(others))


# ------------------------------------------------------------------------------------------------ the stream, restated with numpy
@pytest.mark.parametrize("H,W", [(4, 8), (8, 12)])
@pytest.mark.parametrize("Wn", [1, 3])
@pytest.mark.parametrize("which", [0, 1])
def test_numpy_restatement_round_trips(H, W, Wn, which):
    """random raster [H W, M] symbols / indexes gathered into stream order, through ans.lanes_encode and ans.LanesDecoder segment by
    segment: the symbols come back and every wave stream ends at (2^31 x 64, its word count)"""
    from clc_amd import ans

    p = _models()[which]
    cdf, ln, off = lanes_table()
    g = np.random.default_rng(100 * H + 10 * Wn + which)
    idx = g.integers(0, 8, (H * W, M_)).astype(np.int32)
    maxv = ln[idx] - 2
    sym = (g.integers(0, 1 << 30, (H * W, M_)) % maxv + off[idx]).astype(np.int32)   # inside the rows ...
    sym[3, 5], sym[H * W - 1, M_ - 1], sym[0, 0] = 10**6, -77, off[idx[0, 0]] + maxv[0, 0]   # ... but for three escapes
    order, segs = p._lanes_order(H, W), p._lanes_segments(H, W)
    sym_s, idx_s = np.ascontiguousarray(sym[order]).reshape(-1), np.ascontiguousarray(idx[order]).reshape(-1)
    streams = ans.lanes_encode(sym_s, idx_s, segs, Wn, cdf, ln, off)
    assert len(streams) == Wn and ans.lanes_unpack(ans.lanes_pack(streams)) == streams
    d = ans.LanesDecoder(streams)
    got, at = np.empty_like(sym), 0
    for n in segs:
        px = order[at // M_:(at + n) // M_]
        got[px] = d.decode(idx_s[at:at + n], cdf, ln, off).reshape(-1, M_)   # a decoder's scatter: the step's pixels, channels inner
        at += n
    assert np.array_equal(got, sym) and d.at_end()
    for w in range(Wn):
        x, pos = d.state(w)
        assert (x == np.uint64(1 << 31)).all() and pos == len(streams[w]) // 4


# ------------------------------------------------------------------------------------------------------------------------- refusals
def _waves(g, k):
    return [g.integers(0, 256, 520, dtype=np.uint8).tobytes() for _ in range(k)]


def test_model_refusals_by_name():
    from clc_amd import ans

    g = np.random.default_rng(1)
    two, four = ans.lanes_pack(_waves(g, 2)), ans.lanes_pack(_waves(g, 4))
    plain = _waves(g, 1)[0]
    x = torch.zeros(1, 3, 64, 64)
    for p in _models():
        name = type(p).__name__
        for lanes in (0, 17, -1, True, 4.0, "4"):
            with pytest.raises(ValueError, match=rf"{name}.compress: lanes must be between 1 and 16"):
                p.compress(x, lanes=lanes)
            with pytest.raises(ValueError, match=rf"{name}.decompress: lanes must be between 1 and 16"):
                p.decompress([[b""], [b""]], (1, 1), lanes=lanes)
        for dc in (True, False):
            with pytest.raises(ValueError, match=r"lanes = 2, but the header of image 1 says 4 wave streams"):
                p.decompress([[two, four], [b"", b""]], (1, 1), lanes=2, device_coder=dc)
            with pytest.raises(ValueError, match=r"lanes = 4, but the header of image 0 says 2 wave streams"):
                p.decompress([[two], [b""]], (1, 1), lanes=4, device_coder=dc)
            with pytest.raises(ValueError, match="bad magic"):   # a default-format string handed to the lanes decoder
                p.decompress([[plain], [b""]], (1, 1), lanes=4, device_coder=dc)
            with pytest.raises(ValueError, match="2 y streams for 1 z streams"):
                p.decompress([[two, two], [b""]], (1, 1), lanes=2, device_coder=dc)
        with pytest.raises(ValueError, match="non-zero pad byte"):
            p.decompress([[two[:7] + b"\x02" + two[8:]], [b""]], (1, 1), lanes=2)
        with pytest.raises(ValueError, match=r"image 1 is a lanes stream \(b'CLN1'\); pass lanes= \(its header says 4 wave streams\)"):
            p.decompress([[plain, four], [b"", b""]], (1, 1))
        with pytest.raises(ValueError, match=r"image 0 is a lanes stream \(b'CLN1'\); pass lanes="):
            p.decompress([[two], [b""]], (1, 1), lanes=None)


def test_new_device_entries_refuse_their_arguments_before_any_launch():
    """Each call hands the library host buffers where device pointers belong: a launch would fault, a refusal returns -1 first."""
    from clc_amd import lib

    Lb = lib.load()
    ibuf = (ctypes.c_int32 * 4096)()
    ip = ctypes.addressof(ibuf)

    def refused(rc, who, what):
        assert rc == -1
        msg = Lb.clc_last_error().decode()
        assert who + ":" in msg and what in msg, msg

    names = ("gp", "ldg", "M", "pix", "P", "B", "H", "Wm", "table", "n_scales", "cdfs", "stride", "rows", "sizes", "offs", "words", "spans", "state",
             "W", "y_hat", "ldh", "sym", "ld_sym", "st")
    base = dict(gp=ip, ldg=50, M=24, pix=ip, P=3, B=2, H=4, Wm=8, table=ip, n_scales=64, cdfs=ip, stride=8, rows=4, sizes=ip, offs=ip, words=ip,
                spans=ip, state=ip, W=4, y_hat=ip, ldh=24, sym=ip, ld_sym=72, st=None)
    call = lambda **k: Lb.clc_ar_lanes_decode(*[{**base, **k}[n] for n in names])
    who = "clc_ar_lanes_decode"
    for name in ("gp", "table", "words", "spans", "state", "y_hat"):
        refused(call(**{name: None}), who, "null pointer")
    refused(call(pix=None), who, "null pixel list")
    for name in ("cdfs", "sizes", "offs"):
        refused(call(**{name: None}), who, "null table pointer")
    refused(call(stride=1), who, "cdf_stride >= 2")
    refused(call(rows=0), who, "n_rows >= 1")
    refused(call(n_scales=1), who, "n_scales must be between 2 and 256")
    refused(call(n_scales=257), who, "n_scales must be between 2 and 256")
    refused(call(W=0), who, "W must be between 1 and 16")
    refused(call(W=17), who, "W must be between 1 and 16")
    refused(call(P=-1), who, "P must not be negative")
    for name in ("B", "H", "Wm", "M"):
        refused(call(**{name: 0}), who, "must be positive")
    refused(call(P=1 << 26, M=16, ldg=32, sym=None), who, "n = P * M must be below 2^30")
    refused(call(ldg=47), who, "ldg < 2 M")
    refused(call(ldh=23), who, "ldh < M")
    refused(call(H=1 << 16, Wm=1 << 15), who, "B * H * W must be below 2^31")
    refused(call(ld_sym=71), who, "ld_sym < n")
    refused(call(B=1 << 23, H=1, Wm=1), who, "B * W must be below 2^24")
    assert call(P=0, pix=None, sym=None, ld_sym=0) == 0   # an empty step: nothing to do, nothing launched

    names = ("sym", "idx", "ld", "B", "seg", "P", "W", "cdfs", "stride", "rows", "sizes", "offs", "out", "regions", "result", "st")
    base = dict(sym=ip, idx=ip, ld=100, B=2, seg=ip, P=40, W=4, cdfs=ip, stride=8, rows=4, sizes=ip, offs=ip, out=ip, regions=ip, result=ip, st=None)
    call = lambda **k: Lb.clc_rans_lanes_encode_list(*[{**base, **k}[n] for n in names])
    who = "clc_rans_lanes_encode_list"
    for name in ("sym", "idx", "out", "regions", "result"):
        refused(call(**{name: None}), who, "null pointer")
    refused(call(seg=None), who, "null segment list")
    for name in ("cdfs", "sizes", "offs"):
        refused(call(**{name: None}), who, "null table pointer")
    refused(call(stride=1), who, "cdf_stride >= 2")
    refused(call(rows=0), who, "n_rows >= 1")
    refused(call(W=0), who, "W must be between 1 and 16")
    refused(call(W=17), who, "W must be between 1 and 16")
    refused(call(B=0), who, "B must be positive")
    refused(call(P=-1), who, "P must not be negative")
    refused(call(ld=-1), who, "ld must be between 0 and 2^27 - 1")
    refused(call(ld=1 << 27), who, "ld must be between 0 and 2^27 - 1")
    refused(call(B=1 << 23), who, "B * W must be below 2^24")


def test_wrapper_refusals_without_a_device():
    """the Python wrappers refuse host tensors by name before they touch the library; the by-value encoder keeps its 32 segments"""
    from clc_amd import ops

    t, f = torch.zeros(64, dtype=torch.int32), torch.zeros(4, 48)
    with pytest.raises(ValueError, match="ar ops: the pixel list must be a contiguous int32"):
        ops.ar_lanes_decode(f, 24, t, 1, 2, 2, f, (t, t, t), t, t, t, f)
    with pytest.raises(ValueError, match="rans_lanes_encode_list: symbols must be a contiguous int32 \\[B, T\\] device tensor"):
        ops.rans_lanes_encode_list(t.view(1, 64), t.view(1, 64), [1] * 33, 2, (t, t, t))
    with pytest.raises(ValueError, match="rans_lanes_encode_list: W must be between 1 and 16"):
        ops.rans_lanes_encode_list(t.view(1, 64), t.view(1, 64), [64], 0, (t, t, t))
    with pytest.raises(ValueError, match="rans_lanes_encode: symbols must be a contiguous int32 \\[B, T\\] device tensor"):
        ops.rans_lanes_encode(t.view(1, 64), t.view(1, 64), [64], 2, (t, t, t))


# ---------------------------------------------------------------------------------------------------------------- the default stays put
@pytest.mark.parametrize("which", [0, 1])
def test_defaults_are_todays_code_path(monkeypatch, which):
    """the device halves stubbed (fixed symbols on the CPU), so the host halves of compress / decompress run without a GPU"""
    from clc_amd import ans

    p = _models()[which]
    p.update(force=True)
    cdf, ln, off = p.gaussian_conditional.host_tables()
    B, H, W = 2, 4, 2
    g = np.random.default_rng(7 + which)
    sym = torch.from_numpy(g.integers(-40, 40, (B, H * W, M_)).astype(np.int32))
    idx = torch.from_numpy(g.integers(0, cdf.shape[0], (B, H * W, M_)).astype(np.int32))
    seen = {}
    monkeypatch.setattr(p, "_code_inputs", lambda x: (torch.zeros(B, M_, H, W), "params", [b"z0", b"z1"], (1, 1)))
    if which == 0:
        monkeypatch.setattr(p, "_ar_encode", lambda y, params, order="wavefront": seen.update(order=order) or (sym, idx, None))
        raster = np.arange(H * W)
    else:
        monkeypatch.setattr(p, "_ckbd_encode", lambda y, params: (sym, idx, None))
        raster = p._ckbd_order(H, W)
    in_order = lambda t, order, b: np.ascontiguousarray(t[b].numpy()[order]).reshape(-1)
    want = [ans.encode(in_order(sym, raster, b), in_order(idx, raster, b), cdf, ln, off) for b in range(B)]
    for item in (p.compress(None), p.compress(None, lanes=None)):
        assert sorted(item) == ["kernel_config", "shape", "strings"]   # no "lanes"
        assert item["strings"] == [want, [b"z0", b"z1"]]

    # compress(lanes=): the flat stream-order buffers and the segments reach the device half as they are
    def fake(s, i, segments, Wn):
        seen.update(sym=s, idx=i, segments=segments, W=Wn)
        return [ans.lanes_pack(ans.lanes_encode(s[b].numpy(), i[b].numpy(), segments, Wn, cdf, ln, off)) for b in range(B)]

    monkeypatch.setattr(p, "_lanes_encode_device", fake)
    lanes = p.compress(None, lanes=3)
    assert sorted(lanes) == ["kernel_config", "lanes", "shape", "strings"] and lanes["lanes"] == 3
    assert lanes["kernel_config"] == item["kernel_config"] and lanes["strings"][1] == item["strings"][1]
    order = p._lanes_order(H, W)
    assert seen["W"] == 3 and seen["segments"] == p._lanes_segments(H, W)
    assert seen["segments"] == ([M_] * 8 if which == 0 else [4 * M_, 4 * M_])   # 4 x 2: one pixel per non-empty step | 4 anchors, 4 others
    for b in range(B):
        assert seen["sym"][b].numpy().tolist() == in_order(sym, order, b).tolist()
        assert seen["idx"][b].numpy().tolist() == in_order(idx, order, b).tolist()
    if which == 0:   # order= picks the encoder's schedule of computation only: it reaches _ar_encode and nothing else
        assert seen["order"] == "wavefront"
        assert p.compress(None, order="raster", lanes=3)["strings"] == lanes["strings"] and seen["order"] == "raster"
        assert p.compress(None, "raster")["strings"] == item["strings"]

    # decompress: the default goes through _decode_passes and nothing else
    calls = []
    monkeypatch.setattr(p.entropy_bottleneck, "decompress", lambda s, shape: "z_hat")
    monkeypatch.setattr(p, "_hyper_synthesis", lambda z: torch.zeros(B, 2 * M_, H, W))
    monkeypatch.setattr(p, "_decode_passes", lambda s, params, most, passes, *sch: calls.append(("one", s, most, passes.__name__, sch)) or torch.zeros(1))
    monkeypatch.setattr(p, "_decode_lanes", lambda subs, params, dc=True: calls.append(("lanes", len(subs), len(subs[0]), dc)) or (torch.zeros(1), []))
    monkeypatch.setattr(p, "_synthesis", lambda y: y + 2.0)
    for out in (p.decompress(item["strings"], (1, 1)), p.decompress(item["strings"], (1, 1), lanes=None)):
        assert sorted(out) == ["x_hat"] and float(out["x_hat"]) == 1.0
    today = ("one", item["strings"][0], 1, "_ar_passes", ("raster",)) if which == 0 else ("one", item["strings"][0], 4, "_ckbd_passes", ())
    assert calls == [today] * 2
    p.decompress(lanes["strings"], (1, 1), lanes=3, device_coder=False, check=False)
    assert calls[-1] == ("lanes", 2, 3, False)
    p.decompress(lanes["strings"], (1, 1), lanes=3, check=False)
    assert calls[-1] == ("lanes", 2, 3, True)
