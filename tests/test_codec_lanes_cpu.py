"""The lanes stream of CLC / TCM without a GPU: the segment order restated in numpy, every refusal by name — the models'
and the engine's, before any device work — the argument refusals of the two new device entries, which return before any launch, and
the default compress / decompress, which must not notice any of it.

THE ORDER.  An image's y string holds P = num_slices segments in slice order; segment i is the slice's [h][w][C] block as it lies in
memory — pixels in raster order, channels inner — not the [C][h][w] order of the default stream.  Every comparison is exact."""
import ctypes

import numpy as np
import pytest
import torch

from test_rans_lanes_cpu import lanes_table


def _image(seed, S=5, C=3, h=5, w=9):
    """-> (symbols, indexes) int32 [S][C][h][w]: an image's slices as the default encoder sees them (logical NCHW); n = 135 per segment"""
    cdf, ln, off = lanes_table()
    g = np.random.default_rng(seed)
    idx = g.integers(0, cdf.shape[0], (S, C, h, w)).astype(np.int32)
    sym = (g.integers(-3, 4, idx.shape) + off[idx] + (ln[idx] - 2) // 2).astype(np.int32)
    sym.reshape(-1)[::41] = 10**6
    sym.reshape(-1)[7::53] = -10**6
    return sym, idx


@pytest.mark.parametrize("W", [1, 3])
def test_segment_order_round_trips(W):
    from clc_amd import ans

    cdf, ln, off = lanes_table()
    sym, idx = _image(3)
    S, C, h, w = sym.shape
    n = h * w * C
    nhwc = lambda a: np.ascontiguousarray(a.transpose(0, 2, 3, 1)).reshape(S, n)   # per slice: pixels in raster order, channels inner
    s_flat, i_flat = nhwc(sym), nhwc(idx)
    assert s_flat[2, (1 * w + 4) * C + 2] == sym[2, 2, 1, 4]   # symbol j of a segment: pixel j // C, channel j % C
    streams = ans.lanes_encode(s_flat.reshape(-1), i_flat.reshape(-1), [n] * S, W, cdf, ln, off)
    blob = ans.lanes_pack(streams)
    assert blob[:4] == ans.LANES_MAGIC == b"CLN1" and blob[4] == W
    d = ans.LanesDecoder(ans.lanes_unpack(blob))
    for i in range(S):   # a slice at a time, as the decoder meets them
        got = d.decode(i_flat[i], cdf, ln, off)
        assert np.array_equal(got.reshape(h, w, C).transpose(2, 0, 1), sym[i])
    assert d.at_end()
    # the NCHW order of the default stream is another stream
    other = ans.lanes_encode(sym.reshape(-1), idx.reshape(-1), [n] * S, W, cdf, ln, off)
    assert other != streams


def _models():
    from clc_amd import models

    return [models.CLC(N=64, num_ref_frames=1), models.TCM(N=64)]


def _waves(g, k):
    return [g.integers(0, 256, 520, dtype=np.uint8).tobytes() for _ in range(k)]


def test_model_refusals_by_name():
    """all of them before any device work: the models are on the CPU, where no kernel and no upload can run"""
    from clc_amd import ans

    g = np.random.default_rng(1)
    two, four = ans.lanes_pack(_waves(g, 2)), ans.lanes_pack(_waves(g, 4))
    plain = _waves(g, 1)[0]
    x = torch.zeros(1, 3, 128, 128)
    for p in _models():
        name = type(p).__name__
        for lanes in (0, 17, -1, True, 4.0, "4"):
            with pytest.raises(ValueError, match=rf"{name}.compress: lanes must be between 1 and 16"):
                p.compress(x, lanes=lanes)
            with pytest.raises(ValueError, match=rf"{name}.compress: lanes must be between 1 and 16"):
                p._compress_eager(x, lanes=lanes)
            with pytest.raises(ValueError, match=rf"{name}.decompress: lanes must be between 1 and 16"):
                p.decompress([[b""], [b""]], (2, 2), lanes=lanes)
            with pytest.raises(ValueError, match=rf"{name}.decompress: lanes must be between 1 and 16"):
                p._decompress_eager([[b""], [b""]], (2, 2), lanes=lanes)
        for dc in (True, False):
            with pytest.raises(ValueError, match=r"lanes = 2, but the header of image 1 says 4 wave streams"):
                p.decompress([[two, four], [b"", b""]], (2, 2), lanes=2, device_coder=dc)
            with pytest.raises(ValueError, match=r"lanes = 4, but the header of image 0 says 2 wave streams"):
                p.decompress([[two], [b""]], (2, 2), lanes=4, device_coder=dc)
            with pytest.raises(ValueError, match="bad magic"):   # a default-format string handed to the lanes decoder
                p.decompress([[plain], [b""]], (2, 2), lanes=4, device_coder=dc)
        with pytest.raises(ValueError, match=r"image 1 is a lanes stream \(b'CLN1'\); pass lanes= \(its header says 4 wave streams\)"):
            p.decompress([[plain, four], [b"", b""]], (2, 2))
        with pytest.raises(ValueError, match=r"image 0 is a lanes stream \(b'CLN1'\); pass lanes="):
            p.decompress([[two], [b""]], (2, 2))
        with pytest.raises(ValueError, match="2 y streams for 1 z streams"):
            p._decompress_eager([[two, two], [b""]], (2, 2), lanes=2)


class _Stop(Exception):
    pass


def test_engine_refusals_and_defaults(monkeypatch):
    """the engine on stubbed device halves: the plan builders and runners record what reaches them"""
    from clc_amd import ans, codec

    g = np.random.default_rng(2)
    two = ans.lanes_pack(_waves(g, 2))
    plain = _waves(g, 1)[0]
    m = _models()[1]
    eng = codec.CodecEngine(m, threads=1)
    x = torch.zeros(2, 3, 128, 128)
    for lanes in (0, 17, True, 2.0):
        with pytest.raises(ValueError, match="CodecEngine.compress: lanes must be between 1 and 16"):
            eng.compress(x, lanes=lanes)
        with pytest.raises(ValueError, match="CodecEngine.decompress: lanes must be between 1 and 16"):
            eng.decompress([{"strings": [[two], [b""]], "shape": (2, 2)}], lanes=lanes)
    built = []

    def stop(*a, **k):
        built.append((a, k))
        raise _Stop

    monkeypatch.setattr(eng, "_build_decoder", stop)
    monkeypatch.setattr(eng, "_build_decoder_lanes", stop)
    item = lambda y, **k: {"strings": [[y], [b""]], "shape": (2, 2), **k}
    with pytest.raises(ValueError, match="item 1 was coded with lanes = 2, the call says lanes = None"):
        eng.decompress([item(plain), item(two, lanes=2)])
    with pytest.raises(ValueError, match="item 0 was coded with lanes = 2, the call says lanes = 4"):
        eng.decompress([item(two, lanes=2)], lanes=4)
    with pytest.raises(ValueError, match=r"image 1 is a lanes stream \(b'CLN1'\); pass lanes="):
        eng.decompress([item(plain), item(two)])
    with pytest.raises(ValueError, match="lanes = 3, but the header of image 0 says 2 wave streams"):
        eng.decompress([item(two)], lanes=3)
    with pytest.raises(ValueError, match="bad magic"):
        eng.decompress([item(two), item(plain)], lanes=2)
    assert built == []   # nothing above reached a plan, an upload or a kernel
    # the default decompress goes to today's builder, lanes=W to the new one with W and a words capacity that holds the batch
    with pytest.raises(_Stop):
        eng.decompress([item(plain)])
    assert len(built) == 1 and built[0][0][:2] == (1, (2, 2)) and len(built[0][0]) == 4
    with pytest.raises(_Stop):
        eng.decompress([item(two), item(two)], lanes=2)
    args = built[1][0]
    assert args[:2] == (2, (2, 2)) and args[4] == 2 and args[5] >= 2 * 2 * 130

    # compress: the default builds today's plan (lanes=None) under today's signature; lanes=W another plan under another
    plans = []

    def build(x_, refs, bank=None, lanes=None):
        plans.append(lanes)
        pl = codec._Plan()
        pl.lanes = lanes
        return pl

    monkeypatch.setattr(eng, "_build_encoder", build)
    monkeypatch.setattr(eng, "_run_encoder", lambda pl, x_, refs: [{"strings": [[b"y"], [b"z"]], "shape": (2, 2), "kernel_config": (6, 0),
                                                                     **({"lanes": pl.lanes} if pl.lanes else {})}])
    assert sorted(eng.compress(x)[0]) == ["kernel_config", "shape", "strings"]
    assert list(eng._enc) == [eng._sig(x, None)]
    assert eng.compress(x, lanes=3)[0]["lanes"] == 3 and eng.compress(x, lanes=3)[0]["lanes"] == 3
    assert plans == [None, 3] and list(eng._enc) == [eng._sig(x, None), eng._sig(x, None) + (("lanes", 3),)]
    eng._enc.clear()
    eng.close()


def test_model_defaults_are_todays_code_path(monkeypatch):
    """the model's halves stubbed: the default compress / decompress make today's calls with today's arguments"""
    from clc_amd import ans

    g = np.random.default_rng(3)
    two = ans.lanes_pack(_waves(g, 2))
    for p in _models():
        calls = []

        class Eng:
            def compress(self, x, refs, **k):
                calls.append(("eng.compress", k))
                return [{"strings": [[two if k else b"y"], [b"z"]], "shape": (2, 2), "kernel_config": (6, 0), **({"lanes": k["lanes"]} if k else {})}]

            def decompress(self, items, refs, **k):
                calls.append(("eng.decompress", k))
                return "x_hat"

        monkeypatch.setattr(p, "_prep", lambda x: x)
        monkeypatch.setattr(p, "_codec_engine", lambda x_like: Eng())
        monkeypatch.setattr(p, "_compress_eager", lambda *a, **k: calls.append(("eager.compress", len(a), k)) or {})
        monkeypatch.setattr(p, "_decompress_eager", lambda *a, **k: calls.append(("eager.decompress", len(a), k)) or {})
        x = torch.zeros(1, 3, 128, 128)
        out = p.compress(x)
        assert sorted(out) == ["kernel_config", "shape", "strings"]   # no "lanes"
        assert sorted(p.compress(x, lanes=None)) == ["kernel_config", "shape", "strings"]
        p.decompress(out["strings"], out["shape"])
        p.compress(torch.zeros(2, 3, 128, 128))
        p.decompress([[b"y"], [b"z", b"z"]], (2, 2))
        assert calls == [("eng.compress", {}), ("eng.compress", {}), ("eng.decompress", {}), ("eager.compress", 2, {}), ("eager.decompress", 3, {})]
        del calls[:]
        lanes = p.compress(x, lanes=2)
        assert sorted(lanes) == ["kernel_config", "lanes", "shape", "strings"] and lanes["lanes"] == 2
        p.decompress(lanes["strings"], lanes["shape"], lanes=2, check=False)
        p.decompress(lanes["strings"], lanes["shape"], lanes=2, device_coder=False)
        p.compress(torch.zeros(2, 3, 128, 128), lanes=2)
        assert calls == [("eng.compress", {"lanes": 2}), ("eng.decompress", {"lanes": 2, "check": False}),
                         ("eager.decompress", 3, {"lanes": 2, "device_coder": False, "check": True}), ("eager.compress", 2, {"lanes": 2})]


def test_pack_item_carries_the_string_opaquely():
    from clc_amd import ans, codec

    g = np.random.default_rng(4)
    two = ans.lanes_pack(_waves(g, 2))
    item = {"strings": [[two], [b"zz"]], "shape": torch.Size([2, 2]), "kernel_config": codec.kernel_config(), "lanes": 2}
    back = codec.unpack_item(codec.pack_item(item, image_hw=(128, 128)))
    assert back["strings"] == item["strings"] and "lanes" not in back and tuple(back["shape"]) == (2, 2)


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

    names = ("scale", "ldsc", "mu", "ldmu", "C", "n", "B", "table", "n_scales", "cdfs", "stride", "rows", "sizes", "offs", "words", "spans", "state",
             "W", "y_hat", "ldh", "sym", "ld_sym", "st")
    base = dict(scale=ip, ldsc=7, mu=ip, ldmu=7, C=5, n=65, B=2, table=ip, n_scales=64, cdfs=ip, stride=8, rows=4, sizes=ip, offs=ip, words=ip,
                spans=ip, state=ip, W=4, y_hat=ip, ldh=7, sym=ip, ld_sym=65, st=None)
    call = lambda **k: Lb.clc_rans_lanes_decode_gauss(*[{**base, **k}[n] for n in names])
    who = "clc_rans_lanes_decode_gauss"
    for name in ("scale", "mu", "table", "words", "spans", "state", "y_hat"):
        refused(call(**{name: None}), who, "null pointer")
    for name in ("cdfs", "sizes", "offs"):
        refused(call(**{name: None}), who, "null table pointer")
    refused(call(stride=1), who, "cdf_stride >= 2")
    refused(call(rows=0), who, "n_rows >= 1")
    refused(call(n_scales=1), who, "n_scales must be between 2 and 256")
    refused(call(n_scales=257), who, "n_scales must be between 2 and 256")
    refused(call(W=0), who, "W must be between 1 and 16")
    refused(call(W=17), who, "W must be between 1 and 16")
    refused(call(n=-5), who, "n must not be negative")
    refused(call(B=0), who, "B must be positive")
    refused(call(n=1 << 30, C=1, sym=None), who, "n must be below 2^30")
    refused(call(C=0), who, "whole rows of C > 0 channels")
    refused(call(n=64), who, "whole rows of C > 0 channels")
    for name in ("ldsc", "ldmu", "ldh"):
        refused(call(**{name: 4}), who, "ldsc, ldmu or ldh < C")
    refused(call(ld_sym=64), who, "ld_sym < n")
    refused(call(B=1 << 23), who, "B * W must be below 2^24")
    assert call(n=0, sym=None, ld_sym=0) == 0   # an empty segment: nothing to do, nothing launched

    names = ("words", "n_words", "result", "B", "W", "packed", "cap", "header", "st")
    base = dict(words=ip, n_words=4096, result=ip, B=2, W=3, packed=ip, cap=4096, header=ip, st=None)
    call = lambda **k: Lb.clc_rans_lanes_pack(*[{**base, **k}[n] for n in names])
    who = "clc_rans_lanes_pack"
    for name in ("words", "result", "packed", "header"):
        refused(call(**{name: None}), who, "null pointer")
    refused(call(W=0), who, "W must be between 1 and 16")
    refused(call(W=17), who, "W must be between 1 and 16")
    refused(call(B=0), who, "B must be positive")
    refused(call(B=1 << 23), who, "B * W must be below 2^24")
    refused(call(n_words=-1), who, "n_words must be between 0 and 2^31 - 1")
    refused(call(cap=-1), who, "capacity must be between 0 and 2^31 - 1")
    refused(call(cap=1 << 31), who, "capacity must be between 0 and 2^31 - 1")


def test_wrapper_refusals_without_a_device():
    from clc_amd import ops

    t, f = torch.zeros(64, dtype=torch.int32), torch.zeros(1, 4, 4, 4)
    with pytest.raises(ValueError, match="rans_lanes_decode_gauss: scale must be a float32 \\[B, C, H, W\\] device tensor"):
        ops.rans_lanes_decode_gauss(f, f, f, (t, t, t), t, t, t)
    with pytest.raises(ValueError, match="rans_lanes_pack: out must be a contiguous int32 device tensor"):
        ops.rans_lanes_pack(t, t)
