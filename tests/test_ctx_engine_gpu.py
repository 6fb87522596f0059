"""clc_amd.codec.ContextCodecEngine on mbt2018 and mbt2018-checkerboard: JointAutoregressiveHierarchicalPriors(12, 24) and
JointCheckerboardHierarchicalPriors(12, 24) with the weights, inputs and once-computed reference items of
tests/test_ar_lanes_model_gpu.py's fixtures — one 128x192 image (latent 8x12: 33 wavefront segments of 1 to 4 pixels) and a 2x3x64x128
batch (latent 4x8) — at lanes = 2, one decompress case at lanes = 3.  Every comparison is exact.

The engine's items are model.compress(x, lanes=W)'s byte for byte and its x_hat is model.decompress(..., lanes=W)'s bit for bit, with
and without graphs and whatever the batch; the streams are not degenerate; a shape gets one plan per direction and one replay per call;
a words buffer too small for a longer stream gives a larger plan, never a truncated stream; the device -> host copies are counted; after
an in-place parameter change, update(scale_table=..., force=True) and load_state_dict the engine gives what the model gives now; a
flipped state word raises, naming the image; the container carries an item; the model's default path does not notice any of it.
"""
import copy

import pytest
import torch

from test_ar_lanes_model_gpu import LANES_W, M_, SHAPES, coded, dev, model  # noqa: F401  (fixtures)
from test_ar_model_gpu import _images
from test_cheng_model_gpu import _count_d2h

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def before(model, coded):
    """the default path's bytes and the kernel state, taken before any engine exists"""
    from clc_amd import codec

    return model.compress(coded["image"]["x"])["strings"], codec.kernel_config()


@pytest.fixture(scope="module")
def engine(model, before):
    from clc_amd.codec import ContextCodecEngine

    with ContextCodecEngine(model, lanes=LANES_W) as eng:
        yield eng


def _strings(items):
    return [[it["strings"][0][0] for it in items], [it["strings"][1][0] for it in items]]


def _want_x_hat(model, item, W=LANES_W):
    return model.decompress(item["strings"], item["shape"], lanes=W)["x_hat"]


@pytest.mark.parametrize("name", list(SHAPES))
def test_items_and_x_hat_are_the_model_s(model, coded, engine, name):
    from clc_amd.codec import ContextCodecEngine

    c = coded[name]
    want = c["lanes"]
    B = c["x"].shape[0]
    for b in range(B):   # not a degenerate stream
        assert int(c["sym"][b].abs().max()) >= 2 and int(c["idx"][b].max()) > int(c["idx"][b].min())
    x_hat = _want_x_hat(model, want)
    with ContextCodecEngine(model, lanes=LANES_W, use_graph=False) as eager:
        for eng, graphs in ((engine, 1), (eager, 0)):
            items = eng.compress(c["x"])
            assert eng.last["op"] == "compress" and eng.last["graphs"] == graphs and eng.last["hops"] == 2 and eng.last["rans_ms"] >= 0.0
            assert len(items) == B and _strings(items) == want["strings"]   # y AND z, per image
            for it in items:
                assert sorted(it) == ["kernel_config", "lanes", "shape", "strings"] and it["lanes"] == LANES_W
                assert tuple(it["shape"]) == tuple(want["shape"]) and it["kernel_config"] == want["kernel_config"]
            for check in (True, False):
                out = eng.decompress(items, check=check)
                assert torch.equal(out, x_hat), (graphs, check)
                assert eng.last["op"] == "decompress" and eng.last["graphs"] == graphs and eng.last["hops"] == int(check)


def test_an_image_s_strings_at_batch_2_are_those_at_batch_1(model, coded, engine):
    x = coded["batch"]["x"]
    both = engine.compress(x)
    for b in range(2):
        one = engine.compress(x[b:b + 1])
        assert one[0]["strings"] == both[b]["strings"]
        assert torch.equal(engine.decompress(one), engine.decompress(both)[b:b + 1])


def test_decompress_at_three_lanes(model, coded):
    from clc_amd.codec import ContextCodecEngine

    x = coded["image"]["x"]
    want = model.compress(x, lanes=3)
    with ContextCodecEngine(model, lanes=3) as eng:
        item = dict(want, strings=[want["strings"][0][:1], want["strings"][1][:1]])
        assert torch.equal(eng.decompress([item]), _want_x_hat(model, want, 3))
        assert _strings(eng.compress(x)) == want["strings"]


def test_one_plan_per_direction_and_one_replay(model, coded):
    from clc_amd.codec import ContextCodecEngine

    x = coded["image"]["x"]
    x2 = x.flip(3).contiguous()
    with ContextCodecEngine(model, lanes=LANES_W) as eng:
        a = eng.compress(x)
        assert eng.last["capture_ms"] > 0.0 and eng.last["graphs"] == 1
        xa = eng.decompress(a)
        assert eng.last["capture_ms"] > 0.0 and eng.last["graphs"] == 1 and not eng.last["plan_rebuilt"]
        b = eng.compress(x2)
        assert eng.last["capture_ms"] == 0.0 and eng.last["graphs"] == 1 and not eng.last["plan_rebuilt"]
        xb = eng.decompress(b)
        assert eng.last["capture_ms"] == 0.0 and eng.last["graphs"] == 1 and not eng.last["plan_rebuilt"]
        assert len(eng._enc) == 1 and len(eng._dec) == 1
        assert a[0]["strings"] != b[0]["strings"]
        want = model.compress(x2, lanes=LANES_W)
        assert _strings(b) == want["strings"] and torch.equal(xb, _want_x_hat(model, want))
        assert torch.equal(xa, _want_x_hat(model, coded["image"]["lanes"]))


def test_a_longer_stream_gets_a_larger_plan(model, coded):
    from clc_amd.codec import ContextCodecEngine

    x = coded["image"]["x"]
    flat = torch.full_like(x, 0.5)
    short, long_ = model.compress(flat, lanes=LANES_W), coded["image"]["lanes"]
    assert len(long_["strings"][0][0]) >= len(short["strings"][0][0]) + 4   # at least one 32-bit word more
    with ContextCodecEngine(model, lanes=LANES_W) as eng:
        eng.lanes_words_slack = 1.0
        items = [dict(it, strings=[it["strings"][0][:1], it["strings"][1][:1]]) for it in (short, long_)]
        assert torch.equal(eng.decompress(items[:1]), _want_x_hat(model, short))
        assert not eng.last["plan_rebuilt"]
        cap = next(iter(eng._dec.values())).cap_words
        assert torch.equal(eng.decompress(items[1:]), _want_x_hat(model, long_))
        assert eng.last["plan_rebuilt"] and eng.last["capture_ms"] > 0.0 and len(eng._dec) == 1
        assert next(iter(eng._dec.values())).cap_words > cap
        assert torch.equal(eng.decompress(items[:1]), _want_x_hat(model, short))   # the shorter one fits the larger plan
        assert not eng.last["plan_rebuilt"] and eng.last["capture_ms"] == 0.0


def test_counted_device_to_host_copies(model, coded, engine):
    x = coded["image"]["x"]
    items = engine.compress(x)   # (plans exist: the counts are those of a replay)
    engine.decompress(items)
    with _count_d2h() as n:
        engine.decompress(items, check=False)
    unchecked = n.n
    with _count_d2h() as n:
        engine.decompress(items, check=True)
    checked = n.n
    with _count_d2h() as n:
        engine.compress(x)
    enc = n.n
    print(f"device -> host copies: decompress {unchecked} / {checked} with the check, compress {enc}")
    assert unchecked == 0 and checked == 1 and enc == 2
    assert engine.last["hops"] == 2


def test_the_engine_follows_the_model_s_state(model, coded):
    from clc_amd.codec import ContextCodecEngine
    from clc_amd.models.clc import get_scale_table

    m = copy.deepcopy(model)   # (the module's model stays as the other tests take it)
    x = coded["batch"]["x"]

    def same(eng):
        want = m.compress(x, lanes=LANES_W)
        items = eng.compress(x)
        rebuilt = eng.last["plan_rebuilt"], eng.last["capture_ms"] > 0.0   # (the call that meets a moved state drops both directions' plans)
        assert _strings(items) == want["strings"]
        assert torch.equal(eng.decompress(items), _want_x_hat(m, want))
        assert (eng.last["capture_ms"] > 0.0) == rebuilt[1] and not eng.last["plan_rebuilt"]
        return want["strings"], rebuilt

    with ContextCodecEngine(m, lanes=LANES_W) as eng:
        first, rebuilt = same(eng)
        assert first == coded["batch"]["lanes"]["strings"] and rebuilt == (False, True)
        with torch.no_grad():
            m.entropy_parameters[4].weight.mul_(1.25)   # read by the encoder's and the decoder's graph
        second, rebuilt = same(eng)
        assert rebuilt == (True, True) and second[0] != first[0]
        assert m.update(scale_table=get_scale_table(0.11, 64, 40), force=True)
        third, rebuilt = same(eng)
        assert rebuilt == (True, True) and third[0] != second[0]
        sd = {k: v.clone() for k, v in m.state_dict().items()}
        sd["h_s.4.weight"] *= 1.125
        sd["g_s.6.weight"] *= 0.875
        m.load_state_dict(sd)
        fourth, rebuilt = same(eng)
        assert rebuilt == (True, True) and fourth[0] != third[0]
        assert same(eng) == (fourth, (False, False))   # an unchanged model keeps its plans


def test_end_state_check_and_container(model, coded, engine):
    from clc_amd import codec

    x = coded["batch"]["x"]
    items = engine.compress(x)
    good = engine.decompress(items)
    # a flipped state word (lane 5 of image 1's wave stream 0, a bit of its low word) raises, naming the image — and only that one
    s = bytearray(items[1]["strings"][0][0])
    s[8 + 4 * LANES_W + 8 * 5] ^= 0x10
    bad = [items[0], dict(items[1], strings=[[bytes(s)], items[1]["strings"][1]])]
    with pytest.raises(ValueError, match=r"image 1: wave streams \[.*\] did not decode to their end") as e:
        engine.decompress(bad, check=True)
    assert "image 0" not in str(e.value)
    out = engine.decompress(bad, check=False)   # unchecked: some image, the other one untouched
    assert torch.equal(out[0], good[0])
    # the container carries an item
    blobs = [codec.pack_item(it, image_hw=tuple(x.shape[-2:])) for it in items]
    back = [codec.unpack_item(b) for b in blobs]
    for it, bk in zip(items, back):
        assert bk["strings"] == it["strings"] and tuple(bk["shape"]) == tuple(it["shape"])
    assert torch.equal(engine.decompress(back), good)


def test_encode_list_with_the_caller_s_device_copies(dev, model, coded):
    """ops.rans_lanes_encode_list given regions_dev and segments_dev: the words and results of the call that uploads them itself"""
    from clc_amd import ops

    from clc_amd.models import JointAutoregressiveHierarchicalPriors as AR

    c = coded["image"]
    B, _, H, W = c["y"].shape
    s = model._lanes_schedule(B, H, W, dev)
    if hasattr(model, "_ckbd_lists"):   # either model's symbols and tables, cut by the wavefront's 33 segments
        s.segments = AR._lanes_segments(model, H, W)
        s.order = torch.from_numpy(AR._lanes_order(H, W)).to(dev)
        s.seg_dev = torch.tensor(s.segments, dtype=torch.int32).to(dev)
    assert len(s.segments) == 33
    gc = model.gaussian_conditional
    tables = (gc._quantized_cdf, gc._cdf_length, gc._offset)
    sym, idx = model._lanes_gather(c["sym"], s.order), model._lanes_gather(c["idx"], s.order)
    out, regions, result = ops.rans_lanes_encode_list(sym, idx, s.segments, LANES_W, tables)
    reg_dev = torch.from_numpy(regions).to(dev)
    out2, regions2, result2 = ops.rans_lanes_encode_list(sym, idx, s.segments, LANES_W, tables, regions=regions, regions_dev=reg_dev,
                                                         segments_dev=s.seg_dev)
    assert (regions2 == regions).all() and torch.equal(result2, result) and int(result[..., 1].min()) > 0
    for b in range(B):
        for w in range(LANES_W):
            first, n = (int(v) for v in result[b, w])
            assert torch.equal(out2[first:first + n], out[first:first + n])
    with pytest.raises(ValueError, match="rans_lanes_encode_list: segments_dev holds 32 lengths, segments 33"):
        ops.rans_lanes_encode_list(sym, idx, s.segments, LANES_W, tables, segments_dev=s.seg_dev[:32].contiguous())
    with pytest.raises(ValueError, match=r"rans_lanes_encode_list: regions_dev must be a contiguous int32 \[B, W, 2\] = \(1, 2, 2\) device tensor"):
        ops.rans_lanes_encode_list(sym, idx, s.segments, LANES_W, tables, regions_dev=torch.cat((reg_dev, reg_dev)))


def test_the_default_path_does_not_notice(model, coded, engine, before):
    from clc_amd import codec

    engine.decompress(engine.compress(coded["image"]["x"]))
    after = model.compress(coded["image"]["x"])
    assert sorted(after) == ["kernel_config", "shape", "strings"]
    assert after["strings"] == before[0] == coded["image"]["default"]["strings"]
    assert codec.kernel_config() == before[1] == after["kernel_config"]
