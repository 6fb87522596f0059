"""mbt2018 and mbt2018-checkerboard on the lanes stream (compress(x, lanes=W) / decompress(..., lanes=W); clc_amd/models/hyperprior.py):
JointAutoregressiveHierarchicalPriors(12, 24) with the weights of tests/test_ar_model_gpu.py::pair and
JointCheckerboardHierarchicalPriors(12, 24) with those of tests/test_ckbd_model_gpu.py, on one 128x192 image (latent 8x12: 33 wavefront
steps, one more than the by-value encoder takes) and a 2x3x64x128 batch (latent 4x8), at lanes = 2.  Every comparison is exact.

The device-encoded strings are ans.lanes_pack(ans.lanes_encode(...)) of the encoder's symbols in stream order, whatever order= the
encoder computed in; decompress returns the same x_hat, and the same y_hat bit for bit, from the device decoder, from the host decoder
of the same format and from the default format; the device path's device -> host copies are counted; an image's string does not depend
on the batch around it; the container carries it; a flipped state word raises, naming the image; the default path's bytes and the
kernel_config tag do not notice any of it.
"""
import numpy as np
import pytest
import torch

import ar_ref
import ckbd_ref
from test_ar_model_gpu import _images
from test_cheng_model_gpu import _count_d2h

pytestmark = pytest.mark.gpu

N_, M_ = 12, 24
LANES_W = 2
SHAPES = {"image": (1, 128, 192), "batch": (2, 64, 128)}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module", params=["mbt2018", "checkerboard"])
def model(request, dev):
    """the product model with the weights of tests/test_ar_model_gpu.py::pair / tests/test_ckbd_model_gpu.py::pair; tables built"""
    from clc_amd import models
    from clc_amd.recipe import apply_weight_recipe

    name = "JointAutoregressiveHierarchicalPriors" if request.param == "mbt2018" else "JointCheckerboardHierarchicalPriors"
    r = getattr(ar_ref if request.param == "mbt2018" else ckbd_ref, name)(N_, M_)
    apply_weight_recipe(r, 3)
    with torch.no_grad():
        r.g_a[6].weight.mul_(20.0)
        r.h_s[4].weight.mul_(4.0)
        r.h_s[4].bias.add_(0.6)
        r.entropy_parameters[4].weight.mul_(8.0)
        r.entropy_parameters[4].bias[:M_].add_(0.6)
    p = getattr(models, name)(N_, M_)
    p.load_state_dict(r.state_dict())
    p = p.to(dev).eval()
    p.update(force=True)
    return p


def _encode(model, y, params):
    return model._ckbd_encode(y, params) if hasattr(model, "_ckbd_lists") else model._ar_encode(y, params)


@pytest.fixture(scope="module")
def coded(dev, model):
    """per input: the encoder's tensors, the default item and the lanes item, computed once"""
    out = {}
    for name, (B, h, w) in SHAPES.items():
        x = _images(B, h, w).to(dev)
        y, params, z_strings, z_size = model._code_inputs(x)
        sym, idx, y_hat = _encode(model, y, params)
        out[name] = dict(x=x, y=y, params=params, sym=sym, idx=idx, y_hat=y_hat, default=model.compress(x), lanes=model.compress(x, lanes=LANES_W))
    return out


def _is_ar(model):
    return not hasattr(model, "_ckbd_lists")


@pytest.mark.parametrize("name", list(SHAPES))
def test_bytes_are_the_host_encoder_s(model, coded, name):
    from clc_amd import ans

    c = coded[name]
    B, _, H, W = c["y"].shape
    assert (H, W) == ((8, 12) if name == "image" else (4, 8)) and c["y"].shape[1] == M_
    item = c["lanes"]
    assert sorted(item) == ["kernel_config", "lanes", "shape", "strings"] and item["lanes"] == LANES_W
    assert item["strings"][1] == c["default"]["strings"][1] and item["kernel_config"] == c["default"]["kernel_config"]
    order, segs = model._lanes_order(H, W), model._lanes_segments(H, W)
    assert len(segs) == ((W + 3 * (H - 1)) if _is_ar(model) else 2) and sum(segs) == H * W * M_
    cdf, ln, off = model.gaussian_conditional.host_tables()
    sym, idx = c["sym"].cpu().numpy(), c["idx"].cpu().numpy()
    want = []
    for b in range(B):
        sym_s, idx_s = np.ascontiguousarray(sym[b][order]).reshape(-1), np.ascontiguousarray(idx[b][order]).reshape(-1)
        want.append(ans.lanes_pack(ans.lanes_encode(sym_s, idx_s, segs, LANES_W, cdf, ln, off)))
        assert int(np.abs(sym_s).max()) >= 2 and int(idx_s.max()) > int(idx_s.min())   # not a degenerate stream
    assert item["strings"][0] == want
    if _is_ar(model):   # order= is the encoder's schedule of computation only
        assert model.compress(c["x"], order="raster", lanes=LANES_W)["strings"] == item["strings"]
        assert model.compress(c["x"], order="raster")["strings"] == c["default"]["strings"]


@pytest.mark.parametrize("name", list(SHAPES))
def test_x_hat_and_y_hat_from_every_decoder(model, coded, name):
    from clc_amd import ans
    from clc_amd.models import coding

    c = coded[name]
    lanes, default = c["lanes"], c["default"]
    B = c["y"].shape[0]
    want = model._synthesis(c["y_hat"]).clamp(0, 1)
    subs = [ans.lanes_unpack(s) for s in lanes["strings"][0]]
    for device_coder in (True, False):
        y_hat, state = model._decode_lanes(subs, c["params"], device_coder)
        assert torch.equal(y_hat.view(torch.int32), c["y_hat"].contiguous(memory_format=torch.channels_last).view(torch.int32)), device_coder
        coding.lanes_check(state, subs)   # every wave stream ended at (2^31 x 64, its word count)
        for check in (True, False):
            out = model.decompress(lanes["strings"], lanes["shape"], lanes=LANES_W, device_coder=device_coder, check=check)
            assert sorted(out) == ["x_hat"] and torch.equal(out["x_hat"], want), (device_coder, check)
    if _is_ar(model):
        y_default = model._decode_passes(default["strings"][0], c["params"], 1, model._ar_passes, "raster")
    else:
        y_default = model._ckbd_decode(default["strings"][0], c["params"])
    assert torch.equal(y_default, c["y_hat"])
    assert torch.equal(model.decompress(default["strings"], default["shape"])["x_hat"], want)
    st = model._decode_lanes(subs, c["params"], True)[1]
    assert tuple(st.shape) == (B, LANES_W, 130) and st.dtype == torch.int32


def test_counted_device_to_host_copies(dev, model, coded):
    from clc_amd import ans

    c = coded["image"]
    lanes, default = c["lanes"], c["default"]
    hops = 96 if _is_ar(model) else 2   # the default decoder: one per raster pixel of the 8 x 12 latent, or one per pass
    with _count_d2h() as n:
        model.decompress(default["strings"], default["shape"])
    n_default = n.n
    subs = [ans.lanes_unpack(s) for s in lanes["strings"][0]]
    with _count_d2h() as n:
        model._decode_lanes(subs, c["params"], True)
    y_pass = n.n
    with _count_d2h() as n:
        model.decompress(lanes["strings"], lanes["shape"], lanes=LANES_W, check=False)
    unchecked = n.n
    with _count_d2h() as n:
        model.decompress(lanes["strings"], lanes["shape"], lanes=LANES_W, check=True)
    checked = n.n
    with _count_d2h() as n:
        model.decompress(lanes["strings"], lanes["shape"], lanes=LANES_W, device_coder=False, check=False)
    host = n.n
    with _count_d2h() as n:
        model.compress(c["x"])
    enc_default = n.n
    with _count_d2h() as n:
        model.compress(c["x"], lanes=LANES_W)
    enc_lanes = n.n
    print(f"device -> host copies: default decompress {n_default}, y pass on the device {y_pass}, lanes decompress {unchecked} / {checked} with "
          f"the check, on the host coder {host}; compress {enc_default} default, {enc_lanes} lanes")
    assert n_default == hops and y_pass == 0 and unchecked == 0 and checked == 1
    assert host == (33 if _is_ar(model) else 2)   # the host coder of the same format: a hop per wavefront step, or per pass
    assert enc_lanes <= enc_default + 1


def test_batch_independence_container_and_damage(dev, model):
    from clc_amd import codec

    xb = torch.cat((_images(2, 64, 64), _images(1, 64, 64).flip(3)), 0).to(dev)
    xb = xb[[2, 0, 1]].contiguous()
    both, one = model.compress(xb, lanes=LANES_W), model.compress(xb[1:2], lanes=LANES_W)
    assert len(both["strings"][0]) == 3 and len(set(both["strings"][0])) == 3 and tuple(both["shape"]) == (1, 1)
    assert one["strings"][0][0] == both["strings"][0][1] and one["strings"][1][0] == both["strings"][1][1]
    dec_b = model.decompress(both["strings"], both["shape"], lanes=LANES_W)
    dec_1 = model.decompress([[both["strings"][0][1]], [both["strings"][1][1]]], both["shape"], lanes=LANES_W)
    assert torch.equal(dec_1["x_hat"], dec_b["x_hat"][1:2])
    assert torch.equal(dec_b["x_hat"], model.decompress(**{k: model.compress(xb)[k] for k in ("strings", "shape")})["x_hat"])
    # the container carries the string
    blob = codec.pack_item(one, image_hw=(64, 64))
    strings, shape, meta = codec.unpack(blob)
    assert strings[0][0] == one["strings"][0][0] and strings[1][0] == one["strings"][1][0] and tuple(shape) == (1, 1) and meta["image_hw"] == (64, 64)
    assert torch.equal(model.decompress(strings, shape, lanes=LANES_W)["x_hat"], dec_1["x_hat"])
    # a flipped state word (lane 5 of image 1's wave stream 0, a bit of its low word) raises, naming the image — and only that one
    s = bytearray(both["strings"][0][1])
    s[8 + 4 * LANES_W + 8 * 5] ^= 0x10
    bad = [[both["strings"][0][0], bytes(s), both["strings"][0][2]], both["strings"][1]]
    with pytest.raises(ValueError, match=r"image 1: wave streams \[.*\] did not decode to their end") as e:
        model.decompress(bad, both["shape"], lanes=LANES_W)
    assert "image 0" not in str(e.value) and "image 2" not in str(e.value)
    with pytest.raises(ValueError, match=r"image 1: wave streams"):
        model.decompress(bad, both["shape"], lanes=LANES_W, device_coder=False)
    out = model.decompress(bad, both["shape"], lanes=LANES_W, check=False)   # unchecked: some image, the other two untouched
    assert torch.equal(out["x_hat"][0], dec_b["x_hat"][0]) and torch.equal(out["x_hat"][2], dec_b["x_hat"][2])
    # refusals that need the device half
    with pytest.raises(ValueError, match=r"lanes = 3, but the header of image 0 says 2 wave streams"):
        model.decompress(both["strings"], both["shape"], lanes=3)
    with pytest.raises(ValueError, match="is a lanes stream"):
        model.decompress(both["strings"], both["shape"])


def test_the_default_path_does_not_notice(dev, model, coded):
    from clc_amd import codec, lib

    c = coded["image"]
    tag, hsh, cfg = lib.load().clc_kernel_config_tag(), lib.load().clc_kernel_config_hash(), codec.kernel_config()
    before = model.compress(c["x"])
    item = model.compress(c["x"], lanes=4)
    model.decompress(item["strings"], item["shape"], lanes=4)
    after = model.compress(c["x"])
    assert sorted(after) == ["kernel_config", "shape", "strings"]
    assert before["strings"] == after["strings"] == c["default"]["strings"]
    assert after["kernel_config"] == item["kernel_config"] == cfg == codec.kernel_config()
    assert lib.load().clc_kernel_config_tag() == tag == 6 and lib.load().clc_kernel_config_hash() == hsh
