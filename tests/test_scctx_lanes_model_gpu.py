"""elic2022 on the lanes stream (Elic2022.compress(x, lanes=W) / decompress(..., lanes=W)): models.Elic2022 at scctx_ref.SMALL on a
1x3x128x192 image (latent 8x12) with lanes = 2, the weights of scctx_ref.small_reference().  Every comparison is exact.

The device-encoded strings are ans.lanes_pack(ans.lanes_encode(...)) of the encoder's symbols; decompress returns the same x_hat, and
the same y_hat bit for bit, from the device decoder, from the host decoder of the same format and from the default format; the device
path's device -> host copies are counted; an image's string does not depend on the batch around it; the container carries it; a flipped
state word raises, naming the image; the default path's bytes and the kernel_config tag do not notice any of it.
"""
import numpy as np
import pytest
import torch

import scctx_ref
from test_ar_model_gpu import _images
from test_cheng_model_gpu import _count_d2h

pytestmark = pytest.mark.gpu

SMALL = scctx_ref.SMALL
LANES_W = 2


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev):
    from clc_amd import models

    p = models.Elic2022(**SMALL)
    p.load_state_dict(scctx_ref.small_reference().state_dict())
    p = p.to(dev).eval()
    p.update(force=True)
    return p


@pytest.fixture(scope="module")
def coded(dev, model):
    """one 128x192 image: the encoder's tensors, the default item and the lanes item, computed once"""
    x = _images(1, 128, 192).to(dev)
    y, params, z_strings, z_size = model._code_inputs(x)
    syms, idxs, y_hat = model._scctx_encode(y, params)
    return dict(x=x, y=y, params=params, syms=syms, idxs=idxs, y_hat=y_hat, default=model.compress(x), lanes=model.compress(x, lanes=LANES_W))


def _stream_order(model, coded, b=0):
    from clc_amd.models import scctx_order

    _, _, H, W = coded["y"].shape
    order = scctx_order(H, W, model.groups)
    sym, idx = torch.cat(coded["syms"], 2)[b].cpu().numpy(), torch.cat(coded["idxs"], 2)[b].cpu().numpy()
    return np.ascontiguousarray(sym[order[:, 0], order[:, 1]]), np.ascontiguousarray(idx[order[:, 0], order[:, 1]])


def test_bytes_are_the_host_encoder_s(model, coded):
    from clc_amd import ans

    assert tuple(coded["y"].shape) == (1, SMALL["M"], 8, 12)
    item = coded["lanes"]
    assert sorted(item) == ["kernel_config", "lanes", "shape", "strings"] and item["lanes"] == LANES_W
    assert item["strings"][1] == coded["default"]["strings"][1] and item["kernel_config"] == coded["default"]["kernel_config"]
    sym_s, idx_s = _stream_order(model, coded)
    segs = model._lanes_segments(8, 12)
    assert segs == [48 * c for c in SMALL["groups"] for _ in range(2)] and sum(segs) == sym_s.size
    cdf, ln, off = model.gaussian_conditional.host_tables()
    assert item["strings"][0] == [ans.lanes_pack(ans.lanes_encode(sym_s, idx_s, segs, LANES_W, cdf, ln, off))]
    assert int(np.abs(sym_s).max()) >= 2 and int(idx_s.max()) > int(idx_s.min())   # not a degenerate stream
    extra = len(item["strings"][0][0]) - len(coded["default"]["strings"][0][0])
    print(f"lanes string {len(item['strings'][0][0])} bytes, the default's {len(coded['default']['strings'][0][0])}: + {extra}")
    assert extra <= 8 + 4 * LANES_W + 64 * LANES_W * 12


def test_x_hat_and_y_hat_from_every_decoder(model, coded):
    from clc_amd import ans
    from clc_amd.models import coding

    lanes, default = coded["lanes"], coded["default"]
    want = model._synthesis(coded["y_hat"]).clamp(0, 1)
    subs = [ans.lanes_unpack(s) for s in lanes["strings"][0]]
    for device_coder in (True, False):
        y_hat, state = model._scctx_decode_lanes(subs, coded["params"], device_coder)
        assert torch.equal(y_hat, coded["y_hat"]), device_coder
        coding.lanes_check(state, subs)   # every wave stream ended at (2^31 x 64, its word count)
        for check in (True, False):
            out = model.decompress(lanes["strings"], lanes["shape"], lanes=LANES_W, device_coder=device_coder, check=check)
            assert sorted(out) == ["x_hat"] and torch.equal(out["x_hat"], want), (device_coder, check)
    assert torch.equal(model._scctx_decode(default["strings"][0], coded["params"]), coded["y_hat"])
    assert torch.equal(model.decompress(default["strings"], default["shape"])["x_hat"], want)
    st = model._scctx_decode_lanes(subs, coded["params"], True)[1]
    assert tuple(st.shape) == (1, LANES_W, 130) and st.dtype == torch.int32


def test_counted_device_to_host_copies(dev, model, coded):
    from clc_amd import ans

    lanes, default = coded["lanes"], coded["default"]
    passes = 2 * len(SMALL["groups"])   # 8x12: every pass has pixels
    with _count_d2h() as c:
        model.decompress(default["strings"], default["shape"])
    n_default = c.n
    E = n_default - passes
    subs = [ans.lanes_unpack(s) for s in lanes["strings"][0]]
    with _count_d2h() as c:
        model._scctx_decode_lanes(subs, coded["params"], True)
    y_pass = c.n
    with _count_d2h() as c:
        model.decompress(lanes["strings"], lanes["shape"], lanes=LANES_W, check=False)
    unchecked = c.n
    with _count_d2h() as c:
        model.decompress(lanes["strings"], lanes["shape"], lanes=LANES_W, check=True)
    checked = c.n
    with _count_d2h() as c:
        model.decompress(lanes["strings"], lanes["shape"], lanes=LANES_W, device_coder=False)
    host = c.n
    with _count_d2h() as c:
        model.compress(coded["x"])
    enc_default = c.n
    with _count_d2h() as c:
        model.compress(coded["x"], lanes=LANES_W)
    enc_lanes = c.n
    print(f"device -> host copies: default decompress {n_default} (E = {E}), y pass on the device {y_pass}, lanes decompress {unchecked} / "
          f"{checked} with the check, on the host coder {host}; compress {enc_default} default, {enc_lanes} lanes")
    assert E >= 0 and y_pass == 0 and unchecked == E and checked == E + 1 and host == n_default
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

    tag, hsh, cfg = lib.load().clc_kernel_config_tag(), lib.load().clc_kernel_config_hash(), codec.kernel_config()
    before = model.compress(coded["x"])
    item = model.compress(coded["x"], lanes=4)
    model.decompress(item["strings"], item["shape"], lanes=4)
    after = model.compress(coded["x"])
    assert sorted(after) == ["kernel_config", "shape", "strings"]
    assert before["strings"] == after["strings"] == coded["default"]["strings"]
    assert after["kernel_config"] == item["kernel_config"] == cfg == codec.kernel_config()
    assert lib.load().clc_kernel_config_tag() == tag == 6 and lib.load().clc_kernel_config_hash() == hsh
