"""The split stream of cheng2020 through the model (clc_amd/models/cheng.py): Cheng2020Attention(24, K = 3) with S = 4 sub-streams, the
weights and images of tests/test_cheng_model_gpu.py.  Every comparison is exact.

One 1x3x128x192 image (latent 8x12): each sub-stream is ans.encode_direct of its share of _gmm_encode's triples; decompress returns
exactly g_s(round(y)).clamp(0, 1) from the device decoder, from the host decoder of the same format and from the default format; the
device pass's y_hat is the encoder's bit for bit; the device path makes NO device -> host copy with check=False and ONE (the final coder
states) with check=True, against W + 3 (H - 1) of the hopping decoders.  A 3x3x64x128 batch: an image's split bytes do not depend on the
batch, decode at batch 1 and survive the container.  A flipped word makes check=True raise, naming the sub-stream (among those it
dragged out of step through the context).  The default compress(x) beside all this keeps its bytes.
"""
import numpy as np
import pytest
import torch

from test_cheng_model_gpu import N_, _count_d2h, _images, _pair

pytestmark = pytest.mark.gpu
S_ = 4


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def coded(dev):
    """the model, one image, the encoder's view of it and both formats' items — computed once, read by every test"""
    from clc_amd import ans

    _, p = _pair("Cheng2020Attention", 3, dev)
    p.eval()
    x = _images(1, 128, 192).to(dev)
    y, params, z_strings, z_size = p._code_inputs(x)
    triples, y_hat = p._gmm_encode(y, params)
    return dict(p=p, x=x, y=y, params=params, z_strings=z_strings, triples=triples.cpu().numpy(), y_hat=y_hat,
                want=p._synthesis(torch.round(y)).clamp(0, 1), split=p.compress(x, substreams=S_), plain=p.compress(x), ans=ans)


def test_split_bytes_and_the_default_beside_them(coded):
    ans, t = coded["ans"], coded["triples"]
    split, plain = coded["split"], coded["plain"]
    assert tuple(t.shape) == (1, 8 * 12, N_, 3)
    assert split["substreams"] == S_ and "substreams" not in plain
    assert split["strings"][1] == plain["strings"][1] == coded["z_strings"] and tuple(split["shape"]) == tuple(plain["shape"]) == (2, 3)
    assert split["kernel_config"] == plain["kernel_config"]
    subs = ans.split_unpack(split["strings"][0][0])
    assert len(split["strings"][0]) == 1 and len(subs) == S_
    for s in range(S_):
        assert subs[s] == ans.encode_direct(np.ascontiguousarray(t[0][:, s::S_]).reshape(-1, 3)), s
    # the default path is untouched: still the one stream of all the triples
    assert plain["strings"][0] == [ans.encode_direct(t[0])]
    extra = len(split["strings"][0][0]) - len(plain["strings"][0][0])
    print(f"split stream: {len(split['strings'][0][0])} bytes, one stream {len(plain['strings'][0][0])}: {extra} more at S = {S_}")
    assert extra <= 8 + 4 * S_ + 8 * (S_ - 1) + 4   # header, S - 1 more final states, one word of rounding


def test_device_decode_is_exact_and_hop_free(coded):
    from clc_amd.models import coding

    p, split, plain = coded["p"], coded["split"], coded["plain"]
    H, W = 8, 12
    counts = {}
    for check in (False, True):
        with _count_d2h() as c:
            dec = p.decompress(split["strings"], split["shape"], substreams=S_, check=check)
        counts[check] = c.n
        assert torch.equal(dec["x_hat"], coded["want"])
    print(f"device decoder: {counts[False]} device -> host copies with check=False, {counts[True]} with check=True")
    assert counts == {False: 0, True: 1}
    # the pass itself: no copy, and the encoder's y_hat bit for bit; every sub-stream at its end
    subs = coding.stream_parse(coded["ans"].SPLIT_STREAM, split["strings"][0], S_, "substreams")
    with _count_d2h() as c:
        y_hat, state = p._gmm_decode_split(subs, coded["params"])
    assert c.n == 0
    assert torch.equal(y_hat, coded["y_hat"]) and torch.equal(y_hat, torch.round(coded["y"]))
    st = state.cpu().numpy().view(np.uint32)
    assert st.shape == (1, S_, 4)
    for s in range(S_):
        assert tuple(int(v) for v in st[0, s]) == (0x80000000, 0, len(subs[0][s]) // 4, 0), s
    # the host decoder of the same format, and the default format
    with _count_d2h() as c:
        host = p.decompress(split["strings"], split["shape"], substreams=S_, device_decoder=False)
    assert c.n == W + 3 * (H - 1)
    assert torch.equal(host["x_hat"], coded["want"])
    y_host, none = p._gmm_decode_split(subs, coded["params"], device_decoder=False)
    assert none is None and torch.equal(y_host, coded["y_hat"])
    assert torch.equal(p.decompress(plain["strings"], plain["shape"])["x_hat"], coded["want"])
    assert torch.equal(p._gmm_decode(plain["strings"][0], coded["params"]), coded["y_hat"])


def test_batch_invariance_and_the_container(coded, dev):
    from clc_amd import codec

    p = coded["p"]
    xb = _images(3, 64, 128).to(dev)
    both, one = p.compress(xb, substreams=S_), p.compress(xb[1:2], substreams=S_)
    assert len(both["strings"][0]) == 3 and tuple(both["shape"]) == (1, 2)
    assert one["strings"][0][0] == both["strings"][0][1] and one["strings"][1][0] == both["strings"][1][1]
    yb = p._code_inputs(xb)[0]
    want = p._synthesis(torch.round(yb)).clamp(0, 1)
    dec_b = p.decompress(both["strings"], both["shape"], substreams=S_)
    dec_1 = p.decompress([[both["strings"][0][1]], [both["strings"][1][1]]], both["shape"], substreams=S_)
    assert torch.equal(dec_b["x_hat"], want)
    assert torch.equal(dec_1["x_hat"], want[1:2])
    assert torch.equal(p.decompress(both["strings"], both["shape"], substreams=S_, device_decoder=False)["x_hat"], want)
    blob = codec.pack_item(one, image_hw=(64, 128))
    strings, shape, meta = codec.unpack(blob)
    assert strings[0][0] == one["strings"][0][0] and strings[1][0] == one["strings"][1][0] and tuple(shape) == (1, 2)
    assert meta["image_hw"] == (64, 128)
    assert torch.equal(p.decompress(strings, shape, substreams=S_)["x_hat"], want[1:2])
    with pytest.raises(ValueError, match="header of image 0 says 4"):
        p.decompress(strings, shape, substreams=2)


def test_a_flipped_word_is_named(coded):
    ans, p, split = coded["ans"], coded["p"], coded["split"]
    subs = ans.split_unpack(split["strings"][0][0])
    w = np.frombuffer(subs[2], dtype="<u4").copy()
    assert w.size > 8
    w[w.size // 2] ^= 0xFFFFFFFF
    bad = ans.split_pack(subs[:2] + [w.tobytes()] + subs[3:])
    # (the wrong symbols enter the context of later pixels, so other sub-streams of the image may leave their end too: all are listed)
    with pytest.raises(ValueError, match=r"image 0: sub-streams \[[^\]]*\b2\b[^\]]*\] did not decode to their end"):
        p.decompress([[bad], split["strings"][1]], split["shape"], substreams=S_)
    out = p.decompress([[bad], split["strings"][1]], split["shape"], substreams=S_, check=False)   # returns, some symbols wrong
    assert out["x_hat"].shape == coded["want"].shape and not torch.equal(out["x_hat"], coded["want"])
    # and the intact string still decodes
    assert torch.equal(p.decompress(split["strings"], split["shape"], substreams=S_)["x_hat"], coded["want"])
