"""The lanes stream of ssf2020 (clc_amd/models/video.py) at mid_planes = planes = 8 on the three seeded 128x128 frames of
tests/test_ssf_model_gpu.py — every y is 8x8x8 = 512 symbols, 8 chunks of 64: at W = 16 half the wave streams have no round.

Hyperprior level: the device decoder, the host decoder of the same format and the encoder's y_hat agree bit for bit, the symbols are
the default stream's, the tail escape round-trips, and ``out=`` writes a channel slice in place.  Model level: decompress(compress)
equals the eval forward and the default format's reconstruction bit for bit, a sequence's strings do not depend on the batch, the
device -> host copies are counted (2 F - 1 by default, 0 on the lanes stream, exactly 1 with the end check), a flipped word of
the last frame's residual stream is named by frame, the two formats refuse each other's strings, and YUV 4:2:0 planes go through
encode_yuv420 / decode_yuv420 with the metrics of the float64 restatement.
"""
import numpy as np
import pytest
import torch

import frames_ref
from test_cheng_model_gpu import _count_d2h
from test_ssf_model_gpu import FRAMES, MID, PLANES, _frames, _restatement

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev):
    from clc_amd import models

    p = models.ScaleSpaceFlow(mid_planes=MID, planes=PLANES)
    p.load_state_dict(_restatement().state_dict())
    p = p.to(dev).eval()
    p.update(force=True)
    return p


def _two_sequences(dev):
    frames = [f.to(dev) for f in _frames(batch=2)]
    return [torch.cat((f[:1], f[1:].flip(-1)), 0) for f in frames]


@pytest.fixture(scope="module")
def latent(dev, model):
    """a [2, 8, 8, 8] latent of two different images"""
    with torch.no_grad():
        y = model.img_encoder(_two_sequences(dev)[0].contiguous(memory_format=torch.channels_last))
    assert tuple(y.shape) == (2, PLANES, 8, 8)
    return y


def _host_symbols(hp, item, lanes):
    """the symbols of an item's y strings by the HOST coders, [B, C, H, W]: the default stream in its NCHW order, the lanes stream in NHWC"""
    from clc_amd import ans

    gc = hp.gaussian_conditional
    cdf, ln, off = gc.host_tables()
    z_hat = hp.entropy_bottleneck.decompress(item["strings"][1], item["shape"])
    idx = gc.build_indexes(hp.hyper_decoder_scale(z_hat)).contiguous().cpu().numpy()
    out = np.empty(idx.shape, dtype=np.int32)
    for i, s in enumerate(item["strings"][0]):
        if lanes is None:
            out[i] = ans.decode(s, idx[i].reshape(-1), cdf, ln, off).reshape(idx.shape[1:])
        else:
            d = ans.LanesDecoder(ans.lanes_unpack(s))
            out[i] = d.decode(np.ascontiguousarray(idx[i].transpose(1, 2, 0)).reshape(-1), cdf, ln, off).reshape(idx.shape[2], idx.shape[3], -1).transpose(2, 0, 1)
            assert d.at_end()
    return out, idx


@pytest.mark.parametrize("W", [1, 4, 16])
def test_hyperprior_lanes_round_trip(dev, model, latent, W):
    from clc_amd import ans

    hp = model.img_hyperprior
    y_hat0, item0 = hp.compress(latent)
    y_hat, item = hp.compress(latent, lanes=W)
    assert torch.equal(y_hat, y_hat0) and item["strings"][1] == item0["strings"][1] and tuple(item["shape"]) == (1, 1)
    for s in item["strings"][0]:
        assert s[:4] == ans.LANES_MAGIC and len(ans.lanes_unpack(s)) == W
    on_device = hp.decompress(item["strings"], item["shape"], lanes=W)
    on_host = hp.decompress(item["strings"], item["shape"], lanes=W, device_coder=False)
    assert torch.equal(on_device, on_host) and torch.equal(on_device, y_hat)
    assert torch.equal(hp.decompress(item0["strings"], item0["shape"]), y_hat)
    sym, _ = _host_symbols(hp, item, W)
    sym0, _ = _host_symbols(hp, item0, None)
    assert np.array_equal(sym, sym0) and all(np.count_nonzero(s) >= 8 for s in sym)   # (not the all-zero latent)
    if W == 16:   # 512 symbols are 8 chunks: wave streams 8 .. 15 hold their 64 initial states and nothing else
        assert [len(s) for s in ans.lanes_unpack(item["strings"][0][0])[8:]] == [512] * 8


@pytest.mark.parametrize("W", [1, 4, 16])
def test_hyperprior_lanes_tail_escape(dev, model, latent, W):
    hp = model.img_hyperprior
    big = (latent * 60.0).contiguous(memory_format=torch.channels_last)
    y_hat, item = hp.compress(big, lanes=W)
    sym, idx = _host_symbols(hp, item, W)
    _, ln, off = hp.gaussian_conditional.host_tables()
    v = sym - off[idx]
    outside = (v < 0) | (v >= ln[idx] - 2)   # not a symbol of the row's table: coded through the tail escape
    per_image = outside.reshape(outside.shape[0], -1).sum(axis=1)
    print(f"W = {W}: symbols outside their row per image {per_image.tolist()} of {outside[0].size}, largest |symbol| {int(np.abs(sym).max())}")
    assert (per_image >= 1).all()
    on_device = hp.decompress(item["strings"], item["shape"], lanes=W)
    assert torch.equal(on_device, y_hat) and torch.equal(hp.decompress(item["strings"], item["shape"], lanes=W, device_coder=False), y_hat)
    assert torch.equal(hp.decompress(hp.compress(big)[1]["strings"], item["shape"]), y_hat)


@pytest.mark.parametrize("device_coder", [True, False])
def test_hyperprior_out_writes_the_channel_slice(dev, model, latent, device_coder):
    hp = model.img_hyperprior
    other = (latent.flip(0) * 0.5).contiguous(memory_format=torch.channels_last)
    (a_hat, a), (b_hat, b) = hp.compress(latent, lanes=4), hp.compress(other, lanes=4)
    assert not torch.equal(a_hat, b_hat)
    both = torch.full((2, 2 * PLANES, 8, 8), float("nan"), device=dev).contiguous(memory_format=torch.channels_last)
    got_a = hp.decompress(a["strings"], a["shape"], lanes=4, device_coder=device_coder, out=both[:, :PLANES])
    got_b = hp.decompress(b["strings"], b["shape"], lanes=4, device_coder=device_coder, out=both[:, PLANES:])
    assert got_a.data_ptr() == both.data_ptr() and got_b.data_ptr() == both[:, PLANES:].data_ptr()
    sep = torch.cat((hp.decompress(a["strings"], a["shape"], lanes=4), hp.decompress(b["strings"], b["shape"], lanes=4)), dim=1)
    assert torch.equal(both, sep) and torch.equal(sep, torch.cat((a_hat, b_hat), dim=1))


@pytest.fixture(scope="module")
def coded(dev, model):
    """the two sequences coded at batch 2 in both formats, the eval forward, and the default reconstruction"""
    frames = _two_sequences(dev)
    with torch.no_grad():
        fwd = model(frames)["x_hat"]
    default = model.compress(frames)
    lanes = model.compress(frames, lanes=4)
    return frames, fwd, default, lanes, model.decompress(*default)


def test_model_round_trip_equals_forward_and_default(dev, model, coded):
    frames, fwd, default, (strings, shapes), dec_default = coded
    assert len(strings) == FRAMES and sorted(strings[1]) == ["motion", "residual"]
    dec = model.decompress(strings, shapes, lanes=4)
    host = model.decompress(strings, shapes, lanes=4, device_coder=False)
    for t in range(FRAMES):
        assert torch.equal(dec[t], fwd[t]), f"frame {t}"
        assert torch.equal(dec[t], dec_default[t]) and torch.equal(host[t], dec[t]), f"frame {t}"
    assert float((dec[1] - dec[0]).abs().max()) > 0 and not torch.equal(dec[2][0], dec[2][1])
    # z stays the default stream, byte for byte
    assert strings[0][1] == default[0][0][1] and strings[2]["residual"][1] == default[0][2]["residual"][1]
    # a sequence coded at batch 2 decodes image by image at batch 1, with the same bytes per image
    for i in range(2):
        one_s, one_h = model.compress([f[i:i + 1] for f in frames], lanes=4)
        assert one_s[0][0][0] == strings[0][0][i] and one_s[0][1][0] == strings[0][1][i]
        for t in range(1, FRAMES):
            for k in ("motion", "residual"):
                assert one_s[t][k][0][0] == strings[t][k][0][i] and one_s[t][k][1][0] == strings[t][k][1][i], (i, t, k)
        pick = lambda pair: [[pair[0][i]], [pair[1][i]]]
        sliced = [pick(strings[0])] + [{k: pick(strings[t][k]) for k in ("motion", "residual")} for t in range(1, FRAMES)]
        alone = model.decompress(sliced, shapes, lanes=4)
        for t in range(FRAMES):
            assert torch.equal(alone[t], dec[t][i:i + 1]), (i, t)
    # other widths of the stream decode to the same frames
    for W in (1, 16):
        again = model.decompress(*model.compress(frames, lanes=W), lanes=W)
        assert all(torch.equal(a, b) for a, b in zip(again, dec))


def test_counted_device_to_host_copies(dev, model, coded):
    frames, fwd, default, lanes, _ = coded
    model.decompress(*lanes, lanes=4)   # (every host table is cached by now: compress and the default decompress made them)
    with _count_d2h() as c:
        model.decompress(*default)
    n_default = c.n
    with _count_d2h() as c:
        model.decompress(*lanes, lanes=4, check=False)
    unchecked = c.n
    with _count_d2h() as c:
        model.decompress(*lanes, lanes=4, check=True)
    checked = c.n
    print(f"device -> host copies of decompress, {FRAMES} frames: default {n_default}, lanes {unchecked}, lanes with the end check {checked}")
    assert n_default == 2 * FRAMES - 1 and unchecked == 0 and checked == 1


def test_damage_is_named_by_frame(dev, model, coded):
    from clc_amd import ans

    frames, fwd, default, (strings, shapes), _ = coded
    streams = [bytearray(s) for s in ans.lanes_unpack(strings[-1]["residual"][0][0])]
    word = np.frombuffer(streams[1], dtype="<u4").copy()
    word[2 * 5] ^= 0x10          # one word of wave stream 1: the low word of lane 5's state
    streams[1] = word.tobytes()
    bad_y = [ans.lanes_pack([bytes(s) for s in streams]), strings[-1]["residual"][0][1]]
    bad = list(strings[:-1]) + [{"motion": strings[-1]["motion"], "residual": [bad_y, strings[-1]["residual"][1]]}]
    with pytest.raises(ValueError, match=rf"frame {FRAMES - 1}, residual latent: .*image 0: wave streams \[.*1.*\] did not decode to their end") as e:
        model.decompress(bad, shapes, lanes=4)
    assert "image 1" not in str(e.value) and "motion" not in str(e.value)
    with pytest.raises(ValueError, match=rf"frame {FRAMES - 1}, residual latent"):
        model.decompress(bad, shapes, lanes=4, device_coder=False)
    out = model.decompress(bad, shapes, lanes=4, check=False)   # damaged data decodes to SOME symbols: finite frames, the earlier ones intact
    good = model.decompress(strings, shapes, lanes=4)
    assert all(bool(torch.isfinite(x).all()) for x in out)
    assert all(torch.equal(a, b) for a, b in zip(out[:-1], good[:-1])) and torch.equal(out[-1][1], good[-1][1])


def test_cross_format_refusals(dev, model, coded):
    frames, fwd, default, lanes, _ = coded
    with pytest.raises(ValueError, match="is a lanes stream"):
        model.decompress(*lanes)
    with pytest.raises(ValueError, match=r"frame 0, keyframe latent: .*bad magic"):
        model.decompress(*default, lanes=4)
    with pytest.raises(ValueError, match=r"frame 0, keyframe latent: .*lanes = 16, but the header of image 0 says 4 wave streams"):
        model.decompress(*lanes, lanes=16)
    mixed = [lanes[0][0], default[0][1], lanes[0][2]]
    with pytest.raises(ValueError, match=r"frame 1, motion latent: .*bad magic"):
        model.decompress(mixed, lanes[1], lanes=4)
    hp = model.img_hyperprior
    with pytest.raises(ValueError, match="is a lanes stream"):
        hp.decompress(lanes[0][0], lanes[1][0])
    with pytest.raises(ValueError, match="bad magic"):
        hp.decompress(default[0][0], default[1][0], lanes=4)


def test_yuv420_end_to_end(dev, model):
    """three 8-bit frames of true size 120 x 136 -> padded to 128 x 256 inside encode_yuv420 -> planes of the true size back"""
    from clc_amd import codec, frames

    H, W = 120, 136
    rgb = [torch.nn.functional.interpolate(f, size=(H, W), mode="bilinear", align_corners=False).clamp(0, 1) for f in _frames()]
    planes = [tuple(frames_ref.quantise(v, 8).to(torch.uint8).to(dev) for v in frames_ref.rgb_to_yuv420_values(x, (H, W), 8)) for x in rgb]
    blob = frames.encode_yuv420(model, planes, bit_depth=8, lanes=4)
    strings, shapes, meta = codec.unpack_sequence(blob)
    assert (meta["frames"], meta["batch"], meta["image_hw"], meta["padded_hw"], meta["lanes"], meta["bit_depth"]) == (3, 1, (H, W), (128, 256), 4, 8)
    assert codec.pack_sequence(strings, shapes, lanes=meta["lanes"], image_hw=meta["image_hw"], bit_depth=meta["bit_depth"]) == blob
    dec = frames.decode_yuv420(model, blob)
    assert len(dec) == 3
    for Y, U, V in dec:
        assert Y.dtype == torch.uint8 and tuple(Y.shape) == (1, H, W) and tuple(U.shape) == (1, H // 2, W // 2) and tuple(V.shape) == (1, H // 2, W // 2)
    # the planes are what the pieces give: pad inside yuv420_to_rgb, the model, crop and quantise inside rgb_to_yuv420
    padded = [frames.yuv420_to_rgb(*p, size=(128, 256)) for p in planes]
    recs = model.decompress(*model.compress(padded, lanes=4), lanes=4)
    for got, x in zip(dec, recs):
        for a, b in zip(got, frames.rgb_to_yuv420(x, (H, W))):
            assert torch.equal(a, b)
    m = frames.sequence_metrics(planes, dec, 8, blob=blob)
    assert m["bpp"] == 8.0 * len(blob) / (3 * H * W)
    host = lambda seq: [tuple(p.cpu() for p in f) for f in seq]
    for t, (pa, pb) in enumerate(zip(host(planes), host(dec))):
        for k, name in enumerate(("psnr_y", "psnr_u", "psnr_v")):
            assert abs(m["frames"][t][name] - frames_ref.psnr(pa[k], pb[k], 8)) <= 1e-9, (t, name)
        assert abs(m["frames"][t]["psnr_yuv"] - frames_ref.psnr_yuv(pa, pb, 8)) <= 1e-9, t
    assert abs(m["mean"]["psnr_yuv"] - sum(frames_ref.psnr_yuv(a, b, 8) for a, b in zip(host(planes), host(dec))) / 3) <= 1e-9
    print(f"3 frames of {H}x{W}: {len(blob)} bytes, {m['bpp']:.4f} bpp, PSNR-YUV {m['mean']['psnr_yuv']:.3f} dB")
    assert np.isfinite(m["mean"]["psnr_yuv"])
    # the default format through the same calls
    blob0 = frames.encode_yuv420(model, planes, bit_depth=8, lanes=None)
    assert codec.unpack_sequence(blob0)[2]["lanes"] is None
    for a, b in zip(frames.decode_yuv420(model, blob0), dec):
        assert all(torch.equal(p, q) for p, q in zip(a, b))
