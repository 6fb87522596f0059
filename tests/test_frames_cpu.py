"""The host side of the video path, no GPU: every refusal of clc_amd/frames.py by name (argument checks come before the GPU check,
so CPU tensors reach them), the lanes keyword of ScaleSpaceFlow.compress, the CLV1 sequence container (codec.pack_sequence /
unpack_sequence), the float64 restatement's own identities (tests/frames_ref.py) and psnr_yuv420 on hand-computed sums."""
import math

import pytest
import torch

import frames_ref


def _planes(N=1, H=4, W=6, dtype=torch.uint8):
    return (torch.zeros(N, H, W, dtype=dtype), torch.zeros(N, H // 2, W // 2, dtype=dtype), torch.zeros(N, H // 2, W // 2, dtype=dtype))


def test_refusals_by_name():
    from clc_amd import frames
    from clc_amd.lib import ClcError

    Y, U, V = _planes()
    with pytest.raises(ValueError, match="H and W must be even"):
        frames.yuv420_to_rgb(torch.zeros(1, 5, 6, dtype=torch.uint8), U, V)
    with pytest.raises(ValueError, match="H and W must be even"):
        frames.yuv420_to_rgb(torch.zeros(1, 4, 7, dtype=torch.uint8), U, V)
    with pytest.raises(ValueError, match="H and W must be even"):
        frames.rgb_to_yuv420(torch.zeros(1, 3, 8, 8), (3, 8))
    with pytest.raises(ValueError, match=r"Y is torch.int16; bit_depth=8 planes are torch.uint8"):
        frames.yuv420_to_rgb(Y.to(torch.int16), U, V, bit_depth=8)
    with pytest.raises(ValueError, match=r"V is torch.uint8; bit_depth=10 planes are torch.int16"):
        frames.yuv420_to_rgb(Y.to(torch.int16), U.to(torch.int16), V, bit_depth=10)
    for bits in (7, 17, 8.0, True):
        with pytest.raises(ValueError, match="bit_depth must be an integer 8 .. 16"):
            frames.yuv420_to_rgb(Y, U, V, bit_depth=bits)
        with pytest.raises(ValueError, match="bit_depth must be an integer 8 .. 16"):
            frames.rgb_to_yuv420(torch.zeros(1, 3, 4, 4), bit_depth=bits)
        with pytest.raises(ValueError, match="bit_depth must be an integer 8 .. 16"):
            frames.plane_sse(Y, Y, bit_depth=bits)
        with pytest.raises(ValueError, match="bit_depth must be an integer 8 .. 16"):
            frames.psnr_yuv420(1, 1, 1, 16, bit_depth=bits)
    with pytest.raises(ValueError, match="mode must be 'bilinear' or 'bicubic' .got mode='nearest'"):
        frames.yuv420_to_rgb(Y, U, V, mode="nearest")
    with pytest.raises(ValueError, match="Hp >= H and Wp >= W .got Hp=2, Wp=6 for H=4, W=6"):
        frames.yuv420_to_rgb(Y, U, V, size=(2, 6))
    with pytest.raises(ValueError, match="Hp >= H and Wp >= W"):
        frames.yuv420_to_rgb(Y, U, V, size=(4, 4))
    with pytest.raises(ValueError, match="Hp >= H and Wp >= W"):
        frames.rgb_to_yuv420(torch.zeros(1, 3, 4, 4), (6, 4))
    with pytest.raises(ValueError, match=r"U must be \[N, H/2, W/2\] = \(1, 2, 3\)"):
        frames.yuv420_to_rgb(Y, torch.zeros(1, 2, 2, dtype=torch.uint8), V)
    with pytest.raises(ValueError, match=r"V must be \[N, H/2, W/2\] = \(1, 2, 3\)"):
        frames.yuv420_to_rgb(Y, U, torch.zeros(2, 2, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="rgb must be a .N, 3, Hp, Wp. tensor"):
        frames.rgb_to_yuv420(torch.zeros(1, 4, 4, 4))
    with pytest.raises(ValueError, match="one non-empty shape"):
        frames.plane_sse(Y, torch.zeros(1, 4, 8, dtype=torch.uint8))
    # valid arguments on the CPU: no fallback
    with pytest.raises(ClcError, match="GPU only"):
        frames.yuv420_to_rgb(Y, U, V)
    with pytest.raises(ClcError, match="GPU only"):
        frames.yuv420_to_rgb(*_planes(dtype=torch.int16), bit_depth=10, mode="bicubic", size=(8, 8))
    with pytest.raises(ClcError, match="GPU only"):
        frames.rgb_to_yuv420(torch.zeros(1, 3, 8, 8), (4, 6))
    with pytest.raises(ClcError, match="GPU only"):
        frames.plane_sse(Y, Y)
    with pytest.raises(ValueError, match="frame 1 is not a .Y, U, V. triple"):
        frames.encode_yuv420(None, [(Y, U, V), (Y, U)])
    with pytest.raises(ValueError, match="frames of differing shapes"):
        frames.encode_yuv420(None, [(Y, U, V), _planes(H=6)])
    with pytest.raises(ValueError, match="mode must be"):
        frames.encode_yuv420(None, [(Y, U, V)], mode="lanczos")


def test_lanes_keyword_is_checked_before_the_gpu_check():
    from clc_amd import models

    m = models.ScaleSpaceFlow(mid_planes=8, planes=8)
    frames = [torch.zeros(1, 3, 128, 128)]   # CPU tensors: the GPU check would refuse them
    for lanes in (0, 17):
        with pytest.raises(ValueError, match=rf"ScaleSpaceFlow.compress.*{lanes}"):
            m.compress(frames, lanes=lanes)
        with pytest.raises(ValueError, match=rf"ScaleSpaceFlow.decompress.*{lanes}"):
            m.decompress([[[b""], [b""]]], [(1, 1)], lanes=lanes)
        with pytest.raises(ValueError, match=rf"Hyperprior.compress.*{lanes}"):
            m.img_hyperprior.compress(torch.zeros(1, 8, 8, 8), lanes=lanes)


def _strings(F, B, seed=0):
    g = torch.Generator().manual_seed(seed)
    blob = lambda: bytes(torch.randint(0, 256, (int(torch.randint(0, 40, (1,), generator=g)),), generator=g, dtype=torch.uint8).tolist())
    pair = lambda: [[blob() for _ in range(B)], [blob() for _ in range(B)]]
    strings = [pair()] + [{"motion": pair(), "residual": pair()} for _ in range(F - 1)]
    shapes = [torch.Size([1, 2])] + [{"motion": torch.Size([1, 2]), "residual": torch.Size([1, 2])} for _ in range(F - 1)]
    return strings, shapes


@pytest.mark.parametrize("F,B", [(1, 1), (3, 1), (1, 2), (3, 2)])
def test_sequence_container_round_trip(F, B):
    from clc_amd import codec

    strings, shapes = _strings(F, B, seed=10 * F + B)
    for lanes, bits in ((None, None), (4, 8), (16, 10)):
        blob = codec.pack_sequence(strings, shapes, lanes=lanes, image_hw=(120, 136), bit_depth=bits)
        assert blob[:4] == b"CLV1"
        got_s, got_h, meta = codec.unpack_sequence(blob)
        assert got_s == strings and got_h == shapes
        assert (meta["frames"], meta["batch"], meta["image_hw"], meta["padded_hw"], meta["lanes"], meta["bit_depth"]) == (F, B, (120, 136), (128, 256), lanes, bits)
        assert meta["same_kernel_config"] and (meta["kernel_config_tag"], meta["kernel_config_hash"]) == codec.kernel_config()
        assert codec.pack_sequence(got_s, got_h, lanes=meta["lanes"], image_hw=meta["image_hw"], bit_depth=meta["bit_depth"]) == blob
        # per frame 2 (keyframe) or 4 string lists of B length-prefixed strings after the 24-byte header
        payload = sum(len(s) + 4 for t, fs in enumerate(strings) for group in codec._sequence_groups(t, fs) for s in group)
        assert len(blob) == 24 + payload


def test_sequence_container_refusals():
    from clc_amd import codec

    strings, shapes = _strings(3, 2)
    blob = codec.pack_sequence(strings, shapes, lanes=4, image_hw=(128, 200), bit_depth=8)
    with pytest.raises(ValueError, match="wrong magic"):
        codec.unpack_sequence(b"CLC1" + blob[4:])
    with pytest.raises(ValueError, match="wrong magic"):
        codec.unpack_sequence(b"CL")
    with pytest.raises(ValueError, match="unsupported version 2"):
        codec.unpack_sequence(blob[:4] + b"\x02" + blob[5:])
    with pytest.raises(ValueError, match="cut short"):
        codec.unpack_sequence(blob[:20])
    with pytest.raises(ValueError, match="cut short inside frame 2"):
        codec.unpack_sequence(blob[:-1])
    with pytest.raises(ValueError, match="cut short inside frame 0"):
        codec.unpack_sequence(blob[:26])
    with pytest.raises(ValueError, match="1 trailing bytes"):
        codec.unpack_sequence(blob + b"\0")
    two = codec.pack_sequence(strings[:2], shapes[:2], lanes=4, image_hw=(128, 200), bit_depth=8)
    claims_three = two[:12] + (3).to_bytes(2, "little") + two[14:]   # the frame count field: bytes 12 .. 13
    assert codec.unpack_sequence(two)[2]["frames"] == 2
    with pytest.raises(ValueError, match="frame count 3 disagrees with the strings: the blob ends after 2 whole frames"):
        codec.unpack_sequence(claims_three)
    with pytest.raises(ValueError, match="frame count"):
        codec.pack_sequence(strings, shapes[:2], lanes=4, image_hw=(128, 200))
    with pytest.raises(ValueError, match="does not fit the coded size"):
        codec.pack_sequence(strings, shapes, lanes=4, image_hw=(129, 200))
    with pytest.raises(ValueError, match="pack_sequence.*17"):
        codec.pack_sequence(strings, shapes, lanes=17, image_hw=(128, 200))
    with pytest.raises(ValueError, match="bit_depth must be 8 .. 16 or None"):
        codec.pack_sequence(strings, shapes, lanes=4, image_hw=(128, 200), bit_depth=7)
    short = [strings[0], {"motion": strings[1]["motion"], "residual": [strings[1]["residual"][0][:1], strings[1]["residual"][1]]}]
    with pytest.raises(ValueError, match="frame 1, string list 2 holds 1 strings"):
        codec.pack_sequence(short, shapes[:2], lanes=4, image_hw=(128, 200))
    other = bytearray(blob)
    other[8] ^= 0xFF   # the kernel-config hash: another kernel state's blob
    with pytest.raises(codec.KernelConfigMismatch):
        codec.unpack_sequence(bytes(other))
    assert codec.unpack_sequence(bytes(other), strict=False)[2]["same_kernel_config"] is False


def test_restatement_identities():
    g = torch.Generator().manual_seed(3)
    x = torch.rand((2, 3, 6, 10), generator=g, dtype=torch.float64) * 1.6 - 0.3
    assert (frames_ref.ycbcr2rgb(frames_ref.rgb2ycbcr(x)) - x).abs().max().item() <= 1e-15
    grey = torch.full((1, 3, 2, 2), 0.25, dtype=torch.float64)
    assert (frames_ref.rgb2ycbcr(grey)[:, 1:] - 0.5).abs().max().item() <= 1e-16   # neutral chroma is 0.5: x 255 the tie at 127.5
    # constant chroma survives up-then-down sampling exactly, in both modes and at both depths
    for bits, dtype, (u, v) in ((8, torch.uint8, (90, 201)), (10, torch.int16, (300, 801))):
        Y = torch.randint(0, 2 ** bits, (1, 6, 10), generator=g).to(dtype)
        U, V = torch.full((1, 3, 5), u, dtype=dtype), torch.full((1, 3, 5), v, dtype=dtype)
        for mode in ("bilinear", "bicubic"):
            ycc = frames_ref.rgb2ycbcr(frames_ref.yuv420_to_rgb(Y, U, V, bits, mode))
            c = torch.nn.functional.avg_pool2d(ycc[:, 1:], 2) * (2 ** bits - 1)
            assert (c[:, 0] - u).abs().max().item() <= 1e-10 and (c[:, 1] - v).abs().max().item() <= 1e-10
    # the 16-bit container: -1 as an int16 is the sample 65535
    assert frames_ref.samples(torch.tensor([-1, 0, 1023], dtype=torch.int16)).tolist() == [65535.0, 0.0, 1023.0]
    assert frames_ref.quantise(torch.tensor([0.5, 1.5, 2.5, -3.0, 300.0], dtype=torch.float64), 8).tolist() == [0, 2, 2, 0, 255]


def test_psnr_from_hand_computed_sums():
    from clc_amd import frames

    # 8 bits, 16 luma samples: sse 16 -> mse 1 -> 20 log10(255); chroma planes of 4 samples: sse 16 -> mse 4; sse 1 -> mse 1/4
    got = frames.psnr_yuv420(16, 16, 1, 16, bit_depth=8)
    y, u, v = 20 * math.log10(255), 10 * math.log10(255 ** 2 / 4), 10 * math.log10(255 ** 2 * 4)
    assert got == {"psnr_y": pytest.approx(y, abs=1e-12), "psnr_u": pytest.approx(u, abs=1e-12), "psnr_v": pytest.approx(v, abs=1e-12),
                   "psnr_yuv": pytest.approx((4 * y + u + v) / 6, abs=1e-12)}
    ten = frames.psnr_yuv420(4 * 1023 ** 2, 1, 1, 4, bit_depth=10)   # every luma sample off by the whole range: 0 dB
    assert ten["psnr_y"] == pytest.approx(0.0, abs=1e-12) and ten["psnr_u"] == pytest.approx(20 * math.log10(1023), abs=1e-12)
    same = frames.psnr_yuv420(0, 0, 0, 64)
    assert same["psnr_y"] == math.inf and same["psnr_yuv"] == math.inf
    big = frames.psnr_yuv420(2 ** 40 * 65535 ** 2, 1, 1, 2 ** 40, bit_depth=16)   # sums beyond 2^53 stay exact as Python integers
    assert big["psnr_y"] == pytest.approx(0.0, abs=1e-9)
    with pytest.raises(ValueError, match="n_y must be a positive multiple of 4"):
        frames.psnr_yuv420(1, 1, 1, 6)
