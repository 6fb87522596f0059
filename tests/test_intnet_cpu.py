"""The integer hyper-synthesis net without a GPU: the reference's own arithmetic (tests/intnet_ref.py) against torch in
float64, the requantiser at its edges against Python's unbounded integers, the conversion (clc_amd.intnet.convert must give the
reference's integers), a per-layer error bound that needs no measured number, the hash, container version 4, and every refusal that
happens before the GPU check."""
import struct

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import intnet_ref as R
from clc_amd import codec
from clc_amd import intnet as P
from clc_amd import lib as L


# ---- the reference's convolutions ----
@pytest.mark.parametrize("b,h,w", [(1, 1, 1), (1, 3, 5), (2, 5, 4), (1, 2, 7)], ids=["1x1", "3x5", "b2-5x4", "2x7"])
def test_reference_convolutions_equal_torch_in_float64(b, h, w):
    """integer-valued data in float64 is exact below 2^53: no tolerance"""
    rng = np.random.default_rng(h * 10 + w)
    x = rng.integers(-128, 128, (b, h, w, 32)).astype(np.int8)
    xt = torch.from_numpy(x).double().permute(0, 3, 1, 2)
    wt = rng.integers(-127, 128, (32, 64, 5, 5)).astype(np.int8)
    want = F.conv_transpose2d(xt, torch.from_numpy(wt).double(), stride=2, padding=2, output_padding=1).permute(0, 2, 3, 1).numpy()
    assert np.array_equal(R.deconv5_acc(x, wt), want.astype(np.int64))
    wc = rng.integers(-127, 128, (64, 32, 3, 3)).astype(np.int8)
    want = F.conv2d(xt, torch.from_numpy(wc).double(), padding=1).permute(0, 2, 3, 1).numpy()
    assert np.array_equal(R.conv3_acc(x, wc), want.astype(np.int64))


# ---- the requantiser ----
def _requant_big(a, mp, mn, s):
    m = mp if a >= 0 else mn
    return (a * m + (1 << (s - 1))) >> s   # Python integers: unbounded, >> floors


def test_requantiser_at_its_edges():
    big = (1 << 31) - 1
    cases = []
    for s in (1, 2, 31, 62):
        for mp, mn in ((1 << 30, 0), (1 << 30, 1 << 23), (1 << 30, 1 << 30), (big, big), (3, 1), (1, 1)):
            for a in (0, 1, -1, 2, -2, 3, -3, 5, -5, 127, -128, big, -big, (1 << 30) + 1, -(1 << 30) - 1):
                cases.append((a, mp, mn, s))
    acc = np.array([c[0] for c in cases], dtype=np.int64)
    got = R.requant(acc, 0, np.array([c[1] for c in cases]), np.array([c[2] for c in cases]), np.array([c[3] for c in cases]))
    assert got.tolist() == [_requant_big(*c) for c in cases]
    # ties of both signs round half up: 1/2 -> 1, -1/2 -> 0, 3/2 -> 2, -3/2 -> -1
    assert R.requant(np.array([1, -1, 3, -3]), 0, 1 << 30, 1 << 30, 31).tolist() == [1, 0, 2, -1]
    assert R.requant(np.array([1, -1, 3, -3]), 0, 1, 1, 1).tolist() == [1, 0, 2, -1]          # shift 1
    assert R.requant(np.array([big, -big]), 0, big, big, 62).tolist() == [1, -1]              # shift 62: (2^31 - 1)^2 / 2^62 rounds to 1
    assert R.requant(np.array([-5]), 0, 1 << 30, 0, 31).tolist() == [0]                       # ReLU
    # the clamps of both output kinds, through a 1x1 map whose centre tap is the only live one
    x = np.zeros((1, 1, 1, 32), np.int8)
    x[..., 0] = 1
    w = np.zeros((4, 32, 3, 3), np.int8)
    w[:, 0, 1, 1] = 1
    layer = {"w": w, "bias": np.array([1000, -1000, 126, 40000], np.int32) - 1, "mult_pos": np.full(4, 1 << 30, np.int32),
             "mult_neg": np.full(4, 1 << 30, np.int32), "shift": np.full(4, 30, np.int32)}
    assert R.layer_int8(x, layer, False).reshape(-1).tolist() == [127, -128, 126, 127]
    assert (R.layer_f32(x, layer, False, 8).reshape(-1) * 256).tolist() == [1000.0, -1000.0, 126.0, 32767.0]
    layer["bias"] = np.array([-40000, 0, 0, 0], np.int32)
    assert (R.layer_f32(x, layer, False, 8).reshape(-1) * 256).tolist()[0] == -32768.0


def test_overflow_bound_for_the_largest_served_shape():
    """25 taps x 480 input channels: |acc| < 2^28; |bias| <= 2^30, so |a| < 2^31; m < 2^31, so |a m| < 2^62 and the rounding term
    (< 2^62) keeps the sum inside int64"""
    assert R.acc_bound(25, 480) == 25 * 480 * 128 * 127 < 1 << 28
    a_max = R.acc_bound(25, 480) + R.BIAS_MAX
    assert a_max < 1 << 31
    assert a_max * ((1 << 31) - 1) < 1 << 62
    assert a_max * ((1 << 31) - 1) + (1 << 61) < (1 << 63) - 1
    assert P.BIAS_MAX == R.BIAS_MAX == 1 << 30


# ---- the conversion ----
def _float_layers(seed, N=32, M=64, mean_scale=False):
    g = torch.Generator().manual_seed(seed)
    ch = (N, M, M * 3 // 2, 2 * M) if mean_scale else (N, N, N, M)
    ws = [torch.randn(ch[0], ch[1], 5, 5, generator=g) * 0.05, torch.randn(ch[1], ch[2], 5, 5, generator=g) * 0.05,
          torch.randn(ch[3], ch[2], 3, 3, generator=g) * 0.08]
    bs = [torch.randn(c, generator=g) * 0.1 for c in ch[1:]]
    return ws, bs, ((0.01, 0.01, 1.0) if mean_scale else (0.0, 0.0, 0.0))


def _float_net(ws, bs, slopes, z):
    act = lambda t, s: torch.where(t >= 0, t, t * s)
    t1 = act(F.conv_transpose2d(z, ws[0], bs[0], stride=2, padding=2, output_padding=1), slopes[0])
    t2 = act(F.conv_transpose2d(t1, ws[1], bs[1], stride=2, padding=2, output_padding=1), slopes[1])
    return t1, t2, act(F.conv2d(t2, ws[2], bs[2], padding=1), slopes[2])


@pytest.fixture(scope="module", params=[False, True], ids=["scale", "mean-scale"])
def converted(request):
    ws, bs, slopes = _float_layers(3, mean_scale=request.param)
    ws, bs = [w.double() for w in ws], [b.double() for b in bs]
    z = torch.round(torch.randn(2, 32, 2, 3, generator=torch.Generator().manual_seed(4)).double() * 3) + 0.25
    t1, t2, _ = _float_net(ws, bs, slopes, z)
    amax = [float(t1.abs().max()), float(t2.abs().max())]
    f0 = R.choose_f0(float(z.abs().max()))
    net = R.convert([w.numpy() for w in ws], [b.numpy() for b in bs], amax, slopes, f0)
    return ws, bs, slopes, z, amax, f0, net


def test_conversion_is_deterministic_and_the_product_gives_the_reference_integers(converted):
    ws, bs, slopes, z, amax, f0, net = converted
    again = R.convert([w.numpy() for w in ws], [b.numpy() for b in bs], amax, slopes, f0)
    prod = P.convert([w.numpy() for w in ws], [b.numpy() for b in bs], amax, slopes, f0)
    for a, b, c in zip(net["layers"], again["layers"], prod):
        for k in ("w", "bias", "mult_pos", "mult_neg", "shift"):
            assert a[k].dtype == c[k].dtype and np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]), k
    assert f0 == P.choose_f0(float(z.abs().max())) and 0 <= f0 <= 4 and float(z.abs().max()) * 2 ** f0 <= 127
    for layer in net["layers"]:
        assert ((layer["mult_pos"] >= 1 << 30) & (layer["mult_pos"].astype(np.int64) < 1 << 31)).all()
        assert ((layer["shift"] >= 1) & (layer["shift"] <= 62)).all()
        assert (np.abs(layer["w"].astype(np.int32)) <= 127).all() and np.abs(layer["w"].astype(np.int32)).max() == 127
        assert (layer["mult_neg"] >= 0).all() and (layer["mult_neg"] <= layer["mult_pos"]).all()
    if slopes[2] == 1.0:
        assert np.array_equal(net["layers"][2]["mult_neg"], net["layers"][2]["mult_pos"])   # linear last layer
    else:
        assert not net["layers"][0]["mult_neg"].any()                                        # ReLU
    mod = P.IntegerHyperSynthesis.from_float(ws, bs, amax, slopes, f0, split=slopes[2] == 1.0)
    assert mod.ready and mod.spec_hash() == R.spec_hash(net)


def test_bias_clamp_dead_channel_and_unservable_factor():
    ws, bs, slopes = _float_layers(5)
    bs[0][3] = 1e9
    bs[0][4] = -1e9
    ws[1][:, 7] = 0.0   # a dead output channel: the floor keeps s_w positive
    layers = P.convert([w.double().numpy() for w in ws], [b.double().numpy() for b in bs], [2.0, 2.0], slopes, 2)
    assert layers[0]["bias"][3] == 1 << 30 and layers[0]["bias"][4] == -(1 << 30)
    assert not layers[1]["w"][:, 7].any() and 1 <= layers[1]["shift"][7] <= 62 and layers[1]["mult_pos"][7] >= 1 << 30
    with pytest.raises(ValueError, match="outside 1 .. 62"):
        P.multiplier(2.0 ** 40, 0.0)
    assert P.multiplier(1.0, 1.0) == R.multiplier(1.0, 1.0) == (1 << 30, 1 << 30, 30)
    assert P.multiplier(1.0 - 2.0 ** -40, 0.0) == (1 << 30, 0, 30)   # the mantissa that rounds up to 2^31 carries into the exponent


def test_per_layer_error_bound(converted):
    """The real-valued layer in float64 on the dequantised inputs and weights, in output steps; the integer layer must be within
    0.5 + 2^-20 of a step (2^-14 for the 16-bit last layer) except where it is clamped.  The multiplier carries 30 significant bits:
    its error on |out| <= 2^15 is below 2^-15 of a step."""
    ws, bs, slopes, z, amax, f0, net = converted
    x = R.quantize_input(z.float().numpy(), f0)
    for i, layer in enumerate(net["layers"]):
        xd = torch.from_numpy(x.astype(np.float64) * layer["s_in"]).permute(0, 3, 1, 2)
        sw = torch.from_numpy(layer["s_w"])
        bd = torch.from_numpy(layer["bias"].astype(np.float64)) * layer["s_in"] * sw
        if i < 2:
            wd = torch.from_numpy(layer["w"].astype(np.float64)) * sw.reshape(1, -1, 1, 1)
            real = F.conv_transpose2d(xd, wd, bd, stride=2, padding=2, output_padding=1)
        else:
            wd = torch.from_numpy(layer["w"].astype(np.float64)) * sw.reshape(-1, 1, 1, 1)
            real = F.conv2d(xd, wd, bd, padding=1)
        real = (torch.where(real >= 0, real, real * slopes[i]) / layer["s_out"]).permute(0, 2, 3, 1).numpy()
        r = R.requant(R.layer_acc(x, layer, i < 2), layer["bias"], layer["mult_pos"], layer["mult_neg"], layer["shift"])
        lo, hi, eps = (-128, 127, 2.0 ** -20) if i < 2 else (-32768, 32767, 2.0 ** -14)
        inside = (r > lo) & (r < hi)
        assert inside.mean() > 0.5
        err = np.abs(r.astype(np.float64) - real)[inside]
        assert err.max() <= 0.5 + eps, (i, err.max())
        x = np.clip(r, lo, hi).astype(np.int8) if i < 2 else None


def test_integer_net_follows_the_float_net(converted):
    """not a gate on quality (DESIGN 32 records the measured cost): the converted net's outputs are the float net's within a few
    output steps of the coarsest layer — a conversion that scrambled a layout would be off by the whole range"""
    ws, bs, slopes, z, amax, f0, net = converted
    want = _float_net(ws, bs, slopes, z)[2].numpy()
    got = R.forward(net, z.float().numpy()).astype(np.float64)
    assert got.shape == want.shape
    assert np.abs(got - want).mean() < 0.05 * np.abs(want).max()


# ---- the hash and the container ----
def test_spec_hash_changes_with_every_buffer_f0_and_f_out(converted):
    ws, bs, slopes, z, amax, f0, net = converted
    mod = P.IntegerHyperSynthesis.from_float(ws, bs, amax, slopes, f0, split=slopes[2] == 1.0)
    h0 = mod.spec_hash()
    assert 0 <= h0 < 1 << 32 and h0 == R.spec_hash(net)
    seen = {h0}
    for name, buf in mod.named_buffers():
        old = buf.view(-1)[-1].item()
        buf.view(-1)[-1] = old + 1
        h = mod.spec_hash()
        assert h not in seen, name
        seen.add(h)
        buf.view(-1)[-1] = old
        assert mod.spec_hash() == h0
    mod.fixed_point[0] += 1   # f0 (the loop above moved f_out, the last element)
    assert mod.spec_hash() not in seen
    sd = mod.state_dict()
    fresh = P.IntegerHyperSynthesis(mod.channels, split=mod.split)
    assert not fresh.ready
    fresh.load_state_dict(sd)
    assert fresh.ready and fresh.spec_hash() == mod.spec_hash()


def _v123_expected(ver, tag, h, hw, shape, y, z, model_id=0, n_refs=0, bank_id=None, ids=()):
    head = b"CLC1" + struct.pack("<BBBBHHHHII", ver, model_id, n_refs, tag, hw[0], hw[1], shape[0], shape[1], len(y), len(z))
    if ver >= 2:
        head += struct.pack("<I", h)
    if ver == 3:
        head += struct.pack("<I", bank_id) + struct.pack(f"<{len(ids)}I", *ids)
    return head + z + y


def test_container_version_4_and_the_older_versions_bytes():
    y, z = b"\x01\x02\x03\x04\x05", b"\xaa\xbb\xcc"
    strings, shape, hw = [[y], [z]], (2, 3), (128, 192)
    now = codec.kernel_config()
    # versions 1 - 3: the bytes they produced
    assert codec.pack(strings, shape, hw, kernel_config_=(5, 0x11223344)) == _v123_expected(1, 5, None, hw, shape, y, z)
    assert codec.pack(strings, shape, hw, model_id=2, kernel_config_=(200, 0x11223344)) == _v123_expected(2, 200, 0x11223344, hw, shape, y, z, model_id=2)
    assert codec.pack(strings, shape, hw, kernel_config_=(5, 0x11223344), bank_id=9, ref_ids=[4, 7]) == \
        _v123_expected(3, 5, 0x11223344, hw, shape, y, z, n_refs=2, bank_id=9, ids=(4, 7))
    item = {"strings": strings, "shape": shape, "kernel_config": (5, 0x11223344)}
    assert codec.pack_item(item, hw) == _v123_expected(1, 5, None, hw, shape, y, z)
    # version 4
    blob = codec.pack_item(dict(item, exact=0xDEADBEEF), hw, model_id=3)
    assert blob == b"CLC1" + struct.pack("<BBBBHHHHII", 4, 3, 0, 0, 128, 192, 2, 3, 5, 3) + struct.pack("<I", 0xDEADBEEF) + z + y
    s, sh, meta = codec.unpack(blob, strict=True)   # a foreign kernel state is no reason to refuse it
    assert s == strings and tuple(sh) == shape and meta["exact_hash"] == 0xDEADBEEF and meta["same_kernel_config"] is True
    assert meta["image_hw"] == hw and meta["model_id"] == 3 and "kernel_config_tag" not in meta
    it = codec.unpack_item(blob)
    assert it["exact"] == 0xDEADBEEF and it["strings"] == strings
    # the contrast: the same strings as a version-2 container of another kernel state are refused under strict
    foreign = codec.pack(strings, shape, hw, kernel_config_=((now[0] % 100) + 130, now[1] ^ 1))
    with pytest.raises(codec.KernelConfigMismatch):
        codec.unpack(foreign, strict=True)
    with pytest.raises(ValueError, match="truncated"):
        codec.unpack(blob[:-1])
    bad = bytearray(blob)
    bad[7] = 9   # the tag byte of a version-4 header must be 0
    with pytest.raises(ValueError, match="version-4"):
        codec.unpack(bytes(bad))
    with pytest.raises(ValueError, match="u32"):
        codec.pack_exact(strings, shape, hw, 1 << 32)
    with pytest.raises(ValueError, match="exact stream"):
        codec.check_items([it], None)


# ---- refusals before the GPU check ----
def test_model_refusals_by_name():
    from clc_amd import models as pm
    from clc_amd.models.cheng import Cheng2020Anchor
    from clc_amd.models.elic import Elic2022
    from clc_amd.models.hyperprior import JointAutoregressiveHierarchicalPriors, JointCheckerboardHierarchicalPriors, MeanScaleHyperprior, ScaleHyperprior
    from clc_amd.models.video import ScaleSpaceFlow

    for cls, kw in ((ScaleHyperprior, dict(N=48, M=64)), (ScaleHyperprior, dict(N=32, M=48)), (MeanScaleHyperprior, dict(N=32, M=32))):
        with pytest.raises(ValueError, match="multiple of 32"):
            cls(integer_hyper=True, **kw)
        cls(**kw)   # without the flag these sizes are served as before
    for cls, kw in ((JointAutoregressiveHierarchicalPriors, {}), (JointCheckerboardHierarchicalPriors, {}), (Cheng2020Anchor, {}), (Elic2022, {}),
                    (pm.CLC, {}), (pm.TCM, {}), (ScaleSpaceFlow, {})):
        with pytest.raises(ValueError, match="no integer hyper-synthesis net: integer_hyper"):
            cls(integer_hyper=True, **kw)
        with pytest.raises(ValueError, match="no integer hyper-synthesis net: exact"):
            cls(exact=True, **kw)
    with pytest.raises(TypeError, match="unexpected keyword"):
        ScaleSpaceFlow(bogus=1)

    x = torch.zeros(1, 3, 64, 64)
    plain = ScaleHyperprior(N=32, M=64).eval()
    assert not any("h_s_int" in k for k in plain.state_dict())
    for call in (lambda: plain.compress(x, exact=True), lambda: plain.forward(x, exact=True), lambda: plain.decompress([[b""], [b""]], (1, 1), exact=True),
                 lambda: plain.decompress([[b""], [b""]], (1, 1), exact=123), lambda: plain.integerize(x)):
        with pytest.raises(ValueError, match="integer_hyper=True"):
            call()
    for cls in (ScaleHyperprior, MeanScaleHyperprior):
        m = cls(N=32, M=64, integer_hyper=True).eval()
        keys = [k for k in m.state_dict() if k.startswith("h_s_int.")]
        assert len(keys) == 16 and set(m.state_dict()) - set(keys) == set(cls(N=32, M=64).state_dict())
        with pytest.raises(ValueError, match="not filled"):
            m.compress(x, exact=True)
        with pytest.raises(ValueError, match="not filled"):
            m.decompress([[b""], [b""]], (1, 1), exact=True)
        ws, bs, slopes = _float_layers(1, mean_scale=cls is MeanScaleHyperprior)
        m.h_s_int.fill(P.convert([w.double().numpy() for w in ws], [b.double().numpy() for b in bs], [2.0, 2.0], slopes, 2), 2, 8)
        h = m.h_s_int.spec_hash()
        with pytest.raises(ValueError, match=f"0x{h ^ 1:08x}.*0x{h:08x}"):
            m.decompress([[b""], [b""]], (1, 1), exact=h ^ 1)
        with pytest.raises(TypeError, match="spec_hash as an int"):
            m.decompress([[b""], [b""]], (1, 1), exact="yes")
        m.train()
        with pytest.raises(ValueError, match="training mode"):
            m.forward(x, exact=True)
        m.eval()
        with pytest.raises(L.ClcError, match="GPU only"):   # the product path has no CPU fallback
            m.h_s_int(torch.zeros(1, 32, 1, 1))
        fresh = cls(N=32, M=64, integer_hyper=True)
        fresh.load_state_dict(m.state_dict())
        assert fresh.h_s_int.spec_hash() == h
    with pytest.raises(ValueError, match="multiple of 32"):
        P.IntegerHyperSynthesis((32, 32, 40, 64))


def test_c_abi_refuses_bad_arguments_before_any_launch():
    lib = L.load()
    ok = dict(x=4096, B=1, H=2, W=2, Cin=32, ldx=32, w_packed=4096, bias=4096, mult_pos=4096, mult_neg=4096, shift=4096, y=4096, Cout=32, ldy=32,
              transposed=0, out_kind=0, f_out=8)   # (the pointers are never followed: every case below is refused first)
    bad = [(dict(Cin=48, ldx=48), "multiples of 32"), (dict(Cout=40, ldy=40), "multiples of 32"), (dict(x=0), "NULL"), (dict(H=0), "positive"),
           (dict(transposed=2), "transposed"), (dict(out_kind=3), "out_kind"), (dict(ldx=40), "ldx"), (dict(ldy=34), "ldy"), (dict(ldy=16), "ldy"),
           (dict(w_packed=4100), "aligned"), (dict(out_kind=1, y=4100), "aligned"), (dict(y=4098), "aligned"), (dict(out_kind=1, f_out=31), "f_out")]
    for change, word in bad:
        d = L.IntConvDesc(**dict(ok, **change))
        assert lib.clc_int_conv(d, None) == -1, change
        assert word in lib.clc_last_error().decode(), (change, lib.clc_last_error())
    assert lib.clc_int_conv(None, None) == -1
    for args, word in (((0, 4, 0, 4096), "NULL"), ((4096, 6, 0, 4096), "multiple of 4"), ((4096, 8, 17, 4096), "f0"), ((4100, 8, 0, 4096), "aligned")):
        assert lib.clc_int_quantize(args[0], args[1], args[2], args[3], None) == -1
        assert word in lib.clc_last_error().decode(), args
