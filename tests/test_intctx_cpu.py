"""The integer context model of mbt2018-checkerboard without a GPU: the reference arithmetic (tests/intctx_ref.py) against
float64 convolutions, the conversion (the product's integers are the reference's), the per-layer bound, the overflow bound, the hash,
the state_dict, the version-4 container, and every refusal that is made before the GPU is asked for."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import intctx_ref as X
import intnet_ref as R
from clc_amd import codec
from clc_amd import intnet as P
from clc_amd import lib as L
from clc_amd import ops

N_, M_ = 32, 192


def test_taps_and_offsets_are_the_products():
    assert X.CKBD_TAPS == ops.CKBD_TAPS and len(X.CKBD_TAPS) == 12
    assert X.CKBD_OFFSETS == P.CKBD_OFFSETS and X.K_MAX == 65536


# ---- the arithmetic against float64 ----
@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (2, 1, 2), (1, 2, 1), (2, 3, 3), (1, 5, 4)])
def test_reference_gather_and_sums_equal_torch_in_float64(B, H, W):
    """integers in float64 are exact: the masked 5x5 layer as a full conv2d whose dead taps are zero, read at the non-anchors; the
    1x1 layers as conv2d over the concatenated channels"""
    rng = np.random.default_rng(H * 10 + W)
    Cc, Co = 32, 64
    yq = rng.integers(-128, 128, (B, H, W, Cc)).astype(np.int8)
    wt = rng.integers(-127, 128, (Co, 12, Cc)).astype(np.int8)
    full = np.zeros((Co, Cc, 5, 5))
    for t, (kh, kw) in enumerate(X.CKBD_TAPS):
        full[:, :, kh, kw] = wt[:, t]
    want = F.conv2d(torch.from_numpy(yq.astype(np.float64)).permute(0, 3, 1, 2), torch.from_numpy(full), padding=2).permute(0, 2, 3, 1).numpy()
    others = [(h, w) for h in range(H) for w in range(W) if not (h + w) & 1]
    got = X.rows_acc(X.gather_taps(yq, others, P.CKBD_OFFSETS), wt)
    # the product's packed filter image holds the same [Cout][K] matrix: [ct][kc][h][r][j] <- channel 32 ct + r, k = 32 kc + 16 h + j
    packed = P.pack_rows(wt.reshape(Co, -1))
    assert packed.shape == (Co // 32, 12 * Cc // 32, 2, 32, 16) and packed.dtype == np.int8
    assert packed[1, 3, 1, 5, 7] == wt.reshape(Co, -1)[32 + 5, 32 * 3 + 16 + 7]
    assert np.array_equal(packed.transpose(0, 3, 1, 2, 4).reshape(Co, -1), wt.reshape(Co, -1))
    assert got.dtype == np.int64 and np.array_equal(got, np.stack([want[:, h, w] for h, w in others], 1).astype(np.int64))
    if H == W == 1:   # every tap off the map
        assert not got.any()
    psi = rng.integers(-128, 128, (B, H, W, 64)).astype(np.int8)
    ctx = rng.integers(-128, 128, (B, len(others), Co)).astype(np.int8)
    w1 = rng.integers(-127, 128, (96, 128)).astype(np.int8)
    x = np.concatenate((X.gather_pixels(psi, others), ctx.astype(np.int64)), -1)
    want1 = np.einsum("bpk,ok->bpo", x.astype(np.float64), w1.astype(np.float64))
    assert np.array_equal(X.rows_acc(x, w1), want1.astype(np.int64))
    # an anchor pass reads psi's columns alone
    lay = {"w": w1, "bias": np.zeros(96, np.int32), "mult_pos": np.full(96, 1 << 30, np.int32), "mult_neg": np.full(96, 1 << 30, np.int32),
           "shift": np.full(96, 40, np.int32)}
    xa = X.gather_pixels(psi, others)
    want_a = np.clip((xa @ w1[:, :64].astype(np.int64).T + (1 << 9)) >> 10, -128, 127)
    assert np.array_equal(X.rows_int8(xa, lay, cols=64), want_a.astype(np.int8))


def test_overflow_bound_for_the_largest_served_shape():
    """M = 384: the tap layer's K = 12 * 384 = 4608, |acc| < 2^27; the kernel's limit K <= 65536 gives |acc| <= 2^16 * 2^7 * 127
    < 2^30; |bias| <= 2^30, so |a| < 2^31; m < 2^31, so |a m| < 2^62 and the rounding term keeps the sum inside int64"""
    M = 384
    ks = (12 * M, 4 * M, M * 10 // 3, M * 8 // 3)
    assert max(ks) == 4608 and X.acc_bound(4608) == 4608 * 128 * 127 < 1 << 27
    assert P.K_MAX == X.K_MAX == 65536 and X.acc_bound(X.K_MAX) < 1 << 30
    a_max = X.acc_bound(X.K_MAX) + R.BIAS_MAX
    assert a_max < 1 << 31 and a_max * ((1 << 31) - 1) < 1 << 62 and a_max * ((1 << 31) - 1) + (1 << 61) < (1 << 63) - 1
    with pytest.raises(AssertionError, match="65536"):
        X.rows_acc(np.zeros((1, X.K_MAX + 32), np.int64), np.zeros((32, X.K_MAX + 32), np.int8))


# ---- the conversion ----
def _float_model(seed):
    from clc_amd.models.hyperprior import JointCheckerboardHierarchicalPriors

    torch.manual_seed(seed)
    return JointCheckerboardHierarchicalPriors(N_, M_).eval()


def _float_parts(m):
    from clc_amd.models.coding import linear_filters

    np64 = lambda t: t.detach().double().cpu().numpy()
    hs = [(np64(l.weight), np64(l.bias)) for l in (m.h_s[0], m.h_s[2], m.h_s[4])]
    ep = [(np64(w), np64(b)) for w, b in linear_filters(m.entropy_parameters)]
    return hs, (np64(m.context_prediction.weight), np64(m.context_prediction.bias)), ep


AMAX = {"hs1": 1.7, "hs2": 2.9, "psi": 3.1, "ctx": 4.4, "ep1": 2.2, "ep2": 1.3}


@pytest.fixture(scope="module")
def converted():
    m = _float_model(5)
    with torch.no_grad():
        m.context_prediction.bias.normal_(0, 0.2)
        for i in (0, 2, 4):
            m.entropy_parameters[i].bias.normal_(0, 0.1)
    hs, ctx, ep = _float_parts(m)
    net = X.convert(hs, ctx, ep, AMAX, 9.3, 20.6)
    return m, (hs, ctx, ep), net


def test_conversion_the_product_gives_the_reference_integers(converted):
    m, (hs, ctx, ep), net = converted
    assert (net["f0"], net["f_y"], net["f_out"]) == (3, 2, 8)   # 9.3 * 8 <= 127 < 9.3 * 16; 20.6 * 4 <= 127 < 20.6 * 8
    assert X.choose_f_y(0.0) == P.choose_f_y(0.0) == 4 and X.choose_f_y(500.0) == P.choose_f_y(500.0) == 0
    hs_l, ctx_l, f0, f_y, f_out = P.convert_context_model(hs, ctx, ep, AMAX, 9.3, 20.6)
    again = X.convert(hs, ctx, ep, AMAX, 9.3, 20.6)
    assert (f0, f_y, f_out) == (net["f0"], net["f_y"], net["f_out"])
    for ref, ref2, prod in zip(net["hs"] + net["ctx"], again["hs"] + again["ctx"], hs_l + ctx_l):
        for k in ("w", "bias", "mult_pos", "mult_neg", "shift"):
            assert ref[k].dtype == prod[k].dtype and ref[k].shape == prod[k].shape and np.array_equal(ref[k], prod[k]), k
            assert np.array_equal(ref[k], ref2[k])
    assert net["ctx"][0]["w"].shape == (2 * M_, 12, M_) and net["ctx"][1]["w"].shape == (M_ * 10 // 3, 4 * M_)
    # psi and the context rows share one scale, so layer 1 has one s_in
    assert net["hs"][2]["s_out"] == net["ctx"][0]["s_out"] == net["ctx"][1]["s_in"] == max(AMAX["psi"], AMAX["ctx"]) / 127.0
    assert np.array_equal(net["ctx"][0]["mult_neg"], net["ctx"][0]["mult_pos"]) and np.array_equal(net["ctx"][3]["mult_neg"], net["ctx"][3]["mult_pos"])
    assert (net["ctx"][1]["mult_neg"] < net["ctx"][1]["mult_pos"]).all() and (net["ctx"][1]["mult_neg"] > 0).all()
    # the generalised conversion still gives the hyper nets' integers (tests/intnet_ref.py)
    ws, bs = [w for w, _ in hs], [b for _, b in hs]
    for a, b in zip(R.convert(ws, bs, [1.7, 2.9], (0.01, 0.01, 1.0), 3)["layers"], P.convert(ws, bs, [1.7, 2.9], (0.01, 0.01, 1.0), 3)):
        for k in ("w", "bias", "mult_pos", "mult_neg", "shift"):
            assert np.array_equal(a[k], b[k])


def test_per_layer_error_bound(converted):
    """Each layer of the chain against the real-valued layer in float64 on the dequantised operands, in output steps.  The integer
    layer computes floor(a m 2^-s + 1/2) with m = rint(rho 2^s): rounding to nearest costs at most 0.5 of a step, and the multiplier
    differs from rho 2^s by at most 0.5, a relative error of 2^-31 for mult_pos (>= 2^30) and of 2^-24 for a LeakyReLU mult_neg
    (rho 0.01 2^s >= 0.01 2^30 > 2^23), which moves the result by |real| times that.  1e-9 covers float64's own rounding of real."""
    m, parts, net = converted
    rng = np.random.default_rng(7)
    B, H, W = 2, 3, 4
    psi = rng.integers(-128, 128, (B, H, W, 2 * M_)).astype(np.int8)
    yq = np.zeros((B, H, W, M_), np.int8)
    for h in range(H):
        for w in range(W):
            if (h + w) & 1:
                yq[:, h, w] = rng.integers(-60, 61, (B, M_))
    others = X.passes(H, W)[1]
    got = X.chain(net, others, psi, yq)
    L4 = net["ctx"]
    ins = [X.gather_taps(yq, others), None, got["h1"].astype(np.int64), got["h2"].astype(np.int64)]
    ins[1] = np.concatenate((X.gather_pixels(psi, others), got["ctx"].astype(np.int64)), -1)
    for i, (x, layer) in enumerate(zip(ins, L4)):
        wd = layer["w"].reshape(len(layer["bias"]), -1).astype(np.float64) * layer["s_w"][:, None]
        real = (x.astype(np.float64) * layer["s_in"]) @ wd.T + layer["bias"].astype(np.float64) * layer["s_in"] * layer["s_w"]
        neg = real < 0
        real = np.where(neg, real * layer["slope"], real) / layer["s_out"]
        r = R.requant(X.rows_acc(x, layer["w"]), layer["bias"], layer["mult_pos"], layer["mult_neg"], layer["shift"])
        lo, hi = (-128, 127) if i < 3 else (-32768, 32767)
        eps = np.where(neg & (layer["slope"] != 1.0), 2.0 ** -24, 2.0 ** -31)
        err = np.abs(r.astype(np.float64) - real)
        assert (err <= 0.5 + np.abs(real) * eps + 1e-9).all(), (i, err.max())
        assert ((r > lo) & (r < hi)).mean() > 0.5, i   # (the bound is about the unclamped r; most of it is not at a clamp)


# ---- the hash, the state_dict, the container ----
def _integer_model(net, **kw):
    from clc_amd.models.hyperprior import JointCheckerboardHierarchicalPriors

    m = JointCheckerboardHierarchicalPriors(N_, M_, integer_context=True, **kw).eval()
    pick = lambda layers: [{k: l[k] for k in ("w", "bias", "mult_pos", "mult_neg", "shift")} for l in layers]
    m.h_s_int.fill(pick(net["hs"]), net["f0"], net["f_out"])
    m.ctx_int.fill(pick(net["ctx"]), net["f_y"], net["f_out"])
    return m


def test_hash_is_stable_and_sensitive(converted):
    _, _, net = converted
    m = _integer_model(net)
    h = m.spec_hash()
    assert h == X.spec_hash(net) == P.context_spec_hash(m.h_s_int, m.ctx_int) and 0 <= h < 1 << 32
    assert _integer_model(net).spec_hash() == h
    assert X.spec_hash(X.net_of_state_dict({k: v.numpy() for k, v in m.state_dict().items()})) == h
    with torch.no_grad():
        m.ctx_int.w0[5, 3, 7] += 1   # one weight of the context layer
    h1 = m.spec_hash()
    assert h1 != h
    with torch.no_grad():
        m.ctx_int.w0[5, 3, 7] -= 1
        m.h_s_int.w1[0, 0, 0, 0] += 1
    assert m.spec_hash() not in (h, h1)
    with torch.no_grad():
        m.h_s_int.w1[0, 0, 0, 0] -= 1
    assert m.spec_hash() == h
    for which in range(2):   # f_y, f_out
        with torch.no_grad():
            m.ctx_int.fixed_point[which] += 1
        assert m.spec_hash() != h
        with torch.no_grad():
            m.ctx_int.fixed_point[which] -= 1
    assert m.spec_hash() == h
    changed = dict(net, f_y=net["f_y"] + 1)
    assert X.spec_hash(changed) != h
    # the hyper net's own mode: the int8-output switch adds no key and does not move the 16 keys' hash
    a, b = P.IntegerHyperSynthesis((32, 64, 96, 128), split=True), P.IntegerHyperSynthesis((32, 64, 96, 128), int8_out=True)
    assert list(a.state_dict()) == list(b.state_dict()) and len(a.state_dict()) == 16 and a.spec_hash() == b.spec_hash()


def test_state_dict_round_trip_and_keys(converted):
    from clc_amd.models.hyperprior import JointCheckerboardHierarchicalPriors

    _, _, net = converted
    m = _integer_model(net)
    plain = JointCheckerboardHierarchicalPriors(N_, M_)
    assert not hasattr(plain, "h_s_int") and not hasattr(plain, "ctx_int")
    extra = set(m.state_dict()) - set(plain.state_dict())
    assert set(plain.state_dict()) <= set(m.state_dict())
    assert extra == {k for k in m.state_dict() if k.startswith(("h_s_int.", "ctx_int."))}
    assert len([k for k in extra if k.startswith("h_s_int.")]) == 16 and len([k for k in extra if k.startswith("ctx_int.")]) == 21
    fresh = JointCheckerboardHierarchicalPriors(N_, M_, integer_context=True)
    assert not fresh.ctx_int.ready and not fresh.h_s_int.ready
    fresh.load_state_dict(m.state_dict())
    assert fresh.ctx_int.ready and fresh.spec_hash() == m.spec_hash()
    assert fresh.ctx_int.f_y == net["f_y"]


def test_version_4_container_round_trip(converted):
    _, _, net = converted
    h = _integer_model(net).spec_hash()   # what compress(x, exact=True) puts into its item
    assert h == X.spec_hash(net)
    for lanes in (None, 4):
        item = {"strings": [[b"\x01\x02\x03\x04", b"\x09\x08\x07\x06"], [b"\xaa\xbb", b"\xcc"]], "shape": (2, 3), "kernel_config": codec.kernel_config(),
                "exact": h}
        if lanes:
            item["lanes"] = lanes
        blobs = [codec.pack_item({**item, "strings": [[item["strings"][0][i]], [item["strings"][1][i]]]}, (128, 192)) for i in range(2)]
        for i, blob in enumerate(blobs):
            assert blob[4] == 4
            got = codec.unpack_item(blob, strict=True)
            assert got["exact"] == h and got["meta"]["exact_hash"] == h and tuple(got["shape"]) == (2, 3)
            assert got["strings"] == [[item["strings"][0][i]], [item["strings"][1][i]]]
            with pytest.raises(ValueError, match="exact stream"):
                codec.check_items([got], None)


# ---- refusals before the GPU check ----
def test_refusals_by_name(converted):
    from clc_amd.models.hyperprior import JointAutoregressiveHierarchicalPriors, JointCheckerboardHierarchicalPriors

    _, _, net = converted
    with pytest.raises(ValueError, match="no integer context net: integer_context"):
        JointAutoregressiveHierarchicalPriors(integer_context=True)
    JointAutoregressiveHierarchicalPriors(N_, 24, integer_context=False)
    for kw in (dict(N=N_, M=96), dict(N=N_, M=320), dict(N=48, M=192), dict(N=N_, M=204)):
        with pytest.raises(ValueError, match="multiple of 192 and N a multiple of 32"):
            JointCheckerboardHierarchicalPriors(integer_context=True, **kw)
    JointCheckerboardHierarchicalPriors(N=N_, M=96)   # without the flag these sizes are served as before
    with pytest.raises(ValueError, match="no integer hyper-synthesis net: integer_hyper"):
        JointCheckerboardHierarchicalPriors(N_, M_, integer_context=True, integer_hyper=True)
    with pytest.raises(ValueError, match="rate_levels"):
        JointCheckerboardHierarchicalPriors(N_, M_, integer_context=True, rate_levels=4)
    with pytest.raises(ValueError, match="multiple of 192"):
        P.IntegerContextParameters(96)

    x = torch.zeros(1, 3, 64, 64)
    plain = JointCheckerboardHierarchicalPriors(N_, M_).eval()
    for call in (lambda: plain.compress(x, exact=True), lambda: plain.compress(x, lanes=4, exact=True), lambda: plain.forward(x, exact=True),
                 lambda: plain.decompress([[b""], [b""]], (1, 1), exact=True), lambda: plain.decompress([[b""], [b""]], (1, 1), lanes=4, exact=123),
                 lambda: plain._decode_y_hat([[b""], [b""]], (1, 1), exact=True), lambda: plain.integerize(x), lambda: plain.spec_hash()):
        with pytest.raises(ValueError, match="integer_context=True"):
            call()
    empty = JointCheckerboardHierarchicalPriors(N_, M_, integer_context=True).eval()
    for call in (lambda: empty.compress(x, exact=True), lambda: empty.decompress([[b""], [b""]], (1, 1), exact=True), lambda: empty.forward(x, exact=True)):
        with pytest.raises(ValueError, match="not filled"):
            call()
    half = JointCheckerboardHierarchicalPriors(N_, M_, integer_context=True).eval()
    half.h_s_int.fill([{k: l[k] for k in ("w", "bias", "mult_pos", "mult_neg", "shift")} for l in net["hs"]], net["f0"], net["f_out"])
    with pytest.raises(ValueError, match="integer context net is not filled"):
        half.compress(x, exact=True)
    m = _integer_model(net)
    h = m.spec_hash()
    with pytest.raises(ValueError, match=f"0x{h ^ 1:08x}.*0x{h:08x}"):
        m.decompress([[b""], [b""]], (1, 1), exact=h ^ 1)
    with pytest.raises(ValueError, match=f"0x{h ^ 1:08x}.*0x{h:08x}"):
        m.decompress([[b""], [b""]], (1, 1), lanes=4, exact=h ^ 1)
    with pytest.raises(TypeError, match="spec_hash as an int"):
        m.decompress([[b""], [b""]], (1, 1), exact="yes")
    m.train()
    with pytest.raises(ValueError, match="training mode"):
        m.forward(x, exact=True)
    m.eval()
    with pytest.raises(L.ClcError, match="GPU only"):   # the product path has no CPU fallback
        m.compress(x, exact=True)
    with pytest.raises(ValueError, match="one or two K ranges"):
        P.int_rows([], torch.zeros(1, 2, dtype=torch.int32), 1, 1, 1, None, None, None, None, None, 32, None)


def test_c_abi_refuses_bad_arguments_before_any_launch():
    import ctypes as C

    lib = L.load()
    taps = (C.c_int * 52)(*([0, 1] * 26))
    far = (C.c_int * 2)(0, 200)

    def desc(src=((4096, 32, 32, L.INT_SRC_PIXEL),), **kw):
        ok = dict(nsrc=len(src), pix=4096, P=3, B=1, H=2, W=2, ntaps=0, w_packed=4096, bias=4096, mult_pos=4096, mult_neg=4096, shift=4096, y=4096,
                  Cout=32, ldy=32, out_kind=0, f_out=8)   # (the pointers are never followed: every case below is refused first)
        d = L.IntRowsDesc(**dict(ok, **kw))
        for i, s in enumerate(src[:2]):
            d.src[i] = L.IntSrc(*s)
        return d

    T, D, X_ = L.INT_SRC_TAPS, L.INT_SRC_DENSE, L.INT_SRC_PIXEL
    bad = [(desc(pix=0), "NULL"), (desc(y=0), "NULL"), (desc(shift=0), "NULL"), (desc(src=((0, 32, 32, X_),)), "p is NULL"),
           (desc(src=((4096, 48, 48, X_),)), "multiple of 32"), (desc(Cout=40, ldy=40), "multiple of 32"), (desc(Cout=0), "multiple of 32"),
           (desc(src=((4096, 16, 32, D),)), "ld must be"), (desc(src=((4096, 40, 32, D),)), "ld must be"), (desc(src=((4100, 32, 32, D),)), "aligned"),
           (desc(nsrc=3), "one or two"), (desc(nsrc=0), "one or two"), (desc(src=((4096, 32, 32, 7),)), "kind"),
           (desc(src=((4096, 32, 32, T),), taps=taps, ntaps=26), "1 .. 25 taps"), (desc(src=((4096, 32, 32, T),), taps=taps, ntaps=0), "1 .. 25 taps"),
           (desc(src=((4096, 32, 32, T),), ntaps=12), "taps is NULL"), (desc(src=((4096, 32, 32, T),), taps=far, ntaps=1), "within"),
           (desc(src=((4096, 65536, 65536, X_), (4096, 32, 32, D))), "65536"), (desc(src=((4096, 4096, 4096, T),), taps=taps, ntaps=17), "65536"),
           (desc(out_kind=1, f_out=31), "f_out"), (desc(out_kind=1, f_out=-1), "f_out"), (desc(out_kind=2), "out_kind"),
           (desc(ldy=16), "ldy"), (desc(ldy=34), "ldy"), (desc(P=0), "positive"), (desc(H=0), "positive"),
           (desc(w_packed=4100), "aligned"), (desc(bias=4104), "aligned"), (desc(out_kind=1, y=4100), "aligned"), (desc(y=4098), "aligned"),
           (desc(pix=4098), "pix must be")]
    for d, word in bad:
        assert lib.clc_int_rows(d, None) == -1, word
        assert word in lib.clc_last_error().decode(), (word, lib.clc_last_error())
    assert lib.clc_int_rows(None, None) == -1
