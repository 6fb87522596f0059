"""The lanes stream of CLC / TCM through the models and the CodecEngine, in the configuration of
tests/test_codec_service_gpu.py: CLC(N=64, one reference) and TCM(N=64), 256x256, B = 3, lanes = 2.  Every comparison is exact.

The engine's y strings are ans.lanes_pack(ans.lanes_encode(...)) of the default encoder's symbols and indexes re-ordered to NHWC, the z
strings the default's; x_hat from the device coder, the host coder of the same format, the default format and _decompress_eager are
bit-equal; the graph and the eager engine are identical; an image's strings do not depend on its position in the batch; the container
carries the string; the counted device -> host copies are 2 for compress and 0 / 1 for decompress (check=False / True) against one
per slice between the default's num_slices + 1 graphs; one image
through model.compress / decompress is the batch engine's; a flipped state word is named; a plan with too small a words buffer is
rebuilt, never truncated; and the default path's bytes and tag are afterwards what they were before."""
import numpy as np
import pytest
import torch

from test_cheng_model_gpu import _count_d2h

pytestmark = pytest.mark.gpu

B, W = 3, 2


def _flip_state_word(blob, wave):
    from clc_amd import ans

    streams = [bytearray(s) for s in ans.lanes_unpack(blob)]
    streams[wave][4 * 7 + 1] ^= 0x10   # lane 3's high word
    return ans.lanes_pack([bytes(s) for s in streams])


@pytest.mark.parametrize("kind,R", [("clc", 1), ("tcm", 0)])
def test_lanes_stream_through_engine_and_model(dev, kind, R):
    from clc_amd import ans, codec
    from clc_amd import models as pm
    from clc_amd.recipe import apply_weight_recipe, synthetic_image

    m = pm.CLC(N=64, num_ref_frames=R) if kind == "clc" else pm.TCM(N=64)
    apply_weight_recipe(m, 0)
    m = m.to(dev).eval()
    m.update(force=True)
    S = m.num_slices
    x = torch.cat([synthetic_image(1, 256, 256, 100 + 7 * i, smooth=True) for i in range(B)]).to(dev)
    refs = [torch.cat([synthetic_image(1, 256, 256, 200 + 7 * i + j, smooth=True) for i in range(B)]).to(dev) for j in range(R)]
    cdf, ln, off = m.gaussian_conditional.host_tables()
    tag_before = codec.kernel_config()

    # the default format, launch by launch: strings, x_hat, and the encoder's symbols / indexes as _encode_y receives them
    want, seen = [], []
    encode_y = m._encode_y
    m._encode_y = lambda sp, ip: seen.append((sp, ip)) or encode_y(sp, ip)
    try:
        for i in range(B):
            ri = [r[i:i + 1] for r in refs] if R else None
            enc = m._compress_eager(x[i:i + 1], ri)
            want.append((enc, m._decompress_eager(enc["strings"], enc["shape"], ri)["x_hat"]))
    finally:
        del m._encode_y
    nhwc = lambda parts: np.concatenate([t.permute(0, 2, 3, 1).reshape(-1).cpu().numpy() for t in parts])
    segs = [int(t.numel()) for t in seen[0][0]]
    assert len(segs) == S and segs[0] == 16 * 16 * (320 // S)
    lanes_y = [ans.lanes_pack(ans.lanes_encode(nhwc(sp), nhwc(ip), segs, W, cdf, ln, off)) for sp, ip in seen]
    x_want = torch.cat([w[1] for w in want])
    shape = want[0][0]["shape"]

    results = {}
    for use_graph in (True, False):
        eng = codec.CodecEngine(m, threads=4, use_graph=use_graph)
        default = eng.compress(x, refs)
        assert all("lanes" not in o and o["strings"] == w[0]["strings"] for o, w in zip(default, want))
        outs = eng.compress(x, refs, lanes=W)
        with _count_d2h() as c:
            again = eng.compress(x, refs, lanes=W)
        assert c.n == 2 and eng.last["hops"] == 2
        assert [o["strings"] for o in again] == [o["strings"] for o in outs]
        for i, o in enumerate(outs):
            assert o["lanes"] == W and tuple(o["shape"]) == tuple(shape) and o["kernel_config"] == default[i]["kernel_config"]
            assert o["strings"][0] == [lanes_y[i]], f"image {i}: y string is not the host encoder's over the NHWC segments (graph={use_graph})"
            assert o["strings"][1] == default[i]["strings"][1]
        x_hat = eng.decompress(outs, refs, lanes=W)   # (builds the plan)
        with _count_d2h() as c:
            x0 = eng.decompress(outs, refs, lanes=W, check=False)
        assert c.n == 0 and eng.last["hops"] == 0
        with _count_d2h() as c:
            x1 = eng.decompress(outs, refs, lanes=W)
        assert c.n == 1 and eng.last["hops"] == 1
        x_def = eng.decompress(default, refs)
        with _count_d2h() as c:
            x_def2 = eng.decompress(default, refs)
        # (the default: one download per slice between its num_slices + 1 graphs, which is what its "hops" counts)
        assert c.n == S and eng.last["hops"] == S + 1
        for t in (x_hat, x0, x1, x_def, x_def2):
            assert torch.equal(t, x_want), f"graph={use_graph}"
        # a second, permuted batch through the same plans
        perm = [2, 0, 1]
        outs2 = eng.compress(x[perm], [r[perm] for r in refs], lanes=W)
        for k, i in enumerate(perm):
            assert outs2[k]["strings"] == outs[i]["strings"], "an image's strings depend on its position in the batch"
        assert torch.equal(eng.decompress(outs2, [r[perm] for r in refs], lanes=W), x_want[perm])
        # through the container: the string rides opaquely, the header names no format — lanes= is the caller's
        items = [codec.unpack_item(codec.pack_item(o, image_hw=(256, 256), n_refs=R)) for o in outs]
        assert [it["strings"] for it in items] == [o["strings"] for o in outs]
        assert torch.equal(eng.decompress(items, refs, lanes=W), x_want)
        with pytest.raises(ValueError, match=r"image 0 is a lanes stream \(b'CLN1'\); pass lanes="):
            eng.decompress(items, refs)
        with pytest.raises(ValueError, match="item 0 was coded with lanes = 2, the call says lanes = 3"):
            eng.decompress(outs, refs, lanes=3)
        with pytest.raises(ValueError, match="lanes = 3, but the header of image 0 says 2 wave streams"):
            eng.decompress(items, refs, lanes=3)
        with pytest.raises(ValueError, match="bad magic"):
            eng.decompress(default, refs, lanes=W)
        # a flipped state word is named by the check (and only by the check)
        bad = [dict(o) for o in outs]
        bad[1]["strings"] = [[_flip_state_word(outs[1]["strings"][0][0], 1)], outs[1]["strings"][1]]
        with pytest.raises(ValueError, match=r"image 1: wave streams \[.*1.*\] did not decode to their end"):
            eng.decompress(bad, refs, lanes=W)
        eng.decompress(bad, refs, lanes=W, check=False)
        assert torch.equal(eng.decompress(outs, refs, lanes=W), x_want)   # the plan is none the worse for it
        results[use_graph] = (outs, x_hat)
        if use_graph:
            # a plan built with a words buffer that only just holds a flat batch is rebuilt for this one, never truncated
            small = codec.CodecEngine(m, threads=2)
            small.lanes_words_slack = 1.0
            flat = small.compress(torch.full_like(x, 0.5), refs, lanes=W)
            words = lambda items: sum(len(s) // 4 for it in items for s in ans.lanes_unpack(it["strings"][0][0]))
            (less, x_less), (more, x_more) = sorted(((outs, x_want), (flat, eng.decompress(flat, refs, lanes=W))), key=lambda t: words(t[0]))
            assert words(less) < words(more)
            assert torch.equal(small.decompress(less, refs, lanes=W), x_less) and not small.last["plan_rebuilt"]
            assert next(iter(small._dec.values())).cap_words == words(less)
            assert torch.equal(small.decompress(more, refs, lanes=W), x_more) and small.last["plan_rebuilt"]
            assert torch.equal(small.decompress(more, refs, lanes=W), x_more) and not small.last["plan_rebuilt"]
            assert torch.equal(small.decompress(less, refs, lanes=W), x_less) and not small.last["plan_rebuilt"] and len(small._dec) == 1
            small.close()
        eng.close()
    assert [o["strings"] for o in results[True][0]] == [o["strings"] for o in results[False][0]]

    # the same format on the host coder (a hop per slice) and on the eager device coder, for the batch
    strings = [[o["strings"][0][0] for o in outs], [o["strings"][1][0] for o in outs]]
    rb = refs if R else None
    assert torch.equal(m._decompress_eager(strings, shape, rb, lanes=W, device_coder=False)["x_hat"], x_want)
    assert torch.equal(m._decompress_eager(strings, shape, rb, lanes=W)["x_hat"], x_want)
    assert torch.equal(m.decompress(strings, shape, rb, lanes=W)["x_hat"], x_want)
    eager = m._compress_eager(x, rb, lanes=W)
    assert eager["strings"] == strings and eager["lanes"] == W
    with pytest.raises(ValueError, match=r"image 1: wave streams \[.*1.*\] did not decode to their end"):
        m._decompress_eager([[strings[0][0], _flip_state_word(strings[0][1], 1), strings[0][2]], strings[1]], shape, rb, lanes=W, device_coder=False)

    # one image through the model rides on the engine
    r0 = [r[0:1] for r in refs] if R else None
    one = m.compress(x[0:1], r0, lanes=W)
    assert one["strings"] == outs[0]["strings"] and one["lanes"] == W and m.__dict__.get("_codec_eng") is not None
    assert torch.equal(m.decompress(one["strings"], one["shape"], r0, lanes=W)["x_hat"], x_want[0:1])
    assert m.__dict__["_codec_eng"].last["hops"] == 1 and m.__dict__["_codec_eng"].last["lanes"] == W
    assert torch.equal(m.decompress(one["strings"], one["shape"], r0, lanes=W, device_coder=False)["x_hat"], x_want[0:1])

    # the default path afterwards: the bytes and the tag of before
    d = m.compress(x[0:1], r0)
    assert sorted(d) == ["kernel_config", "shape", "strings"] and d["strings"] == want[0][0]["strings"]
    assert torch.equal(m.decompress(d["strings"], d["shape"], r0)["x_hat"], x_want[0:1])
    assert codec.kernel_config() == tag_before and tag_before[0] == 6
