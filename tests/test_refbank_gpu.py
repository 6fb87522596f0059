"""Reference bank of the codec (clc_amd.refbank; clc_ref_prepare / clc_gather_slots / clc_fingerprint in csrc/refbank.hip): the preparation
recipe against float64 ATen, the gather and the fingerprint, and the bank path of CodecEngine against the tensor path and the eager
methods — byte-identical streams, containers that decode with the bank alone, warm / evicting / stale caches, other banks refused."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def models_by_R(dev):
    """one CLC(N=64) per reference count, built on first use"""
    from clc_amd import models as pm
    from clc_amd.recipe import apply_weight_recipe

    cache = {}

    def get(R):
        if R not in cache:
            m = pm.CLC(N=64, num_ref_frames=R)
            apply_weight_recipe(m, 0)
            m = m.to(dev).eval()
            m.update(force=True)
            cache[R] = m
        return cache[R]

    return get


def _refs(dev):
    """six bank images of several sizes (keys as ReferenceIndex's feature_to_key would name them)"""
    from clc_amd.recipe import synthetic_image

    sizes = [(256, 256), (300, 200), (180, 260), (256, 256), (512, 384), (200, 300)]
    return {f"ref_{i:02d}.png": synthetic_image(1, h, w, 300 + i, smooth=True)[0].to(dev) for i, (h, w) in enumerate(sizes)}


def _ref_f64(img, hw):
    from clc_amd.eval import pad

    r = img.double().cpu()[None]
    if tuple(r.shape[-2:]) != tuple(hw):
        r = F.interpolate(r, size=tuple(hw), mode="bilinear", align_corners=False)
    return pad(r, 128)


def test_ref_prepare_matches_float64(dev):
    from clc_amd import ops

    g = torch.Generator().manual_seed(5)
    big, small, ident = (torch.rand(3, h, w, generator=g).to(dev) for h, w in ((512, 768), (180, 260), (341, 512)))
    for imgs, hw in (([big], (341, 512)), ([small], (200, 300)), ([ident], (341, 512)), ([big, ident, small], (341, 512))):
        out = ops.ref_prepare(imgs, hw)
        assert out.is_contiguous(memory_format=torch.channels_last)
        assert tuple(out.shape) == (len(imgs), 3, (hw[0] + 127) // 128 * 128, (hw[1] + 127) // 128 * 128)
        assert torch.equal(out, ops.ref_prepare(imgs, hw)), "two runs differ"
        for n, img in enumerate(imgs):
            want, (left, right, top, bottom) = _ref_f64(img, hw)
            got = out[n:n + 1].double().cpu()
            assert (got - want).abs().max().item() <= 1e-6, (n, hw, (got - want).abs().max().item())
            inner = torch.zeros_like(got, dtype=torch.bool)
            inner[..., top:got.shape[2] - bottom, left:got.shape[3] - right] = True
            assert torch.all(got[~inner] == 0), "padding is not exactly zero"
            if tuple(img.shape[-2:]) == tuple(hw):
                assert torch.equal(out[n:n + 1, :, top:top + hw[0], left:left + hw[1]].cpu(), img[None].cpu()), "identity is not a copy"
            assert torch.equal(ops.ref_prepare([img], hw)[0], out[n]), "an image alone differs from the same image inside a batch"


def test_gather_slots_matches_cat(dev):
    from clc_amd import ops

    arena = torch.randn(5, 320, 16, 16, device=dev).contiguous(memory_format=torch.channels_last)
    idx = torch.tensor([[0, 3, 3], [4, 0, 1], [3, 3, 2]], dtype=torch.int32)
    B, R = idx.shape
    out = ops.gather_slots(arena, idx.to(dev), B, R)
    want = torch.cat([arena[int(idx[b, r])][None] for r in range(R) for b in range(B)])
    assert out.is_contiguous(memory_format=torch.channels_last) and torch.equal(out, want)


def test_fingerprint_content_not_address(dev, models_by_R):
    from clc_amd import ops

    enc = models_by_R(1).ref_encoder
    ts = list(enc.parameters()) + list(enc.buffers())
    fp = ops.fingerprint(ts).item()
    assert ops.fingerprint([t.clone() for t in ts]).item() == fp, "same content at other addresses"
    assert ops.fingerprint(ts, n_partials=7).item() == fp, "depends on the grid"
    p = ts[len(ts) // 2]
    at = (0,) * p.dim()
    old = p.data[at].clone()
    try:
        p.data[at] = torch.nextafter(old, old + 1)       # one ulp, through p.data (no version-counter bump)
        assert ops.fingerprint(ts).item() != fp
    finally:
        p.data[at] = old
    assert ops.fingerprint(ts).item() == fp


def _tensor_refs(bank, rows, hw):
    prep = [bank.prepare(r, hw) for r in rows]
    R = len(rows[0])
    return prep, [torch.cat([p[j:j + 1] for p in prep]) for j in range(R)]


@pytest.mark.parametrize("R", [1, 3])
def test_bank_codec_end_to_end(dev, models_by_R, R):
    from clc_amd import codec, refbank
    from clc_amd.recipe import synthetic_image

    m = models_by_R(R)
    refs = _refs(dev)
    keys = list(refs)
    bank = refbank.ReferenceBank(m, refs)
    x = torch.cat([synthetic_image(1, 256, 256, 100 + i, smooth=True) for i in range(2)]).to(dev)
    rows = [[keys[1]], [keys[4]]] if R == 1 else [[keys[0], keys[2], keys[2]], [keys[5], keys[1], keys[3]]]
    hw = (256, 256)
    eng = codec.CodecEngine(m, threads=2)
    try:
        outs = eng.compress(x, ref_keys=rows, bank=bank)
        prep, ref_frames = _tensor_refs(bank, rows, hw)
        outs_t = eng.compress(x, ref_frames)
        for b in range(2):
            assert outs[b]["strings"] == outs_t[b]["strings"], f"image {b}: bank streams differ from the tensor path"
            assert outs[b]["ref_ids"] == [bank.index[k] for k in rows[b]] and outs[b]["bank_id"] == bank.bank_id
            assert tuple(outs[b]["image_hw"]) == hw
            eager = m._compress_eager(x[b:b + 1], [prep[b][j:j + 1] for j in range(R)])
            assert outs[b]["strings"] == eager["strings"], f"image {b}: bank streams differ from model._compress_eager"
        # containers decode with the bank alone
        items = [codec.unpack_item(codec.pack_item(o)) for o in outs]
        x_hat = eng.decompress(items, bank=bank)
        assert torch.equal(x_hat, eng.decompress(outs_t, ref_frames)), "bank decode differs from decoding with tensors"
        for b in range(2):
            want = m._decompress_eager(outs[b]["strings"], outs[b]["shape"], [prep[b][j:j + 1] for j in range(R)])["x_hat"]
            assert torch.equal(x_hat[b:b + 1], want), f"image {b}: bank decode differs from the encoder-side reconstruction"
        # warm cache: no new reference encodes
        misses = bank.stats["misses"]
        outs2 = eng.compress(x, ref_keys=rows, bank=bank)
        assert [o["strings"] for o in outs2] == [o["strings"] for o in outs] and bank.stats["misses"] == misses
        assert torch.equal(eng.decompress(outs2, bank=bank), x_hat)
        # a capacity that forces eviction: just the distinct keys of one call
        slot = 4 * 320 * 16 * 16
        small = refbank.ReferenceBank(m, refs, capacity_bytes=slot * len({k for r in rows for k in r}))
        other = [[keys[3]], [keys[0]]] if R == 1 else [[keys[4], keys[3], keys[0]], [keys[3], keys[4], keys[1]]]
        assert [o["strings"] for o in eng.compress(x, ref_keys=rows, bank=small)] == [o["strings"] for o in outs]
        eng.compress(x, ref_keys=other, bank=small)
        outs3 = eng.compress(x, ref_keys=rows, bank=small)
        assert small.stats["evictions"] > 0 and [o["strings"] for o in outs3] == [o["strings"] for o in outs]
        with pytest.raises(ValueError, match="capacity_bytes"):
            eng.compress(x, ref_keys=[rows[0], other[1]] if R == 1 else [rows[0], other[0]], bank=refbank.ReferenceBank(m, refs, capacity_bytes=slot))
    finally:
        eng.close()


def test_bank_stale_weights_and_other_bank(dev, models_by_R):
    from clc_amd import codec, refbank
    from clc_amd.recipe import synthetic_image

    m = models_by_R(1)
    refs = _refs(dev)
    keys = list(refs)
    bank = refbank.ReferenceBank(m, refs)
    x = synthetic_image(1, 256, 256, 150, smooth=True).to(dev)
    rows = [[keys[2]]]
    eng = codec.CodecEngine(m, threads=1)
    w = next(m.ref_encoder.parameters())
    old = w.data.clone()
    try:
        first = eng.compress(x, ref_keys=rows, bank=bank)[0]
        w.data.mul_(1.01)
        inv = bank.stats["invalidations"]
        got = eng.compress(x, ref_keys=rows, bank=bank)[0]
        want = m._compress_eager(x, [bank.prepare(rows[0], (256, 256))])
        assert bank.stats["invalidations"] == inv + 1
        assert got["strings"] == want["strings"], "the bank served latents of the old weights"
        assert got["strings"] != first["strings"]
        # another bank (same images, other key order): its id differs and the container is refused
        other = refbank.ReferenceBank(m, {k: refs[k] for k in reversed(keys)})
        item = codec.unpack_item(codec.pack_item(got))
        with pytest.raises(refbank.BankMismatch):
            eng.decompress([item], bank=other)
        bad = dict(item, meta=dict(item["meta"], ref_ids=[len(keys)]))
        with pytest.raises(ValueError, match="outside"):
            eng.decompress([bad], bank=bank)
    finally:
        w.data.copy_(old)
        eng.close()


def test_evaluate_with_bank_and_retrieval_keys(dev, models_by_R):
    import numpy as np

    from clc_amd import codec, eval as ev, refbank
    from clc_amd.recipe import synthetic_image
    from clc_amd.retrieval import ReferenceIndex

    m = models_by_R(1)
    # references of each query's size: both recipes are an exact copy plus padding, so the rows must agree exactly
    g = torch.Generator().manual_seed(9)
    refs = {f"r{i}": synthetic_image(1, 200, 300, 400 + i, smooth=True)[0] for i in range(4)}
    bank = refbank.ReferenceBank(m, refs)
    qs = [synthetic_image(1, 200, 300, 500 + i, smooth=True)[0] for i in range(2)]
    picks = [["r2"], ["r0"]]
    a = ev.evaluate(m, [(q, [refs[k[0]]]) for q, k in zip(qs, picks)])
    b = ev.evaluate(m, [(q, k) for q, k in zip(qs, picks)], bank=bank)
    assert a["rows"] == b["rows"]
    # ReferenceIndex keys go straight into compress(ref_keys=...)
    feats = torch.rand(4, 16, generator=g)
    index = ReferenceIndex(feats, feature_to_key={i: f"r{i}" for i in range(4)}, n_refs=1, device=dev)
    qk = index.query(torch.rand(2, 16, generator=g).numpy().astype(np.float32))
    x = torch.cat([ev.pad(q[None], 128)[0] for q in qs]).to(dev)
    eng = codec.CodecEngine(m, threads=2)
    try:
        outs = eng.compress(x, ref_keys=qk, bank=bank, image_hw=(200, 300))
        prep, ref_frames = _tensor_refs(bank, qk, (200, 300))
        assert [o["strings"] for o in outs] == [o["strings"] for o in eng.compress(x, ref_frames)]
        assert torch.equal(eng.decompress([codec.unpack_item(codec.pack_item(o)) for o in outs], bank=bank), eng.decompress(outs, ref_frames))
    finally:
        eng.close()
