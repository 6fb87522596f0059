"""The per-step images of the weights (clc_amd.train.StepImages) on CPU tensors: the entry tables of the four batched refreshes against
values written out from their formulas, who is handed which owner's images and when (ops._image / ops.WT_CACHE_VALID), and the use
collector the halo / Winograd selection reads.  No launch: the tables are decoded, never run."""
import ctypes as C

import pytest
import torch
import torch.nn as nn

CL = torch.channels_last


def _filter(*shape):
    t = torch.randn(*shape)
    p = nn.Parameter(t.contiguous(memory_format=CL) if t.dim() == 4 else t)
    p._clc_is_filter = True
    return p


class _Net(nn.Module):
    def __init__(self):
        super().__init__()
        from clc_amd import layers

        self.small, self.big, self.lin, self.idle = _filter(8, 4, 3, 3), _filter(256, 128, 3, 3), _filter(6, 10), _filter(16, 8, 3, 3)
        self.gdn = layers.GDN(8)


def _build(net=None):
    """the image set of _Net with a hand-written use set: `big` takes the halo kernel both ways and Winograd both ways, `small`
    Winograd forward only, `idle` nothing; the 2-D `lin` is named but is no 3x3 filter"""
    from clc_amd.train import StepImages

    net = net or _Net()
    live = list(net.parameters())
    uses = {(id(net.big), k) for k in ("halo", "halo_t", "wino", "wino_t")} | {(id(net.small), "wino"), (id(net.lin), "halo")}
    return net, live, StepImages(net, live, uses)


def _decode(part, struct):
    raw = bytes(part.table.numpy().tobytes())
    assert len(raw) == part.n * C.sizeof(struct)
    return [struct.from_buffer_copy(raw, i * C.sizeof(struct)) for i in range(part.n)]


def _disjoint(part, outs):
    """every output lies inside the part's buffer and no two overlap"""
    lo, hi = part.buf.data_ptr(), part.buf.data_ptr() + 4 * part.buf.numel()
    spans = sorted((t.data_ptr(), t.data_ptr() + 4 * t.numel()) for t in outs)
    assert spans[0][0] >= lo and spans[-1][1] <= hi
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))


def test_tables_match_the_formulas():
    from clc_amd import lib

    net, live, im = _build()
    assert [n for n, _ in net.named_parameters()] == ["small", "big", "lin", "idle", "gdn.beta", "gdn.gamma"]
    img = lambda p, kind: im.map.get((id(p), kind))

    # transpose: every filter, in `live` order; tile_begin accumulates T * ceil(Cout / 32) * ceil(Cin / 32)
    es = _decode(im.transposer, lib.TransposeEntry)
    want = [(net.small, 8, 9, 4, 0), (net.big, 256, 9, 128, 9), (net.lin, 6, 1, 10, 9 + 288), (net.idle, 16, 9, 8, 9 + 288 + 1)]
    assert im.transposer.total == 9 + 288 + 1 + 9 and im.transposer.buf.numel() == 288 + 294912 + 60 + 1152
    for e, (p, Cout, T, Cin, begin) in zip(es, want, strict=True):
        wt = img(p, "wt")
        assert (e.w, e.wt, e.Cout, e.T, e.Cin, e.tile_begin) == (p.data_ptr(), wt.data_ptr(), Cout, T, Cin, begin)
        assert tuple(wt.shape) == (Cin, T * Cout) and wt.is_contiguous()
    _disjoint(im.transposer, [img(p, "wt") for p, *_ in want])

    # halo: size rows * 9 * K, blocks (n // 4 + 255) // 256; forward job (the filter) before the transposed one (its [Cin][9][Cout] image)
    es = _decode(im.halo_packer, lib.HaloPackEntry)
    want = [(net.big, "halo", 256, 128, 0), (img(net.big, "wt"), "halo_t", 128, 256, 288)]
    assert im.halo_packer.total == 576 and im.halo_packer.buf.numel() == 2 * 294912
    for e, (src, kind, rows, K, begin) in zip(es, want, strict=True):
        out = img(net.big, kind)
        assert (e.w, e.out, e.N, e.K, e.block_begin) == (src.data_ptr(), out.data_ptr(), rows, K, begin)
        assert out.numel() == rows * 9 * K
    _disjoint(im.halo_packer, [img(net.big, k) for k in ("halo", "halo_t")])

    # Winograd: size ceil(rows / 128) * 128 * 16 * K, blocks (rows * K // 4 + 255) // 256, data gradients flipped
    es = _decode(im.wino_packer, lib.WinoEntry)
    want = [(net.small, net.small, "wino", 8, 4, 0, 0, 8192), (net.big, net.big, "wino", 256, 128, 0, 1, 524288),
            (net.big, img(net.big, "wt"), "wino_t", 128, 256, 1, 33, 524288)]
    assert im.wino_packer.total == 65 and im.wino_packer.buf.numel() == 8192 + 2 * 524288
    for e, (p, src, kind, rows, K, flip, begin, size) in zip(es, want, strict=True):
        out = img(p, kind)
        assert (e.w, e.out, e.N, e.K, e.flip, e.block_begin) == (src.data_ptr(), out.data_ptr(), rows, K, flip, begin)
        assert out.numel() == size
    _disjoint(im.wino_packer, [img(p, kind) for p, _, kind, *_ in want])

    # GDN: blocks (C * C + C + 255) // 256; the image is the (g_eff, g_eff_t, b_eff) triple, keyed by gamma
    (e,) = _decode(im.gdn_cache, lib.GDNEntry)
    g_eff, g_eff_t, b_eff = img(net.gdn.gamma, "gdn")
    assert (e.gamma, e.beta, e.gamma_eff, e.gamma_eff_t, e.beta_eff, e.C, e.first_block) == (
        net.gdn.gamma.data_ptr(), net.gdn.beta.data_ptr(), g_eff.data_ptr(), g_eff_t.data_ptr(), b_eff.data_ptr(), 8, 0)
    assert (e.gamma_bound, e.beta_bound, e.pedestal) == tuple(C.c_float(v).value for v in net.gdn._consts())
    assert im.gdn_cache.total == 1
    assert (tuple(g_eff.shape), tuple(g_eff_t.shape), tuple(b_eff.shape)) == ((8, 8), (8, 8), (8,))
    _disjoint(im.gdn_cache, [g_eff, g_eff_t, b_eff])

    # nothing else got an image: `small` only Winograd forward, `idle` no pack at all, the 2-D `lin` none despite being named a user
    assert {k: im.count(k) for k in ("wt", "halo", "halo_t", "wino", "wino_t", "gdn")} == dict(wt=4, halo=1, halo_t=1, wino=2, wino_t=1, gdn=1)
    assert len(im.map) == 10
    assert all(img(net.idle, k) is None and img(net.lin, k) is None for k in ("halo", "halo_t", "wino", "wino_t"))
    assert img(net.small, "halo") is None and img(net.small, "wino_t") is None


def test_a_part_without_jobs_has_no_table():
    from clc_amd.train import StepImages

    net = _Net()
    im = StepImages(net, [net.lin], set())
    assert [part.n for part in im.parts] == [1, 0, 0, 0]
    assert not any(hasattr(part, "table") for part in im.parts[1:])


def test_images_are_handed_out_by_owner_and_only_while_valid():
    from clc_amd import ops

    net, live, a = _build()
    _, _, b = _build(net)
    kinds = [(p, k) for p in live for k in ("wt", "halo", "halo_t", "wino", "wino_t", "gdn")]
    assert ops.WT_CACHE_VALID is False
    assert all(ops._image(p, k) is None for p, k in kinds)
    for own, other in ((a, b), (b, a)):
        with own.valid():
            assert ops.WT_CACHE_VALID is True
            for p, k in kinds:
                assert ops._image(p, k) is own.map.get((id(p), k))
            assert ops._image(net.big, "wt") is not other.map[(id(net.big), "wt")]
        assert ops.WT_CACHE_VALID is False
        assert all(ops._image(p, k) is None for p, k in kinds)
    with pytest.raises(ZeroDivisionError):
        with a.valid():
            1 / 0
    assert ops.WT_CACHE_VALID is False
    # outside code sets the plain flag after an owner's refresh: the set made current last answers
    b.make_current()
    ops.WT_CACHE_VALID = True
    try:
        assert ops._image(net.big, "halo") is b.map[(id(net.big), "halo")]
        ops.set_current_images(None)
        assert ops._image(net.big, "halo") is None
    finally:
        ops.WT_CACHE_VALID = False


def test_uses_are_recorded_only_into_an_installed_collector():
    from clc_amd import ops

    w = _filter(8, 4, 3, 3)
    assert ops.USES is None
    ops.note_use(w, "halo")          # nobody collects: nothing happens
    assert ops.USES is None
    with ops.collecting_uses() as outer:
        ops.note_use(w, "halo")
        with ops.collecting_uses() as inner:
            ops.note_use(w, "wino_t")
        ops.note_use(w, "halo_t")
    assert ops.USES is None
    assert outer == {(id(w), "halo"), (id(w), "halo_t")} and inner == {(id(w), "wino_t")}
    ops.note_use(w, "wino")
    assert len(outer) == 2 and len(inner) == 1
    with pytest.raises(ZeroDivisionError):
        with ops.collecting_uses():
            1 / 0
    assert ops.USES is None


def test_no_image_is_stored_on_a_parameter():
    net, live, im = _build()
    with im.valid():
        pass
    for p in net.parameters():
        assert {a for a in p.__dict__ if a.startswith("_clc_")} <= {"_clc_is_filter", "_clc_direct"}
