"""Container version 3 (clc_amd.codec, the reference bank's self-contained files) and bank ids (clc_amd.refbank), host side only."""
import struct

import pytest
import torch


def _item(ids=(3, 0, 7), bank_id=0xDEADBEEF, hw=(250, 380), kc=None):
    from clc_amd import codec

    it = {"strings": [[b"\x01\x02\x03" * 7], [b"\xfe" * 11]], "shape": torch.Size([4, 6]), "kernel_config": kc or codec.kernel_config()}
    if ids is not None:
        it.update(ref_ids=list(ids), bank_id=bank_id, image_hw=hw)
    return it


def test_v3_roundtrip_bytes_and_file(tmp_path):
    from clc_amd import codec

    it = _item()
    blob = codec.pack_item(it)
    assert blob[:4] == b"CLC1" and blob[4] == 3 and blob[6] == 3
    assert len(blob) == 28 + 4 + 3 * 4 + 11 + 21
    tag, h = it["kernel_config"]
    assert struct.unpack("<IIIII", blob[24:44]) == (h, 0xDEADBEEF, 3, 0, 7)
    strings, shape, meta = codec.unpack(blob)
    assert strings == it["strings"] and tuple(shape) == (4, 6)
    assert meta["bank_id"] == 0xDEADBEEF and meta["ref_ids"] == [3, 0, 7] and meta["n_refs"] == 3
    assert meta["image_hw"] == (250, 380) and meta["kernel_config_tag"] == tag and meta["kernel_config_hash"] == h
    assert meta["same_kernel_config"]
    item = codec.unpack_item(blob)
    assert item["meta"]["ref_ids"] == [3, 0, 7] and item["strings"] == it["strings"]
    # through a file: write_file with the same fields writes the same bytes
    n = codec.write_file(tmp_path / "a.clc", it["strings"], it["shape"], (250, 380), kernel_config_=it["kernel_config"], bank_id=0xDEADBEEF,
                         ref_ids=[3, 0, 7])
    assert n == len(blob) and (tmp_path / "a.clc").read_bytes() == blob
    s2, sh2, meta2 = codec.read_file(tmp_path / "a.clc")
    assert s2 == strings and tuple(sh2) == (4, 6) and meta2 == meta


def test_items_without_refs_pack_as_before():
    from clc_amd import codec

    for tag, ver in ((codec.kernel_config()[0], 1), (200, 2)):
        it = _item(ids=None, kc=(tag, 0x12345678))
        blob = codec.pack_item(it, (250, 380), n_refs=1, model_id=2)
        want = b"CLC1" + struct.pack("<BBBBHHHHII", ver, 2, 1, tag, 250, 380, 4, 6, 21, 11)
        if ver == 2:
            want += struct.pack("<I", 0x12345678)
        assert blob == want + it["strings"][1][0] + it["strings"][0][0]
        assert blob == codec.pack(it["strings"], it["shape"], (250, 380), 1, 2, it["kernel_config"])
        _, _, meta = codec.unpack(blob, strict=False)
        assert "bank_id" not in meta and "ref_ids" not in meta


def test_v3_malformed_refused():
    from clc_amd import codec

    blob = codec.pack_item(_item())
    codec.unpack(blob, strict=False)
    for bad in (blob[:-1], blob + b"\0", blob[:30], blob[:40]):          # truncated / oversized (header or streams)
        with pytest.raises(ValueError, match="truncated|oversized"):
            codec.unpack(bad, strict=False)
    for n in (2, 4, 0):                                                  # the id count no longer matches n_refs
        b = bytearray(blob)
        b[6] = n
        with pytest.raises(ValueError):
            codec.unpack(bytes(b), strict=False)
    with pytest.raises(ValueError):                                      # image_hw other than the one the bank prepared at
        codec.pack_item(_item(), (256, 384))
    with pytest.raises(ValueError):
        codec.pack_item(_item(), n_refs=2)


def test_bank_id_depends_on_key_order():
    from clc_amd import models, refbank

    a = refbank.bank_id_of(["k0", "k1", "k2"])
    assert a == refbank.bank_id_of(["k0", "k1", "k2"]) and 0 <= a < 1 << 32
    assert a != refbank.bank_id_of(["k1", "k0", "k2"])
    assert refbank.bank_id_of(["ab", "c"]) != refbank.bank_id_of(["a", "bc"])
    m = models.CLC(N=64, num_ref_frames=1)
    imgs = {k: torch.rand(3, 40, 50) for k in ("k0", "k1", "k2")}
    bank = refbank.ReferenceBank(m, imgs)
    assert bank.keys == ("k0", "k1", "k2") and bank.bank_id == a and bank.index["k2"] == 2
    assert refbank.ReferenceBank(m, {k: imgs[k] for k in ("k2", "k1", "k0")}).bank_id != a
    with pytest.raises(TypeError):
        refbank.ReferenceBank(m, {0: imgs["k0"]})
    with pytest.raises(KeyError):
        bank.prepare(["nope"], (40, 50))
