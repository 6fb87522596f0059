"""Batched, hipGraph-captured encoder / decoder service around the CLC / TCM models.

The reference codec (/root/reference/models/CLC_run.py:629-716, 738-814; eval loop /root/reference/eval_CLC.py:324-338) runs
~550 eager launches per 256x256 image, marshals symbols through Python lists, codes one image at a time and never writes a
file.  Same bitstreams, re-staged for the MI355X:

  compress    ONE captured graph per (batch, size, refs) signature: analysis + hyper transforms, the five slice steps and the
              integer quantise / index kernels -> packed int32 symbols + CDF indexes of every image, ONE device->host copy,
              then one rANS stream per image on host threads (the C++ coder runs outside the GIL).
              z_hat = round(z - median) + median is taken on the device — identical to decoding the z stream just written,
              which is what the reference does (CLC_run.py:643-644) — so nothing waits for the host coder.
  decompress  the slice loop is autoregressive THROUGH the arithmetic decoder (slice i's CDF indexes depend on the decoded
              slices < i), so a host decoder forces one device->host->device hop per slice; everything between two hops is one
              captured graph (6 graphs per signature), the hops use pinned buffers, and the images of a batch are decoded in
              parallel (one decoder state per image).
  lanes=W     the opt-in LANES format of the y string (include/clc_hip.h): W wave streams of 64 rANS lanes per image, the
              slices as segments in NHWC order.  compress codes y inside its graph (clc_rans_lanes_encode, clc_rans_lanes_pack: two
              device->host copies, the header with the z symbols and the packed words); decompress is ONE pinned upload and ONE
              replay of ONE graph with the coder inside every slice step (clc_rans_lanes_decode_gauss): no copy back, no
              synchronize; check=True adds one download of the coder's end states after the replay is issued.
  context     ContextCodecEngine: the same service for mbt2018 and mbt2018-checkerboard (models/hyperprior.py) on the lanes stream — ONE
  models      graph per compress (transforms, the encoder's whole schedule, the lanes encoder and pack) and ONE per decompress (h_s,
              every step's chain and clc_ar_lanes_decode, g_s); DESIGN 28.  The plan tables, their LRU, the capture and the lanes
              stream's host halves are _Engine's, shared by both engines.
  container   `pack` / `unpack` / `write_file` / `read_file`: a self-describing byte layout around {"strings", "shape"}
              (the reference only counts len(strings[k][0]), eval_CLC.py:337).
  sequence    `pack_sequence` / `unpack_sequence`: the CLV1 container of a coded video, what ScaleSpaceFlow.compress returns for a list
              of frames in either stream format (the end-to-end calls are clc_amd/frames.py's).

Streams are byte-identical to model.compress() per image (tests/test_codec_service_gpu.py), which in turn is pinned to the
reference's own compress() by tests/golden/codec_*.npz.
"""
from __future__ import annotations

import math
import struct
import time
from concurrent.futures import ThreadPoolExecutor
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import ans, ops
from .models import coding
from .ops import CL
from .refbank import BankMismatch  # noqa: F401  (raised by CodecEngine.decompress(items, bank=...))

MAGIC = b"CLC1"


# ------------------------------------------------------------------------------------------------ container


class KernelConfigMismatch(ValueError):
    """the container was written by context-model kernels of another summation order than the ones that would decode it"""


def kernel_config_tag() -> int:
    """Tag of the context-model kernels this process would run NOW (clc_kernel_config_tag: the build's kernel generation, or a hash of
    the order-affecting tuning keys when CLC_TUNING / clc_set_tuning / set_precision moved one off its default).  Never 0."""
    from . import lib

    return int(lib.load().clc_kernel_config_tag())


def kernel_config():
    """(tag, 32-bit hash) of the kernel state this process would run NOW.  compress() records it in its result WHEN THE KERNELS RAN, so a
    pack() after the caller restored another tuning / precision state still writes the state that encoded."""
    from . import lib

    L = lib.load()
    return int(L.clc_kernel_config_tag()), int(L.clc_kernel_config_hash()) & 0xFFFFFFFF


def pack(strings, shape, image_hw, n_refs: int = 0, model_id: int = 0, kernel_config_=None, bank_id=None, ref_ids=None) -> bytes:
    """One image: header + z stream + y stream.
    header (little endian): magic 'CLC1' | u8 version | u8 model_id | u8 n_refs | u8 kernel-config tag | u16 H | u16 W (original image) |
    u16 zh | u16 zw (hyper-latent shape = `shape`) | u32 len(y) | u32 len(z) [| u32 kernel-config hash: versions 2, 3]
    [| u32 bank_id | n_refs x u32 ref ids: version 3].
    The tag records which generation of context-model kernels encoded the image: the slice loop is autoregressive through the
    arithmetic decoder, so the decoder only stays in sync when it reproduces the encoder's means / scales bit for bit (the
    reference has the same property across devices and library versions; it records nothing).  Version 1 (24-byte header) under the
    build's default kernel state; version 2 (28 bytes) when an order-affecting tuning key was off its default at ENCODE time: the tag
    then holds 7 bits of a hash and the full 32 bits follow.  kernel_config_: the `kernel_config` entry of compress()'s result
    (default: the state at the time of this call).
    Version 3 (ref_ids given: the references of a clc_amd.refbank.ReferenceBank): the version-2 header, the hash always present, then
    the bank's id and one index into bank.keys per reference; H x W is the size the bank prepared the references at, so the file
    decodes with the bank alone (CodecEngine.decompress(items, bank=...)).
    Version 4 (pack_exact) is the stream of an integer entropy model and is bound to no kernel generation."""
    y, z = strings[0][0], strings[1][0]
    tag, h = kernel_config_ if kernel_config_ is not None else kernel_config()
    if ref_ids is not None:
        ids = [int(i) for i in ref_ids]
        if bank_id is None or not 0 <= int(bank_id) < 1 << 32 or not 0 < len(ids) < 256 or any(not 0 <= i < 1 << 32 for i in ids):
            raise ValueError(f"pack: version 3 needs a u32 bank_id and 1..255 u32 reference ids (got {bank_id}, {len(ids)} ids)")
        if n_refs not in (0, len(ids)):
            raise ValueError(f"pack: n_refs={n_refs} but {len(ids)} reference ids")
        head = MAGIC + struct.pack("<BBBBHHHHII", 3, model_id, len(ids), tag, image_hw[0], image_hw[1], int(shape[0]), int(shape[1]), len(y), len(z))
        head += struct.pack("<II", h, int(bank_id)) + struct.pack(f"<{len(ids)}I", *ids)
        return head + z + y
    ver = 2 if tag >= 128 else 1
    head = MAGIC + struct.pack("<BBBBHHHHII", ver, model_id, n_refs, tag, image_hw[0], image_hw[1], int(shape[0]), int(shape[1]), len(y), len(z))
    if ver == 2:
        head += struct.pack("<I", h)
    return head + z + y


def pack_exact(strings, shape, image_hw, spec_hash, model_id: int = 0) -> bytes:
    """VERSION 4: the stream of compress(x, exact=True), whose entropy parameters come from an integer net (clc_amd/intnet.py) and are
    the same bits under every kernel state and build.  The 28-byte version-2 header with tag byte 0 and, in the u32, the net's
    spec_hash — the name of the entropy model, not of a kernel generation: unpack does not call check_kernel_config for it."""
    if isinstance(spec_hash, bool) or not 0 <= int(spec_hash) < 1 << 32:
        raise ValueError(f"pack_exact: spec_hash must be a u32 (got {spec_hash!r})")
    y, z = strings[0][0], strings[1][0]
    head = MAGIC + struct.pack("<BBBBHHHHII", 4, model_id, 0, 0, image_hw[0], image_hw[1], int(shape[0]), int(shape[1]), len(y), len(z))
    return head + struct.pack("<I", int(spec_hash)) + z + y


def pack_item(item: dict, image_hw=None, n_refs=None, model_id: int = 0) -> bytes:
    """pack() of one compress() result, under the kernel state that result was ENCODED with.  A result of the bank path (it carries
    `ref_ids`, `bank_id`, `image_hw`) is written as version 3; image_hw then defaults to the item's and must equal it.  A result
    that carries "exact" (compress(x, exact=True)) is written as version 4 (pack_exact)."""
    if item.get("exact") is not None:
        if image_hw is None:
            raise ValueError("pack_item: image_hw is required for an item without reference ids")
        if item.get("ref_ids") is not None or n_refs:
            raise ValueError("pack_item: an exact item has no references (version 4 carries none)")
        return pack_exact(item["strings"], item["shape"], image_hw, item["exact"], model_id)
    ids = item.get("ref_ids")
    if ids is None:
        if image_hw is None:
            raise ValueError("pack_item: image_hw is required for an item without reference ids")
        return pack(item["strings"], item["shape"], image_hw, n_refs or 0, model_id, item.get("kernel_config"))
    ihw = item.get("image_hw")
    if image_hw is None:
        image_hw = ihw
    if image_hw is None or (ihw is not None and tuple(int(v) for v in image_hw) != tuple(int(v) for v in ihw)):
        raise ValueError(f"pack_item: image_hw {image_hw} is not the size {ihw} the bank prepared this item's references at")
    return pack(item["strings"], item["shape"], image_hw, n_refs or 0, model_id, item.get("kernel_config"), item["bank_id"], ids)


def check_kernel_config(meta, what="container"):
    """Raise KernelConfigMismatch unless `meta` (from unpack) carries the tag of the kernels that are about to decode.  Tag 0 (files
    written before the tag existed) never matches: those builds summed in other orders."""
    tag = int(meta.get("kernel_config_tag", 0))
    now, now_h = kernel_config()
    h = meta.get("kernel_config_hash")
    if tag != now or (h is not None and int(h) != now_h):
        raise KernelConfigMismatch(f"{what} was encoded under kernel-config tag {tag}" + (f" (hash {int(h):08x})" if h is not None else "") +
                                   f", this build / tuning state decodes under tag {now} (hash {now_h:08x}): the "
                                   "context model would leave the encoder's bit-exact means / scales and the arithmetic decoder would "
                                   "desynchronise silently.  Decode with the build (and CLC_TUNING / precision mode) that encoded, or "
                                   "pass strict=False to read the streams anyway.")


def unpack(blob: bytes, strict: bool = True):
    """-> (strings, shape, meta) as decompress() takes them.  strict (default): refuse a container whose kernel-config tag is not this
    build's (KernelConfigMismatch); strict=False returns it with meta["same_kernel_config"] = False for inspection.  Version 3 adds
    meta["bank_id"] and meta["ref_ids"].  Version 4 sets meta["exact_hash"] and meta["same_kernel_config"] = True and is never
    refused for its kernel state, under strict too: pass meta["exact_hash"] as decompress(..., exact=)."""
    if len(blob) < 24 or blob[:4] != MAGIC:
        raise ValueError("not a CLC1 container (shorter than its 24-byte header, or wrong magic)")
    ver, model_id, n_refs, tag, H, W, zh, zw, ny, nz = struct.unpack("<BBBBHHHHII", blob[4:24])
    if ver not in (1, 2, 3, 4):
        raise ValueError(f"unsupported container version {ver}")
    hl = {1: 24, 2: 28, 3: 32 + 4 * n_refs, 4: 28}[ver]
    if ver == 3 and n_refs == 0:
        raise ValueError("version-3 container without reference ids")
    if len(blob) != hl + ny + nz:
        raise ValueError("truncated / oversized container")
    z, y = blob[hl:hl + nz], blob[hl + nz:hl + nz + ny]
    if ver == 4:
        if tag != 0 or n_refs != 0:
            raise ValueError(f"version-4 container with kernel-config tag {tag} / {n_refs} references (both must be 0)")
        meta = {"image_hw": (H, W), "n_refs": 0, "model_id": model_id, "exact_hash": struct.unpack("<I", blob[24:28])[0], "same_kernel_config": True}
        return [[y], [z]], torch.Size([zh, zw]), meta
    now, now_h = kernel_config()
    meta = {"image_hw": (H, W), "n_refs": n_refs, "model_id": model_id, "kernel_config_tag": tag, "same_kernel_config": tag == now}
    if ver >= 2:
        meta["kernel_config_hash"] = struct.unpack("<I", blob[24:28])[0]
        meta["same_kernel_config"] = tag == now and meta["kernel_config_hash"] == now_h
    if ver == 3:
        meta["bank_id"] = struct.unpack("<I", blob[28:32])[0]
        meta["ref_ids"] = list(struct.unpack(f"<{n_refs}I", blob[32:hl]))
    if strict:
        check_kernel_config(meta)
    return [[y], [z]], torch.Size([zh, zw]), meta


def unpack_item(blob: bytes, strict: bool = True) -> dict:
    """unpack() as the dict CodecEngine.decompress takes; the header's meta rides along and is checked again where decoding starts."""
    strings, shape, meta = unpack(blob, strict)
    if "exact_hash" in meta:   # version 4: what model.decompress(..., exact=) takes
        return {"strings": strings, "shape": shape, "meta": meta, "exact": meta["exact_hash"]}
    return {"strings": strings, "shape": shape, "meta": meta}


def write_file(path, strings, shape, image_hw, n_refs=0, model_id=0, kernel_config_=None, bank_id=None, ref_ids=None):
    blob = pack(strings, shape, image_hw, n_refs, model_id, kernel_config_, bank_id, ref_ids)
    with open(path, "wb") as f:
        f.write(blob)
    return len(blob)


def read_file(path, strict: bool = True):
    with open(path, "rb") as f:
        return unpack(f.read(), strict)


# ------------------------------------------------------------------------------------- sequence container (ssf2020)
SEQ_MAGIC = b"CLV1"
_SEQ_HEAD = "<BBBBIHHHHHH"   # version, kernel-config tag, lanes, bit depth, kernel-config hash, frames, batch, H, W, Hp, Wp
_SEQ_HEAD_LEN = 4 + struct.calcsize(_SEQ_HEAD)


def _sequence_groups(t, strings):
    """frame t's string lists in the container's order: keyframe y, z; later frames motion y, z, residual y, z"""
    return [strings[0], strings[1]] if t == 0 else [strings["motion"][0], strings["motion"][1], strings["residual"][0], strings["residual"][1]]


def pack_sequence(frame_strings, shape_infos, *, lanes, image_hw, bit_depth=None, kernel_config_=None) -> bytes:
    """What ScaleSpaceFlow.compress returned -> one blob, little endian:

        b"CLV1" | u8 version = 1 | u8 kernel-config tag | u8 lanes (0: the default stream format) | u8 bit depth (0: not recorded) |
        u32 kernel-config hash | u16 frames | u16 batch | u16 H | u16 W (true size) | u16 Hp | u16 Wp (coded size, multiples of 128) |
        per frame, per string list (keyframe: y, z; later frames: motion y, z, residual y, z), per image: u32 length | bytes

    The z sizes are not stored: every one is (Hp / 128, Wp / 128).  kernel_config_: the state that encoded (default: this call's)."""
    F = len(frame_strings)
    if F < 1 or F != len(shape_infos) or F >= 1 << 16:
        raise ValueError(f"pack_sequence: frame count: {F} frame strings for {len(shape_infos)} shape infos (1 .. 65535 of each)")
    lanes_n = 0 if lanes is None else coding.lanes_count(lanes, "pack_sequence")
    bits = 0 if bit_depth is None else int(bit_depth)
    if bit_depth is not None and not 8 <= bits <= 16:
        raise ValueError(f"pack_sequence: bit_depth must be 8 .. 16 or None (got bit_depth={bit_depth!r})")
    zh, zw = (int(v) for v in shape_infos[0])
    H, W, Hp, Wp = int(image_hw[0]), int(image_hw[1]), 128 * zh, 128 * zw
    if not (0 < H <= Hp < 1 << 16 and 0 < W <= Wp < 1 << 16):
        raise ValueError(f"pack_sequence: image_hw {(H, W)} does not fit the coded size {(Hp, Wp)} (128 x the z size {(zh, zw)}; u16 fields)")
    for t in range(1, F):
        for k in ("motion", "residual"):
            if tuple(int(v) for v in shape_infos[t][k]) != (zh, zw):
                raise ValueError(f"pack_sequence: frame {t}'s {k} z size {tuple(shape_infos[t][k])} is not the keyframe's {(zh, zw)}")
    B = len(frame_strings[0][0])
    tag, h = kernel_config_ if kernel_config_ is not None else kernel_config()
    parts = [SEQ_MAGIC, struct.pack(_SEQ_HEAD, 1, tag & 0xFF, lanes_n, bits, h, F, B, H, W, Hp, Wp)]
    for t, strings in enumerate(frame_strings):
        for g, group in enumerate(_sequence_groups(t, strings)):
            if len(group) != B or not 0 < B < 1 << 16:
                raise ValueError(f"pack_sequence: frame {t}, string list {g} holds {len(group)} strings, the keyframe's y list {B} (the batch)")
            for s in group:
                parts += [struct.pack("<I", len(s)), bytes(s)]
    return b"".join(parts)


def unpack_sequence(blob: bytes, strict: bool = True):
    """-> (frame_strings, shape_infos, meta) as ScaleSpaceFlow.decompress takes them; meta: frames, batch, image_hw, padded_hw, lanes
    (None: the default format), bit_depth (None: not recorded), kernel_config_tag / _hash, same_kernel_config.  Refused by name: a
    wrong magic or version, a blob cut short, trailing bytes, a frame count that disagrees with the strings; strict (default) also
    another kernel state's blob (KernelConfigMismatch)."""
    blob = bytes(blob)
    if len(blob) < 4 or blob[:4] != SEQ_MAGIC:
        raise ValueError(f"unpack_sequence: wrong magic {blob[:4]!r}: not a {SEQ_MAGIC!r} sequence container")
    if len(blob) < _SEQ_HEAD_LEN:
        raise ValueError(f"unpack_sequence: the blob is cut short: {len(blob)} bytes, the header alone is {_SEQ_HEAD_LEN}")
    ver, tag, lanes_n, bits, h, F, B, H, W, Hp, Wp = struct.unpack(_SEQ_HEAD, blob[4:_SEQ_HEAD_LEN])
    if ver != 1:
        raise ValueError(f"unpack_sequence: unsupported version {ver} (this build reads version 1)")
    if F < 1 or B < 1 or Hp % 128 or Wp % 128 or not (0 < H <= Hp and 0 < W <= Wp) or lanes_n > ans.LANES_MAX_W or bits not in (0,) + tuple(range(8, 17)):
        raise ValueError(f"unpack_sequence: malformed header (frames {F}, batch {B}, size {(H, W)} in {(Hp, Wp)}, lanes {lanes_n}, bit depth {bits})")
    pos, shape = _SEQ_HEAD_LEN, torch.Size([Hp // 128, Wp // 128])
    frame_strings, shape_infos = [], []
    for t in range(F):
        if pos == len(blob):
            raise ValueError(f"unpack_sequence: the frame count {F} disagrees with the strings: the blob ends after {t} whole frames")
        groups = []
        for g in range(2 if t == 0 else 4):
            group = []
            for b in range(B):
                n = struct.unpack("<I", blob[pos:pos + 4])[0] if pos + 4 <= len(blob) else None
                if n is None or pos + 4 + n > len(blob):
                    raise ValueError(f"unpack_sequence: the blob is cut short inside frame {t}, string list {g}, image {b} (at byte {pos} of {len(blob)})")
                group.append(blob[pos + 4:pos + 4 + n])
                pos += 4 + n
            groups.append(group)
        if t == 0:
            frame_strings.append(groups)
            shape_infos.append(shape)
        else:
            frame_strings.append({"motion": groups[0:2], "residual": groups[2:4]})
            shape_infos.append({"motion": shape, "residual": shape})
    if pos != len(blob):
        raise ValueError(f"unpack_sequence: {len(blob) - pos} trailing bytes after the {F} frames the header counts")
    now, now_h = kernel_config()
    meta = {"frames": F, "batch": B, "image_hw": (H, W), "padded_hw": (Hp, Wp), "lanes": lanes_n or None, "bit_depth": bits or None,
            "kernel_config_tag": tag, "kernel_config_hash": h, "same_kernel_config": tag == (now & 0xFF) and h == now_h}
    if strict and not meta["same_kernel_config"]:
        raise KernelConfigMismatch(f"the sequence was encoded under kernel-config tag {tag} (hash {h:08x}), this build / tuning state decodes under "
                                   f"tag {now} (hash {now_h:08x}): the decoder would leave the encoder's bit-exact means / scales; pass "
                                   "strict=False to read the streams anyway")
    return frame_strings, shape_infos, meta


SEQ_Q_MAGIC = b"CLVQ"


def pack_sequence_q(blob: bytes, qs) -> bytes:
    """A CLV1 blob coded under per-frame qualities (variable rate) -> the wrapper, little endian:

        b"CLVQ" | u16 frames | frames x f32 q | the CLV1 blob as pack_sequence wrote it

    CLV1 itself is unchanged (its version stays 1): a reader that knows no qualities refuses the wrapper by its magic.  qs: one finite
    float per frame of the inner blob."""
    blob = bytes(blob)
    if len(blob) < _SEQ_HEAD_LEN or blob[:4] != SEQ_MAGIC:
        raise ValueError(f"pack_sequence_q: the inner blob is not a whole {SEQ_MAGIC!r} container (magic {blob[:4]!r}, {len(blob)} bytes)")
    F = struct.unpack(_SEQ_HEAD, blob[4:_SEQ_HEAD_LEN])[5]
    qs = [float(q) for q in qs]
    if len(qs) != F:
        raise ValueError(f"pack_sequence_q: {len(qs)} qualities for the {F} frames the inner header counts")
    if not all(math.isfinite(q) for q in qs):
        raise ValueError(f"pack_sequence_q: non-finite q in {qs}")
    return b"".join([SEQ_Q_MAGIC, struct.pack(f"<H{F}f", F, *qs), blob])


def unpack_sequence_q(blob: bytes):
    """-> (the inner CLV1 blob for unpack_sequence, [q per frame]).  Refused by name: a wrong magic, a blob cut short, a count that
    disagrees with the inner header, a non-finite q."""
    blob = bytes(blob)
    if len(blob) < 4 or blob[:4] != SEQ_Q_MAGIC:
        raise ValueError(f"unpack_sequence_q: wrong magic {blob[:4]!r}: not a {SEQ_Q_MAGIC!r} container")
    if len(blob) < 6:
        raise ValueError(f"unpack_sequence_q: the blob is cut short: {len(blob)} bytes, the frame count alone ends at byte 6")
    F = struct.unpack("<H", blob[4:6])[0]
    end = 6 + 4 * F
    if len(blob) < end + _SEQ_HEAD_LEN:
        raise ValueError(f"unpack_sequence_q: the blob is cut short: {len(blob)} bytes, {F} qualities and the inner header end at byte {end + _SEQ_HEAD_LEN}")
    qs = list(struct.unpack(f"<{F}f", blob[6:end]))
    inner = blob[end:]
    if inner[:4] != SEQ_MAGIC:
        raise ValueError(f"unpack_sequence_q: wrong inner magic {inner[:4]!r}: the wrapper holds a {SEQ_MAGIC!r} container")
    inner_frames = struct.unpack(_SEQ_HEAD, inner[4:_SEQ_HEAD_LEN])[5]
    if inner_frames != F:
        raise ValueError(f"unpack_sequence_q: the frame count {F} disagrees with the inner header's {inner_frames}")
    if not all(math.isfinite(q) for q in qs):
        raise ValueError(f"unpack_sequence_q: non-finite q in {qs}")
    return inner, qs


# --------------------------------------------------------------------------------------------------- engine


class _Plan:
    pass


def check_items(items, lanes):
    """What decompress refuses about its items before any device work: a "lanes" entry other than the call's, and another kernel state's
    container header (`meta`, from unpack_item) or `kernel_config` entry (from compress)."""
    for k, it in enumerate(items):
        if it.get("exact") is not None or "exact_hash" in (it.get("meta") or {}):
            raise ValueError(f"decompress: item {k} is an exact stream (integer entropy model, container version 4): the engines have no "
                             "integer parameter net — decode it with its model's own decompress(..., exact=) (ScaleHyperprior, "
                             "MeanScaleHyperprior, JointCheckerboardHierarchicalPriors)")
        if it.get("lanes") is not None and it["lanes"] != lanes:
            raise ValueError(f"decompress: item {k} was coded with lanes = {it['lanes']}, the call says lanes = {lanes}")
    if lanes is None:
        coding.refuse_lanes_strings([it["strings"][0][0] for it in items])
    for k, it in enumerate(items):      # items that came out of a container carry its header: refuse another kernel generation's
        if it.get("meta") is not None:
            check_kernel_config(it["meta"], f"item {k}")
        elif it.get("kernel_config") is not None and tuple(it["kernel_config"]) != kernel_config():
            raise KernelConfigMismatch(f"item {k} was encoded under kernel state {tuple(it['kernel_config'])}, this process now decodes under {kernel_config()}")


class _Engine:
    """What CodecEngine and ContextCodecEngine share: the coder threads, the plan tables and their LRU, the capture of a plan's function,
    the life cycle, and the two host halves of the lanes stream (the encoder's downloads, the decoder's upload and replay)."""

    def __init__(self, model, threads: int = 8, use_graph: bool = True, max_plans: int = 0):
        """max_plans > 0: keep at most that many captured signatures per direction (least recently used out first) — a data set of many
        image sizes would otherwise pin one graph memory pool per size for the engine's lifetime."""
        model.eval()
        self.model = model          # (may be a weakref.proxy: the engine a model builds for its own compress() must not keep the model alive)
        self.use_graph = use_graph
        self.pool = ThreadPoolExecutor(max_workers=max(1, threads))
        self._enc = {}
        self._dec = {}
        self.max_plans = int(max_plans)
        self._built_ms = 0.0   # building time of the plans the current call made (_plan)
        self.last = {}   # wall-clock split of the last compress() / decompress() call (ms): device segments incl. the hops' copies and waits | host rANS
        self.zc = int(model.entropy_bottleneck.channels)   # hyper-latent channels (192 in the reference configuration)
        model.update()   # CDF tables (no-op when present)

    def close(self):
        """Release the coder threads and the captured plans (graphs, their memory pools, pinned host buffers)."""
        if self.pool is not None:
            self.pool.shutdown(wait=True)
            self.pool = None
        self._enc.clear()
        self._dec.clear()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---------------------------------------------------------------- shared pieces
    def _plan(self, table, sig, build):
        pl = table.pop(sig, None)          # (re-inserted below: dict order = recency)
        if pl is None:
            while self.max_plans > 0 and len(table) >= self.max_plans:
                table.pop(next(iter(table)))   # least recently used: its graphs, pool and pinned buffers go with it (outside any capture)
            t0 = time.perf_counter()
            pl = build()
            self._built_ms += (time.perf_counter() - t0) * 1e3   # (warm-up passes and captures of the plans a call built)
        table[sig] = pl
        return pl

    def _capture(self, fn):
        """run fn() twice eagerly on a side stream (allocator / lazy kernel attributes), then capture it; -> (graph, outputs)."""
        if not self.use_graph:
            return None, fn()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            fn()
            fn()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with ops.capture_guard(), torch.cuda.graph(g, capture_error_mode=ops.graph_capture_mode()):
            out = fn()
        g.replay()   # capture does not execute: leave valid values behind for the next segment's warm-up passes
        return g, out

    def _last_extras(self, last, pl):
        """what an engine adds to `last` about the plan a call ran"""
        return last

    # ---------------------------------------------------------------- the lanes stream's host halves
    def _lanes_encoder_host(self, pl):
        """a lanes encoder plan's host side: the pinned header twin and the z indexes (pl.packed = (small, packed words), pl.zshape)"""
        pl.small_host = torch.empty(pl.packed[0].shape, dtype=torch.int32).pin_memory()
        pl.words_host = None   # pinned, grown to the largest total seen
        C = self.zc
        pl.zidx = np.ascontiguousarray(np.broadcast_to(np.arange(C, dtype=np.int32).reshape(C, 1, 1), (C,) + pl.zshape)).reshape(-1)
        return pl

    def _finish_lanes_encoder(self, pl, t0):
        """the host half of compress(lanes=W): the header copy (counts, total, z symbols), the copy of `total` words, the containers"""
        small, packed = pl.packed
        B, W = pl.x.shape[0], pl.lanes
        stream = torch.cuda.current_stream()
        pl.small_host.copy_(small, non_blocking=True)
        stream.synchronize()
        head = pl.small_host.numpy()
        total = int(head[B * W])
        if total > packed.numel():
            raise ValueError(f"compress: the wave streams hold {total} words, the packed buffer {packed.numel()}")
        if pl.words_host is None or pl.words_host.numel() < total:
            pl.words_host = torch.empty((max(total, 1) * 5 // 4 + 1024,), dtype=torch.int32).pin_memory()
        if (head[:B * W] >= 0).all():
            pl.words_host[:total].copy_(packed[:total], non_blocking=True)
            stream.synchronize()
        t1 = time.perf_counter()
        ys = coding.lanes_strings(head, pl.words_host.numpy()[:total], B, W)   # (raises by name on a negative code)
        ecdf, eln, eoff = self.model.entropy_bottleneck.host_tables()
        zsym = head[B * W + 1:].reshape(B, -1)
        enc_z = lambda b: ans.encode(zsym[b], pl.zidx, ecdf, eln, eoff)
        zs = list(self.pool.map(enc_z, range(B))) if B > 1 else [enc_z(0)]
        self.last = self._last_extras({"op": "compress", "device_ms": (t1 - t0) * 1e3, "rans_ms": (time.perf_counter() - t1) * 1e3, "hops": 2,
                                       "lanes": W}, pl)
        return [{"strings": [[y], [z]], "shape": torch.Size(pl.zshape), "kernel_config": pl.kernel_config, "lanes": W} for y, z in zip(ys, zs)]

    def _lanes_decoder_buffers(self, pl, B, zshape, dev, W, cap_words):
        """a lanes decoder plan's inputs at fixed device addresses, with their pinned twins: the z symbols and the upload image
        [states | spans | cap_words words] (coding.stream_image), whose views the plan's graph reads"""
        pl.lanes, pl.cap_words = W, int(cap_words)
        pl.z_in = torch.zeros((B, self.zc) + tuple(zshape), dtype=torch.int32, device=dev)
        pl.z_host = torch.empty(pl.z_in.shape, dtype=torch.int32).pin_memory()
        n_state = 2 * ans.LANES
        size = (n_state + 4) * B * W + pl.cap_words
        pl.image = torch.zeros((size,), dtype=torch.int32, device=dev)   # (all zero: empty spans, which read nothing)
        pl.image_host = torch.zeros((size,), dtype=torch.int32).pin_memory()
        pl.state, pl.spans, pl.words = coding.stream_views(pl.image, B, W, n_state)

    lanes_words_slack = 1.5   # a lanes decoder plan's words buffer holds this multiple of what the batch that built it needed

    def _decompress_lanes(self, items, pl_for, W, check):
        """decompress(lanes=W) behind the argument checks; pl_for(cap_words, rebuild) -> the plan"""
        m = self.model
        B = len(items)
        tm = time.perf_counter()
        subs = coding.lanes_parse([it["strings"][0][0] for it in items], W)   # the headers, before any device work
        image = coding.stream_image(subs, 2 * ans.LANES)
        head = (2 * ans.LANES + 4) * B * W
        need = image.size - head
        pl = pl_for(max(need, int(need * self.lanes_words_slack)), False)
        rebuilt = False
        if getattr(pl, "uploaded", None) is not None:
            pl.uploaded.synchronize()   # the previous call's uploads (not its graph) may still be reading the pinned pages written below
        if need > pl.cap_words:   # never truncated: a larger buffer, a new graph
            pl = pl_for(max(need, int(need * self.lanes_words_slack)), True)
            rebuilt = True
        ecdf, eln, eoff = m.entropy_bottleneck.host_tables()
        C = self.zc
        zshape = tuple(pl.z_in.shape[2:])
        zidx = np.ascontiguousarray(np.broadcast_to(np.arange(C, dtype=np.int32).reshape(C, 1, 1), (C,) + zshape)).reshape(-1)
        zh = pl.z_host.numpy()

        def dec_z(b):
            zh[b] = ans.decode(items[b]["strings"][1][0], zidx, ecdf, eln, eoff).reshape(zh.shape[1:])

        if B > 1:
            list(self.pool.map(dec_z, range(B)))
        else:
            dec_z(0)
        t_rans = time.perf_counter() - tm
        tm = time.perf_counter()
        pl.image_host.numpy()[:image.size] = image
        pl.z_in.copy_(pl.z_host, non_blocking=True)
        pl.image[:image.size].copy_(pl.image_host[:image.size], non_blocking=True)   # THE upload: states, spans, words
        if getattr(pl, "uploaded", None) is None:
            pl.uploaded = torch.cuda.Event()
        pl.uploaded.record()
        if pl.graph is not None:
            pl.graph.replay()
            res = pl.out.clone()
        else:
            res = pl.run()
        self.last = self._last_extras({"op": "decompress", "device_ms": 0.0, "rans_ms": t_rans * 1e3, "hops": 1 if check else 0, "lanes": W,
                                       "tail_issue_ms": (time.perf_counter() - tm) * 1e3, "plan_rebuilt": rebuilt}, pl)
        if check:   # ONE download, after everything has been issued
            coding.lanes_check(pl.state, subs)
        return res


class CodecEngine(_Engine):
    """engine = CodecEngine(model); outs = engine.compress(x[B], refs); xs = engine.decompress(outs, refs)."""

    def _sig(self, x, refs):
        # (the kernel state is part of the signature: a captured graph keeps the kernels it was captured with, so a changed tuning /
        #  precision state must not replay the old plan — and the result's `kernel_config` must be the one that encoded)
        return (tuple(x.shape), None if refs is None else tuple(tuple(r.shape) for r in refs), kernel_config())

    # ---------------------------------------------------------------- encoder
    def _bank_slots(self, pl, arena, slots):
        """bank plans: the arena the graphs gather from and the slot table they read (device memory, refreshed per call from pinned memory)."""
        pl.arena = arena
        pl.slot_idx = torch.tensor(slots, dtype=torch.int32).to(arena.device)
        pl.slot_host = torch.empty(pl.slot_idx.shape, dtype=torch.int32).pin_memory()
        pl.R = len(slots[0])

    def _set_slots(self, pl, arena, slots):
        if pl.arena is not arena:   # (arenas are never reallocated: a plan only ever meets the one it was captured with)
            raise RuntimeError("CodecEngine: the bank's arena moved under a captured plan")
        pl.slot_host.numpy()[...] = slots
        pl.slot_idx.copy_(pl.slot_host, non_blocking=True)

    def _bank_features(self, pl):
        """reference features of a bank plan: the gathered latents [R*B, M, h, w] into the unchanged tail of CLC._ref."""
        B = pl.slot_idx.shape[0]
        return self.model._ref_from_latents(ops.gather_slots(pl.arena, pl.slot_idx, B, pl.R), pl.R)

    def _build_encoder(self, x, refs, bank=None, lanes=None):
        m = self.model
        pl = _Plan()
        pl.lanes = lanes
        pl.kernel_config = kernel_config()
        pl.x = x.clone()
        pl.refs = [r.clone() for r in refs] if refs is not None else None
        if bank is not None:
            self._bank_slots(pl, *bank)
        B = x.shape[0]
        S = m.num_slices

        @torch.no_grad()
        def run():
            xx = m._prep(pl.x)
            ref_features = self._bank_features(pl) if bank is not None else m._ref(pl.refs)
            y = m.g_a(xx)
            y_shape = y.shape[2:]
            z = m._fuse_z(m.h_a(y))
            eb = m.entropy_bottleneck
            med = eb._get_medians().reshape(1, -1, 1, 1)
            z_sym = torch.round(z - med).to(torch.int32)                    # == EntropyBottleneck.compress's symbols
            z_hat = (z_sym.float() + med).contiguous(memory_format=CL)      # == decompress(compress(z)), CLC_run.py:643-644
            latent_scales = m.h_scale_s(z_hat)
            latent_means = m.h_mean_s(z_hat)
            syms, idxs, y_hat_slices = [], [], []
            for i, y_slice in enumerate(y.chunk(S, 1)):
                mean_support, mu, scale = m._slice_params(i, latent_means, latent_scales, y_hat_slices, ref_features, y_shape)
                sym, idx, y_hat_slice = m.gaussian_conditional.quantize_and_index(y_slice, mu, scale)
                # (sym, idx: NCHW views of NHWC int32 buffers — the lanes stream takes them as they lie, the default in NCHW order)
                syms.append(sym if lanes is not None else sym.contiguous())
                idxs.append(idx if lanes is not None else idx.contiguous())
                y_hat_slices.append(m._refine(i, mean_support, y_hat_slice, ref_features))
            if lanes is not None:
                return self._lanes_encode(pl, syms, idxs, z_sym.contiguous().reshape(B, -1)), tuple(z.shape[-2:])
            # per image contiguous: [B][slice][C/S][h][w] in the reference's NCHW reshape(-1) order
            ys = torch.stack(syms, dim=1).reshape(B, -1)
            yi = torch.stack(idxs, dim=1).reshape(B, -1)
            zs = z_sym.contiguous().reshape(B, -1)
            return torch.cat((ys, yi, zs), dim=1), tuple(z.shape[-2:])

        pl.graph, (pl.packed, pl.zshape) = self._capture(run)
        pl.run = run
        if lanes is not None:
            return self._lanes_encoder_host(pl)
        pl.host =torch.empty(pl.packed.shape, dtype=torch.int32).pin_memory()
        pl.ny = (pl.packed.shape[1] - self.zc * pl.zshape[0] * pl.zshape[1]) // 2
        C = self.zc
        pl.zidx = np.ascontiguousarray(np.broadcast_to(np.arange(C, dtype=np.int32).reshape(C, 1, 1), (C,) + pl.zshape)).reshape(-1)
        return pl

    def _lanes_encode(self, pl, syms, idxs, zs):
        """inside the encoder's graph: the slices' NHWC symbol / index buffers stacked to [B][T], clc_rans_lanes_encode over the slices as
        segments, clc_rans_lanes_pack -> (small = [B W counts | total | z symbols], the packed words)"""
        gc = self.model.gaussian_conditional
        B, W = zs.shape[0], pl.lanes
        flat = lambda ts: torch.cat([t.permute(0, 2, 3, 1).reshape(B, -1) for t in ts], dim=1)   # (views of the NHWC int32 buffers)
        ys, yi = flat(syms), flat(idxs)
        segments = [int(t[0].numel()) for t in syms]
        if getattr(pl, "regions", None) is None:   # (outside the capture: the first warm-up pass)
            pl.regions = ops.rans_lanes_regions(segments, W, B)
            pl.regions_dev = torch.from_numpy(pl.regions).to(zs.device)
        out, _, result = ops.rans_lanes_encode(ys, yi, segments, W, (gc._quantized_cdf, gc._cdf_length, gc._offset), regions=pl.regions,
                                               regions_dev=pl.regions_dev)
        small = torch.empty((B * W + 1 + zs.numel(),), device=zs.device, dtype=torch.int32)
        packed, _ = ops.rans_lanes_pack(out, result, header=small[:B * W + 1])
        small[B * W + 1:].copy_(zs.reshape(-1))
        return small, packed

    def _bank_model(self, bank):
        m = self.model
        if not getattr(m, "use_ref", True) or not hasattr(m, "ref_encoder"):
            raise ValueError("CodecEngine: a reference bank needs a model that codes with references (CLC, use_ref=True)")
        if bank.model.ref_encoder is not m.ref_encoder:
            raise ValueError("CodecEngine: the bank was built for another model")

    @torch.no_grad()
    def compress(self, x, ref_frames: Optional[Sequence[torch.Tensor]] = None, *, ref_keys=None, bank=None, image_hw=None,
                 lanes=None) -> List[dict]:
        """x [B,3,H,W] (H, W multiples of 128 after eval.pad) -> one {"strings": [[y], [z]], "shape"} per image.
        Bank path (clc_amd.refbank.ReferenceBank): ref_keys = one list of R bank keys per image, image_hw = the size the references are
        resized to before padding (default: x's); the latents come from the bank's cache and the results carry `ref_ids` (indexes into
        bank.keys), `bank_id` and `image_hw` besides, which pack_item() writes as a version-3 container.
        lanes=W (1 .. 16): the y strings in the lanes format, coded on the device inside the graph; the results carry "lanes": W, which
        decompress must be given.  The z strings are the default's."""
        Wn = coding.lanes_count(lanes, "CodecEngine.compress")
        if bank is not None or ref_keys is not None:
            return self._compress_bank(x, ref_frames, ref_keys, bank, image_hw, Wn)
        refs = list(ref_frames) if ref_frames else None
        if not getattr(self.model, "use_ref", True) or not hasattr(self.model, "ref_encoder"):
            refs = None
        sig = self._sig(x, refs) if Wn is None else self._sig(x, refs) + (("lanes", Wn),)
        pl = self._plan(self._enc, sig, lambda: self._build_encoder(x, refs, lanes=Wn))
        return self._run_encoder(pl, x, refs)

    def _compress_bank(self, x, ref_frames, ref_keys, bank, image_hw, lanes=None):
        if bank is None or ref_keys is None or ref_frames:
            raise ValueError("CodecEngine.compress: the bank path takes ref_keys AND bank, and no ref_frames")
        self._bank_model(bank)
        B = x.shape[0]
        rows = [list(r) for r in ref_keys]
        if len(rows) != B or len({len(r) for r in rows}) != 1:
            raise ValueError(f"CodecEngine.compress: ref_keys must hold one list of R keys per image ({B} images), got {[len(r) for r in rows]}")
        hw = tuple(int(v) for v in (image_hw if image_hw is not None else x.shape[-2:]))
        if ((hw[0] + 127) // 128 * 128, (hw[1] + 127) // 128 * 128) != tuple(x.shape[-2:]):
            raise ValueError(f"CodecEngine.compress: image_hw {hw} does not pad to the input's size {tuple(x.shape[-2:])}")
        arena, slots = bank.lookup(rows, hw)
        sig = (tuple(x.shape), len(rows[0]), bank, kernel_config()) + (() if lanes is None else (("lanes", lanes),))
        pl = self._plan(self._enc, sig, lambda: self._build_encoder(x, None, (arena, slots), lanes=lanes))
        self._set_slots(pl, arena, slots)
        outs = self._run_encoder(pl, x, None)
        for o, r in zip(outs, rows):
            o.update(ref_ids=[bank.index[k] for k in r], bank_id=bank.bank_id, image_hw=hw)
        return outs

    def _run_encoder(self, pl, x, refs):
        t0 = time.perf_counter()
        pl.x.copy_(x, non_blocking=True)
        if refs is not None:
            for d, r in zip(pl.refs, refs):
                d.copy_(r, non_blocking=True)
        if pl.graph is not None:
            pl.graph.replay()
        else:
            pl.packed, _ = pl.run()
        if pl.lanes is not None:
            return self._finish_lanes_encoder(pl, t0)
        pl.host.copy_(pl.packed, non_blocking=True)
        torch.cuda.current_stream().synchronize()        # the ONE device->host hop of the encoder
        t1 = time.perf_counter()
        arr = pl.host.numpy()
        gcdf, gln, goff = self.model.gaussian_conditional.host_tables()
        ecdf, eln, eoff = self.model.entropy_bottleneck.host_tables()
        ny = pl.ny

        def encode_one(b):
            row = arr[b]
            return (ans.encode(row[:ny], row[ny:2 * ny], gcdf, gln, goff), ans.encode(row[2 * ny:], pl.zidx, ecdf, eln, eoff))

        streams = list(self.pool.map(encode_one, range(arr.shape[0]))) if arr.shape[0] > 1 else [encode_one(0)]
        self.last = {"op": "compress", "device_ms": (t1 - t0) * 1e3, "rans_ms": (time.perf_counter() - t1) * 1e3, "hops": 1}
        # (a replayed graph holds the kernels of the state it was CAPTURED under: plans are keyed by it, see _sig)
        return [{"strings": [[ys], [zs]], "shape": torch.Size(pl.zshape), "kernel_config": pl.kernel_config} for ys, zs in streams]

    # ---------------------------------------------------------------- decoder
    def _build_decoder_lanes(self, B, zshape, refs, dev, W, cap_words, bank=None):
        """The lanes decoder: ONE graph — hyper-synthesis, per slice the parameter nets, clc_rans_lanes_decode_gauss and the refinement,
        the synthesis transform — over a plan-owned upload image [states | spans | cap_words words] at a fixed device address."""
        m = self.model
        S = m.num_slices
        pl = _Plan()
        pl.refs = [r.clone() for r in refs] if refs is not None else None
        if bank is not None:
            self._bank_slots(pl, *bank)
        self._lanes_decoder_buffers(pl, B, zshape, dev, W, cap_words)
        y_shape = [zshape[0] * 4, zshape[1] * 4]
        gc = m.gaussian_conditional
        tables = (gc._quantized_cdf, gc._cdf_length, gc._offset)

        @torch.no_grad()
        def run():
            ref = self._bank_features(pl) if bank is not None else m._ref(pl.refs)
            med = m.entropy_bottleneck._get_medians().reshape(1, -1, 1, 1)
            z_hat = (pl.z_in.float() + med).contiguous(memory_format=CL)
            ls = m.h_scale_s(z_hat)
            lm = m.h_mean_s(z_hat)
            y_hat = []
            for i in range(S):
                mean_support, mu, scale = m._slice_params(i, lm, ls, y_hat, ref, y_shape)
                y_hat_slice = ops.rans_lanes_decode_gauss(scale, mu, gc.scale_table, tables, pl.words, pl.spans, pl.state)
                y_hat.append(m._refine(i, mean_support, y_hat_slice, ref))
            return m.g_s(torch.cat(y_hat, dim=1)).clamp_(0, 1)

        pl.graph, pl.out = self._capture(run)
        pl.run = run
        return pl

    def _build_decoder(self, B, zshape, refs, dev, bank=None):
        m = self.model
        S = m.num_slices
        pl = _Plan()
        pl.refs = [r.clone() for r in refs] if refs is not None else None
        if bank is not None:
            self._bank_slots(pl, *bank)
        pl.z_in = torch.zeros((B, self.zc) + tuple(zshape), dtype=torch.int32, device=dev)
        yh, yw = zshape[0] * 4, zshape[1] * 4
        Cs = m.M // S
        pl.rv_in = [torch.zeros((B, Cs, yh, yw), dtype=torch.int32, device=dev) for _ in range(S)]
        pl.z_host = torch.empty(pl.z_in.shape, dtype=torch.int32).pin_memory()
        pl.rv_host = [torch.empty(t.shape, dtype=torch.int32).pin_memory() for t in pl.rv_in]
        pl.idx_host = [torch.empty(t.shape, dtype=torch.int32).pin_memory() for t in pl.rv_in]
        # per-slice state, indexed by slice: a segment only ever reads entries written by EARLIER segments' captured runs and
        # writes its own entries, so the eager warm-up passes of one segment cannot disturb what another segment's graph reads
        st = {"y_hat": [None] * S, "ms": [None] * S, "mu": [None] * S}
        y_shape = [yh, yw]
        gc = m.gaussian_conditional

        @torch.no_grad()
        def params(i):
            mean_support, mu, scale = m._slice_params(i, st["lm"], st["ls"], st["y_hat"][:i], st["ref"], y_shape)
            st["ms"][i], st["mu"][i] = mean_support, mu
            return gc.build_indexes(scale).contiguous()

        @torch.no_grad()
        def refine(i):
            rv = pl.rv_in[i].float().contiguous(memory_format=CL)
            st["y_hat"][i] = m._refine(i, st["ms"][i], rv + st["mu"][i], st["ref"])

        @torch.no_grad()
        def seg_first():
            st["ref"] = self._bank_features(pl) if bank is not None else m._ref(pl.refs)
            med = m.entropy_bottleneck._get_medians().reshape(1, -1, 1, 1)
            z_hat = (pl.z_in.float() + med).contiguous(memory_format=CL)
            st["ls"] = m.h_scale_s(z_hat)
            st["lm"] = m.h_mean_s(z_hat)
            return params(0)

        def seg_mid(i):
            def fn():
                refine(i - 1)
                return params(i)
            return fn

        @torch.no_grad()
        def seg_last():
            refine(S - 1)
            return m.g_s(torch.cat(st["y_hat"], dim=1)).clamp_(0, 1)

        pl.segs = []
        for fn in [seg_first] + [seg_mid(i) for i in range(1, S)] + [seg_last]:
            g, out = self._capture(fn)
            pl.segs.append((g, fn, out))
        return pl

    def _bank_rows(self, items, bank, zshape):
        """(key rows, image_hw) of bank items (compress() results of the bank path or unpack_item()ed version-3 containers)."""
        rows, hws = [], set()
        for k, it in enumerate(items):
            meta = it.get("meta") or {}
            ids = it.get("ref_ids", meta.get("ref_ids"))
            bid = it.get("bank_id", meta.get("bank_id"))
            hw = it.get("image_hw", meta.get("image_hw"))
            if ids is None or bid is None or hw is None:
                raise ValueError(f"item {k} names no bank references (encode with compress(..., ref_keys=, bank=) / a version-3 container)")
            if int(bid) != bank.bank_id:
                raise BankMismatch(f"item {k} was encoded against bank {int(bid):08x}, this bank is {bank.bank_id:08x} ({len(bank.keys)} keys): "
                                   "its reference ids would name other images")
            bad = [i for i in ids if not 0 <= int(i) < len(bank.keys)]
            if bad:
                raise ValueError(f"item {k}: reference ids {bad} are outside the bank's {len(bank.keys)} keys")
            rows.append([bank.keys[int(i)] for i in ids])
            hws.add((int(hw[0]), int(hw[1])))
        if len(hws) != 1 or len({len(r) for r in rows}) != 1:
            raise ValueError(f"decompress: the items of one call share one image size and one reference count, got {sorted(hws)}")
        hw = hws.pop()
        if ((hw[0] + 127) // 128 * 128, (hw[1] + 127) // 128 * 128) != (zshape[0] * 64, zshape[1] * 64):
            raise ValueError(f"decompress: image size {hw} does not pad to the streams' {zshape[0] * 64}x{zshape[1] * 64}")
        return rows, hw

    @torch.no_grad()
    def decompress(self, items: Sequence[dict], ref_frames: Optional[Sequence[torch.Tensor]] = None, *, bank=None, lanes=None,
                   check=True) -> torch.Tensor:
        """items: outputs of compress() (or unpack_item()ed containers, whose kernel-config tag is checked here) for B images of one shape -> x_hat [B,3,H,W] clamped to [0,1].
        bank: decode items of the bank path without reference tensors: their ref ids name the bank's keys (BankMismatch for another
        bank's id), the bank prepares and encodes (or finds cached) the references itself.
        lanes=W: the items of compress(lanes=W).  Their headers are parsed and z is decoded on the host; then one pinned upload and ONE
        graph replay, no copy back, no synchronize (self.last["hops"] == 0).  check=True (default; lanes only) downloads the coder's end
        states once, after the replay is issued, and raises ValueError naming the image and the wave streams that did not end where a
        whole stream ends (hops == 1).  Refused by name: lanes outside 1 .. 16 or other than an item's "lanes" / header, a lanes
        string without lanes=, a default string with it."""
        m = self.model
        Wn = coding.lanes_count(lanes, "CodecEngine.decompress")
        check_items(items, Wn)
        B = len(items)
        zshape = tuple(int(v) for v in items[0]["shape"])
        dev = next(m.parameters()).device
        if bank is not None:
            if ref_frames:
                raise ValueError("CodecEngine.decompress: pass ref_frames or bank, not both")
            self._bank_model(bank)
            rows, hw = self._bank_rows(items, bank, zshape)
            arena, slots = bank.lookup(rows, hw)
            sig = (B, zshape, len(rows[0]), bank, kernel_config())
            if Wn is not None:
                def pl_for(cap, rebuild):
                    if rebuild:
                        self._dec.pop(sig + (("lanes", Wn),), None)
                    pl = self._plan(self._dec, sig + (("lanes", Wn),), lambda: self._build_decoder_lanes(B, zshape, None, dev, Wn, cap, (arena, slots)))
                    self._set_slots(pl, arena, slots)
                    return pl
                return self._decompress_lanes(items, pl_for, Wn, check)
            pl = self._plan(self._dec, sig, lambda: self._build_decoder(B, zshape, None, dev, (arena, slots)))
            self._set_slots(pl, arena, slots)
            refs = None
        else:
            refs = list(ref_frames) if ref_frames else None
            if not getattr(m, "use_ref", True) or not hasattr(m, "ref_encoder"):
                refs = None
            sig = (B, zshape, None if refs is None else tuple(tuple(r.shape) for r in refs), kernel_config())
            if Wn is not None:
                def pl_for(cap, rebuild):
                    if rebuild:
                        self._dec.pop(sig + (("lanes", Wn),), None)
                    pl = self._plan(self._dec, sig + (("lanes", Wn),), lambda: self._build_decoder_lanes(B, zshape, refs, dev, Wn, cap))
                    if refs is not None:
                        for d, r in zip(pl.refs, refs):
                            d.copy_(r, non_blocking=True)
                    return pl
                return self._decompress_lanes(items, pl_for, Wn, check)
            pl = self._plan(self._dec, sig, lambda: self._build_decoder(B, zshape, refs, dev))
        if refs is not None:
            for d, r in zip(pl.refs, refs):
                d.copy_(r, non_blocking=True)
        gcdf, gln, goff = m.gaussian_conditional.host_tables()
        ecdf, eln, eoff = m.entropy_bottleneck.host_tables()
        C = self.zc
        zidx = np.ascontiguousarray(np.broadcast_to(np.arange(C, dtype=np.int32).reshape(C, 1, 1), (C,) + zshape)).reshape(-1)
        zh = pl.z_host.numpy()
        t_dev = t_rans = 0.0
        tm = time.perf_counter()

        def dec_z(b):
            zh[b] = ans.decode(items[b]["strings"][1][0], zidx, ecdf, eln, eoff).reshape(zh.shape[1:])

        run_all = (lambda f: list(self.pool.map(f, range(B)))) if B > 1 else (lambda f: f(0))
        run_all(dec_z)
        t_rans += time.perf_counter() - tm
        pl.z_in.copy_(pl.z_host, non_blocking=True)
        decoders = [ans._Decoder(items[b]["strings"][0][0]) for b in range(B)]
        try:
            S = m.num_slices
            for i in range(S + 1):
                tm = time.perf_counter()
                g, fn, out = pl.segs[i]
                if g is not None:
                    g.replay()
                else:
                    out = fn()
                if i == S:
                    res = out.clone() if g is not None else out
                    # (the last segment — refinement of the last slice + the synthesis transform — is still running: the caller's first
                    #  use of x_hat waits for it; `device_ms` covers the segments up to the last hop, `tail_issue_ms` issuing the last one)
                    self.last = {"op": "decompress", "device_ms": t_dev * 1e3, "rans_ms": t_rans * 1e3, "hops": S + 1,
                                 "tail_issue_ms": (time.perf_counter() - tm) * 1e3}
                    return res
                pl.idx_host[i].copy_(out, non_blocking=True)
                torch.cuda.current_stream().synchronize()          # hop i: CDF indexes of slice i for every image
                ih, rh = pl.idx_host[i].numpy(), pl.rv_host[i].numpy()
                t_dev += time.perf_counter() - tm
                tm = time.perf_counter()

                def dec_y(b):
                    rh[b] = decoders[b].decode(ih[b].reshape(-1), gcdf, gln, goff).reshape(rh.shape[1:])

                run_all(dec_y)
                t_rans += time.perf_counter() - tm
                pl.rv_in[i].copy_(pl.rv_host[i], non_blocking=True)
        finally:
            for d in decoders:
                d.close()


class ContextCodecEngine(_Engine):
    """CodecEngine's service for the two context models of models/hyperprior.py on THE LANES STREAM:

        eng = ContextCodecEngine(model, lanes=4); items = eng.compress(x[B]); x_hat = eng.decompress(items, check=True)

    model: a JointAutoregressiveHierarchicalPriors (``mbt2018``) or a JointCheckerboardHierarchicalPriors; every other class is refused by
    name.  An item is CodecEngine.compress(lanes=W)'s, its strings byte for byte model.compress(x, lanes=W)'s, and decompress returns
    model.decompress(strings, shape, lanes=W)["x_hat"] bit for bit: the plans run the model's own pass code (_lanes_encode,
    _lanes_pack_scheduled, _lanes_decode_pass) on a models.hyperprior.PassSchedule they keep.

      compress    ONE graph per (x.shape, W, kernel state): g_a, h_a, z_hat = round(z - median) + median on the device (identical to
                  decoding the z stream that the host writes afterwards, so nothing waits for the host coder), h_s, the encoder's whole
                  schedule, the gather into stream order, the lanes encoder and clc_rans_lanes_pack.  Then two device->host copies
                  (header with the z symbols; the packed words, cut to the header's total) and z on the host threads.
      decompress  headers parsed and z decoded on the host; ONE pinned upload (z symbols; states | spans | words) into plan-owned buffers
                  and ONE replay of ONE graph: z_hat, h_s, per step of the schedule the chain and one clc_ar_lanes_decode, g_s, clamp.
                  No copy back; check=True adds the one download of the coder's end states after the replay is issued.

    MODEL STATE.  A graph holds the addresses of the parameters and entropy-model buffers it was captured over.  Every call compares the
    model's CURRENT tensors — object, data_ptr() and _version of each parameter and buffer, read from the modules anew — with those of
    the previous call and drops every plan when one differs (an in-place change, update(force=True), load_state_dict, .to()): the next
    call rebuilds.  The previous call's tensor objects are held until then, so an identity can never be that of a freed tensor's
    successor, and a dropped plan's graph is never replayed.
    `last`: op, graphs (replays of the call: 1, or 0 without use_graph), hops, rans_ms, device_ms, plan_rebuilt, capture_ms (building
    time of the plans this call made, 0.0 when it made none)."""

    def __init__(self, model, lanes=4, threads: int = 8, use_graph: bool = True, max_plans: int = 0):
        from .models.hyperprior import JointAutoregressiveHierarchicalPriors, JointCheckerboardHierarchicalPriors

        served = (JointAutoregressiveHierarchicalPriors, JointCheckerboardHierarchicalPriors)
        if type(model) not in served:
            name = type(model).__name__
            why = ""
            if name.startswith("Cheng2020"):
                why = ": its compress takes no lanes="
            elif name == "Elic2022":
                why = ": its lanes encoder downloads inside the pass"
            elif hasattr(model, "gaussian_conditional") and not hasattr(model, "context_prediction"):
                why = ": it has no context model to schedule"
            raise ValueError(f"ContextCodecEngine: {name} is not served{why} (it takes {served[0].__name__} and {served[1].__name__})")
        if lanes is None:
            raise ValueError("ContextCodecEngine: lanes=None (the one-stream format) is not served; pass lanes = 1 .. 16")
        self.lanes = coding.lanes_count(lanes, "ContextCodecEngine")
        super().__init__(model, threads, use_graph, max_plans)
        self._state = None

    # ---------------------------------------------------------------- model state
    def _model_state(self):
        return [(t, t.data_ptr(), t._version) for mod in self.model.modules() for held in (mod._parameters, mod._buffers)
                for t in held.values() if t is not None]

    def _begin(self):
        """the start of a public call: plans captured over another model state go"""
        self._built_ms = 0.0
        now, was = self._model_state(), self._state
        self._dropped = False
        if was is None or len(was) != len(now) or any(a[0] is not b[0] or a[1:] != b[1:] for a, b in zip(was, now)):
            self._dropped = bool(self._enc or self._dec)
            if self._dropped:
                torch.cuda.synchronize()   # (a replay of the last call may still run: its graph, pool and buffers go below)
            self._enc.clear()
            self._dec.clear()
        self._state = now

    def _last_extras(self, last, pl):
        """graphs, capture_ms; plan_rebuilt: a plan was replaced — its words buffer was too small, or the model's state had moved"""
        last.update(graphs=0 if pl.graph is None else 1, capture_ms=self._built_ms, plan_rebuilt=last.get("plan_rebuilt", False) or self._dropped)
        return last

    # ---------------------------------------------------------------- encoder
    def _build_encoder(self, x):
        m, W = self.model, self.lanes
        pl = _Plan()
        pl.lanes, pl.kernel_config = W, kernel_config()
        pl.x = x.clone()
        B, dev = x.shape[0], x.device
        pl.sched = m._lanes_schedule(B, x.shape[2] // 16, x.shape[3] // 16, dev)
        pl.regions = ops.rans_lanes_regions(pl.sched.segments, W, B)
        pl.regions_dev = torch.from_numpy(pl.regions).to(dev)

        @torch.no_grad()
        def run():
            y = m._analysis(m._prep(pl.x))
            z = m._hyper_analysis(y)
            med = m.entropy_bottleneck._get_medians().reshape(1, -1, 1, 1)
            z_sym = torch.round(z - med).to(torch.int32)                    # == EntropyBottleneck.compress's symbols
            z_hat = (z_sym.float() + med).contiguous(memory_format=CL)      # == decompress(compress(z)), as _code_inputs takes it
            sym, idx, _ = m._lanes_encode(y, m._hyper_synthesis(z_hat), pl.sched)
            zs = z_sym.contiguous().reshape(-1)
            small = torch.empty((B * W + 1 + zs.numel(),), device=dev, dtype=torch.int32)
            packed, _ = m._lanes_pack_scheduled(sym, idx, pl.sched, W, pl.regions, pl.regions_dev, small[:B * W + 1])
            small[B * W + 1:].copy_(zs)
            return (small, packed), tuple(z.shape[-2:])

        pl.graph, (pl.packed, pl.zshape) = self._capture(run)
        pl.run = run
        return self._lanes_encoder_host(pl)

    @torch.no_grad()
    def compress(self, x) -> List[dict]:
        """x [B, 3, H, W], H and W multiples of 64 -> one {"strings": [[y], [z]], "shape", "kernel_config", "lanes": W} per image"""
        x = self.model._prep(x)
        self._begin()
        pl = self._plan(self._enc, (tuple(x.shape), self.lanes, kernel_config()), lambda: self._build_encoder(x))
        t0 = time.perf_counter()
        pl.x.copy_(x, non_blocking=True)
        if pl.graph is not None:
            pl.graph.replay()
        else:
            pl.packed, _ = pl.run()
        return self._finish_lanes_encoder(pl, t0)

    # ---------------------------------------------------------------- decoder
    def _build_decoder(self, B, zshape, dev, cap_words):
        m = self.model
        pl = _Plan()
        self._lanes_decoder_buffers(pl, B, zshape, dev, self.lanes, cap_words)
        pl.sched = m._lanes_schedule(B, zshape[0] * 4, zshape[1] * 4, dev)

        @torch.no_grad()
        def run():
            med = m.entropy_bottleneck._get_medians().reshape(1, -1, 1, 1)
            z_hat = (pl.z_in.float() + med).contiguous(memory_format=CL)
            params, y_hat = coding.decoder_start(m._hyper_synthesis(z_hat), B, m.M)
            return m._synthesis(m._lanes_decode_pass(params, y_hat, (pl.state, pl.spans, pl.words), pl.sched)).clamp_(0, 1)

        pl.graph, pl.out = self._capture(run)
        pl.run = run
        return pl

    @torch.no_grad()
    def decompress(self, items: Sequence[dict], check=True) -> torch.Tensor:
        """items: compress()'s (or unpack_item()ed containers, whose kernel-config tag is checked here) of B images of one shape -> x_hat
        [B, 3, H, W] clamped to [0, 1].  check=True downloads the coder's end states once, after the replay is issued, and raises
        ValueError naming the image and the wave streams that did not end where a whole stream ends.  Refused by name: an empty list,
        an item whose "lanes" is not the engine's, items of more than one shape, a header of another stream count, a one-stream string."""
        items = list(items)
        if not items:
            raise ValueError("ContextCodecEngine.decompress: no items")
        W = self.lanes
        check_items(items, W)
        shapes = sorted({tuple(int(v) for v in it["shape"]) for it in items})
        if len(shapes) != 1:
            raise ValueError(f"ContextCodecEngine.decompress: the items of one call share one shape, got {shapes}")
        B, zshape = len(items), shapes[0]
        self._begin()
        dev = next(self.model.parameters()).device
        sig = (B, zshape, W, kernel_config())

        def pl_for(cap, rebuild):
            if rebuild:
                self._dec.pop(sig, None)
            return self._plan(self._dec, sig, lambda: self._build_decoder(B, zshape, dev, cap))

        return self._decompress_lanes(items, pl_for, W, check)
