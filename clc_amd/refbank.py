"""Reference bank of the codec: self-contained containers and cached reference latents.

CLC only decodes with the very reference frames that encoded, prepared to the very bits: `evaluate` resizes each reference to the
query's size (bilinear, align_corners=False) and pads it to a multiple of 128 (the reference's eval_CLC.py:246-257, 306-315), and any
difference in those tensors moves the slice loop's means / scales and desynchronises the arithmetic decoder without an error.  The
references come from a FIXED bank (the cluster representatives of clc_amd.retrieval.ReferenceIndex, shared by a whole data set), so

  * a container names its references by index into the bank's ordered keys and carries the bank's id (clc_amd.codec, version 3), and the
    decoder prepares them itself on one kernel of this build (clc_ref_prepare: the recipe's bits under the build's kernel generation);
  * the reference encoder's output depends only on its weights, the kernel state and the prepared image: it is computed once per
    (key, image size) and kept in a fixed-capacity arena per latent shape (LRU over the slots), from which the captured encoder graph and
    the decoder's first segment gather each call's latents (clc_gather_slots, slot indexes in device memory).

The cache is dropped whenever the content of the reference encoder's parameters and buffers (clc_fingerprint: a hash of the bytes, so
writes through `p.data` or the optimizer's in-place updates count) or the kernel configuration changes.  That content read is the one
host synchronisation of a lookup.
"""
from __future__ import annotations

import struct
import zlib
from collections import OrderedDict
from typing import Dict, List, Mapping, Sequence, Tuple

import torch

from . import ops
from .ops import CL

RECIPE_VERSION = 1   # version of the preparation recipe (clc_ref_prepare's definition); part of every bank_id


class BankMismatch(ValueError):
    """the container names its references in another bank than the one that would decode it"""


def bank_id_of(keys: Sequence[str]) -> int:
    """u32 id of an ordered key list: CRC32 over the recipe version and the UTF-8 keys (each NUL-terminated, so that no two lists
    of keys share one byte string)."""
    crc = zlib.crc32(struct.pack("<I", RECIPE_VERSION))
    for k in keys:
        crc = zlib.crc32(k.encode("utf-8") + b"\0", crc)
    return crc & 0xFFFFFFFF


def _padded(hw) -> Tuple[int, int]:
    return (int(hw[0]) + 127) // 128 * 128, (int(hw[1]) + 127) // 128 * 128


class _Arena:
    """one latent shape: `slots` channels_last latents, never reallocated (captured graphs hold its address); LRU over the slots."""

    def __init__(self, slots, shape, device):
        self.tensor = torch.empty((slots,) + tuple(shape), device=device, memory_format=CL).zero_()
        self.lru: "OrderedDict[Tuple[str, Tuple[int, int]], int]" = OrderedDict()   # (key, image_hw) -> slot, least recent first
        self.free = list(range(slots - 1, -1, -1))

    @property
    def slots(self):
        return self.tensor.shape[0]

    def clear(self):
        self.lru.clear()
        self.free = list(range(self.slots - 1, -1, -1))


class ReferenceBank:
    """bank = ReferenceBank(model, {key: image [3, h, w] in [0, 1]}); engine.compress(x, ref_keys=[[k, ...] per image], bank=bank).

    capacity_bytes: size of EACH arena (one per latent shape, i.e. per padded image size); its slot count is capacity_bytes // the
    bytes of one latent (320 x H/16 x W/16 floats: 320 KiB at 256 x 256).  A call that needs more distinct keys than there are slots
    raises."""

    def __init__(self, model, refs: Mapping[str, torch.Tensor], capacity_bytes: int = 256 << 20, device=None):
        if not hasattr(model, "ref_encoder"):
            raise ValueError("ReferenceBank: the model has no reference encoder (TCM codes without references)")
        self.model = model
        dev = torch.device(device) if device is not None else next(model.parameters()).device
        self.keys: Tuple[str, ...] = tuple(refs.keys())
        for k in self.keys:
            if not isinstance(k, str):
                raise TypeError(f"ReferenceBank: keys are strings (ReferenceIndex.query's keys), got {type(k).__name__} {k!r}")
        self.index: Dict[str, int] = {k: i for i, k in enumerate(self.keys)}
        self.images: Dict[str, torch.Tensor] = {}
        for k, r in refs.items():
            r = torch.as_tensor(r)
            if r.dim() == 4 and r.shape[0] == 1:
                r = r[0]
            if r.dim() != 3 or r.shape[0] != 3:
                raise ValueError(f"ReferenceBank: reference {k!r} must be [3, h, w], got {tuple(r.shape)}")
            self.images[k] = r.to(device=dev, dtype=torch.float32).contiguous()
        self.bank_id = bank_id_of(self.keys)
        self.capacity_bytes = int(capacity_bytes)
        self.device = dev
        self._arenas: Dict[Tuple[int, int, int], _Arena] = {}
        self._state = None
        self.stats = {"hits": 0, "misses": 0, "evictions": 0, "invalidations": 0}

    def __len__(self):
        return len(self.keys)

    # ---- the recipe
    def prepare(self, keys: Sequence[str], image_hw) -> torch.Tensor:
        """references `keys` as the encoder reads them: channels_last [len(keys), 3, H, W] =
        eval.pad(F.interpolate(r, image_hw, mode="bilinear", align_corners=False), 128), one clc_ref_prepare launch."""
        return ops.ref_prepare([self.images[self._key(k)] for k in keys], image_hw)

    def _key(self, k):
        if k not in self.index:
            raise KeyError(f"reference {k!r} is not in this bank ({len(self.keys)} keys, bank_id {self.bank_id:08x})")
        return k

    def latent_shape(self, image_hw) -> Tuple[int, int, int]:
        H, W = _padded(image_hw)
        return (int(self.model.M), H // 16, W // 16)

    # ---- residency
    def _refresh(self):
        """drop every cached latent when the reference encoder's content or the kernel state moved (the one host read of a lookup)."""
        from .codec import kernel_config

        enc = self.model.ref_encoder
        fp = int(ops.fingerprint(list(enc.parameters()) + list(enc.buffers())).item()) & 0xFFFFFFFFFFFFFFFF
        state = (fp, kernel_config())
        if state != self._state:
            if self._state is not None:
                self.stats["invalidations"] += 1
            for a in self._arenas.values():
                a.clear()
            self._state = state

    def _arena(self, shape) -> _Arena:
        a = self._arenas.get(shape)
        if a is None:
            slot_bytes = 4 * shape[0] * shape[1] * shape[2]
            n = self.capacity_bytes // slot_bytes
            if n < 1:
                raise ValueError(f"ReferenceBank: capacity_bytes={self.capacity_bytes} holds no latent of shape {shape} ({slot_bytes} bytes)")
            a = self._arenas[shape] = _Arena(n, shape, self.device)
        return a

    @torch.no_grad()
    def lookup(self, key_rows: Sequence[Sequence[str]], image_hw) -> Tuple[torch.Tensor, List[List[int]]]:
        """make the references of every row resident at image size `image_hw` -> (arena [S, M, h, w], slot of each key per row).  All misses
        of the call are encoded in ONE batched ref_encoder pass (no_grad, the codec's batch-invariant kernels)."""
        hw = (int(image_hw[0]), int(image_hw[1]))
        need = list(OrderedDict.fromkeys(self._key(k) for row in key_rows for k in row))
        self._refresh()
        shape = self.latent_shape(hw)
        a = self._arena(shape)
        if len(need) > a.slots:
            raise ValueError(f"ReferenceBank: one call needs {len(need)} distinct references at {hw}, the arena holds {a.slots} "
                             f"(capacity_bytes={self.capacity_bytes}, {4 * shape[0] * shape[1] * shape[2]} bytes per latent): raise capacity_bytes")
        misses = []
        for k in need:
            if (k, hw) in a.lru:
                a.lru.move_to_end((k, hw))
                self.stats["hits"] += 1
            else:
                misses.append(k)
        wanted = {(k, hw) for k in need}
        for k in misses:
            if not a.free:
                victim = next(e for e in a.lru if e not in wanted)   # least recently used entry this call does not read
                a.free.append(a.lru.pop(victim))
                self.stats["evictions"] += 1
            a.lru[(k, hw)] = a.free.pop()
        if misses:
            self.stats["misses"] += len(misses)
            lat = self.model.ref_encoder(self.prepare(misses, hw))
            if tuple(lat.shape[1:]) != shape:
                raise RuntimeError(f"ReferenceBank: reference latents {tuple(lat.shape[1:])}, expected {shape}")
            for i, k in enumerate(misses):
                a.tensor[a.lru[(k, hw)]].copy_(lat[i])
        return a.tensor, [[a.lru[(k, hw)] for k in row] for row in key_rows]

    def clear(self):
        """forget every cached latent (the arenas stay allocated)."""
        for a in self._arenas.values():
            a.clear()
