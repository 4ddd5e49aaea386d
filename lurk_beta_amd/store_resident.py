"""The content-addressed store, resident on the GPU (``lurk_hip_store``, include/lurk_hip.h "the store, resident on the device").

``StoreCore`` is append-only and keeps its digest memo for its whole life (/root/reference/src/lem/store_core.rs:199-248);
``hydrate_z_cache`` (:256-269) hashes what has been interned since the last hydration and ``Prover::prove`` hydrates before every
proof (/root/reference/src/proof/mod.rs:180-198).  ``DeviceStore`` is that memo in HBM: ``append`` hashes the new nodes only, and
``slot_preimages`` turns a MultiFrame's slots (``allocate_slot``, /root/reference/src/lem/circuit.rs:249-315) into the preimage
tensors ``MultiFrameWitness.assemble`` takes without a digest leaving the device.  Nodes are the tuples of ``store_hasher`` with
GLOBAL child ids (ids are assigned in append order, the first node appended is 0)."""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from . import store_hasher as SH
from .witness import SLOT_ORDER, slot_preimage_len

SLOT_ELEM_ZERO, SLOT_ELEM_TAG, SLOT_ELEM_DIGEST, SLOT_ELEM_CONST = 0, 1, 2, 3
_SLOT_TYPES = dict(SLOT_ORDER)


def _slot_type(slot_type) -> int:
    st = _SLOT_TYPES.get(slot_type, slot_type)
    if st not in _SLOT_TYPES.values():
        raise ValueError(f"unknown slot type {slot_type!r}")
    return st


def slot_elems(slot_type, slots) -> np.ndarray:
    """The (n_elems, 2) uint32 array of ``lurk_hip_slot_elem`` {kind, arg} for slots of ONE type, by ``allocate_slot``'s rule
    (circuit.rs:265-308).  A slot is None (absent: the dummy preimage of zeros) or a list of values, each
      ("ptr", id)   Val::Pointer  -> the node's tag, then its digest
      ("num", id)   Val::Num      -> the digest of the node that holds the value
      ("bool", b)   Val::Boolean  -> 1 or 0
    ``slot_type``: a name of ``witness.SLOT_ORDER`` or its number.  A slot whose values do not fill the type's preimage exactly is
    refused (``SlotType::is_compatible``).  Pure host code: needs no device."""
    arity = slot_preimage_len(_slot_type(slot_type))
    out = []
    for k, slot in enumerate(slots):
        if slot is None:
            out += [(SLOT_ELEM_ZERO, 0)] * arity
            continue
        elems = []
        for val in slot:
            kind, arg = val
            if kind == "ptr":
                elems += [(SLOT_ELEM_TAG, int(arg)), (SLOT_ELEM_DIGEST, int(arg))]
            elif kind == "num":
                elems.append((SLOT_ELEM_DIGEST, int(arg)))
            elif kind == "bool":
                elems.append((SLOT_ELEM_CONST, 1 if arg else 0))
            else:
                raise ValueError(f"slot {k}: unknown value kind {kind!r}")
        if len(elems) != arity:
            raise ValueError(f"slot {k}: {len(elems)} preimage elements, a {slot_type} slot takes {arity}")
        out += elems
    if any(not 0 <= a < 1 << 32 for _, a in out):
        raise ValueError("a node id does not fit 32 bits")
    return np.array(out, dtype=np.uint32).reshape(-1, 2)


class DeviceStore:
    """An append-only store on the GPU: per node id the canonical digest and the tag.  Digests leave as (m, 4) uint64 numpy arrays
    (``digests``) or stay as (m, 4) int64 device tensors (``digests_dev``, ``slot_preimages``)."""

    slot_elems = staticmethod(slot_elems)

    def __init__(self, field_id: int, reserve_nodes: int = 0):
        self.field_id = field_id
        self._h = None
        h = ctypes.c_void_p()
        _lib.check(_lib.load().lurk_hip_store_create(ctypes.byref(h), field_id, reserve_nodes))
        self._h = h

    def append(self, nodes: list[tuple], digests: bool = False):
        """``nodes``: ``store_hasher`` tuples whose children are global node ids below the id the node itself receives.  Values are
        re-based per call (no value array stays resident).  Returns the first new id; with ``digests`` also the new nodes' digests."""
        rec, vals = SH.encode(nodes)
        return self.append_records(rec, vals, digests)

    def append_records(self, rec: np.ndarray, vals: np.ndarray, digests: bool = False):
        """The same on encoded records ((n, 8) uint32 ``lurk_hip_store_node``, (m, 4) uint64 values indexed by THIS call's records)."""
        rec = np.ascontiguousarray(rec, dtype=np.uint32).reshape(-1, 8)
        vals = np.ascontiguousarray(vals, dtype=np.uint64).reshape(-1, 4)
        first = ctypes.c_size_t()
        out = np.zeros((rec.shape[0], 4), dtype=np.uint64) if digests else None
        _lib.check(_lib.load().lurk_hip_store_append(self._h, _lib.ptr(rec) if rec.shape[0] else None, rec.shape[0], _lib.ptr(vals) if vals.shape[0] else None,
                                                     vals.shape[0], ctypes.byref(first), _lib.ptr(out)))
        return (first.value, out) if digests else first.value

    def digests(self, ids) -> np.ndarray:
        """(m, 4) uint64 canonical digests of the nodes ``ids``; an id that is not a node is refused."""
        ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
        out = np.zeros((ids.shape[0], 4), dtype=np.uint64)
        _lib.check(_lib.load().lurk_hip_store_digests(self._h, _lib.ptr(ids) if ids.shape[0] else None, ids.shape[0], _lib.ptr(out)))
        return out

    def digests_dev(self, ids, stream=None):
        """``ids``: an int32 device tensor (or anything ``digests`` takes, uploaded) -> (m, 4) int64 device tensor.  Stream-ordered; the
        row of an id that is not a node is zero."""
        import torch

        if not hasattr(ids, "data_ptr"):
            ids = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1).view(np.int32)).cuda()
        assert ids.is_cuda and ids.element_size() == 4 and ids.is_contiguous(), "ids: a contiguous 32-bit device tensor"
        m = ids.numel()
        out = torch.empty((m, 4), dtype=torch.int64, device="cuda")
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.load().lurk_hip_store_digests_dev(self._h, _lib.ptr(ids) if m else None, m, _lib.ptr(out) if m else None, _lib.ptr(s)))
        return out

    def slot_preimages(self, slot_type, slots, mont: bool = True, stream=None):
        """The preimages of ``slots`` (one type, frame-major) as the (n, arity, 4) int64 device tensor ``MultiFrameWitness.assemble``
        takes under that type's name; Montgomery when ``mont`` (pass the same flag to ``assemble``)."""
        import torch

        arity = slot_preimage_len(_slot_type(slot_type))
        elems = slot_elems(slot_type, slots)
        n = elems.shape[0]
        out = torch.empty((n // arity, arity, 4), dtype=torch.int64, device="cuda")
        if n:
            d_elems = torch.from_numpy(elems.view(np.int32)).cuda()
            s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
            _lib.check(_lib.load().lurk_hip_store_slot_preimages_dev(self._h, _lib.ptr(d_elems), n, int(mont), _lib.ptr(out), _lib.ptr(s)))
        return out

    def info(self) -> dict:
        f, dev = ctypes.c_int(), ctypes.c_int()
        v = [ctypes.c_size_t() for _ in range(4)]
        _lib.check(_lib.load().lurk_hip_store_info(self._h, ctypes.byref(f), *[ctypes.byref(x) for x in v], ctypes.byref(dev)))
        return {"field_id": f.value, "n_nodes": v[0].value, "levels": v[1].value, "hashes_done": v[2].value, "capacity": v[3].value, "device": dev.value}

    def __len__(self) -> int:
        return self.info()["n_nodes"]

    def close(self):
        """Frees the device arrays (36 B per node of capacity).  Idempotent; the handle is unusable afterwards."""
        h, self._h = self._h, None
        if h:
            _lib.check(_lib.load().lurk_hip_store_destroy(h))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        # as DeviceTrie: a handle that was never closed gives its memory back when it is collected; nothing can be raised from here
        if getattr(self, "_h", None) is None:
            return
        try:
            self.close()
        except Exception:
            pass
