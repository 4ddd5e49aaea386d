"""Host-side mirror of the trie coprocessor's step circuits over the HIP library (include/lurk_hip.h, "the trie coprocessor's step
circuits"): what ``Trie::synthesize_lookup`` / ``Trie::synthesize_insert`` (/root/reference/src/coprocessor/trie/mod.rs:652-714, 802-880)
allocate and enforce.  The witness blocks are written on the GPU from the proofs a ``DeviceTrie`` leaves there; sizes and rows are host
computations."""
from __future__ import annotations

import ctypes
from collections import namedtuple

import numpy as np

from . import _lib
from .fold import R1CSShape

LOOKUP, INSERT = 0, 1

TrieCircuitSize = namedtuple("TrieCircuitSize", "size num_cons nnz_a nnz_b nnz_c result_col value_col")


def trie_circuit_size(field_id: int, height: int, op: int) -> TrieCircuitSize:
    """``lurk_hip_trie_circuit_size``; value_col is None for a lookup.  Needs no GPU."""
    v = [ctypes.c_size_t() for _ in range(7)]
    _lib.check(_lib.load().lurk_hip_trie_circuit_size(field_id, height, op, *[ctypes.byref(x) for x in v]))
    vals = [x.value for x in v]
    return TrieCircuitSize(*vals[:6], vals[6] if op == INSERT else None)


def trie_circuit_constraints(field_id: int, height: int, op: int):
    """The circuit's rows (``lurk_hip_trie_circuit_constraints``): three CSR triples (indptr, indices, data) for A, B, C over the block's
    local columns, column ``size`` the constant ONE; data (nnz, 4) u64 Montgomery.  Needs no GPU."""
    sz = trie_circuit_size(field_id, height, op)
    out = [(np.zeros(sz.num_cons + 1, dtype=np.uint64), np.zeros(n, dtype=np.uint64), np.zeros((n, 4), dtype=np.uint64)) for n in (sz.nnz_a, sz.nnz_b, sz.nnz_c)]
    _lib.check(_lib.load().lurk_hip_trie_circuit_constraints(field_id, height, op, *[_lib.ptr(a) for m in out for a in m]))
    return tuple(out)


def trie_circuit_shape(field_id: int, height: int, op: int, n_blocks: int, first: int, stride: int, num_vars: int, num_io: int, extra=None) -> R1CSShape:
    """A resident shape of ``n_blocks`` circuits at columns first + b * stride, ONE at column num_vars (``lurk_hip_trie_circuit_r1cs_create``).
    extra = (A, B, C) CSR triples of the caller's further rows over the num_vars + 1 + num_io columns, appended after the circuits' rows."""
    keep, args, extra_cons = [], [None] * 9, 0
    if extra is not None:
        extra_cons = len(extra[0][0]) - 1
        args = []
        for indptr, indices, data in extra:
            ip = np.ascontiguousarray(indptr, dtype=np.uint64)
            ix = np.ascontiguousarray(indices, dtype=np.uint64)
            dv = np.ascontiguousarray(data, dtype=np.uint64)
            if ip.size != extra_cons + 1 or ix.size * 4 != dv.size:
                raise ValueError("malformed CSR matrix")
            keep += [ip, ix, dv]
            args += [_lib.ptr(ip), _lib.ptr(ix), _lib.ptr(dv)]
    h = ctypes.c_void_p()
    _lib.check(_lib.load().lurk_hip_trie_circuit_r1cs_create(ctypes.byref(h), field_id, height, op, n_blocks, first, stride, num_vars, num_io, extra_cons,
                                                             *[a if a is not None else _lib.ptr(None) for a in args]))
    return R1CSShape._wrap(h)


def trie_circuit_witness(field_id: int, height: int, op: int, roots, keys, old_paths, d_w, *, new_values=None, new_paths=None, offsets=None, first: int = 0,
                         stride: int = 0, stream=None) -> None:
    """``lurk_hip_trie_circuit_witness_dev``: the blocks of m = len(keys) circuits into the device tensor ``d_w`` (32-byte Montgomery elements),
    block i at ``offsets[i]`` (a device tensor of uint64) or at first + i * stride.  roots, keys, new_values: device tensors of canonical
    elements ((m, 4) int64; one root serves every block); paths (m, H, 8, 4) as ``DeviceTrie`` returns them.  For a chain the roots are
    [root(T_0), roots[0 .. m - 2]] of ``DeviceTrie.insert_chain``.  Does not synchronise."""
    m = keys.numel() // 4
    root_stride = 0 if roots.numel() == 4 and m != 1 else 1
    assert root_stride == 0 or roots.numel() == 4 * m, "one root, or one root per block"
    _lib.check(_lib.load().lurk_hip_trie_circuit_witness_dev(field_id, height, op, _lib.ptr(roots), root_stride, _lib.ptr(keys), _lib.ptr(new_values), _lib.ptr(old_paths),
                                                             _lib.ptr(new_paths), m, _lib.ptr(d_w), _lib.ptr(offsets), first, stride, _lib.ptr(stream)))
