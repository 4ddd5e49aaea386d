"""Host-side mirror of lurk-beta's sparse Poseidon trie over the HIP hasher.

Mirrors ``coprocessor::trie::Trie<F, ARITY, HEIGHT>`` (/root/reference/src/coprocessor/trie/mod.rs):
``StandardTrie`` = arity 8, height 85 (:43); ``init_empty`` (:464-481), ``path`` (:589-608),
``lookup`` (:635-652), ``insert`` (:745-800), ``prove_lookup`` (:718-743), ``prove_insert`` (:751-800) and the two ``verify``s (:349-362,
:383-424).  Every node hash of ``Trie`` is ``hash8`` on the GPU through ``PoseidonCache``; the child map (hash -> preimage) is
the reference's ``children``/inverse cache (:453-458).

``DeviceTrie`` is the bulk form over the library's device-resident trie (include/lurk_hip.h, "the sparse Poseidon trie"): one
build for all pairs, proofs and verification for batches of keys, nothing hashed node by node from the host.

``DeviceTrieNodes`` is ``children`` itself on the device (include/lurk_hip.h, "root-addressed tries"): every version of every trie in
one content-addressed table, looked up, inserted into and chained from a ROOT, as the coprocessors do with ``Trie::new_with_root``."""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from .poseidon import PoseidonCache, _ints, _limbs

NUM_BITS = {0: 255, 1: 255, 2: 254}


class Trie:
    def __init__(self, field_id: int, height: int = 85, arity: int = 8, cache: PoseidonCache | None = None):
        assert arity == 8, "lurk-beta instantiates the trie with arity 8 only"
        self.field_id, self.height, self.arity = field_id, height, arity
        self.cache = cache or PoseidonCache(field_id)
        self.children: dict[int, tuple[int, ...]] = {}
        self.empty_roots: list[int] = []
        self._init_empty()
        self.root = self.empty_roots[height - 1] if height else 0

    # -- init_empty (:464-481): empty_roots[0] = hash8([0;8]), empty_roots[i] = hash8([empty_roots[i-1];8])
    def _init_empty(self):
        cur = 0
        for _ in range(self.height):
            cur = self._register([cur] * self.arity)
            self.empty_roots.append(cur)

    def _register(self, preimage) -> int:
        h = self.cache.compute_hash(list(preimage))
        self.children[h] = tuple(preimage)
        return h

    def empty_root_for_height(self, h: int) -> int:
        return 0 if h == 0 else self.empty_roots[h - 1]

    def leaves(self) -> int:
        return self.arity ** self.height

    # -- path (:589-608): MSB-first bits, keep the last 3*H bits, 3-bit big-endian digits
    def path(self, key: int) -> list[int]:
        nbits = NUM_BITS[self.field_id]
        be = [(key >> i) & 1 for i in reversed(range(nbits))]
        need = 3 * self.height
        if need > len(be):
            be = [0] * (need - len(be)) + be
        tail = be[len(be) - need:]
        return [tail[i] << 2 | tail[i + 1] << 1 | tail[i + 2] for i in range(0, need, 3)]

    def _preimages_along(self, path: list[int]) -> list[tuple[int, ...]]:
        """Preimage of every node from the root down the path (an absent subtree is the empty one)."""
        out, node = [], self.root
        for level, digit in enumerate(path):
            pre = self.children.get(node)
            if pre is None:  # empty subtree of height (height - level)
                sub = self.empty_root_for_height(self.height - level - 1)
                pre = (sub,) * self.arity
            out.append(pre)
            node = pre[digit]
        return out

    # -- lookup (:635-652): the leaf-level preimage entry is the payload; 0 = absent
    def lookup(self, key: int):
        path = self.path(key)
        pres = self._preimages_along(path)
        v = pres[-1][path[-1]]
        return None if v == 0 else v

    # -- insert (:745-800): replace the entry, re-hash bottom-up
    def insert(self, key: int, value: int) -> bool:
        path = self.path(key)
        pres = self._preimages_along(path)
        existed = pres[-1][path[-1]] != 0
        cur = value
        for pre, digit in zip(reversed(pres), reversed(path)):
            new = list(pre)
            new[digit] = cur
            cur = self._register(new)
        self.root = cur
        return existed

    # -- prove_lookup (:718-743): the H preimages from the root down; the last one holds the payloads
    def prove_lookup(self, key: int) -> list[tuple[int, ...]]:
        return self._preimages_along(self.path(key))

    # -- prove_insert (:751-800): (old path, new path, inserted); the trie is modified as ``insert`` does
    def prove_insert(self, key: int, value: int):
        path = self.path(key)
        old = self._preimages_along(path)
        new, cur = [], value
        for pre, digit in zip(reversed(old), reversed(path)):
            mod = list(pre)
            mod[digit] = cur
            cur = self._register(mod)
            new.append(tuple(mod))
        new.reverse()
        inserted = cur != self.root
        self.root = cur
        return old, new, inserted


def verify_lookup(trie: Trie, root: int, key: int, value: int, preimage_path) -> int:
    """``LookupProof::verify`` (:349-362) with ``trie``'s hasher.  0 = accepted, k + 1 = the hash of preimage k is not the expected
    node, H + 1 = the selected leaf entry is not ``value`` (the codes of lurk_hip_trie_verify_lookup_dev)."""
    nxt = root
    for k, (digit, pre) in enumerate(zip(trie.path(key), preimage_path)):
        if trie.cache.compute_hash(list(pre)) != nxt:
            return k + 1
        nxt = pre[digit]
    return 0 if nxt == value else trie.height + 1


def verify_insert(trie: Trie, old_root: int, new_root: int, key: int, old_value, new_value: int, old_path, new_path) -> int:
    """``InsertProof::verify`` (:383-424), the first failing check: the old proof (1 .. H + 1), the two paths differing in more than one
    position of a level (0x100 + level + 1), the new proof (0x200 + 1 .. H + 1).  ``old_value`` None = absent = 0."""
    code = verify_lookup(trie, old_root, key, old_value or 0, old_path)
    if code:
        return code
    for level, (a, b) in enumerate(zip(old_path, new_path)):
        if sum(x != y for x, y in zip(a, b)) > 1:
            return 0x100 + level + 1
    code = verify_lookup(trie, new_root, key, new_value, new_path)
    return 0x200 + code if code else 0


def path_value(key: int, height: int) -> int:
    """The low 3 * height bits of the key: keys are ordered, and told apart, by it."""
    return int(key) & ((1 << (3 * height)) - 1)


def _dev(a: np.ndarray):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _elems(vals):
    """Python ints or a (m, 4) uint64 array or a device tensor of 32-byte elements -> device tensor (m, 4) int64"""
    if hasattr(vals, "data_ptr"):
        return vals
    if isinstance(vals, np.ndarray):
        return _dev(vals.reshape(-1, 4))
    return _dev(_limbs(list(vals)))


class DeviceTrie:
    """A built trie resident on the GPU (lurk_hip_trie).  Keys, values, roots and proofs cross this interface as device tensors of
    32-byte canonical elements ((m, 4) int64; paths (m, H, 8, 4)); Python ints and numpy arrays are accepted and uploaded."""

    def __init__(self, handle, field_id: int, height: int, n: int):
        self._h, self.field_id, self.height, self.n = handle, field_id, height, n

    @classmethod
    def build(cls, field_id: int, pairs, height: int = 85, stream=None) -> "DeviceTrie":
        """``pairs``: (key, value) Python ints in any order.  Sorted on the host by path value; of pairs that share a path the LAST is
        kept, as sequential inserts would leave it."""
        last = {}
        for k, v in pairs:
            last[path_value(k, height)] = (int(k), int(v))
        order = sorted(last)
        return cls.build_sorted(field_id, _limbs([last[p][0] for p in order]), _limbs([last[p][1] for p in order]), height, stream)

    @classmethod
    def build_sorted(cls, field_id: int, keys, values, height: int = 85, stream=None) -> "DeviceTrie":
        """Keys already reduced and strictly increasing in path order (the library checks and refuses otherwise)."""
        lib = _lib.load()
        dk, dv = _elems(keys), _elems(values)
        n = dk.numel() // 4 if hasattr(dk, "numel") else 0
        h = ctypes.c_void_p()
        _lib.check(lib.lurk_hip_trie_build_dev(ctypes.byref(h), field_id, height, _lib.ptr(dk) if n else None, _lib.ptr(dv) if n else None, n, _lib.ptr(stream)))
        return cls(h, field_id, height, n)

    @property
    def root(self) -> int:
        out = np.zeros(4, dtype=np.uint64)
        _lib.check(_lib.load().lurk_hip_trie_root(self._h, _lib.ptr(out)))
        return _ints(out)[0]

    def _root_dev(self):
        return _dev(_limbs([self.root]))

    def prove_lookup(self, keys, stream=None):
        """-> (paths (m, H, 8, 4), values (m, 4)), device tensors; a value of 0 = absent"""
        import torch

        dk = _elems(keys)
        m = dk.numel() // 4
        paths = torch.empty((m, self.height, 8, 4), dtype=torch.int64, device="cuda")
        values = torch.empty((m, 4), dtype=torch.int64, device="cuda")
        _lib.check(_lib.load().lurk_hip_trie_prove_lookup_dev(self._h, _lib.ptr(dk), m, _lib.ptr(paths), _lib.ptr(values), _lib.ptr(stream)))
        return paths, values

    def prove_insert(self, keys, values, stream=None):
        """m independent insertions into the trie as built -> (old paths, new paths, old values, new roots), device tensors"""
        import torch

        dk, dv = _elems(keys), _elems(values)
        m = dk.numel() // 4
        old = torch.empty((m, self.height, 8, 4), dtype=torch.int64, device="cuda")
        new = torch.empty_like(old)
        old_values = torch.empty((m, 4), dtype=torch.int64, device="cuda")
        new_roots = torch.empty((m, 4), dtype=torch.int64, device="cuda")
        _lib.check(_lib.load().lurk_hip_trie_prove_insert_dev(self._h, _lib.ptr(dk), _lib.ptr(dv), m, _lib.ptr(old), _lib.ptr(new), _lib.ptr(old_values),
                                                              _lib.ptr(new_roots), _lib.ptr(stream)))
        return old, new, old_values, new_roots

    def insert_chain(self, keys, values, *, paths=True, trie=True, stream=None):
        """A chain of dependent insertions (lurk_hip_trie_insert_chain_dev): update i is applied to the trie that update i - 1 left, as
        ``Trie.prove_insert`` called step after step -> (old paths, new paths, old values, roots, new trie); ``roots[i]`` is the root after
        update i and ``new trie`` a ``DeviceTrie`` of the trie after the last one (this one is not modified).  ``paths=False`` leaves the
        two path tensors out, ``trie=False`` the new trie: what was not asked for is None."""
        import torch

        dk, dv = _elems(keys), _elems(values)
        m = dk.numel() // 4 if hasattr(dk, "numel") else 0
        assert (dv.numel() // 4 if hasattr(dv, "numel") else 0) == m, "as many values as keys"
        old = torch.empty((m, self.height, 8, 4), dtype=torch.int64, device="cuda") if paths else None
        new = torch.empty_like(old) if paths else None
        old_values = torch.empty((m, 4), dtype=torch.int64, device="cuda")
        roots = torch.empty((m, 4), dtype=torch.int64, device="cuda")
        h = ctypes.c_void_p()
        _lib.check(_lib.load().lurk_hip_trie_insert_chain_dev(self._h, _lib.ptr(dk) if m else None, _lib.ptr(dv) if m else None, m, _lib.ptr(old) if paths else None,
                                                              _lib.ptr(new) if paths else None, _lib.ptr(old_values), _lib.ptr(roots),
                                                              ctypes.byref(h) if trie else None, _lib.ptr(stream)))
        grown = None
        if trie:
            n = ctypes.c_size_t()
            grown = DeviceTrie(h, self.field_id, self.height, 0)  # owns the handle from here on
            _lib.check(_lib.load().lurk_hip_trie_info(h, None, None, ctypes.byref(n), None))
            grown.n = n.value
        return old, new, old_values, roots, grown

    def verify_lookup(self, keys, values, paths, roots=None, stream=None):
        """-> (codes (m,) numpy uint32, n_failed).  ``roots``: None = this trie's root for every proof, or one root per proof."""
        return verify_lookup_batch(self.field_id, self.height, self._root_dev() if roots is None else roots, keys, values, paths, stream)

    def verify_insert(self, keys, old_values, new_values, old_paths, new_paths, new_roots, old_roots=None, stream=None):
        """-> (codes, n_failed).  ``old_roots``: None = this trie's root for every proof (then ``new_roots`` is one per proof and the
        old root is repeated), or one old root per proof."""
        dn = _elems(new_roots)
        if old_roots is None:
            old_roots = self._root_dev().repeat(dn.numel() // 4, 1)
        return verify_insert_batch(self.field_id, self.height, old_roots, dn, keys, old_values, new_values, old_paths, new_paths, stream)

    def close(self):
        """Frees the device buffers (32 B x n x (H + 2)).  Idempotent; the handle is unusable afterwards."""
        h, self._h = self._h, None
        if h:
            _lib.check(_lib.load().lurk_hip_trie_destroy(h))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        # a handle that was never closed gives its device memory back when it is collected; nothing can be raised from here.  A closed
        # one has nothing left to give back, whenever the collector gets to it (a closed trie kept alive by a traceback is collected
        # at some later collection, not when its last name goes)
        if getattr(self, "_h", None) is None:
            return
        try:
            self.close()
        except Exception:
            pass


class DeviceTrieNodes:
    """The trie's child map (``Trie.children``, the reference's inverse Poseidon cache) resident on the GPU (lurk_hip_trie_nodes): every
    version of every trie of one (field, height), addressed by ROOT.  What ``Trie::new_with_root`` and a host-side root -> handle table
    were for: a root goes in as an element, the walk happens on the device.  Elements cross as for ``DeviceTrie``."""

    def __init__(self, handle, field_id: int, height: int):
        self._h, self.field_id, self.height = handle, field_id, height

    @classmethod
    def create(cls, field_id: int, height: int = 85, reserve_nodes: int = 0) -> "DeviceTrieNodes":
        """``init_empty``: the store holds the ``height`` nodes of the empty chain."""
        h = ctypes.c_void_p()
        _lib.check(_lib.load().lurk_hip_trie_nodes_create(ctypes.byref(h), field_id, height, reserve_nodes))
        return cls(h, field_id, height)

    def info(self) -> dict:
        f, hgt, dev = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        n, slots = ctypes.c_size_t(), ctypes.c_size_t()
        _lib.check(_lib.load().lurk_hip_trie_nodes_info(self._h, ctypes.byref(f), ctypes.byref(hgt), ctypes.byref(n), ctypes.byref(slots), ctypes.byref(dev)))
        return {"field_id": f.value, "height": hgt.value, "n_nodes": n.value, "slots": slots.value, "device": dev.value}

    @property
    def n_nodes(self) -> int:
        return self.info()["n_nodes"]

    def register(self, preimages, stream=None):
        """``register_hash`` for a batch: preimages (count, 8, 4) or a flat list of ints -> digests (count, 4), a device tensor"""
        import torch

        dp = _elems(preimages)
        count = dp.numel() // 32
        digests = torch.empty((count, 4), dtype=torch.int64, device="cuda")
        _lib.check(_lib.load().lurk_hip_trie_nodes_register_dev(self._h, _lib.ptr(dp) if count else None, count, _lib.ptr(digests), _lib.ptr(stream)))
        return digests

    def add_trie(self, trie: DeviceTrie, stream=None):
        """Every node of a built ``DeviceTrie``; nothing is hashed."""
        _lib.check(_lib.load().lurk_hip_trie_nodes_add_trie(self._h, trie._h, _lib.ptr(stream)))

    def get(self, digests, stream=None):
        """-> (preimages (m, 8, 4), found (m,) int32), device tensors; a digest that is not in the store gives a zero row"""
        import torch

        dd = _elems(digests)
        m = dd.numel() // 4
        pre = torch.empty((m, 8, 4), dtype=torch.int64, device="cuda")
        found = torch.empty(max(m, 1), dtype=torch.int32, device="cuda")
        _lib.check(_lib.load().lurk_hip_trie_nodes_get_dev(self._h, _lib.ptr(dd), m, _lib.ptr(pre), _lib.ptr(found), _lib.ptr(stream)))
        return pre, found[:m]

    @staticmethod
    def _stride(dr, m: int) -> int:
        return 0 if dr.numel() == 4 and m != 1 else 1

    def prove_lookup(self, roots, keys, stream=None):
        """``roots``: one root for every key (a single element) or one per key -> (paths (m, H, 8, 4), values (m, 4), status (m,) int32,
        n_missing); status k + 1 = the node expected at level k is not in the store"""
        import torch

        dr, dk = _elems(roots), _elems(keys)
        m = dk.numel() // 4
        paths = torch.empty((m, self.height, 8, 4), dtype=torch.int64, device="cuda")
        values = torch.empty((m, 4), dtype=torch.int64, device="cuda")
        status = torch.empty(max(m, 1), dtype=torch.int32, device="cuda")
        missing = ctypes.c_uint64()
        _lib.check(_lib.load().lurk_hip_trie_nodes_prove_lookup_dev(self._h, _lib.ptr(dr), self._stride(dr, m), _lib.ptr(dk), m, _lib.ptr(paths), _lib.ptr(values),
                                                                    _lib.ptr(status), ctypes.byref(missing), _lib.ptr(stream)))
        return paths, values, status[:m], missing.value

    def prove_insert(self, roots, keys, values, *, register_new=True, stream=None):
        """m independent insertions, each at its own root -> (old paths, new paths, old values, new roots, status, n_missing); with
        ``register_new`` every new root is addressable afterwards"""
        import torch

        dr, dk, dv = _elems(roots), _elems(keys), _elems(values)
        m = dk.numel() // 4
        old = torch.empty((m, self.height, 8, 4), dtype=torch.int64, device="cuda")
        new = torch.empty_like(old)
        old_values = torch.empty((m, 4), dtype=torch.int64, device="cuda")
        new_roots = torch.empty((m, 4), dtype=torch.int64, device="cuda")
        status = torch.empty(max(m, 1), dtype=torch.int32, device="cuda")
        missing = ctypes.c_uint64()
        _lib.check(_lib.load().lurk_hip_trie_nodes_prove_insert_dev(self._h, _lib.ptr(dr), self._stride(dr, m), _lib.ptr(dk), _lib.ptr(dv), m, _lib.ptr(old),
                                                                    _lib.ptr(new), _lib.ptr(old_values), _lib.ptr(new_roots), _lib.ptr(status),
                                                                    ctypes.byref(missing), 1 if register_new else 0, _lib.ptr(stream)))
        return old, new, old_values, new_roots, status[:m], missing.value

    def insert_chain(self, root: int, keys, values, *, paths=True, stream=None):
        """A chain of dependent insertions that starts at the trie named by ``root`` (a Python int) -> (old paths, new paths, old values,
        roots); every ``roots[i]`` is addressable afterwards and the result is ``roots[-1]``"""
        import torch

        dk, dv = _elems(keys), _elems(values)
        m = dk.numel() // 4 if hasattr(dk, "numel") else 0
        old = torch.empty((m, self.height, 8, 4), dtype=torch.int64, device="cuda") if paths else None
        new = torch.empty_like(old) if paths else None
        old_values = torch.empty((m, 4), dtype=torch.int64, device="cuda")
        roots = torch.empty((m, 4), dtype=torch.int64, device="cuda")
        root32 = _limbs([int(root)])
        _lib.check(_lib.load().lurk_hip_trie_nodes_insert_chain_dev(self._h, _lib.ptr(root32), _lib.ptr(dk) if m else None, _lib.ptr(dv) if m else None, m,
                                                                    _lib.ptr(old) if paths else None, _lib.ptr(new) if paths else None, _lib.ptr(old_values),
                                                                    _lib.ptr(roots), _lib.ptr(stream)))
        return old, new, old_values, roots

    def close(self):
        """Frees the table (296 B per slot).  Idempotent; the handle is unusable afterwards."""
        h, self._h = self._h, None
        if h:
            _lib.check(_lib.load().lurk_hip_trie_nodes_destroy(h))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        if getattr(self, "_h", None) is None:
            return
        try:
            self.close()
        except Exception:
            pass


def verify_lookup_batch(field_id: int, height: int, roots, keys, values, paths, stream=None):
    """lurk_hip_trie_verify_lookup_dev: one root for all proofs (a single element) or one per proof -> (codes, n_failed)"""
    import torch

    dk, dv, dp, dr = _elems(keys), _elems(values), _elems(paths), _elems(roots)
    m = dk.numel() // 4
    stride = 0 if dr.numel() == 4 and m != 1 else 1
    codes = torch.zeros(max(m, 1), dtype=torch.int32, device="cuda")
    failed = ctypes.c_uint64()
    _lib.check(_lib.load().lurk_hip_trie_verify_lookup_dev(field_id, height, _lib.ptr(dr), stride, _lib.ptr(dk), _lib.ptr(dv), _lib.ptr(dp), m, _lib.ptr(codes),
                                                           ctypes.byref(failed), _lib.ptr(stream)))
    return codes[:m].cpu().numpy().view(np.uint32), failed.value


def verify_insert_batch(field_id: int, height: int, old_roots, new_roots, keys, old_values, new_values, old_paths, new_paths, stream=None):
    """lurk_hip_trie_verify_insert_dev: one (old, new) root pair for all proofs or one pair per proof -> (codes, n_failed)"""
    import torch

    dk, dov, dnv, dop, dnp = _elems(keys), _elems(old_values), _elems(new_values), _elems(old_paths), _elems(new_paths)
    dor, dnr = _elems(old_roots), _elems(new_roots)
    m = dk.numel() // 4
    assert dor.numel() == dnr.numel(), "as many old roots as new roots"
    stride = 0 if dor.numel() == 4 and m != 1 else 1
    codes = torch.zeros(max(m, 1), dtype=torch.int32, device="cuda")
    failed = ctypes.c_uint64()
    _lib.check(_lib.load().lurk_hip_trie_verify_insert_dev(field_id, height, _lib.ptr(dor), _lib.ptr(dnr), stride, _lib.ptr(dk), _lib.ptr(dov), _lib.ptr(dnv),
                                                           _lib.ptr(dop), _lib.ptr(dnp), m, _lib.ptr(codes), ctypes.byref(failed), _lib.ptr(stream)))
    return codes[:m].cpu().numpy().view(np.uint32), failed.value


def path_digits(field_id: int, height: int, keys) -> np.ndarray:
    """lurk_hip_trie_path_digits (host only): (len(keys), height) uint8"""
    k = _limbs(list(keys))
    out = np.zeros((len(k), height), dtype=np.uint8)
    _lib.check(_lib.load().lurk_hip_trie_path_digits(field_id, height, _lib.ptr(k), len(k), _lib.ptr(out)))
    return out
