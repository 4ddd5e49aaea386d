"""The sparse trie of the reference (src/coprocessor/trie/mod.rs), restated in Python integers: the checker of the device-resident
trie (lurk_hip_trie_*) and of the host mirror.  ``children`` is the reference's child map (hash -> preimage, :453-458); every hash goes
through the C oracle (oracle.coracle.poseidon_batch), memoised per field."""
from __future__ import annotations

from oracle import coracle as C
from oracle import pyref as R

ARITY = 8
_MEMO: dict[int, dict[tuple, int]] = {}


def hash8(field_id: int, preimage) -> int:
    memo = _MEMO.setdefault(field_id, {})
    key = tuple(int(x) for x in preimage)
    if key not in memo:
        assert len(key) == ARITY
        memo[key] = C.limbs_to_ints(C.poseidon_batch(field_id, ARITY, C.ints_to_limbs(list(key)).reshape(1, ARITY, 4)))[0]
    return memo[key]


def path(field_id: int, key: int, height: int) -> list[int]:
    """``Trie::path`` (:589-608): the key's bits most significant first, the last 3 * height of them, in 3-bit big-endian chunks."""
    nbits = R.FIELD_NUM_BITS[field_id]
    bits = [(key >> i) & 1 for i in range(nbits)]
    bits.reverse()
    need = 3 * height
    if need > len(bits):
        bits = [0] * (need - len(bits)) + bits
    tail = bits[len(bits) - need:]
    out = []
    for i in range(0, need, 3):
        acc = 0
        for b in tail[i:i + 3]:
            acc = acc * 2 + b
        out.append(acc)
    return out


class RefTrie:
    def __init__(self, field_id: int, height: int):
        self.field_id, self.height = field_id, height
        self.children: dict[int, tuple[int, ...]] = {}
        self.empty_roots: list[int] = []
        self.init_empty()
        self.root = self.empty_roots[height - 1]

    def copy(self) -> "RefTrie":
        t = object.__new__(RefTrie)
        t.field_id, t.height, t.children, t.empty_roots, t.root = self.field_id, self.height, dict(self.children), self.empty_roots, self.root
        return t

    def register_hash(self, preimage) -> int:
        h = hash8(self.field_id, preimage)
        self.children[h] = tuple(preimage)
        return h

    # :464-481
    def init_empty(self):
        cur = 0
        for _ in range(self.height):
            cur = self.register_hash([cur] * ARITY)
            self.empty_roots.append(cur)

    def path(self, key: int) -> list[int]:
        return path(self.field_id, key, self.height)

    # :725-743
    def prove_lookup_at_path(self, p: list[int]) -> list[tuple[int, ...]]:
        preimages, nxt = [], self.root
        for k in p:
            pre = self.children[nxt]  # KeyError = Error::MissingPreimage
            preimages.append(pre)
            nxt = pre[k]
        return preimages

    def prove_lookup(self, key: int) -> list[tuple[int, ...]]:
        return self.prove_lookup_at_path(self.path(key))

    def lookup(self, key: int):
        p = self.path(key)
        v = self.prove_lookup_at_path(p)[-1][p[-1]]
        return None if v == 0 else v

    # :760-800
    def insert_at_path(self, p: list[int], value: int):
        old = self.prove_lookup_at_path(p)
        new = []
        for k, existing in zip(reversed(p), reversed(old)):
            pre = list(existing)
            pre[k] = value
            value = self.register_hash(pre)
            new.append(tuple(pre))
        new.reverse()
        inserted = value != self.root
        self.root = value
        return old, new, inserted

    def prove_insert(self, key: int, value: int):
        return self.insert_at_path(self.path(key), value)

    def insert(self, key: int, value: int) -> bool:
        return self.prove_insert(key, value)[2]


def verify_lookup(field_id: int, height: int, root: int, key: int, value: int, preimage_path) -> int:
    """``LookupProof::verify`` (:349-362) as a code: 0 = true; k + 1 = ``next != computed_hash`` at preimage k; height + 1 = ``next != value``."""
    nxt = root
    for k, (digit, pre) in enumerate(zip(path(field_id, key, height), preimage_path)):
        if nxt != hash8(field_id, pre):
            return k + 1
        nxt = pre[digit]
    return 0 if nxt == value else height + 1


def verify_insert(field_id: int, height: int, old_root: int, new_root: int, key: int, old_value, new_value: int, old_path, new_path) -> int:
    """``InsertProof::verify`` (:383-424) as a code, the first failing check: the old proof (1 .. H + 1), a level at which the paths differ
    in more than one position (0x100 + level + 1), the new proof (0x200 + 1 .. H + 1)."""
    code = verify_lookup(field_id, height, old_root, key, 0 if old_value is None else old_value, old_path)
    if code:
        return code
    for level, (a, b) in enumerate(zip(old_path, new_path)):
        if tuple(a) != tuple(b) and sum(x != y for x, y in zip(a, b)) > 1:
            return 0x100 + level + 1
    code = verify_lookup(field_id, height, new_root, key, new_value, new_path)
    return 0x200 + code if code else 0
