"""A Python restatement of the trie coprocessor's two step-circuit bodies over oracle.circuit_ref.WitnessCS: what
Trie::synthesize_lookup (/root/reference/src/coprocessor/trie/mod.rs:652-714) and Trie::synthesize_insert (:802-880) allocate and enforce.

TEST INFRASTRUCTURE ONLY.  The composition is read from the reference line by line; the two inner gadgets (neptune's
poseidon_hash_allocated, bellpepper's to_bits_le_strict) are oracle/circuit_ref.py's, imported and unchanged.

Column convention of the library (include/lurk_hip.h): the block is what the two functions allocate, preceded by the two (three)
AllocatedNums they are handed - allocated_root at local column 0, the key as element 0 of its bit-decomposition block, the new value
between the lookup's allocations and synthesize_modify_value_at_path's.  Children are not looked up by hash: the preimages of the proof
are allocated as they are given, which is what the reference allocates for a trie that holds the proof's nodes."""
from __future__ import annotations

from oracle import circuit_ref as CR
from oracle import pyref as R

LOOKUP, INSERT = 0, 1
ARITY, ARITY_BITS = 8, 3


def synthesize_path(cs, height: int, key_var: int):
    """synthesize_path (:611-629): H chunks of three little-endian bits, root level first; None = Boolean::Constant(false)"""
    bits = list(CR.bits_le_strict(cs, key_var))            # :617
    bits += [None] * (ARITY_BITS * height - len(bits))     # :618-620
    bits.reverse()                                         # :621
    tail = bits[len(bits) - ARITY_BITS * height:]          # :624
    return [list(reversed(tail[i:i + ARITY_BITS])) for i in range(0, len(tail), ARITY_BITS)]  # :625-627


def _bool_value(cs, bit) -> bool:
    return bool(cs.aux[bit - 1]) if bit is not None else False


def pick(cs, cond, a: int, b: int) -> int:
    """pick (/root/reference/src/circuit/gadgets/constraints.rs:364-391): a if cond else b; (b - a) * cond = (b - c)"""
    p = cs.p
    c = cs.alloc(cs.aux[a - 1] if _bool_value(cs, cond) else cs.aux[b - 1])
    cs.enforce({b: 1, a: p - 1}, {cond: 1} if cond is not None else {}, {b: 1, c: p - 1})
    return c


def select(cs, frm: list[int], path_bits: list) -> int:
    """select (constraints.rs:334-361)"""
    assert 1 << len(path_bits) == len(frm)
    state, half = list(frm), len(frm) // 2
    for bit in reversed(path_bits):
        state = [pick(cs, bit, state[half + j], state[j]) for j in range(half)]
        half //= 2
    return state[0]


def synthesize_lookup_at_path(cs, field_id: int, root_var: int, path, preimages):
    """synthesize_lookup_at_path (:668-714) -> (found, preimage_path)"""
    preimage_path, nxt = [], root_var
    for k_bits, pre in zip(path, preimages):
        allocated = [cs.alloc(f) for f in pre]                        # :684-699
        preimage_path.append(allocated)
        hashed = CR.poseidon_hash_allocated(cs, field_id, allocated)  # :703-707
        cs.enforce({hashed: 1}, {0: 1}, {nxt: 1})                     # enforce_equal(hashed, next), constraints.rs:14-31
        nxt = select(cs, allocated, k_bits)                           # :711
    return nxt, preimage_path


def index_from_bits(cs, bits) -> int:
    """index_from_bits (:883-892): little-endian"""
    return sum(int(_bool_value(cs, b)) << i for i, b in enumerate(bits))


def synthesize_modify_value_at_path(cs, field_id: int, path, preimage_path, value_var: int) -> int:
    """synthesize_modify_value_at_path (:846-880): from the leaf level upward; nothing ties the new preimage to the old one"""
    for path_bits, existing in reversed(list(zip(path, preimage_path))):
        idx = index_from_bits(cs, path_bits)
        new = [cs.alloc(cs.aux[(value_var if j == idx else existing[j]) - 1]) for j in range(ARITY)]
        value_var = CR.poseidon_hash_allocated(cs, field_id, new)
    return value_var


def trie_circuit(field_id: int, height: int, op: int, root: int, key: int, old_path, value: int | None = None):
    """-> (cs, result variable, value variable or None).  old_path: H preimages of 8 ints, root level first."""
    assert len(old_path) == height and all(len(pre) == ARITY for pre in old_path)
    cs = CR.WitnessCS(R.modulus(field_id))
    root_var = cs.alloc(root)
    key_var = cs.alloc(key)
    path = synthesize_path(cs, height, key_var)                                                 # :659 / :810
    found, preimage_path = synthesize_lookup_at_path(cs, field_id, root_var, path, old_path)  # :661-663 / :828-835
    if op == LOOKUP:
        return cs, found, None
    value_var = cs.alloc(value)
    return cs, synthesize_modify_value_at_path(cs, field_id, path, preimage_path, value_var), value_var  # :837-843


def rows(cs):
    """The recorded constraints in the library's convention: per row three sorted lists of (local column, coefficient != 0); variable v >= 1
    is column v - 1, ONE is column len(aux)."""
    size, p = len(cs.aux), cs.p
    return [tuple(sorted(((size if k == 0 else k - 1), v % p) for k, v in lc.items() if v % p) for lc in abc) for abc in cs.constraints]


def key_block_size(field_id: int) -> int:
    return CR.slot_witness_size(field_id, "bit_decomp")


def closed_forms(field_id: int, height: int, op: int):
    """(size, rows, result_col, value_col) as the issue states them"""
    b = key_block_size(field_id)
    size_lookup, rows_lookup = 1 + b + 403 * height, b + 396 * height
    if op == LOOKUP:
        return size_lookup, rows_lookup, size_lookup - 1, None
    size = size_lookup + 1 + 396 * height
    return size, b + 784 * height, size - 1, size_lookup
