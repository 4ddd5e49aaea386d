"""GPU: what tests/test_gpu_trie.py leaves open.  Tries of more than one block of keys (nodes whose key ranges cross block boundaries,
blocks with many and with no node at a depth); the host mirror's proofs (lurk_beta_amd.trie.Trie.prove_lookup / prove_insert,
verify_lookup / verify_insert: every hash one launch of the GPU hasher) against the Python restatement of the reference
(tests/trie_ref.py); the device verifiers' refusal of a preimage element that is not reduced; the handle's lifetime."""
import random

import numpy as np
import pytest

from oracle import coracle as C
from oracle import pyref as R
from tests import kat
from tests import trie_ref as T

pytestmark = pytest.mark.gpu

BN = kat.BN
H = 3
# two keys in one leaf node, one that leaves them at depth 1, one at depth 0, one value of 0
PAIRS = [(0o123, 11), (0o127, 12), (0o157, 0), (0o523, 14)]
ABSENT = [0o124, 0o160, 0o700]


def _pair():
    from lurk_beta_amd.trie import Trie

    mirror, ref = Trie(BN, height=H), T.RefTrie(BN, H)
    for k, v in PAIRS:
        assert mirror.insert(k, v) == (ref.lookup(k) is not None)
        ref.insert(k, v)
    assert mirror.root == ref.root
    return mirror, ref


def test_mirror_lookup_proofs_and_verifier(hip):
    from lurk_beta_amd import verify_lookup

    mirror, ref = _pair()
    p = R.modulus(BN)
    for key in [k for k, _ in PAIRS] + ABSENT:
        proof = mirror.prove_lookup(key)
        assert proof == ref.prove_lookup(key)
        value = ref.lookup(key) or 0
        assert (mirror.lookup(key) or 0) == value
        assert verify_lookup(mirror, mirror.root, key, value, proof) == 0
    # the codes of the reference's verifier on every single tamper of one proof
    key, value = PAIRS[0]
    digits, honest = ref.path(key), ref.prove_lookup(key)
    cases = [(ref.root, (value + 1) % p, honest), ((ref.root + 1) % p, value, honest)]
    for k in range(H):
        for pos in (digits[k], (digits[k] + 1) % 8):
            bad = [list(x) for x in honest]
            bad[k][pos] = (bad[k][pos] + 1) % p
            cases.append((ref.root, value, [tuple(x) for x in bad]))
    want = [T.verify_lookup(BN, H, r, key, v, pth) for r, v, pth in cases]
    assert want[:2] == [H + 1, 1] and all(want)
    assert [verify_lookup(mirror, r, key, v, pth) for r, v, pth in cases] == want


def test_mirror_insert_proofs_and_verifier(hip):
    from lurk_beta_amd import verify_insert

    mirror, ref = _pair()
    p = R.modulus(BN)
    # a fresh key, an existing key with a new value, an existing key with the value it has (nothing inserted)
    for key, value in [(ABSENT[0], 21), (PAIRS[1][0], 22), (PAIRS[3][0], PAIRS[3][1])]:
        old_root, old_value = ref.root, ref.lookup(key)
        old, new, inserted = mirror.prove_insert(key, value)
        assert (old, new, inserted) == ref.prove_insert(key, value)
        assert mirror.root == ref.root and inserted == (value != (old_value or 0))
        assert verify_insert(mirror, old_root, mirror.root, key, old_value, value, old, new) == 0
        digits = ref.path(key)
        two = [list(x) for x in new]
        for off in ((digits[1] + 1) % 8, (digits[1] + 2) % 8):  # two positions off the path, whatever the insertion changed on it
            two[1][off] = (two[1][off] + 1) % p
        two = [tuple(x) for x in two]
        cases = [(old_root, ref.root, old_value, value, old, two, 0x100 + 2),
                 (old_root, (ref.root + 1) % p, old_value, value, old, new, 0x201),
                 (old_root, ref.root, old_value, (value + 1) % p, old, new, 0x200 + H + 1),
                 ((old_root + 1) % p, ref.root, old_value, value, old, new, 1)]
        for r0, r1, v0, v1, a, b, code in cases:
            assert T.verify_insert(BN, H, r0, r1, key, v0, v1, a, b) == code
            assert verify_insert(mirror, r0, r1, key, v0, v1, a, b) == code


@pytest.mark.parametrize("field_id", [0, 1, 2])
def test_device_verifiers_refuse_an_unreduced_preimage_element(hip, field_id):
    """x and x + p hash alike (the hash is a function of the residue), so a verifier that took both would let two byte strings open one
    node: preimage k with one element + p fails level k, code k + 1, on and off the path, in both verifiers."""
    from lurk_beta_amd.trie import DeviceTrie, verify_insert_batch, verify_lookup_batch

    height = 5
    p = R.modulus(field_id)
    assert 2 * p < 1 << 256  # x + p still fits the 32 bytes
    pairs = [(0o12345, 7), (0o12346, 8), (0o52345, 9)]
    key, new_value = 0o12345, 70
    with DeviceTrie.build(field_id, pairs, height) as t:
        paths, values = t.prove_lookup([key])
        # the second insertion writes the value the key has: its two paths are equal and its new root is the old one
        old, new, old_values, new_roots = t.prove_insert([key, key], [new_value, 7])
        root = t.root
    digits = T.path(field_id, key, height)
    honest = paths.cpu().numpy().view(np.uint64)
    old, new = old.cpu().numpy().view(np.uint64), new.cpu().numpy().view(np.uint64)
    new_root, same_root = C.limbs_to_ints(new_roots.cpu().numpy().view(np.uint64))
    assert same_root == root and np.array_equal(old[1], new[1]) and np.array_equal(old[0], old[1])

    def plus_p(proof, level, pos):
        out = proof.copy()
        x = C.limbs_to_ints(out[0, level, pos].reshape(1, 4))[0]
        out[0, level, pos] = C.ints_to_limbs([x + p]).reshape(4)
        return out

    spots = [(k, pos) for k in (0, height // 2, height - 1) for pos in (digits[k], (digits[k] + 1) % 8)]
    batch = np.concatenate([honest] + [plus_p(honest, k, pos) for k, pos in spots])
    m = len(batch)
    codes, failed = verify_lookup_batch(field_id, height, [root], [key] * m, [7] * m, batch)
    assert list(codes) == [0] + [k + 1 for k, _ in spots] and failed == m - 1
    # the insert verifier.  In the old path: the old proof fails, k + 1.  In the new path alone, of the insertion that changes nothing: the
    # paths differ in that one position only, so the new proof is reached and fails, 0x200 + k + 1.  In the new path of the insertion that
    # changes the value: off the path it is a second differing position of its level, 0x100 + k + 1.
    o0, n0, o1, n1 = old[:1], new[:1], old[1:], new[1:]
    m = 1 + 3 * len(spots)
    olds, news, roots, values_new, want = [o0], [n0], [new_root], [new_value], [0]
    for k, pos in spots:
        olds += [plus_p(o0, k, pos), o1, o0]
        news += [n0, plus_p(n1, k, pos), plus_p(n0, k, pos)]
        roots += [new_root, root, new_root]
        values_new += [new_value, 7, new_value]
        want += [k + 1, 0x200 + k + 1, 0x100 + k + 1 if pos != digits[k] else 0x200 + k + 1]
    codes, failed = verify_insert_batch(field_id, height, [root] * m, roots, [key] * m, [7] * m, values_new, np.concatenate(olds), np.concatenate(news))
    assert list(codes) == want and failed == m - 1


def test_handle_lifetime(hip):
    """close() twice is one destroy, a closed handle is refused by the library, and a handle that is dropped unclosed is destroyed by its
    finaliser (the destroy is observed through the handle it clears)."""
    import gc

    from lurk_beta_amd import LurkHipError
    from lurk_beta_amd.trie import DeviceTrie

    t = DeviceTrie.build(BN, PAIRS, H)
    assert t.root == _pair()[1].root
    t.close()
    t.close()
    assert t._h is None
    with pytest.raises(LurkHipError, match="null"):
        t.prove_lookup([1])
    # dropped unclosed: the finaliser calls close(), watched here through the class
    seen, orig = [], DeviceTrie.close
    t = DeviceTrie.build(BN, PAIRS, H)
    try:
        DeviceTrie.close = lambda self: (seen.append(bool(self._h)), orig(self))[1]
        del t
        gc.collect()
    finally:
        DeviceTrie.close = orig
    assert seen == [True]


@pytest.mark.parametrize("field_id,height,n", [(BN, 4, 700), (0, 3, 300), (BN, 12, 300)])
def test_more_than_one_block_of_keys(hip, field_id, height, n):
    """256 keys to a block: with 700 keys in 8^4 leaves (300 in 8^3) most nodes of the lower levels hold several keys, many ranges cross a block
    boundary and every block compacts a different number of nodes; with 300 keys in 8^12 the second block has no node at most depths."""
    from lurk_beta_amd.trie import DeviceTrie

    rng = random.Random(7 * height + n)
    keys = rng.sample(range(8 ** min(height, 5)), n)
    if height > 5:  # spread over the upper digits too, and a run of 40 keys that share all but their last two digits
        keys = [k << (3 * (height - 5)) | rng.getrandbits(3 * (height - 5)) for k in keys[:n - 40]] + [(0o7654321 << 6) | j for j in range(40)]
    pairs = [(k, rng.randrange(1, R.modulus(field_id))) for k in keys]
    ref = T.RefTrie(field_id, height)
    for k, v in pairs:
        ref.insert(k, v)
    by_path = sorted(keys)
    queries = [by_path[0], by_path[255], by_path[256], by_path[257], by_path[-1], by_path[511 % n]]
    queries += [k for k in range(8 ** min(height, 5) - 1, 0, -1) if k not in set(keys)][:2]
    with DeviceTrie.build(field_id, pairs, height) as t:
        assert t.n == n and t.root == ref.root
        paths, values = t.prove_lookup(queries)
        assert C.limbs_to_ints(values.cpu().numpy().view(np.uint64)) == [ref.lookup(k) or 0 for k in queries]
        want = C.ints_to_limbs([x for k in queries for pre in ref.prove_lookup(k) for x in pre]).reshape(len(queries), height, 8, 4)
        assert np.array_equal(paths.cpu().numpy().view(np.uint64), want)
