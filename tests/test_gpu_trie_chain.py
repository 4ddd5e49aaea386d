"""GPU: chains of dependent inserts on the device-resident trie (lurk_hip_trie_insert_chain_dev, DeviceTrie.insert_chain) against the
reference's sequential inserts (tests/trie_ref.py: RefTrie.prove_insert one after the other, through tests/trie_chain_ref.py): old
paths, new paths, old values and every root element for element; the trie the chain leaves; optional outputs, refusals, streams.
Everything is bit-exact."""
import ctypes
import functools
import random
import threading

import numpy as np
import pytest

from oracle import coracle as C
from oracle import pyref as R
from tests import kat
from tests import trie_chain_ref as CH
from tests import trie_ref as T

pytestmark = pytest.mark.gpu

BN = kat.BN


def _ints(t) -> list[int]:
    return C.limbs_to_ints(t.cpu().numpy().view(np.uint64))


def _paths_np(paths, height) -> np.ndarray:
    flat = [x for proof in paths for pre in proof for x in pre]
    return C.ints_to_limbs(flat).reshape(len(paths), height, 8, 4)


def _u64(t) -> np.ndarray:
    return t.cpu().numpy().view(np.uint64)


def _assert_chain_equals_reference(t, base: T.RefTrie, updates, name=""):
    olds, news, old_values, roots = CH.sequential(base, updates)
    got_old, got_new, got_values, got_roots, _ = t.insert_chain([k for k, _ in updates], [v for _, v in updates], trie=False)
    assert _ints(got_roots) == roots, name
    assert _ints(got_values) == old_values, name
    assert np.array_equal(_u64(got_old), _paths_np(olds, base.height)), name
    assert np.array_equal(_u64(got_new), _paths_np(news, base.height)), name
    return roots


# ---- 1. the case families, three fields, four heights, an empty and a populated base ---------------------------------------------------
@pytest.mark.parametrize("populated", [False, True])
@pytest.mark.parametrize("height", [1, 2, 3, 5])
@pytest.mark.parametrize("field_id", [0, 1, 2])
def test_chain_equals_sequential_reference(hip, field_id, height, populated):
    from lurk_beta_amd.trie import DeviceTrie

    pairs = CH.base_pairs(field_id, height, populated)
    base = CH.base_trie(field_id, height, pairs)
    cases = CH.families(field_id, height, pairs)
    assert {"one key 64 times", "last digit alternating", "first digit alternating", "colliding random keys", "present and absent", "to zero and back",
            "repeats the current value", "one multiset, order a", "one multiset, order b"} == {name for name, _ in cases}
    with DeviceTrie.build(field_id, pairs, height) as t:
        root0 = t.root
        assert root0 == base.root
        ends = {}
        for name, updates in cases:
            assert len(updates) <= 200
            roots = _assert_chain_equals_reference(t, base, updates, name)
            ends[name] = roots
            assert t.root == root0, name  # the handle is not modified
        same = ends["repeats the current value"]
        assert same[0] == same[1]  # (k0, 5) twice: the second changes nothing
        a, b = (dict(cases)["one multiset, order " + x] for x in "ab")
        assert sorted(a) == sorted(b) and a != b and ends["one multiset, order a"][:-1] != ends["one multiset, order b"][:-1]


# ---- 2. the standard height: the reference's golden root, then 64 updates --------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _base85():
    rng = random.Random(85)
    p = R.modulus(BN)
    pairs = [(rng.randrange(p), rng.randrange(1, p)) for _ in range(32)]
    return tuple(pairs), CH.base_trie(BN, 85, pairs)


def _updates85():
    pairs, _ = _base85()
    rng = random.Random(8585)
    p = R.modulus(BN)
    fresh = [rng.randrange(p) for _ in range(20)]
    twin = fresh[0] ^ 5  # shares 84 digits with fresh[0]
    keys = [fresh[0], twin, fresh[0], twin] + [pairs[j][0] for j in range(12)] + fresh + [fresh[3]] * 6 + [pairs[2][0]] * 4
    keys += [rng.choice(fresh + [k for k, _ in pairs]) for _ in range(64 - len(keys))]
    assert len(keys) == 64 and T.path(BN, twin, 85)[:84] == T.path(BN, fresh[0], 85)[:84]
    return [(k, rng.choice([0, rng.randrange(1, p), rng.randrange(1, p)])) for k in keys]


def test_standard_height_golden_root_and_a_chain_of_64(hip):
    from lurk_beta_amd.trie import DeviceTrie

    with DeviceTrie.build(BN, [], 85) as empty:
        assert empty.root == kat.golden_int("empty_root_85")
        old, new, values, roots, grown = empty.insert_chain([123], [456])
        assert _ints(roots) == [kat.golden_int("trie_insert_123_456")] and _ints(values) == [0]
        assert grown.root == kat.golden_int("trie_insert_123_456") and grown.n == 1
        grown.close()
    pairs, base = _base85()
    with DeviceTrie.build(BN, pairs, 85) as t:
        _assert_chain_equals_reference(t, base, _updates85())


# ---- 3. a chain of one is prove_insert -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("height,present", [(85, True), (85, False), (3, True)])
def test_a_chain_of_one_is_prove_insert(hip, height, present):
    import torch

    from lurk_beta_amd.trie import DeviceTrie

    pairs = _base85()[0] if height == 85 else CH.base_pairs(BN, height, True)
    key = pairs[3][0] if present else pairs[3][0] ^ 0x1F0
    with DeviceTrie.build(BN, pairs, height) as t:
        want = t.prove_insert([key], [777])
        got = t.insert_chain([key], [777], trie=False)
        for a, b in zip(want, got[:4]):
            assert torch.equal(a, b)


# ---- 4. at size, checked by the library's own verifier ---------------------------------------------------------------------------------
def test_4096_updates_pass_the_insert_verifier_and_a_corrupted_proof_does_not(hip):
    import torch

    from lurk_beta_amd.trie import DeviceTrie, _elems, verify_insert_batch

    H, n, m = 85, 1 << 12, 1 << 12
    rng = random.Random(4096)
    p = R.modulus(BN)
    base = [(rng.randrange(p), rng.randrange(1, p)) for _ in range(n)]
    hot = [base[j][0] for j in range(8)] + [rng.randrange(p) for _ in range(8)]
    keys = [rng.choice(hot) if j % 8 == 3 else (rng.choice(base)[0] if j % 8 == 5 else rng.randrange(p)) for j in range(m)]
    values = [rng.randrange(p) for _ in range(m)]
    with DeviceTrie.build(BN, base, H) as t:
        dk, dv = _elems(keys), _elems(values)
        old, new, old_values, roots, _ = t.insert_chain(dk, dv, trie=False)
        old_roots = torch.cat([t._root_dev(), roots[:-1]])
        codes, failed = verify_insert_batch(BN, H, old_roots, roots, dk, old_values, dv, old, new)
        assert failed == 0 and not codes.any()
        assert len({tuple(r) for r in _u64(roots).tolist()}) == m  # every update moved the root
        j, d = 2345, 40
        new[j, d, (T.path(BN, keys[j], H)[d] + 1) % 8, 0] ^= 1
        codes, failed = verify_insert_batch(BN, H, old_roots, roots, dk, old_values, dv, old, new)
        assert failed == 1 and list(np.nonzero(codes)[0]) == [j] and codes[j] == 0x100 + d + 1


# ---- 5. the trie the chain leaves ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field_id,height,populated", [(BN, 85, True), (BN, 3, True), (0, 5, False), (1, 2, True)])
def test_out_trie_is_the_built_trie_of_the_final_pairs(hip, field_id, height, populated):
    import torch

    from lurk_beta_amd.trie import DeviceTrie

    if height == 85:
        pairs, updates = list(_base85()[0]), _updates85()
    else:
        pairs = CH.base_pairs(field_id, height, populated)
        updates = dict(CH.families(field_id, height, pairs))["present and absent"] + dict(CH.families(field_id, height, pairs))["to zero and back"]
    final = CH.final_pairs(pairs, updates, height)
    untouched = [k for k, _ in pairs if k not in {u for u, _ in updates}] + [(updates[0][0] ^ 1) | 6]
    queries = [k for k, _ in updates] + untouched
    with DeviceTrie.build(field_id, pairs, height) as t, DeviceTrie.build(field_id, final, height) as built:
        root0 = t.root
        _, _, _, roots, grown = t.insert_chain([k for k, _ in updates], [v for _, v in updates])
        with grown:
            assert _ints(roots)[-1] == grown.root == built.root
            n = ctypes.c_size_t()
            assert hip.lurk_hip_trie_info(grown._h, None, None, ctypes.byref(n), None) == 0
            assert n.value == grown.n == len(final) == len({k & ((1 << (3 * height)) - 1) for k, _ in pairs + updates})
            for a, b in zip(grown.prove_lookup(queries), built.prove_lookup(queries)):
                assert torch.equal(a, b)
        # no update: a handle of its own with the root of t
        none = t.insert_chain([], [])
        assert none[0].shape[0] == 0 and none[3].shape[0] == 0
        with none[4] as copy:
            assert copy.root == root0 and copy.n == t.n and copy._h.value != t._h.value
        assert t.root == root0


# ---- 6. optional outputs ---------------------------------------------------------------------------------------------------------------
def test_optional_outputs(hip):
    import torch

    from lurk_beta_amd import LurkHipError, _lib
    from lurk_beta_amd.trie import DeviceTrie, _elems

    height = 5
    pairs = CH.base_pairs(BN, height, True)
    updates = dict(CH.families(BN, height, pairs))["colliding random keys"]
    dk, dv = _elems([k for k, _ in updates]), _elems([v for _, v in updates])
    m = len(updates)
    call = hip.lurk_hip_trie_insert_chain_dev
    with DeviceTrie.build(BN, pairs, height) as t:
        old, new, old_values, roots, grown = t.insert_chain(dk, dv)
        want_root = grown.root
        grown.close()
        # only the roots
        r = torch.zeros_like(roots)
        _lib.check(call(t._h, _lib.ptr(dk), _lib.ptr(dv), m, None, None, None, _lib.ptr(r), None, None))
        assert torch.equal(r, roots)
        # only the trie
        h = ctypes.c_void_p()
        _lib.check(call(t._h, _lib.ptr(dk), _lib.ptr(dv), m, None, None, None, None, ctypes.byref(h), None))
        with DeviceTrie(h, BN, height, 0) as only:
            assert only.root == want_root
        # the paths without the trie (and without the roots), one path buffer at a time
        o, n_, v = torch.zeros_like(old), torch.zeros_like(new), torch.zeros_like(old_values)
        _lib.check(call(t._h, _lib.ptr(dk), _lib.ptr(dv), m, _lib.ptr(o), _lib.ptr(n_), _lib.ptr(v), None, None, None))
        assert torch.equal(o, old) and torch.equal(n_, new) and torch.equal(v, old_values)
        n_.zero_()
        _lib.check(call(t._h, _lib.ptr(dk), _lib.ptr(dv), m, None, _lib.ptr(n_), None, None, None, None))
        assert torch.equal(n_, new)
        got = t.insert_chain(dk, dv, paths=False, trie=False)
        assert got[0] is None and got[1] is None and got[4] is None and torch.equal(got[2], old_values) and torch.equal(got[3], roots)
        with pytest.raises(LurkHipError, match="no output") as e:
            _lib.check(call(t._h, _lib.ptr(dk), _lib.ptr(dv), m, None, None, None, None, None, None))
        assert e.value.code == 2


# ---- 7. refusals leave everything as it was --------------------------------------------------------------------------------------------
def test_refusals_leave_the_trie_and_the_handle_slot_alone(hip):
    import torch

    from lurk_beta_amd import LurkHipError, _lib
    from lurk_beta_amd.trie import DeviceTrie, _elems

    height, p = 5, R.modulus(BN)
    pairs = CH.base_pairs(BN, height, True)
    probe = pairs[0][0]
    call = hip.lurk_hip_trie_insert_chain_dev
    with DeviceTrie.build(BN, pairs, height) as t:
        root0 = t.root
        proof0 = [x.clone() for x in t.prove_lookup([probe])]

        def unchanged():
            assert t.root == root0
            for a, b in zip(t.prove_lookup([probe]), proof0):
                assert torch.equal(a, b)

        m = 6
        good_k, good_v = [probe, 3, 4, probe, 5, 3], [9, 8, 0, 7, 6, 5]
        buf = lambda: torch.zeros((m, height, 8, 4), dtype=torch.int64, device="cuda")
        o, n_, v, r = buf(), buf(), torch.zeros((m, 4), dtype=torch.int64, device="cuda"), torch.zeros((m, 4), dtype=torch.int64, device="cuda")
        slot = ctypes.c_void_p(0x5A5A)

        def refused(match, handle, keys, values, old, new):
            dk, dv = _elems(keys), _elems(values)
            with pytest.raises(LurkHipError, match=match) as e:
                _lib.check(call(handle, _lib.ptr(dk), _lib.ptr(dv), m, old, new, _lib.ptr(v), _lib.ptr(r), ctypes.byref(slot), None))
            assert e.value.code == 2 and slot.value == 0x5A5A
            assert not o.any() and not n_.any() and not v.any() and not r.any()  # nothing was launched
            unchanged()

        for j in (0, 4, 5):
            bad = list(good_k)
            bad[j] = p + j
            refused(rf"key {j} is not reduced", t._h, bad, good_v, _lib.ptr(o), _lib.ptr(n_))
            bad = list(good_v)
            bad[j] = p
            refused(rf"value {j} is not reduced", t._h, good_k, bad, _lib.ptr(o), _lib.ptr(n_))
        refused("overlap", t._h, good_k, good_v, _lib.ptr(o), o.data_ptr() + 256 * height * (m - 1))
        refused("null trie handle", None, good_k, good_v, _lib.ptr(o), _lib.ptr(n_))
        # and a call that succeeds leaves t alone too
        got = t.insert_chain(good_k, good_v)
        unchanged()
        assert got[4].root == _ints(got[3])[-1] != root0
        got[4].close()


# ---- 8. two chains on two streams over one handle --------------------------------------------------------------------------------------
def test_two_streams_one_handle(hip):
    import torch

    from lurk_beta_amd.trie import DeviceTrie, _elems

    pairs, _ = _base85()
    rng = random.Random(2)
    p = R.modulus(BN)
    chains = []
    for _ in range(2):
        keys = [rng.choice([rng.randrange(p), pairs[rng.randrange(32)][0]]) for _ in range(300)]
        chains.append((_elems(keys), _elems([rng.randrange(p) for _ in keys])))
    with DeviceTrie.build(BN, pairs, 85) as t:
        alone = [t.insert_chain(k, v) for k, v in chains]
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        both, errors = [None, None], []

        def run(j):
            try:
                both[j] = t.insert_chain(*chains[j], stream=streams[j].cuda_stream)
            except Exception as e:  # surfaced below: an exception in a thread is otherwise lost
                errors.append(e)

        threads = [threading.Thread(target=run, args=(j,)) for j in range(2)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert not errors, errors
        for a, b in zip(alone, both):
            for x, y in zip(a[:4], b[:4]):
                assert torch.equal(x, y)
            assert a[4].root == b[4].root
            a[4].close()
            b[4].close()
