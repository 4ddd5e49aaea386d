"""The device-resident store (lurk_hip_store / DeviceStore) on the GPU.  The only reference for digests is the oracle's hydration of the
WHOLE DAG (oracle.c: orc_store_hydrate, the node-by-node recursion) - or, in the hand-built case, pyref's Poseidon on the StoreHasher
layouts written out below: appends in any batches must leave what one shot leaves, each node hashed exactly once."""
import functools

import numpy as np
import pytest

from lurk_beta_amd import DeviceStore, LurkHipError, MultiFrameWitness, _lib
from lurk_beta_amd import store_hasher as SH
from lurk_beta_amd.witness import SLOT_ORDER
from oracle import coracle as C
from oracle import pyref as R

pytestmark = pytest.mark.gpu

FQ, BN = 1, 2  # LURK_FIELD_PALLAS_FQ, LURK_FIELD_BN254_FR
CUTS = (1, 7, 64, 1009)  # prefix lengths at which a DAG is cut into batches: inside a symbol chain, inside a level, inside the spine


def _alternating_dag():
    """levels that alternate between one node and many (test_store_hydration_deep_and_wide_dags_every_digest's third shape)"""
    nodes = []
    prev = [SH._symbol_nodes(nodes, ["a%d" % j]) for j in range(64)]
    for rnd in range(6):
        nodes.append(("tuple2", 1, prev[0], prev[1]))
        top = len(nodes) - 1
        prev = [top] + prev[2:]
        nxt = []
        for j in range(len(prev)):
            nodes.append(("tuple2", 1, prev[j], top))
            nxt.append(len(nodes) - 1)
        prev = nxt
    return nodes


@functools.lru_cache(maxsize=None)
def _case(name):
    """(field, nodes, oracle digests of the whole DAG, oracle levels, number of hashed nodes): computed once, shared, never modified"""
    f, nodes = {"list37_bn": lambda: (BN, SH.list_dag(37)), "list400": lambda: (FQ, SH.list_dag(400)), "wide2000": lambda: (FQ, SH.wide_dag(2000)),
                "alternating": lambda: (FQ, _alternating_dag())}[name]()
    rec, vals = SH.encode(nodes)
    want, levels = C.store_hydrate(f, rec, vals)
    want.setflags(write=False)
    return f, nodes, want, levels, int(np.count_nonzero(rec[:, 0]))


def _batches(n, cuts):
    edges = [0] + [c for c in cuts if c < n] + [n]
    return list(zip(edges[:-1], edges[1:]))


def _check_whole(store, f, want, levels, hashed):
    info = store.info()
    assert info["field_id"] == f and info["n_nodes"] == want.shape[0] and info["capacity"] >= want.shape[0]
    assert info["levels"] == levels
    assert info["hashes_done"] == hashed, "every node is hashed exactly once"
    assert np.array_equal(store.digests(np.arange(want.shape[0])), want)


@pytest.mark.parametrize("name", ["list37_bn", "list400", "wide2000", "alternating"])
@pytest.mark.parametrize("cuts", [CUTS, ()], ids=["prefix_cuts", "all_at_once"])
def test_batches_equal_one_shot(hip, name, cuts):
    f, nodes, want, levels, hashed = _case(name)
    with DeviceStore(f) as store:
        for k, (a, b) in enumerate(_batches(len(nodes), cuts)):
            if k & 1 or not cuts:  # the digests of the new nodes come back when asked for
                first, got = store.append(nodes[a:b], digests=True)
                assert np.array_equal(got, want[a:b]), (name, a, b)
            else:
                first = store.append(nodes[a:b])
            assert first == a and len(store) == b
        _check_whole(store, f, want, levels, hashed)


def test_growth_from_a_capacity_of_eight(hip):
    """reserve_nodes = 8: the arrays grow between appends and inside one (945 nodes into a capacity of 64), device to device"""
    f, nodes, want, levels, hashed = _case("list37_bn")
    with DeviceStore(f, reserve_nodes=8) as store:
        assert store.info()["capacity"] == 8
        caps = []
        for a, b in _batches(len(nodes), CUTS):
            store.append(nodes[a:b])
            caps.append(store.info()["capacity"])
            assert np.array_equal(store.digests(np.arange(b)), want[:b]), "what was resident before the growth is resident after it"
        assert caps == sorted(caps) and len(set(caps)) >= 4 and caps[0] == 8, caps
        _check_whole(store, f, want, levels, hashed)


@pytest.mark.parametrize("f", [FQ, BN])
def test_group_widths_around_the_host_threshold_across_a_batch_boundary(hip, f):
    """The second append adds, per kind, a level of 6 nodes (the host hashes it) and a level of 7 (the device does).  Their children are
    atoms, device-hashed nodes and host-hashed nodes of the FIRST append and nodes earlier in the second one.  Every digest against pyref's
    Poseidon on the StoreHasher layouts (/root/reference/src/lem/store.rs:29-78) written out here."""
    first = [("atom", 3 + j, 1000 + j) for j in range(10)]                                   # ids 0 .. 9
    first += [("tuple2", 1, j, j + 1) for j in range(8)]                                      # ids 10 .. 17: a group of 8, device
    first += [("tuple3", 5, 0, 10, 9), ("tuple3", 5, 11, 1, 2)]                               # ids 18, 19: a group of 2, host
    first += [("comm", 424242, 12)]                                                           # id 20: level 2, host
    dev_old, host_old, atom_old = list(range(10, 18)), [18, 19, 20], list(range(10))
    second = [("atom", 7, 77), ("atom", 6, R.modulus(f) - 1)]                                 # ids 21, 22
    base = len(first)
    chain = 20  # each level hangs under the level before it: six of a kind, then seven of the same kind
    for ki, (kind, nchild) in enumerate((("tuple2", 2), ("tuple3", 3), ("tuple4", 4), ("compact", 3), ("comm", 1))):
        for width in (6, 7):
            ids = []
            for j in range(width):
                pool = [dev_old[(j + width) % 8], base + (j & 1), host_old[j % 3], atom_old[(3 * j) % 10]]
                kids = [chain] + (pool[ki:] + pool[:ki])[:nchild - 1]  # tuple2: device-hashed; tuple3: new atom, host-hashed; tuple4: host, atom, device; ...
                kids = kids[j % nchild:] + kids[:j % nchild]  # the chained child at every position
                second.append(("comm", 900 + j, kids[0]) if kind == "comm" else (kind, 1 + j % 5) + tuple(kids))
                ids.append(base + len(second) - 1)
            chain = ids[width // 2]
    nodes = first + second
    # the expectation: one Poseidon per node, on the layout of its kind
    tag = [8 if nd[0] == "comm" else nd[1] for nd in nodes]
    dig = []
    for nd in nodes:
        kind = nd[0]
        if kind == "atom":
            dig.append(nd[2])
        elif kind == "comm":
            dig.append(R.poseidon_hash(f, [nd[1], tag[nd[2]], dig[nd[2]]]))                   # secret, tag_a, h_a
        elif kind == "compact":
            a, b, c = nd[2:]
            dig.append(R.poseidon_hash(f, [dig[a], tag[b], dig[b], dig[c]]))                   # h_a, tag_b, h_b, h_c
        else:
            dig.append(R.poseidon_hash(f, [x for c in nd[2:] for x in (tag[c], dig[c])]))      # [tag, hash] per child
    want = C.ints_to_limbs(dig)
    with DeviceStore(f) as store:
        assert store.append(first) == 0
        assert store.info()["hashes_done"] == 11
        assert store.append(second) == base
        info = store.info()
        assert info["n_nodes"] == len(nodes) and info["hashes_done"] == 11 + 5 * 13 and info["levels"] == 2 + 10
        got = store.digests(np.arange(len(nodes)))
        bad = [i for i in range(len(nodes)) if not np.array_equal(got[i], want[i])]
        assert not bad, ("nodes with a wrong digest", bad, [nodes[i] for i in bad[:3]])


def test_refusals_leave_the_store_unchanged(hip):
    f, nodes, _, _, _ = _case("list37_bn")
    base = 200
    p = R.modulus(f)
    good = [("atom", 7, 5), ("atom", 6, p - 1), ("tuple2", 1, base, base + 1), ("comm", 99, base + 2), ("tuple3", 5, 17, base + 3, 3)]
    with DeviceStore(f, reserve_nodes=256) as store:
        store.append(nodes[:base])
        before_info, before = store.info(), store.digests(np.arange(base))

        def refused(match, edit, grow=0):
            rec, vals = SH.encode(good)
            if grow:  # pad with valid atoms so that the refused batch would have needed a growth
                rec = np.concatenate([rec, np.tile(rec[:1], (grow, 1))])
            edit(rec, vals)
            with pytest.raises(LurkHipError, match=match) as e:
                store.append_records(rec, vals)
            assert e.value.code == 2  # LURK_HIP_ERR_INVALID_ARG
            assert store.info() == before_info
            assert np.array_equal(store.digests(np.arange(base)), before)
            with pytest.raises(LurkHipError, match="id 0 is out of range"):
                store.digests([base])

        def set_(r, c, v):
            return lambda rec, vals: rec.__setitem__((r, c), v)

        topo = r"record 2: nodes must be in topological order \(children first\)"
        refused(topo, set_(2, 2, base + 2))                                                   # a child id equal to the node's own id
        refused(topo, set_(2, 3, base + 1000))                                                # a child id beyond the store
        refused(r"record 4: nodes must be in topological order", set_(4, 4, base + 5), grow=100)
        refused("record 1: unknown node kind", set_(1, 0, 9))
        refused("record 0: unknown node kind", set_(0, 0, 1))
        refused("record 3: commitment secret index out of range", set_(3, 6, 3))              # the call has three values
        refused("record 0: atom value index out of range", set_(0, 6, 1 << 31))
        refused("record 1: value 1 is not reduced modulo the field order", lambda rec, vals: vals.__setitem__(1, C.ints_to_limbs([p])[0]))
        refused("record 3: value 2 is not reduced", lambda rec, vals: vals.__setitem__(2, np.full(4, 2**64 - 1, dtype=np.uint64)))
        # of two offenders the first is named
        refused("record 1: unknown node kind", lambda rec, vals: (rec.__setitem__((1, 0), 7), rec.__setitem__((3, 2), base + 3)))
        # an empty append is accepted and changes nothing
        assert store.append([]) == base and store.info() == before_info
        # and then a valid append works: the whole against the oracle
        assert store.append(good) == base
        rec, vals = SH.encode(nodes[:base] + good)
        want, levels = C.store_hydrate(f, rec, vals)
        _check_whole(store, f, want, levels, int(np.count_nonzero(rec[:, 0])))
        with pytest.raises(LurkHipError, match="id 2 is out of range"):
            store.digests([0, base + 4, base + 5])
    store.close()  # closed by the with block already: a second close is a no-op
    with pytest.raises(LurkHipError, match="null store handle"):
        store.info()
    with pytest.raises(LurkHipError, match="unknown field id"):
        DeviceStore(3)
    with pytest.raises(LurkHipError, match="unknown field id"):
        DeviceStore(-1)


def test_digests_dev_shuffled_repeated_and_out_of_range(hip):
    import torch

    f, nodes, want, _, _ = _case("list37_bn")
    n = len(nodes)
    rng = np.random.default_rng(11)
    with DeviceStore(f) as store:
        store.append(nodes)
        for m in (1, 1000):
            ids = rng.integers(0, n, size=m, dtype=np.uint32)
            if m > 1:
                ids[5] = ids[6] = ids[700]  # repeated for sure
            got = store.digests_dev(torch.from_numpy(ids.view(np.int32)).cuda())
            torch.cuda.synchronize()
            assert np.array_equal(got.cpu().numpy().view(np.uint64), want[ids])
            # ids that are no nodes: their rows are zero, every other row stays correct
            ids_bad = ids.copy()
            holes = [0] if m == 1 else [3, 500, 999]
            ids_bad[holes] = [n, 0xFFFFFFFF, n + 12345][:len(holes)]
            exp = want[np.where(ids_bad < n, ids_bad, 0)].copy()
            exp[holes] = 0
            got = store.digests_dev(torch.from_numpy(ids_bad.view(np.int32)).cuda())
            torch.cuda.synchronize()
            assert np.array_equal(got.cpu().numpy().view(np.uint64), exp)
        assert store.digests_dev(np.zeros(0, dtype=np.uint32)).shape == (0, 4)


@pytest.mark.parametrize("f", [BN, FQ])
def test_slot_preimages_to_w(hip, f):
    """Two frames of (hash4 x 2, hash6, hash8, commitment, bit_decomp) slots over the nodes of a hydrated list: the preimages built on the
    device from descriptors == those built here from the oracle's digests, W assembled from them is bit-identical to W from the same
    preimages uploaded by the host, and the slot rows hold on it."""
    import torch

    nodes = SH.list_dag(37)
    rec, vals = SH.encode(nodes)
    want, _ = C.store_hydrate(f, rec, vals)
    dig, tag, n = C.limbs_to_ints(want), [int(t) for t in rec[:, 1]], len(nodes)
    counts = {"hash4": 2, "hash6": 1, "hash8": 1, "commitment": 1, "bit_decomp": 1}
    top, thunk, env = n - 1, n - 3, n - 2
    slots = {  # frame-major: frame 0's slots of the type, then frame 1's; one dummy slot per frame, one boolean, nums
        "hash4": [[("ptr", top), ("ptr", 40)], [("ptr", thunk), ("num", 7), ("bool", True)], None, [("ptr", 0), ("ptr", env)]],
        "hash6": [[("ptr", 11), ("ptr", 12), ("ptr", top)], [("ptr", 500), ("ptr", 3), ("ptr", 1000)]],
        "hash8": [None, [("ptr", 100), ("ptr", thunk), ("ptr", 9), ("ptr", 1)]],
        "commitment": [[("num", 1), ("ptr", env)], [("num", top), ("ptr", 2)]],
        "bit_decomp": [[("num", 1)], [("num", 640)]],
    }

    def expected(slot, arity):
        if slot is None:
            return [0] * arity
        out = []
        for kind, arg in slot:
            out += [tag[arg], dig[arg]] if kind == "ptr" else [dig[arg]] if kind == "num" else [1 if arg else 0]
        assert len(out) == arity
        return out

    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()
    mf = MultiFrameWitness(f, 2, 0, 0, slot_counts=counts)
    with DeviceStore(f) as store:
        store.append(nodes[:600])
        store.append(nodes[600:])
        pre_dev, pre_host = {}, {}
        for name, st in SLOT_ORDER:
            arity = 1 if name == "bit_decomp" else st
            exp = C.ints_to_limbs([x for s in slots[name] for x in expected(s, arity)])
            got = store.slot_preimages(name, slots[name], mont=False)
            assert got.shape == (2 * counts[name], arity, 4)
            assert np.array_equal(got.cpu().numpy().view(np.uint64).reshape(-1, 4), exp), name
            pre_dev[name] = store.slot_preimages(name, slots[name], mont=True)
            assert np.array_equal(pre_dev[name].cpu().numpy().view(np.uint64).reshape(-1, 4), C.to_mont(f, exp)), name
            pre_host[name] = dev(C.to_mont(f, exp))
        # ids that are no nodes and unknown kinds give zero, in both forms
        odd = np.array([[1, n], [2, n], [2, 0xFFFFFFFF], [9, 5], [3, 6]], dtype=np.uint32)  # TAG, DIGEST, DIGEST out of range; kind 9; CONST 6
        out, d_odd = torch.empty((5, 4), dtype=torch.int64, device="cuda"), dev(np.ascontiguousarray(odd).view(np.int64))
        for mont in (0, 1):
            _lib.check(hip.lurk_hip_store_slot_preimages_dev(store._h, _lib.ptr(d_odd), 5, mont, _lib.ptr(out), None))
            torch.cuda.synchronize()
            exp = C.ints_to_limbs([0, 0, 0, 0, 6])
            assert np.array_equal(out.cpu().numpy().view(np.uint64), C.to_mont(f, exp) if mont else exp)
        # W from the device-built preimages == W from the same preimages uploaded by the host, bit for bit
        nio = 2
        z_dev = torch.zeros((mf.w_len + 1 + nio, 4), dtype=torch.int64, device="cuda")
        z_host = torch.zeros_like(z_dev)
        mf.assemble(z_dev, pre_dev, mont=True)
        mf.assemble(z_host, pre_host, mont=True)
        torch.cuda.synchronize()
        assert torch.equal(z_dev, z_host)
        assert int((z_dev[:mf.w_len] != 0).any(dim=1).sum()) > mf.w_len // 2, "W was written"
        # and the slot rows hold on it: u = 1, E = 0
        z_dev[mf.w_len:] = dev(C.to_mont(f, C.ints_to_limbs([1, 12345, 678])))
        sh = mf.r1cs(nio)
        try:
            assert sh.is_sat(z_dev) == (0, sh.num_cons)
        finally:
            sh.close()
