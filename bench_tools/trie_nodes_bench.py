#!/usr/bin/env python3
"""Root-addressed tries (lurk_hip_trie_nodes_*) on one device against the handle-based trie calls: BN254 Fr, height 85, a trie of 2^16
random keys.

  add_trie       every node of the built handle into a FRESH store (created outside the timed region, sized so that it does not grow):
                 time, nodes added, bytes resident
  prove_lookup   m = 2^16 keys (every other one present), root-addressed at the trie's root against lurk_hip_trie_prove_lookup_dev
  prove_insert   m = 2^16, with and without register_new, against lurk_hip_trie_prove_insert_dev.  With register_new the first call
                 stores the m * 85 new nodes (reported on its own, with the growth it causes); the repetitions find them present
  insert_chain   m = 2^12 from the trie's root against lurk_hip_trie_insert_chain_dev (paths, values and roots, no new handle); first call
                 and repetitions as above
  register       2^20 random preimages into a fresh store against lurk_hip_poseidon_batch_dev on the same preimages: the difference is
                 the cost of the insert

Method: HIP events on the null stream, the median of 30 after 3 warm-ups, three repetitions of every measurement in one process.
Checked: the root-addressed outputs equal the handle-based ones byte for byte.  Writes JSON (default profiles/r19_trie_nodes_bench.json)
and prints it as one line.

    python bench_tools/trie_nodes_bench.py [--out profiles/r19_trie_nodes_bench.json] [--reps 30]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
FIELD, HEIGHT, LOG_N = 2, 85, 16


def timed(fn, reps, warm=3, setup=None):
    """median of `reps` event-timed calls after `warm` warm-ups; setup() runs before every call, outside the events"""
    import torch

    ms = []
    for i in range(warm + reps):
        arg = setup() if setup else None
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(arg) if setup else fn()
        b.record()
        b.synchronize()
        if i >= warm:
            ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def once(fn):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_trie_nodes_bench.json"))
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    import torch

    from lurk_beta_amd import _lib
    from lurk_beta_amd.poseidon import _limbs
    from lurk_beta_amd.trie import DeviceTrie, DeviceTrieNodes, _dev
    from trie_bench import random_pairs

    torch.cuda.set_device(0)
    lib = _lib.load()
    n = 1 << LOG_N
    keys, values = random_pairs(n, LOG_N)
    res = {"device": torch.cuda.get_device_name(0), "field": "bn254_fr", "height": HEIGHT, "n": n, "reps": args.reps, "warmups": 3, "repetitions": 3}
    three = lambda f: [round(f(), 3) for _ in range(3)]
    with DeviceTrie.build_sorted(FIELD, _dev(keys), _dev(values), HEIGHT) as t:
        root = t.root
        # ---- add_trie
        live = []

        def fresh():
            while live:
                live.pop().close()
            live.append(DeviceTrieNodes.create(FIELD, HEIGHT, reserve_nodes=1 << 23))
            return live[0]

        res["add_trie_ms"] = three(lambda: timed(lambda ns: ns.add_trie(t), args.reps, setup=fresh))
        info = live[0].info()
        res["add_trie_nodes"] = info["n_nodes"] - HEIGHT
        res["store_slots"], res["store_bytes"] = info["slots"], info["slots"] * 296
        res["handle_bytes"] = 32 * n * (HEIGHT + 2)
        ns = live.pop()
        # ---- prove_lookup, m = 2^16
        m = 1 << 16
        qk, _ = random_pairs(m, 77)
        qk[0::2] = keys[np.random.default_rng(5).integers(0, n, size=m // 2)]
        dk, dv = _dev(qk), _dev(random_pairs(m, 78)[1])
        droot = _dev(_limbs([root]))
        paths = torch.empty((m, HEIGHT, 8, 4), dtype=torch.int64, device="cuda")
        vals = torch.empty((m, 4), dtype=torch.int64, device="cuda")
        status = torch.empty(m, dtype=torch.int32, device="cuda")
        P = _lib.ptr

        def look_nodes():
            _lib.check(lib.lurk_hip_trie_nodes_prove_lookup_dev(ns._h, P(droot), 0, P(dk), m, P(paths), P(vals), P(status), None, None))

        want = t.prove_lookup(dk)
        look_nodes()
        assert torch.equal(paths, want[0]) and torch.equal(vals, want[1]) and not status.any()

        def look_handle():
            _lib.check(lib.lurk_hip_trie_prove_lookup_dev(t._h, P(dk), m, P(paths), P(vals), None))

        res["prove_lookup_nodes_ms"] = three(lambda: timed(look_nodes, args.reps))
        res["prove_lookup_handle_ms"] = three(lambda: timed(look_handle, args.reps))
        res["prove_lookup_bytes_written"] = m * HEIGHT * 256
        del want
        # ---- prove_insert, m = 2^16
        new = torch.empty_like(paths)
        roots_out = torch.empty((m, 4), dtype=torch.int64, device="cuda")

        def ins_nodes(register):
            _lib.check(lib.lurk_hip_trie_nodes_prove_insert_dev(ns._h, P(droot), 0, P(dk), P(dv), m, P(paths), P(new), P(vals), P(roots_out), P(status), None,
                                                                register, None))

        def ins_handle():
            _lib.check(lib.lurk_hip_trie_prove_insert_dev(t._h, P(dk), P(dv), m, P(paths), P(new), P(vals), P(roots_out), None))

        ins_handle()
        want_new, want_roots = new.clone(), roots_out.clone()
        ins_nodes(0)
        assert torch.equal(new, want_new) and torch.equal(roots_out, want_roots)
        del want_new
        res["prove_insert_handle_ms"] = three(lambda: timed(ins_handle, args.reps))
        res["prove_insert_nodes_ms"] = three(lambda: timed(lambda: ins_nodes(0), args.reps))
        before = ns.info()
        res["prove_insert_register_first_ms"] = round(once(lambda: ins_nodes(1)), 3)
        after = ns.info()
        res["prove_insert_register_first_nodes"] = after["n_nodes"] - before["n_nodes"]
        res["prove_insert_register_first_slots"] = [before["slots"], after["slots"]]
        assert torch.equal(roots_out, want_roots)
        res["prove_insert_register_present_ms"] = three(lambda: timed(lambda: ins_nodes(1), args.reps))
        del new
        # ---- insert_chain, m = 2^12
        mc = 1 << 12
        ck, cv = dk[:mc].contiguous(), dv[:mc].contiguous()
        root32 = _limbs([root])
        o, nw = paths[:mc], torch.empty((mc, HEIGHT, 8, 4), dtype=torch.int64, device="cuda")
        ov, cr = torch.empty((mc, 4), dtype=torch.int64, device="cuda"), torch.empty((mc, 4), dtype=torch.int64, device="cuda")

        def chain_nodes():
            _lib.check(lib.lurk_hip_trie_nodes_insert_chain_dev(ns._h, P(root32), P(ck), P(cv), mc, P(o), P(nw), P(ov), P(cr), None))

        def chain_handle():
            _lib.check(lib.lurk_hip_trie_insert_chain_dev(t._h, P(ck), P(cv), mc, P(o), P(nw), P(ov), P(cr), None, None))

        chain_handle()
        want_chain = (nw.clone(), cr.clone())
        before = ns.info()
        res["insert_chain_nodes_first_ms"] = round(once(chain_nodes), 3)
        res["insert_chain_first_nodes"] = ns.info()["n_nodes"] - before["n_nodes"]
        assert torch.equal(nw, want_chain[0]) and torch.equal(cr, want_chain[1])
        res["insert_chain_nodes_present_ms"] = three(lambda: timed(chain_nodes, args.reps))
        res["insert_chain_handle_ms"] = three(lambda: timed(chain_handle, args.reps))
        ns.close()
    # ---- register, 2^20 random preimages
    count = 1 << 20
    pre = _dev(random_pairs(count * 8, 99)[1])
    dig = torch.empty((count, 4), dtype=torch.int64, device="cuda")
    live = []

    def fresh_small():
        while live:
            live.pop().close()
        live.append(DeviceTrieNodes.create(FIELD, HEIGHT, reserve_nodes=1 << 21))
        return live[0]

    def batch():
        _lib.check(lib.lurk_hip_poseidon_batch_dev(FIELD, 8, P(pre), count, P(dig), None))

    batch()
    want_dig = dig.clone()
    res["register_ms"] = three(lambda: timed(lambda s: _lib.check(lib.lurk_hip_trie_nodes_register_dev(s._h, P(pre), count, P(dig), None)), args.reps, setup=fresh_small))
    assert torch.equal(dig, want_dig) and live[0].info()["n_nodes"] == HEIGHT + count
    res["poseidon_batch_ms"] = three(lambda: timed(batch, args.reps))
    while live:
        live.pop().close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
