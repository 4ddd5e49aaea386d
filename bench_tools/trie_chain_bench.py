#!/usr/bin/env python3
"""Chains of dependent inserts on the device-resident trie (lurk_hip_trie_insert_chain_dev) on one device: BN254 Fr, height 85, a base
trie of 2^16 random keys.

  chains    m = 2^8, 2^12, 2^16 updates with random keys (every other one a key of the base trie, the rest fresh) and m = 2^12 updates
            of ONE key: old paths, new paths, old values and roots (the whole call: its read-back of keys and values, its allocations,
            its orders and its synchronisation included), and the same call with the new trie as well
  floor     lurk_hip_trie_prove_insert_dev for the same m keys and values: the same m * 85 hashes with nothing chained, one launch
  baseline  the 2^12 random-key chain by sequential inserts on ONE host core through lurk_hip_poseidon_hash_host, into an empty trie,
            measured the way bench_tools/trie_bench.py measures it (its own function); the device chain over an empty trie must end in
            the same root

Method: HIP events on the null stream, the median of five after one warm-up.  Checked in every step: all m insert proofs of the chain
pass lurk_hip_trie_verify_insert_dev against the roots [root(t), roots[:-1]] -> roots (n_failed == 0), and the new trie's root is
roots[-1].  Every step runs in a process of its own under a time limit; after a step that fails or runs out of time nothing further is
started and the result says where it stopped.  Writes JSON (default profiles/r11_trie_chain_bench.json) and prints it as one line.

    python bench_tools/trie_chain_bench.py [--out profiles/r11_trie_chain_bench.json] [--skip-baseline]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
FIELD, HEIGHT, LOG_BASE = 2, 85, 16
STEPS = [("random_2^8", 120), ("random_2^12", 120), ("random_2^16", 240), ("single_key_2^12", 120), ("host_baseline_2^12", 400)]


def chain_updates(step, base_keys):
    from trie_bench import random_pairs

    if step == "single_key_2^12":
        m = 1 << 12
        keys = np.repeat(base_keys[12345:12346], m, axis=0)
    else:
        m = 1 << int(step.split("^")[1])
        keys, _ = random_pairs(m, 1000 + m)
        rng = np.random.default_rng(m)
        rng.shuffle(keys)  # random_pairs sorts
        if not step.startswith("host"):
            keys[0::2] = base_keys[rng.integers(0, len(base_keys), size=(m + 1) // 2)]
    _, values = random_pairs(m, 2000 + m)
    return np.ascontiguousarray(keys), values


def run_step(step):
    import torch

    from lurk_beta_amd import _lib
    from lurk_beta_amd.trie import DeviceTrie, _dev, verify_insert_batch
    from trie_bench import host_sequential_root, random_pairs, timed

    torch.cuda.set_device(0)
    base_keys, base_values = random_pairs(1 << LOG_BASE, LOG_BASE)
    keys, values = chain_updates(step, base_keys)
    m = len(keys)
    dk, dv = _dev(keys), _dev(values)
    if step.startswith("host"):
        root, secs = host_sequential_root(_lib.load(), keys, values)
        with DeviceTrie.build(FIELD, [], HEIGHT) as empty:
            _, _, _, roots, grown = empty.insert_chain(dk, dv, paths=False)
            assert grown.root == root, "the device chain over an empty trie does not end in the host inserts' root"
            grown.close()
        return {"device": torch.cuda.get_device_name(0), "n": m, "seconds": round(secs, 3), "us_per_insert": round(secs / m * 1e6, 1), "root_matches_device_chain": True}
    out = {}
    with DeviceTrie.build_sorted(FIELD, _dev(base_keys), _dev(base_values), HEIGHT) as t:

        def chain():
            out["c"] = t.insert_chain(dk, dv, trie=False)

        def chain_and_trie():
            if "t" in out:
                out["t"][4].close()
            out["t"] = t.insert_chain(dk, dv)

        def floor():
            out["f"] = t.prove_insert(dk, dv)

        def roots_only():
            out["r"] = t.insert_chain(dk, dv, paths=False, trie=False)

        f_med, f_all = timed(floor)
        del out["f"]
        r_med, r_all = timed(roots_only)
        c_med, c_all = timed(chain)
        old, new, old_values, roots, _ = out["c"]
        assert torch.equal(out["r"][3], roots)
        old_roots = torch.cat([t._root_dev(), roots[:-1]])
        codes, failed = verify_insert_batch(FIELD, HEIGHT, old_roots, roots, dk, old_values, dv, old, new)
        assert failed == 0 and not codes.any(), "the verify kernel rejects the chain's own proofs"
        last_root = roots[-1:].clone()
        del out["c"], old, new, codes
        t_med, t_all = timed(chain_and_trie)
        grown = out["t"][4]
        assert torch.equal(grown._root_dev(), last_root) and torch.equal(out["t"][3][-1:], last_root)
        n_new = grown.n
        grown.close()
    r3 = lambda xs: [round(x, 3) for x in xs]
    return {"device": torch.cuda.get_device_name(0), "updates": m, "base_keys": 1 << LOG_BASE, "chain_ms": round(c_med, 3), "chain_all_ms": r3(c_all), "chain_with_new_trie_ms": round(t_med, 3),
            "chain_with_new_trie_all_ms": r3(t_all), "chain_roots_only_ms": round(r_med, 3), "chain_roots_only_all_ms": r3(r_all),
            "prove_insert_floor_ms": round(f_med, 3), "prove_insert_floor_all_ms": r3(f_all), "ratio_to_floor": round(c_med / f_med, 2),
            "us_per_update": round(c_med / m * 1e3, 3), "hashes_per_s": round(m * HEIGHT / c_med * 1e3), "new_trie_keys": n_new, "all_verified": True,
            "proof_bytes_per_update": 2 * HEIGHT * 256}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_trie_chain_bench.json"))
    ap.add_argument("--skip-baseline", action="store_true")
    ap.add_argument("--step", help="internal: run one step in this process and write its result to --out")
    args = ap.parse_args()
    if args.step:
        res = run_step(args.step)
        with open(args.out, "w") as f:
            json.dump(res, f)
        return
    res = {"field": "bn254_fr", "height": HEIGHT, "method": "HIP events, median of 5 after 1 warm-up; one process per step", "steps": {}}
    for step, limit in STEPS:
        if args.skip_baseline and step.startswith("host"):
            continue
        with tempfile.TemporaryDirectory() as tmp:
            piece = os.path.join(tmp, "step.json")
            try:
                rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--out", piece], timeout=limit).returncode
            except subprocess.TimeoutExpired:
                rc = "time limit of %d s" % limit
            if rc != 0:
                res["stopped_at"] = {"step": step, "why": rc}  # nothing further is started
                break
            res["steps"][step] = json.load(open(piece))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    sys.exit(1 if "stopped_at" in res else 0)


if __name__ == "__main__":
    main()
