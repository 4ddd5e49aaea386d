#!/usr/bin/env python3
"""The compressing SNARK on BN254 G1 at 2^20 x 2^20 (lurk_hip_spartan_kzg_prove_dev / _verify_dev / _verify_pairing_dev): proof ms, verify
ms up to the pairing and pairing-complete, the HyperKZG opening's share, the key check, and lurk_hip_fold_padded_dev beside the five-pass
sequence it replaces.  One process, one device.

Method of hyperkzg_bench.py: warm-up, then the median of `regions` regions (synchronize, `steps` calls, synchronize).  The instance is
synthetic and satisfied: row i < n/2 is  w_i * u = w_{n/2 + i}  with W = [free | free], u = 1, E = 0; the key is the powers-of-tau test
key, so EVERY proof is checked by the library's verifier up to the pairing with the trapdoor identity L == [tau]R (Python integers) AND by
the pairing-complete verifier against [tau]H (which must also reject it against the verifier key of tau + 1).  The pairing-complete
time is split by two host-only calls timed alone: the pairing check of the proof's own (L, H), (-R, [tau]H), and one 254-bit G2 multiple
(what the subgroup test of [tau]H costs at every call).  The key check (lurk_hip_kzg_key_check_dev) runs on the bench's own key.  The opening's share
is a stand-alone lurk_hip_hyperkzg_prove_dev of a vector of the same length under the same key (SHA-256 callback transcript), timed in
the same regions, over the proof time.  The fold: HIP events around `fold_iters` launches, rotating through `sets` buffer sets so that
no launch finds its inputs in the 256 MiB Infinity Cache; the five-pass sequence is what the Pasta tail runs (two clears, two
device copies, fold_vec); bytes = 32 (len_W + len_E + N) for the share of HBM.  Prints one JSON line.

    python bench_tools/spartan_kzg_bench.py [--log-n 20] [--steps 3] [--regions 5] [--warmup 2]
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TAU = 0x2B0F3C4D5E6F708192A3B4C5D6E7F8091A2B3C4D5E6F708192A3B4C5D6E7F809
HBM_PEAK = 8.0e12  # B/s, the figure DESIGN.md quotes shares of


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--fold-iters", type=int, default=30)
    ap.add_argument("--sets", type=int, default=6)
    args = ap.parse_args()
    import torch

    import lurk_beta_amd as L
    from lurk_beta_amd import SpartanKzgProver, SpartanKzgVerifier, fold_padded, fold_vec, hyperkzg, pairing, synth
    from tests import bn254_ref as B

    q = B.BN254_R
    tau = TAU % q
    ell, n = args.log_n, 1 << args.log_n
    half = n // 2
    key = hyperkzg.trapdoor_key(tau, n, precompute=True)
    key.reserve(n, 6)
    # ---- the instance
    ip = np.minimum(np.arange(n + 1, dtype=np.uint64), np.uint64(half))
    one = np.tile(B.to_mont(q, [1]), (half, 1))
    A = (ip, np.arange(half, dtype=np.uint64), one)
    Bm = (ip, np.full(half, n, dtype=np.uint64), one)  # column num_vars: u
    Cm = (ip, np.arange(half, n, dtype=np.uint64), one)
    free = synth.scalars(B.FIELD_BN254_FR, 31, 0, half, mont=True)
    d_W = torch.cat([free, free]).contiguous()
    d_E = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    X = [5, 7]
    torch.cuda.synchronize()
    cw, ce = key.commit_device(d_W, n, is_mont=True), key.commit_device(d_E, n, is_mont=True)
    pr = SpartanKzgProver((A, Bm, Cm), n, n, len(X))
    ver = SpartanKzgVerifier.from_shape(pr.shape)
    aff = lambda j: B.from_xy(L.point_to_affine(B.CURVE_BN254, j))

    vk, vk_other = hyperkzg.trapdoor_vk(tau), hyperkzg.trapdoor_vk((tau + 1) % q)

    def check(pf):
        ok, Lp, Rp = ver.verify(X, 1, cw, ce, pf)
        assert ok, f"the verifier rejects the proof at check {ver.last_failed_check}"
        la, ra = aff(Lp), aff(Rp)
        assert ra is not None and la == B.BN254.mul(tau, ra), "the proof fails the trapdoor identity L == [tau] R"
        assert ver.verify_pairing(X, 1, cw, ce, pf, vk), f"the pairing-complete verifier rejects the proof at check {ver.last_failed_check}"
        assert not ver.verify_pairing(X, 1, cw, ce, pf, vk_other) and ver.last_failed_check == 6, "the proof passes under another verifier key"
        return Lp, Rp

    def region(fn, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = [fn() for _ in range(steps)]
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps, got

    prove = lambda: pr.prove(X, 1, d_W, d_E, cw, ce, key)
    x = [int.from_bytes(hashlib.sha256(b"x%d" % i).digest(), "little") % q for i in range(ell)]

    def opening():
        h = hashlib.sha256(b"spartan-kzg-bench")

        def tr(stage, data):
            h.update(bytes([stage]) + (np.ascontiguousarray(data).tobytes() if stage == 0 else b"".join(int(e).to_bytes(32, "little") for e in data)))
            return int.from_bytes(h.digest(), "little") % q or 1

        return hyperkzg.prove(key, d_W, x, tr)

    _, got = region(prove, args.warmup)
    pf0 = got[-1]
    L0, R0 = check(pf0)
    region(opening, 1)
    prove_ms, verify_ms, open_ms, pairing_ms, pair_alone_ms, g2_mul_ms, key_check_ms = [], [], [], [], [], [], []
    neg_r0 = R0.copy()  # -R: y -> p - y on the normalised Jacobian
    neg_r0[4:8] = B.to_mont(B.BN254_P, [(B.BN254_P - aff(R0)[1]) % B.BN254_P])[0]
    pair_g1, pair_g2 = np.stack([L0, neg_r0]), np.stack([pairing.g2_generator(), vk])
    assert pairing.pairing_check(pair_g1, pair_g2)
    assert hyperkzg.key_check(key, vk, 1) and not hyperkzg.key_check(key, vk_other, 1)
    for _ in range(args.regions):  # alternating: all three see the same thermal and clock state
        dt, got = region(prove, args.steps)
        prove_ms.append(dt)
        for pf in got:
            check(pf)
        verify_ms.append(region(lambda: ver.verify(X, 1, cw, ce, pf0), args.steps)[0])
        pairing_ms.append(region(lambda: ver.verify_pairing(X, 1, cw, ce, pf0, vk), args.steps)[0])
        pair_alone_ms.append(region(lambda: pairing.pairing_check(pair_g1, pair_g2), args.steps)[0])
        g2_mul_ms.append(region(lambda: pairing.g2_mul(vk, q - 1), args.steps)[0])
        key_check_ms.append(region(lambda: hyperkzg.key_check(key, vk, 2), args.steps)[0])
        open_ms.append(region(opening, args.steps)[0])
    # ---- the fold kernel against the five passes
    f = B.FIELD_BN254_FR
    gamma = B.to_mont(q, [0x1234567890ABCDEF1234567890ABCDEF, 1])
    coeffs = np.stack([B.to_mont(q, [1])[0], gamma[0]])
    sets = [(synth.scalars(f, 40 + 2 * k, 0, n, mont=True), synth.scalars(f, 41 + 2 * k, 0, n, mont=True), torch.empty((n, 4), dtype=torch.int64, device="cuda"))
            for k in range(args.sets)]
    p1 = [torch.empty((n, 4), dtype=torch.int64, device="cuda") for _ in range(args.sets)]
    p2 = [torch.empty((n, 4), dtype=torch.int64, device="cuda") for _ in range(args.sets)]

    def one_pass(k):
        w, e, o = sets[k % args.sets]
        fold_padded(f, [w, e], coeffs, n, out=o)

    def five_pass(k):
        w, e, o = sets[k % args.sets]
        a, b = p1[k % args.sets], p2[k % args.sets]
        a.zero_()
        b.zero_()
        a.copy_(w)
        b.copy_(e)
        fold_vec(f, a, b, gamma[:1], out=o)

    def events(fn):
        for k in range(args.sets):
            fn(k)
        torch.cuda.synchronize()
        times = []
        for k in range(args.fold_iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(k)
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        return statistics.median(times)

    five_ms, one_ms = events(five_pass), events(one_pass)
    w, e, o = sets[0]
    a, b = p1[0], p2[0]
    fold_padded(f, [w, e], coeffs, n, out=o)
    a.zero_(), b.zero_(), a.copy_(w), b.copy_(e)
    assert torch.equal(o, fold_vec(f, a, b, gamma[:1])), "fold_padded differs from the five-pass sequence"
    p_med, v_med, o_med = statistics.median(prove_ms), statistics.median(verify_ms), statistics.median(open_ms)
    out = {"tool": "spartan_kzg_bench", "device": torch.cuda.get_device_name(0), "log_n": ell, "steps": args.steps, "regions": args.regions, "warmup": args.warmup,
           "key_form": key.info()["form"], "prove_ms": round(p_med, 3), "prove_ms_by_region": [round(v, 3) for v in prove_ms], "verify_ms": round(v_med, 3),
           "verify_ms_by_region": [round(v, 3) for v in verify_ms], "verify_pairing_ms": round(statistics.median(pairing_ms), 3),
           "verify_pairing_ms_by_region": [round(v, 3) for v in pairing_ms], "pairing_check_alone_ms": round(statistics.median(pair_alone_ms), 3),
           "g2_multiple_254_bits_ms": round(statistics.median(g2_mul_ms), 3), "key_check_ms": round(statistics.median(key_check_ms), 3),
           "key_check_ms_by_region": [round(v, 3) for v in key_check_ms], "opening_alone_ms": round(o_med, 3), "opening_share": round(o_med / p_med, 3),
           "fold_padded_ms": round(one_ms, 4), "five_pass_ms": round(five_ms, 4), "fold_padded_bytes": 96 * n,
           "fold_padded_share_of_8TBs": round(96 * n / (one_ms * 1e-3) / HBM_PEAK, 3), "fold_iters": args.fold_iters, "buffer_sets": args.sets,
           "verified": "every proof: the library's verifier and L == [tau] R, the pairing-complete verifier under [tau]H and not under [tau + 1]H; the key check; "
                       "fold_padded == the five passes"}
    print(json.dumps(out))
    pr.close()
    key.close()


if __name__ == "__main__":
    main()
