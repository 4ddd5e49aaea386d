#!/usr/bin/env python3
"""A 2^20-element HyperKZG opening on BN254 G1 (lurk_hip_hyperkzg_prove_dev) beside one synchronous 2^20 commitment: one process, one device.

Method of msm_curve_bench.py: warm-up proofs, then the median of five regions (synchronize, `steps` proofs, synchronize).  The key is the
powers-of-tau test key (a window-table key over [tau^i]G), so EVERY proof of every region is checked by the trapdoor identity: the
library's verifier up to the pairing gives L and R, and L == [tau]R in Python integers (tests/bn254_ref.py).  The transcript is a
SHA-256 over the raw bytes the callback receives (host time inside the proof, as a real transcript's is).  An opening commits about
n + 3 n scalars, so the figure of merit is prove_ms / (4 x commit_ms).  Per-stage times: wall clock between the callback's stages
(folds + commitments | evaluations | B + division + W) and the kernels' own times from the library profiler.  Prints one JSON line.

    python bench_tools/hyperkzg_bench.py [--log-n 20] [--steps 3] [--regions 5] [--warmup 2]
"""
import argparse
import ctypes
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import torch

    import lurk_beta_amd as L
    from lurk_beta_amd import _lib, hyperkzg, synth
    from tests import bn254_ref as B

    q = B.BN254_R
    tau = TAU % q
    ell, n = args.log_n, 1 << args.log_n
    key = hyperkzg.trapdoor_key(tau, n, precompute=True)
    key.reserve(n, 6)
    d_poly = synth.scalars(B.FIELD_BN254_FR, 31, 0, n, mont=True)
    x = [int.from_bytes(hashlib.sha256(b"x%d" % i).digest(), "little") % q for i in range(ell)]
    torch.cuda.synchronize()
    c = key.commit_device(d_poly, n, is_mont=True)

    class Transcript:
        def __init__(self):
            self.h = hashlib.sha256(b"hyperkzg-bench")
            self.out, self.t = {}, {}

        def __call__(self, stage, data):
            self.t[stage] = time.perf_counter()
            self.h.update(bytes([stage]) + (np.ascontiguousarray(data).tobytes() if stage == 0 else b"".join(int(e).to_bytes(32, "little") for e in data)))
            v = int.from_bytes(self.h.digest(), "little") % q
            self.out[stage] = v or 1
            return self.out[stage]

    def one():
        tr = Transcript()
        t0 = time.perf_counter()
        pf = hyperkzg.prove(key, d_poly, x, tr)
        t1 = time.perf_counter()
        return pf, tr, (tr.t[0] - t0, tr.t[1] - tr.t[0], t1 - tr.t[1])

    def check(pf, tr):
        d = tr(2, [int(v) for v in pf["w"].reshape(-1)])
        Lp, Rp, ok, code = hyperkzg.pairing_inputs(ell, c, x, pf["y"], pf["com"], pf["v"], pf["w"], tr.out[0], tr.out[1], d)
        assert ok and code == 0, "the verifier's scalar checks reject the proof"
        la, ra = B.from_xy(L.point_to_affine(B.CURVE_BN254, Lp)), B.from_xy(L.point_to_affine(B.CURVE_BN254, Rp))
        assert ra is not None and la == B.BN254.mul(tau, ra), "the proof fails the trapdoor identity L == [tau] R"

    def region(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = [one() for _ in range(steps)]
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e3 / steps
        for pf, tr, _ in got:
            check(pf, tr)
        return dt, [statistics.median(g[2][k] for g in got) * 1e3 for k in range(3)]

    def commit_region(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            key.commit_device(d_poly, n, is_mont=True)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    region(args.warmup)
    commit_region(5)
    prove_ms, commit_ms, stages = [], [], []
    for _ in range(args.regions):  # alternating: both see the same thermal and clock state
        dt, st = region(args.steps)
        prove_ms.append(dt)
        stages.append(st)
        commit_ms.append(commit_region(10))
    lib = _lib.load()
    _lib.check(lib.lurk_hip_profile_reset())
    _lib.check(lib.lurk_hip_profile_enable(1))
    pf, tr, _ = one()
    torch.cuda.synchronize()
    _lib.check(lib.lurk_hip_profile_enable(0))
    check(pf, tr)
    kernels = {}
    for prefix in ("hkzg_fold", "hkzg_eval", "hkzg_batch", "hkzg_div", "msm"):
        tot, cnt = ctypes.c_double(), ctypes.c_uint64()
        _lib.check(lib.lurk_hip_profile_get(prefix.encode(), ctypes.byref(tot), ctypes.byref(cnt)))
        kernels[prefix] = {"ms": round(tot.value, 4), "launches": int(cnt.value)}
    p_med, c_med = statistics.median(prove_ms), statistics.median(commit_ms)
    out = {"tool": "hyperkzg_bench", "device": torch.cuda.get_device_name(0), "log_n": ell, "steps": args.steps, "regions": args.regions, "warmup": args.warmup,
           "key_form": key.info()["form"], "prove_ms": round(p_med, 3), "prove_ms_by_region": [round(v, 3) for v in prove_ms],
           "commit_ms": round(c_med, 4), "commit_ms_by_region": [round(v, 4) for v in commit_ms], "prove_over_4_commits": round(p_med / (4 * c_med), 3),
           "wall_ms_by_stage": {k: round(statistics.median(s[i] for s in stages), 3) for i, k in enumerate(("folds_and_commitments", "evaluations", "batch_division_and_W"))},
           "kernel_ms_one_profiled_proof": kernels, "verified": "every proof: scalar checks and L == [tau] R"}
    print(json.dumps(out))
    key.close()


if __name__ == "__main__":
    main()
