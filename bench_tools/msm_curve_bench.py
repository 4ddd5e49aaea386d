#!/usr/bin/env python3
"""Pallas, BN254 G1 and Grumpkin commitments side by side: one process, one device, the curves alternating inside every repetition.

Configurations: 2^20 synchronous, 2^20 with two in flight, 2^22 with four in flight (window-table keys, uniform scalars in Montgomery
form, resident in HBM).  Method of the msm workload: five warm-up commitments, then the median of five 20-commitment regions
(synchronize, 20 commitments, synchronize).  Every result of every region is compared with the discrete-log checksum
[sum s_i k_i] G computed in Python integers (tests/bn254_ref.py; Pallas through oracle/pyref.py's curve).  Prints one JSON line.

    python bench_tools/msm_curve_bench.py [--steps 20] [--regions 5] [--warmup 5]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

# bench_tools/issue_model.py over the accumulate kernel's loop (hipcc -O3 -S --cuda-device-only; the BN254 units with the rare doubling
# branch out of line, so that the census is the hot path's): 8 716 issue cycles per wave and mixed addition on the Pasta fields,
# 10 207 on the BN254 fields, on 1024 SIMDs at 2.15 GHz (profiles/r07_acc_issue_model_bn254.txt)
MODEL_G_MADD_PER_S = {"Pallas": 16.17, "BN254": 13.80, "Grumpkin": 13.80}
PROFILED = 5

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import torch

    import lurk_beta_amd as L
    from lurk_beta_amd import _lib, synth
    from oracle import pyref as R
    from tests import bn254_ref as B

    pallas = B.Curve(0, "Pallas", R.PALLAS_P, 5, R.PALLAS_Q, (R.PALLAS_P - 1, 2), 1, 0)
    curves = [pallas, B.BN254, B.GRUMPKIN]
    configs = [("2^20 sync", 20, 1), ("2^20, 2 in flight", 20, 2), ("2^22, 4 in flight", 22, 4)]
    out = {"tool": "msm_curve_bench", "device": torch.cuda.get_device_name(0), "steps": args.steps, "regions": args.regions, "warmup": args.warmup,
           "results": {}}
    for label, log_n, depth in configs:
        n = 1 << log_n
        state = {}
        for c in curves:
            bases = synth.bases(c.id, n)
            key = L.CommitmentKey(c.id, bases, n=n, device=True, precompute=True)
            vecs = [synth.scalars(c.scalar_field, 20 + k, 0, n, mont=True) for k in range(depth)]
            want = []
            for k in range(depth):
                canon = synth.scalars(c.scalar_field, 20 + k, 0, n).cpu().numpy().view(np.uint64)
                want.append(B.dlog_checksum_np(c, canon))
            key.reserve(n, depth)
            state[c.name] = (key, vecs, want, bases)
        torch.cuda.synchronize()

        def region(c, steps):
            key, vecs, want, _ = state[c.name]
            got = []
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if depth == 1:
                for _ in range(steps):
                    got.append((0, key.commit_device(vecs[0], n, is_mont=True)))
            else:
                for i in range(steps + depth):
                    k = i % depth
                    if i >= depth:
                        got.append((k, key.wait(k)))
                    if i < steps:
                        key.submit_device(k, vecs[k], n, is_mont=True)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            for k, pt in got:
                assert B.from_xy(L.point_to_affine(c.id, pt)) == want[k], (c.name, label, "result differs from the dlog checksum")
            return dt * 1e3 / steps

        for c in curves:
            region(c, args.warmup)
        times = {c.name: [] for c in curves}
        for _ in range(args.regions):
            for c in curves:  # alternating: every curve sees the same thermal and clock state
                times[c.name].append(region(c, args.steps))
        res = {}
        for c in curves:
            med = statistics.median(times[c.name])
            res[c.name] = {"ms_per_commit": round(med, 4), "Mscalar_mul_per_s": round(n / med / 1e3, 1), "by_region": [round(x, 4) for x in times[c.name]],
                           "verified": True}
        for c in curves[1:]:
            res[c.name]["ratio_to_pallas"] = round(res[c.name]["ms_per_commit"] / res["Pallas"]["ms_per_commit"], 3)
        if depth == 1:
            # per-kernel times of synchronous commitments (the library's profiler: HIP events on the launch stream, nothing else on the
            # device), and the accumulation against the issue model's bound for its loop (bench_tools/issue_model.py)
            lib = _lib.load()
            for c in curves:
                key, vecs, _, _ = state[c.name]
                _lib.check(lib.lurk_hip_profile_reset())
                _lib.check(lib.lurk_hip_profile_enable(1))
                for _ in range(PROFILED):
                    key.commit_device(vecs[0], n, is_mont=True)
                torch.cuda.synchronize()
                _lib.check(lib.lurk_hip_profile_enable(0))
                ks = {}
                for prefix in ("msm_sort", "msm_tasks", "msm_accumulate", "msm_finalize", "msm_reduce"):
                    tot, cnt = ctypes.c_double(), ctypes.c_uint64()
                    _lib.check(lib.lurk_hip_profile_get(prefix.encode(), ctypes.byref(tot), ctypes.byref(cnt)))
                    ks[prefix] = round(tot.value / PROFILED, 4)
                madds = key.info()["window_bits"] and ((256 + key.info()["window_bits"] - 1) // key.info()["window_bits"]) * n
                bound = MODEL_G_MADD_PER_S[c.name]
                res[c.name]["kernel_ms_sync"] = ks
                res[c.name]["accumulate"] = {"mixed_additions": madds, "achieved_G_madd_per_s": round(madds / ks["msm_accumulate"] / 1e6, 3),
                                             "issue_model_bound_G_madd_per_s": bound,
                                             "frac_of_bound": round(madds / ks["msm_accumulate"] / 1e6 / bound, 4)}
        out["results"][label] = res
        for key, _, _, _ in state.values():
            key.close()
        state.clear()
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
