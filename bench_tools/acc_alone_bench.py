#!/usr/bin/env python3
"""One persistent accumulation ALONE on the device against the plain launch: the rate of a single accumulate wave per SIMD.

The headline has at most two persistent launches resident and on average 1.6-1.7 (profiles/r05_notebook.md 5.5), so for a third of
the time a SIMD holds one accumulate wave with nothing to cover its loads.  This tool measures that state by itself: the 2^22-point
Pallas table key of the headline under LURK_MSM_ACC_PERSISTENT=2, one commitment submitted and awaited at a time (nothing else on
the device), the library profiler's `msm_accumulate_persistent` scope; beside it the plain launch (three waves per SIMD) from
synchronous commitments, scope `msm_accumulate`.  rate = plain ms / persistent-alone ms.  The results of both legs are compared with
each other.  Prints one JSON line.

    python bench_tools/acc_alone_bench.py [--log-n 22] [--reps 10] [--warmup 3]
"""
import argparse
import ctypes
import json
import os
import sys

os.environ["LURK_MSM_ACC_PERSISTENT"] = "2"   # read once, when the library first plans a commitment

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=22)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch

    import lurk_beta_amd as L
    from lurk_beta_amd import _lib, synth

    lib = _lib.load()
    n = 1 << args.log_n
    key = L.CommitmentKey(0, synth.bases(0, n), n=n, device=True, precompute=True)
    key.reserve(n, 2)
    vec = synth.scalars(1, 20, 0, n, mont=True)
    torch.cuda.synchronize()

    def scope(name, reps):
        tot, cnt = ctypes.c_double(), ctypes.c_uint64()
        _lib.check(lib.lurk_hip_profile_get(name.encode(), ctypes.byref(tot), ctypes.byref(cnt)))
        assert cnt.value == reps, (name, cnt.value, reps)   # one launch per commitment, and only this form
        return tot.value / cnt.value

    def leg(run, name):
        for _ in range(args.warmup):
            run()
        torch.cuda.synchronize()
        _lib.check(lib.lurk_hip_profile_reset())
        _lib.check(lib.lurk_hip_profile_enable(1))
        pts = [run() for _ in range(args.reps)]
        torch.cuda.synchronize()
        _lib.check(lib.lurk_hip_profile_enable(0))
        return scope(name, args.reps), pts

    def alone():
        key.submit_device(0, vec, n, is_mont=True)
        return key.wait(0)

    plain_ms, p_plain = leg(lambda: key.commit_device(vec, n, is_mont=True), "msm_accumulate")
    alone_ms, p_alone = leg(alone, "msm_accumulate_persistent")
    assert all(np.array_equal(p, p_plain[0]) for p in p_plain + p_alone), "the two forms disagree"
    info = key.info()
    key.close()
    print(json.dumps({"tool": "acc_alone_bench", "device": torch.cuda.get_device_name(0), "log_n": args.log_n, "window_bits": info["window_bits"],
                      "reps": args.reps, "warmup": args.warmup, "plain_ms": round(plain_ms, 4), "persistent_alone_ms": round(alone_ms, 4),
                      "rate_alone_vs_plain": round(plain_ms / alone_ms, 4), "verified": True}))


if __name__ == "__main__":
    main()
