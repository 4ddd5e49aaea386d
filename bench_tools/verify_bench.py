#!/usr/bin/env python3
"""Times the library verifier beside the library prover and the CPU oracle verifier on the compress workload's instance:
    python bench_tools/verify_bench.py [--log-n 20] [--reps 20] [--warmup 3] [--no-oracle]
One process, one box: a satisfied 2^log_n x 2^log_n product instance (oracle/spartan_fast.py: synth_product_instance, six public inputs,
as bench_workloads/compress.py), one resident window-table key.  Reported: the median wall time of --reps calls after --warmup of
  (a) lurk_hip_spartan_prove_dev,
  (b) lurk_hip_spartan_verify_dev under the same key,
  (c) the parts of (b) through the library profiler (eq_evals, sparse_mle, ipa_s_vector, the commitment's msm_* kernels) in a run of its
      own, host tail = wall - kernels,
  (d) oracle/spartan_fast.py: verify on the CPU (OpenMP threads as OMP_NUM_THREADS says; three calls, median),
  (e) on BN254 G1, for an instance of the same size under a powers-of-tau test key (row i < n/2: w_i * u = w_{n/2 + i}, as
      bench_tools/spartan_kzg_bench.py): lurk_hip_spartan_kzg_verify_dev, which stops before the pairing, and
  (f) lurk_hip_spartan_kzg_verify_pairing_dev, the pairing-complete verifier, on the same proof - accepted under [tau]H and rejected
      with LURK_VERIFY_PAIRING under [tau + 1]H before anything is timed.
The sparse evaluation's HBM fraction is of COMPULSORY bytes (8 B per non-zero, the row pointers, both eq tables once) over 8 TB/s: not
gather traffic."""
import argparse
import ctypes
import gc
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import lurk_beta_amd as L
from lurk_beta_amd import _lib
from lurk_beta_amd.spartan import SpartanProver, SpartanVerifier
from oracle import coracle as C
from oracle import spartan_fast as SF

ap = argparse.ArgumentParser()
ap.add_argument("--log-n", type=int, default=20)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--no-oracle", action="store_true")
args = ap.parse_args()
lib = _lib.load()
c, sf = L.CURVE_PALLAS, L.FIELD_PALLAS_FQ
q = 0x40000000000000000000000000000000224698FC0994A8DD8C46EB2100000001
n = 1 << args.log_n
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()

A, Bm, Cm, W, X = SF.synth_product_instance(sf, n, n, 6, seed=11)
B = C.synth_bases(c, n + 1)
prover = SpartanProver(c, q, [(M[0], M[1], C.to_mont(sf, M[2])) for M in (A, Bm, Cm)], n, n, len(X))
verifier = SpartanVerifier.from_shape(prover.shape, c, q)
d_W, d_E, d_B = dev(C.to_mont(sf, W)), torch.zeros((n, 4), dtype=torch.int64, device="cuda"), dev(B)
key = L.CommitmentKey(c, d_B, n=n, device=True, precompute=True)
key.reserve(n, 2)
cw, ce = key.commit_device(d_W, n, is_mont=True), key.commit_device(d_E, n, is_mont=True)
torch.cuda.synchronize()
nnz = [int(M[0][-1]) for M in (A, Bm, Cm)]
print(f"instance: 2^{args.log_n} x 2^{args.log_n}, non-zeros A/B/C {nnz}, {len(X)} public inputs, table key of {n} points; "
      f"device {torch.cuda.get_device_name(0)}; OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', '(unset)')}")


def wall(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    gc.collect()
    gc.disable()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    gc.enable()
    return ts


def line(name, ts):
    s = sorted(ts)
    print(f"{name:44s} median {statistics.median(s):9.3f} ms   min {s[0]:9.3f}   max {s[-1]:9.3f}   ({len(s)} calls)")
    return statistics.median(s)


proof = prover.prove(X, 1, d_W, d_E, d_B, cw, ce, key=key, in_library=True)
assert verifier.verify(X, 1, cw, ce, proof, key, d_ck=d_B) and verifier.last_failed_check == 0
bad_x = [(X[0] + 1) % q] + X[1:]
assert not verifier.verify(bad_x, 1, cw, ce, proof, key, d_ck=d_B)

t_prove = line("(a) lurk_hip_spartan_prove_dev", wall(lambda: prover.prove(X, 1, d_W, d_E, d_B, cw, ce, key=key, in_library=True), args.reps, args.warmup))
t_verify = line("(b) lurk_hip_spartan_verify_dev", wall(lambda: verifier.verify(X, 1, cw, ce, proof, key, d_ck=d_B), args.reps, args.warmup))
print(f"    (b) / (a) = {t_verify / t_prove:.3f}")

# (c) the parts, in a run of their own (event pairs around every kernel)
lib.lurk_hip_profile_enable(1)
lib.lurk_hip_profile_reset()
ts = wall(lambda: verifier.verify(X, 1, cw, ce, proof, key, d_ck=d_B), args.reps, 0)
lib.lurk_hip_profile_enable(0)
t_prof = line("(c) verify with the profiler on", ts)
kern = 0.0
for name in ("eq_evals", "sparse_mle", "ipa_s_vector", "msm_"):
    tot, cnt = ctypes.c_double(), ctypes.c_uint64()
    _lib.check(lib.lurk_hip_profile_get(name.encode(), ctypes.byref(tot), ctypes.byref(cnt)))
    per = tot.value / args.reps
    kern += per
    extra = ""
    if name == "sparse_mle":
        comp = 8 * sum(nnz) + 3 * 4 * (n + 1) + 32 * (n + 2 * n)
        extra = f"   compulsory bytes {comp / 1e6:.1f} MB -> {comp / (per * 1e-3) / 8e12 * 100:.1f} % of 8 TB/s (compulsory-byte traffic, not gather traffic)"
    print(f"    {name + '*' if name.endswith('_') else name:20s} {per:8.3f} ms per verification, {cnt.value // args.reps} launch scopes{extra}")
print(f"    host tail = wall - kernels: {t_prof - kern:8.3f} ms")

if not args.no_oracle:
    aff = lambda J: SF._aff(c, np.ascontiguousarray(J, dtype=np.uint64))
    acw, ace = aff(cw), aff(ce)
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        assert SF.verify(c, (A, Bm, Cm), n, n, X, B, acw, ace, 1, proof)
        ts.append((time.perf_counter() - t0) * 1e3)
    t_or = line("(d) oracle/spartan_fast.py verify (CPU)", ts)
    print(f"    (d) / (b) = {t_or / t_verify:.1f}")
key.close()
prover.close()

# (e), (f): the BN254 cycle's verifier, up to the pairing and pairing-complete
from lurk_beta_amd import SpartanKzgProver, SpartanKzgVerifier, hyperkzg, synth  # noqa: E402

R_BN = hyperkzg.BN254_R
TAU = 0x2B0F3C4D5E6F708192A3B4C5D6E7F8091A2B3C4D5E6F708192A3B4C5D6E7F809 % R_BN
half = n // 2
kkey = hyperkzg.trapdoor_key(TAU, n, precompute=True)
kkey.reserve(n, 6)
ip = np.minimum(np.arange(n + 1, dtype=np.uint64), np.uint64(half))
one = np.tile(np.array([[((1 << 256) % R_BN >> (64 * w)) & 0xFFFFFFFFFFFFFFFF for w in range(4)]], dtype=np.uint64), (half, 1))
mats = ((ip, np.arange(half, dtype=np.uint64), one), (ip, np.full(half, n, dtype=np.uint64), one), (ip, np.arange(half, n, dtype=np.uint64), one))
free = synth.scalars(L.FIELD_BN254_FR, 31, 0, half, mont=True)
k_W, k_E = torch.cat([free, free]).contiguous(), torch.zeros((n, 4), dtype=torch.int64, device="cuda")
torch.cuda.synchronize()
kcw, kce = kkey.commit_device(k_W, n, is_mont=True), kkey.commit_device(k_E, n, is_mont=True)
kpr = SpartanKzgProver(mats, n, n, 2)
kver = SpartanKzgVerifier.from_shape(kpr.shape)
kproof = kpr.prove([5, 7], 1, k_W, k_E, kcw, kce, kkey)
vk, vk_other = hyperkzg.trapdoor_vk(TAU), hyperkzg.trapdoor_vk((TAU + 1) % R_BN)
assert kver.verify([5, 7], 1, kcw, kce, kproof)[0]
assert kver.verify_pairing([5, 7], 1, kcw, kce, kproof, vk) and kver.last_failed_check == 0
assert not kver.verify_pairing([5, 7], 1, kcw, kce, kproof, vk_other) and kver.last_failed_check == 6
t_upto = line("(e) lurk_hip_spartan_kzg_verify_dev (BN254)", wall(lambda: kver.verify([5, 7], 1, kcw, kce, kproof), args.reps, args.warmup))
t_pair = line("(f) lurk_hip_spartan_kzg_verify_pairing_dev", wall(lambda: kver.verify_pairing([5, 7], 1, kcw, kce, kproof, vk), args.reps, args.warmup))
print(f"    (f) - (e) = {t_pair - t_upto:.3f} ms for the pairing check and the subgroup test of [tau]H;   (f) / (b) = {t_pair / t_verify:.3f}")
kpr.close()
kkey.close()
