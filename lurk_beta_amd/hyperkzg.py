"""Host-side mirror of the HyperKZG opening argument over BN254 G1 (include/lurk_hip.h, "HyperKZG"): EE1 of lurk-beta's default engine
Bn256EngineKZG (/root/reference/src/proof/nova.rs:65-71).  The polynomial and the commitment key stay in HBM; the transcript is a
callback; ``verify`` decides a proof against a verifier key [tau]H by the library's pairing check, ``pairing_inputs`` stops before the
pairing and returns its two G1 inputs.  The protocol is this repository's own statement of the published scheme, not arecibo's byte for
byte.  Also here: the three polynomial primitives the
argument is made of, and the powers-of-tau key tests and benchmarks prove under."""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib

CURVE_BN254 = 2
FIELD_BN254_FR = 2
BN254_R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
ACCEPTED, MALFORMED, FOLD, PAIRING = 0, 1, 2, 3  # LURK_HYPERKZG_*


def _limbs(v: int) -> np.ndarray:
    return np.array([(v >> (64 * w)) & 0xFFFFFFFFFFFFFFFF for w in range(4)], dtype=np.uint64)


def _ints(a) -> list[int]:
    a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4)
    return [int(r[0]) | int(r[1]) << 64 | int(r[2]) << 128 | int(r[3]) << 192 for r in a]


def _scalars(vals) -> np.ndarray:
    vals = [int(v) for v in vals]
    if any(v < 0 or v >> 256 for v in vals):
        raise ValueError("a scalar does not fit 32 bytes")
    return np.stack([_limbs(v) for v in vals]) if vals else np.zeros((1, 4), dtype=np.uint64)


def _stream(stream):
    import torch

    return stream if stream is not None else torch.cuda.current_stream().cuda_stream


def fold_pairs(field_id: int, d_in, x_mont: np.ndarray, stream=None):
    """out[j] = in[2j] + x (in[2j+1] - in[2j]): a new (ceil(len / 2), 4) device tensor (lurk_hip_mle_fold_pairs_dev)."""
    import torch

    n = d_in.shape[0]
    out = torch.empty(((n + 1) // 2, 4), dtype=torch.int64, device=d_in.device)
    x = np.ascontiguousarray(x_mont, dtype=np.uint64)
    _lib.check(_lib.load().lurk_hip_mle_fold_pairs_dev(field_id, _lib.ptr(d_in), n, _lib.ptr(x), _lib.ptr(out), _lib.ptr(_stream(stream))))
    return out


def poly_eval(field_id: int, d_coeffs, points_mont: np.ndarray, stream=None) -> np.ndarray:
    """The polynomial (coefficients low to high, Montgomery, on the device) at 1..4 points: (k, 4) Montgomery values (lurk_hip_poly_eval_dev)."""
    pts = np.ascontiguousarray(points_mont, dtype=np.uint64).reshape(-1, 4)
    out = np.zeros_like(pts)
    _lib.check(_lib.load().lurk_hip_poly_eval_dev(field_id, _lib.ptr(d_coeffs), d_coeffs.shape[0], _lib.ptr(pts), pts.shape[0], _lib.ptr(out), _lib.ptr(_stream(stream))))
    return out


def poly_div_linear(field_id: int, d_coeffs, roots_mont: np.ndarray, stream=None):
    """Division by (X - u_k) for 1..3 roots in one pass: ([quotient_k: (len - 1, 4) device tensor], remainders (k, 4) Montgomery)
    (lurk_hip_poly_div_linear_dev)."""
    import torch

    roots = np.ascontiguousarray(roots_mont, dtype=np.uint64).reshape(-1, 4)
    n, k = d_coeffs.shape[0], roots.shape[0]
    quot = [torch.empty((max(n - 1, 1), 4), dtype=torch.int64, device=d_coeffs.device) for _ in range(k)]
    ptrs = (ctypes.c_void_p * k)(*[q.data_ptr() for q in quot])
    rem = np.zeros_like(roots)
    _lib.check(_lib.load().lurk_hip_poly_div_linear_dev(field_id, _lib.ptr(d_coeffs), n, _lib.ptr(roots), k, ptrs, _lib.ptr(rem), _lib.ptr(_stream(stream))))
    return [q[:n - 1] for q in quot], rem


def kzg_bases(tau: int, n: int, first: int = 0, curve: int = CURVE_BN254, device="cuda"):
    """[tau^(first + i)]G for i < n as an (n, 8) device tensor of affine Montgomery points (lurk_hip_synth_kzg_bases_dev).  A trapdoor
    setup: for tests and benchmarks only."""
    import torch

    out = torch.empty((n, 8), dtype=torch.int64, device=device)
    t = _limbs(int(tau))
    _lib.check(_lib.load().lurk_hip_synth_kzg_bases_dev(curve, _lib.ptr(t), first, n, _lib.ptr(out), _lib.ptr(torch.cuda.current_stream().cuda_stream)))
    return out


def trapdoor_key(tau: int, n: int, precompute: bool = False, window_bits: int = 0, small_form=None):
    """A resident BN254 ``CommitmentKey`` over ck[i] = [tau^i]G, generated on the device.  INSECURE by construction (the caller knows
    tau): it makes a proof checkable without a pairing, L == [tau]R."""
    import torch

    from .msm import CommitmentKey

    bases = kzg_bases(tau, n)
    torch.cuda.synchronize()
    return CommitmentKey(CURVE_BN254, bases, n=n, precompute=precompute, device=True, window_bits=window_bits, small_form=small_form)


def prove(key, d_poly, x, challenge, stream=None) -> dict:
    """lurk_hip_hyperkzg_prove_dev.  key: a BN254 ``CommitmentKey``; d_poly: (2^ell, 4) Montgomery Fr values on the device (not
    modified); x: ell canonical integers (x[0] <-> the most significant index bit); challenge(stage, data) -> canonical integer, with
    data = an (ell - 1, 12) array of Jacobians (stage 0) or the 3 ell canonical integers of v, t-major (stage 1).
    Returns dict(com: (ell - 1, 12) u64, v: three lists of ell integers, w: (3, 12) u64, y: int)."""
    n = d_poly.shape[0]
    ell = max(n.bit_length() - 1, 1)
    x = [int(v) for v in x]
    R = (1 << 256) % BN254_R
    xm = _scalars([v % BN254_R * R % BN254_R for v in x]) if x else np.zeros((1, 4), dtype=np.uint64)
    com = np.zeros((max(ell - 1, 1), 12), dtype=np.uint64)
    v = np.zeros((3 * ell, 4), dtype=np.uint64)
    w = np.zeros((3, 12), dtype=np.uint64)
    y = np.zeros(4, dtype=np.uint64)
    failure = []

    def on_stage(_user, stage, data, count, out_ptr):
        try:
            if stage == 0:
                arr = np.ctypeslib.as_array(ctypes.cast(data, ctypes.POINTER(ctypes.c_uint64)), shape=(count, 12)).copy() if count else np.zeros((0, 12), dtype=np.uint64)
                c = challenge(0, arr)
            else:
                arr = np.ctypeslib.as_array(ctypes.cast(data, ctypes.POINTER(ctypes.c_uint64)), shape=(count, 4)).copy()
                c = challenge(stage, _ints(arr))
            if c is None:
                return 1
            ctypes.memmove(out_ptr, int(c).to_bytes(32, "little"), 32)
            return 0
        except BaseException as e:  # noqa: BLE001 - an exception must not unwind through the C frames
            failure.append(e)
            return 1

    cb = _lib.HYPERKZG_CHALLENGE_FN(on_stage)
    if len(x) != ell:
        raise ValueError("x must hold log2(n) values")
    rc = _lib.load().lurk_hip_hyperkzg_prove_dev(key._ctx, _lib.ptr(d_poly), n, _lib.ptr(xm), ctypes.cast(cb, ctypes.c_void_p), None, _lib.ptr(com), _lib.ptr(v),
                                                 _lib.ptr(w), _lib.ptr(y), _lib.ptr(_stream(stream)))
    if failure:
        raise failure[0]
    _lib.check(rc)
    vi = _ints(v)
    return {"com": com[:ell - 1].copy(), "v": [vi[t * ell:(t + 1) * ell] for t in range(3)], "w": w, "y": _ints(y)[0]}


def pairing_inputs(ell: int, c, x, y: int, com, v, w, r: int, q: int, d: int, curve: int = CURVE_BN254):
    """lurk_hip_hyperkzg_pairing_inputs (host only): the verifier up to the pairing.  c, com (ell - 1), w (3): 96-byte Jacobians as u64
    arrays; x (ell), y, v (three rows of ell), r, q, d: canonical integers.  Returns (L, R, accepted, failed_check) with L, R as
    (12,) u64 Jacobians: the proof is valid iff accepted and e(L, H) == e(R, [tau]H)."""
    cj, xs, ys, comj, vs, wj, rs, qs, ds = _verifier_args(ell, c, x, y, com, v, w, r, q, d)
    L, Rr = np.zeros(12, dtype=np.uint64), np.zeros(12, dtype=np.uint64)
    acc, failed = ctypes.c_int(0), ctypes.c_int(0)
    _lib.check(_lib.load().lurk_hip_hyperkzg_pairing_inputs(curve, ell, _lib.ptr(cj), _lib.ptr(xs), _lib.ptr(ys), _lib.ptr(comj), _lib.ptr(vs), _lib.ptr(wj), _lib.ptr(rs),
                                                            _lib.ptr(qs), _lib.ptr(ds), _lib.ptr(L), _lib.ptr(Rr), ctypes.byref(acc), ctypes.byref(failed)))
    return L, Rr, bool(acc.value), failed.value


def _verifier_args(ell: int, c, x, y: int, com, v, w, r: int, q: int, d: int):
    cj = np.ascontiguousarray(c, dtype=np.uint64).reshape(12)
    comj = np.ascontiguousarray(com, dtype=np.uint64).reshape(-1, 12) if ell > 1 else np.zeros((1, 12), dtype=np.uint64)
    wj = np.ascontiguousarray(w, dtype=np.uint64).reshape(3, 12)
    flat_v = [e for row in v for e in row]
    if len(x) != ell or len(flat_v) != 3 * ell or (ell > 1 and comj.shape[0] != ell - 1):
        raise ValueError("x, v and com must hold ell, 3 ell and ell - 1 entries")
    return cj, _scalars(x), _scalars([y]), comj, _scalars(flat_v), wj, _scalars([r]), _scalars([q]), _scalars([d])


def verify(ell: int, c, x, y: int, com, v, w, r: int, q: int, d: int, tau_h, curve: int = CURVE_BN254):
    """lurk_hip_hyperkzg_verify (host only): the verifier that DECIDES.  The arguments of ``pairing_inputs`` and the verifier key
    tau_h = [tau]H, a (16,) u64 G2 point (``pairing.g2_mul`` / ``trapdoor_vk``).  Returns (accepted, failed_check): accepted means the
    proof is valid; failed_check is PAIRING when only e(L, H) == e(R, tau_h) fails."""
    a = _verifier_args(ell, c, x, y, com, v, w, r, q, d)
    vk = np.ascontiguousarray(tau_h, dtype=np.uint64).reshape(16)
    acc, failed = ctypes.c_int(0), ctypes.c_int(0)
    _lib.check(_lib.load().lurk_hip_hyperkzg_verify(curve, ell, *[_lib.ptr(e) for e in a], _lib.ptr(vk), ctypes.byref(acc), ctypes.byref(failed)))
    return bool(acc.value), failed.value


def trapdoor_vk(tau: int) -> np.ndarray:
    """[tau]H: the verifier key that goes with ``trapdoor_key(tau, ...)``, a (16,) u64 G2 point."""
    from . import pairing

    return pairing.g2_mul(None, int(tau) % BN254_R)


def key_check(key, tau_h, seed: int, stream=None) -> bool:
    """lurk_hip_kzg_key_check_dev: is the resident BN254 ``CommitmentKey`` a powers-of-tau key for the verifier key tau_h?  Two
    commitments under the key with weights drawn from ``seed`` (choose it after the key exists) and one pairing check."""
    vk = np.ascontiguousarray(tau_h, dtype=np.uint64).reshape(16)
    out = ctypes.c_int(0)
    _lib.check(_lib.load().lurk_hip_kzg_key_check_dev(key._ctx, _lib.ptr(vk), int(seed), ctypes.byref(out), _lib.ptr(_stream(stream))))
    return bool(out.value)
