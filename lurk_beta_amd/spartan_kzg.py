"""The compressing SNARK on BN254 G1 (lurk-beta's default cycle): the Spartan sum-checks of ``spartan.py`` opened by HyperKZG, as the
library runs them (include/lurk_hip.h: lurk_hip_spartan_kzg_prove_dev / _prove_batch_dev / _verify_dev / _verify_batch_dev).  Library
calls only: these classes marshal, nothing of the prover is restated in Python (tests/spartan_kzg_ref.py is the independent restatement
the tests compare with).  ``verify`` ends UP TO THE PAIRING and returns the two G1 inputs L, R of e(L, H) = e(R, [tau]H);
``verify_pairing`` takes the verifier key [tau]H and decides.

A proof is a dictionary: polys_outer, claims_outer, eval_E, polys_inner, eval_W, polys_batch, evals_batch as ``SpartanProver`` returns
them (batched: evals_E, evals_W), kzg_com (log2 N - 1 points), kzg_v (3 log2 N integers, t-major), kzg_w (3 points); points are affine
canonical (x, y) tuples, None for the identity."""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib, sumcheck
from .fold import R1CSShape
from .msm import point_to_affine
from .spartan import VERIFY_MALFORMED, _Malformed, _scalars, transpose_csr

CURVE_BN254, FIELD_BN254_FR = 2, 2
VERIFY_PAIRING = 6  # LURK_VERIFY_PAIRING
BN254_R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
BN254_P = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
LABEL = b"lurk-hip spartan v2bn254"
LABEL_BATCHED = LABEL + b"/batched"


def _aff(jac):
    xy = point_to_affine(CURVE_BN254, jac)
    return None if xy == (0, 0) else xy


def _jacobian(pt) -> np.ndarray:
    """(x, y) canonical / None / a 96-byte Jacobian -> Jacobian.  A point off the curve passes (the library rejects it); a coordinate that
    is not below the field order cannot be written in Montgomery form."""
    if pt is None:
        return np.zeros(12, dtype=np.uint64)
    if isinstance(pt, np.ndarray):
        if pt.size != 12:
            raise _Malformed
        return np.ascontiguousarray(pt, dtype=np.uint64).reshape(12)
    if len(pt) != 2 or any(int(c) < 0 or int(c) >= BN254_P for c in pt):
        raise _Malformed
    R = (1 << 256) % BN254_P
    return np.concatenate([sumcheck._limbs([int(pt[0]) * R % BN254_P, int(pt[1]) * R % BN254_P]).reshape(8), sumcheck._limbs([R])[0]])


def _points(pts, count: int) -> np.ndarray:
    pts = list(pts)
    if len(pts) != count:
        raise _Malformed
    out = np.zeros((max(count, 1), 12), dtype=np.uint64)
    for j, pt in enumerate(pts):
        out[j] = _jacobian(pt)
    return out


def _stream(stream):
    import torch

    return stream if stream is not None else torch.cuda.current_stream().cuda_stream


def _kzg_bufs(ell: int) -> dict:
    return dict(kzg_com=np.zeros((max(ell - 1, 1), 12), dtype=np.uint64), kzg_v=np.zeros((3 * ell, 4), dtype=np.uint64), kzg_w=np.zeros((3, 12), dtype=np.uint64))


def _kzg_out(bufs: dict, ell: int) -> dict:
    return dict(kzg_com=[_aff(bufs["kzg_com"][j]) for j in range(ell - 1)], kzg_v=sumcheck._ints(bufs["kzg_v"]), kzg_w=[_aff(bufs["kzg_w"][t]) for t in range(3)])


def _kzg_in(proof: dict, ell: int) -> dict:
    return dict(kzg_com=_points(proof["kzg_com"], ell - 1), kzg_v=_scalars(proof["kzg_v"], 3 * ell), kzg_w=_points(proof["kzg_w"], 3))


class SpartanKzgProver:
    """Keeps the shape and its transpose resident (as ``SpartanProver``).  mats: (A, B, C) as (indptr, indices, data Montgomery over Fr);
    num_cons and num_vars powers of two >= 2.  ``field_id`` is the field the shapes are created over (anything but Fr is refused by the
    library when a proof is asked for)."""

    def __init__(self, mats, num_cons: int, num_vars: int, num_io: int, field_id: int = FIELD_BN254_FR):
        self.curve, self.q, self.sf = CURVE_BN254, BN254_R, field_id
        self.num_cons, self.num_vars, self.num_io = num_cons, num_vars, num_io
        self.shape = R1CSShape(field_id, num_cons, num_vars, num_io, *mats)
        self.shape_t = R1CSShape(field_id, 2 * num_vars, num_cons - 1, 0, *[transpose_csr(*m, 2 * num_vars) for m in mats])

    @classmethod
    def from_shape(cls, curve: int, order: int, shape: R1CSShape, num_cons: int, num_vars: int, num_io: int) -> "SpartanKzgProver":
        """The prover of a shape that is resident already: its transpose is made on the device (``R1CSShape.transposed``), no host CSR
        is needed.  Same arguments as ``SpartanProver.from_shape``; curve and order are BN254's.  The prover owns ``shape`` from here on
        (``close``)."""
        if (curve, order) != (CURVE_BN254, BN254_R):
            raise ValueError("the HyperKZG-opened prover runs on BN254 G1 only")
        self = cls.__new__(cls)
        self.curve, self.q, self.sf = CURVE_BN254, BN254_R, shape.field_id
        self.num_cons, self.num_vars, self.num_io = num_cons, num_vars, num_io
        assert (shape.num_cons, shape.num_vars, shape.num_io) == (num_cons, num_vars, num_io)
        self.shape = shape
        self.shape_t = shape.transposed(2 * num_vars)
        return self

    def prove(self, X, u: int, d_W, d_E, comm_W_jac, comm_E_jac, key, label: bytes = LABEL, stream=None) -> dict:
        """d_W (num_vars, 4), d_E (num_cons, 4): Montgomery device tensors (not modified); the commitments as 96-byte Jacobians; key: the
        resident BN254 ``CommitmentKey`` (powers of tau) that committed W and E, >= max(num_cons, num_vars) points."""
        q, nc, nv = self.q, self.num_cons, self.num_vars
        ell_x, ell_y = nc.bit_length() - 1, nv.bit_length()
        ell = max(nc, nv).bit_length() - 1
        bufs = dict(polys_outer=np.zeros((max(ell_x, 1), 4, 4), dtype=np.uint64), claims_outer=np.zeros((3, 4), dtype=np.uint64), eval_e=np.zeros(4, dtype=np.uint64),
                    polys_inner=np.zeros((ell_y, 3, 4), dtype=np.uint64), eval_w=np.zeros(4, dtype=np.uint64), polys_batch=np.zeros((max(ell, 1), 3, 4), dtype=np.uint64),
                    evals_batch=np.zeros((2, 4), dtype=np.uint64), **_kzg_bufs(max(ell, 1)))
        out = _lib.SpartanKzgProofStruct(*[bufs[k].ctypes.data for k, _ in _lib.SpartanKzgProofStruct._fields_])
        X = list(X)
        x = sumcheck._limbs([int(v) % q for v in X]) if X else np.zeros((1, 4), dtype=np.uint64)
        uu = sumcheck._limbs([int(u) % q])
        cw, ce = np.ascontiguousarray(comm_W_jac, dtype=np.uint64), np.ascontiguousarray(comm_E_jac, dtype=np.uint64)
        _lib.check(_lib.load().lurk_hip_spartan_kzg_prove_dev(self.shape._h, self.shape_t._h, nc, nv, len(X), key._ctx, _lib.ptr(x), _lib.ptr(uu), _lib.ptr(d_W),
                                                              _lib.ptr(d_E), _lib.ptr(cw), _lib.ptr(ce), label, len(label), ctypes.byref(out), _lib.ptr(_stream(stream))))
        ints = sumcheck._ints
        return dict(polys_outer=[ints(bufs["polys_outer"][j]) for j in range(ell_x)], claims_outer=ints(bufs["claims_outer"]), eval_E=ints(bufs["eval_e"])[0],
                    polys_inner=[ints(bufs["polys_inner"][j]) for j in range(ell_y)], eval_W=ints(bufs["eval_w"])[0],
                    polys_batch=[ints(bufs["polys_batch"][j]) for j in range(ell)], evals_batch=ints(bufs["evals_batch"]), **_kzg_out(bufs, ell))

    def close(self):
        self.shape.close()
        self.shape_t.close()


class BatchedSpartanKzgProver:
    """Several relaxed instances of different shapes under ONE BN254 key, ONE proof (lurk_hip_spartan_kzg_prove_batch_dev).
    ``provers``: one ``SpartanKzgProver`` per circuit."""

    def __init__(self, provers):
        assert provers
        self.provers = list(provers)
        self.q = BN254_R

    def prove(self, instances, key, label: bytes = LABEL_BATCHED, stream=None) -> dict:
        """instances[i] = dict(X, u, d_W, d_E, comm_W, comm_E) for provers[i]."""
        q, n = self.q, len(self.provers)
        ell_x = max(p.num_cons for p in self.provers).bit_length() - 1
        ell_y = max(p.num_vars for p in self.provers).bit_length()
        ell = max(max(p.num_cons, p.num_vars) for p in self.provers).bit_length() - 1
        bufs = dict(polys_outer=np.zeros((max(ell_x, 1), 4, 4), dtype=np.uint64), claims_outer=np.zeros((n, 3, 4), dtype=np.uint64), evals_e=np.zeros((n, 4), dtype=np.uint64),
                    polys_inner=np.zeros((ell_y, 3, 4), dtype=np.uint64), evals_w=np.zeros((n, 4), dtype=np.uint64), polys_batch=np.zeros((max(ell, 1), 3, 4), dtype=np.uint64),
                    evals_batch=np.zeros((2 * n, 4), dtype=np.uint64), **_kzg_bufs(max(ell, 1)))
        out = _lib.SpartanKzgBatchProofStruct(*[bufs[k].ctypes.data for k, _ in _lib.SpartanKzgBatchProofStruct._fields_])
        keep, arr = [], (_lib.SpartanInstanceStruct * n)()
        for i, (p, it) in enumerate(zip(self.provers, instances)):
            X = list(it["X"])
            x = sumcheck._limbs([int(v) % q for v in X]) if X else np.zeros((1, 4), dtype=np.uint64)
            uu = sumcheck._limbs([int(it["u"]) % q])
            cw, ce = np.ascontiguousarray(it["comm_W"], dtype=np.uint64), np.ascontiguousarray(it["comm_E"], dtype=np.uint64)
            d_w, d_e = it["d_W"].contiguous(), it["d_E"].contiguous()
            keep += [x, uu, cw, ce, d_w, d_e]
            arr[i] = _lib.SpartanInstanceStruct(p.shape._h.value, p.shape_t._h.value, p.num_cons, p.num_vars, len(X), x.ctypes.data, uu.ctypes.data, d_w.data_ptr(),
                                                d_e.data_ptr(), cw.ctypes.data, ce.ctypes.data)
        _lib.check(_lib.load().lurk_hip_spartan_kzg_prove_batch_dev(ctypes.cast(arr, ctypes.c_void_p), n, key._ctx, label, len(label), ctypes.byref(out),
                                                                    _lib.ptr(_stream(stream))))
        ints = sumcheck._ints
        return dict(polys_outer=[ints(bufs["polys_outer"][j]) for j in range(ell_x)], claims_outer=[ints(bufs["claims_outer"][i]) for i in range(n)],
                    evals_E=ints(bufs["evals_e"]), polys_inner=[ints(bufs["polys_inner"][j]) for j in range(ell_y)], evals_W=ints(bufs["evals_w"]),
                    polys_batch=[ints(bufs["polys_batch"][j]) for j in range(ell)], evals_batch=ints(bufs["evals_batch"]), **_kzg_out(bufs, ell))


class SpartanKzgVerifier:
    """The verifier of ``SpartanKzgProver``'s proofs up to the pairing (lurk_hip_spartan_kzg_verify_dev).  No key: HyperKZG's verifier
    needs only G = (1, 2).  The device work is two eq tables and one sparse evaluation of the resident shape."""

    def __init__(self, mats, num_cons: int, num_vars: int, num_io: int):
        self.q, self.num_cons, self.num_vars, self.num_io = BN254_R, num_cons, num_vars, num_io
        self.shape = R1CSShape(FIELD_BN254_FR, num_cons, num_vars, num_io, *mats)
        self._owns_shape = True
        self.last_failed_check = None

    @classmethod
    def from_shape(cls, shape: R1CSShape) -> "SpartanKzgVerifier":
        """Shares a resident shape (``prover.shape``): nothing is uploaded again."""
        self = cls.__new__(cls)
        self.q, self.num_cons, self.num_vars, self.num_io = BN254_R, shape.num_cons, shape.num_vars, shape.num_io
        self.shape, self._owns_shape, self.last_failed_check = shape, False, None
        return self

    def _marshal(self, X, u, comm_W, comm_E, proof: dict):
        """The statement and the proof in the library's layout: (proof struct, x, u, comm_W, comm_E, the arrays the struct borrows).
        Raises _Malformed / KeyError / TypeError for what cannot be written down at all."""
        nc, nv = self.num_cons, self.num_vars
        ell_x, ell_y = nc.bit_length() - 1, nv.bit_length()
        ell = max(nc, nv).bit_length() - 1
        if any(len(p) != 4 for p in proof["polys_outer"]) or any(len(p) != 3 for p in proof["polys_inner"]) or any(len(p) != 3 for p in proof["polys_batch"]):
            raise _Malformed
        bufs = dict(polys_outer=_scalars([c for p in proof["polys_outer"] for c in p], 4 * ell_x), claims_outer=_scalars(proof["claims_outer"], 3),
                    eval_e=_scalars([proof["eval_E"]], 1), polys_inner=_scalars([c for p in proof["polys_inner"] for c in p], 3 * ell_y),
                    eval_w=_scalars([proof["eval_W"]], 1), polys_batch=_scalars([c for p in proof["polys_batch"] for c in p], 3 * ell),
                    evals_batch=_scalars(proof["evals_batch"], 2), **_kzg_in(proof, ell))
        x, uu = _scalars(X, self.num_io), _scalars([u], 1)
        cw, ce = _jacobian(comm_W), _jacobian(comm_E)
        pf = _lib.SpartanKzgProofStruct(*[bufs[k].ctypes.data for k, _ in _lib.SpartanKzgProofStruct._fields_])
        return pf, x, uu, cw, ce, bufs

    def verify(self, X, u, comm_W, comm_E, proof: dict, label: bytes = LABEL, stream=None):
        """-> (accepted, L, R): accepted SO FAR; L, R: (12,) u64 Jacobians, the identity unless accepted.  The proof is valid iff accepted
        and e(L, H) == e(R, [tau]H).  The first failed check (spartan.VERIFY_*) is left in ``last_failed_check``."""
        nc, nv = self.num_cons, self.num_vars
        L, Rr = np.zeros(12, dtype=np.uint64), np.zeros(12, dtype=np.uint64)
        self.last_failed_check = VERIFY_MALFORMED
        try:
            pf, x, uu, cw, ce, _bufs = self._marshal(X, u, comm_W, comm_E, proof)
        except (_Malformed, KeyError, TypeError):
            return False, L, Rr
        acc, failed = ctypes.c_int(0), ctypes.c_int(0)
        _lib.check(_lib.load().lurk_hip_spartan_kzg_verify_dev(self.shape._h, nc, nv, self.num_io, _lib.ptr(x), _lib.ptr(uu), _lib.ptr(cw), _lib.ptr(ce), label, len(label),
                                                               ctypes.byref(pf), _lib.ptr(L), _lib.ptr(Rr), ctypes.byref(acc), ctypes.byref(failed),
                                                               _lib.ptr(_stream(stream))))
        self.last_failed_check = failed.value
        return bool(acc.value), L, Rr

    def verify_pairing(self, X, u, comm_W, comm_E, proof: dict, tau_h, label: bytes = LABEL, stream=None) -> bool:
        """The verifier that DECIDES (lurk_hip_spartan_kzg_verify_pairing_dev): ``verify`` and then e(L, H) == e(R, tau_h) against the
        verifier key tau_h = [tau]H, a (16,) u64 G2 point.  True: the proof is valid.  ``last_failed_check`` as for ``verify``, with
        VERIFY_PAIRING when only the pairing equation fails."""
        nc, nv = self.num_cons, self.num_vars
        self.last_failed_check = VERIFY_MALFORMED
        try:
            pf, x, uu, cw, ce, _bufs = self._marshal(X, u, comm_W, comm_E, proof)
        except (_Malformed, KeyError, TypeError):
            return False
        vk = np.ascontiguousarray(tau_h, dtype=np.uint64).reshape(16)
        acc, failed = ctypes.c_int(0), ctypes.c_int(0)
        _lib.check(_lib.load().lurk_hip_spartan_kzg_verify_pairing_dev(self.shape._h, nc, nv, self.num_io, _lib.ptr(x), _lib.ptr(uu), _lib.ptr(cw), _lib.ptr(ce), label,
                                                                       len(label), ctypes.byref(pf), _lib.ptr(vk), ctypes.byref(acc), ctypes.byref(failed),
                                                                       _lib.ptr(_stream(stream))))
        self.last_failed_check = failed.value
        return bool(acc.value)

    def close(self):
        if self._owns_shape:
            self.shape.close()


class BatchedSpartanKzgVerifier:
    """The verifier of ``BatchedSpartanKzgProver``'s proofs up to the pairing (lurk_hip_spartan_kzg_verify_batch_dev).  ``verifiers``: one
    ``SpartanKzgVerifier`` per circuit, in the order the batch was proved in."""

    def __init__(self, verifiers):
        assert verifiers
        self.verifiers = list(verifiers)
        self.last_failed_check = None

    def _marshal(self, instances, proof: dict):
        """The instances and the proof in the library's layout: (proof struct, instance array, the arrays they borrow)."""
        n = len(self.verifiers)
        ell_x = max(v.num_cons for v in self.verifiers).bit_length() - 1
        ell_y = max(v.num_vars for v in self.verifiers).bit_length()
        ell = max(max(v.num_cons, v.num_vars) for v in self.verifiers).bit_length() - 1
        keep, arr = [], (_lib.SpartanInstanceStruct * n)()
        if len(instances) != n:
            raise _Malformed
        if any(len(p) != 4 for p in proof["polys_outer"]) or any(len(p) != 3 for p in proof["polys_inner"]) or any(len(p) != 3 for p in proof["polys_batch"]):
            raise _Malformed
        if len(proof["claims_outer"]) != n or any(len(c) != 3 for c in proof["claims_outer"]):
            raise _Malformed
        bufs = dict(polys_outer=_scalars([c for p in proof["polys_outer"] for c in p], 4 * ell_x),
                    claims_outer=_scalars([c for cl in proof["claims_outer"] for c in cl], 3 * n), evals_e=_scalars(proof["evals_E"], n),
                    polys_inner=_scalars([c for p in proof["polys_inner"] for c in p], 3 * ell_y), evals_w=_scalars(proof["evals_W"], n),
                    polys_batch=_scalars([c for p in proof["polys_batch"] for c in p], 3 * ell), evals_batch=_scalars(proof["evals_batch"], 2 * n),
                    **_kzg_in(proof, ell))
        for i, (v, it) in enumerate(zip(self.verifiers, instances)):
            x, uu = _scalars(it["X"], v.num_io), _scalars([it["u"]], 1)
            cw, ce = _jacobian(it["comm_W"]), _jacobian(it["comm_E"])
            keep += [x, uu, cw, ce]
            arr[i] = _lib.SpartanInstanceStruct(v.shape._h.value, None, v.num_cons, v.num_vars, v.num_io, x.ctypes.data, uu.ctypes.data, None, None, cw.ctypes.data,
                                                ce.ctypes.data)
        pf = _lib.SpartanKzgBatchProofStruct(*[bufs[k].ctypes.data for k, _ in _lib.SpartanKzgBatchProofStruct._fields_])
        return pf, arr, (keep, bufs)

    def verify(self, instances, proof: dict, label: bytes = LABEL_BATCHED, stream=None):
        """instances[i] = dict(X, u, comm_W, comm_E) (further keys are ignored).  -> (accepted, L, R) as ``SpartanKzgVerifier.verify``."""
        n = len(self.verifiers)
        L, Rr = np.zeros(12, dtype=np.uint64), np.zeros(12, dtype=np.uint64)
        self.last_failed_check = VERIFY_MALFORMED
        try:
            pf, arr, _keep = self._marshal(instances, proof)
        except (_Malformed, KeyError, TypeError):
            return False, L, Rr
        acc, failed = ctypes.c_int(0), ctypes.c_int(0)
        _lib.check(_lib.load().lurk_hip_spartan_kzg_verify_batch_dev(ctypes.cast(arr, ctypes.c_void_p), n, label, len(label), ctypes.byref(pf), _lib.ptr(L), _lib.ptr(Rr),
                                                                     ctypes.byref(acc), ctypes.byref(failed), _lib.ptr(_stream(stream))))
        self.last_failed_check = failed.value
        return bool(acc.value), L, Rr

    def verify_pairing(self, instances, proof: dict, tau_h, label: bytes = LABEL_BATCHED, stream=None) -> bool:
        """The verifier that DECIDES (lurk_hip_spartan_kzg_verify_pairing_batch_dev): as ``SpartanKzgVerifier.verify_pairing``."""
        n = len(self.verifiers)
        self.last_failed_check = VERIFY_MALFORMED
        try:
            pf, arr, _keep = self._marshal(instances, proof)
        except (_Malformed, KeyError, TypeError):
            return False
        vk = np.ascontiguousarray(tau_h, dtype=np.uint64).reshape(16)
        acc, failed = ctypes.c_int(0), ctypes.c_int(0)
        _lib.check(_lib.load().lurk_hip_spartan_kzg_verify_pairing_batch_dev(ctypes.cast(arr, ctypes.c_void_p), n, label, len(label), ctypes.byref(pf), _lib.ptr(vk),
                                                                             ctypes.byref(acc), ctypes.byref(failed), _lib.ptr(_stream(stream))))
        self.last_failed_check = failed.value
        return bool(acc.value)
