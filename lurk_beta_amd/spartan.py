"""Host-side orchestration of a Spartan-style SNARK for a relaxed R1CS instance over the HIP library: the
structure of arecibo's ``RelaxedR1CSSNARK::prove`` as ``CompressedSNARK::prove`` runs it per curve
(/root/reference/src/proof/nova.rs:341-356) - outer cubic sum-check, inner quadratic sum-check over (A + r B + r^2 C)(r_x, .) z,
the two evaluation claims batched to one point, one inner-product-argument opening.  Every vector (z, Az, Bz, Cz, E, the eq tables, the
key) stays in HBM; the host runs the transcript and moves a few field elements per round.

NOT byte-compatible with arecibo (its Keccak256 transcript and claim rescaling are replaced by the SHA3-based transcript and the
zero padding documented in oracle/spartan_ref.py, whose prover this one must match element for element and whose verifier must
accept the result): no proof bytes exist upstream to be compatible with."""
from __future__ import annotations

import os

import numpy as np

from . import _lib, ipa, sumcheck
from .fold import R1CSShape, fold_vec
from .msm import point_to_affine, require_pasta_curve


class Transcript:
    """arecibo's Keccak256Transcript (the transcript of RelaxedR1CSSNARK / BatchedRelaxedR1CSSNARK, /root/reference/src/proof/nova.rs:92,
    supernova.rs:110) through the library's host implementation (lurk_hip_keccak_transcript_*: restated from arecibo's source, unpinned;
    oracle/keccak_transcript.py is the independent restatement the tests compare with).  The labels and the order of what this prover
    absorbs are its own (oracle/spartan_ref.py): the PROTOCOL is not arecibo's byte for byte, the transcript construction is."""

    _FIELD = {0x40000000000000000000000000000000224698FC094CF91B992D30ED00000001: 0,
              0x40000000000000000000000000000000224698FC0994A8DD8C46EB2100000001: 1,
              0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001: 2}

    def __init__(self, label: bytes, curve: int = 0):
        import ctypes

        self._curve = curve
        self._h = ctypes.c_void_p()
        full = b"lurk-hip spartan v2" + label
        _lib.check(_lib.load().lurk_hip_keccak_transcript_new(ctypes.byref(self._h), full, len(full)))

    def __del__(self):
        try:
            if self._h:
                _lib.load().lurk_hip_keccak_transcript_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def absorb(self, label: bytes, data: bytes):
        _lib.check(_lib.load().lurk_hip_keccak_transcript_absorb(self._h, label, len(label), bytes(data), len(data)))

    def absorb_scalars(self, label: bytes, xs):
        arr = sumcheck._limbs([int(x) for x in xs])
        _lib.check(_lib.load().lurk_hip_keccak_transcript_absorb_scalars(self._h, label, len(label), _lib.ptr(arr), arr.shape[0]))

    def absorb_point(self, label: bytes, xy):
        """xy: affine canonical integers ((0, 0) = the identity), as point_to_affine returns them."""
        x, y = int(xy[0]), int(xy[1])
        self.absorb(label, x.to_bytes(32, "big") + y.to_bytes(32, "big") + (b"\x00" if (x, y) == (0, 0) else b"\x01"))

    def absorb_jacobian(self, label: bytes, jac96: np.ndarray):
        j = np.ascontiguousarray(jac96, dtype=np.uint64)
        _lib.check(_lib.load().lurk_hip_keccak_transcript_absorb_point(self._h, label, len(label), self._curve, _lib.ptr(j)))

    def rounds(self, modulus: int, absorb: bytes, squeeze: bytes, absorb2: bytes = b"", cap: int = 64):
        """A ``challenge`` argument for sumcheck.prove* / ipa.prove over THIS transcript that stays inside the library (sum-check: the round
        polynomial under ``absorb``, the challenge under ``squeeze``; inner-product argument: L under ``absorb``, R under ``absorb2``)."""
        return _lib.KeccakRounds(self._h, self._FIELD[modulus], absorb, squeeze, absorb2=absorb2, curve=self._curve, cap=cap)

    def squeeze(self, label: bytes, modulus: int) -> int:
        out = np.zeros(4, dtype=np.uint64)
        _lib.check(_lib.load().lurk_hip_keccak_transcript_squeeze(self._h, label, len(label), self._FIELD[modulus], _lib.ptr(out)))
        return sumcheck._ints(out)[0]


def transpose_csr(indptr, indices, data, ncols: int):
    """CSR (rows x ncols) -> CSR of the transpose (ncols x rows); data: (nnz, 4) u64."""
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int64)
    data = np.ascontiguousarray(data, dtype=np.uint64).reshape(-1, 4)
    rows = np.repeat(np.arange(indptr.size - 1, dtype=np.int64), np.diff(indptr))
    order = np.argsort(indices, kind="stable")
    t_indptr = np.zeros(ncols + 1, dtype=np.uint64)
    np.cumsum(np.bincount(indices, minlength=ncols), out=t_indptr[1:])
    return t_indptr, rows[order].astype(np.uint64), np.ascontiguousarray(data[order])


class SpartanProver:
    """Keeps the shape and its transpose resident.  mats: (A, B, C) as (indptr, indices, data Montgomery) over columns
    z = [W | u | X | 0 ...] of length 2 num_vars; num_cons and num_vars powers of two."""

    def __init__(self, curve: int, order: int, mats, num_cons: int, num_vars: int, num_io: int):
        require_pasta_curve(curve, "the compressing SNARK")
        self.curve, self.q, self.num_cons, self.num_vars, self.num_io = curve, order, num_cons, num_vars, num_io
        self.sf = 1 if curve == 0 else 0
        assert num_cons & (num_cons - 1) == 0 and num_vars & (num_vars - 1) == 0 and 1 + num_io <= num_vars
        self.shape = R1CSShape(self.sf, num_cons, num_vars, num_io, *mats)
        # the transpose acts on eq(r_x) (num_cons entries = its "z") and yields 2 num_vars rows
        self.shape_t = R1CSShape(self.sf, 2 * num_vars, num_cons - 1, 0, *[transpose_csr(*m, 2 * num_vars) for m in mats])
        self.R = (1 << 256) % order
        self.Rinv = pow(self.R, order - 2, order)

    @classmethod
    def from_shape(cls, curve: int, order: int, shape: R1CSShape, num_cons: int, num_vars: int, num_io: int) -> "SpartanProver":
        """The prover of a shape that is resident already (one the library built, ``R1CSShape.for_frames``, or any other): its transpose
        is made on the device (``R1CSShape.transposed``), no host CSR is needed.  The prover owns ``shape`` from here on (``close``)."""
        require_pasta_curve(curve, "the compressing SNARK")
        self = cls.__new__(cls)
        self.curve, self.q, self.num_cons, self.num_vars, self.num_io = curve, order, num_cons, num_vars, num_io
        self.sf = 1 if curve == 0 else 0
        assert num_cons & (num_cons - 1) == 0 and num_vars & (num_vars - 1) == 0 and 1 + num_io <= num_vars
        assert (shape.field_id, shape.num_cons, shape.num_vars, shape.num_io) == (self.sf, num_cons, num_vars, num_io)
        self.shape = shape
        self.shape_t = shape.transposed(2 * num_vars)
        self.R = (1 << 256) % order
        self.Rinv = pow(self.R, order - 2, order)
        return self

    def _mont(self, vals) -> np.ndarray:
        return sumcheck._limbs([int(v) * self.R % self.q for v in vals])

    def _dev(self, vals):
        import torch

        return torch.from_numpy(self._mont(vals).view(np.int64)).cuda()

    def _mle(self, d_table, point) -> int:
        import torch

        lib = _lib.load()
        if len(point) == 0:
            return sumcheck._ints(d_table[:1].cpu().numpy().view(np.uint64))[0] * self.Rinv % self.q
        eq = sumcheck.eq_evals(self.sf, self._mont(point))
        out = np.zeros(4, dtype=np.uint64)
        _lib.check(lib.lurk_hip_inner_product_dev(self.sf, _lib.ptr(d_table), _lib.ptr(eq), 1 << len(point), _lib.ptr(out), _lib.ptr(torch.cuda.current_stream().cuda_stream)))
        return sumcheck._ints(out)[0] * self.Rinv % self.q

    def prove(self, X, u: int, d_W, d_E, d_ck, comm_W_jac, comm_E_jac, key=None, in_library=None) -> dict:
        """key: the resident ``CommitmentKey`` over d_ck[:N] (the one that committed W and E): the opening argument then runs under it
        without folding the key (ipa.py).  d_W (num_vars, 4), d_E (num_cons, 4): Montgomery device tensors (not modified); d_ck: (N + 1, 8) affine Montgomery points,
        N = max(num_cons, num_vars), the last one the inner-product base; commitments as 96-byte Jacobians."""
        import torch

        q, sf, nc, nv = self.q, self.sf, self.num_cons, self.num_vars
        ell_x, ell_y = nc.bit_length() - 1, nv.bit_length()
        N = max(nc, nv)
        ell = N.bit_length() - 1
        curve_name = b"pallas" if self.curve == 0 else b"vesta"
        if in_library is None:
            in_library = os.environ.get("LURK_SPARTAN_PROVER", "python") == "library"
        if key is not None and in_library:
            # the whole prover as ONE call (lurk_hip_spartan_prove_dev: what a Rust caller binds): this method then only marshals.  Since the
            # library takes its scratch from one arena per stream (round 5) it is the faster form - 30.5 against 30.8 ms per 2^20 proof on one
            # box - and bench.py's default; the sequence below stays as the mirror the tests compare it with
            return self._prove_lib(X, u, d_W, d_E, d_ck, comm_W_jac, comm_E_jac, key, b"lurk-hip spartan v2" + curve_name)
        tr = Transcript(curve_name, self.curve)
        tr.absorb_point(b"comm_W", point_to_affine(self.curve, comm_W_jac))
        tr.absorb_point(b"comm_E", point_to_affine(self.curve, comm_E_jac))
        tr.absorb_scalars(b"uX", [u] + list(X))
        d_z = torch.zeros((2 * nv, 4), dtype=torch.int64, device="cuda")
        d_z[:nv] = d_W
        d_z[nv:nv + 1 + len(X)] = self._dev([u] + list(X))
        d_az, d_bz, d_cz = self.shape.multiply_vec(d_z[: self.shape.num_cols])
        tau = [tr.squeeze(b"t", q) for _ in range(ell_x)]
        d_tau = sumcheck.eq_evals(sf, self._mont(tau))
        d_ucze = fold_vec(sf, d_E, d_cz, self._mont([u]))  # E + u Cz

        # the rounds' transcript work (absorb the round polynomial under "p", squeeze the challenge under "c") happens inside the library
        rounds_outer = tr.rounds(q, b"p", b"c")
        polys_outer, finals, _ = sumcheck.prove(sf, q, 0, [d_tau, d_az.clone(), d_bz.clone(), d_ucze], rounds_outer)
        r_x = rounds_outer.challenges()
        claim_Az, claim_Bz = finals[1], finals[2]
        claim_Cz, eval_E = self._mle(d_cz, r_x), self._mle(d_E, r_x)
        tr.absorb_scalars(b"claims_outer", [claim_Az, claim_Bz, claim_Cz, eval_E])
        r = tr.squeeze(b"r", q)
        claim_inner = (claim_Az + r * claim_Bz + r * r * claim_Cz) % q
        d_eq_rx = sumcheck.eq_evals(sf, self._mont(r_x))
        d_ea, d_eb, d_ec = self.shape_t.multiply_vec(d_eq_rx)
        d_abc = fold_vec(sf, fold_vec(sf, d_ea, d_eb, self._mont([r])), d_ec, self._mont([r * r % q]))
        rounds_inner = tr.rounds(q, b"p", b"c")
        polys_inner, _, _ = sumcheck.prove(sf, q, claim_inner, [d_abc, d_z.clone()], rounds_inner)
        r_y = rounds_inner.challenges()
        eval_W = self._mle(d_W, r_y[1:])
        tr.absorb_scalars(b"eval_W", [eval_W])
        # ---- the two evaluation claims -> one point
        d_p1 = torch.zeros((N, 4), dtype=torch.int64, device="cuda")
        d_p2 = torch.zeros((N, 4), dtype=torch.int64, device="cuda")
        d_p1[:nv] = d_W
        d_p2[:nc] = d_E
        x1 = [0] * (ell - (ell_y - 1)) + r_y[1:]
        x2 = [0] * (ell - ell_x) + r_x
        rho = tr.squeeze(b"rho", q)
        pairs = [(sumcheck.eq_evals(sf, self._mont(x1)), d_p1.clone()), (sumcheck.eq_evals(sf, self._mont(x2)), d_p2.clone())]
        polys_batch, r_z, fin, _ = sumcheck.prove_quad_batch(sf, q, [eval_W, eval_E], pairs, [1, rho], tr.rounds(q, b"p", b"c"))
        evals_batch = [fin[0][1], fin[1][1]]
        tr.absorb_scalars(b"evals_batch", evals_batch)
        gamma = tr.squeeze(b"gamma", q)
        d_joint = fold_vec(sf, d_p1, d_p2, self._mont([gamma]))
        r0 = tr.squeeze(b"ipa_r0", q)

        ipa_chal = tr.rounds(q, b"L", b"r", absorb2=b"R")  # L, R absorbed as affine points, r squeezed: inside the library's round loop

        ck_c = d_ck[N].cpu().numpy().view(np.uint64).reshape(8)
        bf = 0 if self.curve == 0 else 1
        ck_c_jac = np.concatenate([ck_c, _mont_one(bf)])
        Ls, Rs, a_hat, _ = ipa.prove(self.curve, q, None if key is not None else d_ck[:N].clone(), ck_c_jac, d_joint, sumcheck.eq_evals(sf, self._mont(r_z)), r0,
                                     ipa_chal, key=key)
        aff = lambda P: (lambda xy: None if xy == (0, 0) else xy)(point_to_affine(self.curve, P))
        return dict(polys_outer=polys_outer, claims_outer=[claim_Az, claim_Bz, claim_Cz], eval_E=eval_E, polys_inner=polys_inner, eval_W=eval_W,
                    polys_batch=polys_batch, evals_batch=evals_batch, ipa_L=[aff(x) for x in Ls], ipa_R=[aff(x) for x in Rs], ipa_a=a_hat)

    def _prove_lib(self, X, u, d_W, d_E, d_ck, comm_W_jac, comm_E_jac, key, label: bytes) -> dict:
        import ctypes

        import torch

        q, nc, nv = self.q, self.num_cons, self.num_vars
        ell_x, ell_y = nc.bit_length() - 1, nv.bit_length()
        N = max(nc, nv)
        ell = N.bit_length() - 1
        bufs = dict(polys_outer=np.zeros((ell_x, 4, 4), dtype=np.uint64), claims_outer=np.zeros((3, 4), dtype=np.uint64), eval_e=np.zeros(4, dtype=np.uint64),
                    polys_inner=np.zeros((ell_y, 3, 4), dtype=np.uint64), eval_w=np.zeros(4, dtype=np.uint64), polys_batch=np.zeros((max(ell, 1), 3, 4), dtype=np.uint64),
                    evals_batch=np.zeros((2, 4), dtype=np.uint64), ipa_l=np.zeros((max(ell, 1), 12), dtype=np.uint64), ipa_r=np.zeros((max(ell, 1), 12), dtype=np.uint64),
                    ipa_a=np.zeros(4, dtype=np.uint64))
        out = _lib.SpartanProofStruct(*[bufs[k].ctypes.data for k, _ in _lib.SpartanProofStruct._fields_])
        ck_c = d_ck[N].cpu().numpy().view(np.uint64).reshape(8)
        ck_c_jac = np.concatenate([ck_c, _mont_one(0 if self.curve == 0 else 1)])
        x = sumcheck._limbs([int(v) % q for v in X]) if len(X) else np.zeros((1, 4), dtype=np.uint64)
        uu = sumcheck._limbs([int(u) % q])
        cw, ce = np.ascontiguousarray(comm_W_jac, dtype=np.uint64), np.ascontiguousarray(comm_E_jac, dtype=np.uint64)
        s = torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.load().lurk_hip_spartan_prove_dev(self.shape._h, self.shape_t._h, nc, nv, len(X), key._ctx, _lib.ptr(ck_c_jac), _lib.ptr(x), _lib.ptr(uu),
                                                          _lib.ptr(d_W), _lib.ptr(d_E), _lib.ptr(cw), _lib.ptr(ce), label, len(label), ctypes.byref(out), _lib.ptr(s)))
        ints = sumcheck._ints
        aff = lambda P: (lambda xy: None if xy == (0, 0) else xy)(point_to_affine(self.curve, P))
        return dict(polys_outer=[ints(bufs["polys_outer"][j]) for j in range(ell_x)], claims_outer=ints(bufs["claims_outer"]), eval_E=ints(bufs["eval_e"])[0],
                    polys_inner=[ints(bufs["polys_inner"][j]) for j in range(ell_y)], eval_W=ints(bufs["eval_w"])[0],
                    polys_batch=[ints(bufs["polys_batch"][j]) for j in range(ell)], evals_batch=ints(bufs["evals_batch"]),
                    ipa_L=[aff(bufs["ipa_l"][j]) for j in range(ell)], ipa_R=[aff(bufs["ipa_r"][j]) for j in range(ell)], ipa_a=ints(bufs["ipa_a"])[0])

    def close(self):
        self.shape.close()
        self.shape_t.close()


def _mont_one(base_field_id: int) -> np.ndarray:
    p = (0x40000000000000000000000000000000224698FC094CF91B992D30ED00000001, 0x40000000000000000000000000000000224698FC0994A8DD8C46EB2100000001)[base_field_id]
    return sumcheck._limbs([(1 << 256) % p])[0]


class BatchedSpartanProver:
    """Several relaxed R1CS instances of different shapes and sizes under ONE commitment key, ONE proof: the structure of arecibo's
    ``spartan::batched::BatchedRelaxedR1CSSNARK``, which lurk-beta's SuperNova prover compresses with
    (/root/reference/src/proof/supernova.rs:110, 293-302).  One outer (cubic) and one inner (quadratic) sum-check shared by all instances
    through random linear combinations, every instance's two evaluation claims batched to one point, one inner-product-argument opening
    under the resident key.  Not byte-compatible (oracle/spartan_fast.py: prove_batched explains the padding and the transcript); its proof
    must equal that oracle's element for element.  ``provers``: one ``SpartanProver`` per circuit (shape and transpose resident)."""

    def __init__(self, provers):
        assert provers and all(p.curve == provers[0].curve for p in provers)
        self.provers = list(provers)
        self.curve, self.q, self.sf = provers[0].curve, provers[0].q, provers[0].sf

    def prove(self, instances, d_ck, key=None, in_library=None) -> dict:
        """instances[i] = dict(X, u, d_W, d_E, comm_W, comm_E) for provers[i] (device tensors Montgomery, commitments 96-byte Jacobians).
        d_ck: (N + 1, 8) affine Montgomery points, N = the largest num_cons / num_vars; key: the resident CommitmentKey over d_ck[:N].
        in_library (with a resident key): the whole prover as ONE library call, lurk_hip_spartan_prove_batch_dev - what a Rust caller binds;
        the sequence below is its mirror, kept for the tests (both must give the oracle's proof)."""
        import torch

        if in_library is None:
            in_library = os.environ.get("LURK_SPARTAN_PROVER", "python") == "library"
        if key is not None and in_library:
            return self._prove_lib(instances, d_ck, key)

        q, sf, n = self.q, self.sf, len(self.provers)
        P0 = self.provers[0]
        mont, dev, pad = P0._mont, P0._dev, lambda t, m: torch.cat([t, torch.zeros((m - t.shape[0], 4), dtype=torch.int64, device="cuda")]) if t.shape[0] < m else t.clone()
        ell_x = max(p.num_cons for p in self.provers).bit_length() - 1
        ell_y = max(p.num_vars for p in self.provers).bit_length()
        N = max(max(p.num_cons, p.num_vars) for p in self.provers)
        ell = N.bit_length() - 1
        tr = Transcript((b"pallas" if self.curve == 0 else b"vesta") + b"/batched", self.curve)
        tr.absorb_scalars(b"n", [n])
        aff0 = lambda J: (lambda xy: None if xy == (0, 0) else xy)(point_to_affine(self.curve, J))  # the proof's point form: None = the identity
        absorb_pt = lambda label, J: tr.absorb_point(label, point_to_affine(self.curve, J))          # the transcript's: (0, 0) = the identity

        for it in instances:
            absorb_pt(b"comm_W", it["comm_W"])
            absorb_pt(b"comm_E", it["comm_E"])
            tr.absorb_scalars(b"uX", [it["u"]] + list(it["X"]))
        tau = [tr.squeeze(b"t", q) for _ in range(ell_x)]
        rho_o = tr.squeeze(b"rho_outer", q)
        d_tau = sumcheck.eq_evals(sf, mont(tau))
        zs, czs, quads = [], [], []
        for p, it in zip(self.provers, instances):
            nv = p.num_vars
            d_z = torch.zeros((2 * nv, 4), dtype=torch.int64, device="cuda")
            d_z[:nv] = it["d_W"]
            d_z[nv:nv + 1 + len(it["X"])] = dev([it["u"]] + list(it["X"]))
            d_az, d_bz, d_cz = p.shape.multiply_vec(d_z[: p.shape.num_cols])
            d_ucze = fold_vec(sf, it["d_E"], d_cz, mont([it["u"]]))
            zs.append(d_z)
            czs.append(d_cz)
            quads.append((d_tau.clone(), pad(d_az, 1 << ell_x), pad(d_bz, 1 << ell_x), pad(d_ucze, 1 << ell_x)))

        chal = lambda: tr.rounds(q, b"p", b"c")  # every round's absorb / squeeze inside the library's loop

        polys_outer, r_x, fin, _ = sumcheck.prove_cubic_batch(sf, q, quads, [pow(rho_o, i, q) for i in range(n)], chal())
        d_eq_rx = sumcheck.eq_evals(sf, mont(r_x))
        claims_outer, evals_E = [], []
        for p, it, f4, d_cz in zip(self.provers, instances, fin, czs):
            nc = p.num_cons
            px = ell_x - (nc.bit_length() - 1)
            claims_outer.append([f4[1], f4[2], self._ip(d_cz, d_eq_rx[:nc])])
            evals_E.append(p._mle(it["d_E"], r_x[px:]))
        tr.absorb_scalars(b"claims_outer", [c for cl in claims_outer for c in cl] + evals_E)
        r = tr.squeeze(b"r", q)
        rho_i = tr.squeeze(b"rho_inner", q)
        pairs, claims_inner = [], []
        for p, d_z, cl in zip(self.provers, zs, claims_outer):
            d_ea, d_eb, d_ec = p.shape_t.multiply_vec(d_eq_rx[: p.num_cons].contiguous())
            d_abc = fold_vec(sf, fold_vec(sf, d_ea, d_eb, mont([r])), d_ec, mont([r * r % q]))
            pairs.append((pad(d_abc, 1 << ell_y), pad(d_z, 1 << ell_y)))
            claims_inner.append((cl[0] + r * cl[1] + r * r * cl[2]) % q)
        polys_inner, r_y, _, _ = sumcheck.prove_quad_batch(sf, q, claims_inner, pairs, [pow(rho_i, i, q) for i in range(n)], chal())
        evals_W = []
        for p, it in zip(self.provers, instances):
            py = ell_y - p.num_vars.bit_length()
            evals_W.append(p._mle(it["d_W"], r_y[py + 1:]))
        tr.absorb_scalars(b"evals_W", evals_W)
        polys, points, claims = [], [], []
        for p, it, eW, eE in zip(self.provers, instances, evals_W, evals_E):
            nc, nv = p.num_cons, p.num_vars
            py, px = ell_y - nv.bit_length(), ell_x - (nc.bit_length() - 1)
            polys += [pad(it["d_W"], N), pad(it["d_E"], N)]
            points += [[0] * (ell - (nv.bit_length() - 1)) + r_y[py + 1:], [0] * (ell - (nc.bit_length() - 1)) + r_x[px:]]
            claims += [eW, eE]
        rho = tr.squeeze(b"rho", q)
        bp = [(sumcheck.eq_evals(sf, mont(x)), pl.clone()) for x, pl in zip(points, polys)]
        polys_batch, r_z, finb, _ = sumcheck.prove_quad_batch(sf, q, claims, bp, [pow(rho, k, q) for k in range(2 * n)], chal())
        evals_batch = [fb[1] for fb in finb]
        tr.absorb_scalars(b"evals_batch", evals_batch)
        gamma = tr.squeeze(b"gamma", q)
        d_joint = polys[0].clone()
        for k in range(1, 2 * n):
            d_joint = fold_vec(sf, d_joint, polys[k], mont([pow(gamma, k, q)]))
        r0 = tr.squeeze(b"ipa_r0", q)

        ipa_chal = tr.rounds(q, b"L", b"r", absorb2=b"R")

        ck_c = d_ck[N].cpu().numpy().view(np.uint64).reshape(8)
        ck_c_jac = np.concatenate([ck_c, _mont_one(0 if self.curve == 0 else 1)])
        Ls, Rs, a_hat, _ = ipa.prove(self.curve, q, None if key is not None else d_ck[:N].clone(), ck_c_jac, d_joint, sumcheck.eq_evals(sf, mont(r_z)), r0,
                                     ipa_chal, key=key)
        return dict(polys_outer=polys_outer, claims_outer=claims_outer, evals_E=evals_E, polys_inner=polys_inner, evals_W=evals_W, polys_batch=polys_batch,
                    evals_batch=evals_batch, ipa_L=[aff0(x) for x in Ls], ipa_R=[aff0(x) for x in Rs], ipa_a=a_hat)

    def _prove_lib(self, instances, d_ck, key) -> dict:
        import ctypes

        import torch

        q, n = self.q, len(self.provers)
        ell_x = max(p.num_cons for p in self.provers).bit_length() - 1
        ell_y = max(p.num_vars for p in self.provers).bit_length()
        N = max(max(p.num_cons, p.num_vars) for p in self.provers)
        ell = N.bit_length() - 1
        bufs = dict(polys_outer=np.zeros((ell_x, 4, 4), dtype=np.uint64), claims_outer=np.zeros((n, 3, 4), dtype=np.uint64), evals_e=np.zeros((n, 4), dtype=np.uint64),
                    polys_inner=np.zeros((ell_y, 3, 4), dtype=np.uint64), evals_w=np.zeros((n, 4), dtype=np.uint64), polys_batch=np.zeros((max(ell, 1), 3, 4), dtype=np.uint64),
                    evals_batch=np.zeros((2 * n, 4), dtype=np.uint64), ipa_l=np.zeros((max(ell, 1), 12), dtype=np.uint64), ipa_r=np.zeros((max(ell, 1), 12), dtype=np.uint64),
                    ipa_a=np.zeros(4, dtype=np.uint64))
        out = _lib.SpartanBatchProofStruct(*[bufs[k].ctypes.data for k, _ in _lib.SpartanBatchProofStruct._fields_])
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
        ck_c = d_ck[N].cpu().numpy().view(np.uint64).reshape(8)
        ck_c_jac = np.concatenate([ck_c, _mont_one(0 if self.curve == 0 else 1)])
        label = b"lurk-hip spartan v2" + (b"pallas" if self.curve == 0 else b"vesta") + b"/batched"  # (what Transcript prepends)
        s = torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.load().lurk_hip_spartan_prove_batch_dev(ctypes.cast(arr, ctypes.c_void_p), n, key._ctx, _lib.ptr(ck_c_jac), label, len(label), ctypes.byref(out),
                                                                _lib.ptr(s)))
        ints = sumcheck._ints
        aff = lambda P: (lambda xy: None if xy == (0, 0) else xy)(point_to_affine(self.curve, P))
        return dict(polys_outer=[ints(bufs["polys_outer"][j]) for j in range(ell_x)], claims_outer=[ints(bufs["claims_outer"][i]) for i in range(n)],
                    evals_E=ints(bufs["evals_e"]), polys_inner=[ints(bufs["polys_inner"][j]) for j in range(ell_y)], evals_W=ints(bufs["evals_w"]),
                    polys_batch=[ints(bufs["polys_batch"][j]) for j in range(ell)], evals_batch=ints(bufs["evals_batch"]),
                    ipa_L=[aff(bufs["ipa_l"][j]) for j in range(ell)], ipa_R=[aff(bufs["ipa_r"][j]) for j in range(ell)], ipa_a=ints(bufs["ipa_a"])[0])

    def _ip(self, d_a, d_b) -> int:
        import torch

        out = np.zeros(4, dtype=np.uint64)
        d_b = d_b.contiguous()
        _lib.check(_lib.load().lurk_hip_inner_product_dev(self.sf, _lib.ptr(d_a), _lib.ptr(d_b), d_a.shape[0], _lib.ptr(out),
                                                          _lib.ptr(torch.cuda.current_stream().cuda_stream)))
        return sumcheck._ints(out)[0] * self.provers[0].Rinv % self.q


# ---- the verifiers -----------------------------------------------------------------------------------------------------------------
# failed-check codes of the library's verifiers (include/lurk_hip.h: LURK_VERIFY_*)
VERIFY_ACCEPTED, VERIFY_MALFORMED, VERIFY_OUTER, VERIFY_INNER, VERIFY_BATCH, VERIFY_OPENING = 0, 1, 2, 3, 4, 5
_BASE_P = (0x40000000000000000000000000000000224698FC094CF91B992D30ED00000001, 0x40000000000000000000000000000000224698FC0994A8DD8C46EB2100000001)


class _Malformed(Exception):
    """a value of the proof or the statement that cannot be marshalled (wrong count, not a 256-bit integer, a coordinate not reduced)"""


def _scalars(vals, count: int) -> np.ndarray:
    """`count` canonical integers as limbs, NOT reduced: the library rejects what is not below the field order."""
    vals = list(vals)
    if len(vals) != count:
        raise _Malformed
    if any(not isinstance(v, (int, np.integer)) or int(v) < 0 or int(v) >> 256 for v in vals):
        raise _Malformed
    return sumcheck._limbs([int(v) for v in vals]) if count else np.zeros((1, 4), dtype=np.uint64)


def _jacobian(curve: int, pt) -> np.ndarray:
    """A point as the proof dictionaries carry it (affine canonical integers, None = the identity) or as a 96-byte Jacobian -> Jacobian."""
    if pt is None:
        return np.zeros(12, dtype=np.uint64)
    if isinstance(pt, np.ndarray):
        if pt.size != 12:
            raise _Malformed
        return np.ascontiguousarray(pt, dtype=np.uint64).reshape(12)
    p = _BASE_P[0 if curve == 0 else 1]
    if len(pt) != 2 or any(int(c) < 0 or int(c) >= p for c in pt):
        raise _Malformed
    R = (1 << 256) % p
    return np.concatenate([sumcheck._limbs([int(pt[0]) * R % p, int(pt[1]) * R % p]).reshape(8), sumcheck._limbs([R])[0]])


def _ck_c_jacobian(curve: int, N: int, d_ck, ck_c) -> np.ndarray:
    if ck_c is None:
        if d_ck is None:
            raise ValueError("the inner-product base is needed: d_ck (N + 1 points, the last one the base) or ck_c")
        row = d_ck[N]
        ck_c = (row.cpu().numpy() if hasattr(row, "cpu") else np.asarray(row)).view(np.uint64).reshape(8)
    ck_c = np.ascontiguousarray(ck_c, dtype=np.uint64).reshape(-1)
    return ck_c if ck_c.size == 12 else np.concatenate([ck_c, _mont_one(0 if curve == 0 else 1)])


def _points(curve: int, pts, count: int) -> np.ndarray:
    pts = list(pts)
    if len(pts) != count:
        raise _Malformed
    out = np.zeros((max(count, 1), 12), dtype=np.uint64)
    for j, pt in enumerate(pts):
        out[j] = _jacobian(curve, pt)
    return out


class SpartanVerifier:
    """The verifier of ``SpartanProver``'s proofs (CompressedSNARK::verify per curve, /root/reference/src/proof/nova.rs:358-373) as ONE
    library call, lurk_hip_spartan_verify_dev: the shape stays resident, a verification runs two eq tables, one sparse evaluation of the
    shape, the s vector and one commitment under the resident key on the device, the rest on the host.  mats as for the prover."""

    def __init__(self, curve: int, order: int, mats, num_cons: int, num_vars: int, num_io: int):
        require_pasta_curve(curve, "the compressing SNARK")
        self.curve, self.q, self.num_cons, self.num_vars, self.num_io = curve, order, num_cons, num_vars, num_io
        self.sf = 1 if curve == 0 else 0
        assert num_cons & (num_cons - 1) == 0 and num_vars & (num_vars - 1) == 0 and 1 + num_io <= num_vars
        self.shape = R1CSShape(self.sf, num_cons, num_vars, num_io, *mats)
        self._owns_shape = True
        self.last_failed_check = None

    @classmethod
    def from_shape(cls, shape: R1CSShape, curve: int, order: int) -> "SpartanVerifier":
        """Shares a resident shape (``prover.shape``): nothing is uploaded again."""
        self = cls.__new__(cls)
        self.curve, self.q, self.sf = curve, order, 1 if curve == 0 else 0
        self.num_cons, self.num_vars, self.num_io = shape.num_cons, shape.num_vars, shape.num_io
        self.shape, self._owns_shape, self.last_failed_check = shape, False, None
        return self

    def verify(self, X, u, comm_W_jac, comm_E_jac, proof: dict, key, d_ck=None, ck_c=None, label: bytes = None, stream=None) -> bool:
        """proof: the dictionary the provers return.  key: the resident ``CommitmentKey`` that committed W and E; the inner-product base is
        d_ck[N] (N = max(num_cons, num_vars)) or ck_c (an affine Montgomery point or a Jacobian).  Returns the verdict; the first failed
        check (VERIFY_*) is left in ``last_failed_check`` (0 when accepted)."""
        import ctypes

        import torch

        nc, nv = self.num_cons, self.num_vars
        ell_x, ell_y = nc.bit_length() - 1, nv.bit_length()
        N = max(nc, nv)
        ell = N.bit_length() - 1
        ck_c_jac = _ck_c_jacobian(self.curve, N, d_ck, ck_c)
        if label is None:
            label = b"lurk-hip spartan v2" + (b"pallas" if self.curve == 0 else b"vesta")
        self.last_failed_check = VERIFY_MALFORMED
        try:
            if any(len(p) != 4 for p in proof["polys_outer"]) or any(len(p) != 3 for p in proof["polys_inner"]) or any(len(p) != 3 for p in proof["polys_batch"]):
                raise _Malformed
            bufs = dict(polys_outer=_scalars([c for p in proof["polys_outer"] for c in p], 4 * ell_x), claims_outer=_scalars(proof["claims_outer"], 3),
                        eval_e=_scalars([proof["eval_E"]], 1), polys_inner=_scalars([c for p in proof["polys_inner"] for c in p], 3 * ell_y),
                        eval_w=_scalars([proof["eval_W"]], 1), polys_batch=_scalars([c for p in proof["polys_batch"] for c in p], 3 * ell),
                        evals_batch=_scalars(proof["evals_batch"], 2), ipa_l=_points(self.curve, proof["ipa_L"], ell), ipa_r=_points(self.curve, proof["ipa_R"], ell),
                        ipa_a=_scalars([proof["ipa_a"]], 1))
            x, uu = _scalars(X, self.num_io), _scalars([u], 1)
            cw, ce = _jacobian(self.curve, comm_W_jac), _jacobian(self.curve, comm_E_jac)
        except (_Malformed, KeyError, TypeError):
            return False
        pf = _lib.SpartanProofStruct(*[bufs[k].ctypes.data for k, _ in _lib.SpartanProofStruct._fields_])
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        acc, failed = ctypes.c_int(0), ctypes.c_int(0)
        _lib.check(_lib.load().lurk_hip_spartan_verify_dev(self.shape._h, nc, nv, self.num_io, key._ctx, _lib.ptr(ck_c_jac), _lib.ptr(x), _lib.ptr(uu), _lib.ptr(cw),
                                                           _lib.ptr(ce), label, len(label), ctypes.byref(pf), ctypes.byref(acc), ctypes.byref(failed), _lib.ptr(s)))
        self.last_failed_check = failed.value
        return bool(acc.value)

    def close(self):
        if self._owns_shape:
            self.shape.close()


class BatchedSpartanVerifier:
    """The verifier of ``BatchedSpartanProver``'s proofs (lurk_hip_spartan_verify_batch_dev).  ``verifiers``: one ``SpartanVerifier`` per
    circuit, in the order the batch was proved in."""

    def __init__(self, verifiers):
        assert verifiers and all(v.curve == verifiers[0].curve for v in verifiers)
        self.verifiers = list(verifiers)
        self.curve, self.q = verifiers[0].curve, verifiers[0].q
        self.last_failed_check = None

    def verify(self, instances, proof: dict, key, d_ck=None, ck_c=None, label: bytes = None, stream=None) -> bool:
        """instances[i] = dict(X, u, comm_W, comm_E) for verifiers[i] (further keys - the prover's d_W, d_E - are ignored)."""
        import ctypes

        import torch

        n = len(self.verifiers)
        ell_x = max(v.num_cons for v in self.verifiers).bit_length() - 1
        ell_y = max(v.num_vars for v in self.verifiers).bit_length()
        N = max(max(v.num_cons, v.num_vars) for v in self.verifiers)
        ell = N.bit_length() - 1
        ck_c_jac = _ck_c_jacobian(self.curve, N, d_ck, ck_c)
        if label is None:
            label = b"lurk-hip spartan v2" + (b"pallas" if self.curve == 0 else b"vesta") + b"/batched"
        self.last_failed_check = VERIFY_MALFORMED
        keep, arr = [], (_lib.SpartanInstanceStruct * n)()
        try:
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
                        ipa_l=_points(self.curve, proof["ipa_L"], ell), ipa_r=_points(self.curve, proof["ipa_R"], ell), ipa_a=_scalars([proof["ipa_a"]], 1))
            for i, (v, it) in enumerate(zip(self.verifiers, instances)):
                x, uu = _scalars(it["X"], v.num_io), _scalars([it["u"]], 1)
                cw, ce = _jacobian(self.curve, it["comm_W"]), _jacobian(self.curve, it["comm_E"])
                keep += [x, uu, cw, ce]
                arr[i] = _lib.SpartanInstanceStruct(v.shape._h.value, None, v.num_cons, v.num_vars, v.num_io, x.ctypes.data, uu.ctypes.data, None, None, cw.ctypes.data,
                                                    ce.ctypes.data)
        except (_Malformed, KeyError, TypeError):
            return False
        pf = _lib.SpartanBatchProofStruct(*[bufs[k].ctypes.data for k, _ in _lib.SpartanBatchProofStruct._fields_])
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        acc, failed = ctypes.c_int(0), ctypes.c_int(0)
        _lib.check(_lib.load().lurk_hip_spartan_verify_batch_dev(ctypes.cast(arr, ctypes.c_void_p), n, key._ctx, _lib.ptr(ck_c_jac), label, len(label), ctypes.byref(pf),
                                                                 ctypes.byref(acc), ctypes.byref(failed), _lib.ptr(s)))
        self.last_failed_check = failed.value
        return bool(acc.value)
