"""Device-resident relaxed-R1CS folding: the host-side mirror of the three arecibo
operations a Nova folding step runs between its two commitments -
``R1CSShape::multiply_vec``, the cross term of ``R1CSShape::commit_T`` and ``RelaxedR1CSWitness::fold`` -
as called from ``RecursiveSNARK::prove_step`` (/root/reference/src/proof/nova.rs:291-293; arecibo is the
un-vendored ``nova`` dependency of /root/reference/Cargo.toml:128).  All arithmetic runs in liblurk_hip.so;
vectors are torch device tensors of shape (n, 4) int64 holding 32-byte Montgomery field elements."""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib


class R1CSShape:
    """CSR matrices A, B, C (each ``(indptr, indices, data)`` as arecibo's SparseMatrix: usize row pointers,
    usize column indices into z = [W | u | X], 32-byte Montgomery values) kept resident on the GPU."""

    def __init__(self, field_id: int, num_cons: int, num_vars: int, num_io: int, A, B, C):
        self.field_id, self.num_cons, self.num_vars, self.num_io = field_id, num_cons, num_vars, num_io
        self._h = self._create(_lib.load().lurk_hip_r1cs_create, field_id, num_cons, num_vars, num_io, (A, B, C))
        self._keep = None  # the library copied everything

    @staticmethod
    def _create(create, field_or_curve: int, num_cons: int, num_vars: int, num_io: int, matrices):
        args, keep = [], []
        for indptr, indices, data in matrices:
            ip = np.ascontiguousarray(indptr, dtype=np.uint64)
            ix = np.ascontiguousarray(indices, dtype=np.uint64)
            dv = np.ascontiguousarray(data, dtype=np.uint64)
            if ip.size != num_cons + 1 or ix.size * 4 != dv.size:
                raise ValueError("malformed CSR matrix")
            keep += [ip, ix, dv]
            args += [_lib.ptr(ip), _lib.ptr(ix), _lib.ptr(dv)]
        h = ctypes.c_void_p()
        _lib.check(create(ctypes.byref(h), field_or_curve, num_cons, num_vars, num_io, *args))
        return h

    @classmethod
    def for_curve(cls, curve: int, num_cons: int, num_vars: int, num_io: int, A, B, C) -> "R1CSShape":
        """The same shape over the SCALAR field of ``curve`` (``lurk_hip_r1cs_create_for_curve``): the one way to a shape over the BN254
        base field, Grumpkin's scalar field, which ``FoldingContext(CURVE_GRUMPKIN, shape, key)`` folds.  ``field_id`` reports the field."""
        return cls._wrap(cls._create(_lib.load().lurk_hip_r1cs_create_for_curve, curve, num_cons, num_vars, num_io, (A, B, C)))

    @classmethod
    def _wrap(cls, handle) -> "R1CSShape":
        """An R1CSShape around a handle the library created."""
        self = cls.__new__(cls)
        self._h, self._keep = handle, None
        f, dims = ctypes.c_int(), [ctypes.c_size_t() for _ in range(3)]
        _lib.check(_lib.load().lurk_hip_r1cs_dims(handle, ctypes.byref(f), *[ctypes.byref(x) for x in dims]))
        self.field_id, (self.num_cons, self.num_vars, self.num_io) = f.value, [x.value for x in dims]
        return self

    @classmethod
    def for_frames(cls, field_id: int, num_frames: int, counts5, first: int, frame_len: int, num_vars: int, num_io: int, extra=None) -> "R1CSShape":
        """The slot rows of a MultiFrame at the layout ``lurk_hip_frames_witness_dev`` writes (``lurk_hip_frames_r1cs_create``): counts5 per
        frame in (hash4, hash6, hash8, commitment, bit_decomp) order, ONE at column num_vars.  extra = (A, B, C) CSR triples of the caller's
        further rows over the same columns, appended after the slot rows.  The slot rows' order relative to the rest of lurk-beta's real
        circuit is unpinned: for checking, benchmarking and cross-checking a host's own shape."""
        counts = (ctypes.c_size_t * 5)(*[int(c) for c in counts5])
        keep, args, extra_cons = [], [None] * 9, 0
        if extra is not None:
            extra_cons = len(extra[0][0]) - 1
            args = []
            for indptr, indices, data in extra:
                ip = np.ascontiguousarray(indptr, dtype=np.uint64)
                ix = np.ascontiguousarray(indices, dtype=np.uint64)
                dv = np.ascontiguousarray(data, dtype=np.uint64)
                if ip.size != extra_cons + 1 or ix.size * 4 != dv.size:
                    raise ValueError("malformed CSR matrix")
                keep += [ip, ix, dv]
                args += [_lib.ptr(ip), _lib.ptr(ix), _lib.ptr(dv)]
        h = ctypes.c_void_p()
        _lib.check(_lib.load().lurk_hip_frames_r1cs_create(ctypes.byref(h), field_id, num_frames, counts, first, frame_len, num_vars, num_io, extra_cons,
                                                           *[a if a is not None else _lib.ptr(None) for a in args]))
        return cls._wrap(h)

    def is_sat(self, d_z, d_e=None, stream=None):
        """(n_unsat, first_unsat) of A z o B z == u C z + E, u = z[num_vars]; d_e None: E = 0 (R1CSShape::is_sat / is_sat_relaxed).
        first_unsat is num_cons when every row holds.  Synchronises the stream."""
        import torch

        assert d_z.is_cuda and d_z.shape[0] == self.num_cols and (d_e is None or (d_e.is_cuda and d_e.shape[0] == self.num_cons))
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        n, first = ctypes.c_uint64(), ctypes.c_uint64()
        _lib.check(_lib.load().lurk_hip_r1cs_is_sat_dev(self._h, _lib.ptr(d_z), _lib.ptr(d_e), ctypes.byref(n), ctypes.byref(first), _lib.ptr(s)))
        return n.value, first.value

    def sparse_mle(self, d_eq_x, d_eq_y, stream=None) -> np.ndarray:
        """(A~, B~, C~) as a (3, 4) Montgomery array: M~ = sum_i eq_x[i] sum_{k in row i} val[k] eq_y[col[k]] in one launch over the shape
        (lurk_hip_r1cs_sparse_mle_dev: the matrices' multilinear extensions at (r_x, r_y) when the tables are eq(r_x), eq(r_y), or their
        leading parts).  d_eq_x: >= num_cons elements, d_eq_y: more than the largest column.  Synchronises the stream."""
        import torch

        assert d_eq_x.is_cuda and d_eq_y.is_cuda and d_eq_x.is_contiguous() and d_eq_y.is_contiguous()
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        out = np.zeros((3, 4), dtype=np.uint64)
        _lib.check(_lib.load().lurk_hip_r1cs_sparse_mle_dev(self._h, _lib.ptr(d_eq_x), d_eq_x.shape[0], _lib.ptr(d_eq_y), d_eq_y.shape[0], _lib.ptr(out), _lib.ptr(s)))
        return out

    @property
    def num_cols(self) -> int:
        return self.num_vars + 1 + self.num_io

    def info(self) -> dict:
        v = [ctypes.c_size_t() for _ in range(4)]
        _lib.check(_lib.load().lurk_hip_r1cs_info(self._h, *[ctypes.byref(x) for x in v]))
        return {"nnz": (v[0].value, v[1].value, v[2].value), "distinct_coefficients": v[3].value}

    def read(self, which: int):
        """Matrix ``which`` (0 = A, 1 = B, 2 = C) back on the host as the CSR the constructor takes: (indptr, indices, data[(nnz, 4) u64
        Montgomery]) - ``lurk_hip_r1cs_read``.  Synchronises the device."""
        which = int(which)
        nnz = self.info()["nnz"][which] if 0 <= which <= 2 else 0
        indptr = np.zeros(self.num_cons + 1, dtype=np.uint64)
        indices = np.zeros(nnz, dtype=np.uint64)
        data = np.zeros((nnz, 4), dtype=np.uint64)
        _lib.check(_lib.load().lurk_hip_r1cs_read(self._h, which, _lib.ptr(indptr), _lib.ptr(indices) if nnz else None, _lib.ptr(data) if nnz else None))
        return indptr, indices, data

    def transposed(self, rows: int = 0, stream=None) -> "R1CSShape":
        """The transpose as a resident shape of ``rows`` rows (0: num_vars + 1 + num_io) over num_cons columns, made on the device from
        this shape's resident matrices and sharing their coefficients - ``lurk_hip_r1cs_transpose_dev``.  The compressing provers take
        ``transposed(2 * num_vars)`` as their shape_t.  Synchronises the stream once."""
        import torch

        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        h = ctypes.c_void_p()
        _lib.check(_lib.load().lurk_hip_r1cs_transpose_dev(self._h, int(rows), ctypes.byref(h), _lib.ptr(s)))
        return R1CSShape._wrap(h)

    def multiply_vec(self, d_z, stream=None):
        """(A z, B z, C z) - R1CSShape::multiply_vec."""
        import torch

        assert d_z.is_cuda and d_z.shape[0] == self.num_cols
        out = [torch.empty((self.num_cons, 4), dtype=torch.int64, device=d_z.device) for _ in range(3)]
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.load().lurk_hip_r1cs_multiply_vec_dev(self._h, _lib.ptr(d_z), *[_lib.ptr(o) for o in out], _lib.ptr(s)))
        return out

    def cross_term(self, d_z1, d_z2, out=None, stream=None):
        """T = AZ1 o BZ2 + AZ2 o BZ1 - u1 CZ2 - u2 CZ1 - the vector R1CSShape::commit_T commits to."""
        import torch

        assert d_z1.is_cuda and d_z2.is_cuda and d_z1.shape[0] == self.num_cols and d_z2.shape[0] == self.num_cols
        if out is None:
            out = torch.empty((self.num_cons, 4), dtype=torch.int64, device=d_z1.device)
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.load().lurk_hip_r1cs_cross_term_dev(self._h, _lib.ptr(d_z1), _lib.ptr(d_z2), _lib.ptr(out), _lib.ptr(s)))
        return out

    def cross_term_cached(self, d_z2, d_abc1, u1_mont, prev=None, r_prev_mont=None, stream=None):
        """The same T from the running instance's cached products (A z1, B z1, C z1) and z2 alone; u1_mont: the running u (4 x u64, host).
        prev = [A z2, B z2, C z2] of the previous step with its challenge r_prev_mont: folded into the cache IN PLACE by the same launch.
        Returns (T, [A z2, B z2, C z2]) - ``lurk_hip_r1cs_cross_term_cached_dev``."""
        import torch

        assert d_z2.is_cuda and d_z2.shape[0] == self.num_cols and len(d_abc1) == 3
        t = torch.empty((self.num_cons, 4), dtype=torch.int64, device=d_z2.device)
        abc2 = [torch.empty_like(t) for _ in range(3)]
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        u1 = np.ascontiguousarray(u1_mont, dtype=np.uint64).reshape(4)
        rp = None if r_prev_mont is None else np.ascontiguousarray(r_prev_mont, dtype=np.uint64).reshape(4)
        pv = [None, None, None] if prev is None else list(prev)
        _lib.check(_lib.load().lurk_hip_r1cs_cross_term_cached_dev(self._h, _lib.ptr(d_z2), *[_lib.ptr(x) for x in d_abc1], _lib.ptr(u1), *[_lib.ptr(x) for x in pv],
                                                                  _lib.ptr(rp), _lib.ptr(t), *[_lib.ptr(x) for x in abc2], _lib.ptr(s)))
        return t, abc2

    def close(self):
        if self._h:
            _lib.check(_lib.load().lurk_hip_r1cs_destroy(self._h))
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def fold_vec(field_id: int, d_a, d_b, r_mont: np.ndarray, out=None, stream=None):
    """a + r b element-wise (RelaxedR1CSWitness::fold: W1 + r W2, E1 + r T); r = 4 x u64 Montgomery."""
    import torch

    n = d_a.shape[0]
    assert d_a.is_cuda and d_b.is_cuda and d_b.shape[0] == n
    if out is None:
        out = torch.empty_like(d_a)
    r = np.ascontiguousarray(r_mont, dtype=np.uint64).reshape(4)
    s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    _lib.check(_lib.load().lurk_hip_fold_vec_dev(field_id, _lib.ptr(d_a), _lib.ptr(d_b), _lib.ptr(r), n, _lib.ptr(out), _lib.ptr(s)))
    return out


def fold_vecs(field_id: int, pairs, r_mont: np.ndarray, outs=None, stream=None):
    """Several folds a_k + r b_k under one r in ONE launch (``lurk_hip_fold_vecs_dev``, at most 8): pairs = [(d_a, d_b), ...];
    outs[k] may be d_a (in place).  Returns the outputs."""
    import torch

    n = len(pairs)
    if outs is None:
        outs = [torch.empty_like(a) for a, _ in pairs]
    r = np.ascontiguousarray(r_mont, dtype=np.uint64).reshape(4)
    s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    pa = (ctypes.c_void_p * max(n, 1))(*[_lib.ptr(a) for a, _ in pairs])
    pb = (ctypes.c_void_p * max(n, 1))(*[_lib.ptr(b) for _, b in pairs])
    po = (ctypes.c_void_p * max(n, 1))(*[_lib.ptr(o) for o in outs])
    ns = (ctypes.c_size_t * max(n, 1))(*[a.shape[0] for a, _ in pairs])
    _lib.check(_lib.load().lurk_hip_fold_vecs_dev(field_id, n, pa, pb, ns, po, _lib.ptr(r), _lib.ptr(s)))
    return outs


def fold_padded(field_id: int, vecs, coeffs_mont: np.ndarray, n_out: int, out=None, lens=None, stream=None):
    """out[j] = sum_k c_k (j < len_k ? vecs[k][j] : 0) for j < n_out in ONE launch (``lurk_hip_fold_padded_dev``): vectors of different
    lengths read as if zero-padded to n_out.  vecs: (len_k, 4) device tensors, or None for a zero-length vector; coeffs: (count, 4)
    Montgomery.  ``lens`` overrides the tensors' lengths; ``out`` an (n_out, 4) device tensor to write.  Returns the output."""
    import torch

    n = len(vecs)
    if lens is None:
        lens = [0 if v is None else v.shape[0] for v in vecs]
    if out is None:
        out = torch.empty((n_out, 4), dtype=torch.int64, device="cuda")
    c = np.ascontiguousarray(coeffs_mont, dtype=np.uint64).reshape(-1, 4)
    s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    pv = (ctypes.c_void_p * max(n, 1))(*[_lib.ptr(v) for v in vecs])
    ln = (ctypes.c_size_t * max(n, 1))(*lens)
    _lib.check(_lib.load().lurk_hip_fold_padded_dev(field_id, n, pv, ln, _lib.ptr(c), n_out, _lib.ptr(out), _lib.ptr(s)))
    return out
