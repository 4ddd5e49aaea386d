//! Bindings of `include/lurk_hip.h` (module [`ffi`], generated) and the safe wrappers a lurk-beta / arecibo build would use:
//!
//! * [`pasta_msm`]: the API of the `pasta-msm` crate (`pallas(points, scalars)`, `vesta(..)`, and the resident-key form
//!   `init` / `with` of the argumentcomputer fork) over `mult_pippenger_*` / `lurk_hip_msm_ctx_*` - what arecibo's
//!   `DlogGroup::vartime_multiscalar_mul` calls from `CommitmentEngine::commit`
//!   (callers in lurk-beta: `/root/reference/src/proof/nova.rs:287-293`, `supernova.rs:231-244`);
//! * [`FoldingContext`]: one curve's half of `RecursiveSNARK::prove_step` (`NIFS::prove`) with the running pair resident in HBM;
//! * [`poseidon`]: batched `PoseidonCache::hash{3,4,6,8}` (`/root/reference/src/hash.rs:180-204`);
//! * [`store`]: `HipPoseidonCache` (the shape of `PoseidonCache<F>`), `HipStoreHasher` (the shape of `StoreHasher`,
//!   `/root/reference/src/lem/store_core.rs:10-14`, layouts of `/root/reference/src/lem/store.rs:29-78`) and `hydrate`
//!   (`hydrate_z_cache`, `store_core.rs:256-269`, as one level-batched call);
//! * [`hyperkzg`]: the opening argument of the BN254 cycle (`EE1` of `Bn256EngineKZG`, `/root/reference/src/proof/nova.rs:65-71`): the prover
//!   with the polynomial resident, the verifier up to the pairing (the pairing stays with the caller);
//! * [`params`]: the run-time parameter blocks of the two restatements written from memory - Nova's random oracle
//!   (`lurk_hip_ro_params`) and `from_label` (`lurk_hip_ck_params`) - so that the first run beside arecibo can move one field at a time
//!   without rebuilding the library (callers: `/root/reference/src/proof/nova.rs:196-216, 282-295`);
//! * [`dump`]: LURKDUMP writers - `R1CSShape`, the fresh witnesses of consecutive steps and the `CommitmentKey` as the files
//!   `bench.py --workload fold_step --shape-file .. --witness-file ..` measures (`/root/reference/benches/fibonacci.rs:98-122`).
//!
//! Never compiled in the container this repository is built in (no Rust toolchain); the extern block cannot drift from the header
//! (see `rust/gen_sys.py`), the wrappers are a reading aid for the maintainer who wires the feature in.
pub mod dump;
pub mod ffi;
pub mod hyperkzg;
pub mod params;
pub mod spartan_kzg;
pub mod store;
pub mod trie;
pub use ffi::*;

use core::ffi::{c_int, c_void};
use std::ffi::CStr;

/// A non-zero return code of the library with `lurk_hip_last_error()`'s message.
#[derive(Debug, Clone)]
pub struct Error {
    pub code: c_int,
    pub message: String,
}
impl std::fmt::Display for Error {
    fn fmt(&self, f: &mut std::fmt::Formatter<'_>) -> std::fmt::Result {
        write!(f, "lurk_hip error {}: {}", self.code, self.message)
    }
}
impl std::error::Error for Error {}

pub fn check(rc: c_int) -> Result<(), Error> {
    if rc == LURK_HIP_OK {
        return Ok(());
    }
    // SAFETY: the library returns a pointer to a thread-local, NUL-terminated buffer that lives until the next call on this thread
    let message = unsafe { CStr::from_ptr(lurk_hip_last_error()) }.to_string_lossy().into_owned();
    Err(Error { code: rc, message })
}

/// The `pasta-msm` crate's surface.  `pasta_curves` with `repr-c` lays `Affine` out as 64 bytes and `Point` as 96 bytes of
/// Montgomery limbs, which is what the C ABI reads and writes; scalars are handed over in Montgomery form (`is_mont = true`),
/// as pasta-msm does.
pub mod pasta_msm {
    use super::*;
    use pasta_curves::{pallas, vesta};

    macro_rules! curve_mod {
        ($m:ident, $curve_id:expr, $oneshot:ident, $ctx:ident) => {
            /// `pasta_msm::$m(points, scalars)`: everything in host memory, result on return (aborts with the library's message on
            /// failure, as the C symbol of pasta-msm does).
            pub fn $m(points: &[$m::Affine], scalars: &[$m::Scalar]) -> $m::Point {
                let n = points.len().min(scalars.len());
                let mut out = $m::Point::default();
                #[cfg(feature = "oneshot-key-cache")]
                unsafe {
                    lurk_hip_msm_oneshot_key_cache(1);
                }
                // SAFETY: both slices hold at least n elements of the layouts named above; out is 96 writable bytes
                unsafe { $oneshot((&mut out as *mut $m::Point).cast(), points.as_ptr().cast(), n, scalars.as_ptr().cast(), true) };
                out
            }

            /// A commitment key resident in HBM (`CommitmentKey` is constant for a whole proof, `/root/reference/src/proof/nova.rs:196-216`):
            /// `init(points)` / `with(&ctx, scalars)` of the argumentcomputer pasta-msm fork.
            pub struct $ctx(*mut lurk_hip_msm_ctx);
            // SAFETY: every entry point of the library is thread-safe and a handle records its device
            unsafe impl Send for $ctx {}
            unsafe impl Sync for $ctx {}
            impl $ctx {
                pub fn init(points: &[$m::Affine], precompute: bool) -> Result<Self, Error> {
                    let mut p = core::ptr::null_mut();
                    let flags = if precompute { LURK_MSM_FLAG_PRECOMPUTE } else { 0 };
                    check(unsafe { lurk_hip_msm_ctx_create(&mut p, $curve_id, points.as_ptr().cast(), points.len(), flags) })?;
                    Ok(Self(p))
                }
                /// `CE::commit(ck, v)`: MSM over `ck[..v.len()]`
                pub fn with(&self, scalars: &[$m::Scalar]) -> Result<$m::Point, Error> {
                    let mut out = $m::Point::default();
                    check(unsafe { lurk_hip_msm_ctx_run(self.0, (&mut out as *mut $m::Point).cast(), scalars.as_ptr().cast(), scalars.len(), 1) })?;
                    Ok(out)
                }
                /// Scalars already in device memory (e.g. a witness assembled by `lurk_hip_frames_witness_dev`); up to
                /// `LURK_MSM_SLOTS` commitments in flight: `submit` then `wait` on the same slot.
                ///
                /// # Safety
                /// `d_scalars` must point to `n` 32-byte Montgomery scalars in device memory that stay valid until `wait`.
                pub unsafe fn submit(&self, slot: c_int, d_scalars: *const c_void, n: usize, stream: *mut c_void, mode: c_int) -> Result<(), Error> {
                    check(lurk_hip_msm_ctx_submit_dev_mode(self.0, slot, d_scalars, n, 1, stream, mode))
                }
                pub fn wait(&self, slot: c_int) -> Result<$m::Point, Error> {
                    let mut out = $m::Point::default();
                    check(unsafe { lurk_hip_msm_ctx_wait(self.0, slot, (&mut out as *mut $m::Point).cast()) })?;
                    Ok(out)
                }
                /// `lens.len()` short commitments under prefixes of the key in one pass: vector k is the `lens[k]` scalars at element
                /// `offsets[k]` of `d_scalars` and commits to the first `lens[k]` bases.  Window-table keys only, at most
                /// `LURK_MSM_BATCH_MAX_VECTORS` vectors; `wait_batch(slot, lens.len())` on the same slot.
                ///
                /// # Safety
                /// `d_scalars` must point to 32-byte Montgomery scalars in device memory that cover every `offsets[k] + lens[k]` and stay
                /// valid until `wait_batch`.
                pub unsafe fn submit_batch(&self, slot: c_int, d_scalars: *const c_void, offsets: &[usize], lens: &[usize], stream: *mut c_void) -> Result<(), Error> {
                    if offsets.len() != lens.len() {
                        return Err(Error { code: LURK_HIP_ERR_INVALID_ARG, message: "batch: offsets and lens differ in length".into() });
                    }
                    check(lurk_hip_msm_ctx_submit_batch_dev(self.0, slot, d_scalars, offsets.as_ptr(), lens.as_ptr(), lens.len(), 1, stream))
                }
                /// The `count` commitments of the batch submitted on `slot`, each the point `wait` gives for that vector.
                ///
                /// # Safety
                /// `count` must be the number of vectors submitted on `slot`: the library writes that many points.
                pub unsafe fn wait_batch(&self, slot: c_int, count: usize) -> Result<Vec<$m::Point>, Error> {
                    let mut out = vec![$m::Point::default(); count.max(1)];
                    check(lurk_hip_msm_ctx_wait_batch(self.0, slot, out.as_mut_ptr().cast()))?;
                    out.truncate(count);
                    Ok(out)
                }
                /// The key folded by the weights of k inner-product rounds at once (`ck_k[p] = sum_b w_b * ck[b m + p]`, arecibo `ipa_pc`):
                /// `weights` are Montgomery scalars (a power of two of them, at most 2^12), the `n / weights.len()` affine points land in
                /// device memory.  Window-table keys only; `lurk_hip_ipa_prove_dev` calls this by itself.
                ///
                /// # Safety
                /// `d_out` must point to `n / weights.len()` 64-byte records of device memory.
                pub unsafe fn fold_key(&self, n: usize, weights: &[$m::Scalar], d_out: *mut c_void, stream: *mut c_void) -> Result<(), Error> {
                    check(lurk_hip_msm_ctx_fold_key_dev(self.0, n, weights.as_ptr().cast(), weights.len(), d_out, stream))
                }
                pub fn as_ptr(&self) -> *mut lurk_hip_msm_ctx {
                    self.0
                }
            }
            impl Drop for $ctx {
                fn drop(&mut self) {
                    unsafe { lurk_hip_msm_ctx_destroy(self.0) };
                }
            }
        };
    }
    curve_mod!(pallas, LURK_CURVE_PALLAS, mult_pippenger_pallas, MSMContextPallas);
    curve_mod!(vesta, LURK_CURVE_VESTA, mult_pippenger_vesta, MSMContextVesta);
}

/// The `grumpkin-msm` crate's surface (arecibo's MSM crate for the BN254 / Grumpkin cycle, lurk-beta's default): `bn256(points,
/// scalars)` and `grumpkin(points, scalars)` over `mult_pippenger_bn254` / `mult_pippenger_grumpkin`, and a resident key per curve.
/// `halo2curves` with `repr-c` lays `G1Affine` out as 64 bytes and `G1` as 96 bytes of Montgomery limbs (recalled, unpinned - as the
/// symbol names are); scalars are handed over in Montgomery form.  Behind the cargo feature `grumpkin` (it brings in `halo2curves`).
#[cfg(feature = "grumpkin")]
pub mod grumpkin_msm {
    use super::*;
    use halo2curves::{bn256, grumpkin};

    macro_rules! curve_fn {
        ($f:ident, $m:ident, $curve_id:expr, $oneshot:ident, $ctx:ident) => {
            pub fn $f(points: &[$m::G1Affine], scalars: &[$m::Fr]) -> $m::G1 {
                let n = points.len().min(scalars.len());
                let mut out = $m::G1::default();
                // SAFETY: both slices hold at least n elements of the layouts named above; out is 96 writable bytes
                unsafe { $oneshot((&mut out as *mut $m::G1).cast(), points.as_ptr().cast(), n, scalars.as_ptr().cast(), true) };
                out
            }
            /// A commitment key resident in HBM: `init(points)` / `with(&ctx, scalars)`.
            pub struct $ctx(*mut lurk_hip_msm_ctx);
            // SAFETY: every entry point of the library is thread-safe and a handle records its device
            unsafe impl Send for $ctx {}
            unsafe impl Sync for $ctx {}
            impl $ctx {
                pub fn init(points: &[$m::G1Affine], precompute: bool) -> Result<Self, Error> {
                    let mut p = core::ptr::null_mut();
                    let flags = if precompute { LURK_MSM_FLAG_PRECOMPUTE } else { 0 };
                    check(unsafe { lurk_hip_msm_ctx_create(&mut p, $curve_id, points.as_ptr().cast(), points.len(), flags) })?;
                    Ok(Self(p))
                }
                pub fn with(&self, scalars: &[$m::Fr]) -> Result<$m::G1, Error> {
                    let mut out = $m::G1::default();
                    check(unsafe { lurk_hip_msm_ctx_run(self.0, (&mut out as *mut $m::G1).cast(), scalars.as_ptr().cast(), scalars.len(), 1) })?;
                    Ok(out)
                }
                pub fn as_ptr(&self) -> *mut lurk_hip_msm_ctx {
                    self.0
                }
            }
            impl Drop for $ctx {
                fn drop(&mut self) {
                    unsafe { lurk_hip_msm_ctx_destroy(self.0) };
                }
            }
        };
    }
    curve_fn!(bn256, bn256, LURK_CURVE_BN254, mult_pippenger_bn254, MSMContextBn256);
    curve_fn!(grumpkin, grumpkin, LURK_CURVE_GRUMPKIN, mult_pippenger_grumpkin, MSMContextGrumpkin);
}

/// An R1CS shape resident in HBM (arecibo `R1CSShape { A, B, C }` in CSR form, coefficients in Montgomery form).
pub struct R1csShape(*mut lurk_hip_r1cs);
unsafe impl Send for R1csShape {}
unsafe impl Sync for R1csShape {}
/// One sparse matrix as arecibo's `SparseMatrix { data, indices, indptr }` holds it.
pub struct Csr<'a> {
    pub indptr: &'a [u64],
    pub indices: &'a [u64],
    /// `indices.len()` field elements of 32 bytes, Montgomery form
    pub data: &'a [u8],
}
impl R1csShape {
    pub fn new(field_id: c_int, num_cons: usize, num_vars: usize, num_io: usize, a: Csr, b: Csr, c: Csr) -> Result<Self, Error> {
        let mut p = core::ptr::null_mut();
        check(unsafe {
            lurk_hip_r1cs_create(&mut p, field_id, num_cons, num_vars, num_io, a.indptr.as_ptr(), a.indices.as_ptr(), a.data.as_ptr().cast(),
                                 b.indptr.as_ptr(), b.indices.as_ptr(), b.data.as_ptr().cast(), c.indptr.as_ptr(), c.indices.as_ptr(),
                                 c.data.as_ptr().cast())
        })?;
        Ok(Self(p))
    }
    /// The same shape over the SCALAR field of `curve` (`lurk_hip_r1cs_create_for_curve`): the one way to a shape over the BN254 base
    /// field, Grumpkin's scalar field, which `FoldingContext::new(LURK_CURVE_GRUMPKIN, ..)` folds.
    pub fn for_curve(curve: c_int, num_cons: usize, num_vars: usize, num_io: usize, a: Csr, b: Csr, c: Csr) -> Result<Self, Error> {
        let mut p = core::ptr::null_mut();
        check(unsafe {
            lurk_hip_r1cs_create_for_curve(&mut p, curve, num_cons, num_vars, num_io, a.indptr.as_ptr(), a.indices.as_ptr(), a.data.as_ptr().cast(),
                                           b.indptr.as_ptr(), b.indices.as_ptr(), b.data.as_ptr().cast(), c.indptr.as_ptr(), c.indices.as_ptr(),
                                           c.data.as_ptr().cast())
        })?;
        Ok(Self(p))
    }
    /// The slot rows of a MultiFrame at the layout `lurk_hip_frames_witness_dev` writes (`lurk_hip_frames_r1cs_create`): `counts5` per frame
    /// in (hash4, hash6, hash8, commitment, bit_decomp) order, ONE at column `num_vars`; `extra` = the caller's further rows (A, B, C over the
    /// same columns), appended after the slot rows.  The slot rows' order relative to the rest of lurk-beta's real circuit is unpinned: for
    /// checking, benchmarking and cross-checking a host's own shape.
    #[allow(clippy::too_many_arguments)]
    pub fn for_frames(field_id: c_int, num_frames: usize, counts5: &[usize; 5], first: usize, frame_len: usize, num_vars: usize, num_io: usize,
                      extra: Option<(Csr, Csr, Csr)>) -> Result<Self, Error> {
        let mut p = core::ptr::null_mut();
        let null = core::ptr::null::<u64>();
        check(unsafe {
            match extra {
                Some((a, b, c)) => lurk_hip_frames_r1cs_create(&mut p, field_id, num_frames, counts5.as_ptr(), first, frame_len, num_vars, num_io, a.indptr.len().saturating_sub(1),
                                                               a.indptr.as_ptr(), a.indices.as_ptr(), a.data.as_ptr().cast(), b.indptr.as_ptr(), b.indices.as_ptr(),
                                                               b.data.as_ptr().cast(), c.indptr.as_ptr(), c.indices.as_ptr(), c.data.as_ptr().cast()),
                None => lurk_hip_frames_r1cs_create(&mut p, field_id, num_frames, counts5.as_ptr(), first, frame_len, num_vars, num_io, 0, null, null, null.cast(), null, null,
                                                    null.cast(), null, null, null.cast()),
            }
        })?;
        Ok(Self(p))
    }
    /// `R1CSShape::is_sat` / `is_sat_relaxed` on the device: (failing rows, lowest failing row - `num_cons` when none) of
    /// A z o B z == u C z + E; `d_e` null: E = 0.  Synchronises `stream`.
    /// # Safety
    /// `d_z`: `num_vars + 1 + num_io` Montgomery scalars in the current device's memory, `d_e`: `num_cons` of them or null.
    pub unsafe fn is_sat(&self, d_z: *const c_void, d_e: *const c_void, stream: *mut c_void) -> Result<(u64, u64), Error> {
        let (mut n, mut first) = (0u64, 0u64);
        check(lurk_hip_r1cs_is_sat_dev(self.0, d_z, d_e, &mut n, &mut first, stream))?;
        Ok((n, first))
    }
    /// The transpose as a resident shape of `rows_t` rows (0: `num_vars + 1 + num_io`) over `num_cons` columns, made on the device from this
    /// shape's resident matrices and sharing their coefficients (`lurk_hip_r1cs_transpose_dev`): the compressing provers take
    /// `transposed(2 * num_vars, stream)` as their `shape_t`, so no host CSR of the transpose is needed.  Synchronises `stream` once.
    /// # Safety
    /// `stream`: a stream of the device the shape is resident on (the calling thread's current device), or null.
    pub unsafe fn transposed(&self, rows_t: usize, stream: *mut c_void) -> Result<Self, Error> {
        let mut p = core::ptr::null_mut();
        check(lurk_hip_r1cs_transpose_dev(self.0, rows_t, &mut p, stream))?;
        Ok(Self(p))
    }
    /// (num_cons, num_vars, num_io)
    pub fn dims(&self) -> Result<(usize, usize, usize), Error> {
        let (mut f, mut c, mut v, mut io) = (0, 0usize, 0usize, 0usize);
        check(unsafe { lurk_hip_r1cs_dims(self.0, &mut f, &mut c, &mut v, &mut io) })?;
        Ok((c, v, io))
    }
    /// Matrix `which` (0 = A, 1 = B, 2 = C) back on the host as the CSR `new` takes (`lurk_hip_r1cs_read`): for cross-checking a host's own
    /// shape against one the library built (`for_frames`) or transposed.  Synchronises the device.
    pub fn read(&self, which: c_int) -> Result<SlotMatrix, Error> {
        let (rows, _, _) = self.dims()?;
        let mut nnz = [0usize; 3];
        let [na, nb, nc] = &mut nnz;
        check(unsafe { lurk_hip_r1cs_info(self.0, na, nb, nc, core::ptr::null_mut()) })?;
        let n = if (0..3).contains(&which) { nnz[which as usize] } else { 0 };
        let mut m = SlotMatrix { indptr: vec![0; rows + 1], indices: vec![0; n], data: vec![0; n * 32] };
        check(unsafe { lurk_hip_r1cs_read(self.0, which, m.indptr.as_mut_ptr(), m.indices.as_mut_ptr(), m.data.as_mut_ptr().cast()) })?;
        Ok(m)
    }
    pub fn as_ptr(&self) -> *mut lurk_hip_r1cs {
        self.0
    }
}
/// One sparse matrix, owned: of a slot's rows (`lurk_hip_slot_constraints`) or of a resident shape read back (`R1csShape::read`).
pub struct SlotMatrix {
    pub indptr: Vec<u64>,
    pub indices: Vec<u64>,
    pub data: Vec<u8>,
}
/// The constraint rows one slot's gadget enforces on its block: A, B, C; local column `size` is the constant ONE.  Host-only.
pub fn slot_constraints(field_id: c_int, slot_type: c_int) -> Result<[SlotMatrix; 3], Error> {
    let (mut rows, mut na, mut nb, mut nc) = (0usize, 0usize, 0usize, 0usize);
    check(unsafe { lurk_hip_slot_constraints_size(field_id, slot_type, &mut rows, &mut na, &mut nb, &mut nc) })?;
    let mk = |nnz: usize| SlotMatrix { indptr: vec![0; rows + 1], indices: vec![0; nnz], data: vec![0; nnz * 32] };
    let mut m = [mk(na), mk(nb), mk(nc)];
    let [a, b, c] = &mut m;
    check(unsafe {
        lurk_hip_slot_constraints(field_id, slot_type, a.indptr.as_mut_ptr(), a.indices.as_mut_ptr(), a.data.as_mut_ptr().cast(), b.indptr.as_mut_ptr(),
                                  b.indices.as_mut_ptr(), b.data.as_mut_ptr().cast(), c.indptr.as_mut_ptr(), c.indices.as_mut_ptr(), c.data.as_mut_ptr().cast())
    })?;
    Ok(m)
}
impl Drop for R1csShape {
    fn drop(&mut self) {
        unsafe { lurk_hip_r1cs_destroy(self.0) };
    }
}

/// The single-instance compressing prover as one call (`lurk_hip_spartan_prove_dev`): sum-checks, claim batching and the opening with the
/// Keccak transcript inside.  The protocol is the library's own, not arecibo's byte for byte.
pub struct SpartanProof {
    pub polys_outer: Vec<u8>,  // log2(num_cons) x 4 x 32 B, canonical
    pub claims_outer: [u8; 96],
    pub eval_e: [u8; 32],
    pub polys_inner: Vec<u8>,  // (log2(num_vars) + 1) x 3 x 32 B
    pub eval_w: [u8; 32],
    pub polys_batch: Vec<u8>,  // log2(N) x 3 x 32 B, N = max(num_cons, num_vars)
    pub evals_batch: [u8; 64],
    pub ipa_l: Vec<u8>,        // log2(N) x 96 B Jacobians
    pub ipa_r: Vec<u8>,
    pub ipa_a: [u8; 32],
}
/// # Safety
/// `d_w` / `d_e`: `num_vars` / `num_cons` Montgomery scalars in device memory; `shape_t` is the transpose of `shape` (2 `num_vars` rows over
/// `num_cons` columns); `key` holds at least max(`num_cons`, `num_vars`) points and committed W and E.
#[allow(clippy::too_many_arguments)]
pub unsafe fn spartan_prove(shape: &R1csShape, shape_t: &R1csShape, num_cons: usize, num_vars: usize, key: *mut lurk_hip_msm_ctx, ck_c: &[u8; 96], x: &[u8], u: &[u8; 32],
                            d_w: *const c_void, d_e: *const c_void, comm_w: &[u8; 96], comm_e: &[u8; 96], label: &[u8], stream: *mut c_void) -> Result<SpartanProof, Error> {
    let log2 = |n: usize| n.trailing_zeros() as usize;
    let (ell_x, ell_y, ell) = (log2(num_cons), log2(num_vars) + 1, log2(num_cons.max(num_vars)));
    let mut p = SpartanProof {
        polys_outer: vec![0; ell_x * 128], claims_outer: [0; 96], eval_e: [0; 32], polys_inner: vec![0; ell_y * 96], eval_w: [0; 32],
        polys_batch: vec![0; ell.max(1) * 96], evals_batch: [0; 64], ipa_l: vec![0; ell.max(1) * 96], ipa_r: vec![0; ell.max(1) * 96], ipa_a: [0; 32],
    };
    let mut out = lurk_hip_spartan_proof {
        polys_outer: p.polys_outer.as_mut_ptr().cast(), claims_outer: p.claims_outer.as_mut_ptr().cast(), eval_e: p.eval_e.as_mut_ptr().cast(),
        polys_inner: p.polys_inner.as_mut_ptr().cast(), eval_w: p.eval_w.as_mut_ptr().cast(), polys_batch: p.polys_batch.as_mut_ptr().cast(),
        evals_batch: p.evals_batch.as_mut_ptr().cast(), ipa_l: p.ipa_l.as_mut_ptr().cast(), ipa_r: p.ipa_r.as_mut_ptr().cast(), ipa_a: p.ipa_a.as_mut_ptr().cast(),
    };
    check(lurk_hip_spartan_prove_dev(shape.as_ptr(), shape_t.as_ptr(), num_cons, num_vars, x.len() / 32, key, ck_c.as_ptr().cast(), x.as_ptr().cast(), u.as_ptr().cast(),
                                     d_w, d_e, comm_w.as_ptr().cast(), comm_e.as_ptr().cast(), label.as_ptr().cast(), label.len(), &mut out, stream))?;
    Ok(p)
}

/// The batched compressing prover as one call (`lurk_hip_spartan_prove_batch_dev`): n relaxed instances of different shapes under one key,
/// one proof - the structure of arecibo's `BatchedRelaxedR1CSSNARK`, SuperNova's compressor (`/root/reference/src/proof/supernova.rs:110,
/// 293-302`).  Sizes of the outputs: `include/lurk_hip.h`.
pub struct SpartanBatchProof {
    pub polys_outer: Vec<u8>,   // log2(max num_cons) x 4 x 32 B, canonical
    pub claims_outer: Vec<u8>,  // n x 3 x 32 B
    pub evals_e: Vec<u8>,       // n x 32 B
    pub polys_inner: Vec<u8>,   // (log2(max num_vars) + 1) x 3 x 32 B
    pub evals_w: Vec<u8>,       // n x 32 B
    pub polys_batch: Vec<u8>,   // log2(N) x 3 x 32 B
    pub evals_batch: Vec<u8>,   // 2 n x 32 B
    pub ipa_l: Vec<u8>,         // log2(N) x 96 B Jacobians
    pub ipa_r: Vec<u8>,
    pub ipa_a: [u8; 32],
}
/// # Safety
/// Every instance's pointers obey the contract of [`spartan_prove`]; `key` holds at least max(`num_cons`, `num_vars`) points over all instances.
pub unsafe fn spartan_prove_batch(instances: &[lurk_hip_spartan_instance], key: *mut lurk_hip_msm_ctx, ck_c: &[u8; 96], label: &[u8], stream: *mut c_void)
                                  -> Result<SpartanBatchProof, Error> {
    let log2 = |n: usize| n.trailing_zeros() as usize;
    let n = instances.len();
    let max_nc = instances.iter().map(|i| i.num_cons).max().unwrap_or(2);
    let max_nv = instances.iter().map(|i| i.num_vars).max().unwrap_or(2);
    let (ell_x, ell_y, ell) = (log2(max_nc), log2(max_nv) + 1, log2(max_nc.max(max_nv)));
    let mut p = SpartanBatchProof {
        polys_outer: vec![0; ell_x * 128], claims_outer: vec![0; n * 96], evals_e: vec![0; n * 32], polys_inner: vec![0; ell_y * 96], evals_w: vec![0; n * 32],
        polys_batch: vec![0; ell.max(1) * 96], evals_batch: vec![0; 2 * n * 32], ipa_l: vec![0; ell.max(1) * 96], ipa_r: vec![0; ell.max(1) * 96], ipa_a: [0; 32],
    };
    let mut out = lurk_hip_spartan_batch_proof {
        polys_outer: p.polys_outer.as_mut_ptr().cast(), claims_outer: p.claims_outer.as_mut_ptr().cast(), evals_e: p.evals_e.as_mut_ptr().cast(),
        polys_inner: p.polys_inner.as_mut_ptr().cast(), evals_w: p.evals_w.as_mut_ptr().cast(), polys_batch: p.polys_batch.as_mut_ptr().cast(),
        evals_batch: p.evals_batch.as_mut_ptr().cast(), ipa_l: p.ipa_l.as_mut_ptr().cast(), ipa_r: p.ipa_r.as_mut_ptr().cast(), ipa_a: p.ipa_a.as_mut_ptr().cast(),
    };
    check(lurk_hip_spartan_prove_batch_dev(instances.as_ptr(), n, key, ck_c.as_ptr().cast(), label.as_ptr().cast(), label.len(), &mut out, stream))?;
    Ok(p)
}

/// The answer of a verification (`lurk_hip_spartan_verify_dev` / `_verify_batch_dev`): a proof that does not verify is a successful call.
/// `failed_check` is one of `LURK_VERIFY_*` (0 = accepted, 1 malformed input, 2 outer / 3 inner / 4 batching sum-check, 5 the opening).
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct Verdict {
    pub accepted: bool,
    pub failed_check: c_int,
}
/// The verifier of [`spartan_prove`]'s proof: the same statement without the witness and without the transposed shape.
/// # Safety
/// `key` holds at least max(`num_cons`, `num_vars`) points and is the key that committed W and E.
#[allow(clippy::too_many_arguments)]
pub unsafe fn spartan_verify(shape: &R1csShape, num_cons: usize, num_vars: usize, key: *mut lurk_hip_msm_ctx, ck_c: &[u8; 96], x: &[u8], u: &[u8; 32], comm_w: &[u8; 96],
                             comm_e: &[u8; 96], label: &[u8], proof: &SpartanProof, stream: *mut c_void) -> Result<Verdict, Error> {
    let log2 = |n: usize| n.trailing_zeros() as usize;
    let (ell_x, ell_y, ell) = (log2(num_cons), log2(num_vars) + 1, log2(num_cons.max(num_vars)));
    if proof.polys_outer.len() != ell_x * 128 || proof.polys_inner.len() != ell_y * 96 || proof.polys_batch.len() < ell * 96 || proof.ipa_l.len() < ell * 96
        || proof.ipa_r.len() < ell * 96 || x.len() % 32 != 0 {
        return Ok(Verdict { accepted: false, failed_check: LURK_VERIFY_MALFORMED });
    }
    // (the library only reads through these pointers)
    let pf = lurk_hip_spartan_proof {
        polys_outer: proof.polys_outer.as_ptr() as *mut c_void, claims_outer: proof.claims_outer.as_ptr() as *mut c_void, eval_e: proof.eval_e.as_ptr() as *mut c_void,
        polys_inner: proof.polys_inner.as_ptr() as *mut c_void, eval_w: proof.eval_w.as_ptr() as *mut c_void, polys_batch: proof.polys_batch.as_ptr() as *mut c_void,
        evals_batch: proof.evals_batch.as_ptr() as *mut c_void, ipa_l: proof.ipa_l.as_ptr() as *mut c_void, ipa_r: proof.ipa_r.as_ptr() as *mut c_void,
        ipa_a: proof.ipa_a.as_ptr() as *mut c_void,
    };
    let (mut accepted, mut failed): (c_int, c_int) = (0, 0);
    check(lurk_hip_spartan_verify_dev(shape.as_ptr(), num_cons, num_vars, x.len() / 32, key, ck_c.as_ptr().cast(), x.as_ptr().cast(), u.as_ptr().cast(),
                                      comm_w.as_ptr().cast(), comm_e.as_ptr().cast(), label.as_ptr().cast(), label.len(), &pf, &mut accepted, &mut failed, stream))?;
    Ok(Verdict { accepted: accepted != 0, failed_check: failed })
}
/// The verifier of [`spartan_prove_batch`]'s proof; of an instance `shape_t`, `d_w32_mont` and `d_e32_mont` are ignored (may be null).
/// # Safety
/// Every instance's shape, x, u and commitment pointers are valid; `key` as for [`spartan_verify`].
pub unsafe fn spartan_verify_batch(instances: &[lurk_hip_spartan_instance], key: *mut lurk_hip_msm_ctx, ck_c: &[u8; 96], label: &[u8], proof: &SpartanBatchProof,
                                   stream: *mut c_void) -> Result<Verdict, Error> {
    let log2 = |n: usize| n.trailing_zeros() as usize;
    let n = instances.len();
    let max_nc = instances.iter().map(|i| i.num_cons).max().unwrap_or(2);
    let max_nv = instances.iter().map(|i| i.num_vars).max().unwrap_or(2);
    let (ell_x, ell_y, ell) = (log2(max_nc), log2(max_nv) + 1, log2(max_nc.max(max_nv)));
    if proof.polys_outer.len() != ell_x * 128 || proof.claims_outer.len() != n * 96 || proof.evals_e.len() != n * 32 || proof.polys_inner.len() != ell_y * 96
        || proof.evals_w.len() != n * 32 || proof.polys_batch.len() < ell * 96 || proof.evals_batch.len() != 2 * n * 32 || proof.ipa_l.len() < ell * 96
        || proof.ipa_r.len() < ell * 96 {
        return Ok(Verdict { accepted: false, failed_check: LURK_VERIFY_MALFORMED });
    }
    let pf = lurk_hip_spartan_batch_proof {
        polys_outer: proof.polys_outer.as_ptr() as *mut c_void, claims_outer: proof.claims_outer.as_ptr() as *mut c_void, evals_e: proof.evals_e.as_ptr() as *mut c_void,
        polys_inner: proof.polys_inner.as_ptr() as *mut c_void, evals_w: proof.evals_w.as_ptr() as *mut c_void, polys_batch: proof.polys_batch.as_ptr() as *mut c_void,
        evals_batch: proof.evals_batch.as_ptr() as *mut c_void, ipa_l: proof.ipa_l.as_ptr() as *mut c_void, ipa_r: proof.ipa_r.as_ptr() as *mut c_void,
        ipa_a: proof.ipa_a.as_ptr() as *mut c_void,
    };
    let (mut accepted, mut failed): (c_int, c_int) = (0, 0);
    check(lurk_hip_spartan_verify_batch_dev(instances.as_ptr(), n, key, ck_c.as_ptr().cast(), label.as_ptr().cast(), label.len(), &pf, &mut accepted, &mut failed, stream))?;
    Ok(Verdict { accepted: accepted != 0, failed_check: failed })
}
/// `SumcheckProof::verify` on the host (`lurk_hip_sumcheck_verify`, no device needed): the final claim, or `None` when a round fails.
pub fn sumcheck_verify(field_id: c_int, degree: c_int, claim: &[u8; 32], polys: &[u8], challenges: &[u8]) -> Result<Option<[u8; 32]>, Error> {
    let rounds = challenges.len() / 32;
    if challenges.len() % 32 != 0 || degree < 2 || polys.len() != rounds * (degree as usize + 1) * 32 {
        return Ok(None);
    }
    let (mut out, mut ok): ([u8; 32], c_int) = ([0; 32], 0);
    check(unsafe { lurk_hip_sumcheck_verify(field_id, degree, rounds, claim.as_ptr().cast(), polys.as_ptr().cast(), challenges.as_ptr().cast(), out.as_mut_ptr().cast(), &mut ok) })?;
    Ok(if ok != 0 { Some(out) } else { None })
}

/// One curve's half of `RecursiveSNARK::prove_step`: the running relaxed pair (z1 = [W | u | X], E) and the running instance stay in
/// the context; `step` is `NIFS::prove` (commit W2, cross term, commit T, r from the transcript, fold).
/// Borrowing the shape and the key ties their lifetimes to the context's, as the C ABI requires.
pub struct FoldingContext<'a> {
    h: *mut lurk_hip_fold_ctx,
    num_io: usize,
    _shape: core::marker::PhantomData<&'a R1csShape>,
}
/// What a step returns: comm_W2, comm_T (96-byte Jacobians) and the challenge r (32 bytes, Montgomery).
pub struct StepOutput {
    pub comm_w2: [u8; 96],
    pub comm_t: [u8; 96],
    pub r: [u8; 32],
}
impl<'a> FoldingContext<'a> {
    pub fn new(curve: c_int, shape: &'a R1csShape, key: *mut lurk_hip_msm_ctx, num_io: usize) -> Result<Self, Error> {
        let mut h = core::ptr::null_mut();
        check(unsafe { lurk_hip_fold_ctx_create(&mut h, curve, shape.as_ptr(), key) })?;
        Ok(Self { h, num_io, _shape: core::marker::PhantomData })
    }
    /// `w2`: the fresh witness (host memory, Montgomery); `x2`: its public IO; `pp_digest`: 32 canonical bytes.
    pub fn step(&mut self, w2: &[u8], x2: &[u8], pp_digest: &[u8; 32]) -> Result<StepOutput, Error> {
        assert_eq!(x2.len(), 32 * self.num_io);
        let mut out = StepOutput { comm_w2: [0; 96], comm_t: [0; 96], r: [0; 32] };
        check(unsafe {
            lurk_hip_fold_step(self.h, w2.as_ptr().cast(), 0, core::ptr::null_mut(), x2.as_ptr().cast(), pp_digest.as_ptr().cast(),
                               out.comm_w2.as_mut_ptr().cast(), out.comm_t.as_mut_ptr().cast(), out.r.as_mut_ptr().cast())
        })?;
        Ok(out)
    }
    /// The two halves for a caller with its own transcript: `begin` returns (comm_W2, comm_T), `finish(r)` folds.
    pub fn begin(&mut self, w2: &[u8], x2: &[u8]) -> Result<([u8; 96], [u8; 96]), Error> {
        let (mut cw, mut ct) = ([0u8; 96], [0u8; 96]);
        check(unsafe {
            lurk_hip_fold_step_begin(self.h, w2.as_ptr().cast(), 0, core::ptr::null_mut(), x2.as_ptr().cast(), cw.as_mut_ptr().cast(),
                                     ct.as_mut_ptr().cast())
        })?;
        Ok((cw, ct))
    }
    pub fn finish(&mut self, r_mont: &[u8; 32]) -> Result<(), Error> {
        check(unsafe { lurk_hip_fold_step_finish(self.h, r_mont.as_ptr().cast()) })
    }
    /// The halves with the library's transcript: set the digest of the public parameters once; every `begin` then absorbs pp_digest and
    /// the running instance while the device works, and `challenge` finishes behind comm_T with one permutation (r in Montgomery form).
    pub fn set_pp_digest(&mut self, pp_digest: &[u8; 32]) -> Result<(), Error> {
        check(unsafe { lurk_hip_fold_ctx_set_pp_digest(self.h, pp_digest.as_ptr().cast()) })
    }
    pub fn challenge(&mut self) -> Result<[u8; 32], Error> {
        let mut r = [0u8; 32];
        check(unsafe { lurk_hip_fold_step_challenge(self.h, r.as_mut_ptr().cast()) })?;
        Ok(r)
    }
    /// A hook into every step: called once per `step` / `begin` / `begin_prefetched`, on the calling thread, after the step's device work
    /// has been enqueued and before the call blocks on the commitments - where the next witness's slot traces are enqueued
    /// (`lurk_hip_slot_witness_dev`), so that they run beside the step.  A non-zero return fails the step (it is rolled back).
    ///
    /// # Safety
    /// `hook` and `user` must stay valid until the hook is replaced, removed (`None`) or the context dropped; the hook must not call
    /// into this context.
    pub unsafe fn set_submit_hook(&mut self, hook: lurk_hip_fold_submit_hook_fn, user: *mut c_void) -> Result<(), Error> {
        check(lurk_hip_fold_ctx_set_submit_hook(self.h, hook, user))
    }
    /// Staging ahead across devices: `helper` is the same commitment key resident on another device; instances staged with
    /// `prefetch` are committed on the helpers in turn while this context's device folds.
    ///
    /// # Safety
    /// `helper` must outlive the context.
    pub unsafe fn add_helper(&mut self, helper: *mut lurk_hip_msm_ctx) -> Result<(), Error> {
        check(lurk_hip_fold_ctx_add_helper(self.h, helper))
    }
    /// Stage positions `[offset, offset + range.len() / 32)` of the next fresh witness (host memory, Montgomery) and start its commitment.
    pub fn prefetch(&mut self, range: &[u8], offset: usize) -> Result<(), Error> {
        check(unsafe { lurk_hip_fold_step_prefetch(self.h, range.as_ptr().cast(), offset, range.len() / 32, 0, core::ptr::null_mut()) })
    }
    /// Open the step of the oldest staged instance; `patches`: the ranges of W2 known only now.
    pub fn begin_prefetched(&mut self, patches: &[lurk_hip_w2_patch], x2: &[u8]) -> Result<([u8; 96], [u8; 96]), Error> {
        let (mut cw, mut ct) = ([0u8; 96], [0u8; 96]);
        check(unsafe {
            lurk_hip_fold_step_begin_prefetched(self.h, patches.as_ptr(), patches.len(), x2.as_ptr().cast(), cw.as_mut_ptr().cast(), ct.as_mut_ptr().cast())
        })?;
        Ok((cw, ct))
    }
}
impl Drop for FoldingContext<'_> {
    fn drop(&mut self) {
        unsafe { lurk_hip_fold_ctx_destroy(self.h) };
    }
}

/// Batched Poseidon behind `PoseidonCache::hash{3,4,6,8}` (`/root/reference/src/hash.rs:180-204`): `preimages` holds `n * arity`
/// canonical 32-byte elements (`to_repr()`), the result `n` digests.  `arity` must be 3, 4, 6 or 8 (`hash.rs:19-29`).
pub mod poseidon {
    use super::*;
    pub fn hash_batch(field_id: c_int, arity: usize, preimages: &[u8]) -> Result<Vec<u8>, Error> {
        assert!(matches!(arity, 3 | 4 | 6 | 8), "unsupported arity");
        assert_eq!(preimages.len() % (32 * arity), 0);
        let n = preimages.len() / (32 * arity);
        let mut out = vec![0u8; 32 * n];
        check(unsafe { lurk_hip_poseidon_batch(field_id, arity as c_int, preimages.as_ptr().cast(), n, out.as_mut_ptr().cast()) })?;
        Ok(out)
    }
}
