//! The compressing SNARK on BN254 G1 (lurk-beta's default cycle): the Spartan sum-checks of [`crate::spartan_prove`] opened by the
//! HyperKZG argument of [`crate::hyperkzg`], each as one library call with the Keccak transcript inside.  [`verify_pairing`] /
//! [`verify_pairing_batch`] DECIDE against a [`VerifierKey`] by the library's own pairing check.  [`verify`] / [`verify_batch`] end UP TO
//! THE PAIRING for a caller that has its own: they return `(verdict, L, R)` and the proof is valid iff `verdict.accepted` and
//!
//! ```ignore
//! use halo2curves::bn256::{pairing, G1Affine, G2Affine};
//! // l, r: L and R converted from the 96-byte Jacobians; tau_h = [tau]H of the SRS, h = G2Affine::generator()
//! pairing(&l, &h) == pairing(&r, &tau_h)
//! ```
//!
//! on the Rust side.  The protocol is the library's own (include/lurk_hip.h, DESIGN.md section
//! 3.7.3), not arecibo's byte for byte.
use core::ffi::{c_int, c_void};

use crate::ffi::*;
use crate::hyperkzg::VerifierKey;
use crate::{check, Error, R1csShape, Verdict};

/// The proof of [`prove`]: the seven sum-check fields of [`crate::SpartanProof`], then HyperKZG's.
pub struct Proof {
    pub polys_outer: Vec<u8>,  // log2(num_cons) x 4 x 32 B, canonical
    pub claims_outer: [u8; 96],
    pub eval_e: [u8; 32],
    pub polys_inner: Vec<u8>,  // (log2(num_vars) + 1) x 3 x 32 B
    pub eval_w: [u8; 32],
    pub polys_batch: Vec<u8>,  // log2(N) x 3 x 32 B, N = max(num_cons, num_vars)
    pub evals_batch: [u8; 64],
    pub kzg_com: Vec<u8>,      // (log2(N) - 1) x 96 B Jacobians
    pub kzg_v: Vec<u8>,        // 3 log2(N) x 32 B, t-major
    pub kzg_w: [u8; 288],      // 3 x 96 B Jacobians
}
/// The proof of [`prove_batch`].
pub struct BatchProof {
    pub polys_outer: Vec<u8>,
    pub claims_outer: Vec<u8>,  // n x 3 x 32 B
    pub evals_e: Vec<u8>,       // n x 32 B
    pub polys_inner: Vec<u8>,
    pub evals_w: Vec<u8>,       // n x 32 B
    pub polys_batch: Vec<u8>,
    pub evals_batch: Vec<u8>,   // 2 n x 32 B
    pub kzg_com: Vec<u8>,
    pub kzg_v: Vec<u8>,
    pub kzg_w: [u8; 288],
}

fn log2(n: usize) -> usize {
    n.trailing_zeros() as usize
}
fn batch_ells(instances: &[lurk_hip_spartan_instance]) -> (usize, usize, usize) {
    let max_nc = instances.iter().map(|i| i.num_cons).max().unwrap_or(2);
    let max_nv = instances.iter().map(|i| i.num_vars).max().unwrap_or(2);
    (log2(max_nc), log2(max_nv) + 1, log2(max_nc.max(max_nv)))
}

impl Proof {
    /// Every field has the length the header states for this shape.
    fn well_sized(&self, num_cons: usize, num_vars: usize) -> bool {
        let (ell_x, ell_y, ell) = (log2(num_cons), log2(num_vars) + 1, log2(num_cons.max(num_vars)));
        self.polys_outer.len() == ell_x * 128 && self.polys_inner.len() == ell_y * 96 && self.polys_batch.len() >= ell * 96
            && self.kzg_com.len() == ell.saturating_sub(1) * 96 && self.kzg_v.len() == 3 * ell * 32
    }
    /// The proof as the verifiers take it (the library only reads through these pointers).
    fn as_ffi(&self) -> lurk_hip_spartan_kzg_proof {
        lurk_hip_spartan_kzg_proof {
            polys_outer: self.polys_outer.as_ptr() as *mut c_void, claims_outer: self.claims_outer.as_ptr() as *mut c_void, eval_e: self.eval_e.as_ptr() as *mut c_void,
            polys_inner: self.polys_inner.as_ptr() as *mut c_void, eval_w: self.eval_w.as_ptr() as *mut c_void, polys_batch: self.polys_batch.as_ptr() as *mut c_void,
            evals_batch: self.evals_batch.as_ptr() as *mut c_void,
            kzg_com: if self.kzg_com.is_empty() { core::ptr::null_mut() } else { self.kzg_com.as_ptr() as *mut c_void }, kzg_v: self.kzg_v.as_ptr() as *mut c_void,
            kzg_w: self.kzg_w.as_ptr() as *mut c_void,
        }
    }
}
impl BatchProof {
    fn well_sized(&self, instances: &[lurk_hip_spartan_instance]) -> bool {
        let n = instances.len();
        let (ell_x, ell_y, ell) = batch_ells(instances);
        self.polys_outer.len() == ell_x * 128 && self.claims_outer.len() == n * 96 && self.evals_e.len() == n * 32 && self.polys_inner.len() == ell_y * 96
            && self.evals_w.len() == n * 32 && self.polys_batch.len() >= ell * 96 && self.evals_batch.len() == 2 * n * 32
            && self.kzg_com.len() == ell.saturating_sub(1) * 96 && self.kzg_v.len() == 3 * ell * 32
    }
    fn as_ffi(&self) -> lurk_hip_spartan_kzg_batch_proof {
        lurk_hip_spartan_kzg_batch_proof {
            polys_outer: self.polys_outer.as_ptr() as *mut c_void, claims_outer: self.claims_outer.as_ptr() as *mut c_void, evals_e: self.evals_e.as_ptr() as *mut c_void,
            polys_inner: self.polys_inner.as_ptr() as *mut c_void, evals_w: self.evals_w.as_ptr() as *mut c_void, polys_batch: self.polys_batch.as_ptr() as *mut c_void,
            evals_batch: self.evals_batch.as_ptr() as *mut c_void,
            kzg_com: if self.kzg_com.is_empty() { core::ptr::null_mut() } else { self.kzg_com.as_ptr() as *mut c_void }, kzg_v: self.kzg_v.as_ptr() as *mut c_void,
            kzg_w: self.kzg_w.as_ptr() as *mut c_void,
        }
    }
}

/// `lurk_hip_spartan_kzg_prove_dev`.  `key`: the resident BN254 G1 powers-of-tau key that committed W and E.
/// # Safety
/// `d_w` / `d_e`: `num_vars` / `num_cons` Montgomery Fr scalars in device memory; `shape_t` is the transpose of `shape`; `key` is a live
/// context of at least max(`num_cons`, `num_vars`) points.
#[allow(clippy::too_many_arguments)]
pub unsafe fn prove(shape: &R1csShape, shape_t: &R1csShape, num_cons: usize, num_vars: usize, key: *mut lurk_hip_msm_ctx, x: &[u8], u: &[u8; 32], d_w: *const c_void,
                    d_e: *const c_void, comm_w: &[u8; 96], comm_e: &[u8; 96], label: &[u8], stream: *mut c_void) -> Result<Proof, Error> {
    let (ell_x, ell_y, ell) = (log2(num_cons), log2(num_vars) + 1, log2(num_cons.max(num_vars)));
    let mut p = Proof {
        polys_outer: vec![0; ell_x * 128], claims_outer: [0; 96], eval_e: [0; 32], polys_inner: vec![0; ell_y * 96], eval_w: [0; 32],
        polys_batch: vec![0; ell.max(1) * 96], evals_batch: [0; 64], kzg_com: vec![0; ell.saturating_sub(1).max(1) * 96], kzg_v: vec![0; 3 * ell.max(1) * 32],
        kzg_w: [0; 288],
    };
    let mut out = lurk_hip_spartan_kzg_proof {
        polys_outer: p.polys_outer.as_mut_ptr().cast(), claims_outer: p.claims_outer.as_mut_ptr().cast(), eval_e: p.eval_e.as_mut_ptr().cast(),
        polys_inner: p.polys_inner.as_mut_ptr().cast(), eval_w: p.eval_w.as_mut_ptr().cast(), polys_batch: p.polys_batch.as_mut_ptr().cast(),
        evals_batch: p.evals_batch.as_mut_ptr().cast(), kzg_com: p.kzg_com.as_mut_ptr().cast(), kzg_v: p.kzg_v.as_mut_ptr().cast(), kzg_w: p.kzg_w.as_mut_ptr().cast(),
    };
    check(lurk_hip_spartan_kzg_prove_dev(shape.as_ptr(), shape_t.as_ptr(), num_cons, num_vars, x.len() / 32, key, x.as_ptr().cast(), u.as_ptr().cast(), d_w, d_e,
                                         comm_w.as_ptr().cast(), comm_e.as_ptr().cast(), label.as_ptr().cast(), label.len(), &mut out, stream))?;
    p.kzg_com.truncate(ell.saturating_sub(1) * 96);
    Ok(p)
}

/// `lurk_hip_spartan_kzg_prove_batch_dev`.
/// # Safety
/// Every instance's pointers obey the contract of [`prove`].
pub unsafe fn prove_batch(instances: &[lurk_hip_spartan_instance], key: *mut lurk_hip_msm_ctx, label: &[u8], stream: *mut c_void) -> Result<BatchProof, Error> {
    let n = instances.len();
    let (ell_x, ell_y, ell) = batch_ells(instances);
    let mut p = BatchProof {
        polys_outer: vec![0; ell_x * 128], claims_outer: vec![0; n * 96], evals_e: vec![0; n * 32], polys_inner: vec![0; ell_y * 96], evals_w: vec![0; n * 32],
        polys_batch: vec![0; ell.max(1) * 96], evals_batch: vec![0; 2 * n * 32], kzg_com: vec![0; ell.saturating_sub(1).max(1) * 96],
        kzg_v: vec![0; 3 * ell.max(1) * 32], kzg_w: [0; 288],
    };
    let mut out = lurk_hip_spartan_kzg_batch_proof {
        polys_outer: p.polys_outer.as_mut_ptr().cast(), claims_outer: p.claims_outer.as_mut_ptr().cast(), evals_e: p.evals_e.as_mut_ptr().cast(),
        polys_inner: p.polys_inner.as_mut_ptr().cast(), evals_w: p.evals_w.as_mut_ptr().cast(), polys_batch: p.polys_batch.as_mut_ptr().cast(),
        evals_batch: p.evals_batch.as_mut_ptr().cast(), kzg_com: p.kzg_com.as_mut_ptr().cast(), kzg_v: p.kzg_v.as_mut_ptr().cast(), kzg_w: p.kzg_w.as_mut_ptr().cast(),
    };
    check(lurk_hip_spartan_kzg_prove_batch_dev(instances.as_ptr(), n, key, label.as_ptr().cast(), label.len(), &mut out, stream))?;
    p.kzg_com.truncate(ell.saturating_sub(1) * 96);
    Ok(p)
}

/// `lurk_hip_spartan_kzg_verify_dev`: `(verdict, L, R)`; `verdict.accepted` means accepted SO FAR - the pairing of the module's header
/// decides.  L and R are the identity (all zero) on rejection.  No key: HyperKZG's verifier needs only G = (1, 2).
/// # Safety
/// `shape` is a live shape over `LURK_FIELD_BN254_FR`.
#[allow(clippy::too_many_arguments)]
pub unsafe fn verify(shape: &R1csShape, num_cons: usize, num_vars: usize, x: &[u8], u: &[u8; 32], comm_w: &[u8; 96], comm_e: &[u8; 96], label: &[u8], proof: &Proof,
                     stream: *mut c_void) -> Result<(Verdict, [u8; 96], [u8; 96]), Error> {
    let (mut l, mut r) = ([0u8; 96], [0u8; 96]);
    if !proof.well_sized(num_cons, num_vars) || x.len() % 32 != 0 {
        return Ok((Verdict { accepted: false, failed_check: LURK_VERIFY_MALFORMED }, l, r));
    }
    let pf = proof.as_ffi();
    let (mut accepted, mut failed): (c_int, c_int) = (0, 0);
    check(lurk_hip_spartan_kzg_verify_dev(shape.as_ptr(), num_cons, num_vars, x.len() / 32, x.as_ptr().cast(), u.as_ptr().cast(), comm_w.as_ptr().cast(),
                                          comm_e.as_ptr().cast(), label.as_ptr().cast(), label.len(), &pf, l.as_mut_ptr().cast(), r.as_mut_ptr().cast(), &mut accepted,
                                          &mut failed, stream))?;
    Ok((Verdict { accepted: accepted != 0, failed_check: failed }, l, r))
}

/// `lurk_hip_spartan_kzg_verify_batch_dev`; of an instance `shape_t`, `d_w32_mont` and `d_e32_mont` are ignored (may be null).
/// # Safety
/// Every instance's shape, x, u and commitment pointers are valid.
pub unsafe fn verify_batch(instances: &[lurk_hip_spartan_instance], label: &[u8], proof: &BatchProof, stream: *mut c_void)
                           -> Result<(Verdict, [u8; 96], [u8; 96]), Error> {
    let n = instances.len();
    let (mut l, mut r) = ([0u8; 96], [0u8; 96]);
    if !proof.well_sized(instances) {
        return Ok((Verdict { accepted: false, failed_check: LURK_VERIFY_MALFORMED }, l, r));
    }
    let pf = proof.as_ffi();
    let (mut accepted, mut failed): (c_int, c_int) = (0, 0);
    check(lurk_hip_spartan_kzg_verify_batch_dev(instances.as_ptr(), n, label.as_ptr().cast(), label.len(), &pf, l.as_mut_ptr().cast(), r.as_mut_ptr().cast(),
                                                &mut accepted, &mut failed, stream))?;
    Ok((Verdict { accepted: accepted != 0, failed_check: failed }, l, r))
}

/// `lurk_hip_spartan_kzg_verify_pairing_dev`: the verifier that DECIDES - [`verify`] and then `e(L, H) e(-R, [tau]H) == 1` in the library
/// against `vk`.  `Ok(true)`: the proof is valid.
/// # Safety
/// As [`verify`].
#[allow(clippy::too_many_arguments)]
pub unsafe fn verify_pairing(shape: &R1csShape, num_cons: usize, num_vars: usize, x: &[u8], u: &[u8; 32], comm_w: &[u8; 96], comm_e: &[u8; 96], label: &[u8],
                             proof: &Proof, vk: &VerifierKey, stream: *mut c_void) -> Result<bool, Error> {
    if !proof.well_sized(num_cons, num_vars) || x.len() % 32 != 0 {
        return Ok(false);
    }
    let pf = proof.as_ffi();
    let (mut accepted, mut failed): (c_int, c_int) = (0, 0);
    check(lurk_hip_spartan_kzg_verify_pairing_dev(shape.as_ptr(), num_cons, num_vars, x.len() / 32, x.as_ptr().cast(), u.as_ptr().cast(), comm_w.as_ptr().cast(),
                                                  comm_e.as_ptr().cast(), label.as_ptr().cast(), label.len(), &pf, vk.tau_h.as_ptr().cast(), &mut accepted, &mut failed,
                                                  stream))?;
    Ok(accepted != 0)
}

/// `lurk_hip_spartan_kzg_verify_pairing_batch_dev`: [`verify_batch`] and the pairing check.  `Ok(true)`: the proof is valid.
/// # Safety
/// As [`verify_batch`].
pub unsafe fn verify_pairing_batch(instances: &[lurk_hip_spartan_instance], label: &[u8], proof: &BatchProof, vk: &VerifierKey, stream: *mut c_void)
                                   -> Result<bool, Error> {
    if !proof.well_sized(instances) {
        return Ok(false);
    }
    let pf = proof.as_ffi();
    let (mut accepted, mut failed): (c_int, c_int) = (0, 0);
    check(lurk_hip_spartan_kzg_verify_pairing_batch_dev(instances.as_ptr(), instances.len(), label.as_ptr().cast(), label.len(), &pf, vk.tau_h.as_ptr().cast(),
                                                        &mut accepted, &mut failed, stream))?;
    Ok(accepted != 0)
}

/// `lurk_hip_fold_padded_dev`: `d_out[j] = sum_k c_k (j < lens[k] ? d_vecs[k][j] : 0)` for `j < n_out` in one launch.
/// # Safety
/// `d_vecs[k]` is device memory of `lens[k]` x 32 bytes (null when `lens[k]` is 0), `d_out` of `n_out` x 32 bytes, not overlapping an input.
pub unsafe fn fold_padded(field_id: c_int, d_vecs: &[*const c_void], lens: &[usize], coeffs_mont: &[[u8; 32]], n_out: usize, d_out: *mut c_void, stream: *mut c_void)
                          -> Result<(), Error> {
    if d_vecs.len() != lens.len() || d_vecs.len() != coeffs_mont.len() {
        return Err(Error { code: LURK_HIP_ERR_INVALID_ARG, message: "fold_padded: d_vecs, lens and coeffs_mont differ in length".into() });
    }
    check(lurk_hip_fold_padded_dev(field_id, d_vecs.len() as c_int, d_vecs.as_ptr(), lens.as_ptr(), coeffs_mont.as_ptr().cast(), n_out, d_out, stream))
}
