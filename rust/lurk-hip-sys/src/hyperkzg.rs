//! The HyperKZG opening argument of the BN254 cycle (`EE1` of lurk-beta's default `Bn256EngineKZG`,
//! `/root/reference/src/proof/nova.rs:65-71`) over the library: the prover with the polynomial and the key resident in HBM, and the
//! verifier - [`verify`] decides `e(L, H) == e(R, [tau]H)` against a [`VerifierKey`] by the library's pairing check, [`pairing_inputs`]
//! stops before it for a caller with a pairing of its own (halo2curves).  The protocol is the library's own statement of the scheme
//! (include/lurk_hip.h), not arecibo's bytes: the transcript is the caller's closure.
use core::ffi::{c_int, c_void};

use crate::ffi::*;
use crate::{check, Error};

/// What the prover returns: `com` (ell - 1 Jacobians of 96 bytes), `v` (3 ell canonical scalars, t-major), `w` (3 Jacobians), `y`.
#[derive(Debug, Clone)]
pub struct Proof {
    pub com: Vec<[u8; 96]>,
    pub v: Vec<[u8; 32]>,
    pub w: [[u8; 96]; 3],
    pub y: [u8; 32],
}

/// The transcript's side of the call: stage 0 receives the commitments (`count` x 96 bytes), stage 1 the evaluations (`count` x 32
/// bytes); `None` aborts the proof (the key stays usable).
pub trait Transcript {
    fn challenge(&mut self, stage: i32, data: &[u8], count: usize) -> Option<[u8; 32]>;
}

unsafe extern "C" fn trampoline<T: Transcript>(user: *mut c_void, stage: c_int, data: *const c_void, count: usize, out: *mut c_void) -> c_int {
    let t = &mut *(user as *mut T);
    let width = if stage == 0 { 96 } else { 32 };
    let bytes: &[u8] = if count == 0 { &[] } else { core::slice::from_raw_parts(data as *const u8, count * width) };
    match t.challenge(stage, bytes, count) {
        Some(c) => {
            core::ptr::copy_nonoverlapping(c.as_ptr(), out as *mut u8, 32);
            0
        }
        None => 1,
    }
}

/// `key`: a resident BN254 G1 key of at least `n` points; `d_poly`: `n = 2^ell` Montgomery scalars in device memory (not modified);
/// `x_mont`: ell Montgomery scalars, x_0 for the most significant index bit.
///
/// # Safety
/// `key` must be a live context, `d_poly` device memory of `n` x 32 bytes produced on `stream`.
pub unsafe fn prove<T: Transcript>(key: *mut lurk_hip_msm_ctx, d_poly: *const c_void, n: usize, x_mont: &[[u8; 32]], stream: *mut c_void,
                                   transcript: &mut T) -> Result<Proof, Error> {
    let ell = x_mont.len();
    let mut proof = Proof { com: vec![[0u8; 96]; ell.saturating_sub(1)], v: vec![[0u8; 32]; 3 * ell], w: [[0u8; 96]; 3], y: [0u8; 32] };
    let user = transcript as *mut T as *mut c_void;
    check(lurk_hip_hyperkzg_prove_dev(key, d_poly, n, x_mont.as_ptr().cast(), Some(trampoline::<T>), user, proof.com.as_mut_ptr().cast(), proof.v.as_mut_ptr().cast(),
                                      proof.w.as_mut_ptr().cast(), proof.y.as_mut_ptr().cast(), stream))?;
    Ok(proof)
}

/// The verifier up to the pairing (host only).  Scalars canonical; `r`, `q`, `d` from the verifier's own transcript.  Returns
/// (L, R, accepted so far, failed check); the proof is valid iff accepted and the caller's pairing check on (L, R) holds.
pub fn pairing_inputs(c: &[u8; 96], x: &[[u8; 32]], proof: &Proof, r: &[u8; 32], q: &[u8; 32], d: &[u8; 32]) -> Result<([u8; 96], [u8; 96], bool, i32), Error> {
    let (mut l, mut rr) = ([0u8; 96], [0u8; 96]);
    let (mut accepted, mut failed): (c_int, c_int) = (0, 0);
    let ell = x.len() as c_int;
    // SAFETY: every pointer is a live host buffer of the size the header states for `ell`
    check(unsafe {
        lurk_hip_hyperkzg_pairing_inputs(LURK_CURVE_BN254, ell, c.as_ptr().cast(), x.as_ptr().cast(), proof.y.as_ptr().cast(), proof.com.as_ptr().cast(),
                                         proof.v.as_ptr().cast(), proof.w.as_ptr().cast(), r.as_ptr().cast(), q.as_ptr().cast(), d.as_ptr().cast(), l.as_mut_ptr().cast(),
                                         rr.as_mut_ptr().cast(), &mut accepted, &mut failed)
    })?;
    Ok((l, rr, accepted != 0, failed))
}

/// The verifier's half of a KZG setup: `tau_h = [tau]H`, a G2 point in the library's 128-byte form ({x.c0, x.c1, y.c0, y.c1}, each four
/// little-endian u64 Montgomery limbs - halo2curves' `G2Affine` as recalled, unpinned).
#[derive(Debug, Clone, PartialEq, Eq)]
pub struct VerifierKey {
    pub tau_h: [u8; 128],
}

impl VerifierKey {
    /// `[tau]H` from a canonical `tau` below the group order: a TRAPDOOR setup for tests and benchmarks only.
    pub fn trapdoor(tau: &[u8; 32]) -> Result<Self, Error> {
        let mut tau_h = [0u8; 128];
        // SAFETY: out is 128 bytes, the scalar 32; a null point means the generator
        check(unsafe { lurk_hip_bn254_g2_mul(tau_h.as_mut_ptr().cast(), core::ptr::null(), tau.as_ptr().cast()) })?;
        Ok(VerifierKey { tau_h })
    }

    /// Is the resident BN254 G1 key a powers-of-tau key for this verifier key?  Two commitments under the key with weights drawn from
    /// `seed` (choose it after the key exists) and one pairing check.
    ///
    /// # Safety
    /// `key` must be a live context with slots 0 and 1 free.
    pub unsafe fn key_check(&self, key: *mut lurk_hip_msm_ctx, seed: u64, stream: *mut c_void) -> Result<bool, Error> {
        let mut consistent: c_int = 0;
        check(lurk_hip_kzg_key_check_dev(key, self.tau_h.as_ptr().cast(), seed, &mut consistent, stream))?;
        Ok(consistent != 0)
    }
}

/// The verifier that DECIDES (host only): [`pairing_inputs`] and then `e(L, H) e(-R, tau_h) == 1` in the library.  `Ok(true)`: the proof
/// is valid.
pub fn verify(c: &[u8; 96], x: &[[u8; 32]], proof: &Proof, r: &[u8; 32], q: &[u8; 32], d: &[u8; 32], vk: &VerifierKey) -> Result<bool, Error> {
    let (mut accepted, mut failed): (c_int, c_int) = (0, 0);
    let ell = x.len() as c_int;
    // SAFETY: every pointer is a live host buffer of the size the header states for `ell`
    check(unsafe {
        lurk_hip_hyperkzg_verify(LURK_CURVE_BN254, ell, c.as_ptr().cast(), x.as_ptr().cast(), proof.y.as_ptr().cast(), proof.com.as_ptr().cast(), proof.v.as_ptr().cast(),
                                 proof.w.as_ptr().cast(), r.as_ptr().cast(), q.as_ptr().cast(), d.as_ptr().cast(), vk.tau_h.as_ptr().cast(), &mut accepted, &mut failed)
    })?;
    Ok(accepted != 0)
}

/// `[tau^(first + i)]G` for i < n into device memory (64-byte affine records): a TRAPDOOR setup for tests and benchmarks only.
///
/// # Safety
/// `d_out` must be device memory of `n` x 64 bytes.
pub unsafe fn trapdoor_bases(tau: &[u8; 32], first: usize, n: usize, d_out: *mut c_void, stream: *mut c_void) -> Result<(), Error> {
    check(lurk_hip_synth_kzg_bases_dev(LURK_CURVE_BN254, tau.as_ptr().cast(), first, n, d_out, stream))
}
