//! The sparse Poseidon trie of `coprocessor::trie` (`/root/reference/src/coprocessor/trie/mod.rs`) over the library's device-resident
//! form (`include/lurk_hip.h`, "the sparse Poseidon trie"):
//!
//! * [`DeviceTrie`] - the opaque handle: one bulk build from pairs sorted by path value, then `prove_lookup` / `prove_insert` for batches
//!   of keys, `insert_chain` for a sequence of dependent insertions, and the two verifiers for batches of proofs, all on device buffers
//!   (raw pointers, as everywhere in this crate);
//! * [`LookupProof`] / [`InsertProof`] - shaped like the reference's (`:339-369`): a `preimage_path` of `HEIGHT` preimages of `ARITY`
//!   elements, root level first.  [`LookupProof::from_flat`] cuts them out of a batch copied back to the host, and `flat` is what a
//!   verifier call takes.
//!
//! Field elements cross as their canonical 32 bytes.  Never compiled in the container this repository is built in.
use super::*;
use core::ffi::c_void;

pub type Element = [u8; 32];

/// `LookupProof<F, ARITY, HEIGHT>`: `preimage_path[k]` is the preimage of the node at depth k on the key's path.
#[derive(Clone, Debug, PartialEq, Eq)]
pub struct LookupProof<const ARITY: usize = 8> {
    pub preimage_path: Vec<[Element; ARITY]>,
}
impl<const ARITY: usize> LookupProof<ARITY> {
    /// proof `index` of a batch of paths (`m * height * ARITY` elements) as the prove calls write them
    pub fn from_flat(paths: &[Element], height: usize, index: usize) -> Self {
        let at = &paths[index * height * ARITY..(index + 1) * height * ARITY];
        Self { preimage_path: at.chunks_exact(ARITY).map(|c| <[Element; ARITY]>::try_from(c).unwrap()).collect() }
    }
    pub fn flat(&self) -> Vec<Element> {
        self.preimage_path.iter().flatten().copied().collect()
    }
    pub fn height(&self) -> usize {
        self.preimage_path.len()
    }
}

/// `InsertProof<F, ARITY, HEIGHT>`: the lookup proof before the insertion and the one after it.
#[derive(Clone, Debug, PartialEq, Eq)]
pub struct InsertProof<const ARITY: usize = 8> {
    pub old_proof: LookupProof<ARITY>,
    pub new_proof: LookupProof<ARITY>,
}

/// What a verifier call reports: one code per proof (0 = accepted; see the header for the others) and how many are non-zero.
pub struct Verdict {
    pub n_failed: u64,
}

/// A built trie on the device.  The library supports arity 8 only.
pub struct DeviceTrie {
    handle: *mut lurk_hip_trie,
}
unsafe impl Send for DeviceTrie {}
unsafe impl Sync for DeviceTrie {} // the prove calls only read the handle

impl DeviceTrie {
    /// # Safety
    /// `d_keys` / `d_values`: device buffers of `n` elements; keys reduced and strictly increasing in path order (checked, refused otherwise).
    pub unsafe fn build_dev(field_id: c_int, height: usize, d_keys: *const c_void, d_values: *const c_void, n: usize, stream: *mut c_void) -> Result<Self, Error> {
        let mut handle = core::ptr::null_mut();
        check(lurk_hip_trie_build_dev(&mut handle, field_id, height as c_int, d_keys, d_values, n, stream))?;
        Ok(Self { handle })
    }
    pub fn root(&self) -> Result<Element, Error> {
        let mut out = [0u8; 32];
        check(unsafe { lurk_hip_trie_root(self.handle, out.as_mut_ptr().cast()) })?;
        Ok(out)
    }
    /// (field id, height, number of keys, device)
    pub fn info(&self) -> Result<(c_int, usize, usize, c_int), Error> {
        let (mut field, mut height, mut n, mut device) = (0, 0, 0usize, 0);
        check(unsafe { lurk_hip_trie_info(self.handle, &mut field, &mut height, &mut n, &mut device) })?;
        Ok((field, height as usize, n, device))
    }
    /// # Safety
    /// device buffers: `m` keys in, `m * height * 8` path elements and `m` values out
    pub unsafe fn prove_lookup_dev(&self, d_keys: *const c_void, m: usize, d_paths: *mut c_void, d_values: *mut c_void, stream: *mut c_void) -> Result<(), Error> {
        check(lurk_hip_trie_prove_lookup_dev(self.handle, d_keys, m, d_paths, d_values, stream))
    }
    /// # Safety
    /// device buffers; `d_old_paths` and `d_new_paths` (`m * height * 8` elements each) must not overlap
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn prove_insert_dev(&self, d_keys: *const c_void, d_new_values: *const c_void, m: usize, d_old_paths: *mut c_void, d_new_paths: *mut c_void,
                                   d_old_values: *mut c_void, d_new_roots: *mut c_void, stream: *mut c_void) -> Result<(), Error> {
        check(lurk_hip_trie_prove_insert_dev(self.handle, d_keys, d_new_values, m, d_old_paths, d_new_paths, d_old_values, d_new_roots, stream))
    }
    /// A chain of `m` dependent insertions: update i is applied to the trie update i - 1 left (`Trie::prove_insert` step after step).
    /// Every output may be null when it is not wanted, but not all of them; `want_trie` asks for the trie after the last update as a
    /// new handle (this one is not modified).  Synchronises `stream`.
    /// # Safety
    /// device buffers: `m` keys and values in; `m * height * 8` elements per path buffer (they must not overlap), `m` old values and
    /// `m` roots out
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn insert_chain_dev(&self, d_keys: *const c_void, d_values: *const c_void, m: usize, d_old_paths: *mut c_void, d_new_paths: *mut c_void,
                                   d_old_values: *mut c_void, d_roots: *mut c_void, want_trie: bool, stream: *mut c_void) -> Result<Option<DeviceTrie>, Error> {
        let mut handle = core::ptr::null_mut();
        let out = if want_trie { &mut handle as *mut *mut lurk_hip_trie } else { core::ptr::null_mut() };
        check(lurk_hip_trie_insert_chain_dev(self.handle, d_keys, d_values, m, d_old_paths, d_new_paths, d_old_values, d_roots, out, stream))?;
        Ok(if want_trie { Some(DeviceTrie { handle }) } else { None })
    }
}
impl Drop for DeviceTrie {
    fn drop(&mut self) {
        unsafe { lurk_hip_trie_destroy(self.handle) };
    }
}

/// `LookupProof::verify` for `m` proofs.  `one_root`: `d_roots` holds one root for every proof, otherwise one per proof.
/// # Safety
/// device buffers; `d_codes`: `m` u32 out
#[allow(clippy::too_many_arguments)]
pub unsafe fn verify_lookup_dev(field_id: c_int, height: usize, d_roots: *const c_void, one_root: bool, d_keys: *const c_void, d_values: *const c_void,
                                d_paths: *const c_void, m: usize, d_codes: *mut u32, stream: *mut c_void) -> Result<Verdict, Error> {
    let mut n_failed = 0u64;
    check(lurk_hip_trie_verify_lookup_dev(field_id, height as c_int, d_roots, usize::from(!one_root), d_keys, d_values, d_paths, m, d_codes, &mut n_failed, stream))?;
    Ok(Verdict { n_failed })
}

/// `InsertProof::verify` for `m` proofs; an absent old value is passed as 0.
/// # Safety
/// device buffers; `d_codes`: `m` u32 out
#[allow(clippy::too_many_arguments)]
pub unsafe fn verify_insert_dev(field_id: c_int, height: usize, d_old_roots: *const c_void, d_new_roots: *const c_void, one_root: bool, d_keys: *const c_void,
                                d_old_values: *const c_void, d_new_values: *const c_void, d_old_paths: *const c_void, d_new_paths: *const c_void, m: usize,
                                d_codes: *mut u32, stream: *mut c_void) -> Result<Verdict, Error> {
    let mut n_failed = 0u64;
    check(lurk_hip_trie_verify_insert_dev(field_id, height as c_int, d_old_roots, d_new_roots, usize::from(!one_root), d_keys, d_old_values, d_new_values,
                                          d_old_paths, d_new_paths, m, d_codes, &mut n_failed, stream))?;
    Ok(Verdict { n_failed })
}

/// The `height` path digits of every key (host only).
pub fn path_digits(field_id: c_int, height: usize, keys: &[Element]) -> Result<Vec<u8>, Error> {
    let mut out = vec![0u8; keys.len() * height];
    check(unsafe { lurk_hip_trie_path_digits(field_id, height as c_int, keys.as_ptr().cast(), keys.len(), out.as_mut_ptr()) })?;
    Ok(out)
}
