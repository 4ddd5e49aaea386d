//! The sparse Poseidon trie of `coprocessor::trie` (`/root/reference/src/coprocessor/trie/mod.rs`) over the library's device-resident
//! form (`include/lurk_hip.h`, "the sparse Poseidon trie"):
//!
//! * [`DeviceTrie`] - the opaque handle: one bulk build from pairs sorted by path value, then `prove_lookup` / `prove_insert` for batches
//!   of keys, `insert_chain` for a sequence of dependent insertions, and the two verifiers for batches of proofs, all on device buffers
//!   (raw pointers, as everywhere in this crate);
//! * [`TrieNodes`] - the child map of every version of the trie, addressed by root: `new_with_root` on the device;
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

/// The trie's child map on the device (`lurk_hip_trie_nodes`; `include/lurk_hip.h`, "root-addressed tries"): every version of every trie of
/// one (field, height), content-addressed and append-only.  What `Trie::new_with_root` (`:566-576`) and a host-side root -> handle table
/// were for: a root goes in as an element and the walk happens on the device.
pub struct TrieNodes {
    handle: *mut lurk_hip_trie_nodes,
}
unsafe impl Send for TrieNodes {}

/// How many queries of a root-addressed call met a node that is not in the store (`Error::MissingPreimage`); `d_status` says which.
pub struct Missing {
    pub n_missing: u64,
}

impl TrieNodes {
    /// `init_empty`: the store holds the `height` nodes of the empty chain.
    pub fn create(field_id: c_int, height: usize, reserve_nodes: usize) -> Result<Self, Error> {
        let mut handle = core::ptr::null_mut();
        check(unsafe { lurk_hip_trie_nodes_create(&mut handle, field_id, height as c_int, reserve_nodes) })?;
        Ok(Self { handle })
    }
    /// (field id, height, nodes, slots, device)
    pub fn info(&self) -> Result<(c_int, usize, usize, usize, c_int), Error> {
        let (mut field, mut height, mut n, mut slots, mut device) = (0, 0, 0usize, 0usize, 0);
        check(unsafe { lurk_hip_trie_nodes_info(self.handle, &mut field, &mut height, &mut n, &mut slots, &mut device) })?;
        Ok((field, height as usize, n, slots, device))
    }
    /// `register_hash` for `count` preimages; `d_digests_out` may be null.  Synchronises `stream`.
    /// # Safety
    /// device buffers: `count * 8` elements in, `count` digests out
    pub unsafe fn register_dev(&mut self, d_preimages: *const c_void, count: usize, d_digests_out: *mut c_void, stream: *mut c_void) -> Result<(), Error> {
        check(lurk_hip_trie_nodes_register_dev(self.handle, d_preimages, count, d_digests_out, stream))
    }
    /// Every node of a built trie of the same field and height; nothing is hashed.  Synchronises `stream`.
    pub fn add_trie(&mut self, trie: &DeviceTrie, stream: *mut c_void) -> Result<(), Error> {
        check(unsafe { lurk_hip_trie_nodes_add_trie(self.handle, trie.handle, stream) })
    }
    /// `InversePoseidonCache::get` for `m` digests.  Does not synchronise.
    /// # Safety
    /// device buffers: `m` digests in; `m * 8` elements and `m` u32 out
    pub unsafe fn get_dev(&self, d_digests: *const c_void, m: usize, d_preimages: *mut c_void, d_found: *mut u32, stream: *mut c_void) -> Result<(), Error> {
        check(lurk_hip_trie_nodes_get_dev(self.handle, d_digests, m, d_preimages, d_found, stream))
    }
    /// `new_with_root` + `prove_lookup` per query.  `one_root`: `d_roots` holds one root for every query, otherwise one per query.
    /// `count_missing` waits for the walk and reports how many statuses are non-zero.
    /// # Safety
    /// device buffers: roots and `m` keys in; `m * height * 8` path elements, `m` values and `m` u32 statuses out
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn prove_lookup_dev(&self, d_roots: *const c_void, one_root: bool, d_keys: *const c_void, m: usize, d_paths: *mut c_void, d_values: *mut c_void,
                                   d_status: *mut u32, count_missing: bool, stream: *mut c_void) -> Result<Option<Missing>, Error> {
        let mut n_missing = 0u64;
        let out = if count_missing { &mut n_missing as *mut u64 } else { core::ptr::null_mut() };
        check(lurk_hip_trie_nodes_prove_lookup_dev(self.handle, d_roots, usize::from(!one_root), d_keys, m, d_paths, d_values, d_status, out, stream))?;
        Ok(count_missing.then_some(Missing { n_missing }))
    }
    /// `m` independent `new_with_root` + `prove_insert`; with `register_new` every new root is addressable when the call returns.
    /// # Safety
    /// device buffers as `DeviceTrie::prove_insert_dev`, and `m` u32 statuses out
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn prove_insert_dev(&mut self, d_roots: *const c_void, one_root: bool, d_keys: *const c_void, d_new_values: *const c_void, m: usize,
                                   d_old_paths: *mut c_void, d_new_paths: *mut c_void, d_old_values: *mut c_void, d_new_roots: *mut c_void, d_status: *mut u32,
                                   register_new: bool, stream: *mut c_void) -> Result<Missing, Error> {
        let mut n_missing = 0u64;
        check(lurk_hip_trie_nodes_prove_insert_dev(self.handle, d_roots, usize::from(!one_root), d_keys, d_new_values, m, d_old_paths, d_new_paths, d_old_values,
                                                   d_new_roots, d_status, &mut n_missing, c_int::from(register_new), stream))?;
        Ok(Missing { n_missing })
    }
    /// A chain of `m` dependent insertions that starts at the trie named by `root`; every root it leaves is addressable afterwards.
    /// # Safety
    /// device buffers as `DeviceTrie::insert_chain_dev`; each output may be null
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn insert_chain_dev(&mut self, root: &Element, d_keys: *const c_void, d_values: *const c_void, m: usize, d_old_paths: *mut c_void,
                                   d_new_paths: *mut c_void, d_old_values: *mut c_void, d_roots: *mut c_void, stream: *mut c_void) -> Result<(), Error> {
        check(lurk_hip_trie_nodes_insert_chain_dev(self.handle, root.as_ptr().cast(), d_keys, d_values, m, d_old_paths, d_new_paths, d_old_values, d_roots, stream))
    }
}
impl Drop for TrieNodes {
    fn drop(&mut self) {
        unsafe { lurk_hip_trie_nodes_destroy(self.handle) };
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

/// Which of the trie coprocessor's two step circuits: the body of `Trie::synthesize_lookup` (`:652-714`) or of `Trie::synthesize_insert`
/// (`:802-880`) - `include/lurk_hip.h`, "the trie coprocessor's step circuits".
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
#[repr(i32)]
pub enum TrieCircuit {
    Lookup = 0,
    Insert = 1,
}

/// `lurk_hip_trie_circuit_size`: the block's elements, its rows and their non-zeros, and where the result (and, for an insert, the new
/// value) sits in the block.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct TrieCircuitSize {
    pub size: usize,
    pub num_cons: usize,
    pub nnz: [usize; 3],
    pub result_col: usize,
    pub value_col: Option<usize>,
}

/// Host only.
pub fn trie_circuit_size(field_id: c_int, height: usize, op: TrieCircuit) -> Result<TrieCircuitSize, Error> {
    let (mut size, mut rows, mut na, mut nb, mut nc, mut result, mut value) = (0usize, 0usize, 0usize, 0usize, 0usize, 0usize, 0usize);
    check(unsafe { lurk_hip_trie_circuit_size(field_id, height as c_int, op as c_int, &mut size, &mut rows, &mut na, &mut nb, &mut nc, &mut result, &mut value) })?;
    Ok(TrieCircuitSize { size, num_cons: rows, nnz: [na, nb, nc], result_col: result, value_col: (op == TrieCircuit::Insert).then_some(value) })
}

/// The circuit's rows: A, B, C over the block's local columns; local column `size` is the constant ONE.  Host only.
pub fn trie_circuit_constraints(field_id: c_int, height: usize, op: TrieCircuit) -> Result<[SlotMatrix; 3], Error> {
    let sz = trie_circuit_size(field_id, height, op)?;
    let mk = |nnz: usize| SlotMatrix { indptr: vec![0u64; sz.num_cons + 1], indices: vec![0u64; nnz], data: vec![0u8; nnz * 32] };
    let (mut a, mut b, mut c) = (mk(sz.nnz[0]), mk(sz.nnz[1]), mk(sz.nnz[2]));
    check(unsafe {
        lurk_hip_trie_circuit_constraints(field_id, height as c_int, op as c_int, a.indptr.as_mut_ptr(), a.indices.as_mut_ptr(), a.data.as_mut_ptr().cast(),
                                          b.indptr.as_mut_ptr(), b.indices.as_mut_ptr(), b.data.as_mut_ptr().cast(), c.indptr.as_mut_ptr(), c.indices.as_mut_ptr(),
                                          c.data.as_mut_ptr().cast())
    })?;
    Ok([a, b, c])
}

/// A resident shape of `n_blocks` circuits at columns `first + b * stride`, ONE at column `num_vars` (`lurk_hip_trie_circuit_r1cs_create`);
/// `extra` = the caller's further rows (the `synthesize_*_aux` wrappers and whatever else the step circuit holds), appended.
#[allow(clippy::too_many_arguments)]
pub fn trie_circuit_shape(field_id: c_int, height: usize, op: TrieCircuit, n_blocks: usize, first: usize, stride: usize, num_vars: usize, num_io: usize,
                          extra: Option<(Csr, Csr, Csr)>) -> Result<R1csShape, Error> {
    let mut p = core::ptr::null_mut();
    let null = core::ptr::null::<u64>();
    check(unsafe {
        match extra {
            Some((a, b, c)) => lurk_hip_trie_circuit_r1cs_create(&mut p, field_id, height as c_int, op as c_int, n_blocks, first, stride, num_vars, num_io,
                                                                 a.indptr.len().saturating_sub(1), a.indptr.as_ptr(), a.indices.as_ptr(), a.data.as_ptr().cast(),
                                                                 b.indptr.as_ptr(), b.indices.as_ptr(), b.data.as_ptr().cast(), c.indptr.as_ptr(), c.indices.as_ptr(),
                                                                 c.data.as_ptr().cast()),
            None => lurk_hip_trie_circuit_r1cs_create(&mut p, field_id, height as c_int, op as c_int, n_blocks, first, stride, num_vars, num_io, 0, null, null,
                                                      null.cast(), null, null, null.cast(), null, null, null.cast()),
        }
    })?;
    Ok(R1csShape(p))
}

/// The blocks of `m` circuits written into the resident witness `d_w` (`lurk_hip_trie_circuit_witness_dev`): block `i` at `d_offsets[i]`, or
/// at `first + i * stride` when `d_offsets` is null.  `one_root`: `d_roots` holds one root for every block, otherwise one per block - for a
/// chain `[root(T_0), roots[0 .. m - 2]]` of `insert_chain`.  A lookup passes null for `d_new_values` and `d_new_paths`.  The proof is not
/// judged; does not synchronise.
/// # Safety
/// device buffers of canonical elements as the trie calls leave them; `d_w` holds every block
#[allow(clippy::too_many_arguments)]
pub unsafe fn trie_circuit_witness_dev(field_id: c_int, height: usize, op: TrieCircuit, d_roots: *const c_void, one_root: bool, d_keys: *const c_void,
                                       d_new_values: *const c_void, d_old_paths: *const c_void, d_new_paths: *const c_void, m: usize, d_w: *mut c_void,
                                       d_offsets: *const u64, first: usize, stride: usize, stream: *mut c_void) -> Result<(), Error> {
    check(lurk_hip_trie_circuit_witness_dev(field_id, height as c_int, op as c_int, d_roots, usize::from(!one_root), d_keys, d_new_values, d_old_paths, d_new_paths, m,
                                            d_w, d_offsets, first, stride, stream))
}
