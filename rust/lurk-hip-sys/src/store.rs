//! The two Poseidon hooks lurk-beta's store has, over the library:
//!
//! * [`HipPoseidonCache`] - the shape of `PoseidonCache<F>` (`/root/reference/src/hash.rs:86-114, 180-204`): `hash3` / `hash4` /
//!   `hash6` / `hash8` of ONE preimage with the same memoisation, a miss hashed by the library's HOST Poseidon
//!   (`lurk_hip_poseidon_hash_host`: ~20 us, no launch), and `hash_many` for whoever holds a batch (`lurk_hip_poseidon_batch`);
//! * [`HipStoreHasher`] - the shape of `StoreHasher<Tag, FWrap<F>>` (`/root/reference/src/lem/store_core.rs:10-14`) with the preimage
//!   layouts of `impl StoreHasher for PoseidonCache` (`/root/reference/src/lem/store.rs:29-78`): `hash_ptrs` (2, 3 or 4 tagged
//!   pointers -> hash4 / hash6 / hash8), `hash_compact`, `hash_commitment`;
//! * [`hydrate`] - `StoreCore::hydrate_z_cache` (`/root/reference/src/lem/store_core.rs:256-269`) as ONE call: the dehydrated DAG in
//!   topological order, every level hashed as a batch (`lurk_hip_store_hydrate`: wide levels on the device, narrow ones on the host);
//! * [`ResidentStore`] - the same memo kept on the device across hydrations (`lurk_hip_store`): `append` hashes what has been interned
//!   since the last call, `digests` / `digests_dev` read it, `slot_preimages_dev` lays the digests out as a MultiFrame's slot preimages.
//!
//! Field elements cross as their canonical 32 bytes (`PrimeField::to_repr()`); a tag is `F::from(tag as u64)` (`src/tag.rs:99-101`).
//! A generic `impl<F: LurkField> StoreHasher<Tag, FWrap<F>> for HipStoreHasher` is four lines of `to_repr` / `from_repr` around these
//! methods and lives in lurk-beta (it needs its `Tag` and `FWrap` types).  Never compiled in the container this repository is built in.
use super::*;
use core::ffi::c_void;
use std::collections::HashMap;
use std::sync::Mutex;

pub type Digest = [u8; 32];

/// `F::from(tag as u64).to_repr()`
pub fn tag_to_field(tag: u16) -> Digest {
    let mut d = [0u8; 32];
    d[..2].copy_from_slice(&tag.to_le_bytes());
    d
}

/// `PoseidonCache<F>` over the library; `field_id` is one of `LURK_FIELD_*`.
pub struct HipPoseidonCache {
    pub field_id: c_int,
    memo: Mutex<HashMap<Vec<u8>, Digest>>,
}
impl HipPoseidonCache {
    pub fn new(field_id: c_int) -> Self {
        Self { field_id, memo: Mutex::new(HashMap::new()) }
    }
    fn hash(&self, arity: usize, preimage: &[Digest]) -> Result<Digest, Error> {
        assert_eq!(preimage.len(), arity);
        let key: Vec<u8> = preimage.concat();
        if let Some(d) = self.memo.lock().unwrap().get(&key) {
            return Ok(*d);
        }
        let mut out = [0u8; 32];
        check(unsafe { lurk_hip_poseidon_hash_host(self.field_id, arity as c_int, key.as_ptr().cast(), 1, out.as_mut_ptr().cast()) })?;
        self.memo.lock().unwrap().insert(key, out);
        Ok(out)
    }
    pub fn hash3(&self, p: &[Digest; 3]) -> Result<Digest, Error> { self.hash(3, p) }
    pub fn hash4(&self, p: &[Digest; 4]) -> Result<Digest, Error> { self.hash(4, p) }
    pub fn hash6(&self, p: &[Digest; 6]) -> Result<Digest, Error> { self.hash(6, p) }
    pub fn hash8(&self, p: &[Digest; 8]) -> Result<Digest, Error> { self.hash(8, p) }
    /// n preimages of one arity at once (device): what a caller that already holds a level of the DAG should use
    pub fn hash_many(&self, arity: usize, preimages: &[Digest]) -> Result<Vec<Digest>, Error> {
        assert!(matches!(arity, 3 | 4 | 6 | 8) && preimages.len() % arity == 0);
        let n = preimages.len() / arity;
        let mut out = vec![[0u8; 32]; n];
        check(unsafe { lurk_hip_poseidon_batch(self.field_id, arity as c_int, preimages.as_ptr().cast(), n, out.as_mut_ptr().cast()) })?;
        Ok(out)
    }
}

/// `StoreHasher<Tag, FWrap<F>>` (`store_core.rs:10-14`) with `store.rs:29-78`'s layouts; a tagged pointer is `(tag, digest)`.
pub struct HipStoreHasher {
    pub cache: HipPoseidonCache,
}
impl HipStoreHasher {
    pub fn new(field_id: c_int) -> Self {
        Self { cache: HipPoseidonCache::new(field_id) }
    }
    /// 2 pointers -> hash4(tag_a, h_a, tag_b, h_b); 3 -> hash6; 4 -> hash8 (`store.rs:30-66`)
    pub fn hash_ptrs(&self, ptrs: &[(u16, Digest)]) -> Result<Digest, Error> {
        let pre: Vec<Digest> = ptrs.iter().flat_map(|(t, h)| [tag_to_field(*t), *h]).collect();
        match ptrs.len() {
            2 => self.cache.hash(4, &pre),
            3 => self.cache.hash(6, &pre),
            4 => self.cache.hash(8, &pre),
            _ => unimplemented!("hash_ptrs takes 2, 3 or 4 pointers (store.rs:66)"),
        }
    }
    /// hash4(d1, t2, d2, d3) (`store.rs:75-77`)
    pub fn hash_compact(&self, d1: Digest, t2: u16, d2: Digest, d3: Digest) -> Result<Digest, Error> {
        self.cache.hash4(&[d1, tag_to_field(t2), d2, d3])
    }
    /// hash3(secret, tag, hash) (`store.rs:70-73`)
    pub fn hash_commitment(&self, secret: Digest, payload: (u16, Digest)) -> Result<Digest, Error> {
        self.cache.hash3(&[secret, tag_to_field(payload.0), payload.1])
    }
}

/// `hydrate_z_cache` in one call: `nodes` in topological order (children first; `kind` = `LURK_NODE_*`), `values` the atoms' and
/// secrets' field elements; returns the digest of every node and the depth of the DAG.
pub fn hydrate(field_id: c_int, nodes: &[lurk_hip_store_node], values: &[Digest]) -> Result<(Vec<Digest>, usize), Error> {
    let mut out = vec![[0u8; 32]; nodes.len()];
    let mut levels = 0usize;
    check(unsafe {
        lurk_hip_store_hydrate(field_id, nodes.as_ptr(), nodes.len(), values.as_ptr().cast(), values.len(), out.as_mut_ptr().cast(), &mut levels)
    })?;
    Ok((out, levels))
}

/// One element of a hash slot's preimage by description, as `allocate_slot` (`/root/reference/src/lem/circuit.rs:265-308`) builds it:
/// `Val::Pointer` -> [`SlotElem::tag`], [`SlotElem::digest`] of the pointer's node; `Val::Num` -> [`SlotElem::digest`] of the node that
/// holds the value; `Val::Boolean` -> [`SlotElem::constant`]; an absent slot -> [`SlotElem::ZERO`] for every element of its preimage.
pub type SlotElem = lurk_hip_slot_elem;
impl SlotElem {
    pub const ZERO: Self = Self { kind: LURK_SLOT_ELEM_ZERO as u32, arg: 0 };
    pub fn tag(node: u32) -> Self {
        Self { kind: LURK_SLOT_ELEM_TAG as u32, arg: node }
    }
    pub fn digest(node: u32) -> Self {
        Self { kind: LURK_SLOT_ELEM_DIGEST as u32, arg: node }
    }
    pub fn constant(value: u32) -> Self {
        Self { kind: LURK_SLOT_ELEM_CONST as u32, arg: value }
    }
}

/// What [`ResidentStore::info`] reports.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct StoreInfo {
    pub field_id: c_int,
    pub n_nodes: usize,
    pub levels: usize,
    /// Poseidon hashes performed since creation, host and device: the number of non-atom nodes, each hashed once
    pub hashes_done: usize,
    pub capacity: usize,
    pub device: c_int,
}

/// `StoreCore`'s digest memo (`z_cache`, `/root/reference/src/lem/store_core.rs:199-248`) resident on the device: node ids are assigned
/// in append order, an append hashes the new nodes only (`hydrate_z_cache`, `:256-269`, between two proofs), and the digests are
/// handed on where the device wants them.  The header's section "the store, resident on the device" has the contract.
pub struct ResidentStore {
    handle: *mut lurk_hip_store,
}
unsafe impl Send for ResidentStore {}
unsafe impl Sync for ResidentStore {} // appends are serialised by the library; the readers only read the handle

impl ResidentStore {
    /// `reserve_nodes`: the initial capacity, 0 = the library's default; it grows on demand
    pub fn new(field_id: c_int, reserve_nodes: usize) -> Result<Self, Error> {
        let mut handle = core::ptr::null_mut();
        check(unsafe { lurk_hip_store_create(&mut handle, field_id, reserve_nodes) })?;
        Ok(Self { handle })
    }
    pub fn info(&self) -> Result<StoreInfo, Error> {
        let mut i = StoreInfo { field_id: 0, n_nodes: 0, levels: 0, hashes_done: 0, capacity: 0, device: 0 };
        check(unsafe {
            lurk_hip_store_info(self.handle, &mut i.field_id, &mut i.n_nodes, &mut i.levels, &mut i.hashes_done, &mut i.capacity, &mut i.device)
        })?;
        Ok(i)
    }
    /// The nodes interned since the last append, children as GLOBAL node ids below the node's own, `value` an index into `values`
    /// (this call's atoms and secrets).  Returns the id of the first new node; nothing but what narrow levels need crosses PCIe.
    /// A refused append (the message names the offending record) leaves the store as it was.
    pub fn append(&self, nodes: &[lurk_hip_store_node], values: &[Digest]) -> Result<usize, Error> {
        let mut first = 0usize;
        check(unsafe {
            lurk_hip_store_append(self.handle, nodes.as_ptr(), nodes.len(), values.as_ptr().cast(), values.len(), &mut first, core::ptr::null_mut())
        })?;
        Ok(first)
    }
    /// The same, with the digests of the new nodes copied back (what fills `z_cache` on the host).
    pub fn append_with_digests(&self, nodes: &[lurk_hip_store_node], values: &[Digest]) -> Result<(usize, Vec<Digest>), Error> {
        let mut first = 0usize;
        let mut out = vec![[0u8; 32]; nodes.len()];
        check(unsafe {
            lurk_hip_store_append(self.handle, nodes.as_ptr(), nodes.len(), values.as_ptr().cast(), values.len(), &mut first, out.as_mut_ptr().cast())
        })?;
        Ok((first, out))
    }
    /// The digests of the nodes `ids` (host arrays); an id that is not a node is refused by index.
    pub fn digests(&self, ids: &[u32]) -> Result<Vec<Digest>, Error> {
        let mut out = vec![[0u8; 32]; ids.len()];
        check(unsafe { lurk_hip_store_digests(self.handle, ids.as_ptr(), ids.len(), out.as_mut_ptr().cast()) })?;
        Ok(out)
    }
    /// # Safety
    /// `d_ids`: `m` node ids on the device, `d_out`: `m * 32` bytes on the device.  Stream-ordered; an id that is not a node gives zeros.
    pub unsafe fn digests_dev(&self, d_ids: *const u32, m: usize, d_out: *mut c_void, stream: *mut c_void) -> Result<(), Error> {
        check(lurk_hip_store_digests_dev(self.handle, d_ids, m, d_out, stream))
    }
    /// # Safety
    /// `d_elems`: `n_elems` descriptors on the device, `d_out`: `n_elems * 32` bytes on the device - the `d_preimages` of
    /// `lurk_hip_frames_witness_dev` for one slot type when the descriptors are those of its slots in frame-major order.  Stream-ordered.
    pub unsafe fn slot_preimages_dev(&self, d_elems: *const SlotElem, n_elems: usize, as_mont: bool, d_out: *mut c_void, stream: *mut c_void) -> Result<(), Error> {
        check(lurk_hip_store_slot_preimages_dev(self.handle, d_elems, n_elems, as_mont as c_int, d_out, stream))
    }
}
impl Drop for ResidentStore {
    fn drop(&mut self) {
        unsafe { lurk_hip_store_destroy(self.handle) };
    }
}
