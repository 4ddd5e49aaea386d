// trie.hip - the sparse Poseidon trie of coprocessor::trie (/root/reference/src/coprocessor/trie/mod.rs), resident on the device:
// bulk build from sorted (key, value) pairs, lookup / insert proofs for batches of keys, and the two verifiers.
//
// Arity 8, height H <= 85.  A key's path is the low 3 H bits of its canonical value read as H 3-bit digits, top digit first (:589-608);
// those 3 H bits are its PATH VALUE and the keys of a built trie are sorted by it.  A node at depth d is then the contiguous range of
// keys that share their top d digits; its hash lives at the index of the range's first key in level array d (H arrays of n elements:
// level 0 holds the root at index 0, the children of level H - 1 are the leaf values).  Absent children are the empty roots (:464-481).
//
// Every hashing kernel keeps ONE Poseidon state per lane (nine radix-2^29 elements, poseidon29.cuh: the permutation of the batch
// hasher, not a second one) and reads the constant image from LDS as wave-uniform broadcasts exactly as poseidon_batch_kernel does:
// all lanes of a wave are in the same round of the same hash, whatever node or proof they work on.
//
//   trie_order_check_kernel   one lane per key: reduced? path(i) > path(i - 1)?  digits shared with key i - 1 (one byte per key)
//   trie_build_chain_kernel   phase 1, no cooperation: a lane hashes from its leaf up to the depth below which its key is alone
//   trie_build_level_kernel   phase 2, one launch per remaining depth, bottom-up: the first key of every range of >= 2 keys gathers the
//                             (up to 8) children by binary search over the sorted keys and hashes them
//   trie_prove_lookup_kernel  one lane per query: top-down walk by binary search, emits the H preimages and the value
//   trie_prove_insert_kernel  the same walk, then modify_value_at_path (:778-800): H dependent hashes bottom-up in the same lane
//   trie_verify_lookup_kernel / trie_verify_insert_kernel   LookupProof::verify (:349-362) / InsertProof::verify (:383-424), one lane
//                             per proof, the first failing check latched and the chain run to its end
//   trie_chain_*_kernel       a chain of m DEPENDENT inserts in O(H) launches (see "the chain" below): the updates ordered per depth by
//                             (prefix, sequence index), then one hashing launch per depth, bottom-up, one update per lane
//
// What the root-addressed child map (trie_nodes.hip) shares with this unit lives in trie_common.cuh: element loads and stores, the digit and
// range helpers, TrieHasher and the image staging, the handle, the host checks, and trie_chain_run - the chain's ordering and level launches.
#include <memory>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "trie_common.cuh"

namespace lurk {

enum : unsigned { TRIE_BAD_NOT_REDUCED = 1, TRIE_BAD_OUT_OF_ORDER = 2, TRIE_BAD_DUPLICATE = 3 };

struct TrieStatus {
    unsigned long long first_bad;  // (index << 2 | kind) of the lowest offending key, all ones if none
    unsigned int max_shared;       // the most digits two neighbouring keys share: phase 2 starts at that depth
    unsigned int pad;
};

// ---- order check -----------------------------------------------------------------------------------------------------------------------
template <class P>
__global__ __launch_bounds__(TRIE_BLOCK) void trie_order_check_kernel(const uint32_t* __restrict__ keys, size_t n, int height, uint8_t* __restrict__ shared_out,
                                                                       TrieStatus* status) {
    const size_t i = (size_t)blockIdx.x * TRIE_BLOCK + threadIdx.x;
    unsigned shared = 0;
    if (i < n) {
        const Fe<P> k = ld_fe<P>(reinterpret_cast<const uint4*>(keys + i * 8));
        unsigned kind = fe_canonical_ge_mod<P>(k.l) ? TRIE_BAD_NOT_REDUCED : 0u;
        if (i > 0) {
            const Fe<P> p = ld_fe<P>(reinterpret_cast<const uint4*>(keys + (i - 1) * 8));
            // the highest bit in which the two path values differ decides the order and how many digits they share
            int hb = -1;
            bool less = false;
#pragma unroll
            for (int w = 7; w >= 0; w--) {
                const uint32_t m = trie_low_mask(w, 3 * height), a = k.l[w] & m, b = p.l[w] & m;
                if (hb < 0 && a != b) {
                    hb = 32 * w + 31 - __clz((int)(a ^ b));
                    less = a < b;
                }
            }
            if (hb < 0) {
                shared = (unsigned)height;
                if (!kind) kind = TRIE_BAD_DUPLICATE;
            } else {
                shared = (unsigned)((3 * height - 1 - hb) / 3);
                if (less && !kind) kind = TRIE_BAD_OUT_OF_ORDER;
            }
        }
        shared_out[i] = (uint8_t)shared;
        if (kind) atomicMin(&status->first_bad, ((unsigned long long)i << 2) | kind);
    }
    // one atomic per wave for the deepest shared prefix
    unsigned m = shared;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, off));
    if ((threadIdx.x & 63) == 0 && m) atomicMax(&status->max_shared, m);
}

// ---- build -----------------------------------------------------------------------------------------------------------------------------
// Phase 1.  Key i shares at most stop = max(shared[i], shared[i + 1]) digits with any other key, so at every depth > stop its subtree holds
// this key alone: siblings are empty roots and the lane chains the hashes from the leaf up to depth stop + 1 by itself.
template <class P>
__global__ __launch_bounds__(TRIE_BLOCK) __attribute__((amdgpu_waves_per_eu(2, 2))) void trie_build_chain_kernel(TrieView t, const uint4* __restrict__ img,
                                                                                                               int img_vec4, int rf, int rp) {
    extern __shared__ uint4 lds[];
    trie_stage_image(lds, img, img_vec4);
    const TrieHasher<P> h(lds, rf, rp);
    const size_t i = (size_t)blockIdx.x * TRIE_BLOCK + threadIdx.x;
    if (i >= t.n) return;  // no barrier follows
    const int a = i > 0 ? (int)t.shared[i] : -1, b = i + 1 < t.n ? (int)t.shared[i + 1] : -1;
    const int stop = a > b ? a : b;
    const uint32_t* key = t.keys + i * 8;
    Fe<P> cur = ld_fe<P>(t.values + 2 * i);
    for (int d = t.height - 1; d > stop; d--) {  // every live lane of the wave is at the same depth
        const int digit = trie_key_digit(key, t.height, d);
        const F29<P> e = h.in(ld_fe<P>(t.empty + 2 * (t.height - 1 - d))), c = h.in(cur);
        F29<P> s[TRIE_T];
        s[0] = h.tag();
#pragma unroll
        for (int j = 0; j < 8; j++) {
#pragma unroll
            for (int k = 0; k < 9; k++) s[j + 1].l[k] = j == digit ? c.l[k] : e.l[k];
        }
        cur = h.run(s);
        st_fe<P>(t.levels + ((size_t)d * t.n + i) * 2, cur);
    }
}

// Phase 2, depth d.  Key i opens a node of >= 2 keys at depth d when it does not share d digits with key i - 1 and does with key i + 1.  It
// finds the end of the range (the first key that leaves the prefix) and the boundaries between the eight digits by binary search, reads
// each child from level d + 1 (written by phase 1 or by the previous launch; at d = H - 1 the children are the values), hashes, stores.
template <class P>
__global__ __launch_bounds__(TRIE_BLOCK) __attribute__((amdgpu_waves_per_eu(2, 2))) void trie_build_level_kernel(TrieView t, int d, const uint4* __restrict__ img,
                                                                                                               int img_vec4, int rf, int rp) {
    extern __shared__ uint4 lds[];
    __shared__ unsigned short opener[TRIE_BLOCK];
    __shared__ unsigned wave_nodes[TRIE_BLOCK / 64];
    const size_t self = (size_t)blockIdx.x * TRIE_BLOCK + threadIdx.x;
    const bool opens = self + 1 < t.n && (int)t.shared[self + 1] >= d && (self == 0 || (int)t.shared[self] < d);
    // the block's nodes are compacted onto its first lanes: at most every other key opens a node, mostly far fewer, and a wave pays a
    // whole hash for a single live lane
    const unsigned long long mask = __ballot(opens);
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) wave_nodes[wave] = (unsigned)__popcll(mask);
    __syncthreads();
    unsigned before = 0, nodes = 0;
#pragma unroll
    for (unsigned w = 0; w < TRIE_BLOCK / 64; w++) {
        if (w < wave) before += wave_nodes[w];
        nodes += wave_nodes[w];
    }
    if (nodes == 0) return;  // the whole block: one with no node at this depth does not stage the image
    if (opens) opener[before + (unsigned)__popcll(mask & ((1ull << lane) - 1ull))] = (unsigned short)threadIdx.x;
    trie_stage_image(lds, img, img_vec4);  // its barrier publishes opener[] too
    const TrieHasher<P> h(lds, rf, rp);
    if (threadIdx.x >= nodes) return;
    const size_t i = (size_t)blockIdx.x * TRIE_BLOCK + opener[threadIdx.x];
    const Fe<P> ki = ld_fe<P>(reinterpret_cast<const uint4*>(t.keys + i * 8));
    size_t lo = i + 2, end = t.n;  // key i + 1 shares the prefix
    while (lo < end) {
        const size_t mid = lo + ((end - lo) >> 1);
        if (trie_same_prefix(ki.l, t.keys + mid * 8, t.height, d)) lo = mid + 1;
        else end = mid;
    }
    const Fe<P> emp = ld_fe<P>(t.empty + 2 * (t.height - 1 - d));
    const uint4* below = d == t.height - 1 ? t.values : t.levels + (size_t)(d + 1) * t.n * 2;
    F29<P> s[TRIE_T];
    s[0] = h.tag();
    size_t b = i;
#pragma unroll
    for (int c = 0; c < 8; c++) {
        const size_t nb = c < 7 ? trie_digit_lower_bound(t.keys, b, end, t.height, d, c + 1) : end;
        Fe<P> x = emp;
        if (nb > b) x = ld_fe<P>(below + 2 * b);
        s[c + 1] = h.in(x);
        b = nb;
    }
    st_fe<P>(t.levels + ((size_t)d * t.n + i) * 2, h.run(s));
}

// ---- prove -----------------------------------------------------------------------------------------------------------------------------
// The walk of prove_lookup_at_path (:725-743) over the level arrays: at depth d the node on the key's path is the range [lo, hi) of keys
// that share the key's top d digits; emit(d, c, x) receives its eight children.  Once the range is empty the walk has left the populated
// part of the trie and the remaining preimages are the empty ones.  Returns the selected entry of the last preimage (0 = absent).
template <class P, class Emit>
__device__ __forceinline__ Fe<P> trie_walk(const TrieView& t, const uint32_t* key, Emit&& emit) {
    size_t lo = 0, hi = t.n;
    Fe<P> found = fe_zero<P>();
    for (int d = 0; d < t.height; d++) {
        const Fe<P> emp = ld_fe<P>(t.empty + 2 * (t.height - 1 - d));
        const uint4* below = d == t.height - 1 ? t.values : t.levels + (size_t)(d + 1) * t.n * 2;
        const int kd = trie_key_digit(key, t.height, d);
        size_t b = lo, nlo = lo, nhi = lo;
        found = emp;
#pragma unroll 1
        for (int c = 0; c < 8; c++) {
            const size_t nb = c < 7 ? trie_digit_lower_bound(t.keys, b, hi, t.height, d, c + 1) : hi;
            Fe<P> x = emp;
            if (nb > b) x = ld_fe<P>(below + 2 * b);
            emit(d, c, x);
            if (c == kd) {
                nlo = b;
                nhi = nb;
                found = x;
            }
            b = nb;
        }
        lo = nlo;
        hi = nhi;
    }
    return found;
}

template <class P>
__global__ __launch_bounds__(TRIE_BLOCK) void trie_prove_lookup_kernel(TrieView t, const uint32_t* __restrict__ keys, size_t m, uint4* __restrict__ paths,
                                                                        uint4* __restrict__ values) {
    const size_t q = (size_t)blockIdx.x * TRIE_BLOCK + threadIdx.x;
    if (q >= m) return;
    uint4* out = paths + q * (size_t)t.height * 16;
    const Fe<P> v = trie_walk<P>(t, keys + q * 8, [&](int d, int c, const Fe<P>& x) { st_fe<P>(out + ((size_t)d * 8 + c) * 2, x); });
    st_fe<P>(values + 2 * q, v);
}

template <class P>
__global__ __launch_bounds__(TRIE_BLOCK) __attribute__((amdgpu_waves_per_eu(2, 2))) void trie_prove_insert_kernel(TrieView t, const uint32_t* __restrict__ keys,
                                                                                                                const uint4* __restrict__ new_values, size_t m,
                                                                                                                uint4* old_paths, uint4* new_paths,
                                                                                                                uint4* __restrict__ old_values,
                                                                                                                uint4* __restrict__ new_roots, const uint4* __restrict__ img,
                                                                                                                int img_vec4, int rf, int rp) {
    extern __shared__ uint4 lds[];
    trie_stage_image(lds, img, img_vec4);
    const TrieHasher<P> h(lds, rf, rp);
    const size_t q = (size_t)blockIdx.x * TRIE_BLOCK + threadIdx.x;
    if (q >= m) return;  // no barrier follows
    const uint32_t* key = keys + q * 8;
    uint4* oldp = old_paths + q * (size_t)t.height * 16;
    uint4* newp = new_paths + q * (size_t)t.height * 16;
    const Fe<P> v = trie_walk<P>(t, key, [&](int d, int c, const Fe<P>& x) { st_fe<P>(oldp + ((size_t)d * 8 + c) * 2, x); });
    st_fe<P>(old_values + 2 * q, v);
    // modify_value_at_path: replace the entry bottom-up and re-hash (the lane reads back the old preimages it has just written)
    Fe<P> cur = ld_fe<P>(new_values + 2 * q);
    for (int d = t.height - 1; d >= 0; d--) {
        const int digit = trie_key_digit(key, t.height, d);
        F29<P> s[TRIE_T];
        s[0] = h.tag();
#pragma unroll
        for (int j = 0; j < 8; j++) {
            Fe<P> x = ld_fe<P>(oldp + ((size_t)d * 8 + j) * 2);
            if (j == digit) x = cur;
            st_fe<P>(newp + ((size_t)d * 8 + j) * 2, x);
            s[j + 1] = h.in(x);
        }
        cur = h.run(s);
    }
    st_fe<P>(new_roots + 2 * q, cur);
}

// ---- verify ----------------------------------------------------------------------------------------------------------------------------
// LookupProof::verify for one proof: 0 = accepted, k + 1 = the hash of preimage k is not the expected node (level 0: the root),
// H + 1 = the selected leaf entry is not the value.  A preimage element that is not reduced fails its level: the hash is a function of
// the residue, and x and x + p must not both open a node.  No early exit: the first failure latches and the chain runs on.
template <class P>
__device__ __forceinline__ unsigned trie_verify_chain(const TrieHasher<P>& h, int height, const uint32_t* key, const uint4* path, const uint4* root, const uint4* value) {
    unsigned code = 0;
#pragma unroll 1
    for (int d = 0; d < height; d++) {
        F29<P> s[TRIE_T];
        s[0] = h.tag();
        bool bad = false;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const Fe<P> x = ld_fe<P>(path + ((size_t)d * 8 + j) * 2);
            bad = bad || fe_canonical_ge_mod<P>(x.l);
            s[j + 1] = h.in(x);
        }
        const Fe<P> got = h.run(s);
        // the expected node is read after the hash (the root, or the selected entry of the preimage above): nothing but the verdict is
        // carried across the permutation
        const Fe<P> want = ld_fe<P>(d == 0 ? root : path + ((size_t)(d - 1) * 8 + trie_key_digit(key, height, d - 1)) * 2);
        if (code == 0 && (bad || !fe_eq<P>(got, want))) code = (unsigned)d + 1;
    }
    const Fe<P> leaf = ld_fe<P>(path + ((size_t)(height - 1) * 8 + trie_key_digit(key, height, height - 1)) * 2);
    if (code == 0 && !fe_eq<P>(leaf, ld_fe<P>(value))) code = (unsigned)height + 1;
    return code;
}

// failures are counted with one atomic add per wave
__device__ __forceinline__ void trie_count_failures(bool failed, unsigned long long* n_failed) {
    const unsigned long long mask = __ballot(failed);
    if ((threadIdx.x & 63) == 0 && mask) atomicAdd(n_failed, (unsigned long long)__popcll(mask));
}

template <class P>
__global__ __launch_bounds__(TRIE_BLOCK) __attribute__((amdgpu_waves_per_eu(2, 2))) void trie_verify_lookup_kernel(int height, const uint4* __restrict__ roots,
                                                                                                                 size_t root_stride, const uint32_t* __restrict__ keys,
                                                                                                                 const uint4* __restrict__ values,
                                                                                                                 const uint4* __restrict__ paths, size_t m,
                                                                                                                 uint32_t* __restrict__ codes, unsigned long long* n_failed,
                                                                                                                 const uint4* __restrict__ img, int img_vec4, int rf, int rp) {
    extern __shared__ uint4 lds[];
    trie_stage_image(lds, img, img_vec4);
    const TrieHasher<P> h(lds, rf, rp);
    const size_t q = (size_t)blockIdx.x * TRIE_BLOCK + threadIdx.x;
    unsigned code = 0;
    if (q < m) {
        code = trie_verify_chain<P>(h, height, keys + q * 8, paths + q * (size_t)height * 16, roots + 2 * q * root_stride, values + 2 * q);
        codes[q] = code;
    }
    trie_count_failures(code != 0, n_failed);
}

// InsertProof::verify in the reference's order, the first failing check wins: the old proof (1 .. H + 1), then at every level the two
// preimages equal or different in at most one position (0x100 + level + 1), then the new proof (0x200 + 1 .. H + 1).
template <class P>
__global__ __launch_bounds__(TRIE_BLOCK) __attribute__((amdgpu_waves_per_eu(2, 2))) void trie_verify_insert_kernel(
    int height, const uint4* __restrict__ old_roots, const uint4* __restrict__ new_roots, size_t root_stride, const uint32_t* __restrict__ keys,
    const uint4* __restrict__ old_values, const uint4* __restrict__ new_values, const uint4* __restrict__ old_paths, const uint4* __restrict__ new_paths, size_t m,
    uint32_t* __restrict__ codes, unsigned long long* n_failed, const uint4* __restrict__ img, int img_vec4, int rf, int rp) {
    extern __shared__ uint4 lds[];
    trie_stage_image(lds, img, img_vec4);
    const TrieHasher<P> h(lds, rf, rp);
    const size_t q = (size_t)blockIdx.x * TRIE_BLOCK + threadIdx.x;
    unsigned code = 0;
    if (q < m) {
        const uint4* oldp = old_paths + q * (size_t)height * 16;
        const uint4* newp = new_paths + q * (size_t)height * 16;
        unsigned c_old = 0, c_new = 0, c_diff = 0;
#pragma unroll 1
        for (int which = 0; which < 2; which++) {  // one hash site for both chains
            const unsigned c = trie_verify_chain<P>(h, height, keys + q * 8, which ? newp : oldp, (which ? new_roots : old_roots) + 2 * q * root_stride,
                                                    (which ? new_values : old_values) + 2 * q);
            if (which) c_new = c;
            else c_old = c;
        }
#pragma unroll 1
        for (int d = 0; d < height; d++) {
            int differ = 0;
#pragma unroll 1
            for (int j = 0; j < 8; j++)
                differ += !fe_eq<P>(ld_fe<P>(oldp + ((size_t)d * 8 + j) * 2), ld_fe<P>(newp + ((size_t)d * 8 + j) * 2));
            if (differ > 1 && c_diff == 0) c_diff = 0x100u + (unsigned)d + 1;
        }
        code = c_old ? c_old : c_diff ? c_diff : c_new ? 0x200u + c_new : 0u;
        codes[q] = code;
    }
    trie_count_failures(code != 0, n_failed);
}

// ---- the chain: m dependent inserts, level-synchronously -------------------------------------------------------------------------------
// Update i = (key_i, value_i) is applied to T_i and leaves T_{i+1} (insert_at_path, :760-776).  At the node that update i passes at depth d
// the preimage it FINDS is the node's preimage in T_0 with every child entry c replaced by the new hash, one level down, of the latest
// EARLIER update that went through child c; the preimage it LEAVES has its own child's new hash put in as well, and its new hash at depth d
// is the hash of that.  So depth d needs depth d + 1 only: H hashing launches for m * H hashes, whatever m is.
//
// "The latest earlier update through child c" is three binary searches.  ord[e] (e = 1 .. D) holds the updates sorted by (top-e-digit
// prefix, sequence index): a stable sort of ord[e - 1] by skey = 8 * label + digit e - 1, where label[q] is the position at which the
// depth e - 1 node of entry q starts in ord[e - 1].  Along ord[e] the sorted skey[e] is non-decreasing and the updates through child c of
// the node that starts at `node` are the run skey == 8 * node + c, in sequence order.  The splitting stops at the first depth D at which
// every node holds updates of ONE path value: below it the order no longer changes and only an update's own child has an earlier setter,
// its predecessor in the run.  (Random keys: D ~ 2 log8(m).  Two keys that share 84 digits: D = 84.)
constexpr size_t TRIE_CHAIN_MAX = (size_t)1 << 28;  // 8 * label + digit is a 32-bit sort key

// do the keys a and b (memory) have one path value?  a < b in path order?
__device__ __forceinline__ int trie_path_cmp(const uint32_t* a, const uint32_t* b, int height) {
    const uint4 alo = reinterpret_cast<const uint4*>(a)[0], ahi = reinterpret_cast<const uint4*>(a)[1];
    const uint4 blo = reinterpret_cast<const uint4*>(b)[0], bhi = reinterpret_cast<const uint4*>(b)[1];
    const uint32_t aw[8] = {alo.x, alo.y, alo.z, alo.w, ahi.x, ahi.y, ahi.z, ahi.w}, bw[8] = {blo.x, blo.y, blo.z, blo.w, bhi.x, bhi.y, bhi.z, bhi.w};
    int r = 0;
#pragma unroll
    for (int w = 7; w >= 0; w--) {
        const uint32_t m = trie_low_mask(w, 3 * height), x = aw[w] & m, y = bw[w] & m;
        if (r == 0 && x != y) r = x < y ? -1 : 1;
    }
    return r;
}

__device__ __forceinline__ size_t trie_u32_lower_bound(const uint32_t* a, size_t lo, size_t hi, uint32_t v) {
    while (lo < hi) {
        const size_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the sort key of entry q of the order at depth d (ord == nullptr: the identity, every label 0), the entry itself as the sort's value, and
// *mixed = 1 if a node of depth d holds two path values (then depth d has to be split)
__global__ __launch_bounds__(TRIE_BLOCK) void trie_chain_key_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ ord,
                                                                    const uint32_t* __restrict__ label, size_t m, int height, int d, uint32_t* __restrict__ skey,
                                                                    uint32_t* __restrict__ entry, uint32_t* mixed) {
    const size_t q = (size_t)blockIdx.x * TRIE_BLOCK + threadIdx.x;
    if (q >= m) return;
    const uint32_t u = ord ? ord[q] : (uint32_t)q, lab = ord ? label[q] : 0u;
    skey[q] = lab * 8u + (uint32_t)trie_key_digit(keys + (size_t)u * 8, height, d);
    entry[q] = u;
    if (q > 0 && (ord ? label[q - 1] : 0u) == lab) {
        const uint32_t v = ord ? ord[q - 1] : (uint32_t)(q - 1);
        if (trie_path_cmp(keys + (size_t)u * 8, keys + (size_t)v * 8, height) != 0) *mixed = 1u;
    }
}

// label[q] = where the run of skey[q] starts: the node of entry q at the next depth
__global__ __launch_bounds__(TRIE_BLOCK) void trie_chain_label_kernel(const uint32_t* __restrict__ skey, size_t m, uint32_t* __restrict__ label) {
    const size_t q = (size_t)blockIdx.x * TRIE_BLOCK + threadIdx.x;
    if (q < m) label[q] = (uint32_t)trie_u32_lower_bound(skey, 0, q, skey[q]);
}

struct TrieChainLevel {
    const uint32_t* keys;   // m x 8 words
    const uint32_t* ord;    // the order at depth min(d + 1, D); nullptr = the identity (D = 0)
    const uint32_t* skey;   // the sorted keys of ord when d + 1 <= D, else nullptr: then label
    const uint32_t* label;  // where the run (one path value) of entry q starts
    const uint4* below;     // m x 32 B by update: the new hashes of depth d + 1 (at d = H - 1: the new values)
    uint4* here;            // m x 32 B by update: the new hashes of depth d (at d = 0: the roots)
    uint4* old_paths;       // m x H x 8 elements: the preimages of T_0 on entry, patched in place when store_old
    uint4* new_paths;       // or nullptr
    uint4* old_values;      // or nullptr; written at d = H - 1
    size_t m;
    int height, d, store_old;
};

// One update per lane, in the order of the depth below, so that the updates of one node are neighbours.  Nothing but the update's index
// is carried across the permutation.
template <class P>
__global__ __launch_bounds__(TRIE_BLOCK) __attribute__((amdgpu_waves_per_eu(2, 2))) void trie_chain_level_kernel(TrieChainLevel a, const uint4* __restrict__ img,
                                                                                                               int img_vec4, int rf, int rp) {
    extern __shared__ uint4 lds[];
    trie_stage_image(lds, img, img_vec4);
    const TrieHasher<P> h(lds, rf, rp);
    const size_t q = (size_t)blockIdx.x * TRIE_BLOCK + threadIdx.x;
    if (q >= a.m) return;  // no barrier follows
    const size_t i = a.ord ? a.ord[q] : q;
    const int own = trie_key_digit(a.keys + i * 8, a.height, a.d);
    uint4* oldp = a.old_paths + (i * (size_t)a.height + (size_t)a.d) * 16;
    uint4* newp = a.new_paths ? a.new_paths + (i * (size_t)a.height + (size_t)a.d) * 16 : nullptr;
    const size_t node = a.skey ? (size_t)(a.skey[q] >> 3) : (size_t)a.label[q];
    F29<P> s[TRIE_T];
    s[0] = h.tag();
    size_t b = node;  // the run of child 0 starts where the node does
#pragma unroll
    for (int c = 0; c < 8; c++) {
        size_t setter = a.m;  // none
        if (a.skey) {
            const size_t nb = trie_u32_lower_bound(a.skey, b, a.m, (uint32_t)(node * 8 + c + 1));
            if (c == own) {
                if (q > b) setter = a.ord[q - 1];
            } else if (nb > b) {
                const size_t r = trie_u32_lower_bound(a.ord, b, nb, (uint32_t)i);  // the run is in sequence order
                if (r > b) setter = a.ord[r - 1];
            }
            b = nb;
        } else if (c == own && q > node) {
            setter = a.ord ? a.ord[q - 1] : q - 1;
        }
        Fe<P> x;
        if (setter < a.m) {
            x = ld_fe<P>(a.below + 2 * setter);
            if (a.store_old) st_fe<P>(oldp + 2 * c, x);
        } else {
            x = ld_fe<P>(oldp + 2 * c);
        }
        if (c == own) {
            if (a.old_values && a.d == a.height - 1) st_fe<P>(a.old_values + 2 * i, x);
            x = ld_fe<P>(a.below + 2 * i);
        }
        if (newp) st_fe<P>(newp + 2 * c, x);
        s[c + 1] = h.in(x);
    }
    st_fe<P>(a.here + 2 * i, h.run(s));
}

// out_trie: the pairs of T_m.  last[q] = 1 where entry q of the final order is the last update of its path value; upd[] = those entries,
// compacted (they are in path order); every one of them looks itself up among the trie's keys, every key of the trie among them.
__global__ __launch_bounds__(TRIE_BLOCK) void trie_chain_last_kernel(const uint32_t* __restrict__ label, size_t m, uint32_t* __restrict__ last) {
    const size_t q = (size_t)blockIdx.x * TRIE_BLOCK + threadIdx.x;
    if (q < m) last[q] = (q + 1 == m || (label && label[q + 1] != label[q])) ? 1u : 0u;
}
__global__ __launch_bounds__(TRIE_BLOCK) void trie_chain_compact_kernel(const uint32_t* __restrict__ ord, const uint32_t* __restrict__ last,
                                                                        const uint32_t* __restrict__ last_incl, size_t m, uint32_t* __restrict__ upd) {
    const size_t q = (size_t)blockIdx.x * TRIE_BLOCK + threadIdx.x;
    if (q < m && last[q]) upd[last_incl[q] - 1] = ord ? ord[q] : (uint32_t)q;
}
// for update entry r: below[r] = the trie's keys with a smaller path value, present[r] = 1 if the trie holds its path value
__global__ __launch_bounds__(TRIE_BLOCK) void trie_chain_locate_kernel(const uint32_t* __restrict__ tkeys, size_t n, const uint32_t* __restrict__ ukeys,
                                                                       const uint32_t* __restrict__ upd, size_t nu, int height, uint32_t* __restrict__ below,
                                                                       uint32_t* __restrict__ present) {
    const size_t r = (size_t)blockIdx.x * TRIE_BLOCK + threadIdx.x;
    if (r >= nu) return;
    const uint32_t* key = ukeys + (size_t)upd[r] * 8;
    size_t lo = 0, hi = n;
    while (lo < hi) {
        const size_t mid = lo + ((hi - lo) >> 1);
        if (trie_path_cmp(tkeys + mid * 8, key, height) < 0) lo = mid + 1;
        else hi = mid;
    }
    below[r] = (uint32_t)lo;
    present[r] = lo < n && trie_path_cmp(tkeys + lo * 8, key, height) == 0 ? 1u : 0u;
}
// lanes 0 .. n - 1: the trie's pairs that no update replaces; lanes n .. n + nu - 1: the last update of every path value
__global__ __launch_bounds__(TRIE_BLOCK) void trie_chain_merge_kernel(const uint32_t* __restrict__ tkeys, const uint4* __restrict__ tvalues, size_t n,
                                                                      const uint32_t* __restrict__ ukeys, const uint4* __restrict__ uvalues,
                                                                      const uint32_t* __restrict__ upd, size_t nu, const uint32_t* __restrict__ below,
                                                                      const uint32_t* __restrict__ present, const uint32_t* __restrict__ present_incl, int height,
                                                                      uint4* __restrict__ out_keys, uint4* __restrict__ out_values) {
    const size_t g = (size_t)blockIdx.x * TRIE_BLOCK + threadIdx.x;
    if (g >= n + nu) return;
    const uint4 *k, *v;
    size_t pos;
    if (g < n) {
        const uint32_t* key = tkeys + g * 8;
        size_t lo = 0, hi = nu;  // the update entries with a smaller path value
        while (lo < hi) {
            const size_t mid = lo + ((hi - lo) >> 1);
            if (trie_path_cmp(ukeys + (size_t)upd[mid] * 8, key, height) < 0) lo = mid + 1;
            else hi = mid;
        }
        if (lo < nu && trie_path_cmp(ukeys + (size_t)upd[lo] * 8, key, height) == 0) return;  // replaced
        pos = g + lo - (lo ? present_incl[lo - 1] : 0u);
        k = reinterpret_cast<const uint4*>(key);
        v = tvalues + 2 * g;
    } else {
        const size_t r = g - n;
        pos = r + below[r] - (present_incl[r] - present[r]);
        k = reinterpret_cast<const uint4*>(ukeys + (size_t)upd[r] * 8);
        v = uvalues + 2 * (size_t)upd[r];
    }
    out_keys[2 * pos] = k[0];
    out_keys[2 * pos + 1] = k[1];
    out_values[2 * pos] = v[0];
    out_values[2 * pos + 1] = v[1];
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------
static std::string trie_refusal(const char* what, unsigned long long first_bad) {
    const unsigned long long i = first_bad >> 2;
    const std::string k = what + std::string(" ") + std::to_string(i);
    switch ((unsigned)(first_bad & 3)) {
        case TRIE_BAD_NOT_REDUCED: return k + " is not reduced modulo the field order";
        case TRIE_BAD_OUT_OF_ORDER: return k + " is out of order: its path is below that of key " + std::to_string(i - 1);
        default: return k + " has a duplicate path: its low 3 * height bits equal those of key " + std::to_string(i - 1);
    }
}

// the chain's ordering and hashing launches (trie_common.cuh): shared by lurk_hip_trie_insert_chain_dev and the root-addressed chain
void trie_chain_run(int field_id, int H, const void* d_keys32, const void* d_values32, size_t m, uint4* oldp, bool store_old, void* d_new_paths,
                    void* d_old_values32, void* d_roots32, const std::function<void()>& walk, TrieChainScratch& sc, hipStream_t s) {
    with_field(field_id, [&](auto F) {
        using P = decltype(F);
        const uint32_t* keys = (const uint32_t*)d_keys32;
        const unsigned grid = div_up(m, TRIE_BLOCK);
        // scratch: the orders (2 x 4 B per update and depth that is split, H at the most), two rows of new hashes, the sort's storage, and the
        // preimages of T_0 when the caller does not take the old paths
        sc.orders.alloc(2 * (size_t)H * m * 4);
        sc.work.alloc(4 * m * 4);
        sc.hashes.alloc(2 * m * 32);
        sc.flag.alloc(4);
        sc.m = m;
        DevBuf &work = sc.work, &hashes = sc.hashes, &flag = sc.flag, &temp = sc.temp;
        uint32_t *skey_in = work.as<uint32_t>(), *entry_in = skey_in + m, *label = skey_in + 2 * m, *aux = skey_in + 3 * m;
        auto ord_at = [&](int e) { return sc.ord_at(e); };
        auto skey_at = [&](int e) { return sc.skey_at(e); };
        unsigned end_bit = 4;
        while (end_bit < 32 && ((size_t)1 << end_bit) < 8 * m) end_bit++;
        size_t sort_bytes = 0, scan_bytes = 0;
        LURK_HIP_CHECK(rocprim::radix_sort_pairs(nullptr, sort_bytes, skey_in, skey_in, entry_in, entry_in, (unsigned)m, 0, end_bit, s));
        LURK_HIP_CHECK(rocprim::inclusive_scan(nullptr, scan_bytes, aux, aux, m, rocprim::plus<uint32_t>(), s));
        temp.alloc(sort_bytes > scan_bytes ? sort_bytes : scan_bytes);
        LURK_HIP_CHECK(hipMemsetAsync(label, 0, m * 4, s));

        // the orders, top-down: split depth d while one of its nodes holds two path values
        int& D = sc.D;
        D = 0;
        {
            ProfScope ps("trie_chain_order", s);
            for (; D < H; D++) {
                LURK_HIP_CHECK(hipMemsetAsync(flag.p, 0, 4, s));
                hipLaunchKernelGGL(trie_chain_key_kernel, dim3(grid), dim3(TRIE_BLOCK), 0, s, keys, D ? ord_at(D) : (const uint32_t*)nullptr, label, m, H, D, skey_in,
                                   entry_in, flag.as<uint32_t>());
                LURK_HIP_CHECK(hipGetLastError());
                uint32_t mixed = 0;
                LURK_HIP_CHECK(hipMemcpyAsync(&mixed, flag.p, 4, hipMemcpyDeviceToHost, s));
                LURK_HIP_CHECK(hipStreamSynchronize(s));
                if (!mixed) break;
                size_t bytes = temp.bytes;
                LURK_HIP_CHECK(rocprim::radix_sort_pairs(temp.p, bytes, skey_in, skey_at(D + 1), entry_in, ord_at(D + 1), (unsigned)m, 0, end_bit, s));
                hipLaunchKernelGGL(trie_chain_label_kernel, dim3(grid), dim3(TRIE_BLOCK), 0, s, skey_at(D + 1), m, label);
                LURK_HIP_CHECK(hipGetLastError());
            }
        }
        walk();
        // the hashes, bottom-up
        const TrieLaunch L(field_id, s);
        auto kern = trie_chain_level_kernel<P>;
        allow_dynamic_lds((const void*)kern, (int)L.lds_bytes);
        const uint4* below = (const uint4*)d_values32;
        {
            ProfScope ps("trie_chain_levels", s);
            for (int d = H - 1; d >= 0; d--) {
                TrieChainLevel a;
                a.keys = keys;
                const int e = d + 1 < D ? d + 1 : D;
                a.ord = e ? ord_at(e) : nullptr;
                a.skey = d + 1 <= D ? skey_at(e) : nullptr;
                a.label = label;
                a.below = below;
                a.here = d == 0 && d_roots32 ? (uint4*)d_roots32 : hashes.as<uint4>() + (size_t)(d & 1) * m * 2;
                a.old_paths = oldp;
                a.new_paths = (uint4*)d_new_paths;
                a.old_values = (uint4*)d_old_values32;
                a.m = m;
                a.height = H;
                a.d = d;
                a.store_old = store_old ? 1 : 0;
                hipLaunchKernelGGL(kern, dim3(grid), dim3(TRIE_BLOCK), L.lds_bytes, s, a, L.img, L.vec4, L.rf, L.rp);
                LURK_HIP_CHECK(hipGetLastError());
                below = a.here;
            }
        }
    });
}

}  // namespace lurk

using namespace lurk;

extern "C" {

int lurk_hip_trie_path_digits(int field_id, int height, const void* keys32, size_t n, uint8_t* digits) {
    return host_guarded([&] {
        require_trie_field(field_id);
        require_trie_height(height);
        LURK_REQUIRE(n == 0 || (keys32 && digits), "null buffer");
        int nbits = 256;
        with_field(field_id, [&](auto F) { nbits = decltype(F)::NBITS; });
        for (size_t i = 0; i < n; i++) {
            uint32_t k[8];
            memcpy(k, (const char*)keys32 + i * 32, 32);  // caller memory carries no alignment promise
            for (int w = 0; w < 8; w++) k[w] &= trie_low_mask(w, nbits);  // to_le_bits() has NUM_BITS bits: no reduced key has more
            for (int d = 0; d < height; d++) digits[i * (size_t)height + d] = (uint8_t)trie_key_digit(k, height, d);
        }
    });
}

int lurk_hip_trie_build_dev(lurk_hip_trie** out, int field_id, int height, const void* d_keys32, const void* d_values32, size_t n, void* stream) {
    return guarded([&] {
        LURK_REQUIRE(out, "null output handle");
        *out = nullptr;
        require_trie_field(field_id);
        require_trie_height(height);
        LURK_REQUIRE(n == 0 || (d_keys32 && d_values32), "null buffer");
        hipStream_t s = (hipStream_t)stream;
        const std::vector<uint64_t>& er = trie_empty_roots(field_id);
        auto t = std::make_unique<lurk_hip_trie>();  // everything below is released with it if a later step fails
        t->field_id = field_id;
        t->height = height;
        t->device = current_device();
        t->n = n;
        if (n > 0) {
            // the one checking pass, over the caller's keys: nothing else is allocated before it has passed
            t->shared.alloc(n);
            DevBuf status(sizeof(TrieStatus));
            LURK_HIP_CHECK(hipMemsetAsync(status.p, 0xff, 8, s));
            LURK_HIP_CHECK(hipMemsetAsync((char*)status.p + 8, 0, 8, s));
            with_field(field_id, [&](auto F) {
                using P = decltype(F);
                ProfScope ps("trie_order_check", s);
                hipLaunchKernelGGL((trie_order_check_kernel<P>), dim3(div_up(n, TRIE_BLOCK)), dim3(TRIE_BLOCK), 0, s, (const uint32_t*)d_keys32, n, height,
                                   t->shared.as<uint8_t>(), status.as<TrieStatus>());
                LURK_HIP_CHECK(hipGetLastError());
            });
            TrieStatus st;
            LURK_HIP_CHECK(hipMemcpyAsync(&st, status.p, sizeof(st), hipMemcpyDeviceToHost, s));
            LURK_HIP_CHECK(hipStreamSynchronize(s));
            if (st.first_bad != ~0ull) throw HipFailure{LURK_HIP_ERR_INVALID_ARG, trie_refusal("key", st.first_bad)};
            const int deepest = (int)st.max_shared < height - 1 ? (int)st.max_shared : height - 1;

            t->keys.alloc(n * 32);
            t->values.alloc(n * 32);
            t->levels.alloc((size_t)height * n * 32);
            t->empty.alloc((size_t)(height + 1) * 32);
            LURK_HIP_CHECK(hipMemcpyAsync(t->keys.p, d_keys32, n * 32, hipMemcpyDeviceToDevice, s));
            LURK_HIP_CHECK(hipMemcpyAsync(t->values.p, d_values32, n * 32, hipMemcpyDeviceToDevice, s));
            LURK_HIP_CHECK(hipMemcpyAsync(t->empty.p, er.data(), (size_t)(height + 1) * 32, hipMemcpyHostToDevice, s));
            const TrieLaunch L(field_id, s);
            const TrieView v = t->view();
            with_field(field_id, [&](auto F) {
                using P = decltype(F);
                auto chain = trie_build_chain_kernel<P>;
                auto level = trie_build_level_kernel<P>;
                allow_dynamic_lds((const void*)chain, (int)L.lds_bytes);
                allow_dynamic_lds((const void*)level, (int)L.lds_bytes);
                ProfScope ps("trie_build", s);
                hipLaunchKernelGGL(chain, dim3(div_up(n, TRIE_BLOCK)), dim3(TRIE_BLOCK), L.lds_bytes, s, v, L.img, L.vec4, L.rf, L.rp);
                LURK_HIP_CHECK(hipGetLastError());
                // a node of >= 2 keys exists at depth d only if two neighbours share d digits: nothing to do below `deepest` (n == 1: none at all)
                for (int d = n > 1 ? deepest : -1; d >= 0; d--) {
                    hipLaunchKernelGGL(level, dim3(div_up(n, TRIE_BLOCK)), dim3(TRIE_BLOCK), L.lds_bytes, s, v, d, L.img, L.vec4, L.rf, L.rp);
                    LURK_HIP_CHECK(hipGetLastError());
                }
            });
            LURK_HIP_CHECK(hipMemcpyAsync(t->root, t->levels.p, 32, hipMemcpyDeviceToHost, s));
        } else {
            t->empty.alloc((size_t)(height + 1) * 32);
            LURK_HIP_CHECK(hipMemcpyAsync(t->empty.p, er.data(), (size_t)(height + 1) * 32, hipMemcpyHostToDevice, s));
            memcpy(t->root, er.data() + 4 * (size_t)height, 32);
        }
        LURK_HIP_CHECK(hipStreamSynchronize(s));
        *out = t.release();
    });
}

int lurk_hip_trie_root(const lurk_hip_trie* t, void* root32) {
    return host_guarded([&] {
        LURK_REQUIRE(t && root32, "null argument");
        memcpy(root32, t->root, 32);
    });
}

int lurk_hip_trie_info(const lurk_hip_trie* t, int* field_id, int* height, size_t* n, int* device) {
    return host_guarded([&] {
        LURK_REQUIRE(t, "null trie handle");
        if (field_id) *field_id = t->field_id;
        if (height) *height = t->height;
        if (n) *n = t->n;
        if (device) *device = t->device;
    });
}

int lurk_hip_trie_destroy(lurk_hip_trie* t) {
    return host_guarded([&] {
        if (!t) return;
        DeviceGuard g(t->device);
        delete t;
    });
}

int lurk_hip_trie_prove_lookup_dev(const lurk_hip_trie* t, const void* d_keys32, size_t m, void* d_paths, void* d_values32, void* stream) {
    return guarded([&] {
        require_trie_here(t);
        if (m == 0) return;
        LURK_REQUIRE(d_keys32 && d_paths && d_values32, "null buffer");
        hipStream_t s = (hipStream_t)stream;
        const TrieView v = t->view();
        with_field(t->field_id, [&](auto F) {
            using P = decltype(F);
            ProfScope ps("trie_prove_lookup", s);
            hipLaunchKernelGGL((trie_prove_lookup_kernel<P>), dim3(div_up(m, TRIE_BLOCK)), dim3(TRIE_BLOCK), 0, s, v, (const uint32_t*)d_keys32, m, (uint4*)d_paths,
                               (uint4*)d_values32);
            LURK_HIP_CHECK(hipGetLastError());
        });
    });
}

int lurk_hip_trie_prove_insert_dev(const lurk_hip_trie* t, const void* d_keys32, const void* d_new_values32, size_t m, void* d_old_paths, void* d_new_paths,
                                   void* d_old_values32, void* d_new_roots32, void* stream) {
    return guarded([&] {
        require_trie_here(t);
        if (m == 0) return;
        LURK_REQUIRE(d_keys32 && d_new_values32 && d_old_paths && d_new_paths && d_old_values32 && d_new_roots32, "null buffer");
        const size_t path_bytes = m * (size_t)t->height * 256;
        const char *a = (const char*)d_old_paths, *b = (const char*)d_new_paths;
        LURK_REQUIRE(a + path_bytes <= b || b + path_bytes <= a, "d_old_paths and d_new_paths overlap");
        hipStream_t s = (hipStream_t)stream;
        const TrieLaunch L(t->field_id, s);
        const TrieView v = t->view();
        with_field(t->field_id, [&](auto F) {
            using P = decltype(F);
            auto kern = trie_prove_insert_kernel<P>;
            allow_dynamic_lds((const void*)kern, (int)L.lds_bytes);
            ProfScope ps("trie_prove_insert", s);
            hipLaunchKernelGGL(kern, dim3(div_up(m, TRIE_BLOCK)), dim3(TRIE_BLOCK), L.lds_bytes, s, v, (const uint32_t*)d_keys32, (const uint4*)d_new_values32, m,
                               (uint4*)d_old_paths, (uint4*)d_new_paths, (uint4*)d_old_values32, (uint4*)d_new_roots32, L.img, L.vec4, L.rf, L.rp);
            LURK_HIP_CHECK(hipGetLastError());
        });
    });
}

int lurk_hip_trie_verify_lookup_dev(int field_id, int height, const void* d_roots32, size_t root_stride, const void* d_keys32, const void* d_values32,
                                    const void* d_paths, size_t m, uint32_t* d_codes, uint64_t* n_failed, void* stream) {
    return guarded([&] {
        require_trie_field(field_id);
        require_trie_height(height);
        LURK_REQUIRE(root_stride <= 1, "root_stride is 0 (one root for every proof) or 1 (one root per proof)");
        LURK_REQUIRE(n_failed, "null n_failed");
        *n_failed = 0;
        if (m == 0) return;
        LURK_REQUIRE(d_roots32 && d_keys32 && d_values32 && d_paths && d_codes, "null buffer");
        hipStream_t s = (hipStream_t)stream;
        with_field(field_id, [&](auto F) {
            using P = decltype(F);
            std::vector<uint32_t> host;
            require_reduced_dev<P>(d_keys32, m, "key", host, s);
            require_reduced_dev<P>(d_values32, m, "value", host, s);
            const TrieLaunch L(field_id, s);
            DevBuf count(8);
            LURK_HIP_CHECK(hipMemsetAsync(count.p, 0, 8, s));
            auto kern = trie_verify_lookup_kernel<P>;
            allow_dynamic_lds((const void*)kern, (int)L.lds_bytes);
            {
                ProfScope ps("trie_verify_lookup", s);
                hipLaunchKernelGGL(kern, dim3(div_up(m, TRIE_BLOCK)), dim3(TRIE_BLOCK), L.lds_bytes, s, height, (const uint4*)d_roots32, root_stride,
                                   (const uint32_t*)d_keys32, (const uint4*)d_values32, (const uint4*)d_paths, m, d_codes, count.as<unsigned long long>(), L.img, L.vec4,
                                   L.rf, L.rp);
                LURK_HIP_CHECK(hipGetLastError());
            }
            LURK_HIP_CHECK(hipMemcpyAsync(n_failed, count.p, 8, hipMemcpyDeviceToHost, s));
            LURK_HIP_CHECK(hipStreamSynchronize(s));
        });
    });
}

int lurk_hip_trie_verify_insert_dev(int field_id, int height, const void* d_old_roots32, const void* d_new_roots32, size_t root_stride, const void* d_keys32,
                                    const void* d_old_values32, const void* d_new_values32, const void* d_old_paths, const void* d_new_paths, size_t m,
                                    uint32_t* d_codes, uint64_t* n_failed, void* stream) {
    return guarded([&] {
        require_trie_field(field_id);
        require_trie_height(height);
        LURK_REQUIRE(root_stride <= 1, "root_stride is 0 (one root pair for every proof) or 1 (one pair per proof)");
        LURK_REQUIRE(n_failed, "null n_failed");
        *n_failed = 0;
        if (m == 0) return;
        LURK_REQUIRE(d_old_roots32 && d_new_roots32 && d_keys32 && d_old_values32 && d_new_values32 && d_old_paths && d_new_paths && d_codes, "null buffer");
        hipStream_t s = (hipStream_t)stream;
        with_field(field_id, [&](auto F) {
            using P = decltype(F);
            std::vector<uint32_t> host;
            require_reduced_dev<P>(d_keys32, m, "key", host, s);
            require_reduced_dev<P>(d_old_values32, m, "old value", host, s);
            require_reduced_dev<P>(d_new_values32, m, "new value", host, s);
            const TrieLaunch L(field_id, s);
            DevBuf count(8);
            LURK_HIP_CHECK(hipMemsetAsync(count.p, 0, 8, s));
            auto kern = trie_verify_insert_kernel<P>;
            allow_dynamic_lds((const void*)kern, (int)L.lds_bytes);
            {
                ProfScope ps("trie_verify_insert", s);
                hipLaunchKernelGGL(kern, dim3(div_up(m, TRIE_BLOCK)), dim3(TRIE_BLOCK), L.lds_bytes, s, height, (const uint4*)d_old_roots32, (const uint4*)d_new_roots32,
                                   root_stride, (const uint32_t*)d_keys32, (const uint4*)d_old_values32, (const uint4*)d_new_values32, (const uint4*)d_old_paths,
                                   (const uint4*)d_new_paths, m, d_codes, count.as<unsigned long long>(), L.img, L.vec4, L.rf, L.rp);
                LURK_HIP_CHECK(hipGetLastError());
            }
            LURK_HIP_CHECK(hipMemcpyAsync(n_failed, count.p, 8, hipMemcpyDeviceToHost, s));
            LURK_HIP_CHECK(hipStreamSynchronize(s));
        });
    });
}

int lurk_hip_trie_insert_chain_dev(const lurk_hip_trie* t, const void* d_keys32, const void* d_values32, size_t m, void* d_old_paths, void* d_new_paths,
                                   void* d_old_values32, void* d_roots32, lurk_hip_trie** out_trie, void* stream) {
    return guarded([&] {
        require_trie_here(t);
        LURK_REQUIRE(d_old_paths || d_new_paths || d_old_values32 || d_roots32 || out_trie, "no output asked for: every output pointer is null");
        LURK_REQUIRE(m <= TRIE_CHAIN_MAX, "a chain holds at most 2^28 updates");
        hipStream_t s = (hipStream_t)stream;
        const int H = t->height;
        lurk_hip_trie* grown = nullptr;
        if (m == 0) {
            if (out_trie) {
                nested_ok(lurk_hip_trie_build_dev(&grown, t->field_id, H, t->n ? t->keys.p : nullptr, t->n ? t->values.p : nullptr, t->n, stream));
                *out_trie = grown;
            }
            return;
        }
        LURK_REQUIRE(d_keys32 && d_values32, "null buffer");
        const size_t path_bytes = m * (size_t)H * 256;
        if (d_old_paths && d_new_paths) {
            const char *a = (const char*)d_old_paths, *b = (const char*)d_new_paths;
            LURK_REQUIRE(a + path_bytes <= b || b + path_bytes <= a, "d_old_paths and d_new_paths overlap");
        }
        with_field(t->field_id, [&](auto F) {
            using P = decltype(F);
            std::vector<uint32_t> host;  // nothing is launched or allocated on the device before both have passed
            require_reduced_dev<P>(d_keys32, m, "key", host, s);
            require_reduced_dev<P>(d_values32, m, "value", host, s);
        });
        {
            const uint32_t* keys = (const uint32_t*)d_keys32;
            const unsigned grid = div_up(m, TRIE_BLOCK);
            // the preimages of T_0 when the caller does not take the old paths
            DevBuf old_scratch, value_scratch;
            if (!d_old_paths) old_scratch.alloc(path_bytes);
            if (!d_old_values32) value_scratch.alloc(m * 32);
            uint4* oldp = d_old_paths ? (uint4*)d_old_paths : old_scratch.as<uint4>();
            const TrieView v = t->view();
            // the preimages of T_0 along every update's path (and, for now, the values of T_0)
            auto walk = [&] {
                with_field(t->field_id, [&](auto F) {
                    using P = decltype(F);
                    ProfScope ps("trie_chain_walk", s);
                    hipLaunchKernelGGL((trie_prove_lookup_kernel<P>), dim3(grid), dim3(TRIE_BLOCK), 0, s, v, keys, m, oldp,
                                       d_old_values32 ? (uint4*)d_old_values32 : value_scratch.as<uint4>());
                    LURK_HIP_CHECK(hipGetLastError());
                });
            };
            TrieChainScratch sc;
            trie_chain_run(t->field_id, H, d_keys32, d_values32, m, oldp, d_old_paths != nullptr, d_new_paths, d_old_values32, d_roots32, walk, sc, s);
            const int D = sc.D;
            uint32_t *skey_in = sc.work.as<uint32_t>(), *entry_in = skey_in + m, *label = skey_in + 2 * m, *aux = skey_in + 3 * m;
            DevBuf& temp = sc.temp;
            auto ord_at = [&](int e) { return sc.ord_at(e); };
            if (out_trie) {
                // T_m's pairs: the last update of every path value (ord[D] is in path order) merged with the pairs of t that none replaces
                const uint32_t* ord = D ? ord_at(D) : nullptr;
                uint32_t *last = skey_in, *last_incl = entry_in, *upd = aux;
                size_t bytes = temp.bytes;
                hipLaunchKernelGGL(trie_chain_last_kernel, dim3(grid), dim3(TRIE_BLOCK), 0, s, label, m, last);
                LURK_HIP_CHECK(hipGetLastError());
                LURK_HIP_CHECK(rocprim::inclusive_scan(temp.p, bytes, last, last_incl, m, rocprim::plus<uint32_t>(), s));
                hipLaunchKernelGGL(trie_chain_compact_kernel, dim3(grid), dim3(TRIE_BLOCK), 0, s, ord, last, last_incl, m, upd);
                LURK_HIP_CHECK(hipGetLastError());
                uint32_t nu32 = 0, replaced = 0;
                LURK_HIP_CHECK(hipMemcpyAsync(&nu32, last_incl + (m - 1), 4, hipMemcpyDeviceToHost, s));
                LURK_HIP_CHECK(hipStreamSynchronize(s));
                const size_t nu = nu32, n = t->n;
                uint32_t *tbelow = skey_in, *present = entry_in, *present_incl = label;  // last / last_incl / label are done with (nu <= m)
                hipLaunchKernelGGL(trie_chain_locate_kernel, dim3(div_up(nu, TRIE_BLOCK)), dim3(TRIE_BLOCK), 0, s, v.keys, n, keys, upd, nu, H, tbelow, present);
                LURK_HIP_CHECK(hipGetLastError());
                bytes = temp.bytes;
                LURK_HIP_CHECK(rocprim::inclusive_scan(temp.p, bytes, present, present_incl, nu, rocprim::plus<uint32_t>(), s));
                LURK_HIP_CHECK(hipMemcpyAsync(&replaced, present_incl + (nu - 1), 4, hipMemcpyDeviceToHost, s));
                LURK_HIP_CHECK(hipStreamSynchronize(s));
                const size_t total = n + nu - replaced;
                DevBuf mkeys(total * 32), mvalues(total * 32);
                hipLaunchKernelGGL(trie_chain_merge_kernel, dim3(div_up(n + nu, TRIE_BLOCK)), dim3(TRIE_BLOCK), 0, s, v.keys, v.values, n, keys, (const uint4*)d_values32, upd,
                                   nu, tbelow, present, present_incl, H, mkeys.as<uint4>(), mvalues.as<uint4>());
                LURK_HIP_CHECK(hipGetLastError());
                nested_ok(lurk_hip_trie_build_dev(&grown, t->field_id, H, mkeys.p, mvalues.p, total, stream));
            }
            LURK_HIP_CHECK(hipStreamSynchronize(s));
        }
        if (out_trie) *out_trie = grown;
    });
}
}
