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
#include <memory>

#include "common.hpp"
#include "dispatch.hpp"
#include "poseidon.cuh"
#include "poseidon29.cuh"

namespace lurk {

constexpr int TRIE_BLOCK = 256;
constexpr int TRIE_MAX_HEIGHT = 85;  // 3 * 85 = 255 path bits: lurk-beta's StandardTrie (:43)
constexpr int TRIE_T = 9;            // arity 8

enum : unsigned { TRIE_BAD_NOT_REDUCED = 1, TRIE_BAD_OUT_OF_ORDER = 2, TRIE_BAD_DUPLICATE = 3 };

struct TrieStatus {
    unsigned long long first_bad;  // (index << 2 | kind) of the lowest offending key, all ones if none
    unsigned int max_shared;       // the most digits two neighbouring keys share: phase 2 starts at that depth
    unsigned int pad;
};

struct TrieView {
    const uint32_t* keys;   // n x 8 words, canonical, strictly increasing path values
    const uint4* values;    // n x 32 B
    uint4* levels;          // H disjoint arrays of n x 32 B: level d at levels + d * n * 2
    const uint4* empty;     // (H + 1) x 32 B: empty[h] = root of the empty subtree of height h (empty[0] = 0, the empty element)
    const uint8_t* shared;  // shared[i] = digits key i shares with key i - 1 (i >= 1)
    size_t n;
    int height;
};

template <class P>
__device__ __forceinline__ Fe<P> ld_fe(const uint4* p) {
    const uint4 lo = p[0], hi = p[1];
    Fe<P> x;
    x.l[0] = lo.x; x.l[1] = lo.y; x.l[2] = lo.z; x.l[3] = lo.w;
    x.l[4] = hi.x; x.l[5] = hi.y; x.l[6] = hi.z; x.l[7] = hi.w;
    return x;
}
template <class P>
__device__ __forceinline__ void st_fe(uint4* p, const Fe<P>& d) {
    p[0] = make_uint4(d.l[0], d.l[1], d.l[2], d.l[3]);
    p[1] = make_uint4(d.l[4], d.l[5], d.l[6], d.l[7]);
}

// digit d (0 = top) of the path of height `height`, from the key's eight 32-bit words in memory
LURK_HD int trie_key_digit(const uint32_t* key, int height, int d) {
    const int bit = 3 * (height - 1 - d), w = bit >> 5, sh = bit & 31;
    uint32_t v = key[w] >> sh;
    if (sh > 29) v |= key[w + 1] << (32 - sh);  // bit <= 252: a digit that straddles two words starts below word 7
    return (int)(v & 7u);
}
// word w of the mask of a value's low `nbits` bits / of everything from bit `lowbit` up
LURK_HD uint32_t trie_low_mask(int w, int nbits) {
    const int r = nbits - 32 * w;
    return r >= 32 ? 0xffffffffu : r <= 0 ? 0u : ((1u << r) - 1u);
}
LURK_HD uint32_t trie_high_mask(int w, int lowbit) { return ~trie_low_mask(w, lowbit); }

// do the keys a (registers) and b (memory) share their top d digits?
__device__ __forceinline__ bool trie_same_prefix(const uint32_t* a, const uint32_t* b, int height, int d) {
    const uint4 lo = reinterpret_cast<const uint4*>(b)[0], hi = reinterpret_cast<const uint4*>(b)[1];
    const uint32_t bw[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    uint32_t diff = 0;
#pragma unroll
    for (int w = 0; w < 8; w++) diff |= (a[w] ^ bw[w]) & trie_low_mask(w, 3 * height) & trie_high_mask(w, 3 * (height - d));
    return diff == 0;
}

// within [lo, hi), a range of keys that share their top d digits: the first key whose digit d is >= c
__device__ __forceinline__ size_t trie_digit_lower_bound(const uint32_t* keys, size_t lo, size_t hi, int height, int d, int c) {
    while (lo < hi) {
        const size_t mid = lo + ((hi - lo) >> 1);
        if (trie_key_digit(keys + mid * 8, height, d) < c) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// ---- the hash: one state per lane, the constant image in LDS ---------------------------------------------------------------------------
// only the permutation's part of the image is staged (the slot-witness post keys that follow it are not read here): 59 KiB at arity 8
static int trie_image_vec4(int rf, int rp) { return (PoseidonLayout<TRIE_T>(rf, rp).total() + 1) * (P29_STRIDE / 4); }

__device__ __forceinline__ void trie_stage_image(uint4* lds, const uint4* __restrict__ img, int img_vec4) {
    for (int i = threadIdx.x; i < img_vec4; i += TRIE_BLOCK) lds[i] = img[i];
    __syncthreads();
}

template <class P>
struct TrieHasher {
    const uint32_t* C;
    const uint32_t* mont2;
    int rf, rp;
    __device__ __forceinline__ TrieHasher(const uint4* lds, int rf_, int rp_)
        : C(reinterpret_cast<const uint32_t*>(lds)), mont2(C + (size_t)PoseidonLayout<TRIE_T>(rf_, rp_).total() * P29_STRIDE), rf(rf_), rp(rp_) {}
    __device__ __forceinline__ F29<P> tag() const { return ld_const29<P>(C); }
    __device__ __forceinline__ F29<P> in(const Fe<P>& x) const { return poseidon29_from_canonical<P>(x.l, mont2); }
    __device__ __forceinline__ Fe<P> run(F29<P>* s) const {
        poseidon29_permute<P, TRIE_T>(s, C, rf, rp);
        return poseidon29_to_canonical<P>(s[1]);
    }
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

// ---- host side -------------------------------------------------------------------------------------------------------------------------
static void require_trie_field(int field_id) {
    with_field(field_id, [](auto) {});  // "unknown field id"
}
static void require_trie_height(int height) {
    LURK_REQUIRE(height >= 1 && height <= TRIE_MAX_HEIGHT, "trie height must be 1 .. 85 (3 bits of the key per level)");
}

// empty[h] for h = 0 .. 85 (canonical, 4 x u64 each), by the library's host Poseidon: once per field
static const std::vector<uint64_t>& trie_empty_roots(int field_id) {
    static std::mutex mu;
    static std::map<int, std::vector<uint64_t>> cache;
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find(field_id);
    if (it == cache.end()) {
        std::vector<uint64_t> er((TRIE_MAX_HEIGHT + 1) * 4, 0);
        for (int hgt = 1; hgt <= TRIE_MAX_HEIGHT; hgt++) {
            uint64_t pre[8 * 4];
            for (int j = 0; j < 8; j++) memcpy(pre + 4 * j, er.data() + 4 * (hgt - 1), 32);
            nested_ok(lurk_hip_poseidon_hash_host(field_id, 8, pre, 1, er.data() + 4 * hgt));
        }
        it = cache.emplace(field_id, std::move(er)).first;
    }
    return it->second;
}

struct TrieLaunch {  // what every hashing launch needs
    const uint4* img;
    int vec4, rf, rp;
    size_t lds_bytes;
    TrieLaunch(int field_id, hipStream_t s) {
        const PoseidonImageView v = poseidon_image_view(field_id, 8, s);
        img = (const uint4*)v.img;
        rf = v.rf;
        rp = v.rp;
        vec4 = trie_image_vec4(rf, rp);
        LURK_REQUIRE(vec4 <= v.vec4, "the Poseidon image is shorter than its layout");
        lds_bytes = (size_t)vec4 * 16;
    }
};

static std::string trie_refusal(const char* what, unsigned long long first_bad) {
    const unsigned long long i = first_bad >> 2;
    const std::string k = what + std::string(" ") + std::to_string(i);
    switch ((unsigned)(first_bad & 3)) {
        case TRIE_BAD_NOT_REDUCED: return k + " is not reduced modulo the field order";
        case TRIE_BAD_OUT_OF_ORDER: return k + " is out of order: its path is below that of key " + std::to_string(i - 1);
        default: return k + " has a duplicate path: its low 3 * height bits equal those of key " + std::to_string(i - 1);
    }
}

// a verify call's device-resident keys / values, checked on the host before anything is launched: copies, no kernel
template <class P>
static void require_reduced_dev(const void* d_elems, size_t m, const char* what, std::vector<uint32_t>& host, hipStream_t s) {
    host.resize(m * 8);
    LURK_HIP_CHECK(hipMemcpyAsync(host.data(), d_elems, m * 32, hipMemcpyDeviceToHost, s));
    LURK_HIP_CHECK(hipStreamSynchronize(s));
    for (size_t i = 0; i < m; i++)
        if (fe_canonical_ge_mod<P>(host.data() + i * 8))
            throw HipFailure{LURK_HIP_ERR_INVALID_ARG, std::string(what) + " " + std::to_string(i) + " is not reduced modulo the field order"};
}

}  // namespace lurk

using namespace lurk;

struct lurk_hip_trie {
    int field_id = 0, height = 0, device = 0;
    size_t n = 0;
    DevBuf keys, values, levels, empty, shared;
    uint64_t root[4] = {0, 0, 0, 0};
    TrieView view() const {
        return TrieView{keys.as<uint32_t>(), values.as<uint4>(), levels.as<uint4>(), empty.as<uint4>(), shared.as<uint8_t>(), n, height};
    }
};

static void require_trie_here(const lurk_hip_trie* t) {
    LURK_REQUIRE(t, "null trie handle");
    LURK_REQUIRE(current_device() == t->device, "the trie lives on another device than the calling thread's current one");
}

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
}
