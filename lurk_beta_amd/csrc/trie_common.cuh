// trie_common.cuh - what the two trie units share: trie.hip (the handle-based trie: sorted pairs and level arrays) and trie_nodes.hip
// (the root-addressed child map).  Element loads and stores, the path digit, the one-state-per-lane hasher over the batch hasher's
// constant image, the handle itself, and the host-side checks both units make before they launch anything.
#pragma once

#include <functional>
#include <map>
#include <mutex>
#include <vector>

#include "common.hpp"
#include "dispatch.hpp"
#include "poseidon.cuh"
#include "poseidon29.cuh"

namespace lurk {

constexpr int TRIE_BLOCK = 256;
constexpr int TRIE_MAX_HEIGHT = 85;  // 3 * 85 = 255 path bits: lurk-beta's StandardTrie (:43)
constexpr int TRIE_T = 9;            // arity 8

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
inline int trie_image_vec4(int rf, int rp) { return (PoseidonLayout<TRIE_T>(rf, rp).total() + 1) * (P29_STRIDE / 4); }

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

// ---- host side -------------------------------------------------------------------------------------------------------------------------
inline void require_trie_field(int field_id) {
    with_field(field_id, [](auto) {});  // "unknown field id"
}
inline void require_trie_height(int height) {
    LURK_REQUIRE(height >= 1 && height <= TRIE_MAX_HEIGHT, "trie height must be 1 .. 85 (3 bits of the key per level)");
}

// empty[h] for h = 0 .. 85 (canonical, 4 x u64 each), by the library's host Poseidon: once per field
inline const std::vector<uint64_t>& trie_empty_roots(int field_id) {
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

// a call's device-resident keys / values, checked on the host before anything is launched: copies, no kernel
template <class P>
static void require_reduced_dev(const void* d_elems, size_t m, const char* what, std::vector<uint32_t>& host, hipStream_t s) {
    host.resize(m * 8);
    LURK_HIP_CHECK(hipMemcpyAsync(host.data(), d_elems, m * 32, hipMemcpyDeviceToHost, s));
    LURK_HIP_CHECK(hipStreamSynchronize(s));
    for (size_t i = 0; i < m; i++)
        if (fe_canonical_ge_mod<P>(host.data() + i * 8))
            throw HipFailure{LURK_HIP_ERR_INVALID_ARG, std::string(what) + " " + std::to_string(i) + " is not reduced modulo the field order"};
}

// ---- the chain of dependent inserts, shared by its two front ends (trie.hip) -------------------------------------------------------------
// Orders the m updates per depth and hashes bottom-up, one launch per depth, over `oldp`: m x H x 8 elements that hold, for every update,
// the preimages of T_0 along its path once `walk` has been called (it is called after the ordering launches and before the first hash).
// Every output but oldp may be null.  The scratch stays with the caller: the handle-based call builds T_m's pairs from the final order.
struct TrieChainScratch {
    DevBuf orders, work, hashes, flag, temp;
    size_t m = 0;
    int D = 0;  // the depths that were split
    uint32_t* ord_at(int e) const { return orders.as<uint32_t>() + (size_t)(2 * (e - 1)) * m; }  // e = 1 .. D
    uint32_t* skey_at(int e) const { return orders.as<uint32_t>() + (size_t)(2 * (e - 1) + 1) * m; }
};
void trie_chain_run(int field_id, int height, const void* d_keys32, const void* d_values32, size_t m, uint4* oldp, bool store_old, void* d_new_paths,
                    void* d_old_values32, void* d_roots32, const std::function<void()>& walk, TrieChainScratch& sc, hipStream_t s);

}  // namespace lurk

struct lurk_hip_trie {
    int field_id = 0, height = 0, device = 0;
    size_t n = 0;
    lurk::DevBuf keys, values, levels, empty, shared;
    uint64_t root[4] = {0, 0, 0, 0};
    lurk::TrieView view() const {
        return lurk::TrieView{keys.as<uint32_t>(), values.as<uint4>(), levels.as<uint4>(), empty.as<uint4>(), shared.as<uint8_t>(), n, height};
    }
};

inline void require_trie_here(const lurk_hip_trie* t) {
    LURK_REQUIRE(t, "null trie handle");
    LURK_REQUIRE(lurk::current_device() == t->device, "the trie lives on another device than the calling thread's current one");
}
