// trie_nodes.hip - the trie's child map resident on the device: InversePoseidonCache::a8 (src/hash.rs:116-166 of the reference) for one
// (field, height), written by register_hash (src/coprocessor/trie/mod.rs:453-458) and walked from ANY root (new_with_root, :566-576;
// prove_lookup_at_path, :725-743).  Every version of every trie lives in it; a trie is named by its root.
//
// The store is an open-addressing table (linear probing, a power-of-two slot count, at most half full) over three arrays in one allocation:
//   tags     8 B per slot    0 = empty, else the digest's low 64 bits (LURK_TRIE_NODES_TAG_BITS of them), forced non-zero
//   digests  32 B per slot   the node's hash, canonical
//   pre      256 B per slot  its eight children
// The slot a probe starts at comes from the digest's words 2 and 3, not from the tag.  Append-only; a reader compares the tag, then the whole
// digest, and probes on after a mismatch until it meets an empty slot.
//
// Inserting a batch is exact without any payload crossing workgroups inside a launch (the payload stores are plain stores, visible at the
// next launch; the only in-launch communication is the agent-scope atomicCAS on the tag word) and without a lane ever waiting for a slot:
//   trie_nodes_claim_kernel    one item per lane, probes from its home slot: CAS(tag, 0 -> mine) wins the slot, and the lane stores digest and
//                              children there; a slot that already holds MY tag is recorded as the item's provisional duplicate; any other
//                              tag: probe on
//   trie_nodes_confirm_kernel  the next launch: every provisional duplicate compares the slot's digest (stored in an earlier launch, or by the
//                              claimant in the launch before) with its own; a mismatch - one tag, two digests - goes on the overflow list
//   trie_nodes_serial_kernel   ONE lane inserts the overflow items one after the other with a full-digest probe (it sees its own stores)
// An item either claims a slot, or is proved equal to a stored digest, or is inserted serially against everything stored: n_nodes is the
// number of distinct digests whatever the interleaving.  Two items with one digest have one tag and one probe sequence; the first empty
// slot on it goes to one of them and the other meets that tag.
//
//   trie_nodes_walk_kernel     8 lanes per query: H dependent probes from the query's root; lane c copies child c of every node (256 B
//                              coalesced per level) and the next digest is child[digit], broadcast within the eight lanes.  No hash.
//   trie_nodes_get_kernel      8 lanes per digest: the batch form of InversePoseidonCache::get
//   register hashes with the batch hasher's own launch (poseidon_batch_device): wide kernel for small batches, one state per lane beyond
//   trie_nodes_insert_hash_kernel   prove_insert's modify_value_at_path over the old paths the walk has written, one update per lane
#include <cstdlib>
#include <memory>

#include "trie_common.cuh"

namespace lurk {

void poseidon_batch_device(int field_id, int arity, const void* d_pre, void* d_out, size_t n, int flags, hipStream_t s);  // poseidon.hip

constexpr uint32_t NODES_NONE = 0xffffffffu;

struct NodesView {
    unsigned long long* tags;
    uint4* digests;  // 2 per slot
    uint4* pre;      // 16 per slot
    size_t mask;     // slots - 1
    unsigned long long tag_mask;
};

__device__ __forceinline__ unsigned long long nodes_tag(const NodesView& t, const uint4& d0) {
    const unsigned long long g = (((unsigned long long)d0.y << 32) | d0.x) & t.tag_mask;
    return g ? g : 1ull;
}
__device__ __forceinline__ size_t nodes_home(const NodesView& t, const uint4& d0) { return (size_t)((((unsigned long long)d0.w << 32) | d0.z) & t.mask); }
__device__ __forceinline__ bool nodes_same(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1) {
    return ((a0.x ^ b0.x) | (a0.y ^ b0.y) | (a0.z ^ b0.z) | (a0.w ^ b0.w) | (a1.x ^ b1.x) | (a1.y ^ b1.y) | (a1.z ^ b1.z) | (a1.w ^ b1.w)) == 0;
}

// a reader's probe, in a launch after the one that stored: the slot of the digest, or all ones
__device__ __forceinline__ size_t nodes_find(const NodesView& t, const uint4& d0, const uint4& d1) {
    const unsigned long long tag = nodes_tag(t, d0);
    size_t slot = nodes_home(t, d0);
    for (size_t i = 0; i <= t.mask; i++, slot = (slot + 1) & t.mask) {
        const unsigned long long g = t.tags[slot];
        if (g == 0) break;
        if (g == tag && nodes_same(t.digests[2 * slot], t.digests[2 * slot + 1], d0, d1)) return slot;
    }
    return ~(size_t)0;
}

// ---- where a batch's items come from ---------------------------------------------------------------------------------------------------
// digest(i, d0, d1): false = item i is not a node to insert.  children(i, dst): the item's eight children to dst[0 .. 15].
struct NodesArraySrc {  // register: digests and preimages side by side
    const uint4* digests;
    const uint4* pre;
    __device__ __forceinline__ bool digest(size_t i, uint4& d0, uint4& d1) const {
        d0 = digests[2 * i];
        d1 = digests[2 * i + 1];
        return true;
    }
    __device__ __forceinline__ void children(size_t i, uint4* dst) const {
#pragma unroll
        for (int j = 0; j < 16; j++) dst[j] = pre[i * 16 + j];
    }
};
struct NodesRehashSrc {  // growth: the occupied slots of the old arrays
    NodesView old;
    __device__ __forceinline__ bool digest(size_t i, uint4& d0, uint4& d1) const {
        if (old.tags[i] == 0) return false;
        d0 = old.digests[2 * i];
        d1 = old.digests[2 * i + 1];
        return true;
    }
    __device__ __forceinline__ void children(size_t i, uint4* dst) const {
#pragma unroll
        for (int j = 0; j < 16; j++) dst[j] = old.pre[i * 16 + j];
    }
};
// the new paths of m inserts: item q * H + d is the node update q leaves at depth d.  Its preimage is row d of the new path; its hash is
// the root the update leaves (d = 0) or the entry of row d - 1 that the key selects - the hash the insert has just computed.
struct NodesPathSrc {
    const uint32_t* keys;
    const uint4* paths;
    const uint4* roots;
    const uint32_t* status;  // or nullptr; a query with a non-zero status registers nothing
    int height;
    __device__ __forceinline__ bool digest(size_t i, uint4& d0, uint4& d1) const {
        const size_t q = i / (size_t)height;
        const int d = (int)(i % (size_t)height);
        if (status && status[q]) return false;
        const uint4* at = d == 0 ? roots + 2 * q : paths + ((q * (size_t)height + (size_t)(d - 1)) * 8 + (size_t)trie_key_digit(keys + q * 8, height, d - 1)) * 2;
        d0 = at[0];
        d1 = at[1];
        return true;
    }
    __device__ __forceinline__ void children(size_t i, uint4* dst) const {
#pragma unroll
        for (int j = 0; j < 16; j++) dst[j] = paths[i * 16 + j];
    }
};
// a built handle: item i * H + d is the node key i opens at depth d (i == 0 or shared[i] < d).  The hash is read from the level array; the
// children are gathered as trie_build_level_kernel gathers them, absent ones are the empty roots.  Nothing is hashed.
struct NodesTrieSrc {
    TrieView t;
    __device__ __forceinline__ bool digest(size_t idx, uint4& d0, uint4& d1) const {
        const size_t i = idx / (size_t)t.height;
        const int d = (int)(idx % (size_t)t.height);
        if (i > 0 && (int)t.shared[i] >= d) return false;
        const uint4* at = t.levels + ((size_t)d * t.n + i) * 2;
        d0 = at[0];
        d1 = at[1];
        return true;
    }
    __device__ __forceinline__ void children(size_t idx, uint4* dst) const {
        const size_t i = idx / (size_t)t.height;
        const int d = (int)(idx % (size_t)t.height);
        const uint4* kp = reinterpret_cast<const uint4*>(t.keys + i * 8);
        const uint4 klo = kp[0], khi = kp[1];
        const uint32_t ki[8] = {klo.x, klo.y, klo.z, klo.w, khi.x, khi.y, khi.z, khi.w};
        size_t lo = i + 1, end = t.n;  // the first key that leaves the prefix
        while (lo < end) {
            const size_t mid = lo + ((end - lo) >> 1);
            if (trie_same_prefix(ki, t.keys + mid * 8, t.height, d)) lo = mid + 1;
            else end = mid;
        }
        const uint4* emp = t.empty + 2 * (t.height - 1 - d);
        const uint4* below = d == t.height - 1 ? t.values : t.levels + (size_t)(d + 1) * t.n * 2;
        size_t b = i;
#pragma unroll 1
        for (int c = 0; c < 8; c++) {
            const size_t nb = c < 7 ? trie_digit_lower_bound(t.keys, b, end, t.height, d, c + 1) : end;
            const uint4* x = nb > b ? below + 2 * b : emp;
            dst[2 * c] = x[0];
            dst[2 * c + 1] = x[1];
            b = nb;
        }
    }
};

struct NodesCounters {
    unsigned long long claimed;  // slots won in this batch
    unsigned int n_over, pad;
};

// ---- insert ----------------------------------------------------------------------------------------------------------------------------
// `distinct`: the items are known to hold different digests (growth), so a slot with my tag is another node's and the probe goes on.
template <class Src>
__global__ __launch_bounds__(TRIE_BLOCK) void trie_nodes_claim_kernel(NodesView t, Src src, size_t count, uint32_t* __restrict__ pend, NodesCounters* ctr, int distinct) {
    const size_t i = (size_t)blockIdx.x * TRIE_BLOCK + threadIdx.x;
    bool won = false;
    if (i < count) {
        uint32_t mine = NODES_NONE;
        uint4 d0, d1;
        if (src.digest(i, d0, d1)) {
            const unsigned long long tag = nodes_tag(t, d0);
            size_t slot = nodes_home(t, d0);
            for (size_t k = 0; k <= t.mask; k++, slot = (slot + 1) & t.mask) {  // the table is at most half full: an empty slot comes
                const unsigned long long old = atomicCAS(&t.tags[slot], 0ull, tag);
                if (old == 0) {
                    t.digests[2 * slot] = d0;
                    t.digests[2 * slot + 1] = d1;
                    src.children(i, t.pre + slot * 16);
                    won = true;
                    break;
                }
                if (old == tag && !distinct) {
                    mine = (uint32_t)slot;
                    break;
                }
            }
        }
        if (pend) pend[i] = mine;
    }
    const unsigned long long mask = __ballot(won);
    if ((threadIdx.x & 63) == 0 && mask) atomicAdd(&ctr->claimed, (unsigned long long)__popcll(mask));
}

template <class Src>
__global__ __launch_bounds__(TRIE_BLOCK) void trie_nodes_confirm_kernel(NodesView t, Src src, size_t count, const uint32_t* __restrict__ pend, uint32_t* __restrict__ over,
                                                                         NodesCounters* ctr) {
    const size_t i = (size_t)blockIdx.x * TRIE_BLOCK + threadIdx.x;
    if (i >= count || pend[i] == NODES_NONE) return;
    const size_t slot = pend[i];
    uint4 d0, d1;
    src.digest(i, d0, d1);
    if (!nodes_same(t.digests[2 * slot], t.digests[2 * slot + 1], d0, d1)) over[atomicAdd(&ctr->n_over, 1u)] = (uint32_t)i;
}

// one lane, the overflow items one after the other: a full-digest probe against everything stored, its own earlier stores included
template <class Src>
__global__ void trie_nodes_serial_kernel(NodesView t, Src src, const uint32_t* __restrict__ over, unsigned n_over, NodesCounters* ctr) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    unsigned long long claimed = 0;
    for (unsigned k = 0; k < n_over; k++) {
        const size_t i = over[k];
        uint4 d0, d1;
        src.digest(i, d0, d1);
        const unsigned long long tag = nodes_tag(t, d0);
        size_t slot = nodes_home(t, d0);
        for (size_t j = 0; j <= t.mask; j++, slot = (slot + 1) & t.mask) {
            const unsigned long long g = t.tags[slot];
            if (g == 0) {
                t.tags[slot] = tag;
                t.digests[2 * slot] = d0;
                t.digests[2 * slot + 1] = d1;
                src.children(i, t.pre + slot * 16);
                claimed++;
                break;
            }
            if (g == tag && nodes_same(t.digests[2 * slot], t.digests[2 * slot + 1], d0, d1)) break;
        }
    }
    ctr->claimed += claimed;
}

// ---- read ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TRIE_BLOCK) void trie_nodes_get_kernel(NodesView t, const uint4* __restrict__ digests, size_t m, uint4* __restrict__ pre,
                                                                     uint32_t* __restrict__ found) {
    const size_t g = (size_t)blockIdx.x * TRIE_BLOCK + threadIdx.x, j = g >> 3;
    const unsigned c = (unsigned)(g & 7);
    if (j >= m) return;
    const size_t slot = nodes_find(t, digests[2 * j], digests[2 * j + 1]);
    const bool hit = slot != ~(size_t)0;
    uint4 x0 = make_uint4(0, 0, 0, 0), x1 = x0;
    if (hit) {
        x0 = t.pre[slot * 16 + 2 * c];
        x1 = t.pre[slot * 16 + 2 * c + 1];
    }
    pre[j * 16 + 2 * c] = x0;
    pre[j * 16 + 2 * c + 1] = x1;
    if (c == 0) found[j] = hit ? 1u : 0u;
}

// new_with_root + prove_lookup_at_path: status 0 = found, k + 1 = the node expected at level k is not in the store (Error::MissingPreimage);
// then the rows from level k on and the value are zero.  The eight lanes of a query stay together (8 divides the wave).
__global__ __launch_bounds__(TRIE_BLOCK) void trie_nodes_walk_kernel(NodesView t, const uint4* __restrict__ roots, size_t root_stride, const uint32_t* __restrict__ keys,
                                                                      size_t m, int height, uint4* __restrict__ paths, uint4* __restrict__ values,
                                                                      uint32_t* __restrict__ status, unsigned long long* n_missing) {
    const size_t g = (size_t)blockIdx.x * TRIE_BLOCK + threadIdx.x, q = g >> 3;
    const unsigned c = (unsigned)(g & 7);
    if (q >= m) return;
    uint4 cur0 = roots[2 * q * root_stride], cur1 = roots[2 * q * root_stride + 1];
    const uint32_t* key = keys + q * 8;
    uint4* out = paths + q * (size_t)height * 16;
    unsigned st = 0;
    for (int d = 0; d < height; d++) {
        uint4 x0 = make_uint4(0, 0, 0, 0), x1 = x0;
        if (st == 0) {
            const size_t slot = nodes_find(t, cur0, cur1);
            if (slot == ~(size_t)0) {
                st = (unsigned)d + 1;
            } else {
                x0 = t.pre[slot * 16 + 2 * c];
                x1 = t.pre[slot * 16 + 2 * c + 1];
            }
        }
        out[(size_t)d * 16 + 2 * c] = x0;
        out[(size_t)d * 16 + 2 * c + 1] = x1;
        const int digit = trie_key_digit(key, height, d);
        cur0.x = (uint32_t)__shfl((int)x0.x, digit, 8);
        cur0.y = (uint32_t)__shfl((int)x0.y, digit, 8);
        cur0.z = (uint32_t)__shfl((int)x0.z, digit, 8);
        cur0.w = (uint32_t)__shfl((int)x0.w, digit, 8);
        cur1.x = (uint32_t)__shfl((int)x1.x, digit, 8);
        cur1.y = (uint32_t)__shfl((int)x1.y, digit, 8);
        cur1.z = (uint32_t)__shfl((int)x1.z, digit, 8);
        cur1.w = (uint32_t)__shfl((int)x1.w, digit, 8);
    }
    if (c == 0) {
        values[2 * q] = cur0;  // zero after a miss: every row from the missing level on is
        values[2 * q + 1] = cur1;
        status[q] = st;
        if (st && n_missing) atomicAdd(n_missing, 1ull);
    }
}

// ---- hash ------------------------------------------------------------------------------------------------------------------------------
template <class P>
__global__ __launch_bounds__(TRIE_BLOCK) void trie_nodes_reduced_kernel(const uint4* __restrict__ elems, size_t n, unsigned long long* first_bad) {
    const size_t i = (size_t)blockIdx.x * TRIE_BLOCK + threadIdx.x;
    if (i >= n) return;
    const Fe<P> x = ld_fe<P>(elems + 2 * i);
    if (fe_canonical_ge_mod<P>(x.l)) atomicMin(first_bad, (unsigned long long)i);
}

// modify_value_at_path (:778-800) over the old paths the walk has written: H dependent hashes bottom-up, one update per lane.  A query the
// walk could not finish writes zero rows and a zero root.
template <class P>
__global__ __launch_bounds__(TRIE_BLOCK) __attribute__((amdgpu_waves_per_eu(2, 2))) void trie_nodes_insert_hash_kernel(
    int height, const uint32_t* __restrict__ keys, const uint4* __restrict__ new_values, size_t m, const uint4* old_paths, uint4* new_paths,
    uint4* __restrict__ new_roots, const uint32_t* __restrict__ status, const uint4* __restrict__ img, int img_vec4, int rf, int rp) {
    extern __shared__ uint4 lds[];
    trie_stage_image(lds, img, img_vec4);
    const TrieHasher<P> h(lds, rf, rp);
    const size_t q = (size_t)blockIdx.x * TRIE_BLOCK + threadIdx.x;
    if (q >= m) return;  // no barrier follows
    const uint32_t* key = keys + q * 8;
    const uint4* oldp = old_paths + q * (size_t)height * 16;
    uint4* newp = new_paths + q * (size_t)height * 16;
    if (status[q]) {
        const uint4 z = make_uint4(0, 0, 0, 0);
        for (size_t j = 0; j < (size_t)height * 16; j++) newp[j] = z;
        new_roots[2 * q] = z;
        new_roots[2 * q + 1] = z;
        return;
    }
    Fe<P> cur = ld_fe<P>(new_values + 2 * q);
    for (int d = height - 1; d >= 0; d--) {
        const int digit = trie_key_digit(key, height, d);
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

static size_t nodes_round16(size_t b) { return (b + 15) & ~(size_t)15; }
static size_t nodes_bytes(size_t slots) { return nodes_round16(slots * 8) + slots * 32 + slots * 256; }
static size_t nodes_slots_for(size_t nodes) {
    size_t slots = 2;
    while (slots < 2 * nodes) slots <<= 1;
    return slots;
}

}  // namespace lurk

using namespace lurk;

struct lurk_hip_trie_nodes {
    int field_id = 0, height = 0, device = 0;
    size_t n_nodes = 0, slots = 0;
    unsigned long long tag_mask = ~0ull;
    DevBuf mem;  // tags | digests | pre
    static NodesView view_of(const DevBuf& mem, size_t slots, unsigned long long tag_mask) {
        char* p = (char*)mem.p;
        return NodesView{(unsigned long long*)p, (uint4*)(p + nodes_round16(slots * 8)), (uint4*)(p + nodes_round16(slots * 8) + slots * 32), slots - 1, tag_mask};
    }
    NodesView view() const { return view_of(mem, slots, tag_mask); }
};

namespace {

void require_nodes_here(const lurk_hip_trie_nodes* ns) {
    LURK_REQUIRE(ns, "null node store handle");
    LURK_REQUIRE(current_device() == ns->device, "the node store lives on another device than the calling thread's current one");
}

// before a batch of `count` items: at most half the slots may be taken once all of them are in.  One allocation, one re-insert launch over
// the old arrays (their digests are distinct: it only claims), one free.  A failed allocation leaves the store as it was.
void nodes_reserve(lurk_hip_trie_nodes* ns, size_t count, hipStream_t s) {
    if (2 * (ns->n_nodes + count) <= ns->slots) return;
    const size_t slots = nodes_slots_for(ns->n_nodes + count);
    DevBuf mem(nodes_bytes(slots)), ctr(sizeof(NodesCounters));
    LURK_HIP_CHECK(hipMemsetAsync(mem.p, 0, slots * 8, s));
    LURK_HIP_CHECK(hipMemsetAsync(ctr.p, 0, sizeof(NodesCounters), s));
    const NodesView nv = lurk_hip_trie_nodes::view_of(mem, slots, ns->tag_mask);
    {
        ProfScope ps("trie_nodes_grow", s);
        hipLaunchKernelGGL((trie_nodes_claim_kernel<NodesRehashSrc>), dim3(div_up(ns->slots, TRIE_BLOCK)), dim3(TRIE_BLOCK), 0, s, nv, NodesRehashSrc{ns->view()}, ns->slots,
                           (uint32_t*)nullptr, ctr.as<NodesCounters>(), 1);
        LURK_HIP_CHECK(hipGetLastError());
    }
    NodesCounters c;
    LURK_HIP_CHECK(hipMemcpyAsync(&c, ctr.p, sizeof(c), hipMemcpyDeviceToHost, s));
    LURK_HIP_CHECK(hipStreamSynchronize(s));
    LURK_REQUIRE(c.claimed == ns->n_nodes, "the node store lost a node while growing");
    ns->mem = std::move(mem);
    ns->slots = slots;
}

// the batch insert: claim, confirm, and the overflow items serially.  Synchronises: the host learns n_nodes.
template <class Src>
void nodes_insert(lurk_hip_trie_nodes* ns, const Src& src, size_t count, hipStream_t s) {
    if (count == 0) return;
    LURK_REQUIRE(count < ((size_t)1 << 32), "a batch holds fewer than 2^32 nodes");
    nodes_reserve(ns, count, s);
    DevBuf pend(count * 4), over(count * 4), ctr(sizeof(NodesCounters));
    LURK_HIP_CHECK(hipMemsetAsync(ctr.p, 0, sizeof(NodesCounters), s));
    const NodesView v = ns->view();
    const unsigned grid = div_up(count, TRIE_BLOCK);
    NodesCounters c;
    {
        ProfScope ps("trie_nodes_insert", s);
        hipLaunchKernelGGL((trie_nodes_claim_kernel<Src>), dim3(grid), dim3(TRIE_BLOCK), 0, s, v, src, count, pend.as<uint32_t>(), ctr.as<NodesCounters>(), 0);
        LURK_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL((trie_nodes_confirm_kernel<Src>), dim3(grid), dim3(TRIE_BLOCK), 0, s, v, src, count, pend.as<uint32_t>(), over.as<uint32_t>(),
                           ctr.as<NodesCounters>());
        LURK_HIP_CHECK(hipGetLastError());
    }
    LURK_HIP_CHECK(hipMemcpyAsync(&c, ctr.p, sizeof(c), hipMemcpyDeviceToHost, s));
    LURK_HIP_CHECK(hipStreamSynchronize(s));
    if (c.n_over) {  // one tag, two digests: astronomically rare at 64 tag bits
        hipLaunchKernelGGL((trie_nodes_serial_kernel<Src>), dim3(1), dim3(64), 0, s, v, src, over.as<uint32_t>(), c.n_over, ctr.as<NodesCounters>());
        LURK_HIP_CHECK(hipGetLastError());
        LURK_HIP_CHECK(hipMemcpyAsync(&c, ctr.p, sizeof(c), hipMemcpyDeviceToHost, s));
        LURK_HIP_CHECK(hipStreamSynchronize(s));
    }
    ns->n_nodes += (size_t)c.claimed;
}

void nodes_walk(const lurk_hip_trie_nodes* ns, const void* d_roots32, size_t root_stride, const void* d_keys32, size_t m, void* d_paths, void* d_values32,
                uint32_t* d_status, unsigned long long* d_missing, hipStream_t s) {
    ProfScope ps("trie_nodes_walk", s);
    hipLaunchKernelGGL(trie_nodes_walk_kernel, dim3(div_up(m * 8, TRIE_BLOCK)), dim3(TRIE_BLOCK), 0, s, ns->view(), (const uint4*)d_roots32, root_stride,
                       (const uint32_t*)d_keys32, m, ns->height, (uint4*)d_paths, (uint4*)d_values32, d_status, d_missing);
    LURK_HIP_CHECK(hipGetLastError());
}

unsigned long long nodes_tag_mask() {
    const char* e = getenv("LURK_TRIE_NODES_TAG_BITS");
    if (!e || !*e) return ~0ull;
    char* end = nullptr;
    const long bits = strtol(e, &end, 10);
    if (*end || bits < 1 || bits >= 64) return ~0ull;
    return (1ull << bits) - 1ull;
}

}  // namespace

extern "C" {

int lurk_hip_trie_nodes_create(lurk_hip_trie_nodes** out, int field_id, int height, size_t reserve_nodes) {
    return guarded([&] {
        LURK_REQUIRE(out, "null output handle");
        *out = nullptr;
        require_trie_field(field_id);
        require_trie_height(height);
        LURK_REQUIRE(reserve_nodes <= ((size_t)1 << 40), "reserve_nodes is beyond any device");
        const std::vector<uint64_t>& er = trie_empty_roots(field_id);
        auto ns = std::make_unique<lurk_hip_trie_nodes>();
        ns->field_id = field_id;
        ns->height = height;
        ns->device = current_device();
        ns->tag_mask = nodes_tag_mask();
        ns->slots = nodes_slots_for(reserve_nodes > (size_t)height ? reserve_nodes : (size_t)height);
        ns->mem.alloc(nodes_bytes(ns->slots));
        hipStream_t s = nullptr;
        LURK_HIP_CHECK(hipMemsetAsync(ns->mem.p, 0, ns->slots * 8, s));
        // init_empty (:464-481): the empty subtree of height h is hash8 of eight empty subtrees of height h - 1; the hashes are the library's
        std::vector<uint64_t> pre((size_t)height * 32);
        for (int h = 1; h <= height; h++)
            for (int j = 0; j < 8; j++) memcpy(pre.data() + ((size_t)(h - 1) * 8 + j) * 4, er.data() + 4 * (size_t)(h - 1), 32);
        DevBuf d_pre((size_t)height * 256), d_dig((size_t)height * 32);
        LURK_HIP_CHECK(hipMemcpyAsync(d_pre.p, pre.data(), (size_t)height * 256, hipMemcpyHostToDevice, s));
        LURK_HIP_CHECK(hipMemcpyAsync(d_dig.p, er.data() + 4, (size_t)height * 32, hipMemcpyHostToDevice, s));
        nodes_insert(ns.get(), NodesArraySrc{d_dig.as<uint4>(), d_pre.as<uint4>()}, (size_t)height, s);
        *out = ns.release();
    });
}

int lurk_hip_trie_nodes_destroy(lurk_hip_trie_nodes* ns) {
    return host_guarded([&] {
        if (!ns) return;
        DeviceGuard g(ns->device);
        delete ns;
    });
}

int lurk_hip_trie_nodes_info(const lurk_hip_trie_nodes* ns, int* field_id, int* height, size_t* n_nodes, size_t* slots, int* device) {
    return host_guarded([&] {
        LURK_REQUIRE(ns, "null node store handle");
        if (field_id) *field_id = ns->field_id;
        if (height) *height = ns->height;
        if (n_nodes) *n_nodes = ns->n_nodes;
        if (slots) *slots = ns->slots;
        if (device) *device = ns->device;
    });
}

int lurk_hip_trie_nodes_register_dev(lurk_hip_trie_nodes* ns, const void* d_preimages, size_t count, void* d_digests_out, void* stream) {
    return guarded([&] {
        require_nodes_here(ns);
        if (count == 0) return;
        LURK_REQUIRE(d_preimages, "null buffer");
        LURK_REQUIRE(count < ((size_t)1 << 32), "a batch holds fewer than 2^32 nodes");
        hipStream_t s = (hipStream_t)stream;
        with_field(ns->field_id, [&](auto F) {
            using P = decltype(F);
            {
                DevBuf bad(8);
                LURK_HIP_CHECK(hipMemsetAsync(bad.p, 0xff, 8, s));
                hipLaunchKernelGGL((trie_nodes_reduced_kernel<P>), dim3(div_up(count * 8, TRIE_BLOCK)), dim3(TRIE_BLOCK), 0, s, (const uint4*)d_preimages, count * 8,
                                   bad.as<unsigned long long>());
                LURK_HIP_CHECK(hipGetLastError());
                unsigned long long first = 0;
                LURK_HIP_CHECK(hipMemcpyAsync(&first, bad.p, 8, hipMemcpyDeviceToHost, s));
                LURK_HIP_CHECK(hipStreamSynchronize(s));
                if (first != ~0ull)
                    throw HipFailure{LURK_HIP_ERR_INVALID_ARG, "preimage element " + std::to_string(first) + " is not reduced modulo the field order"};
            }
            nodes_reserve(ns, count, s);  // a refused growth leaves nothing hashed
            DevBuf scratch;
            if (!d_digests_out) scratch.alloc(count * 32);
            uint4* dig = d_digests_out ? (uint4*)d_digests_out : scratch.as<uint4>();
            poseidon_batch_device(ns->field_id, 8, d_preimages, dig, count, 0, s);  // the batch hasher itself: one permutation in the library
            nodes_insert(ns, NodesArraySrc{dig, (const uint4*)d_preimages}, count, s);
        });
    });
}

int lurk_hip_trie_nodes_add_trie(lurk_hip_trie_nodes* ns, const lurk_hip_trie* trie, void* stream) {
    return guarded([&] {
        require_nodes_here(ns);
        require_trie_here(trie);
        LURK_REQUIRE(trie->field_id == ns->field_id, "the trie is over another field than the node store");
        LURK_REQUIRE(trie->height == ns->height, "the trie has another height than the node store");
        if (trie->n == 0) return;  // the empty chain is in the store since create
        nodes_insert(ns, NodesTrieSrc{trie->view()}, trie->n * (size_t)trie->height, (hipStream_t)stream);
    });
}

int lurk_hip_trie_nodes_get_dev(const lurk_hip_trie_nodes* ns, const void* d_digests32, size_t m, void* d_preimages, uint32_t* d_found, void* stream) {
    return guarded([&] {
        require_nodes_here(ns);
        if (m == 0) return;
        LURK_REQUIRE(d_digests32 && d_preimages && d_found, "null buffer");
        hipStream_t s = (hipStream_t)stream;
        ProfScope ps("trie_nodes_get", s);
        hipLaunchKernelGGL(trie_nodes_get_kernel, dim3(div_up(m * 8, TRIE_BLOCK)), dim3(TRIE_BLOCK), 0, s, ns->view(), (const uint4*)d_digests32, m, (uint4*)d_preimages,
                           d_found);
        LURK_HIP_CHECK(hipGetLastError());
    });
}

int lurk_hip_trie_nodes_prove_lookup_dev(const lurk_hip_trie_nodes* ns, const void* d_roots32, size_t root_stride, const void* d_keys32, size_t m, void* d_paths,
                                         void* d_values32, uint32_t* d_status, uint64_t* n_missing, void* stream) {
    return guarded([&] {
        require_nodes_here(ns);
        LURK_REQUIRE(root_stride <= 1, "root_stride is 0 (one root for every query) or 1 (one root per query)");
        if (n_missing) *n_missing = 0;
        if (m == 0) return;
        LURK_REQUIRE(d_roots32 && d_keys32 && d_paths && d_values32 && d_status, "null buffer");
        hipStream_t s = (hipStream_t)stream;
        with_field(ns->field_id, [&](auto F) {
            using P = decltype(F);
            std::vector<uint32_t> host;
            require_reduced_dev<P>(d_keys32, m, "key", host, s);
            require_reduced_dev<P>(d_roots32, root_stride ? m : 1, "root", host, s);
        });
        DevBuf missing;
        if (n_missing) {
            missing.alloc(8);
            LURK_HIP_CHECK(hipMemsetAsync(missing.p, 0, 8, s));
        }
        nodes_walk(ns, d_roots32, root_stride, d_keys32, m, d_paths, d_values32, d_status, n_missing ? missing.as<unsigned long long>() : nullptr, s);
        if (n_missing) {
            LURK_HIP_CHECK(hipMemcpyAsync(n_missing, missing.p, 8, hipMemcpyDeviceToHost, s));
            LURK_HIP_CHECK(hipStreamSynchronize(s));
        }
    });
}

int lurk_hip_trie_nodes_prove_insert_dev(lurk_hip_trie_nodes* ns, const void* d_roots32, size_t root_stride, const void* d_keys32, const void* d_new_values32, size_t m,
                                         void* d_old_paths, void* d_new_paths, void* d_old_values32, void* d_new_roots32, uint32_t* d_status, uint64_t* n_missing,
                                         int register_new, void* stream) {
    return guarded([&] {
        require_nodes_here(ns);
        LURK_REQUIRE(root_stride <= 1, "root_stride is 0 (one root for every query) or 1 (one root per query)");
        if (n_missing) *n_missing = 0;
        if (m == 0) return;
        LURK_REQUIRE(d_roots32 && d_keys32 && d_new_values32 && d_old_paths && d_new_paths && d_old_values32 && d_new_roots32 && d_status, "null buffer");
        const int H = ns->height;
        const size_t path_bytes = m * (size_t)H * 256;
        const char *a = (const char*)d_old_paths, *b = (const char*)d_new_paths;
        LURK_REQUIRE(a + path_bytes <= b || b + path_bytes <= a, "d_old_paths and d_new_paths overlap");
        LURK_REQUIRE(m * (size_t)H < ((size_t)1 << 32), "a batch holds fewer than 2^32 nodes");
        hipStream_t s = (hipStream_t)stream;
        with_field(ns->field_id, [&](auto F) {
            using P = decltype(F);
            {
                std::vector<uint32_t> host;
                require_reduced_dev<P>(d_keys32, m, "key", host, s);
                require_reduced_dev<P>(d_new_values32, m, "new value", host, s);
                require_reduced_dev<P>(d_roots32, root_stride ? m : 1, "root", host, s);
            }
            if (register_new) nodes_reserve(ns, m * (size_t)H, s);  // growth comes before the walk: a refused one leaves nothing written
            DevBuf missing;
            if (n_missing) {
                missing.alloc(8);
                LURK_HIP_CHECK(hipMemsetAsync(missing.p, 0, 8, s));
            }
            nodes_walk(ns, d_roots32, root_stride, d_keys32, m, d_old_paths, d_old_values32, d_status, n_missing ? missing.as<unsigned long long>() : nullptr, s);
            const TrieLaunch L(ns->field_id, s);
            auto kern = trie_nodes_insert_hash_kernel<P>;
            allow_dynamic_lds((const void*)kern, (int)L.lds_bytes);
            {
                ProfScope ps("trie_nodes_insert_hash", s);
                hipLaunchKernelGGL(kern, dim3(div_up(m, TRIE_BLOCK)), dim3(TRIE_BLOCK), L.lds_bytes, s, H, (const uint32_t*)d_keys32, (const uint4*)d_new_values32, m,
                                   (const uint4*)d_old_paths, (uint4*)d_new_paths, (uint4*)d_new_roots32, (const uint32_t*)d_status, L.img, L.vec4, L.rf, L.rp);
                LURK_HIP_CHECK(hipGetLastError());
            }
            if (n_missing) LURK_HIP_CHECK(hipMemcpyAsync(n_missing, missing.p, 8, hipMemcpyDeviceToHost, s));
            if (register_new)
                nodes_insert(ns, NodesPathSrc{(const uint32_t*)d_keys32, (const uint4*)d_new_paths, (const uint4*)d_new_roots32, (const uint32_t*)d_status, H},
                             m * (size_t)H, s);
            else if (n_missing)
                LURK_HIP_CHECK(hipStreamSynchronize(s));
        });
    });
}

int lurk_hip_trie_nodes_insert_chain_dev(lurk_hip_trie_nodes* ns, const void* root32_host, const void* d_keys32, const void* d_values32, size_t m, void* d_old_paths,
                                         void* d_new_paths, void* d_old_values32, void* d_roots32, void* stream) {
    return guarded([&] {
        require_nodes_here(ns);
        LURK_REQUIRE(root32_host, "null root");
        LURK_REQUIRE(m <= ((size_t)1 << 28), "a chain holds at most 2^28 updates");
        if (m == 0) return;
        LURK_REQUIRE(d_keys32 && d_values32, "null buffer");
        const int H = ns->height;
        const size_t path_bytes = m * (size_t)H * 256;
        LURK_REQUIRE(m * (size_t)H < ((size_t)1 << 32), "a batch holds fewer than 2^32 nodes");
        if (d_old_paths && d_new_paths) {
            const char *a = (const char*)d_old_paths, *b = (const char*)d_new_paths;
            LURK_REQUIRE(a + path_bytes <= b || b + path_bytes <= a, "d_old_paths and d_new_paths overlap");
        }
        hipStream_t s = (hipStream_t)stream;
        uint32_t root[8];
        memcpy(root, root32_host, 32);
        with_field(ns->field_id, [&](auto F) {
            using P = decltype(F);
            LURK_REQUIRE(!fe_canonical_ge_mod<P>(root), "the root is not reduced modulo the field order");
            std::vector<uint32_t> host;  // nothing is launched or allocated on the device before both have passed
            require_reduced_dev<P>(d_keys32, m, "key", host, s);
            require_reduced_dev<P>(d_values32, m, "value", host, s);
        });
        // every key is walked in T_0 first: a miss refuses the call with nothing hashed or registered
        DevBuf old_scratch, new_scratch, value_scratch, root_scratch, d_root(32), status(m * 4), missing(8);
        if (!d_old_paths) old_scratch.alloc(path_bytes);
        if (!d_new_paths) new_scratch.alloc(path_bytes);
        if (!d_roots32) root_scratch.alloc(m * 32);
        if (!d_old_values32) value_scratch.alloc(m * 32);
        uint4* oldp = d_old_paths ? (uint4*)d_old_paths : old_scratch.as<uint4>();
        void* newp = d_new_paths ? d_new_paths : new_scratch.p;
        void* roots = d_roots32 ? d_roots32 : root_scratch.p;
        LURK_HIP_CHECK(hipMemcpyAsync(d_root.p, root, 32, hipMemcpyHostToDevice, s));
        LURK_HIP_CHECK(hipMemsetAsync(missing.p, 0, 8, s));
        nodes_walk(ns, d_root.p, 0, d_keys32, m, oldp, d_old_values32 ? d_old_values32 : value_scratch.p, status.as<uint32_t>(), missing.as<unsigned long long>(), s);
        unsigned long long n_miss = 0;
        LURK_HIP_CHECK(hipMemcpyAsync(&n_miss, missing.p, 8, hipMemcpyDeviceToHost, s));
        LURK_HIP_CHECK(hipStreamSynchronize(s));
        if (n_miss) {
            std::vector<uint32_t> st(m);
            LURK_HIP_CHECK(hipMemcpy(st.data(), status.p, m * 4, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < m; i++)
                if (st[i])
                    throw HipFailure{LURK_HIP_ERR_INVALID_ARG, "update " + std::to_string(i) + ": missing preimage at level " + std::to_string(st[i] - 1)};
        }
        nodes_reserve(ns, m * (size_t)H, s);  // a refused growth leaves nothing hashed
        TrieChainScratch sc;
        trie_chain_run(ns->field_id, H, d_keys32, d_values32, m, oldp, d_old_paths != nullptr, newp, d_old_values32, roots, [] {}, sc, s);
        // every new node of every T_i: all m roots are addressable
        nodes_insert(ns, NodesPathSrc{(const uint32_t*)d_keys32, (const uint4*)newp, (const uint4*)roots, nullptr, H}, m * (size_t)H, s);
    });
}
}
