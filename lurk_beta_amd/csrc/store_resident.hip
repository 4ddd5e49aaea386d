// store_resident.hip - the content-addressed store of store.hip as a device-resident, append-only handle (lurk_hip_store).
//
// Reference: StoreCore is append-only and keeps its digest memo (z_cache) for its whole life (/root/reference/src/lem/store_core.rs:199-248);
// hydrate_z_cache (:256-269) hashes what has been interned since the last hydration, and Prover::prove hydrates before every proof
// (/root/reference/src/proof/mod.rs:180-198).  The handle keeps, indexed by NODE ID (ids are assigned in append order), the canonical
// digest (32 B) and the tag (4 B) of every node in HBM; an append hashes the new nodes only, and the two readers hand the digests on
// where the device wants them: a gather by id, and the preimages of a MultiFrame's hash slots (allocate_slot,
// /root/reference/src/lem/circuit.rs:249-315) laid out as lurk_hip_frames_witness_dev reads them.
//
// An append is scheduled as the one-shot call is: the new nodes are grouped by (level, arity), a group of more than STORE_HOST_MAX
// nodes is one indexed gather + one batch of the Poseidon kernel, a narrower one goes to the library's host Poseidon.  The new digests
// live in a STAGING array in (level, arity) order on both sides - the hasher's output is contiguous there - with the two marks of
// store.hip: positions below them are valid on the host / on the device, and whichever side is behind catches up with one copy when a
// group changes sides.  What reaches the device side of the staging array is scattered to digests[node id] at once, so a later group
// gathers every child, old or new, from the one resident array.  Children from EARLIER appends that a narrow group needs and the host
// holds no copy of come down once, before the first group: one indexed gather and one copy.
//
//   store_res_gather_kernel         preimages of one group from digests[child id], tags[child id] and this call's values (secrets)
//   store_res_scatter_kernel        digests[dst[k]] = src[k] (the hasher's output) or src[src_idx[k]] (the atoms' values)
//   store_res_digests_kernel        out[j] = digests[ids[j]], zeros for an id that is not a node
//   store_res_slot_preimages_kernel out[j] = the element descriptor j names: zero, a node's tag, a node's digest, a constant
// All four move 16 bytes per access in 256-thread blocks and use no LDS.
#include <algorithm>
#include <memory>

#include "common.hpp"
#include "dispatch.hpp"
#include "field.cuh"
#include "store_layout.hpp"

namespace lurk {

void poseidon_batch_device(int field_id, int arity, const void* d_pre, void* d_out, size_t n, int flags, hipStream_t s);  // poseidon.hip

constexpr int STORE_RES_BLOCK = 256;
constexpr size_t STORE_RES_DEFAULT_CAP = (size_t)1 << 16;  // nodes: 2.25 MiB
constexpr size_t STORE_RES_MAX_NODES = (size_t)1 << 31;    // ids are 32 bits and the kernels index 2 x id
constexpr uint32_t STORE_NO_HOST_COPY = 0xffffffffu;

struct ResNode {  // a new hashed node as the gather kernel reads it: two 16-byte words
    uint32_t kind, secret;  // secret: comm only, an index into this call's values
    uint32_t child[4];      // global node ids
    uint32_t pad[2];
};
static_assert(sizeof(ResNode) == 32, "ResNode is read as two uint4");

// one thread per (group node, preimage element), canonical 32-byte elements, the StoreHasher layouts of store_gather_kernel
template <int ARITY>
__global__ __launch_bounds__(STORE_RES_BLOCK) void store_res_gather_kernel(const uint4* __restrict__ nodes, uint32_t count, const uint4* __restrict__ digests,
                                                                           const uint32_t* __restrict__ tags, const uint4* __restrict__ vals,
                                                                           uint4* __restrict__ pre) {
    const size_t t = (size_t)blockIdx.x * STORE_RES_BLOCK + threadIdx.x;
    if (t >= (size_t)count * ARITY) return;
    const size_t i = t / ARITY;
    const uint32_t e = (uint32_t)(t % ARITY);
    const uint4 a = nodes[2 * i], b = nodes[2 * i + 1];  // {kind, secret, child 0, child 1}, {child 2, child 3, -, -}
    // which child, and its tag (0), its digest (1) or the secret (2)
    uint32_t k, what;
    if (a.x == LURK_NODE_COMPACT) {  // h_a, tag_b, h_b, h_c
        what = e == 1 ? 0u : 1u;
        k = e <= 1 ? e : e - 1;
    } else if (a.x == LURK_NODE_COMM) {  // secret, tag_a, h_a
        what = e == 0 ? 2u : e == 1 ? 0u : 1u;
        k = 0;
    } else {  // [tag, hash] per child
        what = e & 1u;
        k = e >> 1;
    }
    const uint32_t id = k == 0 ? a.z : k == 1 ? a.w : k == 2 ? b.x : b.y;
    uint4 lo = make_uint4(0, 0, 0, 0), hi = lo;
    if (what == 0) {
        lo.x = tags[id];
    } else {
        const uint4* src = what == 2 ? vals + 2 * (size_t)a.y : digests + 2 * (size_t)id;
        lo = src[0];
        hi = src[1];
    }
    pre[2 * t] = lo;
    pre[2 * t + 1] = hi;
}

// one thread per 16-byte half: element k of the source (element src_idx[k] when src_idx is given) becomes the digest of node dst[k]
__global__ __launch_bounds__(STORE_RES_BLOCK) void store_res_scatter_kernel(const uint4* __restrict__ src, const uint32_t* __restrict__ src_idx,
                                                                            const uint32_t* __restrict__ dst, size_t count, uint4* __restrict__ digests) {
    const size_t t = (size_t)blockIdx.x * STORE_RES_BLOCK + threadIdx.x;
    if (t >= 2 * count) return;
    const size_t k = t >> 1, h = t & 1;
    const size_t from = src_idx ? (size_t)src_idx[k] : k;
    digests[2 * (size_t)dst[k] + h] = src[2 * from + h];
}

// one thread per 16-byte half of the output; an id that is not a node reads nothing and gives zeros
__global__ __launch_bounds__(STORE_RES_BLOCK) void store_res_digests_kernel(const uint4* __restrict__ digests, size_t n_nodes, const uint32_t* __restrict__ ids,
                                                                            size_t m, uint4* __restrict__ out) {
    const size_t t = (size_t)blockIdx.x * STORE_RES_BLOCK + threadIdx.x;
    if (t >= 2 * m) return;
    const size_t id = ids[t >> 1];
    out[t] = id < n_nodes ? digests[2 * id + (t & 1)] : make_uint4(0, 0, 0, 0);
}

// one thread per element (the Montgomery form is one product over the whole element)
template <class P>
__global__ __launch_bounds__(STORE_RES_BLOCK) void store_res_slot_preimages_kernel(const uint4* __restrict__ digests, const uint32_t* __restrict__ tags,
                                                                                   size_t n_nodes, const uint2* __restrict__ elems, size_t n_elems, int as_mont,
                                                                                   uint4* __restrict__ out) {
    const size_t j = (size_t)blockIdx.x * STORE_RES_BLOCK + threadIdx.x;
    if (j >= n_elems) return;
    const uint2 d = elems[j];  // {kind, arg}
    const bool node = d.y < n_nodes;
    uint4 lo = make_uint4(0, 0, 0, 0), hi = lo;
    if (d.x == LURK_SLOT_ELEM_TAG) {
        if (node) lo.x = tags[d.y];
    } else if (d.x == LURK_SLOT_ELEM_DIGEST) {
        if (node) {
            lo = digests[2 * (size_t)d.y];
            hi = digests[2 * (size_t)d.y + 1];
        }
    } else if (d.x == LURK_SLOT_ELEM_CONST) {
        lo.x = d.y;
    }
    if (as_mont) {
        Fe<P> x;
        x.l[0] = lo.x; x.l[1] = lo.y; x.l[2] = lo.z; x.l[3] = lo.w;
        x.l[4] = hi.x; x.l[5] = hi.y; x.l[6] = hi.z; x.l[7] = hi.w;
        x = fe_to_mont<P>(x);
        lo = make_uint4(x.l[0], x.l[1], x.l[2], x.l[3]);
        hi = make_uint4(x.l[4], x.l[5], x.l[6], x.l[7]);
    }
    out[2 * j] = lo;
    out[2 * j + 1] = hi;
}

static void launch_gather(int arity, const ResNode* d_nodes, uint32_t count, const void* digests, const void* tags, const void* vals, void* pre, hipStream_t s) {
    const dim3 grid(div_up((size_t)count * arity, STORE_RES_BLOCK)), block(STORE_RES_BLOCK);
    const uint4* nd = reinterpret_cast<const uint4*>(d_nodes);
    switch (arity) {
        case 3: hipLaunchKernelGGL(store_res_gather_kernel<3>, grid, block, 0, s, nd, count, (const uint4*)digests, (const uint32_t*)tags, (const uint4*)vals, (uint4*)pre); break;
        case 4: hipLaunchKernelGGL(store_res_gather_kernel<4>, grid, block, 0, s, nd, count, (const uint4*)digests, (const uint32_t*)tags, (const uint4*)vals, (uint4*)pre); break;
        case 6: hipLaunchKernelGGL(store_res_gather_kernel<6>, grid, block, 0, s, nd, count, (const uint4*)digests, (const uint32_t*)tags, (const uint4*)vals, (uint4*)pre); break;
        default: hipLaunchKernelGGL(store_res_gather_kernel<8>, grid, block, 0, s, nd, count, (const uint4*)digests, (const uint32_t*)tags, (const uint4*)vals, (uint4*)pre); break;
    }
    LURK_HIP_CHECK(hipGetLastError());
}
static void launch_scatter(const void* src, const uint32_t* src_idx, const uint32_t* dst, size_t count, void* digests, hipStream_t s) {
    if (count == 0) return;
    hipLaunchKernelGGL(store_res_scatter_kernel, dim3(div_up(2 * count, STORE_RES_BLOCK)), dim3(STORE_RES_BLOCK), 0, s, (const uint4*)src, src_idx, dst, count,
                       (uint4*)digests);
    LURK_HIP_CHECK(hipGetLastError());
}
static void launch_digests(const void* digests, size_t n_nodes, const uint32_t* d_ids, size_t m, void* d_out, hipStream_t s) {
    if (m == 0) return;
    hipLaunchKernelGGL(store_res_digests_kernel, dim3(div_up(2 * m, STORE_RES_BLOCK)), dim3(STORE_RES_BLOCK), 0, s, (const uint4*)digests, n_nodes, d_ids, m,
                       (uint4*)d_out);
    LURK_HIP_CHECK(hipGetLastError());
}

}  // namespace lurk

using namespace lurk;

struct lurk_hip_store {
    int field_id = 0, device = 0;
    size_t n = 0, cap = 0, levels = 0, hashes = 0;
    DevBuf dig, tags;  // cap x 32 B, cap x 4 B, indexed by node id
    // what scheduling needs, per node: its level, its tag, and where the host copy of its digest is (host_dig, 4 words each) if it has one
    std::vector<uint32_t> level, tag, host_slot;
    std::vector<uint64_t> host_dig;
    mutable std::mutex mu;  // appends are serialised
};

static void require_store_here(const lurk_hip_store* s) {
    LURK_REQUIRE(s, "null store handle");
    LURK_REQUIRE(current_device() == s->device, "the store lives on another device than the calling thread's current one");
}

// capacity for `need` nodes: geometric growth, one device-to-device copy of what is resident.  The new buffers are allocated before the
// old ones are touched: an allocation failure leaves the store as it was.
static void store_reserve(lurk_hip_store* s, size_t need, hipStream_t st) {
    if (need <= s->cap) return;
    const size_t cap = std::min(std::max(need, 2 * s->cap), STORE_RES_MAX_NODES);
    DevBuf dig(cap * 32), tags(cap * 4);
    if (s->n) {
        LURK_HIP_CHECK(hipMemcpyAsync(dig.p, s->dig.p, s->n * 32, hipMemcpyDeviceToDevice, st));
        LURK_HIP_CHECK(hipMemcpyAsync(tags.p, s->tags.p, s->n * 4, hipMemcpyDeviceToDevice, st));
        LURK_HIP_CHECK(hipStreamSynchronize(st));
    }
    s->dig = std::move(dig);
    s->tags = std::move(tags);
    s->cap = cap;
}

[[noreturn]] static void refuse_record(size_t i, const std::string& what) {
    throw HipFailure{LURK_HIP_ERR_INVALID_ARG, "record " + std::to_string(i) + ": " + what};
}

extern "C" {

int lurk_hip_store_create(lurk_hip_store** out, int field_id, size_t reserve_nodes) {
    return guarded([&] {
        LURK_REQUIRE(out, "null output handle");
        *out = nullptr;
        with_field(field_id, [](auto) {});  // "unknown field id"
        LURK_REQUIRE(reserve_nodes <= STORE_RES_MAX_NODES, "too many nodes");
        auto s = std::make_unique<lurk_hip_store>();
        s->field_id = field_id;
        s->device = current_device();
        store_reserve(s.get(), reserve_nodes ? reserve_nodes : STORE_RES_DEFAULT_CAP, nullptr);
        *out = s.release();
    });
}

int lurk_hip_store_destroy(lurk_hip_store* s) {
    return host_guarded([&] {
        if (!s) return;
        DeviceGuard g(s->device);
        delete s;
    });
}

int lurk_hip_store_info(const lurk_hip_store* s, int* field_id, size_t* n_nodes, size_t* levels, size_t* hashes_done, size_t* capacity, int* device) {
    return host_guarded([&] {
        LURK_REQUIRE(s, "null store handle");
        std::lock_guard<std::mutex> lk(s->mu);
        if (field_id) *field_id = s->field_id;
        if (n_nodes) *n_nodes = s->n;
        if (levels) *levels = s->levels;
        if (hashes_done) *hashes_done = s->hashes;
        if (capacity) *capacity = s->cap;
        if (device) *device = s->device;
    });
}

int lurk_hip_store_append(lurk_hip_store* s, const lurk_hip_store_node* nodes, size_t n_new, const void* values32, size_t n_values, size_t* first_id,
                          void* new_digests32) {
    return guarded([&] {
        require_store_here(s);
        std::lock_guard<std::mutex> lk(s->mu);
        LURK_REQUIRE(n_new == 0 || nodes, "null buffer");
        LURK_REQUIRE(n_new < STORE_RES_MAX_NODES && s->n + n_new < STORE_RES_MAX_NODES && n_values < STORE_RES_MAX_NODES, "too many nodes");
        const size_t base = s->n;
        const char* vals = (const char*)values32;
        // ---- every record is checked before anything is allocated, launched or changed; levels on the way ----
        std::vector<uint32_t> level(n_new, 0);
        uint32_t max_level = (uint32_t)s->levels;
        size_t n_hashed = 0;
        with_field(s->field_id, [&](auto F) {
            using P = decltype(F);
            auto check_value = [&](size_t i, uint32_t v, const char* out_of_range) {
                if (!(v < n_values && vals)) refuse_record(i, out_of_range);
                uint32_t w[8];
                memcpy(w, vals + (size_t)v * 32, 32);  // caller memory carries no alignment promise
                if (fe_canonical_ge_mod<P>(w)) refuse_record(i, "value " + std::to_string(v) + " is not reduced modulo the field order");
            };
            for (size_t i = 0; i < n_new; i++) {
                const lurk_hip_store_node& nd = nodes[i];
                if (nd.kind == LURK_NODE_ATOM) {
                    check_value(i, nd.value, "atom value index out of range");
                    continue;
                }
                const int nc = kind_children(nd.kind);
                if (nc == 0) refuse_record(i, "unknown node kind");
                uint32_t lv = 0;
                for (int k = 0; k < nc; k++) {
                    const size_t c = nd.child[k];
                    if (c >= base + i) refuse_record(i, "nodes must be in topological order (children first)");
                    lv = std::max(lv, c < base ? s->level[c] : level[c - base]);
                }
                if (nd.kind == LURK_NODE_COMM) check_value(i, nd.value, "commitment secret index out of range");
                level[i] = lv + 1;
                max_level = std::max(max_level, lv + 1);
                n_hashed++;
            }
        });
        if (first_id) *first_id = base;
        if (n_new == 0) return;
        // ---- shape: the hashed nodes in (level, arity) order = their positions in the staging array; the atoms apart ----
        std::vector<uint32_t> order;  // local indices
        order.reserve(n_hashed);
        std::vector<uint32_t> atoms;  // [node ids | value indices]
        for (size_t i = 0; i < n_new; i++)
            if (nodes[i].kind != LURK_NODE_ATOM) order.push_back((uint32_t)i);
        const size_t n_atoms = n_new - n_hashed;
        atoms.resize(2 * n_atoms);
        for (size_t i = 0, a = 0; i < n_new; i++)
            if (nodes[i].kind == LURK_NODE_ATOM) {
                atoms[a] = (uint32_t)(base + i);
                atoms[n_atoms + a] = nodes[i].value;
                a++;
            }
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
            if (level[a] != level[b]) return level[a] < level[b];
            return kind_arity(nodes[a].kind) < kind_arity(nodes[b].kind);
        });
        std::vector<uint32_t> pos(n_new, 0), order_ids(n_hashed);
        std::vector<ResNode> res(n_hashed);
        struct Group { uint32_t first, count; int arity; };
        std::vector<Group> groups;
        size_t max_dev_elems = 0;
        for (size_t k = 0; k < n_hashed; k++) {
            const lurk_hip_store_node& nd = nodes[order[k]];
            pos[order[k]] = (uint32_t)k;
            order_ids[k] = (uint32_t)(base + order[k]);
            ResNode& r = res[k];
            r.kind = nd.kind;
            r.secret = nd.kind == LURK_NODE_COMM ? nd.value : 0;
            for (int c = 0; c < 4; c++) r.child[c] = c < kind_children(nd.kind) ? nd.child[c] : 0;
            r.pad[0] = r.pad[1] = 0;
            const int arity = kind_arity(nd.kind);
            if (groups.empty() || level[order[k]] != level[order[groups.back().first]] || arity != groups.back().arity) groups.push_back({(uint32_t)k, 0, arity});
            groups.back().count++;
        }
        // children of narrow groups that came with an earlier append and have no host copy: fetched once, below
        std::vector<uint32_t> fetch;
        for (const Group& g : groups) {
            if (g.count > STORE_HOST_MAX) {
                max_dev_elems = std::max(max_dev_elems, (size_t)g.count * g.arity);
                continue;
            }
            for (uint32_t k = 0; k < g.count; k++) {
                const ResNode& r = res[g.first + k];
                for (int c = 0; c < kind_children(r.kind); c++)
                    if (r.child[c] < base && s->host_slot[r.child[c]] == STORE_NO_HOST_COPY) fetch.push_back(r.child[c]);
            }
        }
        std::sort(fetch.begin(), fetch.end());
        fetch.erase(std::unique(fetch.begin(), fetch.end()), fetch.end());
        // ---- every allocation of the call, then the growth: a failure up to here has changed nothing ----
        hipStream_t st = nullptr;
        std::vector<uint32_t> new_tags(n_new);
        for (size_t i = 0; i < n_new; i++) new_tags[i] = nodes[i].tag;
        std::vector<uint64_t> host(n_hashed * 4), fetched(fetch.size() * 4);
        s->level.reserve(base + n_new);
        s->tag.reserve(base + n_new);
        s->host_slot.reserve(base + n_new);
        DevBuf d_nodes(n_hashed * sizeof(ResNode)), d_order(n_hashed * 4), d_stage(n_hashed * 32), d_pre(max_dev_elems * 32), d_vals(n_values * 32),
            d_atoms(2 * n_atoms * 4), d_fetch_ids(fetch.size() * 4), d_fetch(fetch.size() * 32);
        store_reserve(s, base + n_new, st);
        // ---- device: tags, values and atoms up; the old digests narrow groups need down ----
        LURK_HIP_CHECK(hipMemcpyAsync((char*)s->tags.p + base * 4, new_tags.data(), n_new * 4, hipMemcpyHostToDevice, st));
        if (n_values && vals) LURK_HIP_CHECK(hipMemcpyAsync(d_vals.p, vals, n_values * 32, hipMemcpyHostToDevice, st));
        if (n_atoms) {
            LURK_HIP_CHECK(hipMemcpyAsync(d_atoms.p, atoms.data(), 2 * n_atoms * 4, hipMemcpyHostToDevice, st));
            launch_scatter(d_vals.p, d_atoms.as<uint32_t>() + n_atoms, d_atoms.as<uint32_t>(), n_atoms, s->dig.p, st);
        }
        if (!fetch.empty()) {
            LURK_HIP_CHECK(hipMemcpyAsync(d_fetch_ids.p, fetch.data(), fetch.size() * 4, hipMemcpyHostToDevice, st));
            launch_digests(s->dig.p, base, d_fetch_ids.as<uint32_t>(), fetch.size(), d_fetch.p, st);
            LURK_HIP_CHECK(hipMemcpyAsync(fetched.data(), d_fetch.p, fetch.size() * 32, hipMemcpyDeviceToHost, st));
            LURK_HIP_CHECK(hipStreamSynchronize(st));
            for (size_t j = 0; j < fetch.size(); j++) {  // true values of resident nodes: they stay, whatever becomes of this append
                s->host_slot[fetch[j]] = (uint32_t)(s->host_dig.size() / 4);
                s->host_dig.insert(s->host_dig.end(), fetched.begin() + 4 * j, fetched.begin() + 4 * j + 4);
            }
        }
        if (n_hashed) {
            LURK_HIP_CHECK(hipMemcpyAsync(d_nodes.p, res.data(), n_hashed * sizeof(ResNode), hipMemcpyHostToDevice, st));
            LURK_HIP_CHECK(hipMemcpyAsync(d_order.p, order_ids.data(), n_hashed * 4, hipMemcpyHostToDevice, st));
        }
        // ---- the staging array on both sides: positions below the two marks are valid on the host / on the device (store.hip) ----
        size_t host_valid = 0, dev_valid = 0;
        auto to_host = [&](size_t upto) {  // device-computed positions [host_valid, upto) come down
            if (upto <= host_valid) return;
            LURK_HIP_CHECK(hipMemcpyAsync(host.data() + host_valid * 4, (char*)d_stage.p + host_valid * 32, (upto - host_valid) * 32, hipMemcpyDeviceToHost, st));
            LURK_HIP_CHECK(hipStreamSynchronize(st));
            host_valid = upto;
        };
        auto to_device = [&](size_t upto) {  // host-computed positions [dev_valid, upto) go up, and on to digests[node id]
            if (upto <= dev_valid) return;
            LURK_HIP_CHECK(hipMemcpyAsync((char*)d_stage.p + dev_valid * 32, host.data() + dev_valid * 4, (upto - dev_valid) * 32, hipMemcpyHostToDevice, st));
            launch_scatter((char*)d_stage.p + dev_valid * 32, nullptr, d_order.as<uint32_t>() + dev_valid, upto - dev_valid, s->dig.p, st);
            dev_valid = upto;
        };
        // host twin of the gather + one hash: children from earlier appends from the host copies, this append's from the call's own
        // values (atoms) or the staging array
        auto child_digest = [&](uint32_t c, uint64_t* out4) {
            if (c < base) {
                memcpy(out4, s->host_dig.data() + 4 * (size_t)s->host_slot[c], 32);
                return;
            }
            const lurk_hip_store_node& cn = nodes[c - base];
            if (cn.kind == LURK_NODE_ATOM) memcpy(out4, vals + (size_t)cn.value * 32, 32);
            else memcpy(out4, host.data() + 4 * (size_t)pos[c - base], 32);
        };
        auto child_tag = [&](uint32_t c) { return c < base ? s->tag[c] : nodes[c - base].tag; };
        auto hash_on_host = [&](const ResNode& r, uint64_t* out4) {
            uint64_t pre[8 * 4] = {0};
            int arity = kind_arity(r.kind);
            switch (r.kind) {
                case LURK_NODE_COMPACT:
                    child_digest(r.child[0], pre);
                    pre[4] = child_tag(r.child[1]);
                    child_digest(r.child[1], pre + 8);
                    child_digest(r.child[2], pre + 12);
                    break;
                case LURK_NODE_COMM:
                    memcpy(pre, vals + (size_t)r.secret * 32, 32);
                    pre[4] = child_tag(r.child[0]);
                    child_digest(r.child[0], pre + 8);
                    break;
                default:  // tuple2 / 3 / 4
                    for (int c = 0; c < arity / 2; c++) {
                        pre[8 * c] = child_tag(r.child[c]);
                        child_digest(r.child[c], pre + 8 * c + 4);
                    }
                    break;
            }
            nested_ok(lurk_hip_poseidon_hash_host(s->field_id, arity, pre, 1, out4));
        };
        std::vector<uint8_t> host_hashed(n_hashed, 0);
        for (const Group& g : groups) {
            const size_t first = g.first, end = first + g.count;
            if (g.count <= STORE_HOST_MAX) {
                to_host(first);
                for (uint32_t k = 0; k < g.count; k++) {
                    hash_on_host(res[first + k], host.data() + (first + k) * 4);
                    host_hashed[first + k] = 1;
                }
                host_valid = end;
                continue;
            }
            to_device(first);
            ProfScope ps("store_append_level", st);
            launch_gather(g.arity, d_nodes.as<ResNode>() + first, g.count, s->dig.p, s->tags.p, d_vals.p, d_pre.p, st);
            poseidon_batch_device(s->field_id, g.arity, d_pre.p, (char*)d_stage.p + first * 32, g.count, 0, st);
            launch_scatter((char*)d_stage.p + first * 32, nullptr, d_order.as<uint32_t>() + first, g.count, s->dig.p, st);
            dev_valid = end;
        }
        to_device(n_hashed);  // what the host hashed last is resident before the call returns
        if (new_digests32) to_host(n_hashed);
        LURK_HIP_CHECK(hipStreamSynchronize(st));
        if (new_digests32)
            for (size_t i = 0; i < n_new; i++) {
                const void* from = nodes[i].kind == LURK_NODE_ATOM ? (const void*)(vals + (size_t)nodes[i].value * 32) : (const void*)(host.data() + 4 * (size_t)pos[i]);
                memcpy((char*)new_digests32 + i * 32, from, 32);
            }
        // ---- the append has happened: the host side follows ----
        s->level.insert(s->level.end(), level.begin(), level.end());
        s->tag.insert(s->tag.end(), new_tags.begin(), new_tags.end());
        s->host_slot.resize(base + n_new, STORE_NO_HOST_COPY);
        for (size_t k = 0; k < n_hashed; k++)
            if (host_hashed[k]) {
                s->host_slot[order_ids[k]] = (uint32_t)(s->host_dig.size() / 4);
                s->host_dig.insert(s->host_dig.end(), host.begin() + 4 * k, host.begin() + 4 * k + 4);
            }
        s->n = base + n_new;
        s->levels = max_level;
        s->hashes += n_hashed;
    });
}

int lurk_hip_store_digests_dev(const lurk_hip_store* s, const uint32_t* d_ids, size_t m, void* d_out32, void* stream) {
    return guarded([&] {
        require_store_here(s);
        LURK_REQUIRE(m < STORE_RES_MAX_NODES, "too many ids");
        if (m == 0) return;
        LURK_REQUIRE(d_ids && d_out32, "null buffer");
        ProfScope ps("store_digests", (hipStream_t)stream);
        launch_digests(s->dig.p, s->n, d_ids, m, d_out32, (hipStream_t)stream);
    });
}

int lurk_hip_store_digests(const lurk_hip_store* s, const uint32_t* ids, size_t m, void* out32) {
    return guarded([&] {
        require_store_here(s);
        std::lock_guard<std::mutex> lk(s->mu);
        LURK_REQUIRE(m < STORE_RES_MAX_NODES, "too many ids");
        if (m == 0) return;
        LURK_REQUIRE(ids && out32, "null buffer");
        for (size_t i = 0; i < m; i++)
            if (ids[i] >= s->n)
                throw HipFailure{LURK_HIP_ERR_INVALID_ARG, "id " + std::to_string(i) + " is out of range: node " + std::to_string(ids[i]) + " of a store of " +
                                                               std::to_string(s->n) + " nodes"};
        hipStream_t st = nullptr;
        DevBuf d_ids(m * 4), d_out(m * 32);
        LURK_HIP_CHECK(hipMemcpyAsync(d_ids.p, ids, m * 4, hipMemcpyHostToDevice, st));
        launch_digests(s->dig.p, s->n, d_ids.as<uint32_t>(), m, d_out.p, st);
        LURK_HIP_CHECK(hipMemcpyAsync(out32, d_out.p, m * 32, hipMemcpyDeviceToHost, st));
        LURK_HIP_CHECK(hipStreamSynchronize(st));
    });
}

int lurk_hip_store_slot_preimages_dev(const lurk_hip_store* s, const lurk_hip_slot_elem* d_elems, size_t n_elems, int as_mont, void* d_out, void* stream) {
    return guarded([&] {
        require_store_here(s);
        LURK_REQUIRE(n_elems < STORE_RES_MAX_NODES, "too many elements");
        if (n_elems == 0) return;
        LURK_REQUIRE(d_elems && d_out, "null buffer");
        hipStream_t st = (hipStream_t)stream;
        with_field(s->field_id, [&](auto F) {
            using P = decltype(F);
            ProfScope ps("store_slot_preimages", st);
            hipLaunchKernelGGL((store_res_slot_preimages_kernel<P>), dim3(div_up(n_elems, STORE_RES_BLOCK)), dim3(STORE_RES_BLOCK), 0, st, s->dig.as<uint4>(),
                               s->tags.as<uint32_t>(), s->n, reinterpret_cast<const uint2*>(d_elems), n_elems, as_mont, (uint4*)d_out);
            LURK_HIP_CHECK(hipGetLastError());
        });
    });
}

}  // extern "C"
