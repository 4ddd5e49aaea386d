// trie_circuit.hip - the trie coprocessor's step circuits on the device: the witness block Trie::synthesize_lookup / synthesize_insert
// (/root/reference/src/coprocessor/trie/mod.rs:652-714, 802-880) would allocate, written straight into a resident W from the proofs the
// trie calls leave on the device, and the resident shape of the rows (trie_circuit.hpp holds the layout and the rows).
//
// The hot work is one hash8 trace per level of a lookup (m H traces) and a second one per level of an insert (2 m H): the trace bodies of
// the slot-witness kernels (poseidon_trace.cuh), each reading its preimage straight from the path buffer and writing its 396-element
// block at its place in W.  Two launches per call, whatever m and H:
//   poseidon_trace_wide_kernel / poseidon_trace_batch_kernel<.., TrieCircuitJob>   every trace of every call; hash q < m H is level q % H
//       of call q / H's old path (root level first, followed by its seven picks - copies of preimage entries chosen by the key's digit,
//       no arithmetic), hash m H + q is new preimage q % H of call q / H counted from the leaf.  Up to POSEIDON_WIDE_MAX traces take the
//       T-lanes-per-hash form (seven hashes per wave at T = 9, one pick per lane of a group), more take one hash per lane.
//   trie_circuit_head_kernel   one workgroup per call: the root, the key's bit-decomposition block, the new value
#include "common.hpp"
#include "dispatch.hpp"
#include "poseidon_trace.cuh"
#include "trie_circuit.hpp"

namespace lurk {

const SlotCircuit& slot_circuit(int field_id, int slot_type);  // r1cs_sat.hip

constexpr int TC_T = 9;  // arity 8

// where a trace finds its preimage and its block: the destination type of the trace kernels (poseidon_trace.cuh)
struct TrieTracePlace {
    const uint4* src;     // the preimage
    size_t wb;            // the hash block's first element in W
    const uint32_t* key;  // for the picks, null when the trace has none
    int level;
};
struct TrieCircuitJob {
    const uint4* old_paths;   // m x H x 8 canonical elements, root level first
    const uint4* new_paths;   // the same for the new preimages (insert), or null
    const uint32_t* keys;     // m x 8 words, canonical
    void* w;                  // Fe<P>*: the witness vector
    const uint64_t* offsets;  // per-call element offsets, or null: first + i * stride
    size_t first, stride;
    size_t n_old;             // m * H: the traces of the old paths come first
    size_t key_block, size_lookup;
    int height;
    __device__ __forceinline__ size_t block(size_t i) const { return offsets ? (size_t)offsets[i] : first + i * stride; }
    __device__ __forceinline__ TrieTracePlace place(size_t q) const {
        const bool old = q < n_old;
        const size_t r = old ? q : q - n_old, H = (size_t)height;
        const size_t i = r / H, l = r - i * H;
        const size_t blk = block(i);
        TrieTracePlace p;
        p.level = (int)l;
        if (old) {
            p.src = old_paths + q * 16;
            p.wb = blk + 1 + key_block + (TRIE_CIRCUIT_HASH_BLOCK + TRIE_CIRCUIT_PICKS) * l;
            p.key = keys + i * 8;
        } else {  // l counts from the leaf (synthesize_modify_value_at_path), the path buffer from the root
            p.src = new_paths + (i * H + (H - 1 - l)) * 16;
            p.wb = blk + size_lookup + 1 + TRIE_CIRCUIT_HASH_BLOCK * l;
            p.key = nullptr;
        }
        return p;
    }
    // pick `pk` (0 .. 6 in allocation order: rounds of 4, 2, 1) of select(preimage, digit): round r keeps the half its bit 2 - r names, so
    // every pick is a copy of one preimage entry
    template <class P>
    __device__ __forceinline__ void pick(const TrieTracePlace& p, int pk, const uint32_t* mont2) const {
        const int bit = 3 * (height - 1 - p.level), wd = bit >> 5, sh = bit & 31;
        uint32_t v = p.key[wd] >> sh;
        if (sh > 29) v |= p.key[wd + 1] << (32 - sh);  // bit <= 252: a digit that straddles two words starts below word 7
        const int d = (int)(v & 7u);
        const int idx = pk < 4 ? (d & 4) + pk : pk < 6 ? (d & 6) + (pk - 4) : d;
        const uint4 lo = p.src[2 * idx], hi = p.src[2 * idx + 1];
        const uint32_t x[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        trace_store<P>((Fe<P>*)w, p.wb + TRIE_CIRCUIT_HASH_BLOCK + pk, poseidon29_from_canonical<P>(x, mont2));
    }
    // what the trace kernels ask of a destination
    __device__ __forceinline__ size_t base(size_t q) const { return place(q).wb; }
    __device__ __forceinline__ const uint4* preimage(const uint4*, size_t q, int) const { return place(q).src; }
    template <class P>
    __device__ __forceinline__ void beside_wide(size_t q, int e, const uint32_t* mont2) const {  // lane e of the hash's group: one pick each
        const TrieTracePlace p = place(q);
        if (p.key && e < (int)TRIE_CIRCUIT_PICKS) pick<P>(p, e, mont2);
    }
    template <class P>
    __device__ __forceinline__ void beside_lane(size_t q, const uint32_t* mont2) const {
        const TrieTracePlace p = place(q);
        if (!p.key) return;
#pragma unroll 1
        for (int pk = 0; pk < (int)TRIE_CIRCUIT_PICKS; pk++) pick<P>(p, pk, mont2);
    }
};

template <class P>
__global__ __launch_bounds__(BIT_DECOMP_BLOCK) void trie_circuit_head_kernel(TrieCircuitJob job, size_t m, const Fe<P>* __restrict__ roots, size_t root_stride,
                                                                               const Fe<P>* __restrict__ values, const uint32_t* __restrict__ code, int ncode,
                                                                               const uint32_t* __restrict__ masks) {
    __shared__ uint32_t v[8];
    Fe<P>* w = (Fe<P>*)job.w;
    const Fe<P> one = fe_one<P>(), zero = fe_zero<P>();
    for (size_t i = blockIdx.x; i < m; i += gridDim.x) {
        const size_t blk = job.block(i);
        if (threadIdx.x == 0) {
            w[blk] = fe_to_mont<P>(roots[i * root_stride]);
            if (values) w[blk + job.size_lookup] = fe_to_mont<P>(values[i]);
        }
        bit_decomp_trace_block<P>(reinterpret_cast<const Fe<P>*>(job.keys) + i, 0, w, blk + 1, code, ncode, masks, v, one, zero);
    }
}

static void require_circuit_args(int field_id, int height, int op) {
    LURK_REQUIRE(field_id >= 0 && field_id <= 2, "unknown field id");
    LURK_REQUIRE(height >= 1 && height <= TRIE_CIRCUIT_MAX_HEIGHT, "trie height must be 1 .. 85");
    LURK_REQUIRE(op == LURK_TRIE_CIRCUIT_LOOKUP || op == LURK_TRIE_CIRCUIT_INSERT, "unknown trie circuit (LURK_TRIE_CIRCUIT_LOOKUP or _INSERT)");
}
static TrieCircuitDims circuit_dims(int field_id, int height, int op) {
    require_circuit_args(field_id, height, op);
    return trie_circuit_dims(slot_circuit(field_id, LURK_SLOT_BIT_DECOMP), slot_circuit(field_id, LURK_SLOT_HASH8), height, op == LURK_TRIE_CIRCUIT_INSERT);
}
static SlotCircuit circuit_rows(int field_id, int height, int op) {
    require_circuit_args(field_id, height, op);
    const SlotCircuit &bits = slot_circuit(field_id, LURK_SLOT_BIT_DECOMP), &hash8 = slot_circuit(field_id, LURK_SLOT_HASH8);
    LURK_REQUIRE(hash8.size == TRIE_CIRCUIT_HASH_BLOCK, "the hash8 slot block is not 396 elements");
    SlotCircuit c;
    with_field(field_id, [&](auto F) { c = trie_circuit<decltype(F)>(bits, hash8, height, op == LURK_TRIE_CIRCUIT_INSERT); });
    const TrieCircuitDims d = trie_circuit_dims(bits, hash8, height, op == LURK_TRIE_CIRCUIT_INSERT);
    LURK_REQUIRE(c.num_cons == d.num_cons && c.size == d.size, "trie circuit rows and dimensions disagree");
    return c;
}

template <class P>
static void launch_trie_circuit(const TrieCircuitJob& job, size_t m, bool insert, const void* d_roots, size_t root_stride, const void* d_values, int field_id,
                                hipStream_t s) {
    const PoseidonImageView iv = poseidon_image_view(field_id, 8, s);
    const BitDecompView bv = bit_decomp_view(field_id);
    LURK_REQUIRE((size_t)bv.ncode + 1 == job.key_block, "bit-decomposition program and rows disagree on the block size");
    const size_t n = job.n_old * (insert ? 2 : 1), lds_bytes = (size_t)iv.vec4 * 16;
    {
        ProfScope ps("trie_circuit_trace", s);
        if (n <= POSEIDON_WIDE_MAX) {
            auto kern = poseidon_trace_wide_kernel<P, TC_T, TrieCircuitJob>;
            allow_dynamic_lds((const void*)kern, (int)lds_bytes);
            constexpr size_t per_block = (size_t)(POSEIDON_WIDE_BLOCK / 64) * (64 / TC_T);
            hipLaunchKernelGGL(kern, dim3(div_up(n, per_block)), dim3(POSEIDON_WIDE_BLOCK), lds_bytes, s, (const uint4*)nullptr, n, (const uint4*)iv.img, iv.vec4, iv.rf, iv.rp, 0, job);
        } else {
            auto kern = poseidon_trace_batch_kernel<P, TC_T, TrieCircuitJob>;
            allow_dynamic_lds((const void*)kern, (int)lds_bytes);
            unsigned blocks = div_up(n, POSEIDON_BLOCK), cap = grid_cap(2);
            if (blocks > cap) blocks = cap;
            hipLaunchKernelGGL(kern, dim3(blocks), dim3(POSEIDON_BLOCK), lds_bytes, s, (const uint4*)nullptr, n, (const uint4*)iv.img, iv.vec4, iv.rf, iv.rp, 0, job);
        }
        LURK_HIP_CHECK(hipGetLastError());
    }
    ProfScope ps("trie_circuit_head", s);
    const unsigned blocks = m < 65535 ? (unsigned)m : 65535u;
    hipLaunchKernelGGL((trie_circuit_head_kernel<P>), dim3(blocks), dim3(BIT_DECOMP_BLOCK), 0, s, job, m, (const Fe<P>*)d_roots, root_stride, (const Fe<P>*)d_values,
                       bv.code, bv.ncode, bv.masks);
    LURK_HIP_CHECK(hipGetLastError());
}

}  // namespace lurk

using namespace lurk;

extern "C" {

int lurk_hip_trie_circuit_size(int field_id, int height, int op, size_t* size, size_t* num_cons, size_t* nnz_a, size_t* nnz_b, size_t* nnz_c, size_t* result_col,
                               size_t* value_col) {
    return host_guarded([&] {
        LURK_REQUIRE(size && num_cons && nnz_a && nnz_b && nnz_c && result_col, "null output");
        const TrieCircuitDims d = circuit_dims(field_id, height, op);
        const SlotCircuit c = circuit_rows(field_id, height, op);
        *size = d.size;
        *num_cons = d.num_cons;
        *nnz_a = c.m[0].indices.size();
        *nnz_b = c.m[1].indices.size();
        *nnz_c = c.m[2].indices.size();
        *result_col = d.result_col;
        if (value_col && op == LURK_TRIE_CIRCUIT_INSERT) *value_col = d.value_col;
    });
}

int lurk_hip_trie_circuit_constraints(int field_id, int height, int op, uint64_t* a_indptr, uint64_t* a_indices, void* a_data, uint64_t* b_indptr,
                                      uint64_t* b_indices, void* b_data, uint64_t* c_indptr, uint64_t* c_indices, void* c_data) {
    return host_guarded([&] {
        LURK_REQUIRE(a_indptr && a_indices && a_data && b_indptr && b_indices && b_data && c_indptr && c_indices && c_data, "null output");
        const SlotCircuit c = circuit_rows(field_id, height, op);
        uint64_t* ip[3] = {a_indptr, b_indptr, c_indptr};
        uint64_t* ix[3] = {a_indices, b_indices, c_indices};
        void* dv[3] = {a_data, b_data, c_data};
        for (int w = 0; w < 3; w++) {
            const SlotMatrix& m = c.m[w];
            memcpy(ip[w], m.indptr.data(), m.indptr.size() * 8);
            memcpy(ix[w], m.indices.data(), m.indices.size() * 8);
            memcpy(dv[w], m.data.data(), m.data.size() * 8);
        }
    });
}

int lurk_hip_trie_circuit_r1cs_create(lurk_hip_r1cs** shape, int field_id, int height, int op, size_t n_blocks, size_t first, size_t stride, size_t num_vars,
                                      size_t num_io, size_t extra_cons, const uint64_t* xa_indptr, const uint64_t* xa_indices, const void* xa_data,
                                      const uint64_t* xb_indptr, const uint64_t* xb_indices, const void* xb_data, const uint64_t* xc_indptr,
                                      const uint64_t* xc_indices, const void* xc_data) {
    return guarded([&] {
        LURK_REQUIRE(shape, "null output handle");
        *shape = nullptr;
        const TrieCircuitDims d = circuit_dims(field_id, height, op);
        const uint64_t* xip[3] = {xa_indptr, xb_indptr, xc_indptr};
        const uint64_t* xix[3] = {xa_indices, xb_indices, xc_indices};
        const void* xdv[3] = {xa_data, xb_data, xc_data};
        for (int w = 0; w < 3; w++)
            LURK_REQUIRE(extra_cons == 0 || (xip[w] && xip[w][0] == 0 && (xip[w][extra_cons] == 0 || (xix[w] && xdv[w]))), "malformed extra rows");
        // every size in 128 bits first: nothing is allocated for a layout that does not fit
        const unsigned __int128 lim = (unsigned __int128)1 << 32;
        LURK_REQUIRE(num_vars < lim && num_io < lim && num_vars + 1 + num_io < lim, "z has more than 2^32 - 1 entries");
        LURK_REQUIRE(n_blocks < lim && stride < lim && first < lim && extra_cons < lim, "layout overflows");
        LURK_REQUIRE(n_blocks <= 1 || stride >= d.size, "stride shorter than a circuit block");
        if (n_blocks)
            LURK_REQUIRE((unsigned __int128)first + (unsigned __int128)(n_blocks - 1) * stride + d.size <= num_vars, "a circuit block reaches past num_vars");
        LURK_REQUIRE((unsigned __int128)d.num_cons * n_blocks + extra_cons < lim, "more than 2^32 - 1 rows");
        const SlotCircuit c = circuit_rows(field_id, height, op);
        for (int w = 0; w < 3; w++)
            LURK_REQUIRE((unsigned __int128)c.m[w].indices.size() * n_blocks + (extra_cons ? xip[w][extra_cons] : 0) < lim, "more than 2^32 - 1 non-zeros");
        const size_t rows = d.num_cons * n_blocks + extra_cons;
        std::vector<uint64_t> ip[3], ix[3], dv[3];
        for (int w = 0; w < 3; w++) {
            const SlotMatrix& m = c.m[w];
            const size_t nnz = m.indices.size() * n_blocks + (extra_cons ? xip[w][extra_cons] : 0);
            ip[w].reserve(rows + 1);
            ix[w].reserve(nnz);
            dv[w].reserve(nnz * 4);
            ip[w].push_back(0);
            for (size_t b = 0; b < n_blocks; b++) {
                const size_t base = first + b * stride, at = ix[w].size();
                for (uint64_t col : m.indices) ix[w].push_back(col == c.size ? num_vars : base + col);  // ONE is u's column
                dv[w].insert(dv[w].end(), m.data.begin(), m.data.end());
                for (size_t r = 1; r < m.indptr.size(); r++) ip[w].push_back(at + m.indptr[r]);
            }
            if (extra_cons) {
                const size_t at = ix[w].size(), xn = xip[w][extra_cons];
                for (size_t r = 1; r <= extra_cons; r++) {
                    LURK_REQUIRE(xip[w][r] >= xip[w][r - 1] && xip[w][r] <= xn, "extra rows: indptr must be non-decreasing");
                    ip[w].push_back(at + xip[w][r]);
                }
                ix[w].insert(ix[w].end(), xix[w], xix[w] + xn);
                const uint64_t* xd = (const uint64_t*)xdv[w];
                dv[w].insert(dv[w].end(), xd, xd + 4 * xn);
            }
        }
        LURK_REQUIRE(rows > 0, "no rows");
        nested_ok(lurk_hip_r1cs_create(shape, field_id, rows, num_vars, num_io, ip[0].data(), ix[0].data(), dv[0].data(), ip[1].data(), ix[1].data(), dv[1].data(),
                                       ip[2].data(), ix[2].data(), dv[2].data()));
    });
}

int lurk_hip_trie_circuit_witness_dev(int field_id, int height, int op, const void* d_roots32, size_t root_stride, const void* d_keys32,
                                      const void* d_new_values32, const void* d_old_paths, const void* d_new_paths, size_t m, void* d_w, const uint64_t* d_offsets,
                                      size_t first, size_t stride, void* stream) {
    return guarded([&] {
        const TrieCircuitDims d = circuit_dims(field_id, height, op);
        const bool insert = op == LURK_TRIE_CIRCUIT_INSERT;
        LURK_REQUIRE(m <= ((size_t)1 << 28), "more than 2^28 circuit blocks in one call");
        LURK_REQUIRE(root_stride <= 1, "root_stride must be 0 (one root for every block) or 1 (one root per block)");
        LURK_REQUIRE(insert || (!d_new_values32 && !d_new_paths), "a lookup takes no new values and no new paths: both must be NULL");
        if (m == 0) return;
        LURK_REQUIRE(d_roots32 && d_keys32 && d_old_paths && d_w, "null buffer");
        LURK_REQUIRE(!insert || (d_new_values32 && d_new_paths), "null buffer (an insert takes the new values and the new paths)");
        LURK_REQUIRE(d_offsets || m <= 1 || stride >= d.size, "stride shorter than a circuit block");
        TrieCircuitJob job{(const uint4*)d_old_paths, (const uint4*)d_new_paths, (const uint32_t*)d_keys32, d_w, d_offsets, first, stride,
                           m * (size_t)height, d.key_block, d.size_lookup, height};
        with_field(field_id,
                   [&](auto F) { launch_trie_circuit<decltype(F)>(job, m, insert, d_roots32, root_stride, d_new_values32, field_id, (hipStream_t)stream); });
    });
}

}  // extern "C"
