// r1cs_sat.hip - "is this (relaxed) R1CS instance satisfied, and if not where", on the device.
//
// arecibo's R1CSShape::is_sat / is_sat_relaxed: A z o B z == u C z + E row by row, with z = [W | u | X].  A host without this call runs
// lurk_hip_r1cs_multiply_vec_dev and pulls three vectors of num_cons x 32 B back; here a row's three inner products are formed, combined
// as the lazy three-term row  Az * Bz + (-u) * Cz + (-E) * 1  (poseidon29.cuh: Dot29, as the cross term's T in fold.hip), reduced
// canonically and compared with zero - nothing is written per row.  Failing rows are counted and the lowest one is kept through
// atomicAdd / atomicMin on one 16-byte device record (one pair of atomics per wave that holds a failing row).
//
// Row classes.  The lane-per-row kernels of fold.hip are built for the step circuit's synthetic stand-in (3-4 entries per row, a few
// 255-entry bit decompositions).  The slot gadgets' own rows (slot_circuit.hpp) are different: about a third of a Poseidon slot's rows
// carry a linear combination of 8 to 66 entries in A and / or B (the partial rounds), and a wave of 64 neighbouring rows waits for its one
// 60-entry lane.  Rows are therefore classed once per shape, on the first call, into lane / mid / wide rows and one launch covers the
// three classes: r1cs_shape.cuh has the classes (RowClasses), the row product (r1cs_row) and its bounds.
//
// The coefficient dictionary is read through L2 as in fold.hip, or (LURK_SAT_LDS=1, an experiment kept for measurement) copied into LDS
// by 512-thread persistent workgroups, one per CU - see DESIGN.md for what each variant measured.
//
// Also here: the slot gadgets' constraint rows at the C ABI (lurk_hip_slot_constraints*) and the resident shape of a MultiFrame's slots
// (lurk_hip_frames_r1cs_create).
#include <cstdlib>
#include <memory>

#include "dispatch.hpp"
#include "r1cs_bn254fq.hpp"
#include "r1cs_shape.cuh"
#include "slot_circuit.hpp"

namespace lurk {

size_t slot_witness_size(int field_id, int slot_type);  // poseidon.hip

constexpr int SAT_PERSIST_BLOCK = 512;  // two waves per SIMD: 1024 threads leave 128 registers per lane and the row accumulators spill

struct SatDev {
    R1csDev s;
    RowClassDev c;
    size_t u_index;
    unsigned long long* rec;
};

// 256 lanes of one class
template <class P, int G, bool ANY_LEN, bool LDS>
__device__ __forceinline__ void sat_class(const SatDev& d, const uint32_t* dict, const uint32_t* list, uint32_t n, unsigned vb, unsigned nb, uint32_t tid,
                                          const Fe<P>* __restrict__ z, const Fe<P>* __restrict__ e) {
    const uint32_t* one29 = dict + d.s.dict_size * P29_STRIDE;  // the Montgomery one closes the dictionary
    const RowSlot slot = row_slot<G>(list, n, fold_row_block(vb, nb), tid);
    if (G == 1 && !slot.live) return;
    const uint32_t row = slot.row, gl = slot.gl;
    const F29<P> a = r1cs_row<P, G, ANY_LEN, LDS>(d.s.a, dict, one29, d.s.a.rowptr[row], d.s.a.rowptr[row + 1], gl, z);
    const F29<P> b = r1cs_row<P, G, ANY_LEN, LDS>(d.s.b, dict, one29, d.s.b.rowptr[row], d.s.b.rowptr[row + 1], gl, z);
    const F29<P> c = r1cs_row<P, G, ANY_LEN, LDS>(d.s.c, dict, one29, d.s.c.rowptr[row], d.s.c.rowptr[row + 1], gl, z);
    bool fail = false;
    if (slot.live && gl == 0) {
        Dot29<P> acc;
        dot29_init<P>(acc);
        dot29_mac<P>(acc, a, b);
        dot29_mac<P>(acc, f29_from_mont256<P>(fe_neg<P>(z[d.u_index])), c);  // 32 (-u) 2^256: tight, < 2^259 (fold.hip, the cross term)
        if (e) dot29_mac<P>(acc, f29_from_mont256<P>(fe_neg<P>(e[row])), r1cs_coeff<P, LDS>(one29, 0));
        const Fe<P> v = f29_to_mont256<P>(dot29_finish<P>(acc));  // canonical
        uint32_t any = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) any |= v.l[i];
        fail = any != 0;
    }
    // rows ascend with the lane in every class: the lowest failing lane of a wave holds the wave's lowest failing row
    const unsigned long long m = __ballot(fail);
    if (fail && (m & ((1ull << (threadIdx.x & 63)) - 1ull)) == 0) {
        atomicAdd(d.rec, (unsigned long long)__popcll(m));
        atomicMin(d.rec + 1, (unsigned long long)row);
    }
}

// virtual block j of the concatenated classes
template <class P, int GM, bool LDS>
__device__ __forceinline__ void sat_vblock(const SatDev& d, const uint32_t* dict, unsigned j, uint32_t tid, const Fe<P>* __restrict__ z,
                                           const Fe<P>* __restrict__ e) {
    row_class_vblock<GM>(d.c, j, [&](auto g, auto any_len, const uint32_t* list, uint32_t n, unsigned vb, unsigned nb) {
        sat_class<P, decltype(g)::value, decltype(any_len)::value, LDS>(d, dict, list, n, vb, nb, tid, z, e);
    });
}

template <class P, int GM>
__global__ __launch_bounds__(FOLD_BLOCK) void r1cs_sat_kernel(SatDev d, const Fe<P>* __restrict__ z, const Fe<P>* __restrict__ e) {
    sat_vblock<P, GM, false>(d, d.s.dict, blockIdx.x, threadIdx.x, z, e);
}

// the dictionary in LDS: one 512-thread workgroup per CU copies it once and walks virtual blocks gridDim.x * 2 apart (gridDim.x is a
// multiple of FOLD_XCDS: a workgroup's virtual blocks keep its XCD's residue, fold_row_block's contract)
template <class P, int GM>
__global__ __launch_bounds__(SAT_PERSIST_BLOCK) void r1cs_sat_lds_kernel(SatDev d, const Fe<P>* __restrict__ z, const Fe<P>* __restrict__ e) {
    extern __shared__ uint32_t sat_dict[];
    const uint32_t words = (uint32_t)(d.s.dict_size + 1) * P29_STRIDE;
    for (uint32_t i = threadIdx.x; i < words / 4; i += SAT_PERSIST_BLOCK) ((uint4*)sat_dict)[i] = ((const uint4*)d.s.dict)[i];
    __syncthreads();
    const unsigned total = d.c.wide_blocks + d.c.mid_blocks + d.c.lane_blocks;
    for (unsigned j = (threadIdx.x >> 8) * gridDim.x + blockIdx.x; j < total; j += gridDim.x * (SAT_PERSIST_BLOCK / FOLD_BLOCK))
        sat_vblock<P, GM, true>(d, sat_dict, j, threadIdx.x & (FOLD_BLOCK - 1), z, e);
}

// ---- host side ---------------------------------------------------------------------------------------------
static uint32_t env_u32(const char* name, uint32_t dflt) {
    const char* v = getenv(name);
    return v && *v ? (uint32_t)strtoul(v, nullptr, 10) : dflt;
}

// (sat_mu held)
static SatPlan& sat_plan(const R1csShape& sh, uint32_t lane_max, uint32_t mid_max) {
    if (sh.sat && sh.sat->cls.lane_max == lane_max && sh.sat->cls.mid_max == mid_max) return *sh.sat;
    auto plan = std::make_unique<SatPlan>();
    build_row_classes(plan->cls, sh, lane_max, mid_max, false);
    plan->rec.alloc(16);
    LURK_HIP_CHECK(hipHostMalloc((void**)&plan->host, 32, hipHostMallocDefault));
    sh.sat = std::move(plan);
    return *sh.sat;
}

template <class P, int GM>
static void sat_launch(const SatDev& d, bool lds, size_t dict_size, const void* d_z, const void* d_e, hipStream_t s) {
    const unsigned total = d.c.wide_blocks + d.c.mid_blocks + d.c.lane_blocks;
    if (lds) {
        const int bytes = (int)((dict_size + 1) * P29_STRIDE * 4);
        allow_dynamic_lds((const void*)r1cs_sat_lds_kernel<P, GM>, bytes);
        const unsigned cus = (unsigned)num_cus() / FOLD_XCDS * FOLD_XCDS;
        const unsigned grid = std::max(FOLD_XCDS, std::min(cus, total / (SAT_PERSIST_BLOCK / FOLD_BLOCK) / FOLD_XCDS * FOLD_XCDS));
        hipLaunchKernelGGL((r1cs_sat_lds_kernel<P, GM>), dim3(grid), dim3(SAT_PERSIST_BLOCK), bytes, s, d, (const Fe<P>*)d_z, (const Fe<P>*)d_e);
    } else {
        hipLaunchKernelGGL((r1cs_sat_kernel<P, GM>), dim3(total), dim3(FOLD_BLOCK), 0, s, d, (const Fe<P>*)d_z, (const Fe<P>*)d_e);
    }
    LURK_HIP_CHECK(hipGetLastError());
}

template <class P>
static void is_sat(const R1csShape& sh, const void* d_z, const void* d_e, uint64_t* n_unsat, uint64_t* first_unsat, hipStream_t s) {
    if (!sh.num_cons) {
        *n_unsat = 0;
        *first_unsat = 0;
        return;
    }
    // measurement switches ("satisfiability"): the defaults are the variant that was kept
    const uint32_t lane_max = env_u32("LURK_SAT_LANE_MAX", SAT_LANE_MAX), group = env_u32("LURK_SAT_GROUP", SAT_GROUP);
    const uint32_t mid_max = std::min(env_u32("LURK_SAT_MID_MAX", SAT_MID_MAX), 256u);  // the mid class adds partial sums limb-wise: <= 256 entries
    bool lds = env_u32("LURK_SAT_LDS", 0) != 0;
    LURK_REQUIRE(group == 4 || group == 8 || group == 16, "LURK_SAT_GROUP must be 4, 8 or 16");
    LURK_REQUIRE(lane_max <= mid_max, "LURK_SAT_LANE_MAX above LURK_SAT_MID_MAX");
    if ((sh.dict_size + 1) * P29_STRIDE * 4 > 144 * 1024) lds = false;  // does not fit beside nothing: through L2
    std::lock_guard<std::mutex> lk(sh.sat_mu);  // one record per shape: checks of one shape run one after the other
    SatPlan& plan = sat_plan(sh, lane_max, mid_max);
    SatDev d;
    d.s = dev_view(sh);
    d.c = class_view(plan.cls, (int)group);
    d.u_index = sh.num_vars;
    d.rec = plan.rec.as<unsigned long long>();
    plan.host[0] = 0;
    plan.host[1] = sh.num_cons;
    ProfScope ps("r1cs_is_sat", s);
    LURK_HIP_CHECK(hipMemcpyAsync(plan.rec.p, plan.host, 16, hipMemcpyHostToDevice, s));
    if (group == 4) sat_launch<P, 4>(d, lds, sh.dict_size, d_z, d_e, s);
    else if (group == 8) sat_launch<P, 8>(d, lds, sh.dict_size, d_z, d_e, s);
    else sat_launch<P, 16>(d, lds, sh.dict_size, d_z, d_e, s);
    LURK_HIP_CHECK(hipMemcpyAsync(plan.host + 2, plan.rec.p, 16, hipMemcpyDeviceToHost, s));
    LURK_HIP_CHECK(hipStreamSynchronize(s));
    *n_unsat = plan.host[2];
    *first_unsat = plan.host[3];
}

#ifdef LURK_SAT_BN254FQ_TU  // r1cs_sat_bn254fq.hip: the instantiation over the BN254 base field, a code object of its own (the row bounds
                            // for this modulus: fold.hip); this unit reaches it through r1cs_bn254fq.hpp only
void is_sat_bn254fq(const R1csShape& sh, const void* d_z, const void* d_e, uint64_t* n_unsat, uint64_t* first_unsat, hipStream_t s) {
    is_sat<Bn254Fq>(sh, d_z, d_e, n_unsat, first_unsat, s);
}

}  // namespace lurk
#else
// ---- the slot gadgets' rows ------------------------------------------------------------------------------------
static bool slot_is_hash_type(int slot_type) { return slot_type == 3 || slot_type == 4 || slot_type == 6 || slot_type == 8; }

const SlotCircuit& slot_circuit(int field_id, int slot_type) {  // also trie_circuit.hip
    LURK_REQUIRE(field_id >= 0 && field_id <= 2, "unknown field id");
    LURK_REQUIRE(slot_is_hash_type(slot_type) || slot_type == LURK_SLOT_BIT_DECOMP, "unknown slot type");
    static std::mutex mu;
    static std::map<std::pair<int, int>, std::unique_ptr<SlotCircuit>> built;
    std::lock_guard<std::mutex> lk(mu);
    std::unique_ptr<SlotCircuit>& c = built[std::make_pair(field_id, slot_type)];
    if (!c) {
        c = std::make_unique<SlotCircuit>();
        with_field(field_id, [&](auto F) {
            *c = slot_type == LURK_SLOT_BIT_DECOMP ? bit_decomp_slot_circuit<decltype(F)>() : poseidon_slot_circuit<decltype(F)>(slot_type);
        });
    }
    return *c;
}

}  // namespace lurk

using namespace lurk;

extern "C" {

int lurk_hip_slot_constraints_size(int field_id, int slot_type, size_t* num_cons, size_t* nnz_a, size_t* nnz_b, size_t* nnz_c) {
    return host_guarded([&] {
        LURK_REQUIRE(num_cons && nnz_a && nnz_b && nnz_c, "null output");
        const SlotCircuit& c = slot_circuit(field_id, slot_type);
        *num_cons = c.num_cons;
        *nnz_a = c.m[0].indices.size();
        *nnz_b = c.m[1].indices.size();
        *nnz_c = c.m[2].indices.size();
    });
}

int lurk_hip_slot_constraints(int field_id, int slot_type, uint64_t* a_indptr, uint64_t* a_indices, void* a_data, uint64_t* b_indptr, uint64_t* b_indices,
                              void* b_data, uint64_t* c_indptr, uint64_t* c_indices, void* c_data) {
    return host_guarded([&] {
        LURK_REQUIRE(a_indptr && a_indices && a_data && b_indptr && b_indices && b_data && c_indptr && c_indices && c_data, "null output");
        const SlotCircuit& c = slot_circuit(field_id, slot_type);
        uint64_t* ip[3] = {a_indptr, b_indptr, c_indptr};
        uint64_t* ix[3] = {a_indices, b_indices, c_indices};
        void* dv[3] = {a_data, b_data, c_data};
        for (int w = 0; w < 3; w++) {
            const SlotMatrix& m = c.m[w];
            memcpy(ip[w], m.indptr.data(), m.indptr.size() * 8);
            if (!m.indices.empty()) {
                memcpy(ix[w], m.indices.data(), m.indices.size() * 8);
                memcpy(dv[w], m.data.data(), m.data.size() * 8);
            }
        }
    });
}

int lurk_hip_frames_r1cs_create(lurk_hip_r1cs** shape, int field_id, size_t num_frames, const size_t* counts5, size_t first, size_t frame_len,
                                size_t num_vars, size_t num_io, size_t extra_cons, const uint64_t* xa_indptr, const uint64_t* xa_indices, const void* xa_data,
                                const uint64_t* xb_indptr, const uint64_t* xb_indices, const void* xb_data, const uint64_t* xc_indptr,
                                const uint64_t* xc_indices, const void* xc_data) {
    return guarded([&] {
        LURK_REQUIRE(shape, "null output handle");
        *shape = nullptr;
        LURK_REQUIRE(field_id >= 0 && field_id <= 2, "unknown field id");
        LURK_REQUIRE(counts5, "null slot counts");
        static const int types[5] = {LURK_SLOT_HASH4, LURK_SLOT_HASH6, LURK_SLOT_HASH8, LURK_SLOT_COMMITMENT, LURK_SLOT_BIT_DECOMP};
        const uint64_t* xip[3] = {xa_indptr, xb_indptr, xc_indptr};
        const uint64_t* xix[3] = {xa_indices, xb_indices, xc_indices};
        const void* xdv[3] = {xa_data, xb_data, xc_data};
        for (int w = 0; w < 3; w++)
            LURK_REQUIRE(extra_cons == 0 || (xip[w] && xip[w][0] == 0 && (xip[w][extra_cons] == 0 || (xix[w] && xdv[w]))), "malformed extra rows");
        // every size in 128 bits first: nothing is allocated for a layout that does not fit
        const unsigned __int128 lim = (unsigned __int128)1 << 32;
        const SlotCircuit* circ[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
        unsigned __int128 slots_len = 0, frame_rows = 0, frame_nnz[3] = {0, 0, 0};
        for (int k = 0; k < 5; k++) {
            if (!counts5[k]) continue;
            LURK_REQUIRE(counts5[k] < lim, "slot count overflows");
            circ[k] = &slot_circuit(field_id, types[k]);
            LURK_REQUIRE(circ[k]->size == slot_witness_size(field_id, types[k]), "slot rows and slot witness disagree on the block size");
            slots_len += (unsigned __int128)counts5[k] * circ[k]->size;
            frame_rows += (unsigned __int128)counts5[k] * circ[k]->num_cons;
            for (int w = 0; w < 3; w++) frame_nnz[w] += (unsigned __int128)counts5[k] * circ[k]->m[w].indices.size();
        }
        LURK_REQUIRE(num_vars < lim && num_io < lim && num_vars + 1 + num_io < lim, "z has more than 2^32 - 1 entries");
        LURK_REQUIRE(num_frames < lim && frame_len < lim && first < lim && extra_cons < lim, "layout overflows");
        LURK_REQUIRE(num_frames <= 1 || frame_len >= slots_len, "frame_len shorter than the frame's slot blocks");
        if (num_frames)
            LURK_REQUIRE((unsigned __int128)first + (unsigned __int128)(num_frames - 1) * frame_len + slots_len <= num_vars,
                         "a slot block reaches past num_vars");
        const unsigned __int128 rows128 = frame_rows * num_frames + extra_cons;
        LURK_REQUIRE(rows128 < lim, "more than 2^32 - 1 rows");
        for (int w = 0; w < 3; w++)
            LURK_REQUIRE(frame_nnz[w] * num_frames + (extra_cons ? xip[w][extra_cons] : 0) < lim, "more than 2^32 - 1 non-zeros");
        const size_t rows = (size_t)rows128;
        // the whole shape as host CSR, handed to lurk_hip_r1cs_create (which builds the dictionary and the long-row list)
        std::vector<uint64_t> ip[3], ix[3], dv[3];
        for (int w = 0; w < 3; w++) {
            const size_t nnz = (size_t)(frame_nnz[w] * num_frames) + (extra_cons ? xip[w][extra_cons] : 0);
            ip[w].reserve(rows + 1);
            ix[w].reserve(nnz);
            dv[w].reserve(nnz * 4);
            ip[w].push_back(0);
            for (size_t f = 0; f < num_frames; f++) {
                size_t base = first + f * frame_len;
                for (int k = 0; k < 5; k++)
                    for (size_t j = 0; j < counts5[k]; j++) {
                        const SlotMatrix& m = circ[k]->m[w];
                        const size_t size = circ[k]->size, at = ix[w].size();
                        for (uint64_t col : m.indices) ix[w].push_back(col == size ? num_vars : base + col);  // ONE is u's column
                        dv[w].insert(dv[w].end(), m.data.begin(), m.data.end());
                        for (size_t r = 1; r < m.indptr.size(); r++) ip[w].push_back(at + m.indptr[r]);
                        base += size;
                    }
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
        LURK_REQUIRE(lurk_hip_r1cs_create(shape, field_id, rows, num_vars, num_io, ip[0].data(), ix[0].data(), dv[0].data(), ip[1].data(), ix[1].data(),
                                          dv[1].data(), ip[2].data(), ix[2].data(), dv[2].data()) == 0,
                     lurk_hip_last_error());
    });
}

int lurk_hip_r1cs_is_sat_dev(const lurk_hip_r1cs* shape, const void* d_z, const void* d_e, uint64_t* n_unsat, uint64_t* first_unsat, void* stream) {
    return guarded([&] {
        LURK_REQUIRE(shape && d_z && n_unsat && first_unsat, "null argument");
        const R1csShape& sh = shape->sh;
        LURK_REQUIRE(current_device() == sh.device, "the shape is resident on another device than the current one");
        if (sh.field_id == LURK_FIELD_BN254_FQ) is_sat_bn254fq(sh, d_z, d_e, n_unsat, first_unsat, (hipStream_t)stream);
        else with_field(sh.field_id, [&](auto F) { is_sat<decltype(F)>(sh, d_z, d_e, n_unsat, first_unsat, (hipStream_t)stream); });
    });
}

}  // extern "C"
#endif  // LURK_SAT_BN254FQ_TU
