// r1cs_transpose.hip - the transpose of a resident R1CS shape, made on the device (lurk_hip_r1cs_transpose_dev), and a resident shape
// read back to the host as the CSR lurk_hip_r1cs_create takes (lurk_hip_r1cs_read).
//
// The compressing provers (spartan.hip) run their inner sum-check over the transposed shape: 2 num_vars rows over num_cons columns.  A
// resident shape already holds, per non-zero, {column, coefficient id} and a dictionary of the distinct coefficients; its transpose
// holds {row, coefficient id} in column order and the SAME dictionary, so nothing of it has to be hashed, converted or uploaded again.
//
// Per matrix:
//   1. expand:  entry k -> key = its column, payload = {its row, its coefficient id}.  The row of entry k is not stored: a workgroup
//      finds the rows of its first and last entry by bisection of rowptr, every lane then bisects between those two.
//   2. a stable radix sort of the pairs by key (rocPRIM, over the bits the column ids need): equal columns keep their input order, which
//      is ascending row and, inside one row, the order of the source - what a stable argsort of the column indices gives on the host.
//      The sorted payloads ARE the transposed matrix's entry records.
//   3. rowptr' from the run boundaries of the sorted keys: one lane per row pointer bisects for the place where its column's run begins
//      (for an untouched column, where it would), between the places its workgroup found for its first and last pointer.
// Then one pass over the three rowptr' marks the rows with more than FOLD_LONG entries and compacts their ids in ascending order
// (ballot ranks inside a wave, workgroup counts scanned by rocPRIM).  Nothing counts through atomics - a step circuit has an entry in
// the u column in almost every row, which would put ~num_cons atomics on one address - so the result is the same bytes on every run.
//
// Scratch (the stream's arena): two key arrays and one payload array over the largest matrix - 16 B per non-zero, twice that matrix's
// entry array; the second payload array of the sort is the output itself - plus rocPRIM's own storage (histograms and look-back state,
// no copy of the data) and 8 B per 256 output rows.
#include <memory>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "common.hpp"
#include "dispatch.hpp"
#include "r1cs_shape.cuh"

namespace lurk {

constexpr int TR_BLOCK = 256;     // one entry (expand, rowptr') or one output row (long rows) per lane
static_assert(TR_BLOCK == 4 * 64, "the long-row kernels sum four wave64 ballots");

// the row of entry k: the largest i in [lo, hi] with rowptr[i] <= k (empty rows share their successor's pointer and are passed over)
__device__ __forceinline__ uint32_t tr_row_of(const uint32_t* __restrict__ rowptr, uint32_t lo, uint32_t hi, uint32_t k) {
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (rowptr[mid] <= k)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// nnz > 0 (so rows > 0); grid = ceil(nnz / TR_BLOCK)
__global__ __launch_bounds__(TR_BLOCK) void r1cs_transpose_expand_kernel(const uint32_t* __restrict__ rowptr, const uint2* __restrict__ ent, uint32_t rows,
                                                                         uint32_t nnz, uint32_t* __restrict__ keys, uint2* __restrict__ vals) {
    __shared__ uint32_t bound[2];
    const size_t k0 = (size_t)blockIdx.x * TR_BLOCK;
    if (threadIdx.x < 2) {
        const size_t last = k0 + TR_BLOCK - 1 < (size_t)nnz ? k0 + TR_BLOCK - 1 : (size_t)nnz - 1;
        bound[threadIdx.x] = tr_row_of(rowptr, 0, rows - 1, (uint32_t)(threadIdx.x ? last : k0));
    }
    __syncthreads();
    const size_t k = k0 + threadIdx.x;
    if (k >= nnz) return;
    const uint32_t row = tr_row_of(rowptr, bound[0], bound[1], (uint32_t)k);
    const uint2 e = ent[k];
    keys[k] = e.x;
    vals[k] = make_uint2(row, e.y);
}

// where the run of key j begins among the sorted keys: the first position in [lo, hi] whose key is not below j (hi when there is none)
__device__ __forceinline__ uint32_t tr_run_begin(const uint32_t* __restrict__ skeys, uint32_t lo, uint32_t hi, uint32_t j) {
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (skeys[mid] < j)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// nnz > 0; grid covers the rows_t + 1 row pointers, one lane each: rowptr_t[j] = the boundary of run j in the sorted keys.  As in the
// expansion, the workgroup bisects for its first and last row pointer and every lane between those two - an untouched column, or any
// stretch of them, costs its lanes one short search each.  (Seen from the entries - the first entry of a run writes the pointers of the
// columns before it - a stretch of 2^19 untouched columns, which the compressing benchmark's matrices have between W's free part and u,
// is 2^19 stores of one lane: measured, that call took 22.2 ms and takes 0.65 ms this way.)
__global__ __launch_bounds__(TR_BLOCK) void r1cs_transpose_rowptr_kernel(const uint32_t* __restrict__ skeys, uint32_t nnz, uint32_t rows_t,
                                                                         uint32_t* __restrict__ rowptr_t) {
    __shared__ uint32_t bound[2];
    const size_t j0 = (size_t)blockIdx.x * TR_BLOCK;
    if (threadIdx.x < 2) {
        const size_t last = j0 + TR_BLOCK - 1 < (size_t)rows_t ? j0 + TR_BLOCK - 1 : (size_t)rows_t;
        bound[threadIdx.x] = tr_run_begin(skeys, 0, nnz, (uint32_t)(threadIdx.x ? last : j0));
    }
    __syncthreads();
    const size_t j = j0 + threadIdx.x;
    if (j > rows_t) return;
    rowptr_t[j] = tr_run_begin(skeys, bound[0], bound[1], (uint32_t)j);
}

__device__ __forceinline__ bool tr_is_long(const uint32_t* __restrict__ ra, const uint32_t* __restrict__ rb, const uint32_t* __restrict__ rc, size_t j) {
    return ra[j + 1] - ra[j] > FOLD_LONG || rb[j + 1] - rb[j] > FOLD_LONG || rc[j + 1] - rc[j] > FOLD_LONG;
}

// counts[b] = the long rows among rows [b TR_BLOCK, (b + 1) TR_BLOCK)
__global__ __launch_bounds__(TR_BLOCK) void r1cs_transpose_long_count_kernel(const uint32_t* __restrict__ ra, const uint32_t* __restrict__ rb,
                                                                             const uint32_t* __restrict__ rc, uint32_t rows_t, uint32_t* __restrict__ counts) {
    __shared__ uint32_t wave_n[TR_BLOCK / 64];
    const size_t j = (size_t)blockIdx.x * TR_BLOCK + threadIdx.x;
    const bool is_long = j < rows_t && tr_is_long(ra, rb, rc, j);
    const unsigned long long b = __ballot(is_long);
    if ((threadIdx.x & 63) == 0) wave_n[threadIdx.x >> 6] = (uint32_t)__popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
}

// offs = the exclusive scan of counts; long_rows has room for every long row (the host sizes it by the pigeonhole bound)
__global__ __launch_bounds__(TR_BLOCK) void r1cs_transpose_long_write_kernel(const uint32_t* __restrict__ ra, const uint32_t* __restrict__ rb,
                                                                             const uint32_t* __restrict__ rc, uint32_t rows_t, const uint32_t* __restrict__ offs,
                                                                             uint32_t* __restrict__ long_rows) {
    __shared__ uint32_t wave_n[TR_BLOCK / 64];
    const size_t j = (size_t)blockIdx.x * TR_BLOCK + threadIdx.x;
    const bool is_long = j < rows_t && tr_is_long(ra, rb, rc, j);
    const unsigned long long b = __ballot(is_long);
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wave_n[wave] = (uint32_t)__popcll(b);
    __syncthreads();
    if (!is_long) return;
    uint32_t at = offs[blockIdx.x];
    for (unsigned w = 0; w < wave; w++) at += wave_n[w];
    at += (uint32_t)__popcll(b & ((1ull << lane) - 1));
    long_rows[at] = (uint32_t)j;
}

// the inverse of fold.hip's dict_record: canonical radix-2^29 limbs of c 2^261 mod p -> c 2^256 mod p as the ABI carries it
template <class P>
static void dict_value(const uint32_t* rec, uint64_t* mont256) {
    F29<P> f;
    for (int i = 0; i < 9; i++) f.l[i] = rec[i];
    uint32_t w[8];
    f29_pack<P>(f, w);
    for (int d = 0; d < 5; d++) {  // halve modulo p: v < p < 2^255, so v + p fits 256 bits
        if (w[0] & 1) {
            uint64_t carry = 0;
            for (int i = 0; i < 8; i++) {
                carry += (uint64_t)w[i] + P::mod(i);
                w[i] = (uint32_t)carry;
                carry >>= 32;
            }
        }
        for (int i = 0; i < 8; i++) w[i] = (w[i] >> 1) | (i + 1 < 8 ? w[i + 1] << 31 : 0u);
    }
    for (int i = 0; i < 4; i++) mont256[i] = (uint64_t)w[2 * i] | (uint64_t)w[2 * i + 1] << 32;
}

static unsigned bits_for(size_t n) {  // the bits that hold every value below n (at least one)
    unsigned b = 1;
    while (b < 32 && ((size_t)1 << b) < n) b++;
    return b;
}

}  // namespace lurk

using namespace lurk;

extern "C" {

int lurk_hip_r1cs_transpose_dev(const lurk_hip_r1cs* shape, size_t rows_t, lurk_hip_r1cs** out, void* stream) {
    if (out) *out = nullptr;
    return guarded([&] {
        LURK_REQUIRE(shape && out, "null argument");
        const R1csShape& src = shape->sh;
        // a shape over the BN254 base field (lurk_hip_r1cs_create_for_curve on Grumpkin) folds; nothing that takes a transpose is offered over it
        LURK_REQUIRE(src.field_id != LURK_FIELD_BN254_FQ, "lurk_hip_r1cs_transpose_dev is not offered for a shape over the BN254 base field (Grumpkin's scalar field)");
        const size_t ncols = src.num_vars + 1 + src.num_io, lim = (size_t)1 << 32;
        LURK_REQUIRE(src.num_cons > 0, "a shape without rows has no transpose (num_cons = 0)");
        LURK_REQUIRE(src.num_cons < lim, "more than 2^32 - 1 rows");
        LURK_REQUIRE(rows_t < lim, "rows_t must be below 2^32");
        LURK_REQUIRE(rows_t == 0 || rows_t >= ncols, "rows_t is below the shape's num_vars + 1 + num_io columns");
        LURK_REQUIRE(current_device() == src.device, "the shape is resident on another device than the current one");
        if (!rows_t) rows_t = ncols;
        hipStream_t s = (hipStream_t)stream;
        const uint32_t rows = (uint32_t)src.num_cons, rt = (uint32_t)rows_t;

        auto h = std::make_unique<lurk_hip_r1cs>();
        R1csShape& dst = h->sh;
        dst.field_id = src.field_id;
        dst.num_cons = rows_t;
        dst.num_vars = src.num_cons - 1;
        dst.num_io = 0;
        dst.device = src.device;
        dst.dict_size = src.dict_size;
        size_t max_nnz = 0, total_nnz = 0;
        for (int w = 0; w < 3; w++) {
            dst.m[w].nnz = src.m[w].nnz;
            dst.m[w].rowptr.alloc((rows_t + 1) * 4);
            dst.m[w].ent.alloc(src.m[w].nnz * 8);
            max_nnz = src.m[w].nnz > max_nnz ? src.m[w].nnz : max_nnz;
            total_nnz += src.m[w].nnz;
        }
        const size_t dict_bytes = (src.dict_size + 1) * P29_STRIDE * 4;  // with the closing record, the Montgomery one
        dst.dict.alloc(dict_bytes);
        // a long row holds at least FOLD_LONG + 1 entries of the three matrices together
        const size_t long_cap = total_nnz / (FOLD_LONG + 1) < rows_t ? total_nnz / (FOLD_LONG + 1) : rows_t;
        dst.long_rows.alloc(long_cap * 4);

        ProfScope ps("r1cs_transpose", s);
        LURK_HIP_CHECK(hipMemcpyAsync(dst.dict.p, src.dict.p, dict_bytes, hipMemcpyDeviceToDevice, s));
        const unsigned end_bit = bits_for(ncols);
        const unsigned row_blocks = div_up(rows_t, TR_BLOCK);
        size_t temp_bytes = 0;  // the largest of the three sorts (rocPRIM picks its algorithm, and with it its storage, by size) and the scan
        {
            rocprim::double_buffer<uint32_t> qk((uint32_t*)nullptr, (uint32_t*)nullptr);
            rocprim::double_buffer<uint64_t> qv((uint64_t*)nullptr, (uint64_t*)nullptr);
            for (int w = 0; w < 3; w++) {
                size_t bytes = 0;
                if (src.m[w].nnz) LURK_HIP_CHECK(rocprim::radix_sort_pairs(nullptr, bytes, qk, qv, (uint32_t)src.m[w].nnz, 0, end_bit, s));
                temp_bytes = bytes > temp_bytes ? bytes : temp_bytes;
            }
            size_t bytes = 0;
            LURK_HIP_CHECK(rocprim::exclusive_scan(nullptr, bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, (size_t)row_blocks + 1, rocprim::plus<uint32_t>(), s));
            temp_bytes = bytes > temp_bytes ? bytes : temp_bytes;
        }
        ArenaBuf keys(2 * max_nnz * 4, s), vals(max_nnz * 8, s), counts(2 * ((size_t)row_blocks + 1) * 4, s), temp(temp_bytes, s);
        for (int w = 0; w < 3; w++) {
            const CsrDev& m = src.m[w];
            uint32_t* rp_t = dst.m[w].rowptr.as<uint32_t>();
            if (!m.nnz) {
                LURK_HIP_CHECK(hipMemsetAsync(rp_t, 0, (rows_t + 1) * 4, s));
                continue;
            }
            const uint32_t nnz = (uint32_t)m.nnz;
            uint32_t* k0 = (uint32_t*)keys.p;
            hipLaunchKernelGGL(r1cs_transpose_expand_kernel, dim3(div_up(m.nnz, TR_BLOCK)), dim3(TR_BLOCK), 0, s, m.rowptr.as<uint32_t>(), m.ent.as<uint2>(), rows, nnz, k0,
                               (uint2*)vals.p);
            LURK_HIP_CHECK(hipGetLastError());
            rocprim::double_buffer<uint32_t> dk(k0, k0 + max_nnz);
            rocprim::double_buffer<uint64_t> dv((uint64_t*)vals.p, dst.m[w].ent.as<uint64_t>());
            size_t bytes = temp_bytes;
            LURK_HIP_CHECK(rocprim::radix_sort_pairs(temp.p, bytes, dk, dv, nnz, 0, end_bit, s));
            if (dv.current() != dst.m[w].ent.as<uint64_t>())
                LURK_HIP_CHECK(hipMemcpyAsync(dst.m[w].ent.p, dv.current(), m.nnz * 8, hipMemcpyDeviceToDevice, s));
            hipLaunchKernelGGL(r1cs_transpose_rowptr_kernel, dim3(div_up(rows_t + 1, TR_BLOCK)), dim3(TR_BLOCK), 0, s, dk.current(), nnz, rt, rp_t);
            LURK_HIP_CHECK(hipGetLastError());
        }
        // the long rows, ascending
        uint32_t *cnt = (uint32_t*)counts.p, *offs = cnt + row_blocks + 1;
        const uint32_t *ra = dst.m[0].rowptr.as<uint32_t>(), *rb = dst.m[1].rowptr.as<uint32_t>(), *rc = dst.m[2].rowptr.as<uint32_t>();
        LURK_HIP_CHECK(hipMemsetAsync(cnt + row_blocks, 0, 4, s));
        hipLaunchKernelGGL(r1cs_transpose_long_count_kernel, dim3(row_blocks), dim3(TR_BLOCK), 0, s, ra, rb, rc, rt, cnt);
        LURK_HIP_CHECK(hipGetLastError());
        size_t bytes = temp_bytes;
        LURK_HIP_CHECK(rocprim::exclusive_scan(temp.p, bytes, cnt, offs, 0u, (size_t)row_blocks + 1, rocprim::plus<uint32_t>(), s));
        hipLaunchKernelGGL(r1cs_transpose_long_write_kernel, dim3(row_blocks), dim3(TR_BLOCK), 0, s, ra, rb, rc, rt, offs, dst.long_rows.as<uint32_t>());
        LURK_HIP_CHECK(hipGetLastError());
        uint32_t n_long = 0;
        LURK_HIP_CHECK(hipMemcpyAsync(&n_long, offs + row_blocks, 4, hipMemcpyDeviceToHost, s));
        LURK_HIP_CHECK(hipStreamSynchronize(s));  // the one synchronisation: the host keeps n_long
        if (n_long > long_cap) throw HipFailure{LURK_HIP_ERR_HIP, "r1cs transpose: more long rows than the entries allow"};
        dst.n_long = n_long;
        *out = h.release();
    });
}

int lurk_hip_r1cs_read(const lurk_hip_r1cs* shape, int which, uint64_t* indptr, uint64_t* indices, void* data32_mont) {
    return guarded([&] {
        LURK_REQUIRE(shape, "null shape");
        LURK_REQUIRE(which >= 0 && which <= 2, "unknown matrix id (0 = A, 1 = B, 2 = C)");
        const R1csShape& sh = shape->sh;
        const CsrDev& m = sh.m[which];
        LURK_REQUIRE(indptr, "null indptr");
        LURK_REQUIRE(m.nnz == 0 || indices, "null indices");
        LURK_REQUIRE(current_device() == sh.device, "the shape is resident on another device than the current one");
        LURK_HIP_CHECK(hipDeviceSynchronize());  // a shape may still be in the making on some stream
        std::vector<uint32_t> rp(sh.num_cons + 1);
        LURK_HIP_CHECK(hipMemcpy(rp.data(), m.rowptr.p, rp.size() * 4, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < rp.size(); i++) indptr[i] = rp[i];
        if (!m.nnz) return;
        std::vector<uint2> ent(m.nnz);
        LURK_HIP_CHECK(hipMemcpy(ent.data(), m.ent.p, m.nnz * 8, hipMemcpyDeviceToHost));
        for (size_t k = 0; k < m.nnz; k++) indices[k] = ent[k].x;
        if (!data32_mont) return;
        std::vector<uint32_t> words(sh.dict_size * P29_STRIDE);
        if (!words.empty()) LURK_HIP_CHECK(hipMemcpy(words.data(), sh.dict.p, words.size() * 4, hipMemcpyDeviceToHost));
        std::vector<uint64_t> values(sh.dict_size * 4);
        with_scalar_field(sh.field_id, [&](auto F) {
            for (size_t id = 0; id < sh.dict_size; id++) dict_value<decltype(F)>(words.data() + id * P29_STRIDE, values.data() + 4 * id);
        });
        char* out = (char*)data32_mont;  // no alignment promise
        for (size_t k = 0; k < m.nnz; k++) {
            if (ent[k].y >= sh.dict_size) throw HipFailure{LURK_HIP_ERR_HIP, "r1cs read: a coefficient id beyond the dictionary"};
            memcpy(out + 32 * k, values.data() + 4 * (size_t)ent[k].y, 32);
        }
    });
}

}  // extern "C"
