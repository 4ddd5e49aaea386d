// msm_acc_persistent.hip - the persistent form of the bucket accumulation (commitments in flight; round 6: the accumulation of a
// LURK_MSM_SUBMIT_FOLLOW commitment), in its own translation unit so that it CAN be built for another register footprint than the
// plain launch of msm_acc.hip (Makefile: PERSIST_FLAGS / PERSIST_DEFS).  The SHIPPED build sets neither.  The kernel runs the same
// additions as the plain launch (msm_acc_task.cuh); launched with one wave per SIMD it runs them through the PIPELINED task loop of
// curve29.cuh, which keeps the next table record (16 registers) and the index after it in flight under the current addition: 173 VGPRs
// where the plain loop takes 162 (Pasta).  192 is the
// budget: what has to run beside resident accumulations is sized for it and checked on the compiler's own numbers
// (tests/test_cabi_exports.py::test_sort_kernels_fit_beside_a_resident_accumulation, tests/test_acc_pipeline_resources.py): four waves
// of a 1024-thread sort workgroup beside ONE 192-register wave (4 x 72 + 192 <= 512), a 128-register tail wave beside TWO
// (128 + 2 x 192 = 512).  One granule more and the second launch waits for the tail kernels.  (A 144-register build of the plain loop -
// machine LICM off - lets the 56-register sort passes sit beside two; measured in round 4, +1.7 % in flight, -4 % for the folding step: not shipped.)
#ifndef LURK_ACC_RADIX29
#define LURK_ACC_RADIX29 1
#endif
#if !LURK_ACC_RADIX29
#define LURK_MUL_FORCE_INLINE
#endif
#include "common.hpp"
#include "msm_acc_task.cuh"

namespace lurk {

// (XCC, SE, CU) of the running wave as one index < 512 (HW_ID: CU_ID [11:8], SE_ID [14:13]; XCC_ID [3:0])
__device__ __forceinline__ uint32_t msm_cu_index() {
    const uint32_t hw = __builtin_amdgcn_s_getreg((4 /*HW_ID*/) | (0 << 6) | (31 << 11));
    const uint32_t xcc = __builtin_amdgcn_s_getreg((20 /*XCC_ID*/) | (0 << 6) | (3 << 11));
    return (xcc & 7u) * 64u + ((hw >> 13) & 3u) * 16u + ((hw >> 8) & 15u);
}

// Persistent form for commitments in flight: a fixed number of waves per SIMD (the launch grid), each wave pulls the next
// 64 tasks of the longest-first order from a global cursor.  The kernel then never holds more than its share of every
// SIMD's registers and wave slots, so the latency / HBM-bound kernels of the NEXT commitment (sort, plan, bucket
// reduction: other stream, higher priority) find room on every CU while this one keeps the integer VALU busy.
// PIPELINED: the task loop that gathers the next table record under the current addition (curve29.cuh) - the launch with ONE wave per
// SIMD, whose loads nothing else covers.  A launch with two or more waves per SIMD (a LURK_MSM_SUBMIT_FOLLOW commitment,
// LURK_MSM_PERSIST_WGS) keeps the plain loop at 176 registers: its waves cover each other, and what a folding step runs beside a
// two-wave accumulation needs the 160 registers that 2 x 176 leave, not the 128 of 2 x 192 (measured: the rc = 100 step 2.95-2.99 ->
// 3.12-3.19 ms with the pipelined loop in the FOLLOW class; profiles/r13_acc_pipeline_bench.json).
template <class P, bool PIPELINED>
#ifndef LURK_PERSIST_MIN_BLOCKS
#define LURK_PERSIST_MIN_BLOCKS 1  // (HIP: minimum WAVES per SIMD) 4: the compiler holds the kernel to 128 registers (and spills the rest)
#endif
// The register budget is handed to the compiler as well.  It bound the pipelined instantiations while a task ended in a conversion to
// the 8 x 32 form (xyzz29_to_xyzz: ~23 constants parked in VGPRs across the whole task loop, 192 / 190 registers); now that a task
// stores its sum as it stands - a Plane29 record, msm_acc_task.cuh - the kernels sit below it: 173 (Pasta) / 167 (BN254) pipelined,
// 162 / 161 with the plain loop, scratch as before (192 bytes per lane on the Pasta fields, the frame of the out-of-line doubling; none
// on the BN254 fields).  The limit stays as the statement of the budget.  amdgpu_num_vgpr counts registers of the UNIFIED file
// of gfx90a and later in halves (the backend doubles the number: AMDGPUSubtarget::getMaxNumVGPRs), so 96 here is a limit of 192;
// tests/test_acc_pipeline_resources.py fails if a compiler ever reads it another way (the kernel would spill).
#define LURK_PERSIST_VGPR_BUDGET 192
__global__ __launch_bounds__(MSM_ACC_BLOCK, LURK_PERSIST_MIN_BLOCKS) __attribute__((amdgpu_num_vgpr(LURK_PERSIST_VGPR_BUDGET / 2))) void msm_accumulate_persistent_kernel(const uint32_t* __restrict__ sorted, const Affine<P>* __restrict__ table,
                                                                                    const uint2* __restrict__ task_info,
                                                                                    const uint32_t* __restrict__ order,
                                                                                    const uint32_t* __restrict__ task_dest,
                                                                                    const uint32_t* __restrict__ group_task_base, int NG,
                                                                                    Plane29<P>* __restrict__ records, uint32_t* __restrict__ cursor) {
    const uint32_t ntasks = group_task_base[NG];
    const uint32_t lane = threadIdx.x & 63u;
    if (threadIdx.x == 0) atomicAdd(&cursor[MSM_PLACEMENT_BASE + msm_cu_index()], 1u);  // diagnostic: workgroups per CU
    for (;;) {
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(cursor, 64u);
        base = __builtin_amdgcn_readfirstlane(base);  // wave-uniform: the loop control stays scalar
        if (base >= ntasks) break;
        if (base + lane < ntasks) msm_accumulate_task<P, PIPELINED>(base + lane, sorted, table, task_info, order, task_dest, records);
    }
}

// one workgroup of 4 waves per CU (one wave per SIMD); cursor must be zero when the kernel starts
template <class P>
void msm_launch_accumulate_persistent(const uint32_t* sorted, const Affine<P>* table, const uint2* task_info, const uint32_t* order, const uint32_t* task_dest,
                                      const uint32_t* group_task_base, int NG, Plane29<P>* records, uint32_t* cursor, hipStream_t s, unsigned wgs_per_cu) {
    // LURK_MSM_PERSIST_WGS workgroups per CU (1: one wave per SIMD, the form two of which are resident at once; 2: two waves per SIMD - a
    // single accumulation at the multiplier's full rate, for LURK_MSM_MAX_ACC=1)
    static const unsigned wgs = [] { const char* e = getenv("LURK_MSM_PERSIST_WGS"); int v = e ? atoi(e) : 1; return (unsigned)(v < 1 ? 1 : v > 4 ? 4 : v); }();
    // wgs_per_cu != 0: the caller's choice for this launch (a LURK_MSM_SUBMIT_FOLLOW commitment: the PERSISTENT_SLOT_STREAM form of msm_launch_plan.hpp)
    const unsigned waves = wgs_per_cu ? wgs_per_cu : wgs;  // per SIMD
    if (waves == 1)
        hipLaunchKernelGGL((msm_accumulate_persistent_kernel<P, true>), dim3((unsigned)num_cus()), dim3(MSM_ACC_BLOCK), 0, s, sorted, table, task_info, order,
                           task_dest, group_task_base, NG, records, cursor);
    else
        hipLaunchKernelGGL((msm_accumulate_persistent_kernel<P, false>), dim3((unsigned)num_cus() * waves), dim3(MSM_ACC_BLOCK), 0, s, sorted, table, task_info, order,
                           task_dest, group_task_base, NG, records, cursor);
}
#define LURK_ACC_PERSISTENT_INSTANTIATE(P)                                                                                                    \
    template void msm_launch_accumulate_persistent<P>(const uint32_t*, const Affine<P>*, const uint2*, const uint32_t*, const uint32_t*, const uint32_t*, int, \
                                                      Plane29<P>*, uint32_t*, hipStream_t, unsigned);
#ifdef LURK_MSM_BN254_TU  // msm_acc_persistent_bn254.hip
LURK_ACC_PERSISTENT_INSTANTIATE(Bn254Fq)
LURK_ACC_PERSISTENT_INSTANTIATE(Bn254Fr)
#else
LURK_ACC_PERSISTENT_INSTANTIATE(PallasFp)
LURK_ACC_PERSISTENT_INSTANTIATE(PallasFq)
#endif

}  // namespace lurk
