// msm_acc.hip - the dominant kernel of the MSM (bucket accumulation), in its own translation unit.
// The accumulator lives on the radix-2^29 layer (curve29.cuh: products without carry folds, lazy
// reduction); LURK_ACC_RADIX29=0 builds the 8 x 32-bit Montgomery version with the multiplier inlined
// (kept for A/B measurements).
#ifndef LURK_ACC_RADIX29
#define LURK_ACC_RADIX29 1
#endif
#if !LURK_ACC_RADIX29
#define LURK_MUL_FORCE_INLINE
#endif
#include "common.hpp"
#include "msm_acc_task.cuh"

namespace lurk {

// One launch covers every task (the hardware dispatcher balances the workgroups).
template <class P>
__global__ __launch_bounds__(MSM_ACC_BLOCK) void msm_accumulate_kernel(const uint32_t* __restrict__ sorted, const Affine<P>* __restrict__ table,
                                                                         const uint2* __restrict__ task_info, const uint32_t* __restrict__ order,
                                                                         const uint32_t* __restrict__ task_dest,
                                                                         const uint32_t* __restrict__ group_task_base, int NG,
                                                                         Plane29<P>* __restrict__ records) {
#if !defined(LURK_ACC_NO_SETPRIO)
    __builtin_amdgcn_s_setprio(1);  // above a persistent (background) accumulation sharing the SIMD, below every short kernel (3)
#endif
    uint32_t i = blockIdx.x * MSM_ACC_BLOCK + threadIdx.x;
    if (i >= group_task_base[NG]) return;
    msm_accumulate_task<P>(i, sorted, table, task_info, order, task_dest, records);
}

template <class P>
void msm_launch_accumulate(const uint32_t* sorted, const Affine<P>* table, const uint2* task_info, const uint32_t* order, const uint32_t* task_dest,
                           const uint32_t* group_task_base, int NG, Plane29<P>* records, size_t nt, hipStream_t s) {
    hipLaunchKernelGGL((msm_accumulate_kernel<P>), dim3(div_up(nt, MSM_ACC_BLOCK)), dim3(MSM_ACC_BLOCK), 0, s, sorted, table, task_info, order, task_dest,
                       group_task_base, NG, records);
}
#define LURK_ACC_INSTANTIATE(P)                                                                                                                  \
    template void msm_launch_accumulate<P>(const uint32_t*, const Affine<P>*, const uint2*, const uint32_t*, const uint32_t*, const uint32_t*, int, \
                                           Plane29<P>*, size_t, hipStream_t);
#ifdef LURK_MSM_BN254_TU  // msm_acc_bn254.hip: the BN254 / Grumpkin base fields, a code object of their own
LURK_ACC_INSTANTIATE(Bn254Fq)
LURK_ACC_INSTANTIATE(Bn254Fr)
#else
LURK_ACC_INSTANTIATE(PallasFp)
LURK_ACC_INSTANTIATE(PallasFq)
#endif

}  // namespace lurk
