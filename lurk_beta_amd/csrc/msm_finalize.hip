// msm_finalize.hip - stage 5 of the Pippenger pipeline (msm_core.cuh; launched by MsmCtx::enqueue, msm.hip): the task sums of a bucket
// become the bucket, on the slot's record array (msm_stages.hpp: buckets at [0, NB), the sums of the tasks of multi-task buckets behind).
//
// Everything here stays on the radix-2^29 layer: the accumulation stored Plane29 records, the bucket reduction reads them.  Per bucket:
//   0 tasks                 the identity record is written;
//   1 task                  nothing - the accumulation stored that task's sum straight into the bucket's slot (task_dest, msm_plan.hip);
//   2 .. MSM_FIN_SMALL      one lane sums the task records (plane_sum: a chain of xyzz29_add);
//   more                    the bucket goes on a list, a workgroup sums it (msm_big_bucket_kernel, launched behind this one).
// A lane's additions are DEPENDENT, so what the stage costs is nt - 1 times the latency of one general addition on a lane (6.4 us on
// this layer, ~20 us through the 8 x 32 group law).  It matters where a commitment is short: the opening argument's rounds under its
// folded 65 536-point key (8-entry tasks, 2-5 task sums per bucket) spent 69 us of their 420 here.
//
// Both kernels are held to the register budget of a tail wave beside two resident accumulations (128 + 2 x 192 = 512:
// __launch_bounds__(256, LURK_FINALIZE_WAVES)).  The hot-bucket kernel is launched for every commitment, with an empty list for uniform
// scalars: at 133 registers (its 8 x 32 form) that empty launch could not be placed beside two accumulations and waited for one to end.
#include "common.hpp"
#include "msm_core.cuh"
#include "curve29.cuh"
#include "msm_stages.hpp"

namespace lurk {

#ifndef LURK_FINALIZE_WAVES  // waves per SIMD the compiler is to leave room for (4 -> 128 VGPRs, 2 -> 256): msm_finalize_bn254.hip sets 2
#define LURK_FINALIZE_WAVES 4
#endif
#define LURK_FINALIZE_BOUNDS __launch_bounds__(256, LURK_FINALIZE_WAVES)
template <class P>
__global__ LURK_FINALIZE_BOUNDS void msm_finalize_kernel(Plane29<P>* records, const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ task_start,
                                                             const uint32_t* __restrict__ group_task_base, uint32_t NB, uint32_t* __restrict__ big_list,
                                                             uint32_t* __restrict__ big_count, uint32_t S) {
    __builtin_amdgcn_s_setprio(3);  // a latency-bound tail kernel: issue ahead of an accumulation sharing the SIMD
    const size_t key = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (key >= NB) return;
    const uint32_t nt = (cnt[key] + S - 1) / S;
    uint32_t first = 0;  // (only a bucket that is summed here needs it)
    if (nt >= 2 && nt <= MSM_FIN_SMALL) {
        const uint32_t g = (uint32_t)(key / MSM_GRP), b = (uint32_t)(key % MSM_GRP);
        first = group_task_base[g] + task_start[(size_t)g * (MSM_GRP + 1) + b];
    }
    if (plane_finalize_bucket<P>(records, NB, key, nt, first, MSM_FIN_SMALL)) big_list[atomicAdd(big_count, 1u)] = (uint32_t)key;
}

// ---- the hot buckets (more than MSM_FIN_SMALL task sums): one workgroup each, lanes stride the task records, then a tree through LDS
template <class P>
__global__ LURK_FINALIZE_BOUNDS void msm_big_bucket_kernel(Plane29<P>* records, const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ task_start,
                                                               const uint32_t* __restrict__ group_task_base, uint32_t NB,
                                                               const uint32_t* __restrict__ big_list, const uint32_t* __restrict__ big_count, uint32_t S) {
    __builtin_amdgcn_s_setprio(3);
    extern __shared__ uint4 lds_raw[];
    Plane29<P>* sh = reinterpret_cast<Plane29<P>*>(lds_raw);
    const uint32_t nbig = *big_count;
    for (uint32_t i = blockIdx.x; i < nbig; i += gridDim.x) {
        const uint32_t key = big_list[i];
        const uint32_t g = key / MSM_GRP, b = key % MSM_GRP;
        const uint32_t nt = (cnt[key] + S - 1) / S;
        const Plane29<P>* tasks = records + NB + (group_task_base[g] + task_start[(size_t)g * (MSM_GRP + 1) + b]);
        Xyzz29<P> acc, q;
        acc.x = acc.y = acc.zz = acc.zzz = f29_zero<P>();
        bool acc_id = true, q_id;
        for (uint32_t j = threadIdx.x; j < nt; j += 256) {
            plane_load<P>(tasks + j, q, q_id);
            xyzz29_add<P>(acc, acc_id, q, q_id);
        }
        block_tree_sum29<P, 256>(acc, acc_id, sh);
        if (threadIdx.x == 0) plane_store<P>(records + key, acc, acc_id);
        __syncthreads();
    }
}

template <class P>
void msm_launch_finalize(Plane29<P>* records, const uint32_t* cnt, const uint32_t* task_start, const uint32_t* group_task_base, uint32_t NB,
                         uint32_t* big_list, uint32_t* big_count, uint32_t S, hipStream_t s) {
    static_assert(sizeof(Plane29<P>) == MSM_RECORD_BYTES, "the slot's record array is sized by MSM_RECORD_BYTES");
    hipLaunchKernelGGL((msm_finalize_kernel<P>), dim3(div_up((size_t)NB, 256)), dim3(256), 0, s, records, cnt, task_start, group_task_base, NB, big_list, big_count,
                       S);
}
template <class P>
void msm_launch_big_buckets(Plane29<P>* records, const uint32_t* cnt, const uint32_t* task_start, const uint32_t* group_task_base, uint32_t NB,
                            const uint32_t* big_list, const uint32_t* big_count, uint32_t S, hipStream_t s) {
    hipLaunchKernelGGL((msm_big_bucket_kernel<P>), dim3(128), dim3(256), 256 * sizeof(Plane29<P>), s, records, cnt, task_start, group_task_base, NB, big_list,
                       big_count, S);
}
#define LURK_FINALIZE_INSTANTIATE(P)                                                                                                                      \
    template void msm_launch_finalize<P>(Plane29<P>*, const uint32_t*, const uint32_t*, const uint32_t*, uint32_t, uint32_t*, uint32_t*, uint32_t, hipStream_t); \
    template void msm_launch_big_buckets<P>(Plane29<P>*, const uint32_t*, const uint32_t*, const uint32_t*, uint32_t, const uint32_t*, const uint32_t*, uint32_t, \
                                            hipStream_t);
#ifdef LURK_MSM_BN254_TU  // msm_finalize_bn254.hip
LURK_FINALIZE_INSTANTIATE(Bn254Fq)
LURK_FINALIZE_INSTANTIATE(Bn254Fr)
#else
LURK_FINALIZE_INSTANTIATE(PallasFp)
LURK_FINALIZE_INSTANTIATE(PallasFq)
#endif

}  // namespace lurk
