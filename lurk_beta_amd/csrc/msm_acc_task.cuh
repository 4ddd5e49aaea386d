// msm_acc_task.cuh - the body both forms of the bucket accumulation run per task (msm_acc.hip: the plain launch; msm_acc_persistent.hip:
// the persistent form).  One definition of the additions: both forms run the same sequence of xyzz29_madd calls on the same arguments and
// give bit-identical partial sums.  They differ in ONE compile-time choice, PIPELINED, which only moves loads: the persistent form
// launched with one wave per SIMD (nothing to cover a wait) gathers the next table record under the current addition; the plain launch
// (three waves per SIMD, no registers to spare) and the persistent form at two or more waves per SIMD do not - see
// msm_task_accumulate29_raw in curve29.cuh.  The two translation units may also be built with different flags (Makefile: ACC_FLAGS /
// PERSIST_FLAGS).
#pragma once
#include "msm_core.cuh"
#include "curve29.cuh"
#include "msm_stages.hpp"

namespace lurk {

#ifndef LURK_ACC_TASK_NOINLINE
#define LURK_ACC_TASK_NOINLINE 0
#endif
#if LURK_ACC_TASK_NOINLINE
#define LURK_ACC_TASK_ATTR __attribute__((noinline))
#else
#define LURK_ACC_TASK_ATTR __forceinline__
#endif
template <class P, bool PIPELINED = false>
__device__ LURK_ACC_TASK_ATTR void msm_accumulate_task(uint32_t i, const uint32_t* __restrict__ sorted, const Affine<P>* __restrict__ table,
                                                    const uint2* __restrict__ task_info, const uint32_t* __restrict__ order,
                                                    Xyzz<P>* __restrict__ partials) {
    uint32_t t = order[i];
    uint2 ti = task_info[t];
#if LURK_ACC_RADIX29
    partials[t] = msm_task_accumulate29<P, PIPELINED>(sorted, ti.x, ti.y, table);
#else
    partials[t] = msm_task_accumulate<P>(sorted, ti.x, ti.y, table);  // (the 8 x 32-bit A/B build: the plain loop in both forms)
#endif
}

}  // namespace lurk
