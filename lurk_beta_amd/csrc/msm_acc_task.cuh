// msm_acc_task.cuh - the body both forms of the bucket accumulation run per task (msm_acc.hip: the plain launch; msm_acc_persistent.hip:
// the persistent form).  One definition of the additions: both forms run the same sequence of mixed additions (xyzz29_madd_task) on the same arguments and
// give bit-identical task sums.  They differ in ONE compile-time choice, PIPELINED, which only moves loads: the persistent form
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
                                                    const uint32_t* __restrict__ task_dest, Plane29<P>* __restrict__ records) {
    uint32_t t = order[i];
    uint2 ti = task_info[t];
    // The task's sum leaves as it stands, a record on the radix-2^29 layer (no conversion to the 8 x 32 form: finalize and the bucket
    // reduction work on records), at the slot the plan chose: the bucket's own when the bucket is this one task.  What is stored is
    // R-bounded - tight limbs, value < 2^259, what msm_task_accumulate29_raw leaves (the signed loop normalises its sum once, at the end) - as xyzz29_add requires of its inputs
    // (plane_store asserts it under LURK_F29_CHECK).
    Xyzz29<P> acc;
    bool acc_id;
#if LURK_ACC_RADIX29
    msm_task_accumulate29_raw<P, PIPELINED>(sorted, ti.x, ti.y, table, acc, acc_id);
#else
    xyzz29_from_xyzz<P>(msm_task_accumulate<P>(sorted, ti.x, ti.y, table), acc, acc_id);  // (the 8 x 32-bit A/B build: the plain loop in both forms)
#endif
    plane_store<P>(records + task_dest[t], acc, acc_id);
}

}  // namespace lurk
