// msm_acc_persistent_bn254.hip - the persistent bucket accumulation over the BN254 cycle's base fields (BN254 G1: Bn254Fq, Grumpkin: Bn254Fr).
// The templates are msm_acc_persistent.hip's; only the instantiations differ, and they live in a translation unit of their own so that the
// Pasta code objects - and the register budgets tests/test_cabi_exports.py holds them to - do not change.
// Built scratch-free: the two rare doubling branches of curve29.cuh are inlined here (out of line they cost the kernel a 192-byte
// stack frame per lane), which also takes the accumulate kernels from 163 / 187 registers to 154 / 178.
#ifndef LURK_F29_RARE_ATTR  // (a listing with the branch out of line prices the hot path alone: bench_tools/issue_model.py)
#define LURK_F29_RARE_ATTR
#endif
#define LURK_MSM_BN254_TU 1
#include "msm_acc_persistent.hip"
