// msm_precompute_bn254.hip - the window-table build over the BN254 cycle's base fields (BN254 G1: Bn254Fq, Grumpkin: Bn254Fr).
// The templates are msm_precompute.hip's; only the instantiations differ, and they live in a translation unit of their own so that the
// Pasta code objects - and the register budgets tests/test_cabi_exports.py holds them to - do not change.
#define LURK_MSM_BN254_TU 1
#include "msm_precompute.hip"
