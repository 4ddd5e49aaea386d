// msm_finalize_bn254.hip - the finalize stage over the BN254 cycle's base fields (BN254 G1: Bn254Fq, Grumpkin: Bn254Fr).
// The templates are msm_finalize.hip's; only the instantiations differ, and they live in a translation unit of their own so that the
// Pasta code objects - and the register budgets tests/test_cabi_exports.py holds them to - do not change.
// Built scratch-free: the rare doubling branch inlined and room for two waves per SIMD instead of four - the kernels take 136-181
// registers and spill nothing, where the 128-register form of the Pasta units spills 336-560 bytes per lane.  The price: such a wave
// fits beside ONE resident accumulation of this cycle (184 + 184 <= 512), not beside two.
#ifndef LURK_F29_RARE_ATTR  // (a listing with the branch out of line prices the hot path alone: bench_tools/issue_model.py)
#define LURK_F29_RARE_ATTR
#endif
#define LURK_FINALIZE_WAVES 2
#define LURK_MSM_BN254_TU 1
#include "msm_finalize.hip"
