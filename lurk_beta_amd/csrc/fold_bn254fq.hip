// fold_bn254fq.hip - multiply_vec, the two cross terms and the folds over the BN254 base field (Bn254Fq: Grumpkin's scalar field), for
// shapes made by lurk_hip_r1cs_create_for_curve(LURK_CURVE_GRUMPKIN) and the folding context on Grumpkin (step.hip).
// The templates are fold.hip's, where the lazy-accumulation bounds are re-derived for this modulus; only the instantiations differ, and
// they live in a translation unit of their own so that fold.hip's code object - and the register budgets
// tests/test_r1cs_row_resources.py holds it to - does not change.  Defines the *_bn254fq functions of r1cs_bn254fq.hpp.
#define LURK_FOLD_BN254FQ_TU 1
#include "fold.hip"
