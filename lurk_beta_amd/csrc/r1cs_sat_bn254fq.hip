// r1cs_sat_bn254fq.hip - the satisfiability check over the BN254 base field (Bn254Fq: Grumpkin's scalar field): r1cs_sat.hip's templates,
// instantiated in a translation unit of their own so that r1cs_sat.hip's code object does not change (see fold_bn254fq.hip).
// Defines is_sat_bn254fq of r1cs_bn254fq.hpp.
#define LURK_SAT_BN254FQ_TU 1
#include "r1cs_sat.hip"
