// r1cs_bn254fq.hpp - the row and fold kernels over the BN254 base field (Bn254Fq: Grumpkin's scalar field), as ordinary functions.
//
// The templates are fold.hip's and r1cs_sat.hip's; their instantiations over Bn254Fq live in fold_bn254fq.hip and r1cs_sat_bn254fq.hip,
// translation units of their own (the pattern of msm_acc_bn254.hip), so that the code objects of fold.hip and r1cs_sat.hip - and the
// register budgets tests/test_r1cs_row_resources.py holds their kernels to - do not change.  fold.hip, r1cs_sat.hip and step.hip reach
// them through these declarations only: naming a launcher TEMPLATE over Bn254Fq there (a dispatch lambda does) would instantiate the
// kernel in that unit.  Arguments as the templates of the same name take them.
//
// fold_vecs_scalar_field / fold_vec_scalar_field: the bodies of lurk_hip_fold_vecs_dev / lurk_hip_fold_vec_dev over the scalar fields
// of all four curves.  The public calls refuse field id 3 before they get here; a folding context (step.hip), whose field comes from
// its curve and its shape, calls them directly.
#pragma once
#include "common.hpp"

namespace lurk {

struct R1csShape;

void multiply_vec_bn254fq(const R1csShape& sh, const void* d_z, void* az, void* bz, void* cz, hipStream_t s);
void cross_term_bn254fq(const R1csShape& sh, const void* d_z1, const void* d_z2, void* d_t, hipStream_t s);
void cross_term_cached_bn254fq(const R1csShape& sh, const void* d_z2, void* az1, void* bz1, void* cz1, const void* u1_32, const void* prev_a, const void* prev_b,
                               const void* prev_c, const void* r_prev32, void* d_t, void* az2, void* bz2, void* cz2, hipStream_t s);
void fold_vecs_bn254fq(int count, const void* const* a, const void* const* b, const size_t* n, void* const* out, const void* r32, hipStream_t s);
void fold_vec_bn254fq(const void* a, const void* b, const void* r32, size_t n, void* out, hipStream_t s);
void is_sat_bn254fq(const R1csShape& sh, const void* d_z, const void* d_e, uint64_t* n_unsat, uint64_t* first_unsat, hipStream_t s);

void fold_vecs_scalar_field(int field_id, int count, const void* const* d_a, const void* const* d_b, const size_t* n, void* const* d_out, const void* r32_mont,
                            hipStream_t s);
void fold_vec_scalar_field(int field_id, const void* d_a, const void* d_b, const void* r32_mont, size_t n, void* d_out, hipStream_t s);

}  // namespace lurk
