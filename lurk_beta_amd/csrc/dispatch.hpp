// dispatch.hpp - from the ids of the C ABI (lurk_hip.h) to the templated code behind it: field id -> field pack, curve id -> (base field
// pack, scalar field pack), canonical 32 bytes <-> Montgomery Fe<F>.  Nothing falls through to a default field or curve.
#pragma once
#include "common.hpp"
#include "field.cuh"

namespace lurk {

// field id -> f(field pack), over the three fields the provers are offered on
template <class Fn>
void with_field(int field_id, Fn&& f) {
    switch (field_id) {
        case LURK_FIELD_PALLAS_FP: f(PallasFp{}); return;
        case LURK_FIELD_PALLAS_FQ: f(PallasFq{}); return;
        case LURK_FIELD_BN254_FR: f(Bn254Fr{}); return;
    }
    LURK_REQUIRE(false, "unknown field id");
}

// field id -> f(field pack), over the scalar fields of all four curves: with_field's three and the BN254 base field (Grumpkin's scalar
// field).  For HOST helpers on the paths that are keyed by a resident shape or by a folding context (the shape's dictionary, the
// context's u and X): an entry point that takes a field id as an argument goes through with_field and keeps refusing the fourth id.
// No kernel may be instantiated through this: the kernels over Bn254Fq live in fold_bn254fq.hip / r1cs_sat_bn254fq.hip and are reached
// through the ordinary functions of r1cs_bn254fq.hpp.
template <class Fn>
void with_scalar_field(int field_id, Fn&& f) {
    if (field_id == LURK_FIELD_BN254_FQ) {
        f(Bn254Fq{});
        return;
    }
    with_field(field_id, f);
}
// curve id -> the id of its scalar field
inline int curve_scalar_field_id(int curve) {
    switch (curve) {
        case LURK_CURVE_PALLAS: return LURK_FIELD_PALLAS_FQ;
        case LURK_CURVE_VESTA: return LURK_FIELD_PALLAS_FP;
        case LURK_CURVE_BN254: return LURK_FIELD_BN254_FR;
        case LURK_CURVE_GRUMPKIN: return LURK_FIELD_BN254_FQ;
    }
    LURK_REQUIRE(false, "unknown curve id");
    return -1;
}
inline const char* field_name(int field_id) {
    switch (field_id) {
        case LURK_FIELD_PALLAS_FP: return "the Pallas base field";
        case LURK_FIELD_PALLAS_FQ: return "the Pallas scalar field";
        case LURK_FIELD_BN254_FR: return "the BN254 scalar field";
        case LURK_FIELD_BN254_FQ: return "the BN254 base field";
    }
    return "an unknown field";
}

// curve id -> f(base field pack, scalar field pack).  Every entry point that takes a curve id goes through this (or refuses the
// id by name).  The MSM kernels of the BN254 cycle are instantiated in msm_*_bn254.hip only.
template <class Fn>
void with_curve(int curve, Fn&& f) {
    switch (curve) {
        case LURK_CURVE_PALLAS: f(PallasFp{}, PallasFq{}); return;
        case LURK_CURVE_VESTA: f(PallasFq{}, PallasFp{}); return;
        case LURK_CURVE_BN254: f(Bn254Fq{}, Bn254Fr{}); return;
        case LURK_CURVE_GRUMPKIN: f(Bn254Fr{}, Bn254Fq{}); return;
    }
    LURK_REQUIRE(false, "unknown curve id");
}
// the same for code that exists on the Pasta cycle only; its entry points refuse the other ids first (require_pasta_curve)
template <class Fn>
void with_pasta_curve(int curve, Fn&& f) {
    switch (curve) {
        case LURK_CURVE_PALLAS: f(PallasFp{}, PallasFq{}); return;
        case LURK_CURVE_VESTA: f(PallasFq{}, PallasFp{}); return;
    }
    require_pasta_curve(curve, "this entry point");
}

// canonical 32 bytes (no alignment promise) -> Montgomery, refusing a value that is not reduced; and back
template <class F>
Fe<F> fe_read_canonical(const void* p32, const char* what = "a field element") {
    Fe<F> v;
    memcpy(v.l, p32, 32);
    if (fe_canonical_ge_mod<F>(v.l)) throw HipFailure{LURK_HIP_ERR_INVALID_ARG, std::string(what) + " is not reduced modulo the field order"};
    return fe_to_mont<F>(v);
}
template <class F>
void fe_write_canonical(void* out32, const Fe<F>& mont) {
    const Fe<F> c = fe_from_mont<F>(mont);
    memcpy(out32, c.l, 32);
}

}  // namespace lurk
