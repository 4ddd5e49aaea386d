// point_host.hip - the group law on the host over a handful of points: what sums the partial commitments of a multi-device key or of the
// ranks of a distributed prover, and the few [k] P of a folding step.
#include "common.hpp"
#include "dispatch.hpp"
#include "msm_core.cuh"

namespace lurk {

template <class P>
static void point_sum_host(const void* pts, size_t count, void* out) {
    // the caller's buffers carry no alignment promise (Fe<P> is 16-byte aligned): go through memcpy
    Xyzz<P> acc = xyzz_identity<P>();
    for (size_t i = 0; i < count; i++) {
        Jacobian<P> j;
        memcpy(&j, (const char*)pts + i * sizeof(Jacobian<P>), sizeof(j));
        xyzz_add<P>(acc, xyzz_from_jacobian<P>(j));
    }
    const Jacobian<P> r = jacobian_from_affine<P>(xyzz_to_affine<P>(acc));
    memcpy(out, &r, sizeof(r));
}
template <class P>
static void point_affine_canonical_host(const void* pt, void* out) {
    Jacobian<P> j;
    memcpy(&j, pt, sizeof(j));
    // every commitment this library hands out is normalised (Z = the Montgomery one): then (X, Y) ARE the affine coordinates and the field
    // inversion (~17 us on a host core: a quarter of the transcript's time when four commitments are absorbed) is skipped
    const Fe<P> one = fe_one<P>();
    bool z_is_one = true;
    for (int i = 0; i < 8; i++) z_is_one = z_is_one && j.z.l[i] == one.l[i];
    Affine<P> a = z_is_one ? Affine<P>{j.x, j.y} : xyzz_to_affine<P>(xyzz_from_jacobian<P>(j));
    Fe<P> x = fe_from_mont<P>(a.x), y = fe_from_mont<P>(a.y);
    memcpy(out, x.l, 32);
    memcpy((char*)out + 32, y.l, 32);
}

// [k] P on the host (double-and-add over the canonical scalar, top bit first): a handful per folding step
template <class P, class SF>
static void point_mul_host(const void* pt, const void* scalar32, int is_mont, void* out) {
    Fe<SF> k;
    memcpy(k.l, scalar32, 32);
    if (is_mont) k = fe_from_mont<SF>(k);
    Jacobian<P> j;
    memcpy(&j, pt, sizeof(j));
    const Xyzz<P> base = xyzz_from_jacobian<P>(j);
    Xyzz<P> acc = xyzz_identity<P>();
    int top = 255;  // Nova's folding challenges are 128 bits (NUM_CHALLENGE_BITS): start at the highest set bit
    while (top >= 0 && !((k.l[top >> 5] >> (top & 31)) & 1u)) top--;
    for (int i = top; i >= 0; i--) {
        acc = xyzz_dbl<P>(acc);
        if ((k.l[i >> 5] >> (i & 31)) & 1u) xyzz_add<P>(acc, base);
    }
    const Jacobian<P> r = jacobian_from_affine<P>(xyzz_to_affine<P>(acc));
    memcpy(out, &r, sizeof(r));
}


}  // namespace lurk

using namespace lurk;

extern "C" {

// host-side group helpers (a handful of points: partial commitments gathered from the ranks)
int lurk_hip_point_sum_gathered(int curve, void* out, const void* gathered, size_t world) {
    if (world == 0) {
        set_error(LURK_HIP_ERR_INVALID_ARG, "lurk_hip_point_sum_gathered: a world of 0 ranks");
        return LURK_HIP_ERR_INVALID_ARG;
    }
    return lurk_hip_point_sum(curve, out, gathered, world);
}

int lurk_hip_point_sum(int curve, void* out, const void* points, size_t count) {
    return host_guarded([&] {
        LURK_REQUIRE(curve >= LURK_CURVE_PALLAS && curve <= LURK_CURVE_GRUMPKIN, "unknown curve id");
        LURK_REQUIRE(out && (count == 0 || points), "null argument");
        with_curve(curve, [&](auto P, auto) { point_sum_host<decltype(P)>(points, count, out); });
    });
}
int lurk_hip_point_mul(int curve, void* out, const void* point, const void* scalar32, int is_mont) {
    return host_guarded([&] {
        LURK_REQUIRE(curve >= LURK_CURVE_PALLAS && curve <= LURK_CURVE_GRUMPKIN, "unknown curve id");
        LURK_REQUIRE(out && point && scalar32, "null argument");
        with_curve(curve, [&](auto P, auto SF) { point_mul_host<decltype(P), decltype(SF)>(point, scalar32, is_mont, out); });
    });
}
int lurk_hip_point_to_affine_canonical(int curve, void* out_xy64, const void* point) {
    return host_guarded([&] {
        LURK_REQUIRE(curve >= LURK_CURVE_PALLAS && curve <= LURK_CURVE_GRUMPKIN, "unknown curve id");
        LURK_REQUIRE(out_xy64 && point, "null argument");
        with_curve(curve, [&](auto P, auto) { point_affine_canonical_host<decltype(P)>(point, out_xy64); });
    });
}
}
