// msm_sort_bn254.hip - the sort of a commitment whose scalars are over a BN254-cycle field (BN254 G1: Bn254Fr, Grumpkin: Bn254Fq).
//
// The recoding and both sort passes work on canonical 256-bit integers and do not know the modulus (msm_core.cuh: the scalars are
// below 2^254, W c >= 256 for every window width, so the top window never carries out - the argument made there for 255-bit scalars
// holds with a bit to spare).  Only the Montgomery -> canonical step does: it is one kernel here, in a translation unit of its own,
// and the sort proper is msm_sort.hip's, unchanged - its kernel set and register budgets (tests/test_cabi_exports.py) stay what they
// were.  Cost against the fused form of the Pasta fields: one more 32-byte read and write per scalar that arrives in Montgomery form.
#include "msm_sort.hpp"

#include "common.hpp"
#include "msm_core.cuh"

namespace lurk {

template <class SF>
__global__ __launch_bounds__(256) void msm_canon_kernel(const uint4* __restrict__ scalars, uint4* __restrict__ canon, size_t n, int low) {
    if (low) __builtin_amdgcn_s_setprio(0);  // a short kernel beside resident accumulations: see msm_sort.hip
    else __builtin_amdgcn_s_setprio(3);
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint4 lo = scalars[2 * i], hi = scalars[2 * i + 1];
    Fe<SF> s;
    s.l[0] = lo.x; s.l[1] = lo.y; s.l[2] = lo.z; s.l[3] = lo.w;
    s.l[4] = hi.x; s.l[5] = hi.y; s.l[6] = hi.z; s.l[7] = hi.w;
    s = fe_from_mont<SF>(s);
    canon[2 * i] = make_uint4(s.l[0], s.l[1], s.l[2], s.l[3]);
    canon[2 * i + 1] = make_uint4(s.l[4], s.l[5], s.l[6], s.l[7]);
}

template <class SF>
static void sort_bn254(const MsmShape& sh, const void* d_scalars, int is_mont, const MsmSortBufs& b, hipStream_t s) {
    if (is_mont) {
        hipLaunchKernelGGL((msm_canon_kernel<SF>), dim3(div_up(sh.n, 256)), dim3(256), 0, s, (const uint4*)d_scalars, (uint4*)b.canon, sh.n, sh.low_prio);
        d_scalars = b.canon;
    }
    msm_launch_sort_canonical(sh, d_scalars, b, s);
}
template <>
void msm_launch_sort<Bn254Fr>(const MsmShape& sh, const void* d_scalars, int is_mont, const MsmSortBufs& b, hipStream_t s) {
    sort_bn254<Bn254Fr>(sh, d_scalars, is_mont, b, s);
}
template <>
void msm_launch_sort<Bn254Fq>(const MsmShape& sh, const void* d_scalars, int is_mont, const MsmSortBufs& b, hipStream_t s) {
    sort_bn254<Bn254Fq>(sh, d_scalars, is_mont, b, s);
}

}  // namespace lurk
