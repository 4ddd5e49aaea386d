// poseidon_trace.cuh - the slot-witness trace kernels, shared by the translation units that write a traced hash block into W: poseidon.hip
// (a block = one slot of a MultiFrame, placed by TraceDst) and trie_circuit.hip (a block = one level of a trie proof inside a coprocessor
// circuit, placed by its own destination type).  The kernels are templates over the destination, which says
//   base(i)                 where hash i's block starts in W
//   preimage(pre, i, A)     where hash i's preimage is (A elements of 32 B)
//   beside_wide / _lane     what else the hash's lanes write next to the block (nothing for a slot; the picks of a trie level)
// so that one kernel text serves both.  bit_decomp_trace_block is the workgroup-per-value body of the bit-decomposition trace.
#pragma once
#include "poseidon.cuh"
#include "poseidon29.cuh"

namespace lurk {

constexpr int POSEIDON_BLOCK = 256;
constexpr int POSEIDON_WIDE_BLOCK = 256;
constexpr size_t POSEIDON_WIDE_MAX = 8192;  // batches up to this size run one state across T lanes (latency), larger ones one per lane
enum : int { PF_IN_MONT = 1, PF_OUT_MONT = 2 };
constexpr int BIT_DECOMP_BLOCK = 128;

template <class P>
__device__ __forceinline__ F29<P> grp_fetch(const F29<P>& v, int src_lane) {
    F29<P> r;
#pragma unroll
    for (int k = 0; k < 9; k++) r.l[k] = __shfl(v.l[k], src_lane);
    return r;
}

template <class P>
__device__ __forceinline__ void trace_store(Fe<P>* __restrict__ w, size_t idx, const F29<P>& v) {
    const Fe<P> d = f29_to_mont256<P>(v);
    uint4* dst = reinterpret_cast<uint4*>(w + idx);
    dst[0] = make_uint4(d.l[0], d.l[1], d.l[2], d.l[3]);
    dst[1] = make_uint4(d.l[4], d.l[5], d.l[6], d.l[7]);
}
struct TraceDst {
    void* w;                  // Fe<P>*: the witness vector
    const uint64_t* offsets;  // per-slot element offsets, or null
    size_t first, stride;     // ... then first + (i / group) * group_stride + (i % group) * stride
    size_t group = ~(size_t)0, group_stride = 0;  // slots per frame and frame length (frame-major slot numbering)
    __device__ __forceinline__ size_t base(size_t i) const {
        return offsets ? (size_t)offsets[i] : first + (i / group) * group_stride + (i % group) * stride;
    }
    // the preimages are packed in hash order and a slot block holds nothing beside the trace
    __device__ __forceinline__ const uint4* preimage(const uint4* pre, size_t i, int arity) const { return pre + i * (arity * 2); }
    template <class P>
    __device__ __forceinline__ void beside_wide(size_t, int, const uint32_t*) const {}
    template <class P>
    __device__ __forceinline__ void beside_lane(size_t, const uint32_t*) const {}
};

template <class P, int T, class Dst>
__global__ __launch_bounds__(POSEIDON_WIDE_BLOCK) void poseidon_trace_wide_kernel(const uint4* __restrict__ pre, size_t n, const uint4* __restrict__ img,
                                                                                    int img_vec4, int rf, int rp, int flags, Dst dst) {
    extern __shared__ uint4 lds[];
    for (int i = threadIdx.x; i < img_vec4; i += POSEIDON_WIDE_BLOCK) lds[i] = img[i];
    __syncthreads();
    const uint32_t* C = reinterpret_cast<const uint32_t*>(lds);
    const PoseidonLayout<T> L(rf, rp);
    const uint32_t* mont2 = C + (size_t)L.total() * P29_STRIDE;
    const uint32_t* post = mont2 + P29_STRIDE;
    constexpr int G = 64 / T, A = T - 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool in_group = lane < G * T;
    const int g = in_group ? lane / T : 0, e = in_group ? lane % T : 0;
    const int base = g * T;
    const size_t h = ((size_t)blockIdx.x * (POSEIDON_WIDE_BLOCK / 64) + wave) * G + g;
    const bool live = in_group && h < n;
    Fe<P>* w = (Fe<P>*)dst.w;
    const size_t wb = live ? dst.base(h) : 0;

    F29<P> s;
    if (e == 0) {
        s = ld_const29<P>(C);
    } else {
        Fe<P> x = fe_zero<P>();
        if (live) {
            const uint4* src = dst.preimage(pre, h, A) + (e - 1) * 2;
            uint4 lo = src[0], hi = src[1];
            x.l[0] = lo.x; x.l[1] = lo.y; x.l[2] = lo.z; x.l[3] = lo.w;
            x.l[4] = hi.x; x.l[5] = hi.y; x.l[6] = hi.z; x.l[7] = hi.w;
        }
        s = (flags & PF_IN_MONT) ? f29_from_mont256<P>(x) : poseidon29_from_canonical<P>(x.l, mont2);
        if (live) trace_store<P>(w, wb + (e - 1), s);  // the preimage opens the block
    }
    if (live) dst.template beside_wide<P>(h, e, mont2);
    int sbox = 0;  // S-boxes before the current round
    auto sbox_emit = [&](const F29<P>& l, int idx, bool mine) {
        const F29<P> l2 = f29_sqr<P>(l), l4 = f29_sqr<P>(l2), l5 = f29_mul<P>(l4, l);
        if (mine) {
            const size_t o = wb + A + 3 * (size_t)idx;
            trace_store<P>(w, o, l2);
            trace_store<P>(w, o + 1, l4);
            trace_store<P>(w, o + 2, f29_add<P>(l5, ld_const29<P>(post + (size_t)idx * P29_STRIDE)));
        }
        return l5;
    };
    auto full_round = [&](const uint32_t* rc, const uint32_t* mat) {
        s = sbox_emit(f29_carry<P>(f29_add<P>(s, ld_const29<P>(rc + e * P29_STRIDE))), sbox + e, live);
        sbox += T;
        Dot29<P> acc;
        dot29_init<P>(acc);
#pragma unroll
        for (int i = 0; i < T; i++) {
            if (T > 5 && i == 4) dot29_carry<P>(acc);
            dot29_mac<P>(acc, grp_fetch<P>(s, base + i), ld_const29<P>(mat + (e * T + i) * P29_STRIDE));
        }
        s = dot29_finish<P>(acc);
    };
    const uint32_t* mds = C + L.mds() * P29_STRIDE;
#pragma unroll 1
    for (int r = 0; r < L.h; r++) full_round(C + (L.rc1() + r * T) * P29_STRIDE, r == L.h - 1 ? C + L.pre() * P29_STRIDE : mds);
#pragma unroll 1
    for (int p = 0; p < rp; p++) {
        const uint32_t* sp = C + (L.sp() + p * (2 * T - 1)) * P29_STRIDE;
        const F29<P> xl = sbox_emit(f29_carry<P>(f29_add<P>(s, ld_const29<P>(C + (L.pk() + p) * P29_STRIDE))), sbox, live && e == 0);
        sbox += 1;
        const F29<P> x = grp_fetch<P>(xl, base);
        F29<P> a;
#pragma unroll
        for (int k = 0; k < 9; k++) a.l[k] = e == 0 ? x.l[k] : s.l[k];
        F29<P> term = f29_mul<P>(a, ld_const29<P>(sp + e * P29_STRIDE));
#pragma unroll
        for (int off = 1; off < T; off <<= 1) {
#pragma unroll
            for (int k = 0; k < 9; k++) {
                uint32_t t = __shfl_down(term.l[k], off);
                if (e + off < T) term.l[k] += t;
            }
            if (off == 2 || off * 2 >= T) term = f29_carry<P>(term);
        }
        const F29<P> upd = f29_carry<P>(f29_add<P>(s, f29_mul<P>(x, ld_const29<P>(sp + (T - 1 + e) * P29_STRIDE))));
#pragma unroll
        for (int k = 0; k < 9; k++) s.l[k] = e == 0 ? term.l[k] : upd.l[k];
    }
#pragma unroll 1
    for (int r = 0; r < L.h; r++) full_round(r == 0 ? C + L.after() * P29_STRIDE : C + (L.rc2() + (r - 1) * T) * P29_STRIDE, mds);
    if (live && e == 1) trace_store<P>(w, wb + A + 3 * (size_t)sbox, s);  // the digest closes the block
}

template <class P, int T, class Dst>
__global__ __launch_bounds__(POSEIDON_BLOCK) void poseidon_trace_batch_kernel(const uint4* __restrict__ pre, size_t n, const uint4* __restrict__ img,
                                                                                int img_vec4, int rf, int rp, int flags, Dst dst) {
    extern __shared__ uint4 lds[];
    for (int i = threadIdx.x; i < img_vec4; i += POSEIDON_BLOCK) lds[i] = img[i];
    __syncthreads();
    const uint32_t* C = reinterpret_cast<const uint32_t*>(lds);
    const PoseidonLayout<T> L(rf, rp);
    const uint32_t* mont2 = C + (size_t)L.total() * P29_STRIDE;
    const uint32_t* post = mont2 + P29_STRIDE;
    constexpr int A = T - 1;
    Fe<P>* w = (Fe<P>*)dst.w;
    for (size_t h = (size_t)blockIdx.x * POSEIDON_BLOCK + threadIdx.x; h < n; h += (size_t)gridDim.x * POSEIDON_BLOCK) {
        const size_t wb = dst.base(h);
        F29<P> s[T];
        s[0] = ld_const29<P>(C);
        const uint4* src = dst.preimage(pre, h, A);
#pragma unroll
        for (int i = 0; i < A; i++) {
            uint4 lo = src[2 * i], hi = src[2 * i + 1];
            Fe<P> x;
            x.l[0] = lo.x; x.l[1] = lo.y; x.l[2] = lo.z; x.l[3] = lo.w;
            x.l[4] = hi.x; x.l[5] = hi.y; x.l[6] = hi.z; x.l[7] = hi.w;
            s[i + 1] = (flags & PF_IN_MONT) ? f29_from_mont256<P>(x) : poseidon29_from_canonical<P>(x.l, mont2);
            trace_store<P>(w, wb + i, s[i + 1]);
        }
        dst.template beside_lane<P>(h, mont2);
        auto emit = [&](int sbox, const F29<P>& l2, const F29<P>& l4, const F29<P>& l5k) {
            const size_t o = wb + A + 3 * (size_t)sbox;
            trace_store<P>(w, o, l2);
            trace_store<P>(w, o + 1, l4);
            trace_store<P>(w, o + 2, l5k);
        };
        poseidon29_permute_trace<P, T>(s, C, post, rf, rp, emit);
        trace_store<P>(w, wb + A + 3 * ((size_t)T * rf + rp), s[1]);
    }
}

// One workgroup, one bit decomposition (bellpepper's to_bits_le_strict as a program over the field's walk of p - 1, poseidon.hip): the
// block [value | code[j] for every aux] at w[wb].  v: eight words of LDS; every thread of the workgroup calls it.
template <class P>
__device__ __forceinline__ void bit_decomp_trace_block(const Fe<P>* __restrict__ val, int in_mont, Fe<P>* __restrict__ w, size_t wb,
                                                       const uint32_t* __restrict__ code, int ncode, const uint32_t* __restrict__ masks, uint32_t* v,
                                                       const Fe<P>& one, const Fe<P>& zero) {
    if (threadIdx.x == 0) {
        const Fe<P> x = *val;
        const Fe<P> c = in_mont ? fe_from_mont<P>(x) : x;
        for (int k = 0; k < 8; k++) v[k] = c.l[k];
        w[wb] = in_mont ? x : fe_to_mont<P>(x);
    }
    __syncthreads();
    for (int j = threadIdx.x; j < ncode; j += BIT_DECOMP_BLOCK) {
        const uint32_t cd = code[j];
        bool on;
        if (cd & 0x100u) {
            const uint32_t* m = masks + (size_t)(cd & 0xffu) * 8;
            on = true;
            for (int k = 0; k < 8; k++) on = on && ((v[k] & m[k]) == m[k]);
        } else {
            on = (v[cd >> 5] >> (cd & 31)) & 1u;
        }
        w[wb + 1 + j] = on ? one : zero;
    }
    __syncthreads();
}

// the bit-decomposition program of a field on the current device (poseidon.hip), for kernels of another translation unit
struct BitDecompView {
    const uint32_t* code = nullptr;
    const uint32_t* masks = nullptr;
    int ncode = 0;
};
BitDecompView bit_decomp_view(int field_id);

}  // namespace lurk
