// synth.hip - deterministic synthetic inputs generated directly in HBM (bench / tests; SURVEY.md
// section 8d): SplitMix64 in counter mode, seed 0x4C55524B ("LURK") + stream id.  Scalars come in the
// two distributions of the measurement plan (uniform, witness-like); bases are P_i = [k_i]G with a
// known discrete log k_i, which gives full-size MSM runs a cheap exact checksum:
//   sum_i s_i * P_i  ==  [sum_i s_i * k_i mod q] G.
// The definitions mirror oracle/pyref.py (uniform_fe / witness_like_fe / synth_base_scalar); the
// tests compare the two implementations element by element.
#include "common.hpp"
#include "curve.cuh"
#include "dispatch.hpp"

namespace lurk {

constexpr uint64_t SYNTH_SEED = 0x4C55524BULL;

__host__ __device__ inline uint64_t splitmix_at(uint64_t stream, uint64_t index) {
    uint64_t s = SYNTH_SEED + (stream << 32) + index * 0x9E3779B97F4A7C15ULL;
    s += 0x9E3779B97F4A7C15ULL;
    uint64_t z = s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

template <class F>
__device__ Fe<F> synth_uniform(uint64_t stream, uint64_t i) {
    Fe<F> v;
    for (uint64_t retry = 0;; retry++) {
#pragma unroll
        for (int w = 0; w < 4; w++) {
            uint64_t x = splitmix_at(stream, (i * 4 + w) + (retry << 40));
            v.l[2 * w] = (uint32_t)x;
            v.l[2 * w + 1] = (uint32_t)(x >> 32);
        }
        v.l[7] &= (F::NBITS == 255) ? 0x7fffffffu : 0x3fffffffu;
        if (!fe_canonical_ge_mod<F>(v.l)) return v;
    }
}
template <class F>
__device__ Fe<F> synth_witness_like(uint64_t stream, uint64_t i) {
    uint64_t sel = splitmix_at(stream + 100, i) % 100, rep = splitmix_at(stream + 101, i) % 100;
    if (rep < 5) return synth_uniform<F>(stream + 102, 0);
    if (sel < 80) return synth_uniform<F>(stream, i);
    Fe<F> v = fe_zero<F>();
    uint64_t x = splitmix_at(stream + 103, i);
    v.l[0] = (uint32_t)(sel < 92 ? (x & 1) : (x & 0xFFFF));
    return v;
}

template <class F>
__global__ __launch_bounds__(256) void synth_scalars_kernel(uint64_t stream, int dist, size_t first, size_t n, Fe<F>* out, int out_mont) {
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    Fe<F> v = dist == 0 ? synth_uniform<F>(stream, first + i) : synth_witness_like<F>(stream, first + i);
    out[i] = out_mont ? fe_to_mont<F>(v) : v;
}

// ---- fixed-base table: tab[j*256 + d] = d * 256^j * G (affine), j < 32, d < 256 ---------------
// the generator the synthetic bases are multiples of: (-1, 2) on Pallas and Vesta (y^2 = x^3 + 5), (1, 2) on BN254 G1 (y^2 = x^3 + 3),
// (1, sqrt(-16)) on Grumpkin (y^2 = x^3 - 17, the root halo2curves lists)
template <class P>
__device__ Affine<P> synth_generator() {
    Affine<P> g;
    if (P::ID == Bn254Fq::ID) {
        g.x = fe_one<P>();
        g.y = fe_dbl<P>(fe_one<P>());
    } else if (P::ID == Bn254Fr::ID) {
        // 0x0000000000000002cf135e7506a45d632d270d45f1181294833fc48d823f272c, canonical
        Fe<P> y;
        const uint32_t w[8] = {0x823f272cu, 0x833fc48du, 0xf1181294u, 0x2d270d45u, 0x06a45d63u, 0xcf135e75u, 0x00000002u, 0x00000000u};
        for (int i = 0; i < 8; i++) y.l[i] = w[i];
        g.x = fe_one<P>();
        g.y = fe_to_mont<P>(y);
    } else {
        g.x = fe_neg<P>(fe_one<P>());
        g.y = fe_dbl<P>(fe_one<P>());
    }
    return g;
}
template <class P>
__global__ void synth_table_kernel(Affine<P>* tab) {
    int id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= 32 * 256) return;
    int j = id >> 8, d = id & 255;
    const Affine<P> g = synth_generator<P>();
    Xyzz<P> b = xyzz_from_affine<P>(g);
    for (int q = 0; q < 8 * j; q++) b = xyzz_dbl<P>(b);
    tab[id] = xyzz_to_affine<P>(xyzz_mul_small<P>(b, (uint32_t)d));
}
template <class P, class SF>
__global__ __launch_bounds__(256) void synth_bases_kernel(const Affine<P>* __restrict__ tab, size_t first, size_t n, Affine<P>* out) {
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    Fe<SF> k = synth_uniform<SF>(0, first + i);
    if (fe_is_zero<SF>(k)) k.l[0] = 1;
    Xyzz<P> acc = xyzz_identity<P>();
    for (int j = 0; j < 32; j++) {
        uint32_t d = (k.l[j >> 2] >> ((j & 3) * 8)) & 0xff;
        if (d) xyzz_madd<P>(acc, tab[j * 256 + d], false);
    }
    out[i] = xyzz_to_affine<P>(acc);
}

// powers of tau: out[i] = [tau^(first + i)] G - a KZG structured reference string with a KNOWN trapdoor (tests and benchmarks only).
// A lane raises tau to its own index (<= 2 log2(index) products) and walks the fixed-base table like synth_bases_kernel.
template <class P, class SF>
__global__ __launch_bounds__(256) void synth_kzg_bases_kernel(const Affine<P>* __restrict__ tab, Fe<SF> tau_mont, size_t first, size_t n, Affine<P>* out) {
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t e = first + i;
    Fe<SF> k = fe_one<SF>();
    int top = 63;
    while (top >= 0 && !((e >> top) & 1u)) top--;
    for (int b = top; b >= 0; b--) {
        k = fe_mul<SF>(k, k);
        if ((e >> b) & 1u) k = fe_mul<SF>(k, tau_mont);
    }
    k = fe_from_mont<SF>(k);
    Xyzz<P> acc = xyzz_identity<P>();
    for (int j = 0; j < 32; j++) {
        uint32_t d = (k.l[j >> 2] >> ((j & 3) * 8)) & 0xff;
        if (d) xyzz_madd<P>(acc, tab[j * 256 + d], false);
    }
    out[i] = xyzz_to_affine<P>(acc);
}

static std::mutex g_tab_mu;
static std::map<std::pair<int, int>, DevBuf> g_tab;  // (device, curve) -> table

template <class P>
static const Affine<P>* get_table(int curve, hipStream_t s) {
    int dev = 0;
    LURK_HIP_CHECK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_tab_mu);
    auto key = std::make_pair(dev, curve);
    auto it = g_tab.find(key);
    if (it == g_tab.end()) {
        DevBuf b(32 * 256 * sizeof(Affine<P>));
        hipLaunchKernelGGL((synth_table_kernel<P>), dim3(32), dim3(256), 0, s, b.as<Affine<P>>());
        LURK_HIP_CHECK(hipGetLastError());
        LURK_HIP_CHECK(hipStreamSynchronize(s));
        it = g_tab.emplace(key, std::move(b)).first;
    }
    return it->second.as<Affine<P>>();
}

}  // namespace lurk

using namespace lurk;

extern "C" {

int lurk_hip_synth_scalars_dev(int field_id, uint64_t stream_id, int dist, size_t first, size_t n, void* d_out, int out_mont, void* stream) {
    return guarded([&] {
        LURK_REQUIRE(field_id >= 0 && field_id <= LURK_FIELD_BN254_FQ, "unknown field id");
        LURK_REQUIRE(dist == 0 || dist == 1, "dist must be 0 (uniform) or 1 (witness-like)");
        if (n == 0) return;
        LURK_REQUIRE(d_out, "null buffer");
        hipStream_t s = (hipStream_t)stream;
        dim3 grid(div_up(n, 256)), block(256);
        auto launch = [&](auto tag) {
            using F = decltype(tag);
            hipLaunchKernelGGL((synth_scalars_kernel<F>), grid, block, 0, s, stream_id, dist, first, n, (Fe<F>*)d_out, out_mont);
        };
        if (field_id == LURK_FIELD_BN254_FQ) launch(Bn254Fq{});  // the fourth field is served here only
        else with_field(field_id, launch);
        LURK_HIP_CHECK(hipGetLastError());
    });
}

int lurk_hip_synth_bases_dev(int curve, size_t first, size_t n, void* d_out, void* stream) {
    return guarded([&] {
        LURK_REQUIRE(curve >= LURK_CURVE_PALLAS && curve <= LURK_CURVE_GRUMPKIN, "unknown curve id");
        if (n == 0) return;
        LURK_REQUIRE(d_out, "null buffer");
        hipStream_t s = (hipStream_t)stream;
        dim3 grid(div_up(n, 256)), block(256);
        with_curve(curve, [&](auto base, auto scalar) {
            using P = decltype(base);
            const Affine<P>* tab = get_table<P>(curve, s);
            hipLaunchKernelGGL((synth_bases_kernel<P, decltype(scalar)>), grid, block, 0, s, tab, first, n, (Affine<P>*)d_out);
        });
        LURK_HIP_CHECK(hipGetLastError());
    });
}

int lurk_hip_synth_kzg_bases_dev(int curve, const void* tau32_canonical, size_t first, size_t n, void* d_out, void* stream) {
    return guarded([&] {
        LURK_REQUIRE(curve >= LURK_CURVE_PALLAS && curve <= LURK_CURVE_GRUMPKIN, "unknown curve id");
        if (curve != LURK_CURVE_BN254)
            throw HipFailure{LURK_HIP_ERR_INVALID_ARG, std::string("lurk_hip_synth_kzg_bases_dev is offered on BN254 G1 only, not on ") + curve_name(curve)};
        LURK_REQUIRE(tau32_canonical, "null argument");
        Fe<Bn254Fr> tau;
        memcpy(tau.l, tau32_canonical, 32);
        LURK_REQUIRE(!fe_canonical_ge_mod<Bn254Fr>(tau.l), "tau is not reduced modulo the group order");
        LURK_REQUIRE(first + n >= first, "index range overflows");
        if (n == 0) return;
        LURK_REQUIRE(d_out, "null buffer");
        hipStream_t s = (hipStream_t)stream;
        const Affine<Bn254Fq>* tab = get_table<Bn254Fq>(LURK_CURVE_BN254, s);
        hipLaunchKernelGGL((synth_kzg_bases_kernel<Bn254Fq, Bn254Fr>), dim3(div_up(n, 256)), dim3(256), 0, s, tab, fe_to_mont<Bn254Fr>(tau), first, n,
                           (Affine<Bn254Fq>*)d_out);
        LURK_HIP_CHECK(hipGetLastError());
    });
}
}
