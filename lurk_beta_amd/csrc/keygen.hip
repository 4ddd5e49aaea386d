// keygen.hip - commitment-key generation on the device.
//
// Reference: PublicParams::setup (/root/reference/src/proof/nova.rs:196-216) -> arecibo CommitmentEngine::setup(b"ck", n) ->
// DlogGroup::from_label: SHAKE256(label) squeezed 32 bytes per point, point i = pasta_curves hash_to_curve("from_uniform_bytes")
// of its bytes, all batch-normalised to affine.  Both dependencies are un-vendored; restated from their published algorithms
// (oracle/keygen_ref.py states them in Python and checks the constants mathematically; parity unpinned against upstream bytes):
//   hash_to_field   RFC 9380 expand_message_xmd with BLAKE2b-512, DST "<domain>-<curve>_XMD:BLAKE2b_SSWU_RO_", two elements
//   map_to_curve    simplified SWU on the 3-isogenous curve y^2 = x^3 + A x + 1265, Z = -13, sign of y = sgn0(u)
//   + / iso_map     the two images added on the isogenous curve, then the degree-3 isogeny onto y^2 = x^3 + 5
// The XOF stream is inherently sequential: the host squeezes it (Keccak-f[1600]); everything per point - three BLAKE2b hashes, two
// Legendre symbols, two square roots (Tonelli-Shanks, 2-adicity 32), three inversions - runs one point per lane.
// The per-point map and its constants are keygen_point.cuh; here: the XOF, the parameter block, the kernel and the entry points.
#include <memory>
#include <mutex>
#include <string>

#include "common.hpp"
#include "curve.cuh"
#include "dispatch.hpp"
#include "keccak.hpp"
#include "keygen_point.cuh"

namespace lurk {

// ---- SHAKE256 (host): Keccak-f from keccak.hpp ----------------------------------------------------------------------------------
static void shake_xof(size_t RATE, const uint8_t* in, size_t in_len, uint8_t* out, size_t out_len) {
    uint64_t st[25] = {0};
    uint8_t* sb = reinterpret_cast<uint8_t*>(st);  // little-endian host
    size_t pos = 0;
    for (size_t i = 0; i < in_len; i++) {
        sb[pos++] ^= in[i];
        if (pos == RATE) { keccak_f(st); pos = 0; }
    }
    sb[pos] ^= 0x1f;
    sb[RATE - 1] ^= 0x80;
    keccak_f(st);
    size_t got = 0;
    while (got < out_len) {
        size_t take = out_len - got < RATE ? out_len - got : RATE;
        memcpy(out + got, sb, take);
        got += take;
        if (got < out_len) keccak_f(st);
    }
}
void shake256(const uint8_t* in, size_t in_len, uint8_t* out, size_t out_len) { shake_xof(136, in, in_len, out, out_len); }

template <class P>
__global__ __launch_bounds__(128) void keygen_kernel(const uint8_t* __restrict__ uniform, size_t n, KeygenConsts<P> K, Affine<P>* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 128 + threadIdx.x;
    if (i >= n) return;
    out[i] = keygen_point<P>(uniform + i * K.msg_len, K);
}

// ---- run-time parameters of from_label (round 6; include/lurk_hip.h: lurk_hip_ck_params) ----------------------------------------
// Like the random oracle's (transcript.hip): every constant of DlogGroup::from_label / hash_to_curve that was recalled from memory is a
// field, process-wide, defaults = what rounds 1-5 compiled in.
static lurk_hip_ck_params ck_params_default() {
    lurk_hip_ck_params p;
    memset(&p, 0, sizeof(p));
    p.struct_size = (uint32_t)sizeof(p);
    p.xof = LURK_CK_XOF_SHAKE256;
    p.bytes_per_point = 32;
    strcpy(p.domain_prefix, "from_uniform_bytes");
    strcpy(p.curve_name_pallas, "pallas");
    strcpy(p.curve_name_vesta, "vesta");
    strcpy(p.suite, "_XMD:BLAKE2b_SSWU_RO_");
    return p;
}
static std::mutex g_ck_mu;
static lurk_hip_ck_params g_ck = ck_params_default();
static lurk_hip_ck_params ck_params() {
    std::lock_guard<std::mutex> lk(g_ck_mu);
    return g_ck;
}
static bool c_string_within(const char* s, size_t cap) { return memchr(s, 0, cap) != nullptr; }
static void ck_params_validate(const lurk_hip_ck_params& p) {
    LURK_REQUIRE(p.struct_size == sizeof(lurk_hip_ck_params), "lurk_hip_ck_params: struct_size does not match this library's layout");
    LURK_REQUIRE(p.xof == LURK_CK_XOF_SHAKE256 || p.xof == LURK_CK_XOF_SHAKE128, "lurk_hip_ck_params: unknown xof");
    LURK_REQUIRE(p.bytes_per_point >= 1 && p.bytes_per_point <= 64, "lurk_hip_ck_params: bytes_per_point must be in 1..64");
    LURK_REQUIRE(c_string_within(p.domain_prefix, sizeof(p.domain_prefix)) && c_string_within(p.curve_name_pallas, sizeof(p.curve_name_pallas)) &&
                     c_string_within(p.curve_name_vesta, sizeof(p.curve_name_vesta)) && c_string_within(p.suite, sizeof(p.suite)),
                 "lurk_hip_ck_params: a string is not NUL-terminated");
    for (int curve = 0; curve < 2; curve++)
        LURK_REQUIRE(131 + p.bytes_per_point + ck_dst(p, curve, p.domain_prefix).size() + 1 <= 256 && ck_dst(p, curve, p.domain_prefix).size() < 63,
                     "lurk_hip_ck_params: message + domain-separation tag do not fit two BLAKE2b blocks");
}

template <class P>
static void keygen_device(int curve, const char* domain, const void* d_uniform, size_t n, void* d_out, hipStream_t s) {
    if (n == 0) return;
    static_assert(P::ID != 2, "Pasta only");
    LURK_REQUIRE(P::mod(0) == 1u, "unexpected modulus");  // the low 32 bits of p - 1 are zero: 2-adicity 32
    const KeygenConsts<P> K = make_keygen_consts<P>(curve, domain, ck_params());
    ProfScope ps("keygen", s);
    hipLaunchKernelGGL((keygen_kernel<P>), dim3(div_up(n, 128)), dim3(128), 0, s, (const uint8_t*)d_uniform, n, K, (Affine<P>*)d_out);
    LURK_HIP_CHECK(hipGetLastError());
}

static std::vector<uint8_t> ck_xof_stream(const lurk_hip_ck_params& prm, const void* label, size_t label_len, size_t n) {
    std::vector<uint8_t> stream(n * prm.bytes_per_point);
    shake_xof(prm.xof == LURK_CK_XOF_SHAKE128 ? 168 : 136, (const uint8_t*)label, label_len, stream.data(), stream.size());
    return stream;
}

void keygen_from_label_device(int curve, const void* label, size_t label_len, size_t n, void* d_out, hipStream_t s) {
    const lurk_hip_ck_params prm = ck_params();
    const std::vector<uint8_t> stream = ck_xof_stream(prm, label, label_len, n);
    DevBuf d_u(stream.size());
    if (n) LURK_HIP_CHECK(hipMemcpyAsync(d_u.p, stream.data(), stream.size(), hipMemcpyHostToDevice, s));
    with_pasta_curve(curve, [&](auto P, auto) { keygen_device<decltype(P)>(curve, prm.domain_prefix, d_u.p, n, d_out, s); });
    LURK_HIP_CHECK(hipStreamSynchronize(s));  // the staging buffers go out of scope
}

// the same map on the host, one point after the other (~0.3 ms each): the first points of a key for a probe record or a CPU test
template <class P>
static void keygen_from_label_host(int curve, const void* label, size_t label_len, size_t n, void* out) {
    const lurk_hip_ck_params prm = ck_params();
    const std::vector<uint8_t> stream = ck_xof_stream(prm, label, label_len, n);
    const KeygenConsts<P> K = make_keygen_consts<P>(curve, prm.domain_prefix, prm);
    for (size_t i = 0; i < n; i++) {
        const Affine<P> pt = keygen_point<P>(stream.data() + i * prm.bytes_per_point, K);
        memcpy((char*)out + 64 * i, &pt, 64);
    }
}

}  // namespace lurk

using namespace lurk;

extern "C" {

int lurk_hip_shake256(const void* in, size_t in_len, void* out, size_t out_len) {
    // pure host computation (the CPU tests compare it with hashlib)
    return host_guarded([&] {
        LURK_REQUIRE((in || in_len == 0) && (out || out_len == 0), "null buffer");
        shake256((const uint8_t*)in, in_len, (uint8_t*)out, out_len);
    });
}

int lurk_hip_ck_params_get(lurk_hip_ck_params* out) {
    return host_guarded([&] {
        LURK_REQUIRE(out, "null argument");
        *out = ck_params();
    });
}
int lurk_hip_ck_params_set(const lurk_hip_ck_params* params) {
    return host_guarded([&] {
        const lurk_hip_ck_params p = params ? *params : ck_params_default();  // NULL: back to the defaults
        ck_params_validate(p);
        std::lock_guard<std::mutex> lk(g_ck_mu);
        g_ck = p;
    });
}

int lurk_hip_ck_from_label_host(int curve, const void* label, size_t label_len, size_t npoints, void* out_affine64) {
    // pure host computation: no device is needed
    return host_guarded([&] {
        require_pasta_curve(curve, "lurk_hip_ck_from_label_host (hash-to-curve)");
        LURK_REQUIRE((label || label_len == 0) && (npoints == 0 || out_affine64), "null argument");
        LURK_REQUIRE(npoints <= ((size_t)1 << 16), "the host form maps at most 2^16 points: build keys with lurk_hip_ck_from_label_dev / lurk_hip_msm_ctx_from_label");
        with_pasta_curve(curve, [&](auto P, auto) { keygen_from_label_host<decltype(P)>(curve, label, label_len, npoints, out_affine64); });
    });
}

int lurk_hip_ck_hash_to_curve_dev(int curve, const char* domain_prefix, const void* d_uniform32, size_t n, void* d_out_affine64, void* stream) {
    return guarded([&] {
        require_pasta_curve(curve, "lurk_hip_ck_hash_to_curve_dev");
        LURK_REQUIRE(domain_prefix && (n == 0 || (d_uniform32 && d_out_affine64)), "null argument");
        with_pasta_curve(curve, [&](auto P, auto) { keygen_device<decltype(P)>(curve, domain_prefix, d_uniform32, n, d_out_affine64, (hipStream_t)stream); });
    });
}

int lurk_hip_ck_from_label_dev(int curve, const void* label, size_t label_len, size_t npoints, void* d_out_affine64, void* stream) {
    return guarded([&] {
        require_pasta_curve(curve, "lurk_hip_ck_from_label_dev (hash-to-curve)");
        LURK_REQUIRE((label || label_len == 0) && (npoints == 0 || d_out_affine64), "null argument");
        keygen_from_label_device(curve, label, label_len, npoints, d_out_affine64, (hipStream_t)stream);
    });
}
}
