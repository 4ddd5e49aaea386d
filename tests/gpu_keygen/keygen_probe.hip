// keygen_probe.hip - TEST ONLY: the stages of the per-point map of key generation (lurk_beta_amd/csrc/keygen_point.cuh), one case
// per lane, for tests/test_gpu_keygen_stages.py to compare with hashlib, Python integers and oracle/keygen_ref.py.
//
//   keygen_probe <in> <out>
//
// <in>:  u32 n_sets, then per set: u32 curve (0 Pallas, 1 Vesta), op, n, msg_len; char domain_prefix[64], curve_name[16], suite[32]
//        (NUL-terminated: the three parts of the tag, handed to make_keygen_consts as they are); n records of IN_BYTES[op]
// <out>: per set, in input order: n records of OUT_BYTES[op]
// Field elements cross the files as canonical integers, 32 bytes little-endian; the probe converts to and from Montgomery.
//
// Every set runs three times: on the host with the same KG_HD functions in a plain loop, on the device with 128 threads per block
// (keygen_kernel's launch bound) and on the device with 64.  Exit status 0 only if every HIP call succeeded and the three outputs
// are identical bytes.  The host pass covers all sets before the first HIP call, and it is compiled with LURK_FE_CHECK (field.cuh):
// fe_mul, fe_add and fe_sub abort on an operand >= p, so a stage that breaks their contract ends the probe before it touches the
// device, even where the result would still come out right.
#define LURK_FE_CHECK 1
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../lurk_beta_amd/csrc/keygen_point.cuh"

using namespace lurk;

enum Op : int { B2B_HASH = 0, FROM_BE64, IS_SQUARE, SQRT, HASH_TO_FIELD, MAP_TO_CURVE, ISO_ADD, ISO_MAP, POINT, N_OPS };
//                                 b2b  be64 issq sqrt h2f  m2c  add  map  point
static const unsigned IN_BYTES[N_OPS] = {260, 64, 32, 32, 64, 64, 128, 64, 64};
static const unsigned OUT_BYTES[N_OPS] = {64, 32, 4, 32, 64, 128, 68, 64, 64};

template <class P>
KG_HD inline Fe<P> ld_canonical(const uint8_t* src) {  // 32 bytes little-endian, canonical -> Montgomery
    Fe<P> x;
    for (int i = 0; i < 8; i++) {
        uint32_t w = 0;
        for (int k = 0; k < 4; k++) w |= (uint32_t)src[4 * i + k] << (8 * k);
        x.l[i] = w;
    }
    return fe_to_mont<P>(x);
}
template <class P>
KG_HD inline void st_canonical(uint8_t* dst, const Fe<P>& mont) {
    const Fe<P> x = fe_from_mont<P>(mont);
    for (int i = 0; i < 8; i++)
        for (int k = 0; k < 4; k++) dst[4 * i + k] = (uint8_t)(x.l[i] >> (8 * k));
}
KG_HD inline void st_u32(uint8_t* dst, uint32_t v) {
    for (int k = 0; k < 4; k++) dst[k] = (uint8_t)(v >> (8 * k));
}

// one record: `in` and `out` point at this lane's record
template <class P>
KG_HD inline void probe_one(int op, const uint8_t* in, uint8_t* out, const KeygenConsts<P>& K) {
    switch (op) {
        case B2B_HASH: {
            unsigned len = 0;
            for (int k = 0; k < 4; k++) len |= (unsigned)in[k] << (8 * k);
            if (len > 256) len = 256;  // main refuses such a record before anything runs
            uint8_t buf[256];
            for (unsigned k = 0; k < 256; k++) buf[k] = k < len ? in[4 + k] : 0;  // b2b_hash's contract: zero padded
            b2b_hash(buf, len, out);
            break;
        }
        case FROM_BE64: st_canonical<P>(out, kg_from_be64<P>(in, K.r3)); break;
        case IS_SQUARE: st_u32(out, kg_is_square<P>(ld_canonical<P>(in), K) ? 1u : 0u); break;
        case SQRT: st_canonical<P>(out, kg_sqrt<P>(ld_canonical<P>(in), K)); break;
        case HASH_TO_FIELD: {
            Fe<P> u[2];
            kg_hash_to_field<P>(in, K, u);
            st_canonical<P>(out, u[0]);
            st_canonical<P>(out + 32, u[1]);
            break;
        }
        case MAP_TO_CURVE: {
            Affine<P> q0, q1;
            kg_map_to_curve<P>(ld_canonical<P>(in), ld_canonical<P>(in + 32), K, q0, q1);
            st_canonical<P>(out, q0.x);
            st_canonical<P>(out + 32, q0.y);
            st_canonical<P>(out + 64, q1.x);
            st_canonical<P>(out + 96, q1.y);
            break;
        }
        case ISO_ADD: {
            Affine<P> q0, q1;
            q0.x = ld_canonical<P>(in);
            q0.y = ld_canonical<P>(in + 32);
            q1.x = ld_canonical<P>(in + 64);
            q1.y = ld_canonical<P>(in + 96);
            Fe<P> sx, sy;
            const bool identity = kg_iso_add<P>(q0, q1, K, sx, sy);
            st_canonical<P>(out, sx);
            st_canonical<P>(out + 32, sy);
            st_u32(out + 64, identity ? 1u : 0u);
            break;
        }
        case ISO_MAP: {
            const Affine<P> r = kg_iso_map<P>(ld_canonical<P>(in), ld_canonical<P>(in + 32), K);
            st_canonical<P>(out, r.x);
            st_canonical<P>(out + 32, r.y);
            break;
        }
        default: {
            const Affine<P> r = keygen_point<P>(in, K);
            st_canonical<P>(out, r.x);
            st_canonical<P>(out + 32, r.y);
            break;
        }
    }
}

template <class P>
__global__ __launch_bounds__(128) void probe_kernel(int op, unsigned n, unsigned in_bytes, unsigned out_bytes, const uint8_t* __restrict__ in,
                                                    uint8_t* __restrict__ out, KeygenConsts<P> K) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    probe_one<P>(op, in + (size_t)i * in_bytes, out + (size_t)i * out_bytes, K);
}

#define CHECK(x)                                                                          \
    do {                                                                                  \
        hipError_t e_ = (x);                                                              \
        if (e_ != hipSuccess) {                                                           \
            fprintf(stderr, "%s failed: %s\n", #x, hipGetErrorString(e_));                \
            exit(2);                                                                      \
        }                                                                                 \
    } while (0)

struct SetHeader {
    uint32_t curve, op, n, msg_len;
    char domain_prefix[64], curve_name[16], suite[32];
};
struct Set {
    SetHeader h;
    std::vector<uint8_t> in, host;
};

template <class P>
static KeygenConsts<P> set_consts(const SetHeader& h) {
    lurk_hip_ck_params prm;
    memset(&prm, 0, sizeof(prm));
    prm.struct_size = (uint32_t)sizeof(prm);
    prm.bytes_per_point = h.msg_len;
    memcpy(prm.curve_name_pallas, h.curve_name, sizeof(prm.curve_name_pallas));
    memcpy(prm.curve_name_vesta, h.curve_name, sizeof(prm.curve_name_vesta));
    memcpy(prm.suite, h.suite, sizeof(prm.suite));
    return make_keygen_consts<P>((int)h.curve, h.domain_prefix, prm);
}

template <class P>
static void run_host(Set& st) {
    const KeygenConsts<P> K = set_consts<P>(st.h);
    const int op = (int)st.h.op;
    const unsigned ib = IN_BYTES[op], ob = OUT_BYTES[op];
    for (uint32_t i = 0; i < st.h.n; i++) probe_one<P>(op, st.in.data() + (size_t)i * ib, st.host.data() + (size_t)i * ob, K);
}

// the two device runs of one set; returns the number of disagreements (0 or 1)
template <class P>
static int run_device(uint32_t s, const Set& st, std::vector<uint8_t>& o128) {
    const SetHeader& h = st.h;
    const KeygenConsts<P> K = set_consts<P>(h);
    const int op = (int)h.op;
    const unsigned ib = IN_BYTES[op], ob = OUT_BYTES[op];
    const size_t in_size = (size_t)h.n * ib, out_size = (size_t)h.n * ob;
    std::vector<uint8_t> o64(out_size);
    uint8_t *dI, *dO;
    CHECK(hipMalloc(&dI, in_size));
    CHECK(hipMalloc(&dO, out_size));
    CHECK(hipMemcpy(dI, st.in.data(), in_size, hipMemcpyHostToDevice));
    CHECK(hipMemset(dO, 0xA5, out_size));
    probe_kernel<P><<<(h.n + 127) / 128, 128>>>(op, h.n, ib, ob, dI, dO, K);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(o128.data(), dO, out_size, hipMemcpyDeviceToHost));
    CHECK(hipMemset(dO, 0x5A, out_size));
    probe_kernel<P><<<(h.n + 63) / 64, 64>>>(op, h.n, ib, ob, dI, dO, K);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(o64.data(), dO, out_size, hipMemcpyDeviceToHost));
    CHECK(hipFree(dI));
    CHECK(hipFree(dO));
    int bad = 0;
    if (memcmp(o128.data(), o64.data(), out_size) != 0) {
        fprintf(stderr, "set %u curve %u op %d: block sizes 128 and 64 disagree\n", s, h.curve, op);
        bad = 1;
    }
    if (memcmp(o128.data(), st.host.data(), out_size) != 0) {
        fprintf(stderr, "set %u curve %u op %d: the device and the host disagree\n", s, h.curve, op);
        bad = 1;
    }
    return bad;
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s <in> <out>\n", argv[0]);
        return 1;
    }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) {
        fprintf(stderr, "cannot open the input or the output file\n");
        return 1;
    }
    uint32_t n_sets = 0;
    if (fread(&n_sets, 4, 1, in) != 1 || n_sets > 4096) {
        fprintf(stderr, "input truncated\n");
        return 3;
    }
    std::vector<Set> sets(n_sets);
    for (uint32_t s = 0; s < n_sets; s++) {
        SetHeader& h = sets[s].h;
        if (fread(&h, sizeof(h), 1, in) != 1) {
            fprintf(stderr, "input truncated\n");
            return 3;
        }
        if (h.curve > 1 || h.op >= (uint32_t)N_OPS || h.n == 0 || h.n > (1u << 20) || h.msg_len < 1 || h.msg_len > 64 ||
            !memchr(h.domain_prefix, 0, sizeof(h.domain_prefix)) || !memchr(h.curve_name, 0, sizeof(h.curve_name)) ||
            !memchr(h.suite, 0, sizeof(h.suite))) {
            fprintf(stderr, "bad set header: curve %u op %u n %u msg_len %u\n", h.curve, h.op, h.n, h.msg_len);
            return 3;
        }
        const unsigned ib = IN_BYTES[h.op], ob = OUT_BYTES[h.op];
        sets[s].in.resize((size_t)h.n * ib);
        sets[s].host.resize((size_t)h.n * ob);
        if (fread(sets[s].in.data(), 1, sets[s].in.size(), in) != sets[s].in.size()) {
            fprintf(stderr, "input truncated\n");
            return 3;
        }
        if (h.op == B2B_HASH)
            for (uint32_t i = 0; i < h.n; i++) {
                uint32_t len;
                memcpy(&len, sets[s].in.data() + (size_t)i * ib, 4);
                if (len > 256) {
                    fprintf(stderr, "set %u record %u: length %u above 256\n", s, i, len);
                    return 3;
                }
            }
    }
    fclose(in);
    int disagreements = 0;
    try {
        for (uint32_t s = 0; s < n_sets; s++) {  // the host pass: no HIP call yet
            if (sets[s].h.curve == 0) run_host<PallasFp>(sets[s]);
            else run_host<PallasFq>(sets[s]);
        }
        for (uint32_t s = 0; s < n_sets; s++) {
            std::vector<uint8_t> o(sets[s].host.size());
            disagreements += sets[s].h.curve == 0 ? run_device<PallasFp>(s, sets[s], o) : run_device<PallasFq>(s, sets[s], o);
            if (fwrite(o.data(), 1, o.size(), out) != o.size()) {
                fprintf(stderr, "output write failed\n");
                return 4;
            }
        }
    } catch (const HipFailure& e) {
        fprintf(stderr, "%s\n", e.msg.c_str());
        return 3;
    }
    if (fclose(out) != 0) return 4;
    printf("sets %u, disagreements %d\n", n_sets, disagreements);
    return disagreements ? 5 : 0;
}
