// field_probe.hip - TEST ONLY: the device arithmetic layer (field.cuh, field29.cuh and the generated asm blocks they call),
// one operation per lane, for tests/test_gpu_field_arith.py to compare with Python integers.
//
//   field_probe <in> <out>
//
// <in>:  u32 n_sets, then per set: u32 field, n, width (8 or 9), n_ops, ops[n_ops], A[n * width], B[n * width]
// <out>: per set and op, in input order: n rows of 9 u32 (8 x 32 results use the first 8 words, the 9th is 0)
//
// Every op runs twice, with 256 and with 64 threads per block, and the two results must be identical; one lane per row, so a
// grid of n / 64 or n / 256 blocks.  Exit status 0 only if every HIP call succeeded and the two block sizes agreed.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../lurk_beta_amd/csrc/field29.cuh"

using namespace lurk;

enum Op : int {
    FE_ADD = 0, FE_SUB, FE_NEG, FE_MUL, FE_SQR, FE_TO_MONT, FE_FROM_MONT, FE_INV, FE_DOT3, FE_DOT9,
    F29_MUL = 10, F29_SQR, F29_ADD, F29_SUB, F29_CARRY, F29_FROM_MONT256, F29_TO_MONT256, F29_INVERT, F29_DOT3, F29_DOT9,
    N_OPS
};

template <class P>
__device__ Fe<P> ld_fe(const uint32_t* src, int width, int row) {
    Fe<P> x;
#pragma unroll
    for (int k = 0; k < 8; k++) x.l[k] = src[(size_t)row * width + k];
    return x;
}
// width 9: the nine limbs as given; width 8: the 9 x 29 limbs of the same plain integer
template <class P>
__device__ F29<P> ld_f29(const uint32_t* src, int width, int row) {
    if (width == 8) {
        uint32_t w[8];
#pragma unroll
        for (int k = 0; k < 8; k++) w[k] = src[(size_t)row * width + k];
        return f29_from_plain<P>(w);
    }
    F29<P> x;
#pragma unroll
    for (int k = 0; k < 9; k++) x.l[k] = src[(size_t)row * width + k];
    return x;
}

template <class P, int T>
__device__ Fe<P> dot_rows(const uint32_t* A, const uint32_t* B, int width, int row, int n) {
    DotAcc<P> acc;
    dot_init<P>(acc);
    for (int j = 0; j < T; j++) {
        const int r = (row + j) % n;
        dot_mac<P>(acc, ld_fe<P>(A, width, r), ld_fe<P>(B, width, r));
    }
    return dot_finish<P, T>(acc);
}
// the call pattern of poseidon29_dense: a carry pass before the fifth term of a longer sum
template <class P, int T>
__device__ F29<P> dot29_rows(const uint32_t* A, const uint32_t* B, int width, int row, int n) {
    Dot29<P> acc;
    dot29_init<P>(acc);
    for (int j = 0; j < T; j++) {
        const int r = (row + j) % n;
        if (T > 5 && j == 4) dot29_carry<P>(acc);
        dot29_mac<P>(acc, ld_f29<P>(A, width, r), ld_f29<P>(B, width, r));
    }
    return dot29_finish<P>(acc);
}

template <class P>
__global__ void probe_kernel(int op, int n, int width, const uint32_t* __restrict__ A, const uint32_t* __restrict__ B,
                             uint32_t* __restrict__ O) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t r[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (op < F29_MUL) {
        const Fe<P> a = ld_fe<P>(A, width, i), b = ld_fe<P>(B, width, i);
        Fe<P> x;
        switch (op) {
            case FE_ADD: x = fe_add<P>(a, b); break;
            case FE_SUB: x = fe_sub<P>(a, b); break;
            case FE_NEG: x = fe_neg<P>(a); break;
            case FE_MUL: x = fe_mul<P>(a, b); break;
            case FE_SQR: x = fe_sqr<P>(a); break;
            case FE_TO_MONT: x = fe_to_mont<P>(a); break;
            case FE_FROM_MONT: x = fe_from_mont<P>(a); break;
            case FE_INV: x = fe_inv<P>(a); break;
            case FE_DOT3: x = dot_rows<P, 3>(A, B, width, i, n); break;
            default: x = dot_rows<P, 9>(A, B, width, i, n); break;
        }
        for (int k = 0; k < 8; k++) r[k] = x.l[k];
    } else if (op == F29_FROM_MONT256 || op == F29_TO_MONT256) {
        if (op == F29_FROM_MONT256) {
            const F29<P> x = f29_from_mont256<P>(ld_fe<P>(A, width, i));
            for (int k = 0; k < 9; k++) r[k] = x.l[k];
        } else {
            const Fe<P> x = f29_to_mont256<P>(ld_f29<P>(A, width, i));
            for (int k = 0; k < 8; k++) r[k] = x.l[k];
        }
    } else {
        const F29<P> a = ld_f29<P>(A, width, i), b = ld_f29<P>(B, width, i);
        F29<P> x;
        switch (op) {
            case F29_MUL: x = f29_mul<P>(a, b); break;
            case F29_SQR: x = f29_sqr<P>(a); break;
            case F29_ADD: x = f29_add<P>(a, b); break;
            case F29_SUB: x = f29_sub<P>(a, b); break;
            case F29_CARRY: x = f29_carry<P>(a); break;
            case F29_INVERT: x = f29_invert<P>(a); break;
            case F29_DOT3: x = dot29_rows<P, 3>(A, B, width, i, n); break;
            default: x = dot29_rows<P, 9>(A, B, width, i, n); break;
        }
        for (int k = 0; k < 9; k++) r[k] = x.l[k];
    }
    for (int k = 0; k < 9; k++) O[(size_t)i * 9 + k] = r[k];
}

#define CHECK(x)                                                                          \
    do {                                                                                  \
        hipError_t e_ = (x);                                                              \
        if (e_ != hipSuccess) {                                                           \
            fprintf(stderr, "%s failed: %s\n", #x, hipGetErrorString(e_));                \
            exit(2);                                                                      \
        }                                                                                 \
    } while (0)

static void launch(int field, int op, int n, int width, const uint32_t* A, const uint32_t* B, uint32_t* O, int bs) {
    const int grid = (n + bs - 1) / bs;
    if (field == 0) probe_kernel<PallasFp><<<grid, bs>>>(op, n, width, A, B, O);
    else if (field == 1) probe_kernel<PallasFq><<<grid, bs>>>(op, n, width, A, B, O);
    else probe_kernel<Bn254Fr><<<grid, bs>>>(op, n, width, A, B, O);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
}

static uint32_t rd(FILE* f) {
    uint32_t v;
    if (fread(&v, 4, 1, f) != 1) {
        fprintf(stderr, "input truncated\n");
        exit(3);
    }
    return v;
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
    const uint32_t n_sets = rd(in);
    int disagreements = 0;
    for (uint32_t s = 0; s < n_sets; s++) {
        const int field = (int)rd(in), n = (int)rd(in), width = (int)rd(in), n_ops = (int)rd(in);
        if (field < 0 || field > 2 || n <= 0 || n > (1 << 22) || (width != 8 && width != 9) || n_ops <= 0 || n_ops > N_OPS) {
            fprintf(stderr, "bad set header: field %d n %d width %d ops %d\n", field, n, width, n_ops);
            return 3;
        }
        std::vector<int> ops(n_ops);
        for (int k = 0; k < n_ops; k++) {
            ops[k] = (int)rd(in);
            if (ops[k] < 0 || ops[k] >= N_OPS) {
                fprintf(stderr, "bad op %d\n", ops[k]);
                return 3;
            }
        }
        const size_t in_words = (size_t)n * width, out_words = (size_t)n * 9;
        std::vector<uint32_t> a(in_words), b(in_words), o256(out_words), o64(out_words);
        if (fread(a.data(), 4, in_words, in) != in_words || fread(b.data(), 4, in_words, in) != in_words) {
            fprintf(stderr, "input truncated\n");
            return 3;
        }
        uint32_t *dA, *dB, *dO;
        CHECK(hipMalloc(&dA, in_words * 4));
        CHECK(hipMalloc(&dB, in_words * 4));
        CHECK(hipMalloc(&dO, out_words * 4));
        CHECK(hipMemcpy(dA, a.data(), in_words * 4, hipMemcpyHostToDevice));
        CHECK(hipMemcpy(dB, b.data(), in_words * 4, hipMemcpyHostToDevice));
        for (int k = 0; k < n_ops; k++) {
            CHECK(hipMemset(dO, 0xA5, out_words * 4));
            launch(field, ops[k], n, width, dA, dB, dO, 256);
            CHECK(hipMemcpy(o256.data(), dO, out_words * 4, hipMemcpyDeviceToHost));
            CHECK(hipMemset(dO, 0x5A, out_words * 4));
            launch(field, ops[k], n, width, dA, dB, dO, 64);
            CHECK(hipMemcpy(o64.data(), dO, out_words * 4, hipMemcpyDeviceToHost));
            if (memcmp(o256.data(), o64.data(), out_words * 4) != 0) {
                fprintf(stderr, "set %u field %d op %d: block sizes 256 and 64 disagree\n", s, field, ops[k]);
                disagreements++;
            }
            if (fwrite(o256.data(), 4, out_words, out) != out_words) {
                fprintf(stderr, "output write failed\n");
                return 4;
            }
        }
        CHECK(hipFree(dA));
        CHECK(hipFree(dB));
        CHECK(hipFree(dO));
    }
    fclose(in);
    if (fclose(out) != 0) return 4;
    printf("sets %u, block-size disagreements %d\n", n_sets, disagreements);
    return disagreements ? 5 : 0;
}
