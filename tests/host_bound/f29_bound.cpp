// f29_bound.cpp - TEST ONLY (host, g++): the radix-2^29 products of field29.cuh with LURK_F29_CHECK, on operands whose nine limbs
// all hold one value, for tests/test_f29_p1_bound.py.  A bound violation prints "F29 bound violated: ..." and aborts.
//
//   f29_bound <field 0|1|2> <mul|mul30|sqr30|dot2> <limb of a> <limb of b>
//
// Prints the nine result limbs.  dot2: the two-term row a * b + a * b through dot29_finish2.
#define LURK_F29_CHECK 1
#include "../../lurk_beta_amd/csrc/field29.cuh"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace lurk;

template <class P>
static int run(const char* op, uint32_t la, uint32_t lb) {
    F29<P> a, b, r;
    for (int i = 0; i < 9; i++) { a.l[i] = la; b.l[i] = lb; }
    if (!strcmp(op, "mul")) r = f29_mul<P>(a, b);
    else if (!strcmp(op, "mul30")) r = f29_mul30<P>(a, b);
    else if (!strcmp(op, "sqr30")) r = f29_sqr30<P>(a);
    else if (!strcmp(op, "dot2")) {
        Dot29<P> row;
        dot29_init<P>(row);
        dot29_mac<P>(row, a, b);
        dot29_mac<P>(row, a, b);
        r = dot29_finish2<P>(row);
    } else return 2;
    printf("p1 form %d:", (int)f29_p1_form<P>());
    for (int i = 0; i < 9; i++) printf(" %u", r.l[i]);
    printf("\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 5) return 2;
    setvbuf(stdout, nullptr, _IONBF, 0);  // the message must be out before abort()
    static_assert(F29_CHECKS_ACTIVE, "LURK_F29_CHECK is not active");
    const int field = atoi(argv[1]);
    const uint32_t la = (uint32_t)strtoul(argv[3], nullptr, 0), lb = (uint32_t)strtoul(argv[4], nullptr, 0);
    if (field == 0) return run<PallasFp>(argv[2], la, lb);
    if (field == 1) return run<PallasFq>(argv[2], la, lb);
    return run<Bn254Fr>(argv[2], la, lb);
}
