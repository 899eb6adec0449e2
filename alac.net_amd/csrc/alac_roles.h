// alac_roles.h -- which wave of a 16-stream paired workgroup does what, by the SIMD it sits on and the workgroup's turn on its
// CU.  Plain constexpr C++ (no HIP): the kernel and a host-side check (tests/test_pair_roles.py) read the same function.
//
// A 16-stream workgroup has four working waves, one per SIMD: entropy, output and two FIR waves.  Two such workgroups share a CU
// at 4096 packets.  The two-pass kernels rotate the roles (entropy on SIMD k, output on k + 1, FIR on k + 2 and k + 3 at turn k):
// with two workgroups per CU that puts each entropy wave beside a FIR wave of the other workgroup.  The lightest worst case is
// entropy beside output on two SIMDs and FIR beside FIR on the other two, which no rotation gives.  This permutation does:
//   turn 0   E O F F        turn 2   F F E O
//   turn 1   O E F F        turn 3   F F O E
#ifndef ALAC_ROLES_H
#define ALAC_ROLES_H

enum { PAIR_ROLE_ENTROPY = 0, PAIR_ROLE_OUTPUT = 1, PAIR_ROLE_FIR0 = 2, PAIR_ROLE_FIR1 = 3 };

// the role of the wave on SIMD `simd` (0..3) of the workgroup whose turn on its CU is `turn` (any value: taken modulo 4)
constexpr int pair_role_of_simd(unsigned turn, unsigned simd) {
    return ((simd >> 1) & 1u) == ((turn >> 1) & 1u) ? ((simd & 1u) == (turn & 1u) ? PAIR_ROLE_ENTROPY : PAIR_ROLE_OUTPUT)
                                                    : PAIR_ROLE_FIR0 + (int)(simd & 1u);
}

namespace pair_roles_check {
// every workgroup uses each SIMD once: its four SIMDs carry the four roles
constexpr bool each_simd_once(unsigned turn) {
    unsigned seen = 0;
    for (unsigned s = 0; s < 4; s++) seen |= 1u << pair_role_of_simd(turn, s);
    return seen == 15u;
}
// two consecutive turns never put two entropy waves on one SIMD
constexpr bool entropy_apart(unsigned turn) {
    for (unsigned s = 0; s < 4; s++)
        if (pair_role_of_simd(turn, s) == PAIR_ROLE_ENTROPY && pair_role_of_simd(turn + 1, s) == PAIR_ROLE_ENTROPY) return false;
    return true;
}
// four consecutive turns load every SIMD with one entropy, one output and two FIR waves
constexpr bool four_turns_even(unsigned turn) {
    for (unsigned s = 0; s < 4; s++) {
        int e = 0, o = 0, f = 0;
        for (unsigned k = 0; k < 4; k++) {
            const int r = pair_role_of_simd(turn + k, s);
            e += r == PAIR_ROLE_ENTROPY;
            o += r == PAIR_ROLE_OUTPUT;
            f += r >= PAIR_ROLE_FIR0;
        }
        if (e != 1 || o != 1 || f != 2) return false;
    }
    return true;
}
constexpr bool all_turns() {
    for (unsigned t = 0; t < 4; t++)
        if (!each_simd_once(t) || !entropy_apart(t) || !four_turns_even(t)) return false;
    return true;
}
static_assert(all_turns(), "the paired workgroup's role permutation");
}  // namespace pair_roles_check

#endif
