"""The role permutation of the 16-stream paired kernel (alac.net_amd/csrc/alac_roles.h), checked on the host: a small C++ program
includes the header the kernel includes and walks turns 0..3 of pair_role_of_simd.  No GPU.

  - every workgroup uses each SIMD exactly once (its four SIMDs carry entropy, output, FIR 0 and FIR 1);
  - two consecutive turns never put two entropy waves on one SIMD;
  - four consecutive turns load every SIMD with one entropy, one output and two FIR waves;
  - two workgroups with turns 2 k and 2 k + 1 pair entropy with output and FIR with FIR, which no rotation does.
"""
import os
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "alac.net_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include "alac_roles.h"
int main() {
    int bad = 0;
    for (unsigned t = 0; t < 4; t++) {
        unsigned seen = 0;
        for (unsigned s = 0; s < 4; s++) {
            const int r = pair_role_of_simd(t, s);
            if (r < 0 || r > 3) { std::printf("turn %u simd %u: role %d\n", t, s, r); return 1; }
            seen |= 1u << r;
            if (pair_role_of_simd(t + 4, s) != r) { std::printf("turn %u: not modulo 4\n", t); bad++; }
            if (r == PAIR_ROLE_ENTROPY && pair_role_of_simd(t + 1, s) == PAIR_ROLE_ENTROPY) { std::printf("turns %u, %u: two entropy waves on SIMD %u\n", t, t + 1, s); bad++; }
        }
        if (seen != 15u) { std::printf("turn %u: roles %x\n", t, seen); bad++; }
    }
    for (unsigned t = 0; t < 4; t++)
        for (unsigned s = 0; s < 4; s++) {
            int count[4] = {0, 0, 0, 0};
            for (unsigned k = 0; k < 4; k++) count[pair_role_of_simd(t + k, s)]++;
            if (count[PAIR_ROLE_ENTROPY] != 1 || count[PAIR_ROLE_OUTPUT] != 1 || count[PAIR_ROLE_FIR0] + count[PAIR_ROLE_FIR1] != 2) {
                std::printf("turns %u..%u: SIMD %u carries %d entropy, %d output, %d FIR\n", t, t + 3, s, count[0], count[1], count[2] + count[3]);
                bad++;
            }
        }
    for (unsigned t = 0; t < 4; t += 2)
        for (unsigned s = 0; s < 4; s++) {
            const int a = pair_role_of_simd(t, s), b = pair_role_of_simd(t + 1, s);
            const bool light = (a == PAIR_ROLE_ENTROPY && b == PAIR_ROLE_OUTPUT) || (a == PAIR_ROLE_OUTPUT && b == PAIR_ROLE_ENTROPY) ||
                               (a >= PAIR_ROLE_FIR0 && b >= PAIR_ROLE_FIR0);
            if (!light) { std::printf("turns %u, %u: SIMD %u carries roles %d and %d\n", t, t + 1, s, a, b); bad++; }
        }
    std::printf("%s\n", bad ? "FAILED" : "ok");
    return bad != 0;
}
"""


def test_role_permutation(tmp_path):
    src, exe = tmp_path / "pair_roles.cpp", tmp_path / "pair_roles"
    src.write_text(PROGRAM)
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-I", CSRC, "-o", str(exe), str(src)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
