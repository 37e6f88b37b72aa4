// Host build of rray_amd/csrc/quartic.inc (the torus solver, compiled unchanged with the device qualifiers defined
// away) for tests/test_quartic_host.py.  Reads "a4 a3 a2 a1 a0" per line (hexadecimal floats) from stdin and prints
// the number of roots and the roots (hexadecimal floats) per line, in the solver's order.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#define __device__
#define __forceinline__ inline
using std::fabs;
using std::sqrt;
#include "../../rray_amd/csrc/quartic.inc"

int main() {
    char a[5][64];
    while (scanf("%63s %63s %63s %63s %63s", a[0], a[1], a[2], a[3], a[4]) == 5) {
        double c[5];
        for (int i = 0; i < 5; i++) c[i] = strtod(a[i], nullptr);
        const RqRoots r = rq_quartic(c[0], c[1], c[2], c[3], c[4]);
        printf("%d", r.n);
        for (int i = 0; i < r.n; i++) printf(" %a", r.v[i]);
        printf("\n");
    }
    return 0;
}
