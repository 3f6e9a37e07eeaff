// Prints what cheb_coefficients (control_amd/csrc/chebyshev.hpp) returns, as the 64-bit words of
// the doubles.  Arguments: groups of `its emin emax eimag`, the three doubles as 16 hex digits of
// their words.  Per group one line: "scale" and 3 (its - 1) words c1 c2 c3 of the steps 2 .. its.
// The header needs nothing of HIP: this file is compiled without its include path.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../control_amd/csrc/chebyshev.hpp"

static double from_word(const char *hex) {
    const uint64_t w = std::strtoull(hex, nullptr, 16);
    double d;
    std::memcpy(&d, &w, sizeof d);
    return d;
}
static void put(double d) {
    uint64_t w;
    std::memcpy(&w, &d, sizeof w);
    std::printf(" %016" PRIx64, w);
}

int main(int argc, char **argv) {
    if (argc < 5 || (argc - 1) % 4 != 0) {
        std::fprintf(stderr, "usage: cheb_coefficients (its emin emax eimag)...\n");
        return 2;
    }
    for (int a = 1; a + 3 < argc; a += 4) {
        const int its = std::atoi(argv[a]);
        const kkt::ChebCoefficients c = kkt::cheb_coefficients(
            its, from_word(argv[a + 1]), from_word(argv[a + 2]), from_word(argv[a + 3]));
        if ((int)c.steps.size() != (its > 1 ? its - 1 : 0)) return 3;
        std::printf("coef");
        put(c.scale);
        for (int s = 2; s <= its; ++s) {
            put(c.step(s).c1);
            put(c.step(s).c2);
            put(c.step(s).c3);
        }
        std::printf("\n");
    }
    return 0;
}
