// Host driver of tests/test_dd_host.py: runs the compensated dot product of
// conflux_amd/csrc/dd.hpp on vectors read from a file.  No GPU code.
//
//   dd_host_main <file>
// file:   ncases, then per case: K, then K lines "a x" (hex floats)
// stdout: per case one line "<one accumulator> <4 strided accumulators,
//         merged>" (hex floats) — the second is the shape of the kernel's
//         cross-lane reduction
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dd.hpp"

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = std::fopen(argv[1], "r");
    if (!f) return 2;
    int ncases = 0;
    if (std::fscanf(f, "%d", &ncases) != 1) return 2;
    for (int t = 0; t < ncases; ++t) {
        int K = 0;
        if (std::fscanf(f, "%d", &K) != 1 || K <= 0) return 2;
        std::vector<double> a(K), x(K);
        char sa[64], sx[64];
        for (int k = 0; k < K; ++k) {
            if (std::fscanf(f, "%63s %63s", sa, sx) != 2) return 2;
            a[k] = std::strtod(sa, nullptr);
            x[k] = std::strtod(sx, nullptr);
        }
        dd::Acc one{0.0, 0.0};
        for (int k = 0; k < K; ++k) dd::add_product(one, a[k], x[k]);
        dd::Acc part[4] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}};
        for (int k = 0; k < K; ++k) dd::add_product(part[k & 3], a[k], x[k]);
        dd::merge(part[0], part[2]);
        dd::merge(part[1], part[3]);
        dd::merge(part[0], part[1]);
        std::printf("%a %a\n", dd::round(one), dd::round(part[0]));
    }
    std::fclose(f);
    return 0;
}
