// Host driver of tests/test_norm1est_host.py: runs the 1-norm estimator of
// conflux_amd/csrc/norm1est.hpp with host callbacks on matrices read from a
// file.  No GPU code.
//
//   norm1est_host_main <file>
// file:   binary; int32 ncases, then per case int32 n and n*n doubles
//         (row-major)
// stdout: per case one line "<est ||A^-1||1> <nsolves> <est ||A^-1||inf>
//         <nsolves>" (hex floats, decimal counts); then one last line: the
//         rcond that rcond_from gives for callbacks that return inf.
//
// The matrix is factored here by a few-line partial-pivot elimination
// (PA = LU in place); solve applies A^-1, solve_t applies A^-T.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <utility>
#include <vector>

#include "norm1est.hpp"

struct Lu {
    int n;
    std::vector<double> f;  // L (unit, strict lower) and U
    std::vector<int> perm;  // row r of PA is row perm[r] of A
    std::vector<double> t;
    explicit Lu(int n_, std::vector<double> a)
        : n(n_), f(std::move(a)), perm(n_), t(n_) {
        for (int i = 0; i < n; ++i) perm[i] = i;
        for (int k = 0; k < n; ++k) {
            int p = k;
            for (int i = k + 1; i < n; ++i)
                if (std::fabs(f[i * n + k]) > std::fabs(f[p * n + k])) p = i;
            if (p != k) {
                for (int j = 0; j < n; ++j)
                    std::swap(f[k * n + j], f[p * n + j]);
                std::swap(perm[k], perm[p]);
            }
            for (int i = k + 1; i < n; ++i) {
                const double l = f[i * n + k] /= f[k * n + k];
                for (int j = k + 1; j < n; ++j) f[i * n + j] -= l * f[k * n + j];
            }
        }
    }
    void solve(double *x) {  // x <- A^-1 x: L U x = P b
        for (int i = 0; i < n; ++i) t[i] = x[perm[i]];
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < i; ++j) t[i] -= f[i * n + j] * t[j];
        for (int i = n - 1; i >= 0; --i) {
            for (int j = i + 1; j < n; ++j) t[i] -= f[i * n + j] * t[j];
            t[i] /= f[i * n + i];
        }
        for (int i = 0; i < n; ++i) x[i] = t[i];
    }
    void solve_t(double *x) {  // x <- A^-T x: U^T L^T P x = b
        for (int i = 0; i < n; ++i) t[i] = x[i];
        for (int i = 0; i < n; ++i) {
            for (int j = 0; j < i; ++j) t[i] -= f[j * n + i] * t[j];
            t[i] /= f[i * n + i];
        }
        for (int i = n - 1; i >= 0; --i)
            for (int j = i + 1; j < n; ++j) t[i] -= f[j * n + i] * t[j];
        for (int i = 0; i < n; ++i) x[perm[i]] = t[i];
    }
};

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t ncases = 0;
    if (std::fread(&ncases, 4, 1, f) != 1) return 2;
    for (int c = 0; c < ncases; ++c) {
        int32_t n = 0;
        if (std::fread(&n, 4, 1, f) != 1 || n <= 0) return 2;
        std::vector<double> a((size_t)n * n);
        if (std::fread(a.data(), 8, a.size(), f) != a.size()) return 2;
        Lu lu(n, std::move(a));
        auto s = [&](double *x) { lu.solve(x); };
        auto st = [&](double *x) { lu.solve_t(x); };
        const norm1est::Result one = norm1est::estimate(n, s, st);
        const norm1est::Result inf = norm1est::estimate(n, st, s);
        std::printf("%a %d %a %d\n", one.est, one.nsolves, inf.est,
                    inf.nsolves);
    }
    std::fclose(f);
    const int n = 8;
    auto blow = [&](double *x) {
        for (int i = 0; i < n; ++i) x[i] = std::numeric_limits<double>::infinity();
    };
    const norm1est::Result r = norm1est::estimate(n, blow, blow);
    std::printf("%a %d\n", norm1est::rcond_from(1.0, r.est), r.nsolves);
    return 0;
}
