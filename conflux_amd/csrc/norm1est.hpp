// norm1est.hpp — Higham's 1-norm estimator (Hager's method as refined in
// N. J. Higham, "FORTRAN codes for estimating the one-norm of a real or
// complex matrix", ACM TOMS 14 (1988); the iteration LAPACK ships as dlacn2)
// for the condition estimates conflux_lu_rcond / conflux_chol_rcond.  The
// reference has no counterpart (it has no solve at all).
//
// Host-only and header-only.  The matrix M whose 1-norm is estimated (here
// an inverse) is given by two callbacks on host vectors of length n:
//     solve(x):    x <- M x
//     solve_t(x):  x <- M^T x
// The O(n) steps between them — sign vector, 1-norm, argmax — run here in
// one fixed sequential order, so the result is a pure function of what the
// callbacks return.  The estimate is a LOWER bound on ||M||1, almost always
// within a factor 3 and usually exact.  ||M||inf = ||M^T||1: swap the two
// callbacks.
//
//   x = 1/n;  x <- M x;  est = ||x||1;  xi = sign(x);  x <- M^T xi
//   repeat (at most 5 rounds in all):
//     j = first argmax |x|;  x = e_j;  x <- M x;  est_old = est; est = ||x||1
//     stop if sign(x) == xi (a repeated sign vector) or est <= est_old
//     xi = sign(x);  x <- M^T xi
//     stop if x[j_old] == max|x| (the same column would be chosen again)
//   safeguard: x_i = (-1)^i (1 + i/(n-1));  x <- M x;
//              est = max(est, 2 ||x||1 / (3 n))
// At most 2 + 2*4 + 1 = 11 applications.
#pragma once

#include <cmath>
#include <vector>

namespace norm1est {

struct Result {
    double est;   // the estimate of ||M||1 (may be non-finite if M is)
    int nsolves;  // callback applications used
};

template <typename Solve, typename SolveT>
Result estimate(int n, Solve &&solve, SolveT &&solve_t) {
    constexpr int ITMAX = 5;
    Result res{0.0, 0};
    if (n <= 0) return res;
    std::vector<double> x(n, 1.0 / n);
    std::vector<int> isgn(n);
    auto asum = [&]() {
        double s = 0;
        for (int i = 0; i < n; ++i) s += std::fabs(x[i]);
        return s;
    };
    auto first_argmax = [&]() {
        int j = 0;
        for (int i = 1; i < n; ++i)
            if (std::fabs(x[i]) > std::fabs(x[j])) j = i;
        return j;
    };
    auto apply_signs = [&]() {
        for (int i = 0; i < n; ++i) {
            isgn[i] = x[i] > 0 ? 1 : -1;
            x[i] = isgn[i];
        }
    };
    solve(x.data());
    ++res.nsolves;
    if (n == 1) {
        res.est = std::fabs(x[0]);
        return res;
    }
    double est = asum();
    apply_signs();
    solve_t(x.data());
    ++res.nsolves;
    int j = first_argmax();
    for (int iter = 2;; ++iter) {
        for (int i = 0; i < n; ++i) x[i] = 0.0;
        x[j] = 1.0;
        solve(x.data());
        ++res.nsolves;
        const double est_old = est;
        est = asum();
        bool repeated = true;
        for (int i = 0; i < n; ++i)
            if ((x[i] > 0 ? 1 : -1) != isgn[i]) {
                repeated = false;
                break;
            }
        if (repeated || est <= est_old) break;
        apply_signs();
        solve_t(x.data());
        ++res.nsolves;
        const int jlast = j;
        j = first_argmax();
        if (x[jlast] == std::fabs(x[j]) || iter >= ITMAX) break;
    }
    double alt = 1.0;
    for (int i = 0; i < n; ++i) {
        x[i] = alt * (1.0 + double(i) / double(n - 1));
        alt = -alt;
    }
    solve(x.data());
    ++res.nsolves;
    const double temp = 2.0 * (asum() / (3.0 * n));
    if (temp > est) est = temp;
    res.est = est;
    return res;
}

// rcond = 1 / (||A|| * est||A^-1||); 0 when ||A|| is 0 or not finite, or the
// estimate is 0 or not finite (a zero pivot), never an error.
inline double rcond_from(double anorm, double est_inv) {
    if (!(anorm > 0) || !std::isfinite(anorm)) return 0.0;
    if (!(est_inv > 0) || !std::isfinite(est_inv)) return 0.0;
    return (1.0 / est_inv) / anorm;
}

}  // namespace norm1est
