// dd.hpp — compensated ("doubled") dot-product arithmetic, host and device.
//
// Ogita–Rump–Oishi Dot2: every product goes through an error-free two_prod,
// every addition through an error-free two_sum, and the rounding errors are
// collected in a second word.  The pair (s, c) carries the sum as if it had
// been accumulated in twice the working precision; round() rounds it once.
// For a length-n dot product
//     |round() - exact| <= u |exact| + gamma_n^2 sum|a_k x_k|,   u = 2^-53.
//
// CONTRACTION HAZARD.  hipcc compiles device code with -ffp-contract=fast,
// under which `s + p` directly after `p = a * x` becomes fma(a, x, s): one
// rounding instead of two, so the "error" two_sum then recovers belongs to
// a different operation and the transformation is silently no longer
// error-free (results stay plausible, the extra digits are gone).  Every
// function below therefore switches contraction off for its own body with
// `#pragma clang fp contract(off)`; the one fused operation that IS wanted
// (two_prod's residual) is an explicit fma() call, which the pragma does
// not touch.  The build's global flags stay as they are.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CONFLUX_HD __host__ __device__
#else
#define CONFLUX_HD
#endif

namespace dd {

// p + e == a * x exactly (barring over/underflow)
CONFLUX_HD inline void two_prod(double a, double x, double &p, double &e) {
#pragma clang fp contract(off)
    p = a * x;
    e = fma(a, x, -p);
}

// s + e == a + b exactly; Knuth's branch-free six-operation form
CONFLUX_HD inline void two_sum(double a, double b, double &s, double &e) {
#pragma clang fp contract(off)
    s = a + b;
    const double bb = s - a;
    const double aa = s - bb;
    const double db = b - bb;
    const double da = a - aa;
    e = da + db;
}

struct Acc {
    double s, c;  // running sum and the rounding errors it has shed so far
};

// acc += a * x
CONFLUX_HD inline void add_product(Acc &acc, double a, double x) {
#pragma clang fp contract(off)
    double p, e, t, q;
    two_prod(a, x, p, e);
    two_sum(acc.s, p, t, q);
    acc.s = t;
    acc.c = acc.c + (e + q);
}

// acc += other: combines partial accumulators (cross-lane, cross-wave).
// Symmetric in its operands — two_sum and the error add both commute — so a
// butterfly in which partners merge in opposite order agrees on every lane.
CONFLUX_HD inline void merge(Acc &acc, const Acc &other) {
#pragma clang fp contract(off)
    double t, q;
    two_sum(acc.s, other.s, t, q);
    acc.s = t;
    acc.c = (acc.c + other.c) + q;
}

// the single rounding
CONFLUX_HD inline double round(const Acc &acc) {
#pragma clang fp contract(off)
    return acc.s + acc.c;
}

}  // namespace dd
