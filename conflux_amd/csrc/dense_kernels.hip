// dense_kernels.hip — the device-resident dense interface (gfx950): a caller's
// dense n x n device matrix in and out of the engine's tile-cyclic rank
// buffers, right-hand sides in and out of the sweeps' contiguous buffer, and
// the log-determinant reduction over the stored diagonal.  The reference has
// no counterpart: its callers write lu_params::data on the host.
//
//   k_import_rowmajor<VEC>  dense row-major -> one rank's Ml x Nl buffer, the
//                           identity padding outside the leading n x n block
//                           written in the same pass.  VEC: 16-byte accesses
//                           along the contiguous v-long tile-row segments.
//   k_import_colmajor       the same from a column-major source: 32 x 32
//                           tiles of the DESTINATION transposed through LDS
//                           (pitch 33 doubles), so the global read runs along
//                           the source's contiguous index and the global
//                           write along the destination's.
//   k_export_rowmajor<VEC>  the inverse map, cropped to n.
//   k_rhs_stage_in / _out   B (n x nrhs, ldb) <-> X (N x nrhs), optionally
//                           through perm, zero tail in, crop out.
//   k_diag_gather           a rank's share of the leading n diagonal entries.
//   k_logdet_reduce         sum log|d_i| in doubled precision, fixed order.
//
// The owner map is the engine's (reference layout.cpp:95-123): local (lr, lc)
// of rank (pi, pj) is global ((lr / v * Px + pi) * v + lr % v, same in j).
// Every element offset is 64-bit (N^2 passes 2^31 at N = 65536); the flat
// kernels are grid-stride under the project's grid cap.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "dd.hpp"
#include "kernels.hpp"

namespace dk {

// element (gi, gj) of blockdiag(A, I)
__device__ __forceinline__ double pad_or_load(const double *__restrict__ dA,
                                              int64_t off, int64_t gi,
                                              int64_t gj, int n) {
    if (gi < n && gj < n) return dA[off];
    return gi == gj ? 1.0 : 0.0;
}

template <bool VEC>
__global__ void k_import_rowmajor(const double *__restrict__ dA, int64_t lda,
                                  int n, double *__restrict__ dst, int Ml,
                                  int Nl, int v, int Px, int Py, int pi,
                                  int pj) {
    constexpr int W = VEC ? 2 : 1;  // VEC: v even, so a pair stays in one tile
    const int64_t ncw = Nl / W;
    const int64_t total = (int64_t)Ml * ncw;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         idx < total; idx += stride) {
        const int lr = (int)(idx / ncw), lc = (int)(idx % ncw) * W;
        const int64_t gi = (int64_t)(lr / v * Px + pi) * v + lr % v;
        const int64_t gj = (int64_t)(lc / v * Py + pj) * v + lc % v;
        const int64_t so = gi * lda + gj, d_o = (int64_t)lr * Nl + lc;
        if (VEC) {
            double2 o;
            if (gi < n && gj + 1 < n) {
                o = *reinterpret_cast<const double2 *>(dA + so);
            } else {
                o.x = pad_or_load(dA, so, gi, gj, n);
                o.y = pad_or_load(dA, so + 1, gi, gj + 1, n);
            }
            *reinterpret_cast<double2 *>(dst + d_o) = o;
        } else {
            dst[d_o] = pad_or_load(dA, so, gi, gj, n);
        }
    }
}

// Column-major source: dA[gj * lda + gi].  A block owns a 32 x 32 tile of the
// destination (local coordinates, independent of v) per trip.  Load: lane x
// walks local ROWS, i.e. the source's contiguous index in runs of min(v, 32).
// Store: lane x walks local COLUMNS, contiguous in the destination.  LDS tile
// [col][row], pitch 33 doubles: the 8-byte store of a 16-lane group covers 32
// consecutive dwords (one bank each), and the 8-byte read of a 32-lane group
// sits at dword 2 * (33 x + y), 66 x mod 64 = 2 x: all 32 distinct.
#define DK_TT 32
__global__ __launch_bounds__(256) void k_import_colmajor(
    const double *__restrict__ dA, int64_t lda, int n,
    double *__restrict__ dst, int Ml, int Nl, int v, int Px, int Py, int pi,
    int pj) {
    __shared__ double tile[DK_TT][DK_TT + 1];
    const int x = threadIdx.x & 31, y = threadIdx.x >> 5;  // y in 0..7
    const int64_t tr = (Ml + DK_TT - 1) / DK_TT, tc = (Nl + DK_TT - 1) / DK_TT;
    for (int64_t t = blockIdx.x; t < tr * tc; t += gridDim.x) {
        const int lr0 = (int)(t / tc) * DK_TT, lc0 = (int)(t % tc) * DK_TT;
        const int lr = lr0 + x;
        const int64_t gi = (int64_t)(lr / v * Px + pi) * v + lr % v;
        for (int k = y; k < DK_TT; k += 8) {
            const int lc = lc0 + k;
            if (lr < Ml && lc < Nl) {
                const int64_t gj = (int64_t)(lc / v * Py + pj) * v + lc % v;
                tile[k][x] = pad_or_load(dA, gj * lda + gi, gi, gj, n);
            }
        }
        __syncthreads();
        for (int k = y; k < DK_TT; k += 8)
            if (lr0 + k < Ml && lc0 + x < Nl)
                dst[(int64_t)(lr0 + k) * Nl + lc0 + x] = tile[x][k];
        __syncthreads();
    }
}

template <bool VEC>
__global__ void k_export_rowmajor(const double *__restrict__ src, int Ml,
                                  int Nl, int v, int Px, int Py, int pi,
                                  int pj, double *__restrict__ dF, int64_t ldf,
                                  int n) {
    constexpr int W = VEC ? 2 : 1;
    const int64_t ncw = Nl / W;
    const int64_t total = (int64_t)Ml * ncw;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         idx < total; idx += stride) {
        const int lr = (int)(idx / ncw), lc = (int)(idx % ncw) * W;
        const int64_t gi = (int64_t)(lr / v * Px + pi) * v + lr % v;
        const int64_t gj = (int64_t)(lc / v * Py + pj) * v + lc % v;
        if (gi >= n || gj >= n) continue;
        const int64_t s_o = (int64_t)lr * Nl + lc, d_o = gi * ldf + gj;
        if (VEC && gj + 1 < n)
            *reinterpret_cast<double2 *>(dF + d_o) =
                *reinterpret_cast<const double2 *>(src + s_o);
        else
            dF[d_o] = src[s_o];
    }
}

// X (N x nrhs, ld = nrhs) row r <- B row (idx ? idx[r] : r) for r < n, zero
// below.  A source row outside B (a padding row pivoted into the leading
// block: singular input only) reads as zero instead of past the caller's
// buffer.
__global__ void k_rhs_stage_in(const double *__restrict__ B, int64_t ldb,
                               int n, const int *__restrict__ idx,
                               double *__restrict__ X, int64_t N, int nrhs) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < N * nrhs; i += stride) {
        const int64_t r = i / nrhs, c = i % nrhs;
        const int64_t s = (idx && r < n) ? idx[r] : r;
        X[i] = (r < n && s >= 0 && s < n) ? B[s * ldb + c] : 0.0;
    }
}

// B row (idx ? idx[r] : r) <- X row r, r < n only; rows that would land
// outside B are dropped (singular input only, as above).
__global__ void k_rhs_stage_out(const double *__restrict__ X, int nrhs, int n,
                                const int *__restrict__ idx,
                                double *__restrict__ B, int64_t ldb) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < (int64_t)n * nrhs; i += stride) {
        const int64_t r = i / nrhs, c = i % nrhs;
        const int64_t d = idx ? idx[r] : r;
        if (d >= 0 && d < n) B[d * ldb + c] = X[i];
    }
}

// out[g] = F[lr][lr] for the global diagonal indices g < n this rank owns
// (rank (p, p) of a Px x Px grid: diagonal tile t lives on p = t % Px)
__global__ void k_diag_gather(const double *__restrict__ F, int Ml, int Nl,
                              int v, int Px, int p, int n,
                              double *__restrict__ out) {
    const int stride = gridDim.x * blockDim.x;
    for (int lr = blockIdx.x * blockDim.x + threadIdx.x; lr < Ml;
         lr += stride) {
        const int64_t g = (int64_t)(lr / v * Px + p) * v + lr % v;
        if (g < n) out[g] = F[(int64_t)lr * Nl + lr];
    }
}

// out[0] = sum_i log|d_i| over the finite non-zero d_i, out[1] = how many
// d_i < 0, out[2] = 1 if some d_i == 0, + 2 if some d_i is not finite.
// One block: thread t takes i = t, t + 256, ... in order, the 256 partial
// sums merge in a fixed tree, so two calls agree bitwise.  The sum runs
// through dd.hpp's two_sum pairs and is rounded once: it adds no error that
// grows with n to the per-term rounding of log().
__global__ __launch_bounds__(256) void k_logdet_reduce(
    const double *__restrict__ d, int n, double *__restrict__ out) {
    __shared__ double ss[256], sc[256];
    __shared__ int sneg[256], sflag[256];
    const int tid = threadIdx.x;
    dd::Acc acc{0.0, 0.0};
    int neg = 0, flag = 0;
    for (int i = tid; i < n; i += 256) {
        const double x = d[i];
        if (x == 0.0) {
            flag |= 1;
        } else if (!isfinite(x)) {
            flag |= 2;
        } else {
            neg += x < 0.0;
            dd::merge(acc, dd::Acc{log(fabs(x)), 0.0});
        }
    }
    ss[tid] = acc.s;
    sc[tid] = acc.c;
    sneg[tid] = neg;
    sflag[tid] = flag;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) {
            dd::Acc a{ss[tid], sc[tid]};
            dd::merge(a, dd::Acc{ss[tid + w], sc[tid + w]});
            ss[tid] = a.s;
            sc[tid] = a.c;
            sneg[tid] += sneg[tid + w];
            sflag[tid] |= sflag[tid + w];
        }
        __syncthreads();
    }
    if (tid == 0) {
        out[0] = dd::round(dd::Acc{ss[0], sc[0]});
        out[1] = (double)sneg[0];
        out[2] = (double)sflag[0];
    }
}

static inline unsigned cap_grid(int64_t total, int per_block = 256) {
    int64_t g = (total + per_block - 1) / per_block;
    if (g > (1 << 22)) g = 1 << 22;  // grid-stride kernels cover the rest
    return (unsigned)(g < 1 ? 1 : g);
}

static inline bool aligned16(const void *p) {
    return (reinterpret_cast<uintptr_t>(p) & 15) == 0;
}

}  // namespace dk

using namespace dk;

void launch_dense_import(const double *dA, int64_t lda, int n, int order,
                         double *dst, int Ml, int Nl, int v, int Px, int Py,
                         int pi, int pj, hipStream_t s) {
    if (order == 1) {
        const int64_t tiles = (int64_t)((Ml + DK_TT - 1) / DK_TT) *
                              ((Nl + DK_TT - 1) / DK_TT);
        hipLaunchKernelGGL(k_import_colmajor, dim3(cap_grid(tiles, 1)),
                           dim3(256), 0, s, dA, lda, n, dst, Ml, Nl, v, Px, Py,
                           pi, pj);
        return;
    }
    const int64_t total = (int64_t)Ml * Nl;
    if (v % 2 == 0 && lda % 2 == 0 && aligned16(dA) && aligned16(dst))
        hipLaunchKernelGGL(k_import_rowmajor<true>, dim3(cap_grid(total / 2)),
                           dim3(256), 0, s, dA, lda, n, dst, Ml, Nl, v, Px, Py,
                           pi, pj);
    else
        hipLaunchKernelGGL(k_import_rowmajor<false>, dim3(cap_grid(total)),
                           dim3(256), 0, s, dA, lda, n, dst, Ml, Nl, v, Px, Py,
                           pi, pj);
}

void launch_dense_export(const double *src, int Ml, int Nl, int v, int Px,
                         int Py, int pi, int pj, double *dF, int64_t ldf,
                         int n, hipStream_t s) {
    const int64_t total = (int64_t)Ml * Nl;
    if (v % 2 == 0 && ldf % 2 == 0 && aligned16(dF) && aligned16(src))
        hipLaunchKernelGGL(k_export_rowmajor<true>, dim3(cap_grid(total / 2)),
                           dim3(256), 0, s, src, Ml, Nl, v, Px, Py, pi, pj, dF,
                           ldf, n);
    else
        hipLaunchKernelGGL(k_export_rowmajor<false>, dim3(cap_grid(total)),
                           dim3(256), 0, s, src, Ml, Nl, v, Px, Py, pi, pj, dF,
                           ldf, n);
}

void launch_rhs_stage_in(const double *B, int64_t ldb, int n, const int *idx,
                         double *X, int64_t N, int nrhs, hipStream_t s) {
    if (N <= 0 || nrhs <= 0) return;
    hipLaunchKernelGGL(k_rhs_stage_in, dim3(cap_grid(N * nrhs)), dim3(256), 0,
                       s, B, ldb, n, idx, X, N, nrhs);
}

void launch_rhs_stage_out(const double *X, int nrhs, int n, const int *idx,
                          double *B, int64_t ldb, hipStream_t s) {
    if (n <= 0 || nrhs <= 0) return;
    hipLaunchKernelGGL(k_rhs_stage_out, dim3(cap_grid((int64_t)n * nrhs)),
                       dim3(256), 0, s, X, nrhs, n, idx, B, ldb);
}

void launch_diag_gather(const double *F, int Ml, int Nl, int v, int Px, int p,
                        int n, double *out, hipStream_t s) {
    hipLaunchKernelGGL(k_diag_gather, dim3(cap_grid(Ml)), dim3(256), 0, s, F,
                       Ml, Nl, v, Px, p, n, out);
}

void launch_logdet_reduce(const double *d, int n, double *out3,
                          hipStream_t s) {
    hipLaunchKernelGGL(k_logdet_reduce, dim3(1), dim3(256), 0, s, d, n, out3);
}
