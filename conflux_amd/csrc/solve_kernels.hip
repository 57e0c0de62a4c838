// solve_kernels.hip — CDNA4 (gfx950) kernels of the multi-RHS solve
// (conflux_lu_solve / conflux_chol_solve): the getrs/potrs pair on the
// stored factors.  The reference has no solve; these kernels consume what
// its LU_rep leaves behind (C result buffer + perm,
// conflux_opt.hpp:1660-1754).
//
//   k_trsm_left_tri_mfma  X (v x N) <- T^-1 X for T lower/upper, unit/non-unit,
//                         any v >= 1, T read in place out of global F (ldt = N).
//   k_update_skinny       C (M x nrhs) -= A (M x K) B (K x nrhs), nrhs <= 16:
//                         the tall rank-v update of a sweep, bandwidth-bound
//                         (each element of F is read once per sweep).
//
// Neither kernel synchronises across blocks: every block owns its slice of
// X / C outright — no flags, no atomics, nothing that can spin.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "kernels.hpp"

typedef double f64x4 __attribute__((ext_vector_type(4)));

namespace ck {

// ---------------------------------------------------------------------------
// General left triangular solve.  Structure of k_trsm_left_mfma (kernels.hip):
// each block owns 128 columns of X, sweeps 32-row panels (forward for lower,
// BACKWARD for upper), rank-32 updates on v_mfma_f64_16x16x4_f64 out of
// double-buffered LDS, 32x32 diagonal solve as a register triangle (one
// thread per column).  32-blocks are aligned at row 0, so the ragged block
// (v % 32 != 0) is the last one — the FIRST one an upper sweep processes.
// It is identity-padded in LDS (diagonal 1, off-diagonal 0, X rows 0); the
// padding is never stored.  The half of T on the other side of the diagonal
// (and the diagonal itself when UNIT) is never read.
// ---------------------------------------------------------------------------
#define TRI_COLS 128
template <bool UPPER, bool UNIT>
__global__ __launch_bounds__(256) void k_trsm_left_tri_mfma(
    const double *__restrict__ T, int64_t ldt, double *__restrict__ X,
    int64_t ldx, int v, int64_t N) {
    __shared__ double sXj[32][TRI_COLS + 1];
    __shared__ double sXp[2][32][TRI_COLS + 1];  // double-buffered
    __shared__ double sT[2][32][33];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int frow = lane & 15, fk = lane >> 4;
    const int64_t c0 = (int64_t)blockIdx.x * TRI_COLS;
    const int cols = (int)min((int64_t)TRI_COLS, N - c0);
    const int nblk = (v + 31) / 32;
    double rx[16], rt[4];  // 32x128 X panel + 32x32 T block per iteration
    auto load_t_regs = [&](int pb, int jb) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + i * 256;
            const int gr = jb + (e >> 5), gc = pb + (e & 31);
            rt[i] = (gr < v && gc < v) ? T[(int64_t)gr * ldt + gc] : 0.0;
        }
    };
    auto load_x_regs = [&](int pb) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int e = tid + i * 256;
            const int gr = pb + (e >> 7), cc = e & (TRI_COLS - 1);
            rx[i] = (cc < cols && gr < v) ? X[(int64_t)gr * ldx + c0 + cc]
                                          : 0.0;
        }
    };
    auto write_bufs = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int e = tid + i * 256;
            sXp[buf][e >> 7][e & (TRI_COLS - 1)] = rx[i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + i * 256;
            sT[buf][e >> 5][e & 31] = rt[i];
        }
    };
    for (int it = 0; it < nblk; ++it) {
        const int jb = (UPPER ? nblk - 1 - it : it) * 32;
        // solved panels so far: `it` of them, below (lower) / above (upper)
        auto pb_of = [&](int i) { return UPPER ? jb + 32 * (i + 1) : 32 * i; };
        __syncthreads();
        for (int i = tid; i < 32 * TRI_COLS; i += 256) {
            const int gr = jb + (i >> 7), cc = i & (TRI_COLS - 1);
            if (cc < cols)
                sXj[i >> 7][cc] =
                    gr < v ? X[(int64_t)gr * ldx + c0 + cc] : 0.0;
        }
        int cur = 0;
        if (it > 0) {
            load_x_regs(pb_of(0));
            load_t_regs(pb_of(0), jb);
            write_bufs(0);
        }
        __syncthreads();  // also covers the sXj stage
        for (int p = 0; p < it; ++p) {
            if (p + 1 < it) {
                load_x_regs(pb_of(p + 1));
                load_t_regs(pb_of(p + 1), jb);
            }
            // sXj[32 x cols] -= sT[32 x 32] * sXp[32 x cols] on MFMA:
            // wave w owns cols [32w, 32w+32): 2 row-tiles x 2 col-tiles
            if (wave * 32 < cols) {
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) {
                    const int cbase = wave * 32 + ct * 16;
                    f64x4 acc[2] = {f64x4{0, 0, 0, 0}, f64x4{0, 0, 0, 0}};
#pragma unroll
                    for (int kk = 0; kk < 8; ++kk) {
                        const int k = kk * 4 + fk;
                        const double b = sXp[cur][k][cbase + frow];
#pragma unroll
                        for (int rt_ = 0; rt_ < 2; ++rt_)
                            acc[rt_] = __builtin_amdgcn_mfma_f64_16x16x4f64(
                                sT[cur][rt_ * 16 + frow][k], b, acc[rt_], 0,
                                0, 0);
                    }
#pragma unroll
                    for (int rt_ = 0; rt_ < 2; ++rt_)
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            sXj[rt_ * 16 + 4 * q + fk][cbase + frow] -=
                                acc[rt_][q];
                }
            }
            if (p + 1 < it) write_bufs(cur ^ 1);
            __syncthreads();
            cur ^= 1;
        }
        // diagonal block, masked to its triangle and identity-padded
        for (int i = tid; i < 32 * 32; i += 256) {
            const int r = i >> 5, c = i & 31;
            const int gr = jb + r, gc = jb + c;
            double t;
            if (r == c)
                t = (UNIT || gr >= v) ? 1.0 : T[(int64_t)gr * ldt + gc];
            else
                t = ((UPPER ? c > r : c < r) && gr < v && gc < v)
                        ? T[(int64_t)gr * ldt + gc]
                        : 0.0;
            sT[0][r][c] = t;
        }
        __syncthreads();
        if (tid < cols) {  // diagonal solve: thread = column
            double x[32];
#pragma unroll
            for (int r = 0; r < 32; ++r) x[r] = sXj[r][tid];
            if (UPPER) {
#pragma unroll
                for (int k = 31; k >= 0; --k) {
                    if (!UNIT) x[k] /= sT[0][k][k];
                    const double xk = x[k];
#pragma unroll
                    for (int r = 0; r < 32; ++r)
                        if (r < k) x[r] -= sT[0][r][k] * xk;
                }
            } else {
#pragma unroll
                for (int k = 0; k < 32; ++k) {
                    if (!UNIT) x[k] /= sT[0][k][k];
                    const double xk = x[k];
#pragma unroll
                    for (int r = 0; r < 32; ++r)
                        if (r > k) x[r] -= sT[0][r][k] * xk;
                }
            }
#pragma unroll
            for (int r = 0; r < 32; ++r) sXj[r][tid] = x[r];
        }
        __syncthreads();
        for (int i = tid; i < 32 * TRI_COLS; i += 256) {
            const int gr = jb + (i >> 7), cc = i & (TRI_COLS - 1);
            if (cc < cols && gr < v)
                X[(int64_t)gr * ldx + c0 + cc] = sXj[i >> 7][cc];
        }
    }
}

// ---------------------------------------------------------------------------
// Skinny update C (M x nrhs) -= A (M x K) * B (K x nrhs), 1 <= nrhs <= 16,
// K <= SKN_KMAX per launch.  One 16x16 MFMA tile per wave: 16 rows of A
// against the whole (zero-padded to 16 columns) B, which the block stages in
// LDS once.  A is a column panel of F (lda = N), so lanes walk ALONG k: lane
// (row = l & 15, fk = l >> 4) loads 4 consecutive doubles of its row per
// 16-wide k chunk — a wave reads 16 row segments of 128 contiguous bytes per
// chunk and 512 per 64-wide group.  The MFMA's k index is a free permutation
// as long as both operands agree: step (u, s) of a group multiplies
// A[row][g*64 + u*16 + fk*4 + s] with B[the same k][col].
// Waves grid-stride over 16-row tiles; each tile of C has one owner.
// ---------------------------------------------------------------------------
#define SKN_KMAX 512
#define SKN_RS 20  // sB row stride: rows 4 apart land 32 banks apart (b64)
template <bool FAST>  // FAST: K % 64 == 0, A 16-B aligned, lda even
__global__ __launch_bounds__(256) void k_update_skinny(
    const double *__restrict__ A, int64_t lda, const double *__restrict__ B,
    int64_t ldb, double *__restrict__ C, int64_t ldc, int M, int nrhs, int K) {
    __shared__ double sB[SKN_KMAX][SKN_RS];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int frow = lane & 15, fk = lane >> 4;
    const int ngrp = (K + 63) / 64;
    for (int i = tid; i < ngrp * 64 * 16; i += 256) {
        const int k = i >> 4, c = i & 15;
        sB[k][c] = (k < K && c < nrhs) ? B[(int64_t)k * ldb + c] : 0.0;
    }
    __syncthreads();
    const int ntiles = (M + 15) / 16;
    for (int t = blockIdx.x * 4 + wave; t < ntiles; t += gridDim.x * 4) {
        const int row = t * 16 + frow;
        // rows past M re-read row M-1 (in bounds); their results are dropped
        const double *ap = A + (int64_t)min(row, M - 1) * lda + fk * 4;
        double ra[2][4][4];  // [buffer][chunk u][s]
        auto load_group = [&](int g, int buf) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int k0 = g * 64 + u * 16;
                if (FAST) {
                    const double2 lo = *(const double2 *)(ap + k0);
                    const double2 hi = *(const double2 *)(ap + k0 + 2);
                    ra[buf][u][0] = lo.x;
                    ra[buf][u][1] = lo.y;
                    ra[buf][u][2] = hi.x;
                    ra[buf][u][3] = hi.y;
                } else {
#pragma unroll
                    for (int s = 0; s < 4; ++s)
                        ra[buf][u][s] =
                            (k0 + fk * 4 + s < K) ? ap[k0 + s] : 0.0;
                }
            }
        };
        f64x4 acc = {0, 0, 0, 0};
        load_group(0, 0);
        for (int g = 0; g < ngrp; g += 2) {
            // two groups per trip so the register buffers index statically
            if (g + 1 < ngrp) load_group(g + 1, 1);
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int s = 0; s < 4; ++s)
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(
                        ra[0][u][s], sB[g * 64 + u * 16 + fk * 4 + s][frow],
                        acc, 0, 0, 0);
            if (g + 1 < ngrp) {
                if (g + 2 < ngrp) load_group(g + 2, 0);
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int s = 0; s < 4; ++s)
                        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(
                            ra[1][u][s],
                            sB[(g + 1) * 64 + u * 16 + fk * 4 + s][frow], acc,
                            0, 0, 0);
            }
        }
        // f64 16x16x4 C/D map: lane l, reg q -> D[4*q + (l >> 4)][l & 15]
        if (frow < nrhs) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = t * 16 + 4 * q + fk;
                if (r < M) C[(int64_t)r * ldc + frow] -= acc[q];
            }
        }
    }
}

}  // namespace ck

using namespace ck;

void launch_trsm_left_tri_mfma(const double *T, int64_t ldt, double *X,
                               int64_t ldx, int v, int64_t N, int upper,
                               int unit, hipStream_t s) {
    if (N <= 0 || v <= 0) return;
    const dim3 grid((unsigned)((N + TRI_COLS - 1) / TRI_COLS)), block(256);
    if (upper && unit)
        hipLaunchKernelGGL((k_trsm_left_tri_mfma<true, true>), grid, block, 0,
                           s, T, ldt, X, ldx, v, N);
    else if (upper)
        hipLaunchKernelGGL((k_trsm_left_tri_mfma<true, false>), grid, block, 0,
                           s, T, ldt, X, ldx, v, N);
    else if (unit)
        hipLaunchKernelGGL((k_trsm_left_tri_mfma<false, true>), grid, block, 0,
                           s, T, ldt, X, ldx, v, N);
    else
        hipLaunchKernelGGL((k_trsm_left_tri_mfma<false, false>), grid, block,
                           0, s, T, ldt, X, ldx, v, N);
}

void launch_update_skinny(const double *A, int64_t lda, const double *B,
                          int64_t ldb, double *C, int64_t ldc, int M, int nrhs,
                          int K, hipStream_t s) {
    if (M <= 0 || nrhs <= 0 || nrhs > 16 || K <= 0) return;
    // one wave per 16-row tile, 4 waves per block; beyond 2048 blocks
    // (8 per CU) the waves grid-stride
    const int nblocks = std::min((M + 63) / 64, 2048);
    for (int k0 = 0; k0 < K; k0 += SKN_KMAX) {  // C -= is additive over K
        const int kc = std::min(SKN_KMAX, K - k0);
        const double *a = A + k0;
        const double *b = B + (int64_t)k0 * ldb;
        const bool fast = kc % 64 == 0 && lda % 2 == 0 &&
                          ((uintptr_t)a & 15) == 0;
        if (fast)
            hipLaunchKernelGGL(k_update_skinny<true>, dim3(nblocks), dim3(256),
                               0, s, a, lda, b, ldb, C, ldc, M, nrhs, kc);
        else
            hipLaunchKernelGGL(k_update_skinny<false>, dim3(nblocks),
                               dim3(256), 0, s, a, lda, b, ldb, C, ldc, M,
                               nrhs, kc);
    }
}
