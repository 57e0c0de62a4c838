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
// of the transposed solve (conflux_lu_solve_trans, A^T X = B on the same
// factors, read in place — no transposed copy of F):
//
//   k_trsm_left_tri_mfma<.., TRANS>   X <- T^-T X on the stored T.
//   k_update_skinny_t     C (M x nc) -= A^T B, A a K x M row panel of F,
//                         nc <= 16; the launcher loops over 16-column groups.
//   k_col_abs_sums        ||A||1 for the condition estimate.
//
// and of the refined solves (conflux_lu_solve_refined /
// conflux_chol_solve_refined), which the reference has no counterpart of
// either:
//
//   k_residual_dd         R (M x nrhs) = B - A (M x K) X (K x nrhs) with a
//                         doubled-precision accumulator (dd.hpp), one
//                         rounding per entry; vector ALU, bandwidth-bound.
//   k_residual_dd_t_part / _finish
//                         R (K x nrhs) = B - A^T X on the same stored A: the
//                         reduction over rows split across waves and blocks,
//                         partials merged in an order fixed by indices.
//   k_row_abs_sums, k_colmax_abs, k_axpy_masked
//                         ||A||inf, per-column max|.| and the masked X += D
//                         of the refinement loop.
//
// No kernel synchronises across blocks: every block owns its slice of
// X / C / R outright — no flags, no atomics, nothing that can spin — and
// every reduction runs in a fixed order, so results are deterministic.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "dd.hpp"
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
//
// TRANS solves T^T X = B on the same stored T: S = T^T is the opposite
// triangle, so the sweep runs in the opposite direction (SUP below).  The
// 32x32 blocks of T are still loaded along their STORED rows (coalesced) and
// transposed on the way into LDS (sT's rows are padded to 33 doubles, so the
// transposed writes spread over the banks); everything downstream of LDS is
// unchanged.
// ---------------------------------------------------------------------------
#define TRI_COLS 128
template <bool UPPER, bool UNIT, bool TRANS = false>
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
    constexpr bool SUP = UPPER != TRANS;  // the triangle of the solved system
    double rx[16], rt[4];  // 32x128 X panel + 32x32 T block per iteration
    // block (rows jb.., columns pb..) of the solved system; TRANS: that is
    // stored block (rows pb.., columns jb..), read along its stored rows
    auto load_t_regs = [&](int pb, int jb) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + i * 256;
            const int gr = (TRANS ? pb : jb) + (e >> 5);
            const int gc = (TRANS ? jb : pb) + (e & 31);
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
            if (TRANS)
                sT[buf][e & 31][e >> 5] = rt[i];
            else
                sT[buf][e >> 5][e & 31] = rt[i];
        }
    };
    for (int it = 0; it < nblk; ++it) {
        const int jb = (SUP ? nblk - 1 - it : it) * 32;
        // solved panels so far: `it` of them, below (lower) / above (upper)
        auto pb_of = [&](int i) { return SUP ? jb + 32 * (i + 1) : 32 * i; };
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
            // (r, c) in the solved system; TRANS walks c slowest so that
            // consecutive threads still read one stored row of T
            const int r = TRANS ? i & 31 : i >> 5, c = TRANS ? i >> 5 : i & 31;
            const int gr = jb + r, gc = jb + c;
            const int64_t at =
                TRANS ? (int64_t)gc * ldt + gr : (int64_t)gr * ldt + gc;
            double t;
            if (r == c)
                t = (UNIT || gr >= v) ? 1.0 : T[at];
            else
                t = ((SUP ? c > r : c < r) && gr < v && gc < v) ? T[at] : 0.0;
            sT[0][r][c] = t;
        }
        __syncthreads();
        if (tid < cols) {  // diagonal solve: thread = column
            double x[32];
#pragma unroll
            for (int r = 0; r < 32; ++r) x[r] = sXj[r][tid];
            if (SUP) {
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

// ---------------------------------------------------------------------------
// Transposed skinny update C (M x nc) -= A^T B with A stored K x M — a ROW
// panel of F (lda = ldf), the update of the A^T X = B sweeps — B (K x nc),
// 1 <= nc <= 16, K <= SKN_KMAX per launch.  Same tiling as k_update_skinny:
// one 16x16 MFMA tile per wave, B staged (zero-padded to 16 columns) in LDS
// once per block, waves grid-stride over 16-row tiles of C, one owner each.
// The MFMA A operand [row i][k] is F[k][i], so here the lanes walk ACROSS the
// stored row: lane (i = l & 15, fk = l >> 4) loads A[k][16 t + i] for
// k = 4 kk + fk — the 16 lanes of a k read 128 contiguous bytes of one stored
// row, a wave 4 such rows per load.  Any k order serves the global loads
// equally, so the steps use k_update_skinny's: step (u, s) of a group takes
// k = g*64 + u*16 + fk*4 + s for both operands, which keeps the sB reads of
// the four fk groups 4 rows (32 banks) apart.  Loads run one 64-deep k group
// (16 per lane) ahead of the MFMAs in a second register buffer.
// FULL: K % 64 == 0, no k bound checks.  Columns past M re-read column M-1
// (in bounds); their results are dropped.  Rows k >= K are never read.
// The compiler's resource usage (-Rpass-analysis=kernel-resource-usage),
// FULL / not: 248 / 250 VGPRs, 2 / 1 waves per SIMD, no spill, no scratch.
// The 80 KiB of sB cap a CU at two blocks (2 waves per SIMD) anyway, as for
// k_update_skinny, so FULL — what the sweeps launch whenever 64 | sb — loses
// nothing to its registers.
// ---------------------------------------------------------------------------
template <bool FULL>
__global__ __launch_bounds__(256) void k_update_skinny_t(
    const double *__restrict__ A, int64_t lda, const double *__restrict__ B,
    int64_t ldb, double *__restrict__ C, int64_t ldc, int M, int nc, int K) {
    __shared__ double sB[SKN_KMAX][SKN_RS];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int frow = lane & 15, fk = lane >> 4;
    const int ngrp = (K + 63) / 64;
    for (int i = tid; i < ngrp * 64 * 16; i += 256) {
        const int k = i >> 4, c = i & 15;
        sB[k][c] = (k < K && c < nc) ? B[(int64_t)k * ldb + c] : 0.0;
    }
    __syncthreads();
    const int ntiles = (M + 15) / 16;
    for (int t = blockIdx.x * 4 + wave; t < ntiles; t += gridDim.x * 4) {
        const double *ap = A + min(t * 16 + frow, M - 1);
        double ra[2][4][4];  // [buffer][chunk u][s]
        auto load_group = [&](int g, int buf) {
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const int k = g * 64 + u * 16 + fk * 4 + s;
                    ra[buf][u][s] =
                        (FULL || k < K) ? ap[(int64_t)k * lda] : 0.0;
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
        if (frow < nc) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = t * 16 + 4 * q + fk;
                if (r < M) C[(int64_t)r * ldc + frow] -= acc[q];
            }
        }
    }
}

// ---------------------------------------------------------------------------
// Extra-precise residual R (M x nrhs) = B - A (M x K) X (K x nrhs): every
// product and every addition goes through the doubled accumulator of dd.hpp,
// B enters as the accumulator's initial value, and each entry is rounded
// exactly once, at the end.  MFMA cannot do this (it rounds per step), so
// the work is on the vector ALU: 10 fp64 operations per (element of A,
// column).
//
// Work split.  A wave owns RES_R = 4 rows outright and all of K; its 64
// lanes walk ALONG k, lane l taking the 16-byte pair k = 128 * step + 2 l —
// a wave reads 1 KiB contiguous per row and step (k_update_skinny's access
// pattern, one row segment per wave instead of 16).  The block (4 waves,
// 16 rows) stages X through LDS in RES_KC-deep chunks, column-major, so the
// lanes' 16-byte LDS reads are contiguous and conflict-free and one X pair
// is reused by the 4 rows.  M = 16384 gives 4096 waves, 4 per SIMD.  K is
// NOT split across waves or blocks: the only cross-thread combination is
// the 64-lane merge butterfly at the end of a row, whose order is fixed by
// the lane ids, so R does not depend on the grid or on scheduling.
//
// Column group.  A launch handles NC <= RES_G = 4 columns in one pass over
// A (a template parameter: the single-RHS pass must not pay for padding
// columns); the launcher loops over groups.  4 rows x 4 columns of (s, c)
// accumulators are 64 VGPRs, the double-buffered A pairs 32 and one X pair
// 4.  The compiler's resource usage (-Rpass-analysis=kernel-resource-usage)
// for NC = 1 / 2 / 3 / 4: 88 / 106 / 120 / 138 VGPRs, 5 / 4 / 4 / 3 waves
// per SIMD, no VGPR or SGPR spill, no scratch.  8 columns would need 128
// VGPRs for accumulators alone and halve the occupancy, to no gain: a pass
// is already ALU-bound at 4 columns (10 * 4 operations per 8 bytes of A;
// measured at 16384^2: 0.40 ms at NC = 1, the speed of the memory, 0.85 ms
// at NC = 4).
//
// FAST: A 16-byte aligned and lda even, so every lane's pair is one 16-byte
// load; otherwise (and for the last odd element of a row) scalar loads.
// Elements at k >= K are never read: they enter as exact zeros.  Rows past
// M re-read row M-1 (in bounds) and their results are dropped, so all four
// waves reach every barrier.
// ---------------------------------------------------------------------------
#define RES_G 4
#define RES_R 4
#define RES_KC 1024
template <int NC, bool FAST>
__global__ __launch_bounds__(256) void k_residual_dd(
    const double *__restrict__ A, int64_t lda, const double *__restrict__ X,
    const double *__restrict__ B, double *__restrict__ R, int M, int K,
    int nrhs, int c0) {
    __shared__ double sX[NC][RES_KC];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int row0 = (blockIdx.x * 4 + wave) * RES_R;
    const double *ap[RES_R];
    dd::Acc acc[RES_R][NC];
#pragma unroll
    for (int r = 0; r < RES_R; ++r) {
        const int row = min(row0 + r, M - 1);
        ap[r] = A + (int64_t)row * lda;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            acc[r][c].s = lane == 0 ? B[(int64_t)row * nrhs + c0 + c] : 0.0;
            acc[r][c].c = 0.0;
        }
    }
    double ra[2][RES_R][2];  // [buffer][row][element of the pair]
    auto load_step = [&](int st, int buf) {
        const int k = st * 128 + lane * 2;
#pragma unroll
        for (int r = 0; r < RES_R; ++r) {
            if (FAST && k + 1 < K) {
                const double2 v = *(const double2 *)(ap[r] + k);
                ra[buf][r][0] = v.x;
                ra[buf][r][1] = v.y;
            } else {
                ra[buf][r][0] = k < K ? ap[r][k] : 0.0;
                ra[buf][r][1] = k + 1 < K ? ap[r][k + 1] : 0.0;
            }
        }
    };
    auto consume = [&](int st, int buf) {
        const int kl = (st * 128 + lane * 2) & (RES_KC - 1);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const double2 x = *(const double2 *)&sX[c][kl];
#pragma unroll
            for (int r = 0; r < RES_R; ++r) {
                dd::add_product(acc[r][c], -ra[buf][r][0], x.x);
                dd::add_product(acc[r][c], -ra[buf][r][1], x.y);
            }
        }
    };
    constexpr int SPC = RES_KC / 128;  // steps per chunk (even)
    const int nsteps = (K + 127) / 128;
    load_step(0, 0);
    for (int st = 0; st < nsteps; st += 2) {
        // two steps per trip so the register buffers index statically
        if (st % SPC == 0) {
            const int kc = st * 128;
            __syncthreads();  // the previous chunk is consumed
            for (int i = tid; i < NC * RES_KC; i += 256) {
                const int c = i % NC, k = i / NC;
                sX[c][k] = (kc + k < K)
                               ? X[(int64_t)(kc + k) * nrhs + c0 + c]
                               : 0.0;
            }
            __syncthreads();
        }
        if (st + 1 < nsteps) load_step(st + 1, 1);
        consume(st, 0);
        if (st + 1 < nsteps) {
            if (st + 2 < nsteps) load_step(st + 2, 0);
            consume(st + 1, 1);
        }
    }
    // 64-lane butterfly; merge is symmetric, so every lane ends with the
    // same pair and the order is a function of the lane ids alone
#pragma unroll
    for (int r = 0; r < RES_R; ++r)
#pragma unroll
        for (int c = 0; c < NC; ++c) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                dd::Acc o;
                o.s = __shfl_xor(acc[r][c].s, off);
                o.c = __shfl_xor(acc[r][c].c, off);
                dd::merge(acc[r][c], o);
            }
            if (lane == 0 && row0 + r < M)
                R[(int64_t)(row0 + r) * nrhs + c0 + c] =
                    dd::round(acc[r][c]);
        }
}

// ---------------------------------------------------------------------------
// Transposed extra-precise residual R (K x nrhs) = B - A^T X, A stored M x K
// and read IN PLACE along its stored rows (no transposed copy), X (M x nrhs):
//     R[j][c] = round(B[j][c] - sum_i A[i][j] X[i][c]),
// every product and addition through dd.hpp, one rounding per entry — the
// residual of the refined A^T X = B solve.  k_residual_dd cannot serve: it
// reduces along a stored row, across lanes; here the reduction runs DOWN the
// rows and each lane owns output entries.
//
// Work split, two kernels.
//   k_residual_dd_t_part   a block owns RT_W = 128 columns x RT_CH = 256 rows
//       of A.  Lane l of every wave owns the column pair j = 128 strip + 2 l
//       (one 16-byte load per row; a wave reads 1 KiB contiguous per row) and
//       accumulates its two columns in registers; wave w takes the rows
//       16 t + 4 w + u (u < 4) of the chunk, four rows per step, the next
//       step's loads issued before the current one is consumed.  X[i][c] is
//       the same for all lanes of a wave: the row index is built from
//       readfirstlane(wave), so the compiler fetches it with scalar loads
//       into SGPRs (checked in the ISA: one s_load_dwordx2 per row and
//       column, no vector load of X).
//       One lane per column pair alone would give K / 128 waves — 128 at
//       16384 — hence the split of the reduction over waves and blocks:
//       16384^2 gives 128 x 64 blocks, 32768 waves.
//       The four waves' partial (s, c) pairs meet in LDS and wave 0 writes
//       the block's partial to the workspace W[chunk][column][j].
//   k_residual_dd_t_finish one thread per (j, column): B[j][c] is the
//       accumulator's initial value, the chunks' partials are merged into it
//       and the pair is rounded once.
// Workspace: ceil(M / 256) x min(nrhs, RES_G) x K pairs of doubles —
// 1 / 16 of A's bytes per column at most, written once and read once.
//
// WHAT FIXES THE MERGE ORDER.  Nothing but indices: a lane adds its rows in
// ascending row order; wave 0 merges the waves' pairs as ((w0 + w1) + w2) +
// w3 after a barrier; the finish thread merges the chunks as (((B + p0) +
// p1) + ...) in ascending chunk index, after the part kernel has completed
// (stream order).  Every partial has exactly one writer and is complete
// before it is read; there are no atomics and no flags, so neither the
// grid's scheduling nor the launch width can change a bit, and two calls
// agree bitwise.  A column's arithmetic does not involve the other columns
// of its group, so its bits do not depend on nrhs or on the group it is in.
//
// Column group: RES_G = 4, as for k_residual_dd, for the same reason — a
// pass is ALU-bound at 4 columns (10 * 4 operations per 8 bytes of A), so a
// wider group buys no bandwidth and costs registers (measured at 16384^2:
// 0.37 ms at NC = 1, the speed of the memory and 0.89 x k_residual_dd's
// pass of the same run; 0.57 ms at NC = 4).  The compiler's
// resource usage (-Rpass-analysis=kernel-resource-usage) of the part kernel
// for NC = 1 / 2 / 3 / 4, FAST and scalar path alike: 64 / 80 / 96 / 114
// VGPRs, 8 / 6 / 5 / 4 waves per SIMD, 6 / 12 / 18 / 24 KiB of LDS per
// block, no VGPR or SGPR spill, no scratch (two accumulator pairs per column
// instead of k_residual_dd's four, hence more waves than its 5 / 4 / 4 /
// 3).  The finish kernel: 58 VGPRs, 8 waves, no LDS, no scratch.
//
// FAST: A 16-byte aligned and lda even, so every lane's pair is one 16-byte
// load; otherwise, and for the last column of an odd K, scalar loads.
// Bounds: columns j >= K and rows i >= M are never read (a lane without a
// column accumulates zeros and stores nothing; a row past M is skipped by a
// wave-uniform branch, so X is not read there either); W and R are written
// inside K only.  All four waves reach the one barrier.
// ---------------------------------------------------------------------------
#define RT_CH 256
#define RT_W 128
template <int NC, bool FAST>
__global__ __launch_bounds__(256) void k_residual_dd_t_part(
    const double *__restrict__ A, int64_t lda, const double *__restrict__ X,
    double2 *__restrict__ W, int M, int K, int nrhs, int c0) {
    __shared__ double2 sP[3][NC][RT_W];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j0 = blockIdx.x * RT_W + lane * 2;
    const int r0 = blockIdx.y * RT_CH;
    const int rend = min(r0 + RT_CH, M);
    dd::Acc acc[2][NC];
#pragma unroll
    for (int c = 0; c < NC; ++c)
        acc[0][c] = acc[1][c] = dd::Acc{0.0, 0.0};
    double ra[2][4][2];   // [buffer][row u][element of the pair]
    double rx[2][4][NC];  // wave-uniform: SGPRs
    auto load_step = [&](int st, int buf) {
        const int rb = r0 + st * 16 + wave * 4;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int row = rb + u;
            ra[buf][u][0] = ra[buf][u][1] = 0.0;
            if (row < rend) {  // wave-uniform
                const double *ap = A + (int64_t)row * lda + j0;
                if (FAST && j0 + 1 < K) {
                    const double2 v = *(const double2 *)ap;
                    ra[buf][u][0] = v.x;
                    ra[buf][u][1] = v.y;
                } else {
                    if (j0 < K) ra[buf][u][0] = ap[0];
                    if (j0 + 1 < K) ra[buf][u][1] = ap[1];
                }
#pragma unroll
                for (int c = 0; c < NC; ++c)
                    rx[buf][u][c] = X[(int64_t)row * nrhs + c0 + c];
            }
        }
    };
    auto consume = [&](int st, int buf) {
        const int rb = r0 + st * 16 + wave * 4;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (rb + u < rend) {  // wave-uniform
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    dd::add_product(acc[0][c], -ra[buf][u][0], rx[buf][u][c]);
                    dd::add_product(acc[1][c], -ra[buf][u][1], rx[buf][u][c]);
                }
            }
        }
    };
    const int nsteps = (rend - r0 + 15) / 16;
    load_step(0, 0);
    for (int st = 0; st < nsteps; st += 2) {
        // two steps per trip so the register buffers index statically
        if (st + 1 < nsteps) load_step(st + 1, 1);
        consume(st, 0);
        if (st + 1 < nsteps) {
            if (st + 2 < nsteps) load_step(st + 2, 0);
            consume(st + 1, 1);
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int e = 0; e < 2; ++e)
                sP[wave - 1][c][lane * 2 + e] =
                    make_double2(acc[e][c].s, acc[e][c].c);
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int e = 0; e < 2; ++e) {
#pragma unroll
                for (int w = 0; w < 3; ++w) {  // ((w0 + w1) + w2) + w3
                    const double2 p = sP[w][c][lane * 2 + e];
                    dd::merge(acc[e][c], dd::Acc{p.x, p.y});
                }
                if (j0 + e < K)
                    W[((int64_t)blockIdx.y * NC + c) * K + j0 + e] =
                        make_double2(acc[e][c].s, acc[e][c].c);
            }
    }
}

// R[j][c0 + c] = round(((B[j][c0 + c] + p_0) + p_1) + ... ), p_ch = W[ch][c][j]:
// one thread per (j, c), threads along j so the 16-byte reads of W coalesce.
__global__ __launch_bounds__(64) void k_residual_dd_t_finish(
    const double2 *__restrict__ W, const double *__restrict__ B,
    double *__restrict__ R, int K, int nrhs, int c0, int nc, int nchunks) {
    const int j = blockIdx.x * 64 + threadIdx.x, c = blockIdx.y;
    if (j >= K) return;
    dd::Acc acc{B[(int64_t)j * nrhs + c0 + c], 0.0};
#pragma unroll 8
    for (int ch = 0; ch < nchunks; ++ch) {
        const double2 p = W[((int64_t)ch * nc + c) * K + j];
        dd::merge(acc, dd::Acc{p.x, p.y});
    }
    R[(int64_t)j * nrhs + c0 + c] = dd::round(acc);
}

// out[row] = sum_k |A[row][k]|: one wave per row, lanes along k, butterfly in
// a fixed order.  max over the rows (k_colmax_abs) gives ||A||inf.
__global__ __launch_bounds__(256) void k_row_abs_sums(
    const double *__restrict__ A, int64_t lda, int M, int K,
    double *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const double *a = A + (int64_t)row * lda;
    double s = 0;
    for (int k = lane; k < K; k += 64) s += fabs(a[k]);
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) out[row] = s;
}

// out[col] = sum_i |A[i][col]|: one thread per column walking the rows in
// order (a row of threads reads a contiguous row segment), so the sum has one
// fixed order.  max over the columns (k_colmax_abs) gives ||A||1.
__global__ __launch_bounds__(64) void k_col_abs_sums(
    const double *__restrict__ A, int64_t lda, int M, int K,
    double *__restrict__ out) {
    const int col = blockIdx.x * 64 + threadIdx.x;
    if (col >= K) return;
    double s = 0;
    for (int i = 0; i < M; ++i) s += fabs(A[(int64_t)i * lda + col]);
    out[col] = s;
}

// out[j] = max_i |V[i][j]| of an n x ncols array (ld = ncols): one block per
// column.  A NaN in the column is returned, not skipped.
__global__ __launch_bounds__(256) void k_colmax_abs(
    const double *__restrict__ V, int64_t n, int ncols,
    double *__restrict__ out) {
    __shared__ double part[256];
    const int tid = threadIdx.x, j = blockIdx.x;
    auto nmax = [](double m, double a) { return (a > m || a != a) ? a : m; };
    double m = 0;
    for (int64_t i = tid; i < n; i += 256) m = nmax(m, fabs(V[i * ncols + j]));
    part[tid] = m;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) part[tid] = nmax(part[tid], part[tid + w]);
        __syncthreads();
    }
    if (tid == 0) out[j] = part[0];
}

// X[:, j] += D[:, j] for the columns with mask[j] != 0
__global__ void k_axpy_masked(double *__restrict__ X,
                              const double *__restrict__ D,
                              const int *__restrict__ mask, int64_t n,
                              int ncols) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < n * ncols; i += stride)
        if (mask[i % ncols]) X[i] += D[i];
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

void launch_trsm_left_tri_mfma_t(const double *T, int64_t ldt, double *X,
                                 int64_t ldx, int v, int64_t N,
                                 int upper_stored, int unit, hipStream_t s) {
    if (N <= 0 || v <= 0) return;
    const dim3 grid((unsigned)((N + TRI_COLS - 1) / TRI_COLS)), block(256);
    if (upper_stored && unit)
        hipLaunchKernelGGL((k_trsm_left_tri_mfma<true, true, true>), grid,
                           block, 0, s, T, ldt, X, ldx, v, N);
    else if (upper_stored)
        hipLaunchKernelGGL((k_trsm_left_tri_mfma<true, false, true>), grid,
                           block, 0, s, T, ldt, X, ldx, v, N);
    else if (unit)
        hipLaunchKernelGGL((k_trsm_left_tri_mfma<false, true, true>), grid,
                           block, 0, s, T, ldt, X, ldx, v, N);
    else
        hipLaunchKernelGGL((k_trsm_left_tri_mfma<false, false, true>), grid,
                           block, 0, s, T, ldt, X, ldx, v, N);
}

void launch_update_skinny_t(const double *A, int64_t lda, const double *B,
                            int64_t ldb, double *C, int64_t ldc, int M,
                            int nrhs, int K, hipStream_t s) {
    if (M <= 0 || nrhs <= 0 || K <= 0) return;
    const int nblocks = std::min((M + 63) / 64, 2048);
    // 16-column groups of B and C (each re-reads the panel); C -= is
    // additive over K
    for (int c0 = 0; c0 < nrhs; c0 += 16) {
        const int nc = std::min(16, nrhs - c0);
        for (int k0 = 0; k0 < K; k0 += SKN_KMAX) {
            const int kc = std::min(SKN_KMAX, K - k0);
            const double *a = A + (int64_t)k0 * lda;
            const double *b = B + (int64_t)k0 * ldb + c0;
            if (kc % 64 == 0)
                hipLaunchKernelGGL(k_update_skinny_t<true>, dim3(nblocks),
                                   dim3(256), 0, s, a, lda, b, ldb, C + c0,
                                   ldc, M, nc, kc);
            else
                hipLaunchKernelGGL(k_update_skinny_t<false>, dim3(nblocks),
                                   dim3(256), 0, s, a, lda, b, ldb, C + c0,
                                   ldc, M, nc, kc);
        }
    }
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

template <int NC>
static void launch_residual_group(const double *A, int64_t lda,
                                  const double *X, const double *B, double *R,
                                  int M, int K, int nrhs, int c0, bool fast,
                                  hipStream_t s) {
    const dim3 grid((unsigned)((M + 4 * RES_R - 1) / (4 * RES_R))), block(256);
    if (fast)
        hipLaunchKernelGGL((k_residual_dd<NC, true>), grid, block, 0, s, A,
                           lda, X, B, R, M, K, nrhs, c0);
    else
        hipLaunchKernelGGL((k_residual_dd<NC, false>), grid, block, 0, s, A,
                           lda, X, B, R, M, K, nrhs, c0);
}

int conflux_residual_group_width() { return RES_G; }

void launch_residual_dd(const double *A, int64_t lda, const double *X,
                        const double *B, double *R, int M, int K, int nrhs,
                        hipStream_t s) {
    if (M <= 0 || K <= 0 || nrhs <= 0) return;
    const bool fast = lda % 2 == 0 && ((uintptr_t)A & 15) == 0;
    for (int c0 = 0; c0 < nrhs; c0 += RES_G) {  // one pass over A per group
        switch (std::min(RES_G, nrhs - c0)) {
            case 4:
                launch_residual_group<4>(A, lda, X, B, R, M, K, nrhs, c0,
                                         fast, s);
                break;
            case 3:
                launch_residual_group<3>(A, lda, X, B, R, M, K, nrhs, c0,
                                         fast, s);
                break;
            case 2:
                launch_residual_group<2>(A, lda, X, B, R, M, K, nrhs, c0,
                                         fast, s);
                break;
            default:
                launch_residual_group<1>(A, lda, X, B, R, M, K, nrhs, c0,
                                         fast, s);
        }
    }
}

template <int NC>
static void launch_residual_t_group(const double *A, int64_t lda,
                                    const double *X, const double *B,
                                    double *R, double2 *W, int M, int K,
                                    int nrhs, int c0, bool fast,
                                    hipStream_t s) {
    const int nchunks = (M + RT_CH - 1) / RT_CH;
    const dim3 grid((unsigned)((K + RT_W - 1) / RT_W), (unsigned)nchunks);
    if (fast)
        hipLaunchKernelGGL((k_residual_dd_t_part<NC, true>), grid, dim3(256),
                           0, s, A, lda, X, W, M, K, nrhs, c0);
    else
        hipLaunchKernelGGL((k_residual_dd_t_part<NC, false>), grid, dim3(256),
                           0, s, A, lda, X, W, M, K, nrhs, c0);
    hipLaunchKernelGGL(k_residual_dd_t_finish,
                       dim3((unsigned)((K + 63) / 64), (unsigned)NC), dim3(64),
                       0, s, W, B, R, K, nrhs, c0, NC, nchunks);
}

int conflux_residual_t_chunk() { return RT_CH; }

size_t residual_dd_t_ws_bytes(int M, int K, int nrhs) {
    if (M <= 0 || K <= 0 || nrhs <= 0) return 0;
    return (size_t)((M + RT_CH - 1) / RT_CH) * std::min(RES_G, nrhs) * K *
           sizeof(double2);
}

int launch_residual_dd_t(const double *A, int64_t lda, const double *X,
                         const double *B, double *R, int M, int K, int nrhs,
                         hipStream_t s, double *ws) {
    if (M <= 0 || K <= 0 || nrhs <= 0) return 0;
    double *own = nullptr;
    if (!ws) {
        if (hipMalloc(&own, residual_dd_t_ws_bytes(M, K, nrhs)) != hipSuccess)
            return -1;
        ws = own;
    }
    double2 *W = reinterpret_cast<double2 *>(ws);
    const bool fast = lda % 2 == 0 && ((uintptr_t)A & 15) == 0;
    // one pass over A per group; the groups share W in stream order
    for (int c0 = 0; c0 < nrhs; c0 += RES_G) {
        switch (std::min(RES_G, nrhs - c0)) {
            case 4:
                launch_residual_t_group<4>(A, lda, X, B, R, W, M, K, nrhs, c0,
                                           fast, s);
                break;
            case 3:
                launch_residual_t_group<3>(A, lda, X, B, R, W, M, K, nrhs, c0,
                                           fast, s);
                break;
            case 2:
                launch_residual_t_group<2>(A, lda, X, B, R, W, M, K, nrhs, c0,
                                           fast, s);
                break;
            default:
                launch_residual_t_group<1>(A, lda, X, B, R, W, M, K, nrhs, c0,
                                           fast, s);
        }
    }
    if (own) {  // hipFree waits for the kernels that use it
        const hipError_t e = hipStreamSynchronize(s);
        (void)hipFree(own);
        if (e != hipSuccess) return -1;
    }
    return 0;
}

void launch_row_abs_sums(const double *A, int64_t lda, int M, int K,
                         double *out, hipStream_t s) {
    if (M <= 0 || K <= 0) return;
    hipLaunchKernelGGL(k_row_abs_sums, dim3((unsigned)((M + 3) / 4)),
                       dim3(256), 0, s, A, lda, M, K, out);
}

void launch_col_abs_sums(const double *A, int64_t lda, int M, int K,
                         double *out, hipStream_t s) {
    if (M <= 0 || K <= 0) return;
    hipLaunchKernelGGL(k_col_abs_sums, dim3((unsigned)((K + 63) / 64)),
                       dim3(64), 0, s, A, lda, M, K, out);
}

void launch_colmax_abs(const double *V, int64_t n, int ncols, double *out,
                       hipStream_t s) {
    if (n <= 0 || ncols <= 0) return;
    hipLaunchKernelGGL(k_colmax_abs, dim3((unsigned)ncols), dim3(256), 0, s,
                       V, n, ncols, out);
}

void launch_axpy_masked(double *X, const double *D, const int *mask,
                        int64_t n, int ncols, hipStream_t s) {
    if (n <= 0 || ncols <= 0) return;
    const int64_t blocks = std::min<int64_t>((n * ncols + 255) / 256, 4096);
    hipLaunchKernelGGL(k_axpy_masked, dim3((unsigned)blocks), dim3(256), 0, s,
                       X, D, mask, n, ncols);
}
