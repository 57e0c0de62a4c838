/* conflux_lu.h — C ABI of the MI355X-native CONFLUX LU engine.
 *
 * Drop-in boundary for the reference's miniapp-visible surface
 * (SURVEY.md §8b).  Each entry point names the reference interface it
 * replaces:
 *
 *   conflux_lu_create/destroy   <-> conflux::lu_params<double>(N, N, v,
 *                                   Px, Py, Pz, comm) construction/teardown
 *                                   (reference src/conflux/lu/lu_params.hpp:401-413);
 *                                   the MPI communicator argument becomes
 *                                   (rank, world, nccl_uid) — one process per
 *                                   GPU, RCCL over xGMI instead of MPI.
 *   conflux_lu_init_matrix      <-> lu_params::InitMatrix()
 *                                   (lu_params.hpp:141-376); seeded generator
 *                                   is the documented grid-independent
 *                                   splitmix64 fill (oracle/gen_input.py).
 *   conflux_lu_set_matrix_local <-> writing lu_params::data directly
 *                                   (public member, lu_params.hpp:394).
 *   conflux_lu_factor           <-> std::size_t conflux::LU_rep<double>(
 *                                   lu_params&, T* C, int* perm)
 *                                   (conflux_opt.hpp:343-346): factors a copy
 *                                   of the input (input buffer not clobbered),
 *                                   returns wall-clock ms of the
 *                                   barrier-fenced superstep loop.
 *   conflux_lu_get_factors      <-> the CONFLUX_WITH_VALIDATION outputs of
 *                                   LU_rep (C result buffer + permutation,
 *                                   conflux_opt.hpp:1660-1754, 1821-1823) —
 *                                   always available here (superset), gated
 *                                   by the store_factors flag for timing runs.
 *   conflux_lu_solve /          <-> nothing: the reference has no solve.  These
 *   conflux_chol_solve              consume those same outputs (C result
 *                                   buffer + perm, conflux_opt.hpp:1660-1754)
 *                                   on device — the getrs/potrs a caller
 *                                   otherwise runs on the host after
 *                                   un-tiling the factors.
 *   conflux_lu_solve_refined /  <-> nothing either: iterative refinement with
 *   conflux_chol_solve_refined      a doubled-precision residual on top of
 *                                   those solves (LAPACK xGERFSX's scheme).
 *   conflux_lu_solve_trans      <-> nothing: the reference has no solve.  A^T X
 *                                   = B on the same stored factors (getrs with
 *                                   trans = 'T'), read in place.
 *   conflux_lu_solve_refined_trans /   <-> nothing: the refinement for A^T X
 *   conflux_lu_solve_refined_device /      = B, and all of it on the caller's
 *   conflux_chol_solve_refined_device      device buffers.
 *   conflux_lu_rcond /          <-> nothing: the reference has no solve.  The
 *   conflux_chol_rcond              reciprocal condition number (gecon /
 *                                   pocon) from Higham's 1-norm estimator
 *                                   over those solves.
 *   conflux_lu_set_matrix_device / <-> nothing: the reference's callers fill
 *   conflux_lu_get_factors_device /    lu_params::data on the host, in its
 *   conflux_lu_solve_device /          layout.  These take and return the
 *   conflux_chol_solve_device /        caller's own dense DEVICE buffers, of
 *   conflux_lu_logical_order           any order n <= N_padded.
 *   conflux_lu_slogdet /          <-> nothing: sign and log|det| (LU) and
 *   conflux_chol_logdet               log det (Cholesky) from the stored
 *                                     diagonal, reduced on device.
 *
 * Ownership: caller owns all host buffers passed in; the engine owns device
 * memory.  Deterministic given (input, grid, v, world).  All functions
 * return 0 on success, negative CONFLUX_LU_E* on failure (the reference has
 * no error channel — asserts only).
 */
#ifndef CONFLUX_LU_H
#define CONFLUX_LU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CONFLUX_LU_OK 0
#define CONFLUX_LU_EARG (-1)      /* bad/unsupported parameter combination */
#define CONFLUX_LU_EHIP (-2)      /* HIP runtime failure */
#define CONFLUX_LU_ECOMM (-3)     /* RCCL / bootstrap failure */
#define CONFLUX_LU_EINTERNAL (-4) /* invariant violation inside the engine */

#define CONFLUX_LU_UID_BYTES 128  /* == NCCL_UNIQUE_ID_BYTES */

typedef struct conflux_lu_ctx conflux_lu_ctx;

/* Grid restrictions (match the reference's de-facto envelope):
 * Px == Py, Px a power of two, v % Pz == 0, Ml >= 2v (reference buffer
 * sizing, conflux_opt.hpp:447 vs :291).  N is rounded UP to a multiple of
 * v*Px exactly like the reference (lu_params.hpp:67-71): conflux_lu_dims
 * reports the padded size, local buffers are sized for it, and the
 * generator fills the padding the way the reference's InitMatrix does
 * (a caller-supplied matrix in the engine's own layout should extend the
 * padding with nonsingular data, e.g. the same random fill — zero padding
 * would hit zero pivots, as it would in the reference;
 * conflux_lu_set_matrix_device pads by itself, with an identity block that
 * stays out of the caller's problem).
 *
 * world == Px*Py*Pz processes, one per GPU.  rank r maps to grid coords
 * (pi, pj, pk) = (r / (Py*Pz), (r / Pz) % Py, r % Pz) — the reference's
 * MPI_Cart row-major order (lu_params.hpp:84-108).
 * nccl_uid: CONFLUX_LU_UID_BYTES bytes generated by rank 0
 *           (conflux_lu_make_uid) and distributed by the caller; may be NULL
 *           when world == 1. */
int conflux_lu_create(int N, int v, int Px, int Py, int Pz,
                      int rank, int world, const char *nccl_uid,
                      conflux_lu_ctx **out);

int conflux_lu_make_uid(char uid[CONFLUX_LU_UID_BYTES]);

/* Fill the rank-local tiles with the seeded synthetic input
 * A[i,j] = 5 + U[0,1) (splitmix64(seed, i, j)); device-side, grid-independent. */
int conflux_lu_init_matrix(conflux_lu_ctx *ctx, uint64_t seed);

/* SPD variant for the Cholesky path: sym(gen) + 2N on the diagonal. */
int conflux_lu_init_matrix_spd(conflux_lu_ctx *ctx, uint64_t seed);

/* Cholesky factorization A = L L^T of the current (SPD) matrix — the
 * CONFCHOX path (reference src/conflux/cholesky/Cholesky.cpp:857
 * conflux::parallelCholesky; cholesky_miniapp CLI kept).  After a
 * store_factors run, conflux_lu_get_factors returns L in the tile-cyclic
 * layout (lower triangle valid) and an identity permutation. */
int conflux_chol_factor(conflux_lu_ctx *ctx, double *elapsed_ms);

/* Upload the rank-local Ml x Nl row-major buffer (tile-cyclic owner map of
 * reference layout.cpp:95-123).  Layers pk > 0 must pass zeros (the engine
 * zero-fills when local == NULL). */
int conflux_lu_set_matrix_local(conflux_lu_ctx *ctx, const double *local);

/* Enable/disable per-step factor collection (default ON; turn OFF for
 * timing runs — mirrors the reference's CONFLUX_WITH_VALIDATION gate). */
int conflux_lu_store_factors(conflux_lu_ctx *ctx, int enable);

/* Pivoting strategy: 1 = tournament pivoting (the reference
 * algorithm, default); 0 = none — the Python prototype's EmptyPivot fast
 * path for diagonally dominant inputs (python/conflux.py enum; the C++
 * reference implements tournament only).  perm is identity with mode 0;
 * validation works unchanged. */
int conflux_lu_set_pivoting(conflux_lu_ctx *ctx, int mode);

/* Factor (a copy of) the current matrix.  elapsed_ms: wall time of the
 * barrier-fenced superstep loop (reference convention,
 * conflux_opt.hpp:531-532, 1805-1807). */
int conflux_lu_factor(conflux_lu_ctx *ctx, double *elapsed_ms);

/* After a store_factors run: fetch the local Ml x Nl tile-cyclic slice of
 * the factored matrix F (pivoted row order: strict lower = L, upper = U;
 * same layout as the reference's C result buffer) and/or the global pivot
 * vector perm[M] (row r of PA = row perm[r] of A).  Either pointer may be
 * NULL.  Ranks with pk > 0 receive F_local = 0. */
/* ||PA - LU||_F / ||A||_F on device (CONFLUX_WITH_VALIDATION equivalent,
 * conflux_miniapp.cpp:169-507, no ScaLAPACK).  Requires store_factors.
 * Stripe-streamed (one N^2 staging buffer + O(vN) stripes), so bench-scale
 * single-GPU sizes fit in HBM.  When world > 1 this is COLLECTIVE over the
 * engine's communicator: every rank must call; pk == 0 ranks ship their
 * locals to rank 0, which computes and broadcasts the residual — all ranks
 * return the same value. */
int conflux_lu_validate(conflux_lu_ctx *ctx, double *resid);

/* Cholesky counterpart: ||A - L L^T||_F / ||A||_F on device
 * (reference CholeskyValidation, Cholesky.cpp:738-772 analogue). */
int conflux_chol_validate(conflux_lu_ctx *ctx, double *resid);

int conflux_lu_get_factors(conflux_lu_ctx *ctx, double *F_local, int *perm);

/* Solve A X = B with the factors of the last store_factors LU run
 * (tournament or nopiv) — the getrs of this library.  The reference has no
 * solve; this consumes what LU_rep leaves behind, the C result buffer and
 * perm (conflux_opt.hpp:1660-1754), without a trip through the host.
 * B: host, N_padded x nrhs, row-major, ldb = nrhs; overwritten with X.
 * elapsed_ms (may be NULL): device time of the two sweeps, excluding the
 * H2D/D2H of B.  Block forward/backward sweeps on device; the stored factors
 * are not modified, so any number of solves may follow one factor.
 * CONFLUX_LU_EARG when: B == NULL, nrhs <= 0, no factorization yet, the
 * last factorization ran with store_factors off or was a Cholesky one.
 * Real multi-process runs (world > 1) are NOT YET SUPPORTED: every rank
 * returns CONFLUX_LU_EARG before any communication.  The single-process
 * simulation grids (rank < 0) are supported. */
int conflux_lu_solve(conflux_lu_ctx *ctx, double *B, int nrhs,
                     double *elapsed_ms);

/* Same for the last Cholesky run: L L^T X = B (potrs).  EARG after an LU
 * factorization. */
int conflux_chol_solve(conflux_lu_ctx *ctx, double *B, int nrhs,
                       double *elapsed_ms);

/* Solve A X = B and improve X by extra-precise iterative refinement.  The
 * reference has no counterpart (it has no solve at all); the scheme is
 * LAPACK's xGERFSX idea on the engine's own buffers: the residual
 * R = B - A X is accumulated in doubled precision against the input
 * snapshot the factorization kept on device and rounded once, a correction
 * D = solve(R) comes from the stored factors, and X += D — column by
 * column, until a column's correction reaches the last bit, stops
 * shrinking by at least 2x per pass (it is then frozen and that correction
 * is NOT applied), its residual is exactly zero, or max_iter passes have
 * run.  What this buys: the no-pivot fast path (conflux_lu_set_pivoting(0))
 * becomes backward stable on general input after one pass, and an
 * ill-conditioned system (cond(A) well below 2^53) is solved to forward
 * error ~2^-53 instead of cond * 2^-53.
 * B: host, N_padded x nrhs, row-major, ldb = nrhs; overwritten with X.
 * max_iter >= 0; 0 = the plain solve (X bitwise equal to conflux_lu_solve)
 *           plus its backward error.
 * berr[nrhs] (may be NULL): componentwise-in-columns normwise backward
 *           error of the RETURNED X,
 *           max_i|R_ij| / (||A||inf max_i|X_ij| + max_i|B_ij|),
 *           0 when the denominator is 0; R in doubled precision, so the
 *           figure is trustworthy down to ~2^-106 relative.
 * ferr[nrhs] (may be NULL): max_i|D_ij| / max_i|X_ij| of the last correction
 *           applied to column j, 0 if none was.  An ESTIMATE of the forward
 *           error of the X before that correction, hence pessimistic for
 *           the returned X while the iteration converges — not a bound.
 * iters (may be NULL): number of passes that applied a correction to at
 *           least one column.
 * elapsed_ms (may be NULL): device time from the first sweep to the last
 *           residual, the per-pass host decisions included; excludes the
 *           H2D/D2H of B.
 * Deterministic: two calls on the same factors and B agree bitwise.  The
 * stored factors and the input snapshot are only read.  The Cholesky
 * variant multiplies by the stored input as it stands, so BOTH triangles
 * of the input must hold A (conflux_lu_init_matrix_spd and a full-matrix
 * upload do; a lower-only upload does not).
 * CONFLUX_LU_EARG: max_iter < 0, and every case in which conflux_lu_solve /
 * conflux_chol_solve return it (world > 1 included, before any
 * communication). */
int conflux_lu_solve_refined(conflux_lu_ctx *ctx, double *B, int nrhs,
                             int max_iter, double *berr, double *ferr,
                             int *iters, double *elapsed_ms);

int conflux_chol_solve_refined(conflux_lu_ctx *ctx, double *B, int nrhs,
                               int max_iter, double *berr, double *ferr,
                               int *iters, double *elapsed_ms);

/* Solve A^T X = B with the factors of the last store_factors LU run — the
 * trans = 'T' of getrs, for adjoint problems and for callers whose matrix is
 * stored column-major (for them the engine's A is their A^T).  The reference
 * has no counterpart (it has no solve at all).  A^T = U^T L^T P: a forward
 * sweep with U^T, a backward sweep with L^T, then X[perm[r]] = Z[r].  Both
 * sweeps read the stored factors in place, along their stored rows; no
 * transposed copy of F is made, so a Px = Py = 1 run allocates no N^2
 * buffer, exactly like conflux_lu_solve.
 * Every convention of conflux_lu_solve holds: B host, N_padded x nrhs,
 * row-major, overwritten with X; elapsed_ms (may be NULL) is the device time
 * of the two sweeps; the factors are only read; tournament and no-pivot runs
 * and the simulation grids are supported; CONFLUX_LU_EARG in the same cases
 * (world > 1 included, before any communication).  After a Cholesky run it
 * returns CONFLUX_LU_EARG: there A = A^T and conflux_chol_solve is the
 * answer.  env CONFLUX_SOLVE_BLOCK applies.  CONFLUX_SOLVE_SKINNY does NOT:
 * the transposed update has no GEMM variant to switch to, every nrhs runs
 * through the skinny kernel in groups of 16 columns. */
int conflux_lu_solve_trans(conflux_lu_ctx *ctx, double *B, int nrhs,
                           double *elapsed_ms);

/* conflux_lu_solve_refined for A^T X = B: X = conflux_lu_solve_trans(B), the
 * residual R = B - A^T X in doubled precision, D = conflux_lu_solve_trans(R),
 * the same decision rules.  The residual reads the input snapshot in place,
 * along its stored rows — no transposed copy, so a Px = Py = 1 run still
 * allocates no N^2 buffer; its reduction over the rows is split over the
 * grid through a workspace of N_padded / 256 partial vectors per column of a
 * group, merged in an order fixed by indices alone.
 * Every convention of conflux_lu_solve_refined holds (B host, N_padded x
 * nrhs, overwritten with X; berr, ferr, iters, elapsed_ms; deterministic;
 * factors and snapshot only read), with two differences: berr's norm is
 * ||A^T||inf = ||A||1, the figure conflux_lu_rcond(norm = 0) caches, and
 * max_iter = 0 gives X bitwise equal to conflux_lu_solve_trans.
 * CONFLUX_LU_EARG: max_iter < 0 and every case in which
 * conflux_lu_solve_trans returns it — after a Cholesky run included (there
 * A = A^T: conflux_chol_solve_refined) and world > 1, before any
 * communication. */
int conflux_lu_solve_refined_trans(conflux_lu_ctx *ctx, double *B, int nrhs,
                                   int max_iter, double *berr, double *ferr,
                                   int *iters, double *elapsed_ms);

/* Reciprocal condition number of the matrix of the last store_factors LU
 * run (gecon): rcond = 1 / (||A|| * est||A^-1||) in the 1-norm (norm = 0) or
 * the infinity norm (norm = 1).  The reference has no counterpart.  ||A|| is
 * exact, from the input snapshot the factorization kept on device;
 * ||A^-1|| comes from Higham's 1-norm estimator (LAPACK's dlacn2
 * iteration), which alternates single-RHS solves with A and A^T on the
 * stored factors.  The estimate is a lower bound on ||A^-1||, so rcond is an
 * UPPER bound on the true value — in practice within a factor 3 and usually
 * within a few percent.  cond(A) ~ 1 / rcond is the number that
 * conflux_lu_solve_refined's "cond(A) well below 2^53" and the no-pivot fast
 * path's "diagonally dominant" ask about.
 * After conflux_lu_set_matrix_device with n < N_padded, rcond describes the
 * caller's n x n matrix: ||A|| is taken over the leading n rows and columns
 * of the snapshot and the estimator runs at dimension n.  After every other
 * way of setting the matrix (logical order == N_padded) it describes the
 * PADDED N_padded x N_padded matrix the engine factored, padding rows and
 * columns included.
 * rcond = 0 when ||A|| == 0 or the estimate is not finite (a zero pivot) —
 * not an error.
 * anorm (may be NULL): ||A|| in the chosen norm; computed once per
 *           factorization and norm, then cached.
 * nsolves (may be NULL): single-RHS solves used, 1 <= nsolves <= 12.
 * elapsed_ms (may be NULL): device time of the estimation loop, the
 *           N-double transfers between its steps included; excludes ||A||.
 * Deterministic: two calls agree bitwise.  The stored factors and the input
 * snapshot are only read.
 * CONFLUX_LU_EARG: rcond == NULL, norm not 0 or 1, and every case in which
 * conflux_lu_solve returns it (world > 1 included, before any
 * communication). */
int conflux_lu_rcond(conflux_lu_ctx *ctx, int norm, double *rcond,
                     double *anorm, int *nsolves, double *elapsed_ms);

/* Same for the last Cholesky run (pocon): A is symmetric, the two norms
 * coincide and both of the estimator's solves are conflux_chol_solve's.
 * ||A|| is taken from the stored input as it stands, so BOTH triangles of
 * the input must hold A (the rule of conflux_chol_solve_refined).  EARG
 * after an LU factorization. */
int conflux_chol_rcond(conflux_lu_ctx *ctx, double *rcond, double *anorm,
                       int *nsolves, double *elapsed_ms);

/* ---- Device-resident dense interface (no reference counterpart) ----------
 *
 * Point the engine at a matrix the caller already holds on the device: any
 * order 1 <= n <= N_padded (whole tiles of padding included), row- or
 * column-major, no host trip and no re-tiling by the caller.  The engine
 * factors blockdiag(A, I) of order N_padded.  Tournament pivoting never picks
 * an all-zero candidate row and the zero-pivot rule never scales by one, so
 * the identity block is inert: perm[n:] is the identity, F[n:, n:] == I, both
 * off-diagonal blocks of F are exactly zero, and the padded problem is the
 * caller's problem plus rows that do not couple to it.
 *
 * Pointers and streams: every d* pointer is DEVICE memory owned by the
 * caller.  The calls enqueue on the engine's own stream and return after
 * synchronizing it; they do not wait for any other stream, so the caller
 * must have finished producing the buffers (synchronize the producing stream
 * first).  Single process only: the one-rank engine (world == 1) and the
 * simulation grids (rank < 0); world > 1 returns CONFLUX_LU_EARG before any
 * communication, like the solves.
 *
 * Logical order: the context remembers n.  conflux_lu_init_matrix*,
 * conflux_lu_set_matrix_local and the simulation upload reset it to
 * N_padded, after which everything behaves as it always did.  What follows
 * the logical order of the matrix last factored: the *_device calls below
 * (the refined solves conflux_lu_solve_refined_device /
 * conflux_chol_solve_refined_device among them),
 * conflux_lu_slogdet / conflux_chol_logdet and conflux_lu_rcond /
 * conflux_chol_rcond.  What keeps describing the PADDED matrix:
 * conflux_lu_validate / conflux_chol_validate (the residual numerator is
 * unaffected, ||A||_F gains the N_padded - n ones), the host-buffer solves
 * (B has N_padded rows) and conflux_lu_get_factors.
 *
 * conflux_lu_set_matrix_device: dA holds element (i, j) at dA[i * lda + j]
 * (order 0, row-major) or dA[j * lda + i] (order 1, column-major), lda >= n.
 * Marks the input fresh exactly as conflux_lu_set_matrix_local does: the
 * next factor snapshots it, repeated factors restore the snapshot,
 * conflux_lu_set_pivoting(0) and conflux_chol_factor work unchanged
 * (blockdiag(SPD, I) is SPD).  Layers pk > 0 are zeroed.
 * CONFLUX_LU_EARG: dA == NULL, n < 1, n > N_padded, lda < n, order not 0/1,
 * world > 1. */
int conflux_lu_set_matrix_device(conflux_lu_ctx *ctx, const double *dA,
                                 int64_t lda, int n, int order);

/* The logical order of the CURRENT input (N_padded unless the last matrix
 * came through conflux_lu_set_matrix_device). */
int conflux_lu_logical_order(conflux_lu_ctx *ctx, int *n);

/* After a store_factors run: the leading n x n block of the factored matrix
 * (pivoted row order, strict lower = L, upper = U; Cholesky: lower = L) as a
 * dense row-major device matrix dF (ldf >= n), and/or the leading n entries
 * of perm as int32 on the device.  Either pointer may be NULL.
 * CONFLUX_LU_EARG: no stored factorization, ldf < n with dF given,
 * world > 1. */
int conflux_lu_get_factors_device(conflux_lu_ctx *ctx, double *dF,
                                  int64_t ldf, int *dperm);

/* conflux_lu_solve (trans = 0) / conflux_lu_solve_trans (trans = 1) on the
 * caller's device buffer: dB is n x nrhs, row-major, ldb >= nrhs, overwritten
 * in place with X; the ldb - nrhs slack of every row is not touched.
 * elapsed_ms has conflux_lu_solve's meaning; CONFLUX_SOLVE_BLOCK /
 * CONFLUX_SOLVE_SKINNY apply as there.  The sweeps are the host entry
 * points' sweeps — with n == N_padded the bits agree.
 * CONFLUX_LU_EARG: dB == NULL, nrhs <= 0, ldb < nrhs, trans not 0/1, and
 * every case in which conflux_lu_solve returns it (world > 1 included). */
int conflux_lu_solve_device(conflux_lu_ctx *ctx, double *dB, int64_t ldb,
                            int nrhs, int trans, double *elapsed_ms);

/* Same for the last Cholesky run (conflux_chol_solve's guards). */
int conflux_chol_solve_device(conflux_lu_ctx *ctx, double *dB, int64_t ldb,
                              int nrhs, double *elapsed_ms);

/* conflux_lu_solve_refined (trans = 0) / conflux_lu_solve_refined_trans
 * (trans = 1) on the caller's device buffer: dB is n x nrhs, row-major,
 * ldb >= nrhs, n the logical order of the matrix last factored; overwritten
 * in place with X, the ldb - nrhs slack of every row is not touched.  The
 * engine keeps its own zero-extended copy of B for the residual, so nothing
 * but the window is written.  berr, ferr (host arrays of nrhs doubles),
 * iters and elapsed_ms have conflux_lu_solve_refined's meaning and may be
 * NULL.
 * Everything describes the caller's n x n matrix: ||A|| in berr is the norm
 * of the leading n x n block of the snapshot (inf-norm, 1-norm with trans —
 * the figures conflux_lu_rcond reports), the residual and the column maxima
 * range over the leading n rows, and the padding rows of X, R and D stay
 * exactly zero.  With n == N_padded, X, berr, ferr and iters are bitwise
 * those of the host entry points; max_iter = 0 gives X bitwise equal to
 * conflux_lu_solve_device.
 * CONFLUX_LU_EARG: dB == NULL, nrhs <= 0, ldb < nrhs, trans not 0/1,
 * max_iter < 0, and every case in which conflux_lu_solve returns it
 * (world > 1 included, before any communication). */
int conflux_lu_solve_refined_device(conflux_lu_ctx *ctx, double *dB,
                                    int64_t ldb, int nrhs, int trans,
                                    int max_iter, double *berr, double *ferr,
                                    int *iters, double *elapsed_ms);

/* Same for the last Cholesky run (conflux_chol_solve_refined on a device
 * buffer; max_iter = 0 is conflux_chol_solve_device bit for bit).  The
 * both-triangles rule of conflux_chol_solve_refined still holds: the
 * residual multiplies by the stored input as it stands, so the n x n matrix
 * handed to conflux_lu_set_matrix_device must hold A in BOTH triangles. */
int conflux_chol_solve_refined_device(conflux_lu_ctx *ctx, double *dB,
                                      int64_t ldb, int nrhs, int max_iter,
                                      double *berr, double *ferr, int *iters,
                                      double *elapsed_ms);

/* det(A) of the n x n matrix of the last store_factors LU run as
 * sign * exp(logabsdet): logabsdet = sum log|U_ii| over the leading n
 * diagonal entries (summed on device in doubled precision, in a fixed order:
 * two calls agree bitwise), sign = det(P) * prod sign(U_ii) in {-1, +1}.
 * A zero pivot gives sign = 0, logabsdet = -inf — not an error; a non-finite
 * pivot gives NaN in both.
 * CONFLUX_LU_EARG: a NULL output, and conflux_lu_solve's guard cases (no
 * factorization, store_factors off, a Cholesky run, world > 1). */
int conflux_lu_slogdet(conflux_lu_ctx *ctx, double *sign, double *logabsdet);

/* log det(A) = 2 * sum log L_ii for the last Cholesky run; EARG after an LU
 * factorization. */
int conflux_chol_logdet(conflux_lu_ctx *ctx, double *logdet);

/* Dimensions derived by the engine (reference lu_params.hpp:67-82). */
int conflux_lu_dims(conflux_lu_ctx *ctx, int *Ml, int *Nl, int *Nt,
                    int *nlayr, int *M_padded, int *N_padded);

/* Per-kernel timing stats from the last factor() call (HIP events on the
 * launch stream).  kernel: 0 = trailing-update DGEMM, 1 = panel getrf,
 * 2 = TRSMs, 3 = row movement.  Returns total seconds, launch count and
 * total algorithmic flops (for kernel 0) via out params. */
int conflux_lu_kernel_stats(conflux_lu_ctx *ctx, int kernel,
                            double *seconds, long *launches, double *flops);

int conflux_lu_destroy(conflux_lu_ctx *ctx);

/* Library self-description (for loud failure when the HIP path is absent). */
const char *conflux_lu_build_info(void);

#ifdef __cplusplus
}
#endif
#endif /* CONFLUX_LU_H */
