// Host-side launch API of the HIP kernels (kernels.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#define CONFLUX_PANEL_MAX_BLOCKS 256

void launch_init_matrix(double *A, int Ml, int Nl, int v, int Px, int Py,
                        int pi, int pj, int zero_layer, uint64_t seed,
                        hipStream_t s);
void launch_copy2d(const double *src, int64_t lds, double *dst, int64_t ldd,
                   int rows, int64_t cols, hipStream_t s);
void launch_zero2d(double *dst, int64_t ldd, int rows, int64_t cols,
                   hipStream_t s);
void launch_add2d(const double *src, int64_t lds, double *dst, int64_t ldd,
                  int rows, int64_t cols, hipStream_t s);
void launch_row_gather(const double *src, int64_t lds, double *dst,
                       int64_t ldd, const int *idx, int n_rows, int64_t cols,
                       hipStream_t s);
void launch_row_scatter(const double *src, int64_t lds, double *dst,
                        int64_t ldd, const int *idx, int n_rows, int64_t cols,
                        hipStream_t s);
void launch_rowperm_skip(double *mat, int64_t ld, const int *dst_idx,
                         const int *src_idx, int row_base, int n_rows,
                         int64_t skip0, int64_t skipn, int64_t tot_cols,
                         double *tmp, hipStream_t s);
// fused inter-leaf glue of factor_panel (32-column leaves only): prep = the
// leaf's row permutation (sub-panel at columns [jb, jb+32) skipped, tot_cols
// other columns, 64-entry swap map relative to row jb) plus, with L given,
// the unit-lower solve of rows jb..jb+31 right of the sub-panel; update =
// C (M x N) -= A (M x 32) B (32 x N).  Bitwise equal to launch_rowperm_skip
// + launch_trsm_left_lower_unit32 + launch_dgemm_f64 at K = 32.
void launch_panel_glue_prep(double *mat, int64_t ld, const int *dst_idx,
                            const int *src_idx, int jb, int tot_cols,
                            const double *L, int64_t ldl, hipStream_t s);
void launch_panel_glue_update(const double *A, int64_t lda, const double *B,
                              int64_t ldb, double *C, int64_t ldc, int M,
                              int N, hipStream_t s);
int launch_panel_factor(double *panel, int64_t ldp, int m, int nb, void *sync,
                        int *ipiv, unsigned int epoch0, int *swap_dst,
                        int *swap_src, hipStream_t s);
int conflux_panel_sync_bytes();
int conflux_panel_err_offset();  // byte offset of the give-up word (u32)
void conflux_panel_spin_read(void *sync, unsigned long long *out,
                             hipStream_t s);
// leaf-kernel switches (CONFLUX_PANEL_REG / _PUBLISH / _PHASE_STATS); the
// setters return the previous mode.  phase_read: the eight cycle totals of
// the instrumented kernels (four phases summed over all blocks, then block
// 0's), read and reset.
int conflux_panel_reg_mode();
int conflux_panel_publish_mode();
int conflux_panel_phase_stats_mode();
int conflux_panel_set_reg_mode(int mode);
int conflux_panel_set_publish_mode(int mode);
int conflux_panel_set_phase_stats_mode(int mode);
void conflux_panel_phase_read(void *sync, unsigned long long *out8,
                              hipStream_t s);
int conflux_panel_nb();
int conflux_panel_rpb();
int conflux_panel_blocks_per_cu();
void launch_trsm_left_lower_unit32(const double *L, int64_t ldl, double *X,
                                   int64_t ldx, int nb, int64_t N,
                                   hipStream_t s);
void launch_trsm_right_upper32(const double *U, int64_t ldu, double *X,
                               int64_t ldx, int nb, int64_t M, int trans,
                               hipStream_t s);
void launch_trsm_right_mfma(const double *U, int64_t ldu, double *X,
                            int64_t ldx, int v, int64_t M, int trans,
                            hipStream_t s);
void launch_trsm_left_mfma(const double *L, int64_t ldl, double *X,
                           int64_t ldx, int v, int64_t N, hipStream_t s);
// stripe-resident editions of the two fused solves (bit-identical to them):
// a block keeps its 32-wide stripe of X in LDS for the whole triangle.
// conflux_trsm_stripe_fits(v): v % 32 == 0 and the stripe fits the LDS.
// ws: conflux_trsm_stripe_ws_doubles(v) doubles of device scratch per
// launch in flight; the launch first copies the triangle into it block-major.
int conflux_trsm_stripe_width();
bool conflux_trsm_stripe_fits(int v);
int64_t conflux_trsm_stripe_ws_doubles(int v);
void launch_trsm_right_stripe(const double *U, int64_t ldu, double *X,
                              int64_t ldx, int v, int64_t M, int trans,
                              double *ws, hipStream_t s);
void launch_trsm_left_stripe(const double *L, int64_t ldl, double *X,
                             int64_t ldx, int v, int64_t N, double *ws,
                             hipStream_t s);
// The same solves in two parts, for callers that use one triangle for several
// launches or solve out of place.  launch_trsm_pack_tri fills ws from the
// triangle ((swap, tr) = (0, 0): X U^-1, (1, 1): X L^-T, (1, 0): L^-1 X); the
// *_packed launches read Xs (leading dimension lds) and write Xd (ldd).  Xd
// may be Xs (in place, what the two launches above do); otherwise the two
// windows must not overlap and Xs is left untouched.
void launch_trsm_pack_tri(const double *T, int64_t ldt, int v, int swap,
                          int tr, double *ws, hipStream_t s);
void launch_trsm_right_stripe_packed(const double *ws, const double *Xs,
                                     int64_t lds, double *Xd, int64_t ldd,
                                     int v, int64_t M, hipStream_t s);
void launch_trsm_left_stripe_packed(const double *ws, const double *Xs,
                                    int64_t lds, double *Xd, int64_t ldd,
                                    int v, int64_t N, hipStream_t s);
// solve_kernels.hip: X (v x N) <- T^-1 X, T lower/upper, unit/non-unit, any
// v >= 1, read in place (ldt = the global N); C (M x nrhs) -= A B, nrhs <= 16
void launch_trsm_left_tri_mfma(const double *T, int64_t ldt, double *X,
                               int64_t ldx, int v, int64_t N, int upper,
                               int unit, hipStream_t s);
void launch_update_skinny(const double *A, int64_t lda, const double *B,
                          int64_t ldb, double *C, int64_t ldc, int M, int nrhs,
                          int K, hipStream_t s);
// solve_kernels.hip, transposed solve: X (v x N) <- T^-T X on the same stored
// triangle (upper_stored names the half of T that holds it); C (M x nrhs) -=
// A^T B with A stored K x M (a row panel of F), any nrhs (16-column groups);
// out[col] = sum_i |A[i][col]|
void launch_trsm_left_tri_mfma_t(const double *T, int64_t ldt, double *X,
                                 int64_t ldx, int v, int64_t N,
                                 int upper_stored, int unit, hipStream_t s);
void launch_update_skinny_t(const double *A, int64_t lda, const double *B,
                            int64_t ldb, double *C, int64_t ldc, int M,
                            int nrhs, int K, hipStream_t s);
void launch_col_abs_sums(const double *A, int64_t lda, int M, int K,
                         double *out, hipStream_t s);
// solve_kernels.hip, refinement: R (M x nrhs) = B - A X in doubled precision
// (ld of X, B, R = nrhs; R must not alias B or X), in passes of
// conflux_residual_group_width() columns; out[row] = sum_k |A[row][k]|;
// out[j] = max_i |V[i][j]|; X[:, j] += D[:, j] where mask[j] != 0
void launch_residual_dd(const double *A, int64_t lda, const double *X,
                        const double *B, double *R, int M, int K, int nrhs,
                        hipStream_t s);
int conflux_residual_group_width();
// R (K x nrhs) = B - A^T X in doubled precision, A stored M x K and read in
// place, X (M x nrhs), B and R (K x nrhs), ld = nrhs; same column groups.
// The row reduction is cut into conflux_residual_t_chunk()-row chunks whose
// partials go through ws (residual_dd_t_ws_bytes(M, K, nrhs) bytes of device
// memory); ws == nullptr allocates and frees one and then synchronises s.
// Returns 0, or -1 when that allocation or synchronisation fails.
int launch_residual_dd_t(const double *A, int64_t lda, const double *X,
                         const double *B, double *R, int M, int K, int nrhs,
                         hipStream_t s, double *ws = nullptr);
size_t residual_dd_t_ws_bytes(int M, int K, int nrhs);
int conflux_residual_t_chunk();
void launch_row_abs_sums(const double *A, int64_t lda, int M, int K,
                         double *out, hipStream_t s);
void launch_colmax_abs(const double *V, int64_t n, int ncols, double *out,
                       hipStream_t s);
void launch_axpy_masked(double *X, const double *D, const int *mask,
                        int64_t n, int ncols, hipStream_t s);
// dense_kernels.hip, the device-resident dense interface.  import: one rank
// buffer dst (Ml x Nl, rank (pi, pj)) <- blockdiag(A, I) from the caller's
// n x n dA (order 0: dA[i * lda + j], 1: dA[j * lda + i]); export: the
// inverse map from a rank buffer into dF (row-major, ldf), cropped to n.
// rhs_stage_in: X (N x nrhs, ld = nrhs) row r <- B row (idx ? idx[r] : r) for
// r < n, zero below; rhs_stage_out: B row (idx ? idx[r] : r) <- X row r,
// r < n.  diag_gather: out[g] = the diagonal entries g < n that rank (p, p)
// holds; logdet_reduce: out3 = {sum log|d_i| (doubled precision, fixed
// order), count of d_i < 0, 1 * any zero + 2 * any non-finite}.
void launch_dense_import(const double *dA, int64_t lda, int n, int order,
                         double *dst, int Ml, int Nl, int v, int Px, int Py,
                         int pi, int pj, hipStream_t s);
void launch_dense_export(const double *src, int Ml, int Nl, int v, int Px,
                         int Py, int pi, int pj, double *dF, int64_t ldf,
                         int n, hipStream_t s);
void launch_rhs_stage_in(const double *B, int64_t ldb, int n, const int *idx,
                         double *X, int64_t N, int nrhs, hipStream_t s);
void launch_rhs_stage_out(const double *X, int nrhs, int n, const int *idx,
                          double *B, int64_t ldb, hipStream_t s);
void launch_diag_gather(const double *F, int Ml, int Nl, int v, int Px, int p,
                        int n, double *out, hipStream_t s);
void launch_logdet_reduce(const double *d, int n, double *out3,
                          hipStream_t s);
void launch_tril_unit(const double *F, double *L, int64_t n, hipStream_t s);
void launch_tril_unit_rows(const double *F, int64_t ldf, double *L,
                           int64_t ldl, int rows, int64_t row0, int64_t ncols,
                           hipStream_t s);
void launch_triu_rows(double *F, int64_t ldf, int rows, int64_t row0,
                      hipStream_t s);
void launch_transpose_add_lower(double *A, int64_t n, hipStream_t s);
void launch_tril(const double *F, double *L, int64_t n, hipStream_t s);
void launch_triu(const double *F, double *U, int64_t n, hipStream_t s);
// *out += sum A[i]^2, the same bits on every run; ws: CONFLUX_FROB2_WS_DOUBLES
// doubles of device scratch (launches on one stream may share it)
#define CONFLUX_FROB2_WS_DOUBLES 4096
void launch_frob2(const double *A, int64_t nelem, double *out, double *ws,
                  hipStream_t s);
void launch_potrf32(double *A, int64_t lda, int nb, hipStream_t s);
void launch_getrf32_nopiv(double *A, int64_t lda, int nb, hipStream_t s);
void launch_dgemm_f64_nt(const double *A, int64_t lda, const double *B,
                         int64_t ldb, double *C, int64_t ldc, int M, int64_t N,
                         int K, hipStream_t s);
void launch_dgemm_f64_nt_tril(const double *A, int64_t lda, const double *B,
                              int64_t ldb, double *C, int64_t ldc, int M,
                              int64_t N, int K, int v, int r0off,
                              int64_t c0off, int Px, int Py, int pi, int pj,
                              hipStream_t s);
void launch_init_matrix_spd(double *A, int Ml, int Nl, int v, int Px, int Py,
                            int pi, int pj, int zero_layer, uint64_t seed,
                            int64_t Nglob, hipStream_t s);
void launch_dgemm_f64(const double *A, int64_t lda, const double *B,
                      int64_t ldb, double *C, int64_t ldc, int M, int64_t N,
                      int K, hipStream_t s,
                      int maxwg = 0);
// GEMM launch switches (CONFLUX_GEMM_VARIANT / _STRIP / _NTC give the
// defaults); the setters return the previous value.
int conflux_gemm_set_variant(int variant);
int conflux_gemm_set_strip_w(int w);
int conflux_gemm_set_ntc(int on);
void launch_pack_candidate(const double *A10, int64_t lda, const int *gri,
                           int f, int n_src, int n_out, int v, const int *idx,
                           double *cand, hipStream_t s);
void launch_row_move(const double *src, int64_t lds, double *dst, int64_t ldd,
                     const int *src_idx, const int *dst_idx, int n_rows,
                     int64_t cols, hipStream_t s);
void launch_extract_col0_int(const double *cand, int stride, int n, int *out,
                             hipStream_t s);
void launch_slab_pack(const double *X, int64_t ldx, int n, int nlayr, int Pz,
                      double *out, hipStream_t s);
