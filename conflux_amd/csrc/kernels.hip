// kernels.hip — CDNA4 (gfx950) kernels of the MI355X-native CONFLUX LU engine.
//
// Re-expressions of the reference's compute units (SURVEY.md §2 checklist):
//   k_dgemm_mfma       <- trailing-update cblas_dgemm (conflux_opt.hpp:1628-1633)
//                         and the panel-update GEMMs of blocked getrf/TRSM;
//                         hand-written v_mfma_f64_16x16x4_f64, LDS-staged.
//   k_panel_factor     <- LAPACKE_dgetrf partial pivoting
//                         (conflux_opt.hpp:143-166 LUP): persistent sub-panel
//                         kernel, LDS-resident rows, grid-wide first-max
//                         argmax per column via an agent-scope
//                         release/acquire slab handshake.
//   k_trsm_*           <- cblas_dtrsm Right/Upper/NonUnit (:1347) and
//                         Left/Lower/Unit (:1539), 32-wide diagonal blocks +
//                         k_dgemm_mfma updates.
//   k_row_gather/scatter/move, k_swap_map/k_rowperm_*, k_copy2d, ...
//                      <- push_pivots_up / permute_rows / dlaswp / mcopy
//                         (conflux_opt.hpp:176-218, utils.hpp:48-160,
//                          memory_utils.hpp:8-34) as coalesced index-vector
//                         kernels.
//   k_init_matrix      <- lu_params::InitMatrix random fill (splitmix64
//                         variant, oracle/gen_input.py — bit-identical).
//
// All fp64.  No CUDA-compat shims, no library GEMMs on the hot path.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <type_traits>

#include "kernels.hpp"

#define DEVFN __device__ __forceinline__

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));
// two adjacent doubles at an address that is only 8-byte aligned
typedef double f64x2u __attribute__((ext_vector_type(2), aligned(8)));

namespace ck {

// ---------------------------------------------------------------------------
// input generator (matches oracle/gen_input.py bit-for-bit)
// ---------------------------------------------------------------------------
DEVFN uint64_t splitmix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

DEVFN double gen_entry(int64_t gi, int64_t gj, uint64_t seed) {
    uint64_t key = ((uint64_t)gi << 32) ^ (uint64_t)gj;
    key += seed * 0xBF58476D1CE4E5B9ull;
    const uint64_t h = splitmix64(key);
    return 5.0 + (double)(h >> 11) * (1.0 / 9007199254740992.0);
}

// Grid-stride: a flat launch over Ml x Nl elements would need 2^32 threads
// at N=65536, one past HIP's 32-bit total-thread launch limit — the launch
// is REJECTED SILENTLY and the matrix stays zero (found the hard way; the
// launchers below cap the grid and every at-risk kernel strides).
__global__ void k_init_matrix(double *__restrict__ A, int Ml, int Nl, int v,
                              int Px, int Py, int pi, int pj, int zero_layer,
                              uint64_t seed, int spd, int64_t Nglob) {
    const int64_t total = (int64_t)Ml * Nl;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         idx < total; idx += stride) {
        if (zero_layer) {
            A[idx] = 0.0;
            continue;
        }
        const int r = (int)(idx / Nl), c = (int)(idx % Nl);
        // local (r, c) -> global (i, j): tile-cyclic map (layout.cpp:95-123)
        const int64_t gi = (int64_t)(r / v * Px + pi) * v + r % v;
        const int64_t gj = (int64_t)(c / v * Py + pj) * v + c % v;
        if (spd) {
            // symmetric positive definite: sym(gen)/1 + 2N on the diagonal
            double x = 0.5 * (gen_entry(gi, gj, seed) + gen_entry(gj, gi, seed));
            if (gi == gj) x += 2.0 * (double)Nglob;
            A[idx] = x;
            continue;
        }
        A[idx] = gen_entry(gi, gj, seed);
    }
}

// ---------------------------------------------------------------------------
// 2D strided copies / zero / add (mcopy & reduce-combine re-expressions)
// ---------------------------------------------------------------------------
__global__ void k_copy2d(const double *__restrict__ src, int64_t lds,
                         double *__restrict__ dst, int64_t ldd,
                         int rows, int64_t cols) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < (int64_t)rows * cols; i += stride) {
        const int64_t r = i / cols, c = i % cols;
        dst[r * ldd + c] = src[r * lds + c];
    }
}

__global__ void k_zero2d(double *__restrict__ dst, int64_t ldd, int rows,
                         int64_t cols) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < (int64_t)rows * cols; i += stride)
        dst[(i / cols) * ldd + i % cols] = 0.0;
}

__global__ void k_add2d(const double *__restrict__ src, int64_t lds,
                        double *__restrict__ dst, int64_t ldd, int rows,
                        int64_t cols) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < (int64_t)rows * cols; i += stride)
        dst[(i / cols) * ldd + i % cols] += src[(i / cols) * lds + i % cols];
}

// dst row i <- src row idx[i]   (gather; push_pivots_up phase 1/3,
// candidate winner permute — utils.hpp inverse_permute_rows)
__global__ void k_row_gather(const double *__restrict__ src, int64_t lds,
                             double *__restrict__ dst, int64_t ldd,
                             const int *__restrict__ idx, int n_rows,
                             int64_t cols) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < (int64_t)n_rows * cols; i += stride) {
        const int64_t r = i / cols, c = i % cols;
        dst[r * ldd + c] = src[(int64_t)idx[r] * lds + c];
    }
}

// dst row idx[i] <- src row i   (scatter; push_pivots_up phase 2,
// A01 pivot-order placement — conflux_opt.hpp:1251-1258)
__global__ void k_row_scatter(const double *__restrict__ src, int64_t lds,
                              double *__restrict__ dst, int64_t ldd,
                              const int *__restrict__ idx, int n_rows,
                              int64_t cols) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < (int64_t)n_rows * cols; i += stride) {
        const int64_t r = i / cols, c = i % cols;
        dst[(int64_t)idx[r] * ldd + c] = src[r * lds + c];
    }
}

// src rows idx[i] copied to dst rows dst_idx[i] within SAME buffer is unsafe;
// engine always stages through separate buffers (3-phase like the reference).



// gather/scatter with a skipped column range [skip0, skip0+skipn): the
// sub-panel columns were already swapped inside k_panel_factor.
__global__ void k_rowperm_gather_skip(const double *__restrict__ src,
                                      int64_t lds, double *__restrict__ tmp,
                                      const int *__restrict__ src_idx,
                                      int row_base, int n_rows, int64_t skip0,
                                      int64_t skipn, int64_t tot_cols) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < (int64_t)n_rows * tot_cols; i += stride) {
        const int64_t r = i / tot_cols, cc = i % tot_cols;
        const int64_t c = (cc < skip0) ? cc : cc + skipn;
        tmp[r * tot_cols + cc] = src[(int64_t)(row_base + src_idx[r]) * lds + c];
    }
}

__global__ void k_rowperm_scatter_skip(const double *__restrict__ tmp,
                                       double *__restrict__ dst, int64_t ldd,
                                       const int *__restrict__ dst_idx,
                                       int row_base, int n_rows, int64_t skip0,
                                       int64_t skipn, int64_t tot_cols) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < (int64_t)n_rows * tot_cols; i += stride) {
        const int64_t r = i / tot_cols, cc = i % tot_cols;
        const int64_t c = (cc < skip0) ? cc : cc + skipn;
        dst[(int64_t)(dst_idx[r] + row_base) * ldd + c] = tmp[r * tot_cols + cc];
    }
}

// dst row dst_idx[i] <- src row src_idx[i]; row sets must be disjoint
// (push_pivots_up phase 2: early non-pivots into vacated late-pivot slots)
__global__ void k_row_move(const double *__restrict__ src, int64_t lds,
                           double *__restrict__ dst, int64_t ldd,
                           const int *__restrict__ src_idx,
                           const int *__restrict__ dst_idx, int n_rows,
                           int64_t cols) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < (int64_t)n_rows * cols; i += stride) {
        const int64_t r = i / cols, c = i % cols;
        dst[(int64_t)dst_idx[r] * ldd + c] = src[(int64_t)src_idx[r] * lds + c];
    }
}



// ---------------------------------------------------------------------------
// panel column step: argmax + swap + scale + rank-1 on a col-major sub-panel
// ---------------------------------------------------------------------------
// One launch per column c of an nb-wide sub-panel held col-major in `cm`
// (ld = ldc, rows 0..m).  Matches LAPACK dgetrf partial pivoting: pivot =
// first row (smallest index) with max |value| in column c among rows c..m;
// swap full sub-panel rows c <-> piv; scale col c below diag by 1/pivot
// (multiply by reciprocal, as dscal does); rank-1 update cols c+1..nb.
//
// Inter-block protocol (cdna_hip_programming.md §6 G16, R1 form):
//   every block: phase-A local argmax over its rows -> sc1 payload stores ->
//   vmcnt drain -> relaxed-agent flag(epoch); block 0 polls all flags,
//   reduces with the first-max rule, performs the swap OUTSIDE the disputed
//   region, publishes both affected rows sc1 + flag; blocks then finish from
//   registers + the published slab (no plain re-reads of swapped data).
#define PANEL_TPB 256
// (rows per block is now a template parameter of k_panel_factor —
// QR*TPB, default 256x256 = 1 row/thread from the r02 shape sweep;
// panel_shape() below picks the instantiation)
#define PANEL_NB 32             // sub-panel width == register column budget

// --------------------------------------------------------------------------
// persistent sub-panel factorization (v2): ONE launch factors a whole
// nb(<=32)-wide sub-panel.  Each block owns QR*TPB rows, held in LDS for
// all nb columns; the only cross-block traffic per column is the slab
// handshake: every block publishes its candidate row (full nb values) and
// the block owning the diagonal row publishes it, so the row swap is
// performed by the OWNING blocks from slab data — no cross-block reads of
// matrix memory, no fences on the bulk (G16 R1: sc1 payload -> drain ->
// flag; consumers poll relaxed + read sc1).
// --------------------------------------------------------------------------
// All per-column slabs are DOUBLE-BUFFERED by column parity: a fast block
// may publish column c+1 while a slow one still reads column c (it cannot
// reach c+2's publish before every block published c+1, so two slots
// suffice).  Single-buffered slabs raced (old flag + new payload is
// observable: no ordering between one block's reads and another's writes).
//
// The per-block key is SELF-VALIDATING (G16 R2, "the data IS the flag"): the
// 64-bit pattern of the block's candidate |value| travels as two adjacent
// 8-byte granules, each tagged with the full 32-bit epoch,
//   key[par][b][0] = (epoch<<32) | hi32(bits),  key[par][b][1] = ... lo32,
// so one poll pass (two independent loads = one fabric trip) returns the
// value together with its validity and no dependent key read follows.  A
// stale slot (taller earlier panel, tournament panel, earlier factorization)
// carries an older epoch in BOTH granules and is rejected; the host's zero
// memset stays valid because epoch >= 1.  The winner's ROW INDEX is payload:
// it rides in a 17th 16-byte chunk of the block's candidate record.
#define PANEL_REC (PANEL_NB + 2)  // doubles per candidate record (272 B)
#define PANEL_GR_IDX (2 * PANEL_NB)     // granule holding the row index
#define PANEL_GR_REC (2 * PANEL_NB + 2)  // granules per R2 record (528 B)
struct PanelSync2 {
    alignas(16) unsigned long long key[2][CONFLUX_PANEL_MAX_BLOCKS][2];
    // candidate record: PANEL_NB row values, then one 16-byte chunk whose
    // first int is the candidate's (sub-panel-relative) row index
    alignas(16) double cand_row[2][CONFLUX_PANEL_MAX_BLOCKS][PANEL_REC];
    alignas(16) double diag_row[2][PANEL_NB];
    unsigned int err;
    // diagnostics: total key-poll iterations (all blocks, all columns) —
    // read+reset by conflux_panel_spin_stats (CONFLUX_SPIN_STATS=1)
    unsigned long long spin_sum;
    // ---- drain-free (R2) payload of k_panel_factor_reg: every double of a
    // candidate row / of the diagonal row travels as two self-validating
    // granules like the key, (epoch<<32)|hi32 and (epoch<<32)|lo32, each
    // written by ONE aligned 8-byte relaxed agent-scope store.  Granule
    // PANEL_GR_IDX of a block's record carries the winner's row index.  The
    // R1 slabs above stay: k_panel_factor (ragged leaves, mode 0) and the
    // register leaf's R1 form use them on the same struct within one
    // factorization, the epoch running on from launch to launch.
    alignas(16) unsigned long long
        cand_gr[2][CONFLUX_PANEL_MAX_BLOCKS][PANEL_GR_REC];
    alignas(16) unsigned long long diag_gr[2][2 * PANEL_NB];
    // diagnostics of the instrumented instantiations: shader-clock cycles
    // of wave 0 per column phase (poll wait, poll passed -> pivot and
    // diagonal row in LDS, barrier -> end of the row update and reduction,
    // combine -> key posted); [0..3] summed over all blocks, [4..7] block 0
    // alone.  Read and reset by conflux_panel_phase_read.
    unsigned long long phase[8];
};


typedef unsigned int __attribute__((address_space(1))) gu32;
typedef unsigned long long __attribute__((address_space(1))) gu64;
#define RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

DEVFN void st_rlx_u64(unsigned long long *p, unsigned long long v) {
    __hip_atomic_store((gu64 *)p, v, RLX_AGENT);
}
DEVFN unsigned long long ld_rlx_u64(const unsigned long long *p) {
    return __hip_atomic_load((const gu64 *)p, RLX_AGENT);
}
DEVFN void st_rlx_u32(unsigned int *p, unsigned int v) {
    __hip_atomic_store((gu32 *)p, v, RLX_AGENT);
}
DEVFN unsigned int ld_rlx_u32(const unsigned int *p) {
    return __hip_atomic_load((const gu32 *)p, RLX_AGENT);
}
DEVFN void st_rlx_f64(double *p, double v) {
    union { double d; unsigned long long u; } x;
    x.d = v;
    st_rlx_u64((unsigned long long *)p, x.u);
}
DEVFN double ld_rlx_f64(const double *p) {
    union { double d; unsigned long long u; } x;
    x.u = ld_rlx_u64((const unsigned long long *)p);
    return x.d;
}
DEVFN void drain_stores() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// Wave64 first-max reduction of a (|value|, index) pair on the DPP network
// (no LDS round trips): after wave_first_max() LANE 63 holds the pair with
// the largest value, the smallest index among equal values.  The fold is
// commutative and associative (values are never NaN here: a NaN never
// becomes a candidate), so the order of the DPP stages does not matter.  A
// lane whose DPP source is outside its row, or whose row is masked off,
// keeps its own pair and folds it with itself (a no-op).  All 64 lanes must
// be active.
template <int CTRL, int ROW_MASK>
DEVFN void dpp_fold_first_max(double &d, int &idx) {
    union { double d; int i[2]; } s, o;
    s.d = d;
    o.i[0] = __builtin_amdgcn_update_dpp(s.i[0], s.i[0], CTRL, ROW_MASK, 0xf,
                                         false);
    o.i[1] = __builtin_amdgcn_update_dpp(s.i[1], s.i[1], CTRL, ROW_MASK, 0xf,
                                         false);
    const int oi =
        __builtin_amdgcn_update_dpp(idx, idx, CTRL, ROW_MASK, 0xf, false);
    if (o.d > d || (o.d == d && oi < idx)) {
        d = o.d;
        idx = oi;
    }
}
DEVFN void wave_first_max(double &d, int &idx) {
    dpp_fold_first_max<0x111, 0xf>(d, idx);  // row_shr:1
    dpp_fold_first_max<0x112, 0xf>(d, idx);  // row_shr:2
    dpp_fold_first_max<0x114, 0xf>(d, idx);  // row_shr:4
    dpp_fold_first_max<0x118, 0xf>(d, idx);  // row_shr:8 -> lane 15 of a row
    dpp_fold_first_max<0x142, 0xa>(d, idx);  // row_bcast:15 into rows 1, 3
    dpp_fold_first_max<0x143, 0xc>(d, idx);  // row_bcast:31 into rows 2, 3
}

// instrumented instantiations: one block's four phase totals into the sync
// struct (lane 0 of wave 0; relaxed agent-scope adds, read by the host after
// the stream has drained)
DEVFN void panel_phase_add(PanelSync2 *sync, const unsigned long long (&ph)[4],
                           bool block0) {
    for (int i = 0; i < 4; ++i) {
        (void)__hip_atomic_fetch_add((gu64 *)&sync->phase[i], ph[i],
                                     RLX_AGENT);
        if (block0)
            (void)__hip_atomic_fetch_add((gu64 *)&sync->phase[4 + i], ph[i],
                                         RLX_AGENT);
    }
}

// Value-only edition for reductions whose index IS the lane: the wave's
// largest value by six DPP folds of one v_max_f64 each, returned uniform;
// the first lane holding it is then one ballot away, instead of carrying the
// index through two compares and three selects per fold.  Values are never
// NaN here either.  All 64 lanes must be active.
template <int CTRL, int ROW_MASK>
DEVFN void dpp_fold_max(double &d) {
    union { double d; int i[2]; } s, o;
    s.d = d;
    o.i[0] = __builtin_amdgcn_update_dpp(s.i[0], s.i[0], CTRL, ROW_MASK, 0xf,
                                         false);
    o.i[1] = __builtin_amdgcn_update_dpp(s.i[1], s.i[1], CTRL, ROW_MASK, 0xf,
                                         false);
    d = fmax(d, o.d);
}
DEVFN double wave_max(double d) {
    dpp_fold_max<0x111, 0xf>(d);
    dpp_fold_max<0x112, 0xf>(d);
    dpp_fold_max<0x114, 0xf>(d);
    dpp_fold_max<0x118, 0xf>(d);
    dpp_fold_max<0x142, 0xa>(d);
    dpp_fold_max<0x143, 0xc>(d);
    union { double d; int i[2]; } s, o;
    s.d = d;
    o.i[0] = __builtin_amdgcn_readlane(s.i[0], 63);
    o.i[1] = __builtin_amdgcn_readlane(s.i[1], 63);
    return o.d;
}

typedef int i32x4 __attribute__((ext_vector_type(4)));
union F64x2Bits {
    double d[2];
    i32x4 v;
};

// ---------------------------------------------------------------------------
// TRSM diagonal-block solvers (32-wide; the v%32!=0 fallback path and the
// sub-panel solve inside factor_panel — the whole-panel solves use the
// fused k_trsm_*_mfma kernels below)
// ---------------------------------------------------------------------------
// X (nb x N, row-major ld) <- L^{-1} X with L (nb x nb, ld ldl) unit-lower:
// thread j owns column j; column values kept in registers.
// cblas_dtrsm Left/Lower/NoTrans/Unit re-expression (conflux_opt.hpp:1539).
__global__ __launch_bounds__(256) void k_trsm_left_lower_unit32(
    const double *__restrict__ L, int64_t ldl, double *__restrict__ X,
    int64_t ldx, int nb, int64_t N) {
    __shared__ double sL[32][33];
    const int tid = threadIdx.x;
    for (int i = tid; i < nb * nb; i += 256) sL[i / nb][i % nb] = L[(i / nb) * ldl + i % nb];
    __syncthreads();
    const int64_t j = (int64_t)blockIdx.x * 256 + tid;
    if (j >= N) return;
    double x[32];
#pragma unroll
    for (int r = 0; r < 32; ++r) x[r] = (r < nb) ? X[r * ldx + j] : 0.0;
#pragma unroll
    for (int r = 1; r < 32; ++r) {
        double acc = x[r];
#pragma unroll
        for (int i = 0; i < r; ++i) acc -= sL[r][i] * x[i];
        if (r < nb) x[r] = acc;
    }
#pragma unroll
    for (int r = 0; r < 32; ++r)
        if (r < nb) X[r * ldx + j] = x[r];
}

// ---------------------------------------------------------------------------
// persistent sub-panel getrf: ONE launch factors the nb(<=32)-wide sub-panel
// with LAPACK partial pivoting (first-max rule).  Blocks own QR*TPB rows
// held in LDS for all nb columns; per column the only cross-block traffic is
// the slab handshake; the row swap is performed by the OWNING blocks from
// slab-published rows (no cross-block matrix reads, no write races).
// ---------------------------------------------------------------------------
template <int QR, int TPB, bool STATS = false>
                            // rows/block = QR*TPB; QR=1 halves the
                            // per-column local update (1 row/thread);
                            // TPB=256 gives 67 KB LDS (2 blocks/CU);
                            // STATS: wave 0 times the column's phases
                            // (PanelSync2::phase), default build has none
__global__ __launch_bounds__(TPB) void k_panel_factor(
    double *__restrict__ panel, int64_t ldp, int m, int nb,
    PanelSync2 *__restrict__ sync, int *__restrict__ ipiv,
    unsigned int epoch0, int nblocks, int *__restrict__ swap_dst,
    int *__restrict__ swap_src, int backoff) {
    constexpr int RPB = QR * TPB;
    const int tid = threadIdx.x, bid = blockIdx.x;
    const int r0 = bid * RPB + tid;
    __shared__ double rows[QR][TPB][PANEL_NB + 1];
    __shared__ double piv_lds[PANEL_NB];
    __shared__ double diag_lds[PANEL_NB];
    __shared__ double red_abs[TPB];
    __shared__ int red_row[TPB];
    __shared__ int sh_piv;  // winner's row, from the winner record
    // block 0 lane 0 composes the dlaswp row-permutation incrementally as
    // pivots are decided (replaces the separate k_swap_map launch):
    __shared__ int sm_base[PANEL_NB];
    __shared__ int sm_opos[PANEL_NB], sm_osrc[PANEL_NB];
    __shared__ int sm_novf;
    if (bid == 0 && tid == 0) {
        for (int i = 0; i < nb; ++i) sm_base[i] = i;
        sm_novf = 0;
    }
    const auto srsrc = __builtin_amdgcn_make_buffer_rsrc(
        (void *)sync, (short)0, (int)sizeof(PanelSync2), 0x00020000);

    unsigned long long spin_acc = 0;  // key-poll iterations (diagnostics)
    unsigned long long ph[4] = {0, 0, 0, 0}, pt0 = 0, pt1 = 0, pt2 = 0;
    // give-up bound of the key poll: a broken hand-off must end the kernel
    // in about two seconds (legitimate waits are well under a millisecond).
    // One poll pass costs the two granule loads' round trip to L2 plus the
    // backoff's s_sleep(k) = 64*k clocks ~= 27*k ns at 2.4 GHz.  The spin
    // diagnostic gives the pass time: ~14.1 M passes per N=16384
    // factorization over ~32 polling lanes x 16384 columns of ~7 us each
    // is ~27 passes per column, ~0.26 us per pass at k = 2, so the load
    // trip is ~200 ns:  passes = 2e9 ns / (200 + 27*k) ns  (~7.9 M at k=2;
    // a loaded fabric lengthens a pass, and with it the bound, by 1.5-3x).
    // factor_panel reads sync->err after every panel and reports the
    // column code.
    const unsigned sleep_k =
        backoff == 1 ? 1u : backoff == 2 ? 2u : backoff >= 4 ? 4u : 0u;
    const unsigned spin_limit = 2000000000u / (200u + 27u * sleep_k);
    for (int q = 0; q < QR; ++q) {
        const int r = r0 + q * TPB;
        for (int cc = 0; cc < nb; ++cc)
            rows[q][tid][cc] = (r < m) ? panel[(int64_t)r * ldp + cc] : 0.0;
    }

    // ---- cooperative publication of column pc's candidate: lanes 0-15
    // stream the winner row, lanes 16-31 the diag row, as 16-byte sc1
    // buffer stores.  The owning (thread, q) of any row r is computable
    // from r directly (r = bid*RPB + tid + q*TPB), so the publishing lanes
    // read the owner's LDS slot; all publishing lanes are wave 0, one wave
    // drain covers them, then lane 0 posts the two key granules (R2: the
    // granules carry the candidate |value| itself).  Lane 32 adds the
    // candidate's row index as the record's 17th chunk.  There is no diag
    // flag: the diagonal row pc is owned by block 0 (see the static_assert
    // below), block 0 stores it before the same drain that precedes its key,
    // and every block's lane 0 polls block 0's key — so the diag row is
    // visible to a block once its key poll has passed.
    static_assert(PANEL_NB <= RPB,
                  "diag row pc < nb <= PANEL_NB must lie in block 0");
    auto publish_col = [&](int pc, double wa, int wrow) {
        const unsigned int pep = epoch0 + (unsigned)pc;
        const int ppar = (int)(pep & 1u);
        const int rec_off =
            (int)offsetof(PanelSync2, cand_row) +
            (ppar * CONFLUX_PANEL_MAX_BLOCKS + bid) * PANEL_REC * 8;
        if (tid == 32) {
            i32x4 rv = {wrow, 0, 0, 0};
            __builtin_amdgcn_raw_buffer_store_b128(
                rv, srsrc, rec_off + PANEL_NB * 8, 0, /*sc1*/ 16);
        }
        if (tid < 16) {
            const int lrow = (wrow < m) ? wrow - bid * RPB : 0;
            const int wq = lrow >= TPB;
            const int wtid = lrow - wq * TPB;
            F64x2Bits x;
            x.d[0] = rows[wq][wtid][2 * tid];
            x.d[1] = rows[wq][wtid][2 * tid + 1];
            if (2 * tid < nb)
                __builtin_amdgcn_raw_buffer_store_b128(
                    x.v, srsrc, rec_off + 16 * tid, 0, /*sc1*/ 16);
        } else if (tid < 32 && pc >= bid * RPB &&
                   pc < (bid + 1) * RPB) {
            const int l = tid - 16;
            const int lrow = pc - bid * RPB;
            const int dq = lrow >= TPB;
            const int dtid = lrow - dq * TPB;
            F64x2Bits x;
            x.d[0] = rows[dq][dtid][2 * l];
            x.d[1] = rows[dq][dtid][2 * l + 1];
            if (2 * l < nb)
                __builtin_amdgcn_raw_buffer_store_b128(
                    x.v, srsrc,
                    (int)offsetof(PanelSync2, diag_row) +
                        ppar * PANEL_NB * 8 + 16 * l,
                    0, /*sc1*/ 16);
        }
        // ONE wave drain covers every payload store (all from wave 0), then
        // lane 0 posts the key: the full bit pattern of wa (the -1.0 "no
        // candidate" value and any NaN included), split over two granules
        // that each carry the epoch
        if (tid < 64) drain_stores();
        if (tid == 0) {
            union { double d; unsigned long long u; } a;
            a.d = wa;
            const unsigned long long tag = (unsigned long long)pep << 32;
            st_rlx_u64(&sync->key[ppar][bid][0], tag | (a.u >> 32));
            st_rlx_u64(&sync->key[ppar][bid][1], tag | (a.u & 0xffffffffull));
        }
    };
    // combine the four per-wave partials (redundantly on wave 0's lanes)
    auto combine_partials = [&](double &wa, int &wrow) {
        wa = red_abs[0];
        wrow = red_row[0];
        for (int wv = 1; wv < TPB / 64; ++wv) {
            const double oa = red_abs[wv];
            const int orr = red_row[wv];
            if (oa > wa || (oa == wa && orr < wrow)) { wa = oa; wrow = orr; }
        }
    };
    // per-wave DPP reduction + LDS partial write of a (|value|, row) pair
    auto reduce_to_partials = [&](double amax, int arow) {
        wave_first_max(amax, arow);
        if ((tid & 63) == 63) {
            red_abs[tid >> 6] = amax;
            red_row[tid >> 6] = arow;
        }
    };

    // column 0's candidate: first-max over own rows, then publish.  Every
    // later column's candidate is reduced and published at the TAIL of the
    // previous column's update (the values are final there), so a column
    // step starts directly at the key poll — one barrier and one LDS read
    // pass fewer per column.
    {
        double amax = -1.0;
        int arow = m;
        for (int q = 0; q < QR; ++q) {
            const int r = r0 + q * TPB;
            if (r >= 0 && r < m) {
                const double a = fabs(rows[q][tid][0]);
                if (a > amax || (a == amax && r < arow)) { amax = a; arow = r; }
            }
        }
        reduce_to_partials(amax, arow);
        __syncthreads();
        double wa;
        int wrow;
        combine_partials(wa, wrow);
        publish_col(0, wa, wrow);
    }

    for (int c = 0; c < nb; ++c) {
        const unsigned int epoch = epoch0 + (unsigned)c;
        const int par = (int)(epoch & 1u);  // slab parity slot
        const int diag_off =
            (int)offsetof(PanelSync2, diag_row) + par * PANEL_NB * 8;

        // ---- EVERY block reduces the global winner itself (redundant,
        // deterministic): lane b polls block b's two key granules until
        // both carry this column's epoch, rebuilds the |value| from them,
        // then one wave reduction with the first-max rule.  Saves the
        // central reducer's publish round trip.  Per-column critical chain
        // (three fabric trips): publisher's drain -> key granules visible
        // to the poll -> winner record + diag row read.
        //
        // Tie-break: this RELIES on blocks owning contiguous ascending row
        // ranges [bid*RPB, (bid+1)*RPB) (r0 = bid*RPB + tid, + q*TPB, for
        // every QR/TPB shape) and on each block's candidate being its own
        // first max: then "smaller row wins" between blocks is "smaller
        // block index wins" — the row index is not needed for the
        // reduction and arrives with the winner record.  A row-cyclic
        // block layout would need the row back in the key.
        if (tid < 64) {
            if constexpr (STATS) pt0 = clock64();
            double a_d = -1.0;
            int a_win = 0;
            for (int b = tid; b < nblocks; b += 64) {
                unsigned long long g0, g1;
                unsigned spins = 0;
                for (;;) {
                    // two independent loads: one trip per pass
                    g0 = ld_rlx_u64(&sync->key[par][b][0]);
                    g1 = ld_rlx_u64(&sync->key[par][b][1]);
                    if ((unsigned)(g0 >> 32) == epoch &&
                        (unsigned)(g1 >> 32) == epoch)
                        break;
                    if (backoff == 1) __builtin_amdgcn_s_sleep(1);
                    else if (backoff == 2) __builtin_amdgcn_s_sleep(2);
                    else if (backoff >= 4) __builtin_amdgcn_s_sleep(4);
                    if (++spins > spin_limit) {
                        st_rlx_u32(&sync->err, 1u + (unsigned)c);
                        break;
                    }
                }
                spin_acc += spins;
                union { double d; unsigned long long u; } a;
                a.u = (g0 << 32) | (g1 & 0xffffffffull);
                // b ascends per lane: strictly-greater keeps the lower block
                if (a.d > a_d) {
                    a_d = a.d;
                    a_win = b;
                }
            }
            // lanes >= nblocks still hold the (-1.0, 0) start value, which
            // never replaces a real candidate
            wave_first_max(a_d, a_win);
            if constexpr (STATS) pt1 = clock64();
            // the polling wave is the loading wave: broadcast the winner and
            // issue the payload loads at once (no LDS round + barrier in
            // between).  The wavefront-scope fence emits no instruction; it
            // keeps the compiler from moving the sc1 loads above the poll.
            const int win = __builtin_amdgcn_readlane(a_win, 63);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            i32x4 rec = {0, 0, 0, 0};
            if (tid == 16 || (tid < 16 && 2 * tid < nb))
                rec = __builtin_amdgcn_raw_buffer_load_b128(
                    srsrc,
                    (int)offsetof(PanelSync2, cand_row) +
                        (par * CONFLUX_PANEL_MAX_BLOCKS + win) * PANEL_REC *
                            8 +
                        16 * tid,
                    0, /*sc1*/ 16);
            if (tid < 16 && 2 * tid < nb) {
                F64x2Bits x;
                x.v = rec;
                piv_lds[2 * tid] = x.d[0];
                piv_lds[2 * tid + 1] = x.d[1];
                x.v = __builtin_amdgcn_raw_buffer_load_b128(
                    srsrc, diag_off + 16 * tid, 0, /*sc1*/ 16);
                diag_lds[2 * tid] = x.d[0];
                diag_lds[2 * tid + 1] = x.d[1];
            }
            // lane 16 holds the record's 17th chunk: the winner's row
            const int w_row = __builtin_amdgcn_readlane(rec[0], 16);
            if (tid == 0) {
                sh_piv = w_row;
                if (bid == 0) {
                    ipiv[c] = w_row;
                    // compose the swap (c <-> w_row) into the row map
                    int *b;
                    if (w_row < nb) {
                        b = &sm_base[w_row];
                    } else {
                        int j = 0;
                        for (; j < sm_novf && sm_opos[j] != w_row; ++j) {
                        }
                        if (j == sm_novf) {
                            sm_opos[j] = w_row;
                            sm_osrc[j] = w_row;
                            ++sm_novf;
                        }
                        b = &sm_osrc[j];
                    }
                    const int t = sm_base[c];
                    sm_base[c] = *b;
                    *b = t;
                }
            }
        }
        __syncthreads();
        if constexpr (STATS)
            if (tid < 64) pt2 = clock64();
        const int piv = sh_piv;
        const double pivval = piv_lds[c];
        const bool do_scale = pivval != 0.0;
        const double recip = do_scale ? 1.0 / pivval : 0.0;

        // ---- update own rows; track the next column's candidate inline --
        double namax = -1.0;
        int narow = m;
        for (int q = 0; q < QR; ++q) {
            const int r = r0 + q * TPB;
            if (r >= m) continue;
            double *my = rows[q][tid];
            if (r == c) {
                for (int cc = 0; cc < nb; ++cc) my[cc] = piv_lds[cc];
            } else if (r == piv) {
                for (int cc = 0; cc < c; ++cc) my[cc] = diag_lds[cc];
                const double v0 = diag_lds[c];
                const double l = do_scale ? v0 * recip : v0;
                my[c] = l;
                for (int cc = c + 1; cc < nb; ++cc)
                    my[cc] = diag_lds[cc] - l * piv_lds[cc];
            } else if (r > c) {
                const double l = do_scale ? my[c] * recip : my[c];
                my[c] = l;
                for (int cc = c + 1; cc < nb; ++cc)
                    my[cc] -= l * piv_lds[cc];
            }
            // candidates for column c+1 are exactly the rows updated above
            if (r > c && c + 1 < nb) {
                const double a = fabs(my[c + 1]);
                if (a > namax || (a == namax && r < narow)) {
                    namax = a;
                    narow = r;
                }
            }
        }
        if (c + 1 < nb) reduce_to_partials(namax, narow);
        __syncthreads();
        unsigned long long pt3 = 0;
        if constexpr (STATS)
            if (tid < 64) pt3 = clock64();
        if (c + 1 < nb) {
            // tail-publish column c+1's candidate (values final after the
            // barrier above; the publish overlaps other blocks' update
            // tails instead of gating the next column's start)
            double wa;
            int wrow;
            combine_partials(wa, wrow);
            publish_col(c + 1, wa, wrow);
        }
        if constexpr (STATS)
            if (tid < 64) {
                ph[0] += pt1 - pt0;
                ph[1] += pt2 - pt1;
                ph[2] += pt3 - pt2;
                ph[3] += clock64() - pt3;
            }
    }
    if constexpr (STATS)
        if (tid == 0) panel_phase_add(sync, ph, bid == 0);

    // write back (plain stores; next kernels see them at the launch boundary)
    for (int q = 0; q < QR; ++q) {
        const int r = r0 + q * TPB;
        if (r >= m) continue;
        for (int cc = 0; cc < nb; ++cc)
            panel[(int64_t)r * ldp + cc] = rows[q][tid][cc];
    }
    // spin diagnostics: wave-0 lanes aggregated, one atomicAdd per block
    if (tid < 64) {
        unsigned long long t = spin_acc;
        for (int w2 = 32; w2 > 0; w2 >>= 1) t += __shfl_down(t, w2);
        if (tid == 0 && t)
            (void)__hip_atomic_fetch_add((gu64 *)&sync->spin_sum, t,
                                         RLX_AGENT);
    }
    // block 0: emit the composed row-permutation map (identity-padded by
    // duplicating entry 0 — benign identical concurrent writes downstream).
    // sm_* visibility: lane 0's last update precedes the column loop's
    // closing __syncthreads, so no extra barrier (and none would be legal
    // in this divergent tail).
    if (bid == 0 && tid < 2 * PANEL_NB && swap_dst) {
        const int i = tid;
        int d, sv;
        if (i < nb) {
            d = i;
            sv = sm_base[i];
        } else if (i - nb < sm_novf) {
            d = sm_opos[i - nb];
            sv = sm_osrc[i - nb];
        } else {
            d = 0;
            sv = sm_base[0];
        }
        if (i < 2 * nb) {
            swap_dst[i] = d;
            swap_src[i] = sv;
        }
    }
}

// ---------------------------------------------------------------------------
// register-resident leaf: k_panel_factor for full 32-column sub-panels with
// the thread's row held in 32 fp64 registers from load to write-back
// (CONFLUX_PANEL_REG, default 1; 256 rows per block, one row per thread).
// Pivots, factors and the swap map are bit for bit k_panel_factor's: the
// same first-max rule, recip = 1.0 / pivot by IEEE division, l = x * recip,
// one explicit fma(-l, piv[cc], x) per update.
//
// Register arrays need compile-time indices, so the arithmetic of a column
// is panel_reg_column<C>, reached through a 32-way switch inside the ROLLED
// column loop; the poll, the reductions and the publication are shared code.
// LDS holds only what is shared: the pivot row and the diagonal row (read
// back as uniform broadcast reads, 16 bytes at a time), the per-wave
// partials, the winner's row and the staging slots of the publication.
// Block 0's swap map lives in registers of its wave 0 (see below), and the
// wave reductions are one v_max_f64 per DPP fold plus a ballot (the row, or
// the block, IS the lane).
//
// Publication.  The rows no longer sit in LDS where wave 0 could fetch the
// block's winner, and the block's winner is known only after the column's
// second barrier.  So BEFORE that barrier every wave stages its OWN
// candidate row (the lane that owns the wave's first-max writes its 32
// registers to stage[wave]), and block 0's lane c+1 stages the next diagonal
// row (rows 0..31 all live in wave 0 of block 0).  After the barrier wave 0
// combines the four partials, reads stage[winner's wave] and publishes — so,
// as in k_panel_factor, EVERY hand-off store of a block is issued by wave 0.
// Ordering, R1 form (PUBLISH = 0): all payload stores are sc1 stores of one
// wave, that wave drains (vmcnt(0)), then its lane 0 posts the key; no
// second storing wave exists, so no cross-wave ordering is needed beyond the
// barrier that already orders the LDS staging.  R2 form (PUBLISH = 1): the
// payload travels as self-validating granules (PanelSync2::cand_gr /
// diag_gr), payload and key are issued back to back with NO drain, and the
// consumer re-reads its granules until every tag carries the column's epoch
// (bounded like the key poll; err code 0x10000 + 1 + column).  R2 is not
// offered for k_panel_factor: it keeps the R1 slabs.
// Resources (gfx950 code object metadata, PUBLISH 0 / 1): 157 / 165 VGPRs,
// 1848 B LDS, no scratch, no spilled VGPRs, 22.9 / 23.4 KB of code.  Above 128
// registers two 256-thread blocks fit a CU: the same 2 blocks per CU and 256
// rows per block as k_panel_factor's default shape, so
// conflux_panel_blocks_per_cu() and conflux_panel_rpb() serve both.
// ---------------------------------------------------------------------------
#define PANEL_REG_TPB 256
typedef double f64x2 __attribute__((ext_vector_type(2)));

// column C of one thread's row: scale by the reciprocal and rank-1 update
// for rows below C.  Only this part indexes the register row by the column,
// so only this part is instantiated 32 times; the two swap cases are
// column-independent copies around it (see the column loop).  Returns the
// value column C+1's candidate is taken from.
template <int C>
DEVFN double panel_reg_column(double (&my)[PANEL_NB], const double *piv_lds,
                              int r) {
    const double pivval = piv_lds[C];
    const bool do_scale = pivval != 0.0;
    const double recip = do_scale ? 1.0 / pivval : 0.0;
    if (r > C) {
        const double l = do_scale ? my[C] * recip : my[C];
        my[C] = l;
#pragma unroll
        for (int cc = C + 1; cc < PANEL_NB; ++cc)
            my[cc] = fma(-l, piv_lds[cc], my[cc]);
    }
    if constexpr (C + 1 < PANEL_NB) return my[C + 1];
    else return 0.0;
}

template <bool R2, bool STATS>
__global__ __launch_bounds__(PANEL_REG_TPB) void k_panel_factor_reg(
    double *__restrict__ panel, int64_t ldp, int m,
    PanelSync2 *__restrict__ sync, int *__restrict__ ipiv,
    unsigned int epoch0, int nblocks, int *__restrict__ swap_dst,
    int *__restrict__ swap_src, int backoff) {
    constexpr int TPB = PANEL_REG_TPB, NB = PANEL_NB, NW = TPB / 64;
    const int tid = threadIdx.x, bid = blockIdx.x;
    const int lane = tid & 63, wv = tid >> 6;
    const int r = bid * TPB + tid;
    const bool owns_c = bid == 0 && wv == 0;  // rows 0..31: wave 0, block 0
    __shared__ alignas(16) double piv_lds[NB];
    __shared__ alignas(16) double diag_lds[NB];
    __shared__ alignas(16) double stage[NW][NB];  // each wave's candidate row
    __shared__ alignas(16) double stage_d[NB];    // block 0: next diag row
    __shared__ double red_abs[NW];
    __shared__ int red_row[NW];
    __shared__ int sh_piv;
    // the dlaswp row map k_panel_factor composes in LDS with lane 0 walking
    // the overflow list (one dependent LDS read per entry, on block 0's
    // critical path between its poll and the block barrier: the r06 phase
    // split shows block 0 spending 3.4x the other blocks' time there) lives
    // in REGISTERS of block 0's wave 0 here: lane i holds sm_base[i] and
    // overflow entry i; the list search is one ballot, every read a
    // readlane with a uniform index.  Same map, entry for entry.
    int sm_base_r = tid, sm_opos_r = 0, sm_osrc_r = 0, sm_novf = 0;
    const auto srsrc = __builtin_amdgcn_make_buffer_rsrc(
        (void *)sync, (short)0, (int)sizeof(PanelSync2), 0x00020000);
    unsigned long long spin_acc = 0;
    unsigned long long ph[4] = {0, 0, 0, 0}, pt0 = 0, pt1 = 0, pt2 = 0;
    // give-up bound: as in k_panel_factor
    const unsigned sleep_k =
        backoff == 1 ? 1u : backoff == 2 ? 2u : backoff >= 4 ? 4u : 0u;
    const unsigned spin_limit = 2000000000u / (200u + 27u * sleep_k);
    auto backoff_sleep = [&]() {
        if (backoff == 1) __builtin_amdgcn_s_sleep(1);
        else if (backoff == 2) __builtin_amdgcn_s_sleep(2);
        else if (backoff >= 4) __builtin_amdgcn_s_sleep(4);
    };

    // ---- load: 16 x 16 bytes, 256 contiguous bytes per row
    double my[NB];
    if (r < m) {
        const f64x2 *src = (const f64x2 *)(panel + (int64_t)r * ldp);
#pragma unroll
        for (int k = 0; k < NB / 2; ++k) {
            const f64x2 t = src[k];
            my[2 * k] = t.x;
            my[2 * k + 1] = t.y;
        }
    } else {
#pragma unroll
        for (int cc = 0; cc < NB; ++cc) my[cc] = 0.0;
    }
    auto stage_row = [&](double *dst) {
#pragma unroll
        for (int k = 0; k < NB / 2; ++k) {
            f64x2 t;
            t.x = my[2 * k];
            t.y = my[2 * k + 1];
            ((f64x2 *)dst)[k] = t;
        }
    };
    // per-wave first-max of the threads' candidates (amax = |value|, or
    // -1.0 without one): rows ascend with the lane, so the first lane that
    // holds the wave's maximum is the first-max row.  Lane 0 writes the
    // wave's partial, the lane owning the wave's winner stages its row,
    // block 0's lane dcol stages the diagonal row dcol
    auto reduce_and_stage = [&](double amax, int dcol) {
        const double mx = wave_max(amax);
        const unsigned long long hit =
            __builtin_amdgcn_ballot_w64(amax == mx);
        const int wrow_w = mx > -1.0
                               ? bid * TPB + wv * 64 + (int)__builtin_ctzll(hit)
                               : m;
        if (lane == 0) {
            red_abs[wv] = mx;
            red_row[wv] = wrow_w;
        }
        if (wrow_w < m && r == wrow_w) stage_row(stage[wv]);
        // A block without any candidate publishes stage[0]; it wins only
        // when NO block has one (every remaining entry of the column is a
        // NaN).  k_panel_factor publishes the block's first row as it stands
        // then, so a wave 0 without a candidate stages that row: the two
        // kernels return the same bits on such input too.  Ordinary data
        // never takes this branch.
        if (wv == 0 && wrow_w >= m && lane == 0) stage_row(stage[0]);
        if (owns_c && tid == dcol) stage_row(stage_d);
    };
    // wave 0 only, after the barrier that follows reduce_and_stage
    auto combine_partials = [&](double &wa, int &wrow) {
        wa = red_abs[0];
        wrow = red_row[0];
        for (int w = 1; w < NW; ++w) {
            const double oa = red_abs[w];
            const int orr = red_row[w];
            if (oa > wa || (oa == wa && orr < wrow)) { wa = oa; wrow = orr; }
        }
    };
    // wave 0 only: publish column pc's candidate record (+ block 0: the
    // diagonal row pc) and post the key.  A block without a candidate
    // (wa = -1.0) publishes stage[0], its first row (see reduce_and_stage):
    // it wins only when no block has a candidate.
    auto publish_col = [&](int pc, double wa, int wrow) {
        const unsigned int pep = epoch0 + (unsigned)pc;
        const int ppar = (int)(pep & 1u);
        const int wwave = wrow < m ? (wrow - bid * TPB) >> 6 : 0;
        const unsigned long long tag = (unsigned long long)pep << 32;
        union { double d; unsigned long long u; } a;
        if constexpr (R2) {
            // lanes 0-31: the two granules of one double of the candidate
            // row; block 0's lanes 32-63: of the diagonal row.  Each granule
            // is ONE aligned 8-byte atomic store; no drain before the key.
            if (tid < 32) {
                a.d = stage[wwave][tid];
                unsigned long long *g = &sync->cand_gr[ppar][bid][2 * tid];
                st_rlx_u64(g, tag | (a.u >> 32));
                st_rlx_u64(g + 1, tag | (a.u & 0xffffffffull));
            } else if (bid == 0) {
                a.d = stage_d[tid - 32];
                unsigned long long *g = &sync->diag_gr[ppar][2 * (tid - 32)];
                st_rlx_u64(g, tag | (a.u >> 32));
                st_rlx_u64(g + 1, tag | (a.u & 0xffffffffull));
            }
            if (tid == 0)
                st_rlx_u64(&sync->cand_gr[ppar][bid][PANEL_GR_IDX],
                           tag | (unsigned long long)(unsigned)wrow);
        } else {
            const int rec_off =
                (int)offsetof(PanelSync2, cand_row) +
                (ppar * CONFLUX_PANEL_MAX_BLOCKS + bid) * PANEL_REC * 8;
            if (tid == 32) {
                i32x4 rv = {wrow, 0, 0, 0};
                __builtin_amdgcn_raw_buffer_store_b128(
                    rv, srsrc, rec_off + NB * 8, 0, /*sc1*/ 16);
            }
            if (tid < 16) {
                F64x2Bits x;
                x.d[0] = stage[wwave][2 * tid];
                x.d[1] = stage[wwave][2 * tid + 1];
                __builtin_amdgcn_raw_buffer_store_b128(
                    x.v, srsrc, rec_off + 16 * tid, 0, /*sc1*/ 16);
            } else if (tid < 32 && bid == 0) {
                const int l = tid - 16;
                F64x2Bits x;
                x.d[0] = stage_d[2 * l];
                x.d[1] = stage_d[2 * l + 1];
                __builtin_amdgcn_raw_buffer_store_b128(
                    x.v, srsrc,
                    (int)offsetof(PanelSync2, diag_row) + ppar * NB * 8 +
                        16 * l,
                    0, /*sc1*/ 16);
            }
            // R1: the one storing wave drains, then posts the key
            drain_stores();
        }
        if (tid == 0) {
            a.d = wa;
            st_rlx_u64(&sync->key[ppar][bid][0], tag | (a.u >> 32));
            st_rlx_u64(&sync->key[ppar][bid][1], tag | (a.u & 0xffffffffull));
        }
    };

    // column 0's candidate; every later one is reduced and published at the
    // tail of the previous column's update
    {
        // (a NaN is never a candidate: the comparison is false for it)
        double amax = -1.0;
        if (r < m && fabs(my[0]) > -1.0) amax = fabs(my[0]);
        reduce_and_stage(amax, 0);
        __syncthreads();
        if (tid < 64) {
            double wa;
            int wrow;
            combine_partials(wa, wrow);
            publish_col(0, wa, wrow);
        }
    }

    for (int c = 0; c < NB; ++c) {
        const unsigned int epoch = epoch0 + (unsigned)c;
        const int par = (int)(epoch & 1u);
        // ---- wave 0 of EVERY block: poll all keys, reduce the winner
        // (lower block wins ties: blocks own ascending row ranges), fetch the
        // winner's record and the diagonal row into LDS
        if (tid < 64) {
            if constexpr (STATS) pt0 = clock64();
            double a_d = -1.0;
            int a_win = 0;
            for (int b = tid; b < nblocks; b += 64) {
                unsigned long long g0, g1;
                unsigned spins = 0;
                for (;;) {
                    g0 = ld_rlx_u64(&sync->key[par][b][0]);
                    g1 = ld_rlx_u64(&sync->key[par][b][1]);
                    if ((unsigned)(g0 >> 32) == epoch &&
                        (unsigned)(g1 >> 32) == epoch)
                        break;
                    backoff_sleep();
                    if (++spins > spin_limit) {
                        st_rlx_u32(&sync->err, 1u + (unsigned)c);
                        break;
                    }
                }
                spin_acc += spins;
                union { double d; unsigned long long u; } a;
                a.u = (g0 << 32) | (g1 & 0xffffffffull);
                if (a.d > a_d) {
                    a_d = a.d;
                    a_win = b;
                }
            }
            // up to 64 blocks lane b polled block b alone: first lane with
            // the largest key; more blocks: the (value, index) fold
            int win;
            if (nblocks <= 64) {
                const double mx = wave_max(a_d);
                win = (int)__builtin_ctzll(
                    __builtin_amdgcn_ballot_w64(a_d == mx));
            } else {
                wave_first_max(a_d, a_win);
                win = __builtin_amdgcn_readlane(a_win, 63);
            }
            if constexpr (STATS) pt1 = clock64();
            int w_row;
            if constexpr (R2) {
                // lane i: double i of the winner's record, lane 32+i: double
                // i of the diagonal row, every lane: the row-index granule.
                // Re-read until every tag is this column's epoch (normally
                // the first pass: the key was posted after the payload).
                const unsigned long long *src =
                    tid < 32 ? &sync->cand_gr[par][win][2 * tid]
                             : &sync->diag_gr[par][2 * (tid - 32)];
                const unsigned long long *isrc =
                    &sync->cand_gr[par][win][PANEL_GR_IDX];
                unsigned long long g0, g1, gi;
                unsigned spins = 0;
                for (;;) {
                    g0 = ld_rlx_u64(src);
                    g1 = ld_rlx_u64(src + 1);
                    gi = ld_rlx_u64(isrc);
                    const bool stale = (unsigned)(g0 >> 32) != epoch ||
                                       (unsigned)(g1 >> 32) != epoch ||
                                       (unsigned)(gi >> 32) != epoch;
                    if (__builtin_amdgcn_ballot_w64(stale) == 0ull) break;
                    backoff_sleep();
                    if (++spins > spin_limit) {
                        if (tid == 0)
                            st_rlx_u32(&sync->err,
                                       0x10000u + 1u + (unsigned)c);
                        break;
                    }
                }
                spin_acc += tid == 0 ? spins : 0u;
                union { double d; unsigned long long u; } a;
                a.u = (g0 << 32) | (g1 & 0xffffffffull);
                if (tid < 32) piv_lds[tid] = a.d;
                else diag_lds[tid - 32] = a.d;
                w_row = __builtin_amdgcn_readfirstlane((int)(unsigned)gi);
            } else {
                // R1: sc1 loads behind the poll, as in k_panel_factor
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                i32x4 rec = {0, 0, 0, 0};
                if (tid <= 16)
                    rec = __builtin_amdgcn_raw_buffer_load_b128(
                        srsrc,
                        (int)offsetof(PanelSync2, cand_row) +
                            (par * CONFLUX_PANEL_MAX_BLOCKS + win) *
                                PANEL_REC * 8 +
                            16 * tid,
                        0, /*sc1*/ 16);
                if (tid < 16) {
                    F64x2Bits x;
                    x.v = rec;
                    piv_lds[2 * tid] = x.d[0];
                    piv_lds[2 * tid + 1] = x.d[1];
                    x.v = __builtin_amdgcn_raw_buffer_load_b128(
                        srsrc,
                        (int)offsetof(PanelSync2, diag_row) + par * NB * 8 +
                            16 * tid,
                        0, /*sc1*/ 16);
                    diag_lds[2 * tid] = x.d[0];
                    diag_lds[2 * tid + 1] = x.d[1];
                }
                w_row = __builtin_amdgcn_readlane(rec[0], 16);
            }
            if (tid == 0) {
                sh_piv = w_row;
                if (bid == 0) ipiv[c] = w_row;
            }
            if (bid == 0) {
                // compose the swap (c <-> w_row) into the row map; w_row, c,
                // j and sm_novf are wave-uniform, all 64 lanes are active
                int bval, j = 0;
                if (w_row < NB) {
                    bval = __builtin_amdgcn_readlane(sm_base_r, w_row);
                } else {
                    const unsigned long long hit = __builtin_amdgcn_ballot_w64(
                        tid < sm_novf && sm_opos_r == w_row);
                    if (hit) {
                        j = __builtin_ctzll(hit);
                    } else {
                        j = sm_novf;
                        if (tid == j) {
                            sm_opos_r = w_row;
                            sm_osrc_r = w_row;
                        }
                        ++sm_novf;
                    }
                    bval = __builtin_amdgcn_readlane(sm_osrc_r, j);
                }
                const int t = __builtin_amdgcn_readlane(sm_base_r, c);
                if (tid == c) sm_base_r = bval;
                if (w_row < NB) {
                    if (tid == w_row) sm_base_r = t;
                } else if (tid == j) {
                    sm_osrc_r = t;
                }
            }
        }
        __syncthreads();
        if constexpr (STATS)
            if (tid < 64) pt2 = clock64();
        const int piv = sh_piv;

        // ---- the column's arithmetic on the register row
        double nxt = 0.0;
#define PANEL_REG_CASE(C)                                                     \
    case C:                                                                   \
        nxt = panel_reg_column<C>(my, piv_lds, r);                            \
        break;
        // the pivot's old row (below c) takes the diagonal row: load it
        // over the register row and let the normal path scale and update
        // it — columns below c copied, column c scaled, the rest
        // fma(-l, piv[cc], diag[cc]), exactly k_panel_factor's r == piv
        // arithmetic.  One wave per column pays this branch.
        if (r == piv && r > c) {
#pragma unroll
            for (int k = 0; k < NB / 2; ++k) {
                const f64x2 t = ((const f64x2 *)diag_lds)[k];
                my[2 * k] = t.x;
                my[2 * k + 1] = t.y;
            }
        }
        switch (c) {
            PANEL_REG_CASE(0) PANEL_REG_CASE(1) PANEL_REG_CASE(2)
            PANEL_REG_CASE(3) PANEL_REG_CASE(4) PANEL_REG_CASE(5)
            PANEL_REG_CASE(6) PANEL_REG_CASE(7) PANEL_REG_CASE(8)
            PANEL_REG_CASE(9) PANEL_REG_CASE(10) PANEL_REG_CASE(11)
            PANEL_REG_CASE(12) PANEL_REG_CASE(13) PANEL_REG_CASE(14)
            PANEL_REG_CASE(15) PANEL_REG_CASE(16) PANEL_REG_CASE(17)
            PANEL_REG_CASE(18) PANEL_REG_CASE(19) PANEL_REG_CASE(20)
            PANEL_REG_CASE(21) PANEL_REG_CASE(22) PANEL_REG_CASE(23)
            PANEL_REG_CASE(24) PANEL_REG_CASE(25) PANEL_REG_CASE(26)
            PANEL_REG_CASE(27) PANEL_REG_CASE(28) PANEL_REG_CASE(29)
            PANEL_REG_CASE(30) PANEL_REG_CASE(31)
        }
#undef PANEL_REG_CASE
        // row c takes the pivot row in all 32 columns: a select, and only in
        // the wave that holds rows 0..31 (a wave-uniform branch)
        if (owns_c) {
            const bool is_c = r == c;
#pragma unroll
            for (int cc = 0; cc < NB; ++cc)
                my[cc] = is_c ? piv_lds[cc] : my[cc];
        }
        // candidates for column c+1 are exactly the rows updated above
        if (c + 1 < NB) {
            double namax = -1.0;
            if (r > c && r < m && fabs(nxt) > -1.0) namax = fabs(nxt);
            reduce_and_stage(namax, c + 1);
        }
        __syncthreads();
        unsigned long long pt3 = 0;
        if constexpr (STATS)
            if (tid < 64) pt3 = clock64();
        if (c + 1 < NB && tid < 64) {
            double wa;
            int wrow;
            combine_partials(wa, wrow);
            publish_col(c + 1, wa, wrow);
        }
        if constexpr (STATS)
            if (tid < 64) {
                ph[0] += pt1 - pt0;
                ph[1] += pt2 - pt1;
                ph[2] += pt3 - pt2;
                ph[3] += clock64() - pt3;
            }
    }
    if constexpr (STATS)
        if (tid == 0) panel_phase_add(sync, ph, bid == 0);

    // ---- write back: 16 x 16 bytes per row
    if (r < m) {
        f64x2 *dst = (f64x2 *)(panel + (int64_t)r * ldp);
#pragma unroll
        for (int k = 0; k < NB / 2; ++k) {
            f64x2 t;
            t.x = my[2 * k];
            t.y = my[2 * k + 1];
            dst[k] = t;
        }
    }
    if (tid < 64) {
        unsigned long long t = spin_acc;
        for (int w2 = 32; w2 > 0; w2 >>= 1) t += __shfl_down(t, w2);
        if (tid == 0 && t)
            (void)__hip_atomic_fetch_add((gu64 *)&sync->spin_sum, t,
                                         RLX_AGENT);
    }
    // block 0: emit the composed row-permutation map in k_panel_factor's
    // layout (identity-padded by duplicating entry 0): lane k writes entry k
    // and overflow entry k
    if (bid == 0 && tid < 64 && swap_dst) {
        const int base0 = __builtin_amdgcn_readlane(sm_base_r, 0);
        if (tid < NB) {
            const bool used = tid < sm_novf;
            swap_dst[tid] = tid;
            swap_src[tid] = sm_base_r;
            swap_dst[NB + tid] = used ? sm_opos_r : 0;
            swap_src[NB + tid] = used ? sm_osrc_r : base0;
        }
    }
}

// X (M x nb, row-major ld) <- X U^{-1} with U (nb x nb, ld ldu) upper
// non-unit: 256 rows per block staged through LDS (coalesced), thread r owns
// row r.  cblas_dtrsm Right/Upper/NoTrans/NonUnit (conflux_opt.hpp:1347).
__global__ __launch_bounds__(256) void k_trsm_right_upper32(
    const double *__restrict__ U, int64_t ldu, double *__restrict__ X,
    int64_t ldx, int nb, int64_t M, int trans) {
    __shared__ double sU[32][33];
    __shared__ double sX[256][33];
    const int tid = threadIdx.x;
    // trans: sU[i][c] = U[c][i] — solves X*L^T = B for lower-triangular L
    // (cblas_dtrsm Right/Lower/Trans/NonUnit, reference Cholesky.cpp:280)
    for (int i = tid; i < nb * nb; i += 256)
        sU[i / nb][i % nb] = trans ? U[(i % nb) * ldu + i / nb]
                                   : U[(i / nb) * ldu + i % nb];
    const int64_t r0 = (int64_t)blockIdx.x * 256;
    const int rows = (int)min((int64_t)256, M - r0);
    // stage rows r0..r0+rows coalesced: thread t covers elements t, t+256, ...
    for (int i = tid; i < rows * nb; i += 256) sX[i / nb][i % nb] = X[(r0 + i / nb) * ldx + i % nb];
    __syncthreads();
    if (tid < rows) {
        double x[32];
#pragma unroll
        for (int c = 0; c < 32; ++c) x[c] = (c < nb) ? sX[tid][c] : 0.0;
#pragma unroll
        for (int c = 0; c < 32; ++c) {
            double acc = x[c];
#pragma unroll
            for (int i = 0; i < c; ++i) acc -= x[i] * sU[i][c];
            if (c < nb) x[c] = acc / sU[c][c];
        }
#pragma unroll
        for (int c = 0; c < 32; ++c)
            if (c < nb) sX[tid][c] = x[c];
    }
    __syncthreads();
    for (int i = tid; i < rows * nb; i += 256) X[(r0 + i / nb) * ldx + i % nb] = sX[i / nb][i % nb];
}

// ---------------------------------------------------------------------------
// MFMA fp64 GEMM:  C (M x N, ldc) -= A (M x K, lda) * B (K x N, ldb)
// ---------------------------------------------------------------------------
// One kernel template, k_dgemm_mfma<Cfg>, instantiated once per edition (the
// Gemm* configs below), and the async-staged k_dgemm_f64_glds further down.
// Common to all: a BM x 128 block tile walked in K-tiles of BK; fragments of
// v_mfma_f64_16x16x4_f64; XCD-aware block swizzle (T1) and the strip tile
// order.  In the template A is transposed in LDS so fragment reads are
// conflict-free.  GEMM_BM / GEMM_BK are the tile of every edition but
// GemmBm256.
#define GEMM_BM 128
#define GEMM_BN 128
#define GEMM_BK 16

// tile order: strips of `strip_w` tile-columns walked row-major, so the
// ~512 concurrently-resident workgroups form a 2D window (e.g. 64 wg =
// 8 rows x 8 cols at strip_w 8) instead of a 1D row slice.  Cuts the
// B-panel re-read traffic from ntm full passes to one pass per strip that
// stays L2/LLC-hot, and keeps each A row-panel hot for strip_w consecutive
// tiles.  Bijective for ragged tails; strip_w <= 1 is the flat order.
DEVFN void gemm_tile_of(int wg, int ntm, int ntn, int strip_w, int &tm,
                        int &tn) {
    if (strip_w > 1 && strip_w < ntn) {
        const int per = ntm * strip_w;
        const int full = ntn / strip_w;
        const int strip = wg / per;
        if (strip < full) {
            const int rem = wg % per;
            tm = rem / strip_w;
            tn = strip * strip_w + rem % strip_w;
        } else {
            const int rem = wg - full * per;
            const int wc = ntn - full * strip_w;
            tm = rem / wc;
            tn = full * strip_w + rem % wc;
        }
    } else {
        tm = wg / ntn;
        tn = wg % ntn;
    }
}

// Tile-cyclic lower-triangle mask of the NT edition (the Cholesky c4
// single-launch update): workgroups whose GLOBAL v-tile row < v-tile col exit
// immediately, so one rectangular launch covers the trapezoid of tiles with
// i >= j and spends nothing on the rest.  mask.v == 0 disables.  A 128-wide
// workgroup never straddles a v-tile boundary (v % 128 == 0 enforced by the
// launcher).
struct TriMask {
    int v;          // global tile size (0 = no mask)
    int r0off;      // launch-local row 0's offset within the rank-local A11
    int64_t c0off;  // same for columns
    int Px, Py, pi, pj;
};
struct GemmNoTail {};  // editions without a trailing kernel argument
constexpr int gemm_log2(int x) { return x <= 1 ? 0 : 1 + gemm_log2(x / 2); }

// Compile-time facts of one edition of k_dgemm_mfma:
//   BM x 128 block tile, K-tiles of BK;
//   TPB threads = TPB/64 waves as a (TPB/64/WN) x WN grid, each wave owning a
//     64 x (16*FN) sub-tile as 4 x FN MFMA fragments;
//   BT: B is stored N x K row-major (C -= A * B^T), not K x N;
//   PERSIST: grid-stride loop over tiles, so the grid may be smaller than the
//     tile count;
//   MINB: minimum blocks per CU of the launch bounds;
//   Tail: the kernel's last argument -- int = the non-temporal epilogue flag,
//     TriMask = the lower-triangle early exit, GemmNoTail = none.
// The editions are named types so that a trace shows which one ran.
template <int BM_, int BK_, int TPB_, int WN_, int FN_, bool BT_,
          bool PERSIST_, int MINB_, class Tail_>
struct GemmCfg {
    static constexpr int BM = BM_, BK = BK_, TPB = TPB_, WN = WN_, FN = FN_;
    static constexpr int MINB = MINB_;
    static constexpr bool BT = BT_, PERSIST = PERSIST_;
    using Tail = Tail_;
};
// CONFLUX_GEMM_VARIANT=0: 4 waves (2x2) of 64x64.
struct GemmW4 : GemmCfg<128, 16, 256, 2, 4, false, false, 1, GemmNoTail> {};
// Variant 1, the default and the flop carrier of every factorization: 8 waves
// (2x4) of 64x32.  NOTE (r02 measured): its launch bounds (512, 4) are
// load-bearing -- they force a 128-register allocation (with a small scratch
// spill) whose schedule sustains 57.7 TF; relaxing to (512, 2) (166 regs, no
// spill, same 2-waves/SIMD occupancy) drops to 44.3, and software-pipelining
// the fragment loads on top of it reaches only 45.  Keep the tight bound.
struct GemmW8 : GemmCfg<128, 16, 512, 4, 2, false, true, 4, int> {};
// Variant 3: 256x128 block tile, 8 waves as 4x2 of 64x64 -- double the
// accumulator chains per wave and half the barriers per flop vs GemmW8; the
// half-depth K-tile keeps it at 49.5 KB LDS -> 2 wg/CU.  Not persistent:
// meant for the uncapped full-chip launches; the capped overlap path keeps
// GemmW8.
struct GemmBm256 : GemmCfg<256, 8, 512, 2, 4, false, false, 1, GemmNoTail> {};
// NT edition of GemmW8: C -= A * B^T with B stored (N x K) row-major -- the
// computeA11 low-rank update (reference Cholesky.cpp:345-351).
struct GemmW8NT : GemmCfg<128, 16, 512, 4, 2, true, false, 4, TriMask> {};

// Register-staged global->LDS with the write-after-barrier placement (guide
// §5.5 T14), double-buffered, one barrier per K-step.
template <class Cfg>
__global__ __launch_bounds__(Cfg::TPB, Cfg::MINB) void k_dgemm_mfma(
    const double *__restrict__ A, int64_t lda, const double *__restrict__ B,
    int64_t ldb, double *__restrict__ C, int64_t ldc, int M, int64_t N, int K,
    int ntm, int ntn, int strip_w, typename Cfg::Tail tail) {
    constexpr int BM = Cfg::BM, BN = GEMM_BN, BK = Cfg::BK, TPB = Cfg::TPB;
    constexpr int WN = Cfg::WN, FN = Cfg::FN;
    // staged elements per thread per K-tile: element e = tid + i*TPB of the
    // BM*BK (A) or BK*BN (B) tile, so consecutive lanes read consecutive
    // addresses along the BK-wide rows of A (and of an N x K B) or the
    // BN-wide rows of a K x N B
    constexpr int NA = BM * BK / TPB, NB = BK * BN / TPB;
    // e is decoded with shifts and masks by the tile's row width (BK for A,
    // BW for B): `/` and `%` by the same constants end as the same shifts
    // but through other passes, and GemmW8's schedule is not the same after
    // them (tools/isa_diff.py: its spill count changes)
    constexpr int BW = Cfg::BT ? BK : BN;
    constexpr int LBK = gemm_log2(BK), LBW = gemm_log2(BW);
    constexpr bool NTC = std::is_same<typename Cfg::Tail, int>::value;
    constexpr bool MASKED = std::is_same<typename Cfg::Tail, TriMask>::value;
    static_assert(TPB / 64 / WN * 64 == BM && WN * FN * 16 == BN,
                  "the wave grid must cover the block tile");
    static_assert(NA * TPB == BM * BK && NB * TPB == BK * BN && BK % 4 == 0,
                  "the K-tile must split evenly over threads and MFMA steps");
    static_assert(1 << LBK == BK && 1 << LBW == BW, "powers of two");

    __shared__ double As[2][BK][BM + 1];   // transposed, padded
    __shared__ double Bs[2][BK][BN + 2];   // double-buffered
    // PERSIST: grid-stride over tiles.  gridDim may be capped below nwg so
    // the concurrent panel kernel (needs whole CUs: 135 KB LDS/block) can
    // co-schedule during lookahead.  gridDim == nwg -> one iteration,
    // identical to the plain launch.  Otherwise: exactly one tile per block.
    const int nwg = ntm * ntn;
    for (int vwg = blockIdx.x; !Cfg::PERSIST || vwg < nwg; vwg += gridDim.x) {
    // bijective XCD swizzle (guide §5: q/r form).  Written out here, not a
    // helper shared with k_dgemm_f64_glds: as an inlined function it leaves
    // GemmW8NT with other scalar registers (tools/isa_diff.py)
    int wg = vwg;
    {
        const int q = nwg >> 3, r = nwg & 7;
        const int xcd = vwg & 7, idx = vwg >> 3;
        // inverse of dispatch round-robin: give each XCD a contiguous chunk
        wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
        if (nwg < 8) wg = vwg;          // tiny grids: identity
    }
    int tm, tn;
    gemm_tile_of(wg, ntm, ntn, strip_w, tm, tn);
    const int row0 = tm * BM;
    const int64_t col0 = (int64_t)tn * BN;
    if constexpr (MASKED) {
        if (tail.v > 0) {
            const int gti =
                (int)((tail.r0off + row0) / tail.v) * tail.Px + tail.pi;
            const int gtj =
                (int)((tail.c0off + col0) / tail.v) * tail.Py + tail.pj;
            if (gti < gtj) return;  // above the global tile diagonal: untouched
        }
    }

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm0 = (wave / WN) * 64;             // wave's 64 x 16*FN sub-tile
    const int wn0 = (wave % WN) * (16 * FN);
    const int frow = lane & 15;                   // fragment row/col lane part
    const int fk = lane >> 4;                     // fragment k lane part

    f64x4 acc[4][FN];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = f64x4{0, 0, 0, 0};

    double ra[NA], rb[NB];                        // staging registers
    const int ktiles = (K + BK - 1) / BK;

    auto load_a = [&](int kt) {
        const int kk = kt * BK;
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int e = tid + i * TPB;
            const int r = e >> LBK, k = e & (BK - 1);  // row-major in tile
            const int gr = row0 + r;
            ra[i] = (gr < M && kk + k < K) ? A[(int64_t)gr * lda + kk + k] : 0.0;
        }
    };
    auto load_b = [&](int kt) {
        const int kk = kt * BK;
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int e = tid + i * TPB;
            // B's tile is row-major like B itself: K x N, or (BT) N x K,
            // coalesced over k within each B row like the A staging
            const int hi = e >> LBW, lo = e & (BW - 1);
            const int k = Cfg::BT ? lo : hi;
            const int64_t gc = col0 + (Cfg::BT ? hi : lo);
            rb[i] = (kk + k < K && gc < N)
                        ? (Cfg::BT ? B[gc * ldb + kk + k]
                                   : B[(int64_t)(kk + k) * ldb + gc])
                        : 0.0;
        }
    };
    auto write_lds = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int e = tid + i * TPB;
            As[buf][e & (BK - 1)][e >> LBK] = ra[i];
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int e = tid + i * TPB;
            if constexpr (Cfg::BT)
                Bs[buf][e & (BW - 1)][e >> LBW] = rb[i];
            else
                Bs[buf][e >> LBW][e & (BW - 1)] = rb[i];
        }
    };

    load_a(0);
    load_b(0);
    write_lds(0);
    __syncthreads();

    int cur = 0;
    for (int kt = 0; kt < ktiles; ++kt) {
        if (kt + 1 < ktiles) {           // issue next tile's global loads
            load_a(kt + 1);
            load_b(kt + 1);
        }
#pragma unroll
        for (int kk = 0; kk < BK / 4; ++kk) {
            const int k = kk * 4 + fk;
            double af[4], bf[FN];
#pragma unroll
            for (int i = 0; i < 4; ++i) af[i] = As[cur][k][wm0 + i * 16 + frow];
#pragma unroll
            for (int j = 0; j < FN; ++j) bf[j] = Bs[cur][k][wn0 + j * 16 + frow];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < FN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(
                        af[i], bf[j], acc[i][j], 0, 0, 0);
        }
        // write t+1 into the other buffer (everyone finished reading it at
        // the barrier that ended step t-1), then one barrier per K-step
        if (kt + 1 < ktiles) write_lds(cur ^ 1);
        __syncthreads();
        cur ^= 1;
    }

    // epilogue: C -= acc   (read-modify-write, coalesced over frag columns)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < FN; ++j) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                // f64 16x16x4 C/D map (hardware-verified by mfma_probe):
                // lane l, reg q -> D[4*q + (l>>4)][l & 15]
                const int r = row0 + wm0 + i * 16 + q * 4 + fk;
                const int64_t cidx = col0 + wn0 + j * 16 + frow;
                if (r < M && cidx < N) {
                    double *cp = &C[(int64_t)r * ldc + cidx];
                    if constexpr (NTC) {
                        // non-temporal RMW: C has zero reuse — keep its
                        // 4.3 GB/launch from evicting hot lines (the
                        // concurrent panel's sync slabs) out of the LLC
                        if (tail)
                            __builtin_nontemporal_store(
                                __builtin_nontemporal_load(cp) - acc[i][j][q],
                                cp);
                        else
                            *cp -= acc[i][j][q];
                    } else {
                        *cp -= acc[i][j][q];
                    }
                }
            }
        }
    }
    if constexpr (!Cfg::PERSIST) return;
    // next tile re-stages buffer 0; the kt-loop's closing barrier already
    // ordered every wave's last LDS read before it
    if (vwg + gridDim.x < nwg) __syncthreads();
    }
}


// ---------------------------------------------------------------------------
// fused inter-leaf glue of factor_panel: two launches per 32-column leaf in
// place of gather + scatter + k_trsm_left_lower_unit32 + a K=32
// k_dgemm_mfma<GemmW8>.  No inter-block communication in either kernel; both
// reproduce the old chain BIT FOR BIT (tests/test_panel_glue_gpu.py compares
// the two paths).
// ---------------------------------------------------------------------------
// k_panel_glue_prep: thread = one column of [0, skip0) u [skip0 + 32,
// tot_cols + 32), the columns launch_rowperm_skip covers at skipn = 32.  It
// reads the column's 64 listed source rows (row_base + src_idx[i]) into
// registers, then stores them to rows dst_idx[i] + row_base: every read of a
// column precedes every write of it in ONE thread's program order, columns
// are disjoint between threads, so the permutation needs no staging buffer
// and no barrier (the one barrier below only publishes L).  Entries 0..31 of the map have dst = i (the sub-panel's new
// rows 0..31, see k_panel_factor's tail), so for a column right of the
// sub-panel x[0..31] IS the U block's column and the unit-lower solve with
// L (32 x 32, the sub-panel's own top block, in the skipped columns and so
// never written here) runs on the registers before the store.  Each element
// receives k_trsm_left_lower_unit32's chain of operations (x[r] -= l[r][i] *
// x[i], i ascending, each contracted to one fma); only the order in which
// independent chains are interleaved differs (see the loop).  The map's
// identity padding repeats entry 0 (dst 0, the source of entry 0): row 0 is
// not changed by a unit-lower solve, so the repeated stores carry the value
// entry 0 stores.  L == nullptr: permutation only.
__global__ __launch_bounds__(64) void k_panel_glue_prep(
    double *mat, int64_t ld, const int *__restrict__ dst_idx,
    const int *__restrict__ src_idx, int row_base, int skip0, int tot_cols,
    const double *__restrict__ L, int64_t ldl) {
    __shared__ double sL[32][33];
    const int tid = threadIdx.x;
    const int cc0 = blockIdx.x * 64;
    // block-uniform: some column of this block lies right of the sub-panel
    const bool right = L && cc0 + 63 >= skip0;
    // L and the column are loaded together: the kernel is a chain of memory
    // round trips (map -> column -> store) and each costs several us under
    // the concurrent trailing GEMM, so L must not add one of its own
    double lreg[16];
    if (right) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int e = tid + j * 64;
            lreg[j] = L[(int64_t)(e >> 5) * ldl + (e & 31)];
        }
    }
    const int cc = cc0 + tid;
    const bool active = cc < tot_cols;
    const int64_t c = (cc < skip0) ? cc : cc + 32;
    // the map is read with wave-uniform indices, i.e. by scalar loads, 16
    // entries a load.  (Measured alternative: one vector load per array plus
    // readlane broadcasts — 34 vs 27 us per launch under the trailing GEMM.)
    double x[64];
    if (active) {
#pragma unroll
        for (int i = 0; i < 64; ++i)
            x[i] = mat[(int64_t)(row_base + src_idx[i]) * ld + c];
    }
    if (right) {  // block-uniform, so the barrier is legal here
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int e = tid + j * 64;
            sL[e >> 5][e & 31] = lreg[j];
        }
        __syncthreads();
        if (active && cc >= skip0) {
            // column-oriented order: x[i] is final once steps 0..i-1 ran,
            // and row r still receives its terms with i ascending — the
            // same chain of fmas per element as the row-oriented loop of
            // k_trsm_left_lower_unit32, with 31 - i independent ones a step
#pragma unroll
            for (int i = 0; i < 31; ++i) {
                const double xi = x[i];
#pragma unroll
                for (int r = i + 1; r < 32; ++r) x[r] -= sL[r][i] * xi;
            }
        }
    }
    if (active) {
#pragma unroll
        for (int i = 0; i < 64; ++i)
            mat[(int64_t)(dst_idx[i] + row_base) * ld + c] = x[i];
    }
}

// k_panel_glue_update: C (M x N) -= A (M x 32) * B (32 x N), K = 32 only.
// One (64*WM) x (32*WN) tile per block, one 64 x 32 sub-tile per wave (the
// GemmW8 edition's 4 x 2 fragments of v_mfma_f64_16x16x4_f64).  The whole K
// is staged once (one barrier, no K loop) and the C tile is loaded into
// registers BEFORE the staging writes and the MFMAs, so its HBM latency
// overlaps them; then one subtraction and the store.  Bit-identity with
// k_dgemm_mfma<GemmW8> at K = 32: accumulators start at zero, the eight
// k-blocks of 4 run ascending with the same lane -> k map, then C = C - acc.
// __launch_bounds__(.., 3): three 256-thread blocks a CU is what the 50 KB
// of LDS admits, and under the concurrent trailing GEMM the kernel's share
// of the memory system follows the bytes it keeps in flight.
template <int WM, int WN>
__global__ __launch_bounds__(64 * WM * WN, 3) void k_panel_glue_update(
    const double *__restrict__ A, int64_t lda, const double *__restrict__ B,
    int64_t ldb, double *__restrict__ C, int64_t ldc, int M, int N) {
    constexpr int K = 32, BM = 64 * WM, BN = 32 * WN, TPB = 64 * WM * WN;
    constexpr int NA = BM * K / 2 / TPB;   // staged element PAIRS per thread
    constexpr int NBE = K * BN / 2 / TPB;
    __shared__ double As[K][BM + 1];   // transposed, padded
    __shared__ alignas(16) double Bs[K][BN + 2];
    const int row0 = blockIdx.y * BM;
    const int col0 = blockIdx.x * BN;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm0 = (wave / WN) * 64;             // wave's 64x32 sub-tile
    const int wn0 = (wave % WN) * 32;
    const int frow = lane & 15;                   // fragment row/col lane part
    const int fk = lane >> 4;                     // fragment k lane part
    // Column assignment inside the wave's 32 columns: lane part frow of
    // fragment j holds column 2*frow + j (not j*16 + frow), so a lane's two
    // fragments are ADJACENT columns — every C access is 16 bytes a lane,
    // half the requests of the 8-byte form, and one 16-byte LDS read feeds
    // both B operands.  Which MFMA column slot an element sits in does not
    // enter its arithmetic.
    const int wc = wn0 + 2 * frow;                // tile column of fragment 0

    // stage A (BM x 32) and B (32 x BN): two adjacent elements per access
    f64x2u ra[NA], rb[NBE];
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const int e = tid + i * TPB;              // pair index, 16 per row
        const int gr = row0 + (e >> 4);
        ra[i] = (gr < M)
                    ? *(const f64x2u *)&A[(int64_t)gr * lda + 2 * (e & 15)]
                    : f64x2u{0, 0};
    }
#pragma unroll
    for (int i = 0; i < NBE; ++i) {
        const int e = tid + i * TPB;              // pair index, BN/2 per row
        const int gc = col0 + 2 * (e % (BN / 2));
        const double *bp = &B[(int64_t)(e / (BN / 2)) * ldb + gc];
        rb[i] = (gc + 1 < N) ? *(const f64x2u *)bp
                             : f64x2u{gc < N ? *bp : 0.0, 0.0};
    }
    // C prefetch (f64 16x16x4 C/D map: lane l, reg q -> D[4*q + (l>>4)][.]):
    // issued before the staging writes and the MFMAs so its latency overlaps
    // them.  cr[i][q] = the lane's two columns of row i*16 + q*4 + fk.
    f64x2u cr[4][4];
    const int gc0 = col0 + wc;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r = row0 + wm0 + i * 16 + q * 4 + fk;
            const double *cp = &C[(int64_t)r * ldc + gc0];
            cr[i][q] = (r < M && gc0 + 1 < N)
                           ? *(const f64x2u *)cp
                           : f64x2u{(r < M && gc0 < N) ? *cp : 0.0, 0.0};
        }
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const int e = tid + i * TPB;
        As[2 * (e & 15)][e >> 4] = ra[i][0];
        As[2 * (e & 15) + 1][e >> 4] = ra[i][1];
    }
#pragma unroll
    for (int i = 0; i < NBE; ++i) {
        const int e = tid + i * TPB;
        *(f64x2 *)&Bs[e / (BN / 2)][2 * (e % (BN / 2))] =
            f64x2{rb[i][0], rb[i][1]};
    }
    __syncthreads();

    // one 16-row fragment pair at a time: 16 accumulator registers live
    // instead of 64, which is what lets three blocks share a CU
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        f64x4 acc0 = f64x4{0, 0, 0, 0}, acc1 = f64x4{0, 0, 0, 0};
#pragma unroll
        for (int kk = 0; kk < K / 4; ++kk) {
            const int k = kk * 4 + fk;
            const double af = As[k][wm0 + i * 16 + frow];
            const f64x2 bf = *(const f64x2 *)&Bs[k][wc];
            acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(af, bf[0], acc0, 0, 0,
                                                        0);
            acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(af, bf[1], acc1, 0, 0,
                                                        0);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r = row0 + wm0 + i * 16 + q * 4 + fk;
            double *cp = &C[(int64_t)r * ldc + gc0];
            const f64x2u o = {cr[i][q][0] - acc0[q], cr[i][q][1] - acc1[q]};
            if (r < M && gc0 + 1 < N)
                *(f64x2u *)cp = o;
            else if (r < M && gc0 < N)
                *cp = o[0];
        }
    }
}


// ---------------------------------------------------------------------------
// glds variant: async global->LDS staging (__builtin_amdgcn_global_load_lds,
// 16-byte pieces), one barrier per K-step, XOR-swizzled SOURCE addresses so
// the lane-linear LDS image reads conflict-free (guide rule 21 / T2).
// Layouts: As [BK][BM] row-of-m linear, A-chunk (row, p) stored at p^(row&7);
//          Bs [BK][BN] linear, B-chunk (k, np) stored at np^((k&3)<<1).
// Envelope (checked by launch_dgemm_f64, which runs k_dgemm_mfma<GemmW8>
// instead when any of it fails): K % 16 == 0 (no K tail: a short last K-tile would
// read rows of B that do not exist), lda, ldb and N even and A, B 16-byte
// aligned (every 16-byte piece is then aligned and lies wholly inside or
// wholly outside the matrix).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(512, 4) void k_dgemm_f64_glds(
    const double *__restrict__ A, int64_t lda, const double *__restrict__ B,
    int64_t ldb, double *__restrict__ C, int64_t ldc, int M, int64_t N, int K,
    int ntm, int ntn, int strip_w) {
    int wg = blockIdx.x;
    {   // XCD swizzle, as in k_dgemm_mfma
        const int nwg = ntm * ntn;
        const int q = nwg >> 3, r = nwg & 7;
        const int xcd = wg & 7, idx = wg >> 3;
        wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
        if (nwg < 8) wg = blockIdx.x;
    }
    int tm, tn;
    gemm_tile_of(wg, ntm, ntn, strip_w, tm, tn);
    const int row0 = tm * GEMM_BM;
    const int64_t col0 = (int64_t)tn * GEMM_BN;

    // ONE shared object (a second one makes hipcc drain vmcnt(0) before
    // every ds_read — guide §5 trap (a)).  [2 buffers][A 16*128 | B 16*128]
    // carve: buf b: A at b*(BK*BM), B at 2*BK*BM + b*(BK*BN)
    __shared__ double smem[2 * (GEMM_BK * GEMM_BM + GEMM_BK * GEMM_BN)];
    // (through locals: an array initialised from `smem` directly becomes a
    // static initialiser holding an LDS address, which does not compile)
    double *As0 = smem;
    double *As[2] = {As0, As0 + GEMM_BK * GEMM_BM};
    double *Bs0 = smem + 2 * GEMM_BK * GEMM_BM;
    double *Bs[2] = {Bs0, Bs0 + GEMM_BK * GEMM_BN};

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm0 = (wave >> 2) * 64;
    const int wn0 = (wave & 3) * 32;
    const int frow = lane & 15;
    const int fk = lane >> 4;

    f64x4 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f64x4{0, 0, 0, 0};

    const int ktiles = (K + GEMM_BK - 1) / GEMM_BK;
    // A: 1024 16B chunks (row, p), linear ci = row*8 + p_lds; 2 waves-worth
    // per wave (16 wave-instructions over 8 waves = 2 each).
    // chunk for this lane at issue w (w = 0,1): ci = wave*128 + w*64 + lane
    // B: 1024 chunks (k, np), ci = k*64 + np_lds; same split.
    auto stage = [&](int buf, int kt) {
        const int kk = kt * GEMM_BK;
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            const int ci = wave * 128 + w * 64 + lane;
            // A chunk (row, p_lds) holds source k-pair p_lds ^ (row & 7);
            // out-of-range rows load the block's first row (junk rows are
            // discarded by the epilogue bounds).  K is a multiple of 16
            // everywhere in this engine (v, nlayr, NB all are), so there is
            // no K-tail.
            const int arow = ci >> 3, ap = ci & 7;
            const int asrc_p = ap ^ (arow & 7);
            const double *agp =
                A + (int64_t)(row0 + ((row0 + arow < M) ? arow : 0)) * lda +
                kk + 2 * asrc_p;
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) uint32_t *)agp,
                (__attribute__((address_space(3))) uint32_t
                     *)(As[buf] + (int64_t)(wave * 128 + w * 64) * 2),
                16, 0, 0);
            // B chunk (k, np_lds) holds source col-pair np_lds ^ ((k&3)<<1).
            // Clamp only when the chunk's FIRST column is out of range (a
            // half-valid chunk must still load its valid column; its second
            // 8 bytes may read past row end — within hipMalloc's page
            // granularity, and its value only lands in discarded lanes).
            const int ck = ci >> 6, cnp = ci & 63;
            const int bsrc_np = cnp ^ ((ck & 3) << 1);
            const double *bgp =
                B + (int64_t)(kk + ck) * ldb + col0 + 2 * bsrc_np;
            if (col0 + 2 * bsrc_np >= N) bgp = B + (int64_t)(kk + ck) * ldb;
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) uint32_t *)bgp,
                (__attribute__((address_space(3))) uint32_t
                     *)(Bs[buf] + (int64_t)(ci - lane) * 2),
                16, 0, 0);
        }
    };

    stage(0, 0);
    int cur = 0;
    for (int kt = 0; kt < ktiles; ++kt) {
        // ONE barrier per K-step: its per-wave vmcnt(0) drains the stage
        // issued LAST iteration (it flew under that iteration's compute),
        // and the barrier itself guarantees every wave finished reading the
        // buffer the next stage overwrites.
        __syncthreads();
        if (kt + 1 < ktiles) stage(cur ^ 1, kt + 1);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const int k = kk * 4 + fk;
            const int ap = k >> 1, ae = k & 1;
            double af[4], bf[2];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = wm0 + i * 16 + frow;
                af[i] = As[cur][row * 16 + 2 * (ap ^ (row & 7)) + ae];
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int n = wn0 + j * 16 + frow;
                const int np = (n >> 1) ^ ((k & 3) << 1);
                bf[j] = Bs[cur][k * 128 + 2 * np + (n & 1)];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(
                        af[i], bf[j], acc[i][j], 0, 0, 0);
        }
        cur ^= 1;
    }

#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = row0 + wm0 + i * 16 + q * 4 + fk;
                const int64_t cidx = col0 + wn0 + j * 16 + frow;
                if (r < M && cidx < N) C[(int64_t)r * ldc + cidx] -= acc[i][j][q];
            }
        }
    }
}


// ---------------------------------------------------------------------------
// Cholesky kernels (CONFCHOX path; reference
// src/conflux/cholesky/Cholesky.cpp): k_potrf32 <- the 32-wide micro-factor
// of LAPACKE_dpotrf('L') (Cholesky.cpp:192); the right/lower/trans TRSM is
// k_trsm_right_tri32 with trans=1 (updateA10's dtrsm, Cholesky.cpp:280);
// the NoTrans x Trans low-rank update (computeA11, Cholesky.cpp:345-351) is
// k_dgemm_mfma<GemmW8NT> above.
// ---------------------------------------------------------------------------
// single block: in-place lower Cholesky of the nb x nb (nb <= 32) diagonal
// block, row-major ld.  Sequential over columns in LDS (no pivoting).
__global__ __launch_bounds__(256) void k_potrf32(double *__restrict__ A,
                                                 int64_t lda, int nb) {
    __shared__ double sA[32][33];
    const int tid = threadIdx.x;
    for (int i = tid; i < nb * nb; i += 256)
        sA[i / nb][i % nb] = A[(i / nb) * lda + i % nb];
    __syncthreads();
    for (int c = 0; c < nb; ++c) {
        if (tid == 0) sA[c][c] = sqrt(sA[c][c]);
        __syncthreads();
        const double inv = 1.0 / sA[c][c];
        if (tid > c && tid < nb) sA[tid][c] *= inv;
        __syncthreads();
        // trailing update: element (i, j), i > c, c < j <= i
        for (int e = tid; e < nb * nb; e += 256) {
            const int i = e / nb, j = e % nb;
            if (i > c && j > c && j <= i) sA[i][j] -= sA[i][c] * sA[j][c];
        }
        __syncthreads();
    }
    for (int i = tid; i < nb * nb; i += 256)
        A[(i / nb) * lda + i % nb] = sA[i / nb][i % nb];
}

// 32x32 LU WITHOUT pivoting (the Python prototype's EmptyPivot fast path,
// SURVEY §8f4 — for diagonally dominant inputs): per column, scale below
// the diagonal by 1/pivot and rank-1 the trailing sub-block.  Single block,
// same shape as k_potrf32.
__global__ __launch_bounds__(256) void k_getrf32_nopiv(double *__restrict__ A,
                                                       int64_t lda, int nb) {
    __shared__ double sA[32][33];
    const int tid = threadIdx.x;
    for (int i = tid; i < nb * nb; i += 256)
        sA[i / nb][i % nb] = A[(i / nb) * lda + i % nb];
    __syncthreads();
    for (int c = 0; c < nb; ++c) {
        const double piv = sA[c][c];
        const double inv = (piv != 0.0) ? 1.0 / piv : 0.0;  // LAPACK-style:
        __syncthreads();                                    // no scaling on 0
        if (tid > c && tid < nb && piv != 0.0) sA[tid][c] *= inv;
        __syncthreads();
        for (int e = tid; e < nb * nb; e += 256) {
            const int i = e / nb, j = e % nb;
            if (i > c && j > c) sA[i][j] -= sA[i][c] * sA[c][j];
        }
        __syncthreads();
    }
    for (int i = tid; i < nb * nb; i += 256)
        A[(i / nb) * lda + i % nb] = sA[i / nb][i % nb];
}

// ---------------------------------------------------------------------------
// misc small kernels for the distributed path
// ---------------------------------------------------------------------------
// candidate pack: cand row i = [ gri[f+i] | A10[f+i, 0..v) ]  (prepend_column,
// utils.hpp:13-26 + step-1 copy conflux_opt.hpp:698-705)
// cand row i = [ gri[f+s] | A10[f+s, :] ] with s = idx ? idx[i] : i;
// s >= n_src stands for the reference's zero-padded candidate rows
// (step0_padding, conflux_opt.hpp:604-614).
__global__ void k_pack_candidate(const double *__restrict__ A10, int64_t lda,
                                 const int *__restrict__ gri, int f, int n_src,
                                 int n_out, int v, const int *__restrict__ idx,
                                 double *__restrict__ cand) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)n_out * (v + 1)) return;
    const int r = (int)(i / (v + 1)), c = (int)(i % (v + 1));
    const int s = idx ? idx[r] : r;
    if (s >= n_src) { cand[i] = 0.0; return; }
    cand[i] = (c == 0) ? (double)gri[f + s] : A10[(int64_t)(f + s) * lda + c - 1];
}

__global__ void k_extract_col0_int(const double *__restrict__ cand, int stride,
                                   int n, int *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (int)cand[(int64_t)i * stride];
}

// slab pack for the A10 spread (conflux_opt.hpp:1389-1399): column slab
// [pk*nlayr, (pk+1)*nlayr) of X (n x v) -> contiguous n x nlayr at slab pk
__global__ void k_slab_pack(const double *__restrict__ X, int64_t ldx, int n,
                            int nlayr, int Pz, double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)n * nlayr * Pz) return;
    const int pk = (int)(i / ((int64_t)n * nlayr));
    const int64_t rest = i % ((int64_t)n * nlayr);
    const int r = (int)(rest / nlayr), c = (int)(rest % nlayr);
    out[i] = X[(int64_t)r * ldx + pk * nlayr + c];
}

}  // namespace ck

// ---------------------------------------------------------------------------
// launch wrappers (host side)
// ---------------------------------------------------------------------------
using namespace ck;

static inline int64_t cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }

static inline unsigned cap_grid(int64_t total) {
    int64_t g = cdiv64(total, 256);
    if (g > (1 << 22)) g = 1 << 22;  // grid-stride kernels cover the rest
    return (unsigned)g;
}

void launch_init_matrix(double *A, int Ml, int Nl, int v, int Px, int Py,
                        int pi, int pj, int zero_layer, uint64_t seed,
                        hipStream_t s) {
    const int64_t total = (int64_t)Ml * Nl;
    hipLaunchKernelGGL(k_init_matrix, dim3(cap_grid(total)), dim3(256), 0, s,
                       A, Ml, Nl, v, Px, Py, pi, pj, zero_layer, seed, 0,
                       (int64_t)0);
}

void launch_init_matrix_spd(double *A, int Ml, int Nl, int v, int Px, int Py,
                            int pi, int pj, int zero_layer, uint64_t seed,
                            int64_t Nglob, hipStream_t s) {
    const int64_t total = (int64_t)Ml * Nl;
    hipLaunchKernelGGL(k_init_matrix, dim3(cap_grid(total)), dim3(256), 0, s,
                       A, Ml, Nl, v, Px, Py, pi, pj, zero_layer, seed, 1,
                       Nglob);
}

void launch_copy2d(const double *src, int64_t lds, double *dst, int64_t ldd,
                   int rows, int64_t cols, hipStream_t s) {
    if (rows <= 0 || cols <= 0) return;
    hipLaunchKernelGGL(k_copy2d, dim3(cap_grid((int64_t)rows * cols)),
                       dim3(256), 0, s, src, lds, dst, ldd, rows, cols);
}

void launch_zero2d(double *dst, int64_t ldd, int rows, int64_t cols,
                   hipStream_t s) {
    if (rows <= 0 || cols <= 0) return;
    hipLaunchKernelGGL(k_zero2d, dim3(cap_grid((int64_t)rows * cols)),
                       dim3(256), 0, s, dst, ldd, rows, cols);
}

void launch_add2d(const double *src, int64_t lds, double *dst, int64_t ldd,
                  int rows, int64_t cols, hipStream_t s) {
    if (rows <= 0 || cols <= 0) return;
    hipLaunchKernelGGL(k_add2d, dim3(cap_grid((int64_t)rows * cols)),
                       dim3(256), 0, s, src, lds, dst, ldd, rows, cols);
}

void launch_row_gather(const double *src, int64_t lds, double *dst,
                       int64_t ldd, const int *idx, int n_rows, int64_t cols,
                       hipStream_t s) {
    if (n_rows <= 0 || cols <= 0) return;
    hipLaunchKernelGGL(k_row_gather, dim3(cap_grid((int64_t)n_rows * cols)),
                       dim3(256), 0, s, src, lds, dst, ldd, idx, n_rows, cols);
}

void launch_row_scatter(const double *src, int64_t lds, double *dst,
                        int64_t ldd, const int *idx, int n_rows, int64_t cols,
                        hipStream_t s) {
    if (n_rows <= 0 || cols <= 0) return;
    hipLaunchKernelGGL(k_row_scatter, dim3(cap_grid((int64_t)n_rows * cols)),
                       dim3(256), 0, s, src, lds, dst, ldd, idx, n_rows, cols);
}





void launch_rowperm_skip(double *mat, int64_t ld, const int *dst_idx,
                         const int *src_idx, int row_base, int n_rows,
                         int64_t skip0, int64_t skipn, int64_t tot_cols,
                         double *tmp, hipStream_t s) {
    if (n_rows <= 0 || tot_cols <= 0) return;
    const int64_t n = (int64_t)n_rows * tot_cols;
    hipLaunchKernelGGL(k_rowperm_gather_skip, dim3(cap_grid(n)), dim3(256),
                       0, s, mat, ld, tmp, src_idx, row_base, n_rows, skip0,
                       skipn, tot_cols);
    hipLaunchKernelGGL(k_rowperm_scatter_skip, dim3(cap_grid(n)), dim3(256),
                       0, s, tmp, mat, ld, dst_idx, row_base, n_rows, skip0,
                       skipn, tot_cols);
}

// fused glue, step 1: the leaf's row permutation over the non-sub-panel
// columns of a `tot_cols + 32`-wide panel (swap map of 64 entries, sub-panel
// at columns [jb, jb + 32), rows relative to jb) and, with L != nullptr, the
// unit-lower solve of rows jb..jb+31 of the columns right of the sub-panel
void launch_panel_glue_prep(double *mat, int64_t ld, const int *dst_idx,
                            const int *src_idx, int jb, int tot_cols,
                            const double *L, int64_t ldl, hipStream_t s) {
    if (tot_cols <= 0) return;
    hipLaunchKernelGGL(k_panel_glue_prep, dim3((unsigned)cdiv64(tot_cols, 64)),
                       dim3(64), 0, s, mat, ld, dst_idx, src_idx, jb, jb,
                       tot_cols, L, ldl);
}

// fused glue, step 2: C (M x N) -= A (M x 32) B (32 x N).  Tile shape:
// CONFLUX_GLUE_TILE = 0: 128x128, 1: 64x128, 2 (default): 128x64 — in
// context the two 256-thread shapes tie and the 128x128 one gains nothing
// over the old chain (sweep in DESIGN §9); 128x64 wastes the least of a tile
// on the narrow last leaves.  Plain 2-D grid, one tile per block.
void launch_panel_glue_update(const double *A, int64_t lda, const double *B,
                              int64_t ldb, double *C, int64_t ldc, int M,
                              int N, hipStream_t s) {
    if (M <= 0 || N <= 0) return;
    static int tile = -1;
    if (tile < 0) {
        const char *e = getenv("CONFLUX_GLUE_TILE");
        tile = e ? atoi(e) : 2;
        if (tile < 0 || tile > 2) tile = 2;
    }
#define GLUE_UPDATE(WM, WN)                                                   \
    hipLaunchKernelGGL((k_panel_glue_update<WM, WN>),                         \
                       dim3((unsigned)cdiv64(N, 32 * WN),                     \
                            (unsigned)cdiv64(M, 64 * WM)),                    \
                       dim3(64 * WM * WN), 0, s, A, lda, B, ldb, C, ldc, M, N)
    if (tile == 0) GLUE_UPDATE(2, 4);
    else if (tile == 1) GLUE_UPDATE(1, 4);
    else GLUE_UPDATE(2, 2);
#undef GLUE_UPDATE
}

// panel block shape: CONFLUX_PANEL_RPB (rows/block) x CONFLUX_PANEL_TPB
// (threads).  r02 A/B at N=16384: 256 rows/block 1-row/thread (67 KB LDS,
// 2 blocks/CU) beats the original 512x256 2-rows/thread: 205 vs 223
// ms/step in context, panel 122 vs 137 ms sequential.  Default 256x256.
static void panel_shape(int *qr, int *tpb) {
    static int g_qr = -1, g_tpb = 0;
    if (g_qr < 0) {
        const char *r = getenv("CONFLUX_PANEL_RPB");
        const char *t = getenv("CONFLUX_PANEL_TPB");
        g_tpb = t ? atoi(t) : 256;
        if (g_tpb != 512 && g_tpb != 128) g_tpb = 256;
        const int rpb = r ? atoi(r) : 256;
        g_qr = (rpb / g_tpb >= 2) ? 2 : 1;
    }
    *qr = g_qr;
    *tpb = g_tpb;
}

// Leaf-kernel switches, process-global like the glue switch of the engine;
// each setter returns the previous mode.
//   CONFLUX_PANEL_REG (default 1): full 32-column leaves run the
//     register-resident k_panel_factor_reg; 0 = k_panel_factor everywhere.
//   CONFLUX_PANEL_PUBLISH (default 0): hand-off form of the register leaf,
//     1 = drain-free granule payload (R2), 0 = sc1 payload + drain + key.
//     R2 is 4 % faster on the sequential panel but did not pass the A/B
//     rule under the concurrent trailing GEMM (profiles/r06_panel_ab.log).
//   CONFLUX_PANEL_PHASE_STATS (default 0): run the instrumented
//     instantiations that time the phases of a column.
static int g_panel_reg = -1, g_panel_publish = -1, g_panel_phase = -1;
static int env_mode(int &g, const char *name, int dflt) {
    if (g < 0) {
        const char *e = getenv(name);
        g = e ? (atoi(e) != 0) : dflt;
    }
    return g;
}
int conflux_panel_reg_mode() {
    return env_mode(g_panel_reg, "CONFLUX_PANEL_REG", 1);
}
int conflux_panel_publish_mode() {
    return env_mode(g_panel_publish, "CONFLUX_PANEL_PUBLISH", 0);
}
int conflux_panel_phase_stats_mode() {
    return env_mode(g_panel_phase, "CONFLUX_PANEL_PHASE_STATS", 0);
}
int conflux_panel_set_reg_mode(int mode) {
    const int prev = conflux_panel_reg_mode();
    g_panel_reg = mode != 0;
    return prev;
}
int conflux_panel_set_publish_mode(int mode) {
    const int prev = conflux_panel_publish_mode();
    g_panel_publish = mode != 0;
    return prev;
}
int conflux_panel_set_phase_stats_mode(int mode) {
    const int prev = conflux_panel_phase_stats_mode();
    g_panel_phase = mode != 0;
    return prev;
}

static int panel_qr() {
    int qr, tpb;
    panel_shape(&qr, &tpb);
    return qr;
}

int conflux_panel_blocks_per_cu() {  // LDS/block ~= QR*TPB*264 B + tails
    int qr, tpb;
    panel_shape(&qr, &tpb);
    const int rows = qr * tpb;
    return rows <= 128 ? 4 : rows <= 256 ? 2 : 1;  // 34/67/135 KB of 160
}

int launch_panel_factor(double *panel, int64_t ldp, int m, int nb, void *sync,
                        int *ipiv, unsigned int epoch0, int *swap_dst,
                        int *swap_src, hipStream_t s) {
    static int backoff = -1;
    if (backoff < 0) {
        const char *e = getenv("CONFLUX_PANEL_SLEEP");
        backoff = e ? atoi(e) : 2;  // r02 sweep at the 256x256 shape:
                                    // 0/1/2/4 -> 203.5/202.2/201.5/201.5
                                    // ms/step in context
    }
    int qr, tpb;
    panel_shape(&qr, &tpb);
    int rpb = qr * tpb;
    int nblocks = (int)cdiv64(m, rpb);
    if (nblocks < 1) nblocks = 1;
    if (nblocks > CONFLUX_PANEL_MAX_BLOCKS && rpb < 512) {
        // very tall panel (m > 64k rows): auto-promote to 512-row blocks
        qr = 2; tpb = 256; rpb = 512;
        nblocks = (int)cdiv64(m, rpb);
    }
    if (nblocks > CONFLUX_PANEL_MAX_BLOCKS) return -1;  // not resident: refuse
    const int stats = conflux_panel_phase_stats_mode();
    // register-resident leaf: full 32-column leaves at the default 256x256
    // shape whose rows are 16-byte aligned (its loads and stores are 16
    // bytes wide).  Same rows per block and the same 2 blocks per CU as the
    // LDS kernel at that shape, so conflux_panel_rpb() and
    // conflux_panel_blocks_per_cu() hold for both and the refusal above is
    // the same.
    if (conflux_panel_reg_mode() && nb == PANEL_NB && m >= PANEL_NB &&
        qr == 1 &&
        tpb == PANEL_REG_TPB && ldp % 2 == 0 &&
        ((uintptr_t)panel & 15u) == 0) {
        const int r2 = conflux_panel_publish_mode();
#define PANEL_REG_LAUNCH(R2, ST)                                              \
    hipLaunchKernelGGL((k_panel_factor_reg<R2, ST>), dim3(nblocks),           \
                       dim3(PANEL_REG_TPB), 0, s, panel, ldp, m,              \
                       (PanelSync2 *)sync, ipiv, epoch0, nblocks, swap_dst,   \
                       swap_src, backoff)
        if (r2 && stats) PANEL_REG_LAUNCH(true, true);
        else if (r2) PANEL_REG_LAUNCH(true, false);
        else if (stats) PANEL_REG_LAUNCH(false, true);
        else PANEL_REG_LAUNCH(false, false);
#undef PANEL_REG_LAUNCH
        return 0;
    }
    if (stats && qr == 1 && tpb == 256) {
        // instrumented build of the default-shape LDS kernel
        hipLaunchKernelGGL((k_panel_factor<1, 256, true>), dim3(nblocks),
                           dim3(256), 0, s, panel, ldp, m, nb,
                           (PanelSync2 *)sync, ipiv, epoch0, nblocks,
                           swap_dst, swap_src, backoff);
        return 0;
    }
    if (qr == 1 && tpb == 512)
        hipLaunchKernelGGL((k_panel_factor<1, 512>), dim3(nblocks), dim3(512),
                           0, s, panel, ldp, m, nb, (PanelSync2 *)sync, ipiv,
                           epoch0, nblocks, swap_dst, swap_src, backoff);
    else if (qr == 1 && tpb == 128)
        hipLaunchKernelGGL((k_panel_factor<1, 128>), dim3(nblocks), dim3(128),
                           0, s, panel, ldp, m, nb, (PanelSync2 *)sync, ipiv,
                           epoch0, nblocks, swap_dst, swap_src, backoff);
    else if (qr == 1)
        hipLaunchKernelGGL((k_panel_factor<1, 256>), dim3(nblocks), dim3(256),
                           0, s, panel, ldp, m, nb, (PanelSync2 *)sync, ipiv,
                           epoch0, nblocks, swap_dst, swap_src, backoff);
    else
        hipLaunchKernelGGL((k_panel_factor<2, 256>), dim3(nblocks), dim3(256),
                           0, s, panel, ldp, m, nb, (PanelSync2 *)sync, ipiv,
                           epoch0, nblocks, swap_dst, swap_src, backoff);
    return 0;
}

void conflux_panel_spin_read(void *sync, unsigned long long *out,
                             hipStream_t s) {
    (void)hipMemcpyAsync(out, (char *)sync + offsetof(PanelSync2, spin_sum),
                         8, hipMemcpyDeviceToHost, s);
    (void)hipStreamSynchronize(s);
    (void)hipMemsetAsync((char *)sync + offsetof(PanelSync2, spin_sum), 0, 8,
                         s);
}

// the eight phase totals (PanelSync2::phase), read and reset like spin_sum
void conflux_panel_phase_read(void *sync, unsigned long long *out8,
                              hipStream_t s) {
    char *p = (char *)sync + offsetof(PanelSync2, phase);
    (void)hipMemcpyAsync(out8, p, 64, hipMemcpyDeviceToHost, s);
    (void)hipStreamSynchronize(s);
    (void)hipMemsetAsync(p, 0, 64, s);
}

int conflux_panel_sync_bytes() { return (int)sizeof(PanelSync2); }
int conflux_panel_err_offset() { return (int)offsetof(PanelSync2, err); }
int conflux_panel_nb() { return PANEL_NB; }
int conflux_panel_rpb() {
    int qr, tpb;
    panel_shape(&qr, &tpb);
    return qr * tpb;
}

void launch_trsm_left_lower_unit32(const double *L, int64_t ldl, double *X,
                                   int64_t ldx, int nb, int64_t N,
                                   hipStream_t s) {
    if (N <= 0 || nb <= 0) return;
    hipLaunchKernelGGL(k_trsm_left_lower_unit32, dim3(cdiv64(N, 256)),
                       dim3(256), 0, s, L, ldl, X, ldx, nb, N);
}

void launch_trsm_right_upper32(const double *U, int64_t ldu, double *X,
                               int64_t ldx, int nb, int64_t M, int trans,
                               hipStream_t s) {
    if (M <= 0 || nb <= 0) return;
    hipLaunchKernelGGL(k_trsm_right_upper32, dim3(cdiv64(M, 256)), dim3(256),
                       0, s, U, ldu, X, ldx, nb, M, trans);
}

// ---------------------------------------------------------------------------
// Fused whole-panel TRSMs, MFMA edition: ONE launch applies the full v x v
// triangle (v % 32 == 0).  Left-looking over 32-wide panels; the
// rank-32 updates run on the matrix cores (v_mfma_f64_16x16x4_f64, the
// lane maps verified by tools/mfma_probe), the 32x32 diagonal solves as
// register triangles (the k_trsm_*32 pattern).  Each block owns a stripe
// of X exclusively and stages panels through LDS, so the blocked chain's
// 31 launches and its 16 HBM re-writes of X collapse into one kernel.
// (A VALU version of this idea lost 3x to the blocked chain — the updates
// belong on MFMA; see DESIGN.md ablations.)
// ---------------------------------------------------------------------------

// X (M x v, row-major) <- X * U^-1 (trans=0) or X * L^-T (trans=1).
#define TRM_ROWS 128
__global__ __launch_bounds__(256) void k_trsm_right_mfma(
    const double *__restrict__ U, int64_t ldu, double *__restrict__ X,
    int64_t ldx, int v, int64_t M, int trans) {
    __shared__ double sXj[TRM_ROWS][33];     // current panel
    __shared__ double sXp[2][TRM_ROWS][33];  // solved panels, double-buffered
    __shared__ double sU[2][32][33];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int frow = lane & 15, fk = lane >> 4;
    const int64_t r0 = (int64_t)blockIdx.x * TRM_ROWS;
    const int rows = (int)min((int64_t)TRM_ROWS, M - r0);
    // register staging (w8-GEMM style): next panel's loads issue while MFMA
    // consumes the current LDS buffer — one barrier per 32-panel, HBM
    // latency hidden behind the update
    double rx[16], ru[4];  // 128x32 X panel + 32x32 U block per iteration
    auto load_u_regs = [&](int pb, int jb) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + i * 256;
            ru[i] = trans
                        ? U[(int64_t)(jb + (e & 31)) * ldu + pb + (e >> 5)]
                        : U[(int64_t)(pb + (e >> 5)) * ldu + jb + (e & 31)];
        }
    };
    auto load_x_regs = [&](int pb) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int e = tid + i * 256;
            rx[i] = (e >> 5) < rows
                        ? X[(r0 + (e >> 5)) * ldx + pb + (e & 31)]
                        : 0.0;
        }
    };
    auto write_bufs = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int e = tid + i * 256;
            sXp[buf][e >> 5][e & 31] = rx[i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + i * 256;
            sU[buf][e >> 5][e & 31] = ru[i];
        }
    };
    for (int jb = 0; jb < v; jb += 32) {
        __syncthreads();
        for (int i = tid; i < rows * 32; i += 256)
            sXj[i >> 5][i & 31] = X[(r0 + (i >> 5)) * ldx + jb + (i & 31)];
        int cur = 0;
        if (jb > 0) {
            load_x_regs(0);
            load_u_regs(0, jb);
            write_bufs(0);
        }
        __syncthreads();  // also covers the sXj stage
        for (int pb = 0; pb < jb; pb += 32) {
            if (pb + 32 < jb) {
                load_x_regs(pb + 32);
                load_u_regs(pb + 32, jb);
            }
            // sXj[rows x 32] -= sXp[rows x 32] * sU[32 x 32] on MFMA:
            // wave w owns rows [32w, 32w+32): 2 row-tiles x 2 col-tiles
            if (wave * 32 < rows) {
#pragma unroll
                for (int rt = 0; rt < 2; ++rt) {
                    const int rbase = wave * 32 + rt * 16;
                    f64x4 acc[2] = {f64x4{0, 0, 0, 0}, f64x4{0, 0, 0, 0}};
#pragma unroll
                    for (int kk = 0; kk < 8; ++kk) {
                        const int k = kk * 4 + fk;
                        const double a = sXp[cur][rbase + frow][k];
#pragma unroll
                        for (int ct = 0; ct < 2; ++ct)
                            acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(
                                a, sU[cur][k][ct * 16 + frow], acc[ct], 0, 0,
                                0);
                    }
#pragma unroll
                    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            sXj[rbase + 4 * q + fk][ct * 16 + frow] -=
                                acc[ct][q];
                }
            }
            if (pb + 32 < jb) write_bufs(cur ^ 1);
            __syncthreads();
            cur ^= 1;
        }
        // diagonal block into sU[0] for the solve
        for (int i = tid; i < 32 * 32; i += 256)
            sU[0][i >> 5][i & 31] =
                trans ? U[(int64_t)(jb + (i & 31)) * ldu + jb + (i >> 5)]
                      : U[(int64_t)(jb + (i >> 5)) * ldu + jb + (i & 31)];
        __syncthreads();
        if (tid < rows) {  // diagonal solve: thread = row, register triangle
            double x[32];
#pragma unroll
            for (int c = 0; c < 32; ++c) x[c] = sXj[tid][c];
#pragma unroll
            for (int c = 0; c < 32; ++c) {
                double acc = x[c];
#pragma unroll
                for (int i = 0; i < 32; ++i)
                    if (i < c) acc -= x[i] * sU[0][i][c];
                x[c] = acc / sU[0][c][c];
            }
#pragma unroll
            for (int c = 0; c < 32; ++c) sXj[tid][c] = x[c];
        }
        __syncthreads();
        for (int i = tid; i < rows * 32; i += 256)
            X[(r0 + (i >> 5)) * ldx + jb + (i & 31)] = sXj[i >> 5][i & 31];
    }
}

// X (v x N, row-major) <- L^-1 * X, L v x v unit lower.
#define TRM_COLS 128
__global__ __launch_bounds__(256) void k_trsm_left_mfma(
    const double *__restrict__ L, int64_t ldl, double *__restrict__ X,
    int64_t ldx, int v, int64_t N) {
    __shared__ double sXj[32][TRM_COLS + 1];
    __shared__ double sXp[2][32][TRM_COLS + 1];  // double-buffered
    __shared__ double sL[2][32][33];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int frow = lane & 15, fk = lane >> 4;
    const int64_t c0 = (int64_t)blockIdx.x * TRM_COLS;
    const int cols = (int)min((int64_t)TRM_COLS, N - c0);
    double rx[16], rl[4];  // 32x128 X panel + 32x32 L block per iteration
    auto load_l_regs = [&](int pb, int jb) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + i * 256;
            rl[i] = L[(int64_t)(jb + (e >> 5)) * ldl + pb + (e & 31)];
        }
    };
    auto load_x_regs = [&](int pb) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int e = tid + i * 256;
            rx[i] = (e & (TRM_COLS - 1)) < cols
                        ? X[(int64_t)(pb + (e >> 7)) * ldx + c0 +
                            (e & (TRM_COLS - 1))]
                        : 0.0;
        }
    };
    auto write_bufs = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int e = tid + i * 256;
            sXp[buf][e >> 7][e & (TRM_COLS - 1)] = rx[i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + i * 256;
            sL[buf][e >> 5][e & 31] = rl[i];
        }
    };
    for (int jb = 0; jb < v; jb += 32) {
        __syncthreads();
        for (int i = tid; i < 32 * TRM_COLS; i += 256)
            if ((i & (TRM_COLS - 1)) < cols)
                sXj[i >> 7][i & (TRM_COLS - 1)] =
                    X[(int64_t)(jb + (i >> 7)) * ldx + c0 +
                      (i & (TRM_COLS - 1))];
        int cur = 0;
        if (jb > 0) {
            load_x_regs(0);
            load_l_regs(0, jb);
            write_bufs(0);
        }
        __syncthreads();  // also covers the sXj stage
        for (int pb = 0; pb < jb; pb += 32) {
            if (pb + 32 < jb) {
                load_x_regs(pb + 32);
                load_l_regs(pb + 32, jb);
            }
            // sXj[32 x cols] -= sL[32 x 32] * sXp[32 x cols] on MFMA:
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
                        for (int rt = 0; rt < 2; ++rt)
                            acc[rt] = __builtin_amdgcn_mfma_f64_16x16x4f64(
                                sL[cur][rt * 16 + frow][k], b, acc[rt], 0, 0,
                                0);
                    }
#pragma unroll
                    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            sXj[rt * 16 + 4 * q + fk][cbase + frow] -=
                                acc[rt][q];
                }
            }
            if (pb + 32 < jb) write_bufs(cur ^ 1);
            __syncthreads();
            cur ^= 1;
        }
        for (int i = tid; i < 32 * 32; i += 256)
            sL[0][i >> 5][i & 31] =
                L[(int64_t)(jb + (i >> 5)) * ldl + jb + (i & 31)];
        __syncthreads();
        if (tid < cols) {  // diagonal solve: thread = column, unit lower
            double x[32];
#pragma unroll
            for (int r = 0; r < 32; ++r) x[r] = sXj[r][tid];
#pragma unroll
            for (int k = 0; k < 32; ++k) {
                const double xk = x[k];
#pragma unroll
                for (int r = 0; r < 32; ++r)
                    if (r > k) x[r] -= sL[0][r][k] * xk;
            }
#pragma unroll
            for (int r = 0; r < 32; ++r) sXj[r][tid] = x[r];
        }
        __syncthreads();
        for (int i = tid; i < 32 * TRM_COLS; i += 256)
            if ((i & (TRM_COLS - 1)) < cols)
                X[(int64_t)(jb + (i >> 7)) * ldx + c0 + (i & (TRM_COLS - 1))] =
                    sXj[i >> 7][i & (TRM_COLS - 1)];
    }
}

// ---------------------------------------------------------------------------
// Stripe-resident editions of the two fused solves.  The kernels above
// re-read every solved 32-wide panel of their stripe from global memory for
// each diagonal block (v/32 * (v/32 - 1) / 2 staged panels per launch, each
// a load -> LDS write -> barrier hop), which makes them latency chains whose
// time does not depend on the width of X.  Here a block loads a TRS_W-wide
// stripe ONCE, keeps all v/32 panels in LDS for its life and writes the
// stripe back once; inside the jb/pb loops only the 32x32 triangle blocks
// come from global memory (L2-resident, from a block-major copy made by
// k_trsm_pack_tri), prefetched into registers one item ahead of the barrier
// chain.  Every element sees the operations of the
// kernels above in the same order (left-looking over pb, a fresh accumulator
// per pb, the same eight MFMAs with k = 4*kk + fk, X -= acc, the same
// diagonal solve), so the results are bit-identical; rows (right) and
// columns (left) of X are independent, so the narrower stripe changes no sum.
// One wave per 16x16 output tile: 4 waves, one per SIMD, one block per CU.
// ---------------------------------------------------------------------------
#define TRS_W 32
#define TRS_MAXP 16  // panels resident: v <= 512 -> 18 * 8448 B = 148.5 KiB

// Every block of a stripe solve reads the whole triangle, one 32x32 block
// per item, all blocks at about the same time.  In place (ld = v = 512
// doubles) the 32 rows of a block lie 4 KiB apart, so the whole chip's reads
// of an item queue up on the few L2 channels those rows share.  The triangle
// is therefore first copied block-major (8 KiB contiguous per block, in the
// order the solves consume them: block (pb, jb), pb <= jb, at index
// jb/32 * (jb/32 + 1) / 2 + pb/32), already oriented as the solve stages it:
//   P[r][c] = T[(pb + r) * ld + jb + c]   swap = 0, tr = 0  (X U^-1)
//   P[r][c] = T[(jb + c) * ld + pb + r]   swap = 1, tr = 1  (X L^-T)
//   P[r][c] = T[(jb + r) * ld + pb + c]   swap = 1, tr = 0  (L^-1 X)
__global__ __launch_bounds__(256) void k_trsm_pack_tri(
    const double *__restrict__ T, int64_t ld, double *__restrict__ P, int swap,
    int tr) {
    int j = 0;
    while ((j + 1) * (j + 2) / 2 <= (int)blockIdx.x) ++j;
    const int pb = ((int)blockIdx.x - j * (j + 1) / 2) * 32, jb = j * 32;
    const int rb = swap ? jb : pb, cb = swap ? pb : jb;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int e = threadIdx.x + i * 256;
        const int r = e >> 5, c = e & 31;
        P[(int64_t)blockIdx.x * 1024 + e] =
            T[(int64_t)(rb + (tr ? c : r)) * ld + cb + (tr ? r : c)];
    }
}

__device__ inline int trs_blk(int pb, int jb) {
    return ((jb >> 5) * ((jb >> 5) + 1) / 2 + (pb >> 5)) * 1024;
}

// Xd (M x v, row-major) <- Xs * U^-1 or Xs * L^-T; U = the packed triangle.
// A block reads its stripe of Xs once and writes it to Xd once, so Xd may be
// Xs itself (the in-place solve: neither pointer is __restrict__) or another
// array with its own leading dimension; Xs is not written in that case.
__global__ __launch_bounds__(256) void k_trsm_right_stripe(
    const double *__restrict__ U, const double *Xs, int64_t lds, double *Xd,
    int64_t ldd, int v, int64_t M) {
    __shared__ double sX[TRS_MAXP][TRS_W][33];  // [panel][row][col]
    __shared__ double sU[2][32][33];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int frow = lane & 15, fk = lane >> 4;
    const int rt = wave >> 1, ct = wave & 1;  // this wave's 16x16 tile
    const int64_t r0 = (int64_t)blockIdx.x * TRS_W;
    const int rows = (int)min((int64_t)TRS_W, M - r0);
    double ru[4];
    auto load_u_regs = [&](int pb, int jb) {  // pb == jb: the diagonal block
#pragma unroll
        for (int i = 0; i < 4; ++i) ru[i] = U[trs_blk(pb, jb) + tid + i * 256];
    };
    auto write_u = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + i * 256;
            sU[buf][e >> 5][e & 31] = ru[i];
        }
    };
    load_u_regs(0, 0);
    for (int i = tid; i < TRS_W * v; i += 256) {
        const int r = i / v, cc = i - r * v;
        sX[cc >> 5][r][cc & 31] = r < rows ? Xs[(r0 + r) * lds + cc] : 0.0;
    }
    write_u(0);
    __syncthreads();
    int cur = 0;
    for (int jb = 0; jb < v; jb += 32) {
        double(*sXj)[33] = sX[jb >> 5];
        for (int pb = 0; pb < jb; pb += 32) {
            load_u_regs(pb + 32, jb);  // next update block, or the diagonal
            const double(*sXp)[33] = sX[pb >> 5];
            f64x4 acc = {0, 0, 0, 0};
#pragma unroll
            for (int kk = 0; kk < 8; ++kk) {
                const int k = kk * 4 + fk;
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(
                    sXp[rt * 16 + frow][k], sU[cur][k][ct * 16 + frow], acc, 0,
                    0, 0);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
                sXj[rt * 16 + 4 * q + fk][ct * 16 + frow] -= acc[q];
            write_u(cur ^ 1);
            __syncthreads();
            cur ^= 1;
        }
        // sU[cur] holds the diagonal block; fetch the next jb's first update
        // block behind the solve
        const bool more = jb + 32 < v;
        if (more) load_u_regs(0, jb + 32);
        if (tid < rows) {  // diagonal solve: thread = row, register triangle
            double x[32];
#pragma unroll
            for (int c = 0; c < 32; ++c) x[c] = sXj[tid][c];
#pragma unroll
            for (int c = 0; c < 32; ++c) {
                double acc = x[c];
#pragma unroll
                for (int i = 0; i < 32; ++i)
                    if (i < c) acc -= x[i] * sU[cur][i][c];
                x[c] = acc / sU[cur][c][c];
            }
#pragma unroll
            for (int c = 0; c < 32; ++c) sXj[tid][c] = x[c];
        }
        if (more) write_u(cur ^ 1);
        __syncthreads();
        cur ^= 1;
    }
    for (int i = tid; i < rows * v; i += 256) {
        const int r = i / v, cc = i - r * v;
        Xd[(r0 + r) * ldd + cc] = sX[cc >> 5][r][cc & 31];
    }
}

// Xd (v x N, row-major) <- L^-1 * Xs, L unit lower = the packed triangle;
// Xd == Xs is the in-place solve, as above.
__global__ __launch_bounds__(256) void k_trsm_left_stripe(
    const double *__restrict__ L, const double *Xs, int64_t lds, double *Xd,
    int64_t ldd, int v, int64_t N) {
    __shared__ double sX[TRS_MAXP][32][TRS_W + 1];  // [panel][k][col]
    __shared__ double sL[2][32][33];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int frow = lane & 15, fk = lane >> 4;
    const int rt = wave >> 1, ct = wave & 1;  // this wave's 16x16 tile
    const int64_t c0 = (int64_t)blockIdx.x * TRS_W;
    const int cols = (int)min((int64_t)TRS_W, N - c0);
    double rl[4];
    auto load_l_regs = [&](int pb, int jb) {  // pb == jb: the diagonal block
#pragma unroll
        for (int i = 0; i < 4; ++i) rl[i] = L[trs_blk(pb, jb) + tid + i * 256];
    };
    auto write_l = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + i * 256;
            sL[buf][e >> 5][e & 31] = rl[i];
        }
    };
    load_l_regs(0, 0);
    for (int i = tid; i < v * TRS_W; i += 256) {
        const int r = i >> 5, cc = i & (TRS_W - 1);
        sX[r >> 5][r & 31][cc] =
            cc < cols ? Xs[(int64_t)r * lds + c0 + cc] : 0.0;
    }
    write_l(0);
    __syncthreads();
    int cur = 0;
    for (int jb = 0; jb < v; jb += 32) {
        double(*sXj)[TRS_W + 1] = sX[jb >> 5];
        for (int pb = 0; pb < jb; pb += 32) {
            load_l_regs(pb + 32, jb);  // next update block, or the diagonal
            const double(*sXp)[TRS_W + 1] = sX[pb >> 5];
            f64x4 acc = {0, 0, 0, 0};
#pragma unroll
            for (int kk = 0; kk < 8; ++kk) {
                const int k = kk * 4 + fk;
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(
                    sL[cur][rt * 16 + frow][k], sXp[k][ct * 16 + frow], acc, 0,
                    0, 0);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
                sXj[rt * 16 + 4 * q + fk][ct * 16 + frow] -= acc[q];
            write_l(cur ^ 1);
            __syncthreads();
            cur ^= 1;
        }
        const bool more = jb + 32 < v;
        if (more) load_l_regs(0, jb + 32);
        if (tid < cols) {  // diagonal solve: thread = column, unit lower
            double x[32];
#pragma unroll
            for (int r = 0; r < 32; ++r) x[r] = sXj[r][tid];
#pragma unroll
            for (int k = 0; k < 32; ++k) {
                const double xk = x[k];
#pragma unroll
                for (int r = 0; r < 32; ++r)
                    if (r > k) x[r] -= sL[cur][r][k] * xk;
            }
#pragma unroll
            for (int r = 0; r < 32; ++r) sXj[r][tid] = x[r];
        }
        if (more) write_l(cur ^ 1);
        __syncthreads();
        cur ^= 1;
    }
    for (int i = tid; i < v * TRS_W; i += 256) {
        const int r = i >> 5, cc = i & (TRS_W - 1);
        if (cc < cols) Xd[(int64_t)r * ldd + c0 + cc] = sX[r >> 5][r & 31][cc];
    }
}

int conflux_trsm_stripe_width() { return TRS_W; }
bool conflux_trsm_stripe_fits(int v) {
    return v > 0 && v % 32 == 0 && v <= 32 * TRS_MAXP;
}

int64_t conflux_trsm_stripe_ws_doubles(int v) {
    const int64_t np = v / 32;
    return np * (np + 1) / 2 * 1024;
}

void launch_trsm_pack_tri(const double *T, int64_t ldt, int v, int swap,
                          int tr, double *ws, hipStream_t s) {
    if (v <= 0) return;
    const int nblk = (int)(conflux_trsm_stripe_ws_doubles(v) / 1024);
    hipLaunchKernelGGL(k_trsm_pack_tri, dim3(nblk), dim3(256), 0, s, T, ldt, ws,
                       swap, tr);
}

void launch_trsm_right_stripe_packed(const double *ws, const double *Xs,
                                     int64_t lds, double *Xd, int64_t ldd,
                                     int v, int64_t M, hipStream_t s) {
    if (M <= 0 || v <= 0) return;
    hipLaunchKernelGGL(k_trsm_right_stripe, dim3(cdiv64(M, TRS_W)), dim3(256),
                       0, s, ws, Xs, lds, Xd, ldd, v, M);
}

void launch_trsm_left_stripe_packed(const double *ws, const double *Xs,
                                    int64_t lds, double *Xd, int64_t ldd,
                                    int v, int64_t N, hipStream_t s) {
    if (N <= 0 || v <= 0) return;
    hipLaunchKernelGGL(k_trsm_left_stripe, dim3(cdiv64(N, TRS_W)), dim3(256),
                       0, s, ws, Xs, lds, Xd, ldd, v, N);
}

void launch_trsm_right_stripe(const double *U, int64_t ldu, double *X,
                              int64_t ldx, int v, int64_t M, int trans,
                              double *ws, hipStream_t s) {
    if (M <= 0 || v <= 0) return;
    launch_trsm_pack_tri(U, ldu, v, trans ? 1 : 0, trans ? 1 : 0, ws, s);
    launch_trsm_right_stripe_packed(ws, X, ldx, X, ldx, v, M, s);
}

void launch_trsm_left_stripe(const double *L, int64_t ldl, double *X,
                             int64_t ldx, int v, int64_t N, double *ws,
                             hipStream_t s) {
    if (N <= 0 || v <= 0) return;
    launch_trsm_pack_tri(L, ldl, v, 1, 0, ws, s);
    launch_trsm_left_stripe_packed(ws, X, ldx, X, ldx, v, N, s);
}

void launch_trsm_right_mfma(const double *U, int64_t ldu, double *X,
                            int64_t ldx, int v, int64_t M, int trans,
                            hipStream_t s) {
    if (M <= 0 || v <= 0) return;
    hipLaunchKernelGGL(k_trsm_right_mfma, dim3(cdiv64(M, TRM_ROWS)),
                       dim3(256), 0, s, U, ldu, X, ldx, v, M, trans);
}

void launch_trsm_left_mfma(const double *L, int64_t ldl, double *X,
                           int64_t ldx, int v, int64_t N, hipStream_t s) {
    if (N <= 0 || v <= 0) return;
    hipLaunchKernelGGL(k_trsm_left_mfma, dim3(cdiv64(N, TRM_COLS)), dim3(256),
                       0, s, L, ldl, X, ldx, v, N);
}

// validation helpers (the reference's CONFLUX_WITH_VALIDATION
// ||PA-LU||_F check, conflux_miniapp.cpp:169-507, without ScaLAPACK) --------
__global__ void k_tril_unit(const double *__restrict__ F, double *__restrict__ L,
                            int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < n * n; i += stride) {
        const int64_t r = i / n, c = i % n;
        L[i] = (r > c) ? F[i] : (r == c ? 1.0 : 0.0);
    }
}

__global__ void k_tril(const double *__restrict__ F, double *__restrict__ L,
                       int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < n * n; i += stride) {
        const int64_t r = i / n, c = i % n;
        L[i] = (r >= c) ? F[i] : 0.0;
    }
}

__global__ void k_triu(const double *__restrict__ F, double *__restrict__ U,
                       int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < n * n; i += stride) {
        const int64_t r = i / n, c = i % n;
        U[i] = (r <= c) ? F[i] : 0.0;
    }
}

// *out += sum A[i]^2 in two launches with a FIXED summation order: each block
// leaves its partial in ws[blockIdx.x], then one block adds the partials in
// index order.  (Blocks adding to *out atomically combine in arrival order,
// which made the validators' value differ in its last bits from run to run.)
__global__ void k_frob2_part(const double *__restrict__ A, int64_t n,
                             double *__restrict__ ws) {
    __shared__ double part[256];
    const int tid = threadIdx.x;
    double s = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < n;
         i += (int64_t)gridDim.x * 256)
        s += A[i] * A[i];
    part[tid] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) part[tid] += part[tid + w];
        __syncthreads();
    }
    if (tid == 0) ws[blockIdx.x] = part[0];
}

__global__ __launch_bounds__(256) void k_frob2_sum(
    const double *__restrict__ ws, int nparts, double *__restrict__ out) {
    __shared__ double part[256];
    const int tid = threadIdx.x;
    double s = 0;
    for (int i = tid; i < nparts; i += 256) s += ws[i];
    part[tid] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) part[tid] += part[tid + w];
        __syncthreads();
    }
    if (tid == 0) *out += part[0];
}

void launch_tril_unit(const double *F, double *L, int64_t n, hipStream_t s) {
    hipLaunchKernelGGL(k_tril_unit, dim3(cap_grid(n * n)), dim3(256), 0, s,
                       F, L, n);
}

// stripe variants for the streamed ||PA-LU|| validation: operate on a
// `rows`-row horizontal stripe whose first row is GLOBAL row `row0` of the
// factored matrix, so validation peaks at one N^2 buffer instead of five
// (bench-scale single-GPU sizes fit in HBM this way).
__global__ void k_tril_unit_rows(const double *__restrict__ F, int64_t ldf,
                                 double *__restrict__ L, int64_t ldl,
                                 int rows, int64_t row0, int64_t ncols) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < (int64_t)rows * ncols; i += stride) {
        const int64_t r = i / ncols, c = i % ncols, g = row0 + r;
        L[r * ldl + c] = (g > c) ? F[r * ldf + c] : (g == c ? 1.0 : 0.0);
    }
}

// zero the strict lower part of stripe rows in place (rows become pure U)
__global__ void k_triu_rows(double *__restrict__ F, int64_t ldf, int rows,
                            int64_t row0) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t w = row0 + rows;  // strict-lower cols are < global row < w
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < (int64_t)rows * w; i += stride) {
        const int64_t r = i / w, c = i % w;
        if (c < row0 + r) F[r * ldf + c] = 0.0;
    }
}

void launch_tril_unit_rows(const double *F, int64_t ldf, double *L,
                           int64_t ldl, int rows, int64_t row0, int64_t ncols,
                           hipStream_t s) {
    if (rows <= 0 || ncols <= 0) return;
    hipLaunchKernelGGL(k_tril_unit_rows, dim3(cap_grid((int64_t)rows * ncols)),
                       dim3(256), 0, s, F, ldf, L, ldl, rows, row0, ncols);
}

void launch_triu_rows(double *F, int64_t ldf, int rows, int64_t row0,
                      hipStream_t s) {
    if (rows <= 0) return;
    hipLaunchKernelGGL(k_triu_rows,
                       dim3(cap_grid((int64_t)rows * (row0 + rows))),
                       dim3(256), 0, s, F, ldf, rows, row0);
}
// A <- A + tril(A,-1)^T, i.e. mirror the strict lower triangle up (makes a
// lower-stored symmetric matrix explicit).  One thread per upper element.
__global__ void k_sym_mirror_up(double *__restrict__ A, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < n * n; i += stride) {
        const int64_t r = i / n, c = i % n;
        if (r < c) A[i] = A[c * n + r];
    }
}

void launch_transpose_add_lower(double *A, int64_t n, hipStream_t s) {
    hipLaunchKernelGGL(k_sym_mirror_up, dim3(cap_grid(n * n)), dim3(256),
                       0, s, A, n);
}

void launch_tril(const double *F, double *L, int64_t n, hipStream_t s) {
    hipLaunchKernelGGL(k_tril, dim3(cap_grid(n * n)), dim3(256), 0, s, F,
                       L, n);
}
void launch_triu(const double *F, double *U, int64_t n, hipStream_t s) {
    hipLaunchKernelGGL(k_triu, dim3(cap_grid(n * n)), dim3(256), 0, s, F,
                       U, n);
}
void launch_frob2(const double *A, int64_t nelem, double *out, double *ws,
                  hipStream_t s) {
    int blocks = (int)cdiv64(nelem, 256 * 16);
    if (blocks > CONFLUX_FROB2_WS_DOUBLES) blocks = CONFLUX_FROB2_WS_DOUBLES;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(k_frob2_part, dim3(blocks), dim3(256), 0, s, A, nelem,
                       ws);
    hipLaunchKernelGGL(k_frob2_sum, dim3(1), dim3(256), 0, s, ws, blocks, out);
}

void launch_potrf32(double *A, int64_t lda, int nb, hipStream_t s) {
    if (nb <= 0) return;
    hipLaunchKernelGGL(k_potrf32, dim3(1), dim3(256), 0, s, A, lda, nb);
}

void launch_getrf32_nopiv(double *A, int64_t lda, int nb, hipStream_t s) {
    if (nb <= 0) return;
    hipLaunchKernelGGL(k_getrf32_nopiv, dim3(1), dim3(256), 0, s, A, lda, nb);
}

// process-global GEMM launch switches: the environment gives the default on
// first use, the setters below override it and return the previous value
static int g_gemm_variant = -1;
static int g_gemm_strip_w = -1;
static int g_gemm_ntc = -1;

// 0 = GemmW4, 1 = GemmW8, 2 = k_dgemm_f64_glds, 3 = GemmBm256
static int gemm_variant() {
    if (g_gemm_variant < 0) {
        const char *e = getenv("CONFLUX_GEMM_VARIANT");
        g_gemm_variant = e ? atoi(e) : 1;
    }
    return g_gemm_variant;
}

static int gemm_strip_w() {  // strip width in tiles; 0/1 = flat order
    if (g_gemm_strip_w < 0) {
        const char *e = getenv("CONFLUX_GEMM_STRIP");
        g_gemm_strip_w = e ? std::max(0, atoi(e)) : 8;
    }
    return g_gemm_strip_w;
}

static int gemm_ntc() {  // non-temporal C epilogue (GemmW8)
    if (g_gemm_ntc < 0) {
        const char *e = getenv("CONFLUX_GEMM_NTC");
        g_gemm_ntc = e ? (atoi(e) != 0) : 0;
    }
    return g_gemm_ntc;
}

int conflux_gemm_set_variant(int variant) {
    const int prev = gemm_variant();
    g_gemm_variant = variant;
    return prev;
}

int conflux_gemm_set_strip_w(int w) {
    const int prev = gemm_strip_w();
    g_gemm_strip_w = std::max(0, w);
    return prev;
}

int conflux_gemm_set_ntc(int on) {
    const int prev = gemm_ntc();
    g_gemm_ntc = on != 0;
    return prev;
}

// k_dgemm_f64_glds stages whole 16-byte pieces and has no K tail: it may run
// only inside this envelope.  Outside it variant 2 launches GemmW8.
static bool gemm_glds_ok(const double *A, int64_t lda, const double *B,
                         int64_t ldb, int64_t N, int K) {
    return K % GEMM_BK == 0 && lda % 2 == 0 && ldb % 2 == 0 && N % 2 == 0 &&
           (uintptr_t)A % 16 == 0 && (uintptr_t)B % 16 == 0;
}

void launch_dgemm_f64(const double *A, int64_t lda, const double *B,
                      int64_t ldb, double *C, int64_t ldc, int M, int64_t N,
                      int K, hipStream_t s, int maxwg) {
    if (M <= 0 || N <= 0 || K <= 0) return;
    int variant = gemm_variant();
    if (variant == 2 && !gemm_glds_ok(A, lda, B, ldb, N, K)) variant = 1;
    const int ntm = (int)cdiv64(M, variant == 3 ? GemmBm256::BM : GEMM_BM);
    const int ntn = (int)cdiv64(N, GEMM_BN);
    const int sw = gemm_strip_w();
    int nwg = ntm * ntn;
    // cap (persistent edition only): leave CUs free for a concurrent panel
    if (maxwg > 0 && variant == 1 && nwg > maxwg) nwg = maxwg;
    if (variant == 3)
        hipLaunchKernelGGL(k_dgemm_mfma<GemmBm256>, dim3(nwg),
                           dim3(GemmBm256::TPB), 0, s, A, lda, B, ldb, C, ldc,
                           M, N, K, ntm, ntn, sw, GemmNoTail{});
    else if (variant == 2)
        hipLaunchKernelGGL(k_dgemm_f64_glds, dim3(nwg), dim3(512), 0, s,
                           A, lda, B, ldb, C, ldc, M, N, K, ntm, ntn, sw);
    else if (variant == 1)
        hipLaunchKernelGGL(k_dgemm_mfma<GemmW8>, dim3(nwg), dim3(GemmW8::TPB),
                           0, s, A, lda, B, ldb, C, ldc, M, N, K, ntm, ntn, sw,
                           gemm_ntc());
    else
        hipLaunchKernelGGL(k_dgemm_mfma<GemmW4>, dim3(nwg), dim3(GemmW4::TPB),
                           0, s, A, lda, B, ldb, C, ldc, M, N, K, ntm, ntn, sw,
                           GemmNoTail{});
}

void launch_dgemm_f64_nt(const double *A, int64_t lda, const double *B,
                         int64_t ldb, double *C, int64_t ldc, int M, int64_t N,
                         int K, hipStream_t s) {
    if (M <= 0 || N <= 0 || K <= 0) return;
    const int ntm = (int)cdiv64(M, GEMM_BM);
    const int ntn = (int)cdiv64(N, GEMM_BN);
    hipLaunchKernelGGL(k_dgemm_mfma<GemmW8NT>, dim3(ntm * ntn),
                       dim3(GemmW8NT::TPB), 0, s, A, lda, B, ldb, C, ldc, M, N,
                       K, ntm, ntn, gemm_strip_w(),
                       TriMask{0, 0, 0, 0, 0, 0, 0});
}

// Cholesky c4 single-launch variant: the trapezoid of v-tiles with global
// tile row >= tile col, launched as one rectangle with the TriMask.
// Requires v % 128 == 0 (caller falls back to per-tile launches otherwise).
void launch_dgemm_f64_nt_tril(const double *A, int64_t lda, const double *B,
                              int64_t ldb, double *C, int64_t ldc, int M,
                              int64_t N, int K, int v, int r0off,
                              int64_t c0off, int Px, int Py, int pi, int pj,
                              hipStream_t s) {
    if (M <= 0 || N <= 0 || K <= 0) return;
    const int ntm = (int)cdiv64(M, GEMM_BM);
    const int ntn = (int)cdiv64(N, GEMM_BN);
    hipLaunchKernelGGL(k_dgemm_mfma<GemmW8NT>, dim3(ntm * ntn),
                       dim3(GemmW8NT::TPB), 0, s, A, lda, B, ldb, C, ldc, M, N,
                       K, ntm, ntn, gemm_strip_w(),
                       TriMask{v, r0off, c0off, Px, Py, pi, pj});
}

void launch_pack_candidate(const double *A10, int64_t lda, const int *gri,
                           int f, int n_src, int n_out, int v, const int *idx,
                           double *cand, hipStream_t s) {
    if (n_out <= 0) return;
    hipLaunchKernelGGL(k_pack_candidate,
                       dim3(cdiv64((int64_t)n_out * (v + 1), 256)), dim3(256),
                       0, s, A10, lda, gri, f, n_src, n_out, v, idx, cand);
}

void launch_row_move(const double *src, int64_t lds, double *dst, int64_t ldd,
                     const int *src_idx, const int *dst_idx, int n_rows,
                     int64_t cols, hipStream_t s) {
    if (n_rows <= 0 || cols <= 0) return;
    hipLaunchKernelGGL(k_row_move, dim3(cap_grid((int64_t)n_rows * cols)),
                       dim3(256), 0, s, src, lds, dst, ldd, src_idx, dst_idx,
                       n_rows, cols);
}

void launch_extract_col0_int(const double *cand, int stride, int n, int *out,
                             hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_extract_col0_int, dim3(cdiv64(n, 256)), dim3(256), 0,
                       s, cand, stride, n, out);
}

void launch_slab_pack(const double *X, int64_t ldx, int n, int nlayr, int Pz,
                      double *out, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_slab_pack,
                       dim3(cdiv64((int64_t)n * nlayr * Pz, 256)), dim3(256),
                       0, s, X, ldx, n, nlayr, Pz, out);
}
