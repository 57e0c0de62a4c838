// engine.cpp — host orchestration of the MI355X-native CONFLUX LU engine.
//
// C++ host + HIP kernels behind the C ABI of include/conflux_lu.h.
// Re-implements the reference superstep loop conflux::LU_rep<double>
// (reference src/conflux/lu/conflux_opt.hpp:344-1827) MI355X-first:
//   * one process per GPU, RCCL point-to-point over xGMI instead of MPI
//     cartesian collectives (SURVEY.md §2 C1-C11 mapping; at the BASELINE
//     grids every exchange is <=2 ranks per dimension, so direct
//     ncclSend/ncclRecv beats ring collectives on 7-link xGMI),
//   * all per-rank compute as hand-written HIP kernels (kernels.hip),
//   * a single-process SIMULATION mode (rank == -1) that runs every rank's
//     state on one GPU with device-to-device copies as the transport — the
//     full multi-rank choreography is parity-tested on a 1-GPU box and the
//     distributed transport only swaps the copy layer for RCCL.
//
// Grid restrictions (de-facto reference envelope): Px == Py,
// power-of-two Px, v % Pz == 0, N % (v*Px) == 0, Ml >= 2v.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <numeric>
#include <string>
#include <set>
#include <vector>

#include "../../include/conflux_lu.h"
#include "kernels.hpp"
#include "norm1est.hpp"
#include "pivot_push.hpp"

#define HIPCHK(x)                                                       \
    do {                                                                \
        hipError_t e_ = (x);                                            \
        if (e_ != hipSuccess) {                                         \
            std::fprintf(stderr, "[conflux_lu] HIP error %s at %s:%d\n", \
                         hipGetErrorString(e_), __FILE__, __LINE__);    \
            return CONFLUX_LU_EHIP;                                     \
        }                                                               \
    } while (0)

#define NCCLCHK(x)                                                       \
    do {                                                                 \
        ncclResult_t e_ = (x);                                           \
        if (e_ != ncclSuccess) {                                         \
            std::fprintf(stderr, "[conflux_lu] RCCL error %s at %s:%d\n", \
                         ncclGetErrorString(e_), __FILE__, __LINE__);    \
            return CONFLUX_LU_ECOMM;                                     \
        }                                                                \
    } while (0)

namespace {

// a process knob: the integer the environment gives `name`, `def` where it
// is unset.  Callers that want it read once keep the result in a static.
int env_int(const char *name, int def) {
    const char *e = getenv(name);
    return e ? atoi(e) : def;
}

struct RankState {
    int pi = 0, pj = 0, pk = 0, grank = 0;
    // device buffers (fp64 unless noted)
    double *A11 = nullptr;      // Ml x Nl (working copy)
    double *A11in = nullptr;    // input snapshot (lazily allocated; the
                                // reference's LU_rep factors a COPY,
                                // conflux_opt.hpp:398)
    double *A10 = nullptr;      // Ml x v
    double *A01 = nullptr;      // v x Nl
    double *A10Rcv = nullptr;   // Ml x nlayr
    double *A01Rcv = nullptr;   // nlayr x Nl
    double *A10Rcv2 = nullptr;  // second set: the single-rank Cholesky
    double *A01Rcv2 = nullptr;  // lookahead double-buffers the slabs
    double *A00 = nullptr;      // v x v (packed LU of the pivot block)
    double *cand = nullptr;     // 2v x (v+1)
    double *panel = nullptr;    // max(2v, Ml) x v — getrf workspace
    double *cm = nullptr;       // col-major sub-panel scratch, Ml x PANEL_NB
    double *A01pack = nullptr;  // v x Nl — packed pivot rows
    double *rowtmp = nullptr;   // v x Nl — push/pack staging
    double *redtmp = nullptr;   // (Pz-1) x Ml x v — reduce recv staging
    double *slabs = nullptr;    // Ml x v — A10 slab pack
    double *Fres = nullptr;     // Ml x Nl (store_factors only)
    double *A10hist = nullptr;  // Ml x Nl (store_factors only)
    double *triws = nullptr;    // stripe-resident panel solves' scratch
    int *d_ipiv = nullptr;      // v
    int *d_swap = nullptr;      // 128: laswp dst/src row maps
    int *d_idx = nullptr;       // 4v: pivot rows / early / late / order
    int *d_gri = nullptr;       // Ml
    int *d_gpivots = nullptr;   // v
    int *d_perm = nullptr;      // max(2v, Ml)
    void *sync = nullptr;       // PanelSync
    // host bookkeeping (identical across pj, pk for fixed pi, tracked per rank)
    std::vector<int> gri;       // Ml: global row at each local position
    std::vector<int> igri;      // M: local position of a global row this
                                // rank row owns, -1 elsewhere
    int *h_idx = nullptr;       // pinned, 2 slots x 4v: staging for d_idx
    int fnp = 0, nact = 0;
};

struct TimeCat {
    double seconds = 0;
    long launches = 0;
    double flops = 0;
};

struct EvPair {
    hipEvent_t a, b;
    int cat;
    double flops;
};

// the process knobs of the LU step, resolved once per factorization by
// factor_loop (resolve_knobs); the step functions read nothing else
struct Knobs {
    bool split_trsm = true;  // CONFLUX_SPLIT_TRSM: the left solve on its own
                             // stream (read once per process)
    bool slice_trsm = true;  // CONFLUX_SLICE_TRSM: next panel's columns of
                             // the left solve first (once per process)
    bool lookahead = true;   // CONFLUX_LOOKAHEAD: next panel chain concurrent
                             // with the trailing update (once per
                             // factorization: tests set it between two)
    int gemm_cap = 432;      // CONFLUX_GEMM_CAP: grid cap of the trailing
                             // update under the look-ahead (once per process)
    bool gap_stats = false;  // CONFLUX_GAP_STATS (once per process)
};

struct Ctx {
    int N = 0, v = 0, Px = 1, Py = 1, Pz = 1;
    int M = 0, Ml = 0, Nl = 0, Nt = 0, Mt = 0, nlayr = 0, tA11x = 0, tA11y = 0;
    int world = 1, rank = 0;
    int n = 0;                   // logical order of the current input: the
                                 // leading n x n block is the caller's matrix,
                                 // the rest identity padding
                                 // (conflux_lu_set_matrix_device); N otherwise
    int nf = 0;                  // the same for the matrix last snapshotted,
                                 // i.e. the one the stored factors describe
    bool sim = false;            // all ranks in this process, 1 GPU
    bool input_dirty = true;     // A11 holds fresh input not yet snapshotted
    bool store_factors = true;
    int factored_kind = 0;       // stored factors a solve may use: 0 = none,
                                 // 1 = LU, 2 = Cholesky
    double anorm_inf = -1;       // ||A11in||inf for the refined solves; < 0 =
                                 // not computed since the last factorization
    double anorm_one = -1;       // ||A11in||1 for the condition estimate, same
    double anorm_lead[2] = {-1, -1};  // 1- and inf-norm of the leading nf x nf
                                 // block when nf < N, same lifetime
    int pivoting = 1;            // 1 = tournament (reference), 0 = none
                                 // (EmptyPivot fast path)
    bool have_comm = false;
    ncclComm_t comm{};
    ncclComm_t pcomm{};          // second comm for the lookahead panel chain
    bool have_pcomm = false;
    hipStream_t stream{};
    hipStream_t panel_stream{};  // lookahead stream (distributed mode)
    hipStream_t trsm_stream{};   // step-5 A01 solve (r02: its own stream —
                                 // on panel_stream it serialized against
                                 // the next panel chain, the saturated
                                 // pipeline: 175 of 213 ms busy)
    hipEvent_t ev_pc{};          // panel-columns-updated event
    hipEvent_t ev_t3{};          // step-3 complete (gates the step-5 TRSM)
    hipEvent_t ev_t5{};          // step-5 TRSM complete (gates the C9 spread)
    hipEvent_t ev_t5a{};         // panel-slice of the A01 solve complete
    std::vector<RankState> rs;   // size P (sim) or 1 (distributed)
    std::vector<int> pivotInds;  // M, global pivot ids (all ranks identical)
    unsigned epoch = 1;
    int direct = 0;              // one-rank direct bits of the factorization
                                 // in flight (ORD_*, set by factor_loop)
    Knobs knobs;                 // same lifetime, same place
    std::vector<EvPair> evs;
    size_t evs_used = 0;
    TimeCat cats[4];
    std::string err;
};

// c.stream names the stream every helper enqueues on.  A region that runs on
// another stream retargets it through this guard, which puts the previous
// stream back on every exit, error returns included.
struct StreamGuard {
    Ctx &c;
    hipStream_t saved;
    StreamGuard(Ctx &c_, hipStream_t s) : c(c_), saved(c_.stream) {
        c.stream = s;
    }
    ~StreamGuard() { c.stream = saved; }
    StreamGuard(const StreamGuard &) = delete;
    StreamGuard &operator=(const StreamGuard &) = delete;
};

inline int grank_of(const Ctx &c, int pi, int pj, int pk) {
    return (pi * c.Py + pj) * c.Pz + pk;  // MPI_Cart row-major order
}

inline int64_t i64(int a) { return (int64_t)a; }

int alloc_rank(Ctx &c, RankState &r, int pi, int pj, int pk) {
    r.pi = pi;
    r.pj = pj;
    r.pk = pk;
    r.grank = grank_of(c, pi, pj, pk);
    const int64_t Ml = c.Ml, Nl = c.Nl, v = c.v;
    const int64_t prows = std::max(i64(2 * c.v), Ml);
    HIPCHK(hipMalloc(&r.A11, Ml * Nl * 8));
    HIPCHK(hipMalloc(&r.A10, Ml * v * 8));
    HIPCHK(hipMalloc(&r.A01, v * Nl * 8));
    HIPCHK(hipMalloc(&r.A10Rcv, Ml * i64(c.nlayr) * 8));
    HIPCHK(hipMalloc(&r.A01Rcv, i64(c.nlayr) * Nl * 8));
    HIPCHK(hipMalloc(&r.A00, v * v * 8));
    HIPCHK(hipMalloc(&r.cand, i64(2 * c.v) * (v + 1) * 8));
    HIPCHK(hipMalloc(&r.panel, prows * v * 8));
    HIPCHK(hipMalloc(&r.A01pack, v * Nl * 8));
    HIPCHK(hipMalloc(&r.rowtmp, v * Nl * 8));
    HIPCHK(hipMalloc(&r.redtmp, i64(std::max(1, c.Pz - 1)) * Ml * v * 8));
    HIPCHK(hipMalloc(&r.slabs, Ml * v * 8));
    HIPCHK(hipMalloc(&r.d_ipiv, (v + 8) * 4));
    HIPCHK(hipMalloc(&r.d_swap, 128 * 4));
    HIPCHK(hipMalloc(&r.d_idx, 4 * v * 4));
    HIPCHK(hipMalloc(&r.d_gri, Ml * 4));
    HIPCHK(hipMalloc(&r.d_gpivots, v * 4));
    HIPCHK(hipMalloc(&r.d_perm, prows * 4));
    HIPCHK(hipMalloc(&r.sync, conflux_panel_sync_bytes()));
    HIPCHK(hipMemset(r.sync, 0, conflux_panel_sync_bytes()));
    HIPCHK(hipHostMalloc(&r.h_idx, size_t(2) * 4 * v * 4));
    std::memset(r.h_idx, 0, size_t(2) * 4 * v * 4);
    r.gri.resize(c.Ml);
    return 0;
}

int ensure_factor_bufs(Ctx &c, RankState &r, bool need_hist = true) {
    if (!r.Fres) HIPCHK(hipMalloc(&r.Fres, i64(c.Ml) * c.Nl * 8));
    if (need_hist && !r.A10hist)  // LU-only L-history (chol never reads it)
        HIPCHK(hipMalloc(&r.A10hist, i64(c.Ml) * c.Nl * 8));
    return 0;
}

void free_rank(RankState &r) {
    for (double *p : {r.A11, r.A11in, r.A10, r.A01, r.A10Rcv, r.A01Rcv,
                      r.A10Rcv2, r.A01Rcv2,
                      r.A00, r.cand, r.panel, r.cm, r.A01pack, r.rowtmp,
                      r.redtmp, r.slabs, r.Fres, r.A10hist, r.triws})
        if (p) (void)hipFree(p);
    for (int *p : {r.d_ipiv, r.d_swap, r.d_idx, r.d_gri, r.d_gpivots, r.d_perm})
        if (p) (void)hipFree(p);
    if (r.sync) (void)hipFree(r.sync);
    if (r.h_idx) (void)hipHostFree(r.h_idx);
}

// timing bracket helpers ----------------------------------------------------
int ev_begin(Ctx &c, int cat, double flops, size_t *slot) {
    if (c.evs_used >= c.evs.size()) {
        EvPair p;
        HIPCHK(hipEventCreate(&p.a));
        HIPCHK(hipEventCreate(&p.b));
        p.cat = 0;
        p.flops = 0;
        c.evs.push_back(p);
    }
    EvPair &p = c.evs[c.evs_used];
    p.cat = cat;
    p.flops = flops;
    *slot = c.evs_used++;
    HIPCHK(hipEventRecord(p.a, c.stream));
    return 0;
}
int ev_end(Ctx &c, size_t slot) {
    HIPCHK(hipEventRecord(c.evs[slot].b, c.stream));
    return 0;
}

// CONFLUX_NANCHECK=1 debug tracer: sync + sample a device buffer for
// non-finite values, print tag.  Zero overhead when the env is unset.
void nanscan(Ctx &c, const char *tag, int k, const double *p, int64_t nelem) {
    static const int on = env_int("CONFLUX_NANCHECK", 0);
    if (!on || !p || nelem <= 0) return;
    (void)hipStreamSynchronize(c.stream);
    const int64_t ns = std::min<int64_t>(nelem, 1 << 20);
    std::vector<double> s(ns);
    // sample the head and the tail halves
    (void)hipMemcpy(s.data(), p, (ns / 2) * 8, hipMemcpyDeviceToHost);
    (void)hipMemcpy(s.data() + ns / 2, p + nelem - (ns - ns / 2),
                    (ns - ns / 2) * 8, hipMemcpyDeviceToHost);
    long bad = 0, zeros = 0;
    double mn = 1e300, mx = 0;
    for (double x : s) {
        if (!std::isfinite(x)) {
            ++bad;
            continue;
        }
        const double a = std::fabs(x);
        if (a == 0) ++zeros;
        if (a > mx) mx = a;
        if (a < mn) mn = a;
    }
    std::fprintf(stderr,
                 "[nanscan] k=%d %-12s bad=%ld/%lld zeros=%ld min=%.3e "
                 "max=%.3e\n",
                 k, tag, bad, (long long)ns, zeros, mn, mx);
}

// ---------------------------------------------------------------------------
// panel getrf with partial pivoting on r.panel (n x v, ld = v), matching
// LAPACKE_dgetrf semantics (reference LUP, conflux_opt.hpp:143-166):
// ipiv_out[i] = absolute panel row swapped with row i at column i (0-based).
// ---------------------------------------------------------------------------
// CONFLUX_PANEL_GLUE: 1 (default) = the fused two-launch inter-leaf glue,
// 0 = the four-launch chain (rowperm pair, 32-wide solve, K=32 GEMM) it
// replaces — kept as the fallback for ragged leaves and as the reference the
// tests compare against.  Process-global; conflux_lu_debug_set_panel_glue
// overrides it.
int g_panel_glue = -1;
int panel_glue_mode() {
    if (g_panel_glue < 0) g_panel_glue = env_int("CONFLUX_PANEL_GLUE", 1) != 0;
    return g_panel_glue;
}

// CONFLUX_PANEL_PHASE_STATS=1: host-side totals of the instrumented leaf
// kernels' phase cycles (four phases over all blocks, then block 0's four)
// and the number of columns they cover; factor_panel adds to them after
// every panel, conflux_lu_debug_panel_phase_stats reads and resets them.
unsigned long long g_panel_phase_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
unsigned long long g_panel_phase_cols = 0;

int factor_panel(Ctx &c, RankState &r, int n, std::vector<int> &ipiv_out) {
    const int v = c.v;
    const int NB = conflux_panel_nb();
    const int nsteps = std::min(v, n);
    ipiv_out.assign(v, 0);
    size_t slot;
    if (ev_begin(c, 1, 0, &slot)) return CONFLUX_LU_EHIP;
    // A flat chain of NB-wide leaves.  (Two ablations that lost were taken
    // out: a recursive xGETRF2-shaped glue and a capped glue grid, DESIGN.md
    // section 9.)
    const int glue = panel_glue_mode();
    for (int jb = 0; jb < nsteps; jb += NB) {
        const int nb = std::min(NB, nsteps - jb);
        const int m = n - jb;  // rows of the sub-panel
        // fused glue (CONFLUX_PANEL_GLUE, default 1): a full 32-column
        // leaf with columns to its right and rows below it takes two
        // purpose-built launches, bitwise equal to the four-launch
        // chain below.  The last leaf of a panel (nothing to its right)
        // uses the prep kernel for its permutation alone.  Ragged
        // leaves and row-less updates stay on the chain.
        const bool fused = glue && nb == 32 && jb + nb < v && m > nb;
        const bool fused_perm = glue && nb == 32 && jb + nb == v && v > nb;
        // the leaf: persistent factor kernel, which composes the realized
        // sub-panel-relative permutation
        if (launch_panel_factor(r.panel + i64(jb) * v + jb, v, m, nb, r.sync,
                                r.d_ipiv + jb, c.epoch, r.d_swap,
                                r.d_swap + 64, c.stream)) {
            c.err = "panel grid not resident";
            return CONFLUX_LU_EINTERNAL;
        }
        c.epoch += nb;
        if (fused || fused_perm) {
            launch_panel_glue_prep(
                r.panel, v, r.d_swap, r.d_swap + 64, jb, v - nb,
                fused ? r.panel + i64(jb) * v + jb : nullptr, v, c.stream);
        } else if (v > nb) {
            // full-width rowperm, applied in two parallel passes over the
            // non-sub-panel columns
            launch_rowperm_skip(r.panel, v, r.d_swap, r.d_swap + 64, jb,
                                2 * nb, jb, nb, v - nb, r.rowtmp, c.stream);
        }
        if (fused) {
            launch_panel_glue_update(r.panel + i64(jb + nb) * v + jb, v,
                                     r.panel + i64(jb) * v + jb + nb, v,
                                     r.panel + i64(jb + nb) * v + jb + nb, v,
                                     m - nb, v - jb - nb, c.stream);
        } else if (jb + nb < v && m > nb) {
            // U block: rows jb..jb+nb of cols jb+nb..v
            launch_trsm_left_lower_unit32(r.panel + i64(jb) * v + jb, v,
                                          r.panel + i64(jb) * v + jb + nb, v,
                                          nb, v - jb - nb, c.stream);
            // trailing sub-panel update on the full grid
            launch_dgemm_f64(r.panel + i64(jb + nb) * v + jb, v,
                             r.panel + i64(jb) * v + jb + nb, v,
                             r.panel + i64(jb + nb) * v + jb + nb, v, m - nb,
                             v - jb - nb, nb, c.stream, 0);
        }
    }
    if (ev_end(c, slot)) return CONFLUX_LU_EHIP;
    // fetch ipiv + the err word of the sync struct (set by a key poll that
    // gave up): same stream, one sync
    std::vector<int> raw(v);
    unsigned int perr = 0;
    char *d_err = (char *)r.sync + conflux_panel_err_offset();
    HIPCHK(hipMemcpyAsync(raw.data(), r.d_ipiv, nsteps * 4,
                          hipMemcpyDeviceToHost, c.stream));
    HIPCHK(hipMemcpyAsync(&perr, d_err, 4, hipMemcpyDeviceToHost, c.stream));
    HIPCHK(hipStreamSynchronize(c.stream));
    if (perr) {
        HIPCHK(hipMemsetAsync(d_err, 0, 4, c.stream));
        if (perr >= 0x10000u)
            c.err = "panel hand-off timed out in the granule payload "
                    "re-read: column code " +
                    std::to_string(perr - 0x10000u) +
                    " (1 + sub-panel column)";
        else
            c.err = "panel hand-off timed out in the key poll: column code " +
                    std::to_string(perr) + " (1 + sub-panel column)";
        return CONFLUX_LU_EINTERNAL;
    }
    if (conflux_panel_phase_stats_mode()) {
        unsigned long long ph[8];
        conflux_panel_phase_read(r.sync, ph, c.stream);
        for (int i = 0; i < 8; ++i) g_panel_phase_acc[i] += ph[i];
        g_panel_phase_cols += nsteps;
    }
    for (int jb = 0; jb < nsteps; jb += NB) {
        const int nb = std::min(NB, nsteps - jb);
        for (int s = 0; s < nb; ++s) ipiv_out[jb + s] = jb + raw[jb + s];
    }
    return 0;
}

// perm from ipiv exactly as the reference builds it (conflux_opt.hpp:160-165)
void ipiv_to_perm(const std::vector<int> &ipiv, int n, int v,
                  std::vector<int> &perm) {
    perm.resize(std::max(2 * v, n));
    std::iota(perm.begin(), perm.end(), 0);
    for (int i = 0; i < std::min(v, n); ++i) std::swap(perm[i], perm[ipiv[i]]);
}

// CONFLUX_TRSM_STRIPE: 1 (default) = the stripe-resident fused solves (a
// block keeps its stripe of X in LDS for the whole triangle), 0 = the
// panel-streaming fused solves they replace — kept as the A/B baseline and
// as the bitwise reference the tests compare against.  Where the stripe does
// not fit the LDS for this v the streaming kernels run in either mode.
// Process-global; conflux_lu_debug_set_trsm_stripe overrides it.
int g_trsm_stripe = -1;
int trsm_stripe_mode() {
    if (g_trsm_stripe < 0)
        g_trsm_stripe = env_int("CONFLUX_TRSM_STRIPE", 1) != 0;
    return g_trsm_stripe;
}

// the stripe solves' scratch (block-major copy of the triangle): slot 0 for
// the right solve, slot 1 for the left solve, which may run concurrently
// which: 0 = the right solve's triangle, 1 = the left solve's; set: the
// one-rank direct path packs step k's pair into set k & 1 while step k-1's
// left solve may still read the other
int stripe_ws(RankState &r, int v, int which, double **ws, int set = 0) {
    const int64_t n = conflux_trsm_stripe_ws_doubles(v);
    if (!r.triws) HIPCHK(hipMalloc(&r.triws, 4 * n * 8));
    *ws = r.triws + (2 * set + which) * n;
    return 0;
}

// the fused single-launch solves on r.A00 (v % 32 == 0), by mode
int fused_trsm_right(RankState &r, double *X, int64_t ldx, int v, int64_t M,
                     int trans, hipStream_t s) {
    if (trsm_stripe_mode() && conflux_trsm_stripe_fits(v)) {
        double *ws;
        if (stripe_ws(r, v, 0, &ws)) return CONFLUX_LU_EHIP;
        launch_trsm_right_stripe(r.A00, v, X, ldx, v, M, trans, ws, s);
    } else
        launch_trsm_right_mfma(r.A00, v, X, ldx, v, M, trans, s);
    return 0;
}

int fused_trsm_left(RankState &r, double *X, int64_t ldx, int v, int64_t N,
                    hipStream_t s) {
    if (trsm_stripe_mode() && conflux_trsm_stripe_fits(v)) {
        double *ws;
        if (stripe_ws(r, v, 1, &ws)) return CONFLUX_LU_EHIP;
        launch_trsm_left_stripe(r.A00, v, X, ldx, v, N, ws, s);
    } else
        launch_trsm_left_mfma(r.A00, v, X, ldx, v, N, s);
    return 0;
}

// blocked TRSMs on full panels (diag blocks of PANEL_NB + MFMA updates) -----
// ---------------------------------------------------------------------------
// CONFLUX_ONE_RANK_DIRECT: on the one-rank grid (one process, Px = Py = Pz =
// 1, not simulated) the step between two panel chains need not mirror the
// distributed exchanges.  A bit mask, default 7, process-global;
// conflux_lu_debug_set_one_rank_direct overrides it:
//   1  the panel solves read A11 and write A10Rcv / A01Rcv directly, the
//      panel input is one copy, each triangle is packed once per step
//   2  the row push of A11 covers only the 2v columns the next panel chain
//      needs before the solves start; the rest follows on the solve stream
//   4  the column block of the panel just factored is neither solved for nor
//      updated (no later step reads it)
// 0 keeps the staged path of the distributed grids: the A/B baseline and the
// bitwise reference of tests/test_one_rank_direct_gpu.py.  No bit changes a
// floating-point operation on an element that is read afterwards.
enum { ORD_SOLVES = 1, ORD_PUSH = 2, ORD_DEAD = 4, ORD_ALL = 7 };
int g_one_rank_direct = -1;
int one_rank_direct_mode() {
    if (g_one_rank_direct < 0)
        g_one_rank_direct =
            env_int("CONFLUX_ONE_RANK_DIRECT", ORD_ALL) & ORD_ALL;
    return g_one_rank_direct;
}
// the bits in force on this engine; bit 1 needs the stripe solves
int one_rank_direct_bits(const Ctx &c) {
    if (c.sim || c.world != 1 || c.Px != 1 || c.Py != 1 || c.Pz != 1) return 0;
    int bits = one_rank_direct_mode();
    if (!(trsm_stripe_mode() && conflux_trsm_stripe_fits(c.v)))
        bits &= ~ORD_SOLVES;
    return bits;
}

// direct path: pack both triangles of A00 for step k (on c.stream, where A00
// was just written)
int pack_step_triangles(Ctx &c, RankState &r, int k) {
    double *wsu, *wsl;
    if (stripe_ws(r, c.v, 0, &wsu, k & 1) || stripe_ws(r, c.v, 1, &wsl, k & 1))
        return CONFLUX_LU_EHIP;
    launch_trsm_pack_tri(r.A00, c.v, c.v, 0, 0, wsu, c.stream);
    launch_trsm_pack_tri(r.A00, c.v, c.v, 1, 0, wsl, c.stream);
    return 0;
}

// direct path: Xd (M x v) <- Xs * U^-1 / Xd (v x N) <- L^-1 * Xs with step
// k's packed triangles; Xs is only read
int trsm_right_direct(Ctx &c, RankState &r, int k, const double *Xs,
                      int64_t lds, double *Xd, int64_t ldd, int64_t M) {
    double *ws;
    size_t slot;
    if (stripe_ws(r, c.v, 0, &ws, k & 1) || ev_begin(c, 2, 0, &slot))
        return CONFLUX_LU_EHIP;
    launch_trsm_right_stripe_packed(ws, Xs, lds, Xd, ldd, c.v, M, c.stream);
    return ev_end(c, slot);
}

int trsm_left_direct(Ctx &c, RankState &r, int k, const double *Xs,
                     int64_t lds, double *Xd, int64_t ldd, int64_t N) {
    double *ws;
    size_t slot;
    if (stripe_ws(r, c.v, 1, &ws, k & 1) || ev_begin(c, 2, 0, &slot))
        return CONFLUX_LU_EHIP;
    launch_trsm_left_stripe_packed(ws, Xs, lds, Xd, ldd, c.v, N, c.stream);
    return ev_end(c, slot);
}

int trsm_right_upper(Ctx &c, RankState &r, double *X, int64_t ldx, int M) {
    const int v = c.v, NB = conflux_panel_nb();
    size_t slot;
    if (ev_begin(c, 2, 0, &slot)) return CONFLUX_LU_EHIP;
    if (v % 32 == 0) {  // fused single-launch MFMA solve
        if (fused_trsm_right(r, X, ldx, v, M, 0, c.stream))
            return CONFLUX_LU_EHIP;
        return ev_end(c, slot);
    }
    for (int jb = 0; jb < v; jb += NB) {
        const int nb = std::min(NB, v - jb);
        launch_trsm_right_upper32(r.A00 + i64(jb) * v + jb, v, X + jb, ldx, nb,
                                  M, 0, c.stream);
        if (jb + nb < v)
            launch_dgemm_f64(X + jb, ldx, r.A00 + i64(jb) * v + jb + nb, v,
                             X + jb + nb, ldx, M, v - jb - nb, nb, c.stream);
    }
    return ev_end(c, slot);
}

int trsm_left_lower(Ctx &c, RankState &r, double *X, int64_t ldx, int64_t N) {
    const int v = c.v, NB = conflux_panel_nb();
    size_t slot;
    if (ev_begin(c, 2, 0, &slot)) return CONFLUX_LU_EHIP;
    if (v % 32 == 0) {  // fused single-launch MFMA solve
        if (fused_trsm_left(r, X, ldx, v, N, c.stream)) return CONFLUX_LU_EHIP;
        return ev_end(c, slot);
    }
    for (int jb = 0; jb < v; jb += NB) {
        const int nb = std::min(NB, v - jb);
        launch_trsm_left_lower_unit32(r.A00 + i64(jb) * v + jb, v,
                                      X + i64(jb) * ldx, ldx, nb, N, c.stream);
        if (jb + nb < v)
            launch_dgemm_f64(r.A00 + i64(jb + nb) * v + jb, v,
                             X + i64(jb) * ldx, ldx, X + i64(jb + nb) * ldx,
                             ldx, v - jb - nb, N, nb, c.stream);
    }
    return ev_end(c, slot);
}

// ---------------------------------------------------------------------------
// transport helpers: sim = device-to-device copies, dist = RCCL send/recv
// ---------------------------------------------------------------------------
RankState *get_rs(Ctx &c, int pi, int pj, int pk) {
    if (c.sim) return &c.rs[grank_of(c, pi, pj, pk)];
    RankState &me = c.rs[0];
    return (me.pi == pi && me.pj == pj && me.pk == pk) ? &me : nullptr;
}

int d2d(Ctx &c, double *dst, const double *src, int64_t n) {
    HIPCHK(hipMemcpyAsync(dst, src, n * 8, hipMemcpyDeviceToDevice, c.stream));
    return 0;
}

// The copy layer: one function per exchange pattern, each holding its own
// sim/dist branch.  The step functions say WHAT moves; nothing below reads
// c.stream before it is called, so the callers' stream swaps keep working.
using BufOf = std::function<double *(RankState &)>;

// C1/C7 depth reduce (MPI_Reduce conflux_opt.hpp:636, :1164): for every item,
// sum `count` doubles at bufof(rank) over the pk dimension of process column
// (pi, pj) onto layer 0, in deterministic pk-ascending order.  One call is
// one RCCL group.  `comm` is a parameter on purpose: the reduce used to read
// a mutable "current communicator" field that every step function had to set
// first, and the Cholesky step once forgot — its Pz>1 reduce ran on a NULL
// communicator (caught by the shimccl 2x2x2 distributed test).
struct ReduceItem {
    int pi, pj;
    int64_t count;
    BufOf bufof;
};

int depth_reduce(Ctx &c, ncclComm_t comm, const std::vector<ReduceItem> &items) {
    if (c.Pz == 1) return 0;
    if (c.sim) {
        for (const auto &it : items) {
            if (it.count <= 0) continue;
            RankState &root = *get_rs(c, it.pi, it.pj, 0);
            for (int pk = 1; pk < c.Pz; ++pk)
                launch_add2d(it.bufof(*get_rs(c, it.pi, it.pj, pk)), it.count,
                             it.bufof(root), it.count, 1, it.count, c.stream);
        }
        return 0;
    }
    RankState &me = c.rs[0];
    auto slot = [&](int pk) { return me.redtmp + i64(pk - 1) * c.Ml * c.v; };
    auto mine = [&](const ReduceItem &it) {
        return it.count > 0 && it.pi == me.pi && it.pj == me.pj;
    };
    NCCLCHK(ncclGroupStart());
    for (const auto &it : items) {
        if (!mine(it)) continue;
        if (me.pk != 0)
            NCCLCHK(ncclSend(it.bufof(me), it.count, ncclDouble,
                             grank_of(c, it.pi, it.pj, 0), comm, c.stream));
        else
            for (int pk = 1; pk < c.Pz; ++pk)
                NCCLCHK(ncclRecv(slot(pk), it.count, ncclDouble,
                                 grank_of(c, it.pi, it.pj, pk), comm,
                                 c.stream));
    }
    NCCLCHK(ncclGroupEnd());
    // the adds read the staged layers, so they come after the group closes
    for (const auto &it : items)
        if (mine(it) && me.pk == 0)
            for (int pk = 1; pk < c.Pz; ++pk)
                launch_add2d(slot(pk), it.count, it.bufof(me), it.count, 1,
                             it.count, c.stream);
    return 0;
}

// C8 column-slab spread: for each rank row pi, rows row0_of(rank)..Ml of the
// root (pi, kcol, 0)'s A10 (v wide) go to every (pi, pj, pk)'s A10Rcv as the
// pk-th nlayr-wide slab.  LU passes fnp (its active rows are fnp..Ml, i.e.
// nact = Ml - fnp), Cholesky and no-pivot LU pass f2.  Rank rows with no
// rows left move nothing; root and receivers share pi and every rank
// derives the row count from the same plan, so the skip is symmetric.
// Afterwards root->slabs holds the packed slabs (Cholesky's c3
// transpose-spread reads them); with Py == Pz == 1 there is a single slab,
// nothing is packed and A10Rcv itself is that slab.
int spread_col_slabs(Ctx &c, int kcol,
                     const std::function<int(const RankState &)> &row0_of) {
    const int v = c.v, Py = c.Py, Pz = c.Pz;
    for (auto &r : c.rs) {
        const int f = row0_of(r), n = c.Ml - f;
        const int64_t cnt = i64(n) * c.nlayr;
        double *src = r.A10 + i64(f) * v;
        if (Py == 1 && Pz == 1) {
            launch_copy2d(src, v, r.A10Rcv, c.nlayr, n, v, c.stream);
            continue;
        }
        if (n <= 0) continue;
        const bool root = r.pj == kcol && r.pk == 0;
        if (c.sim) {
            if (!root) continue;
            launch_slab_pack(src, v, n, c.nlayr, Pz, r.slabs, c.stream);
            for (int pj = 0; pj < Py; ++pj)
                for (int pk = 0; pk < Pz; ++pk)
                    if (d2d(c, get_rs(c, r.pi, pj, pk)->A10Rcv,
                            r.slabs + pk * cnt, cnt))
                        return CONFLUX_LU_EHIP;
            continue;
        }
        NCCLCHK(ncclGroupStart());
        if (root) {
            launch_slab_pack(src, v, n, c.nlayr, Pz, r.slabs, c.stream);
            for (int pj = 0; pj < Py; ++pj)
                for (int pk = 0; pk < Pz; ++pk) {
                    if (pj == kcol && pk == 0) continue;
                    NCCLCHK(ncclSend(r.slabs + pk * cnt, cnt, ncclDouble,
                                     grank_of(c, r.pi, pj, pk), c.comm,
                                     c.stream));
                }
        } else {
            NCCLCHK(ncclRecv(r.A10Rcv, cnt, ncclDouble,
                             grank_of(c, r.pi, kcol, 0), c.comm, c.stream));
        }
        NCCLCHK(ncclGroupEnd());
        if (root && d2d(c, r.A10Rcv, r.slabs, cnt)) return CONFLUX_LU_EHIP;
    }
    return 0;
}

// C9 row-panel spread: for each pj with w_of(pj) > 0, layer pk (nlayr rows)
// of the root (krow, pj, 0)'s A01 (v x w, ld w) goes to A01Rcv + off_of(pj)
// (ld Nl) on every (pi, pj, pk).  Receivers stage through redtmp.
int spread_row_panel(Ctx &c, int krow, const std::function<int64_t(int)> &w_of,
                     const std::function<int64_t(int)> &off_of) {
    const int Px = c.Px, Pz = c.Pz, nl = c.nlayr;
    for (int pj = 0; pj < c.Py; ++pj) {
        const int64_t w = w_of(pj), off = off_of(pj);
        if (w <= 0) continue;
        if (c.sim) {
            RankState &root = *get_rs(c, krow, pj, 0);
            for (int pi = 0; pi < Px; ++pi)
                for (int pk = 0; pk < Pz; ++pk)
                    launch_copy2d(root.A01 + i64(pk) * nl * w, w,
                                  get_rs(c, pi, pj, pk)->A01Rcv + off, c.Nl,
                                  nl, w, c.stream);
            continue;
        }
        RankState &me = c.rs[0];
        if (me.pj != pj) continue;
        const bool root = me.pi == krow && me.pk == 0;
        NCCLCHK(ncclGroupStart());
        if (root) {
            for (int pi = 0; pi < Px; ++pi)
                for (int pk = 0; pk < Pz; ++pk) {
                    if (pi == krow && pk == 0) continue;
                    NCCLCHK(ncclSend(me.A01 + i64(pk) * nl * w, i64(nl) * w,
                                     ncclDouble, grank_of(c, pi, pj, pk),
                                     c.comm, c.stream));
                }
        } else {
            NCCLCHK(ncclRecv(me.redtmp, i64(nl) * w, ncclDouble,
                             grank_of(c, krow, pj, 0), c.comm, c.stream));
        }
        NCCLCHK(ncclGroupEnd());
        launch_copy2d(root ? me.A01 : me.redtmp, w, me.A01Rcv + off, c.Nl, nl,
                      w, c.stream);
    }
    return 0;
}

// tile broadcast: `count` doubles at bufof(rank) go from global rank `root`
// to the global ranks `dests` (root excluded), sends posted in that order.
int bcast_tile(Ctx &c, const BufOf &bufof, int64_t count, int root,
               const std::vector<int> &dests) {
    if (c.sim) {
        for (int g : dests)
            if (d2d(c, bufof(c.rs[g]), bufof(c.rs[root]), count))
                return CONFLUX_LU_EHIP;
        return 0;
    }
    RankState &me = c.rs[0];
    const bool recv =
        std::find(dests.begin(), dests.end(), me.grank) != dests.end();
    if (dests.empty() || (me.grank != root && !recv)) return 0;
    NCCLCHK(ncclGroupStart());
    if (me.grank == root)
        for (int g : dests)
            NCCLCHK(ncclSend(bufof(me), count, ncclDouble, g, c.comm,
                             c.stream));
    else
        NCCLCHK(ncclRecv(bufof(me), count, ncclDouble, root, c.comm,
                         c.stream));
    NCCLCHK(ncclGroupEnd());
    return 0;
}

// barrier-fenced timed region (reference conflux_opt.hpp:531-532,1805-07):
// fence, run `body`, fence, then surface any failed launch and fold the
// event brackets `body` recorded into the category stats.
int timed_region(Ctx &c, double *elapsed_ms, const std::function<int()> &body) {
    auto fence = [&]() -> int {
        HIPCHK(hipStreamSynchronize(c.stream));
        if (c.have_comm) {
            // one-element allreduce as a device barrier
            static double *scratch = nullptr;
            if (!scratch) HIPCHK(hipMalloc(&scratch, 8));
            NCCLCHK(ncclAllReduce(scratch, scratch, 1, ncclDouble, ncclSum,
                                  c.comm, c.stream));
            HIPCHK(hipStreamSynchronize(c.stream));
        }
        return 0;
    };
    if (int rc = fence()) return rc;
    const auto t1 = std::chrono::high_resolution_clock::now();
    if (int rc = body()) return rc;
    if (int rc = fence()) return rc;
    const auto t2 = std::chrono::high_resolution_clock::now();
    HIPCHK(hipGetLastError());  // surface any failed launch loudly
    if (elapsed_ms)
        *elapsed_ms =
            std::chrono::duration<double, std::milli>(t2 - t1).count();
    for (size_t i = 0; i < c.evs_used; ++i) {
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, c.evs[i].a, c.evs[i].b));
        TimeCat &t = c.cats[c.evs[i].cat];
        t.seconds += ms * 1e-3;
        t.launches += 1;
        t.flops += c.evs[i].flops;
    }
    return 0;
}

}  // namespace

// ===========================================================================
// the superstep loop
// ===========================================================================
namespace {

struct StepPlan {
    // host bookkeeping shared by all ranks after the gpivots broadcast
    std::vector<int> gpivots;                    // v
    std::vector<std::vector<int>> lrows;         // per pi: global rows
    std::vector<std::vector<int>> order;         // per pi: pivot-order slots
    int n_early0 = 0;  // rank 0's early count of the push, for the sliced
                       // push's second part
};

// g2lnoTile (conflux_opt.cpp:74-98)
void plan_from_gpivots(Ctx &c, StepPlan &sp) {
    sp.lrows.assign(c.Px, {});
    sp.order.assign(c.Px, {});
    for (int i = 0; i < (int)sp.gpivots.size(); ++i) {
        const int g = sp.gpivots[i];
        const int pOwn = (g / c.v) % c.Px;
        sp.lrows[pOwn].push_back(g);
        sp.order[pOwn].push_back(i);
    }
}

int phase01(Ctx &c, int k, StepPlan &sp);
int run_step(Ctx &c, int k, StepPlan &sp);

// CONFLUX_GAP_STATS=1: host wall time of the serial stretch between two panel
// chains, accumulated over run_step calls and printed to stderr after each
// factorization: run_step entry -> first TRSM enqueue, the gri/igri update
// alone, run_step entry -> the ev_pc record.  Off by default (no clock reads).
using GapClock = std::chrono::steady_clock;
struct GapStats {
    double to_trsm = 0, gri = 0, to_evpc = 0;
    long steps = 0, evpc_steps = 0;
    GapClock::time_point t0;  // entry of the step in flight
};
GapStats g_gap;
inline double gap_ms(GapClock::time_point a, GapClock::time_point b) {
    return std::chrono::duration<double, std::milli>(b - a).count();
}

// The knobs of the factorization about to start.  CONFLUX_LOOKAHEAD is read
// here, once per factorization; the others keep their first value for the
// life of the process.
Knobs resolve_knobs() {
    static const int split = env_int("CONFLUX_SPLIT_TRSM", 1);
    // CONFLUX_SLICE_TRSM HISTORY: off by default from r02 to r06.  With r02's
    // fused TRSM, which streamed all previously-solved 32-wide L panels
    // through LDS once PER LAUNCH whatever the X width, the split nearly
    // tripled the solve cost (trsm 33 -> 65 ms/job) and the step was slower
    // (229.6 vs 201 ms at N=16384).  The r05 stripe solves are
    // width-proportional: re-measured in r07 (profiles/r07_leaf_body_ab.log)
    // the split costs 7 ms of solve time (trsm 22.5 -> 29.5 ms/job) and the
    // step is 5-6 ms FASTER in every alternated pair, so it is on by default
    // (CONFLUX_SLICE_TRSM=0 turns it off).  Same pivots either way.
    static const int slice = env_int("CONFLUX_SLICE_TRSM", 1);
    // r02 re-sweep with 256-row panel blocks: 432 ~= 400 (201.5 ms) > 448 >
    // 464 at N=16384
    static const int cap = env_int("CONFLUX_GEMM_CAP", 432);
    static const int gap = env_int("CONFLUX_GAP_STATS", 0);
    Knobs kn;
    kn.split_trsm = split != 0;
    kn.slice_trsm = slice != 0;
    kn.lookahead = env_int("CONFLUX_LOOKAHEAD", 1) != 0;
    kn.gemm_cap = cap;
    kn.gap_stats = gap != 0;
    return kn;
}

int factor_loop(Ctx &c, double *elapsed_ms) {
    // reset per-factor state
    for (auto &r : c.rs) {
        r.fnp = 0;
        r.nact = c.Ml;
        for (int i = 0; i < c.Ml; ++i)
            r.gri[i] = (i / c.v * c.Px + r.pi) * c.v + i % c.v;
        r.igri.assign(c.M, -1);
        for (int i = 0; i < c.Ml; ++i) r.igri[r.gri[i]] = i;
        HIPCHK(hipMemcpyAsync(r.d_gri, r.gri.data(), c.Ml * 4,
                              hipMemcpyHostToDevice, c.stream));
        if (c.store_factors) {
            if (ensure_factor_bufs(c, r)) return CONFLUX_LU_EHIP;
            launch_zero2d(r.Fres, c.Nl, c.Ml, c.Nl, c.stream);
            launch_zero2d(r.A10hist, c.Nl, c.Ml, c.Nl, c.stream);
        }
    }
    c.pivotInds.assign(c.M, -1);
    c.evs_used = 0;
    for (auto &t : c.cats) t = TimeCat{};
    g_gap = GapStats{};
    c.direct = one_rank_direct_bits(c);
    c.knobs = resolve_knobs();

    int rc = timed_region(c, elapsed_ms, [&]() -> int {
        StepPlan sp;
        int rc = phase01(c, 0, sp);
        if (rc) return rc;
        for (int k = 0; k < c.Nt; ++k) {
            rc = run_step(c, k, sp);
            if (rc) return rc;
        }
        return 0;
    });
    if (rc) return rc;
    static const int spin_stats = env_int("CONFLUX_SPIN_STATS", 0);
    if (spin_stats) {
        for (auto &r : c.rs) {
            unsigned long long sp2 = 0;
            conflux_panel_spin_read(r.sync, &sp2, c.stream);
            std::fprintf(stderr, "[spinstats] rank %d spins=%llu\n",
                         r.grank, sp2);
        }
    }
    if (conflux_panel_phase_stats_mode() && g_panel_phase_cols) {
        const unsigned long long *p = g_panel_phase_acc;
        std::fprintf(stderr,
                     "[phasestats] cols=%llu cycles all blocks: wait=%llu "
                     "load=%llu update=%llu publish=%llu | block 0: wait=%llu "
                     "load=%llu update=%llu publish=%llu\n",
                     g_panel_phase_cols, p[0], p[1], p[2], p[3], p[4], p[5],
                     p[6], p[7]);
        for (auto &x : g_panel_phase_acc) x = 0;
        g_panel_phase_cols = 0;
    }
    if (c.knobs.gap_stats)
        std::fprintf(stderr,
                     "[gapstats] steps=%ld entry->trsm=%.3f ms  gri/igri=%.3f "
                     "ms  entry->ev_pc=%.3f ms (%ld steps)\n",
                     g_gap.steps, g_gap.to_trsm, g_gap.gri, g_gap.to_evpc,
                     g_gap.evpc_steps);
    return 0;
}

// Geometry and mode of superstep k, computed once per step (make_step) from
// the grid, c.direct and c.knobs; no step function decides any of it again.
struct Step {
    int k = 0;
    int loff = 0;         // local column of the panel's block
    int kcol = 0, krow = 0;
    int64_t wA01 = 0;     // columns loff..Nl
    bool look = false;    // a step k+1 exists
    int ncol = 0;         // its process column
    int64_t lnext = 0;    // its local column
    // the two panel solves run on two streams (steps 4 & 5)
    bool split_trsm = false;
    // degenerate 1-rank grid: solve the v columns step k+1's panel needs
    // FIRST and record ev_t5a after them, so the (a) GEMM and the next panel
    // chain start without waiting for the rest of the A01 solve.  Only where
    // the next panel may run concurrently: in sequential mode
    // (CONFLUX_LOOKAHEAD=0) nothing waits for the slice and the split costs
    // its 7 ms for nothing.
    bool slice_first = false;
    // one-rank direct path (c.direct, see one_rank_direct_mode): direct =
    // the solves read A11 and write the Rcv buffers, nothing is staged in
    // A10 / A01pack / A01; sliced = only columns [loff, lnext + v) of A11 are
    // pushed before ev_t3, the rest on the solve stream behind the slice
    // solve; dead = the panel's own column block [loff, loff + v) is neither
    // solved for nor updated.  Stream and hazard argument: DESIGN.md section 1.
    bool direct = false, sliced = false;
    int64_t dead = 0;
    int64_t wfirst = 0;   // columns from loff pushed and packed before ev_t3
};

Step make_step(const Ctx &c, int k) {
    Step s;
    s.k = k;
    s.loff = (k / c.Py) * c.v;
    s.kcol = k % c.Py;
    s.krow = k % c.Px;
    s.wA01 = c.Nl - s.loff;
    s.look = k + 1 < c.Nt;
    s.ncol = (k + 1) % c.Py;
    s.lnext = i64(c.v) * ((k + 1) / c.Py);
    s.split_trsm = !c.sim && c.trsm_stream && c.knobs.split_trsm;
    s.slice_first = s.split_trsm && c.knobs.slice_trsm && c.Pz == 1 &&
                    c.Px == 1 && s.look && c.panel_stream && c.knobs.lookahead;
    s.direct = c.direct & ORD_SOLVES;
    s.sliced = (c.direct & ORD_PUSH) && s.slice_first;
    s.dead = (c.direct & ORD_DEAD) ? c.v : 0;
    s.wfirst = s.sliced ? s.lnext + c.v - s.loff : s.wA01;
    return s;
}

// ---- steps 0 and 1: the panel chain (phase01) -----------------------------

// dgetrf contract violated (ipiv[i] outside [i, n)): scan the panel input for
// non-finite data and say what was found
int ipiv_range_error(Ctx &c, RankState &r, int k, int i, int piv, int n) {
    std::vector<double> samp(i64(std::min(n, 4096)) * c.v);
    (void)hipMemcpy(samp.data(), r.panel, samp.size() * 8,
                    hipMemcpyDeviceToHost);
    long bad = 0;
    for (double x : samp)
        if (!std::isfinite(x)) ++bad;
    c.err = "panel ipiv out of range: k=" + std::to_string(k) +
            " i=" + std::to_string(i) + " ipiv=" + std::to_string(piv) +
            " n=" + std::to_string(n) + " nonfinite=" + std::to_string(bad) +
            "/" + std::to_string(samp.size()) +
            " panel[0]=" + std::to_string(samp[0]);
    return CONFLUX_LU_EINTERNAL;
}

// step 0: copy the active column block to A10, depth-reduce (C1).  One-rank
// direct: the column block goes straight into the panel and A10 is not
// written (its only readers are the push, the right solve and the slab
// spread of the staged path).
int reduce_panel_column(Ctx &c, const Step &st) {
    if (st.direct) return 0;
    const int v = c.v;
    for (auto &r : c.rs) {
        if (r.pj != st.kcol) continue;
        launch_copy2d(r.A11 + i64(r.fnp) * c.Nl + st.loff, c.Nl,
                      r.A10 + i64(r.fnp) * v, v, r.nact, v, c.stream);
    }
    // the panel chain's comm (it may overlap main-stream exchanges);
    // fnp/nact are the same on every rank of a rank row
    std::vector<ReduceItem> items;
    for (auto &r : c.rs)
        if (r.pj == st.kcol && (r.pk == 0 || !c.sim))
            items.push_back({r.pi, st.kcol, i64(r.nact) * v,
                             [v](RankState &x) {
                                 return x.A10 + i64(x.fnp) * v;
                             }});
    return depth_reduce(c, c.pcomm, items) ? CONFLUX_LU_ECOMM : 0;
}

// step 1, local part: big LUP on every rank's reduced column panel
// (conflux_opt.hpp:727), then either the result itself (Px == 1) or the
// winners as round-0 candidates
int factor_local_panels(Ctx &c, const Step &st, StepPlan &sp, int n_rounds) {
    const int v = c.v, k = st.k;
    std::vector<int> perm, ipiv;
    for (auto &r : c.rs) {
        if (r.pj != st.kcol || r.pk != 0) continue;
        const int n = r.nact;
        if (st.direct)
            launch_copy2d(r.A11 + i64(r.fnp) * c.Nl + st.loff, c.Nl, r.panel,
                          v, n, v, c.stream);
        else
            launch_copy2d(r.A10 + i64(r.fnp) * v, v, r.panel, v, n, v,
                          c.stream);
        ipiv.clear();
        if (n > 0) {
            if (factor_panel(c, r, n, ipiv)) return CONFLUX_LU_EINTERNAL;
            // dgetrf contract: ipiv[i] in [i, n) — catches any kernel-side
            // pivot corruption before it can index out of bounds below
            for (int i = 0; i < std::min(v, n); ++i)
                if (ipiv[i] < i || ipiv[i] >= n)
                    return ipiv_range_error(c, r, k, i, ipiv[i], n);
        }
        ipiv_to_perm(ipiv, n, v, perm);
        if (n == 0) std::iota(perm.begin(), perm.end(), 0);

        if (n_rounds == 0) {
            // Px == 1 (reference gap; intent): A00 = top v x v of factors,
            // gpivots = candidate col 0 gathered by perm — all host-side
            launch_copy2d(r.panel, v, r.A00, v, std::min(v, n), v, c.stream);
            if (st.direct && pack_step_triangles(c, r, k))
                return CONFLUX_LU_EHIP;
            for (int i = 0; i < v; ++i)
                sp.gpivots[i] = (perm[i] < n) ? r.gri[r.fnp + perm[i]] : 0;
            if (!c.sim && c.world > 1)  // feed the C4 broadcast
                HIPCHK(hipMemcpyAsync(r.d_gpivots, sp.gpivots.data(), v * 4,
                                      hipMemcpyHostToDevice, c.stream));
        } else {
            // winners = candidate rows perm[:v] (id col + A10 row), placed
            // top/bottom by the round-0 pairing (conflux_opt.hpp:724,741-751)
            HIPCHK(hipMemcpyAsync(r.d_perm, perm.data(), v * 4,
                                  hipMemcpyHostToDevice, c.stream));
            const int part0 = std::min(r.pi ^ 1, c.Px - 1);
            const int64_t off = (part0 < r.pi) ? i64(v) * (v + 1) : 0;
            launch_pack_candidate(r.A10, v, r.d_gri, r.fnp, n, v, v, r.d_perm,
                                  r.cand + off, c.stream);
        }
    }
    return 0;
}

// step 1, the tournament: per round, exchange halves with the butterfly
// partner (C2) and factor the merged 2v x v candidate
int tournament_rounds(Ctx &c, const Step &st, int n_rounds) {
    const int v = c.v, kcol = st.kcol;
    const int64_t half = i64(v) * (v + 1);
    std::vector<int> perm, ipiv;
    for (int rd = 0; rd < n_rounds; ++rd) {
        // each pair (lo,hi) ends with [lo winners ; hi winners]
        if (!c.sim) {
            RankState &me = c.rs[0];
            if (me.pj == kcol && me.pk == 0) {
                const int src = me.pi ^ (1 << rd);
                const int64_t soff = (src < me.pi) ? half : 0;
                const int64_t roff = half - soff;
                NCCLCHK(ncclGroupStart());
                NCCLCHK(ncclSend(me.cand + soff, half, ncclDouble,
                                 grank_of(c, src, kcol, 0), c.pcomm, c.stream));
                NCCLCHK(ncclRecv(me.cand + roff, half, ncclDouble,
                                 grank_of(c, src, kcol, 0), c.pcomm, c.stream));
                NCCLCHK(ncclGroupEnd());
            }
        } else {
            for (int pi = 0; pi < c.Px; ++pi) {
                const int src = pi ^ (1 << rd);
                if (src < pi) continue;  // handle each pair once
                RankState &lo = *get_rs(c, pi, kcol, 0);
                RankState &hi = *get_rs(c, src, kcol, 0);
                // lo's winners sit in its top half, hi's in its bottom half
                if (d2d(c, hi.cand, lo.cand, half)) return CONFLUX_LU_EHIP;
                if (d2d(c, lo.cand + half, hi.cand + half, half))
                    return CONFLUX_LU_EHIP;
            }
        }
        for (auto &r : c.rs) {
            if (r.pj != kcol || r.pk != 0) continue;
            // LUP on the merged 2v x v candidate (cols 1..v+1)
            launch_copy2d(r.cand + 1, v + 1, r.panel, v, 2 * v, v, c.stream);
            if (factor_panel(c, r, 2 * v, ipiv)) return CONFLUX_LU_EINTERNAL;
            ipiv_to_perm(ipiv, 2 * v, v, perm);
            HIPCHK(hipMemcpyAsync(r.d_perm, perm.data(), v * 4,
                                  hipMemcpyHostToDevice, c.stream));
            launch_row_gather(r.cand, v + 1, r.rowtmp, v + 1, r.d_perm, v,
                              v + 1, c.stream);
            if (rd == n_rounds - 1) {
                if (d2d(c, r.cand, r.rowtmp, half)) return CONFLUX_LU_EHIP;
                launch_copy2d(r.panel, v, r.A00, v, v, v, c.stream);
            } else {
                const int nxt = r.pi ^ (1 << (rd + 1));
                const int64_t off = (nxt < r.pi) ? half : 0;
                if (d2d(c, r.cand + off, r.rowtmp, half))
                    return CONFLUX_LU_EHIP;
            }
        }
    }
    return 0;
}

// after the tournament: gpivots out of candidate col 0
// (conflux_opt.hpp:810-816), A00 transpose-pair exchange (C3), gpivots
// broadcast (C4), and the download that ends the chain in a host sync
int exchange_a00_gpivots(Ctx &c, const Step &st, StepPlan &sp, int n_rounds) {
    const int v = c.v, kcol = st.kcol, krow = st.krow;
    if (n_rounds > 0)
        for (auto &r : c.rs) {
            if (r.pj != kcol || r.pk != 0) continue;
            launch_extract_col0_int(r.cand, v + 1, v, r.d_gpivots, c.stream);
        }
    if (!c.sim) {
        RankState &me = c.rs[0];
        NCCLCHK(ncclGroupStart());
        if (me.pj == kcol && me.pk == 0 && !(me.pi == krow && me.pj == kcol))
            NCCLCHK(ncclSend(me.A00, i64(v) * v, ncclDouble,
                             grank_of(c, krow, me.pi, 0), c.pcomm, c.stream));
        if (me.pi == krow && me.pk == 0 && !(me.pj == kcol))
            NCCLCHK(ncclRecv(me.A00, i64(v) * v, ncclDouble,
                             grank_of(c, me.pj, kcol, 0), c.pcomm, c.stream));
        // gpivots: root (pi, kcol, 0) -> its jk plane
        if (me.pj == kcol && me.pk == 0) {
            for (int pj = 0; pj < c.Py; ++pj)
                for (int pk = 0; pk < c.Pz; ++pk) {
                    if (pj == kcol && pk == 0) continue;
                    NCCLCHK(ncclSend(me.d_gpivots, v, ncclInt32,
                                     grank_of(c, me.pi, pj, pk), c.pcomm,
                                     c.stream));
                }
        } else {
            NCCLCHK(ncclRecv(me.d_gpivots, v, ncclInt32,
                             grank_of(c, me.pi, kcol, 0), c.pcomm, c.stream));
        }
        NCCLCHK(ncclGroupEnd());
        HIPCHK(hipMemcpyAsync(sp.gpivots.data(), me.d_gpivots, v * 4,
                              hipMemcpyDeviceToHost, c.stream));
    } else {
        // all participants hold identical winners; A00 lands on row krow
        RankState &part = *get_rs(c, 0, kcol, 0);
        HIPCHK(hipMemcpyAsync(sp.gpivots.data(), part.d_gpivots, v * 4,
                              hipMemcpyDeviceToHost, c.stream));
        for (int pi = 0; pi < c.Px; ++pi)
            for (int pj = 0; pj < c.Py; ++pj)
                if (pi == krow && pj != kcol)
                    if (d2d(c, get_rs(c, pi, pj, 0)->A00, part.A00,
                            i64(v) * v))
                        return CONFLUX_LU_EHIP;
    }
    HIPCHK(hipStreamSynchronize(c.stream));
    return 0;
}

// steps 0 and 1 of superstep k on c.stream: on return sp holds its pivot plan
int phase01(Ctx &c, int k, StepPlan &sp) {
    const Step st = make_step(c, k);
    const int n_rounds =
        c.Px > 1 ? (int)std::ceil(std::log2((double)c.Px)) : 0;
    sp.gpivots.assign(c.v, -1);
    if (int rc = reduce_panel_column(c, st)) return rc;
    if (int rc = factor_local_panels(c, st, sp, n_rounds)) return rc;
    if (int rc = tournament_rounds(c, st, n_rounds)) return rc;
    if (n_rounds > 0 || (!c.sim && c.world > 1))
        if (int rc = exchange_a00_gpivots(c, st, sp, n_rounds)) return rc;
    plan_from_gpivots(c, sp);
    std::copy_n(sp.gpivots.begin(), c.v, c.pivotInds.begin() + i64(k) * c.v);
    return 0;
}

// ---- steps 2..6 (run_step) ------------------------------------------------

// rows that move, one column window [col0, col0 + cols) of mat at a time:
// pivot rows to rowtmp, early rows down to the late positions, pivot rows to
// [f, f + cnt) (d_idx as uploaded by push_pivot_rows)
int push_rows(Ctx &c, RankState &r, double *mat, int64_t ld, int64_t col0,
              int64_t cols, int f, int cnt, int n_early) {
    const int v = c.v;
    size_t slot;
    if (ev_begin(c, 3, 0, &slot)) return CONFLUX_LU_EHIP;
    launch_row_gather(mat + col0, ld, r.rowtmp, cols, r.d_idx, cnt, cols,
                      c.stream);
    launch_row_move(mat + col0, ld, mat + col0, ld, r.d_idx + v,
                    r.d_idx + 2 * v, n_early, cols, c.stream);
    launch_copy2d(r.rowtmp, cols, mat + i64(f) * ld + col0, ld, cnt, cols,
                  c.stream);
    return ev_end(c, slot);
}

// step 2: push pivot rows up, pack, depth-reduce (C7)
int push_pivot_rows(Ctx &c, const Step &st, StepPlan &sp) {
    const int v = c.v, k = st.k;
    const int64_t Nl = c.Nl;
    for (auto &r : c.rs) {
        const auto &lr = sp.lrows[r.pi];
        const auto &ord = sp.order[r.pi];
        const int cnt = (int)lr.size();
        const int f = r.fnp;
        // this step's index lists are built in one pinned staging slot and
        // go up in one copy; layout (= d_idx): [0,v) lrows, [v,2v) early,
        // [2v,3v) late, [3v,4v) order.  Two slots alternate by step, so a
        // slot is rewritten only after a later step's panel download has
        // synchronized past the copy that read it.
        int *const stage = r.h_idx + (k & 1) * 4 * v;
        int *const lrows_loc = stage, *const early = stage + v,
                   *const late = stage + 2 * v;
        for (int i = 0; i < cnt; ++i) {
            const int p = (lr[i] >= 0 && lr[i] < c.M) ? r.igri[lr[i]] : -1;
            if (p < 0) {
                c.err = "pivot push: global row " + std::to_string(lr[i]) +
                        " is not on rank row " + std::to_string(r.pi) +
                        " (k=" + std::to_string(k) + ")";
                return CONFLUX_LU_EINTERNAL;
            }
            lrows_loc[i] = p;
            stage[3 * v + i] = ord[i];
        }
        int n_early = 0, n_late = 0;
        if (pivot_push::lists(lrows_loc, cnt, f, c.Ml, early, late, &n_early,
                              &n_late)) {
            std::set<int> uniq(lr.begin(), lr.end());
            c.err = "pivot push invariant: k=" + std::to_string(k) +
                    " cnt=" + std::to_string(cnt) +
                    " uniq=" + std::to_string(uniq.size()) +
                    " early=" + std::to_string(n_early) +
                    " late=" + std::to_string(n_late) +
                    " f=" + std::to_string(f);
            return CONFLUX_LU_EINTERNAL;
        }
        if (cnt)
            HIPCHK(hipMemcpyAsync(r.d_idx, stage, size_t(4) * v * 4,
                                  hipMemcpyHostToDevice, c.stream));
        sp.n_early0 = n_early;
        // (sliced: columns left of loff are not read again)
        if (st.sliced ? push_rows(c, r, r.A11, Nl, st.loff, st.wfirst, f, cnt,
                                  n_early)
                      : push_rows(c, r, r.A11, Nl, 0, Nl, f, cnt, n_early))
            return CONFLUX_LU_EHIP;
        if (!st.direct && push_rows(c, r, r.A10, v, 0, v, f, cnt, n_early))
            return CONFLUX_LU_EHIP;
        if (c.store_factors &&
            push_rows(c, r, r.A10hist, Nl, 0, Nl, f, cnt, n_early))
            return CONFLUX_LU_EHIP;
        // host gri/igri update (identical shuffle)
        GapClock::time_point gri_t0;
        if (c.knobs.gap_stats) gri_t0 = GapClock::now();
        pivot_push::apply(r.gri.data(), r.igri.data(), lrows_loc, cnt, f,
                          early, late, n_late);
        // d_gri's only device reader is the tournament's candidate pack
        // (factor_local_panels, grids with Px > 1); positions outside [f,
        // last late row] did not change
        if (c.Px > 1 && cnt) {
            const int hi = n_late ? late[n_late - 1] + 1 : f + cnt;
            HIPCHK(hipMemcpyAsync(r.d_gri + f, r.gri.data() + f,
                                  size_t(hi - f) * 4, hipMemcpyHostToDevice,
                                  c.stream));
        }
        if (c.knobs.gap_stats) g_gap.gri += gap_ms(gri_t0, GapClock::now());
        r.fnp += cnt;
        r.nact -= cnt;
        // pack pivot rows cols loff.. for the depth reduce
        if (!st.direct)
            launch_copy2d(r.A11 + i64(f) * Nl + st.loff, Nl, r.A01pack,
                          st.wA01, cnt, st.wfirst, c.stream);
    }
    std::vector<ReduceItem> items;
    for (int pi = 0; pi < c.Px; ++pi)
        for (int pj = 0; pj < c.Py; ++pj)
            items.push_back({pi, pj, i64(sp.lrows[pi].size()) * st.wA01,
                             [](RankState &x) { return x.A01pack; }});
    return depth_reduce(c, c.comm, items) ? CONFLUX_LU_ECOMM : 0;
}

// step 3: route packed pivot rows to row krow, pivot-ordered (C5/C6).
// One-rank direct: nothing, the left solve reads the pivot rows where the
// push left them.
int route_pivot_rows(Ctx &c, const Step &st, StepPlan &sp) {
    if (st.direct) return 0;
    const int v = c.v, Px = c.Px, krow = st.krow;
    const int64_t wA01 = st.wA01;
    if (c.sim) {
        for (int pj = 0; pj < c.Py; ++pj) {
            RankState &dst = *get_rs(c, krow, pj, 0);
            for (int pi = 0; pi < Px; ++pi) {
                RankState &src = *get_rs(c, pi, pj, 0);
                const int cnt = (int)sp.lrows[pi].size();
                if (!cnt) continue;
                HIPCHK(hipMemcpyAsync(dst.d_idx, sp.order[pi].data(), cnt * 4,
                                      hipMemcpyHostToDevice, c.stream));
                launch_row_scatter(src.A01pack, wA01, dst.A01, wA01, dst.d_idx,
                                   cnt, wA01, c.stream);
            }
        }
        return 0;
    }
    RankState &me = c.rs[0];
    if (me.pk != 0) return 0;
    NCCLCHK(ncclGroupStart());
    if (me.pi != krow) {
        const int cnt = (int)sp.lrows[me.pi].size();
        if (cnt)
            NCCLCHK(ncclSend(me.A01pack, i64(cnt) * wA01, ncclDouble,
                             grank_of(c, krow, me.pj, 0), c.comm, c.stream));
    } else {
        int64_t off = 0;
        for (int pi = 0; pi < Px; ++pi) {
            if (pi == krow) continue;
            const int cnt = (int)sp.lrows[pi].size();
            if (cnt)
                NCCLCHK(ncclRecv(me.redtmp + off, i64(cnt) * wA01, ncclDouble,
                                 grank_of(c, pi, me.pj, 0), c.comm, c.stream));
            off += i64(cnt) * wA01;
        }
    }
    NCCLCHK(ncclGroupEnd());
    if (me.pi != krow) return 0;
    // scatter own + received rows into A01 by pivot order
    const int cnt_own = (int)sp.lrows[krow].size();
    if (cnt_own) {
        HIPCHK(hipMemcpyAsync(me.d_idx + 3 * v, sp.order[krow].data(),
                              cnt_own * 4, hipMemcpyHostToDevice, c.stream));
        launch_row_scatter(me.A01pack, wA01, me.A01, wA01, me.d_idx + 3 * v,
                           cnt_own, st.wfirst, c.stream);
    }
    int64_t off = 0;
    for (int pi = 0; pi < Px; ++pi) {
        if (pi == krow) continue;
        const int cnt = (int)sp.lrows[pi].size();
        if (cnt) {
            HIPCHK(hipMemcpyAsync(me.d_idx, sp.order[pi].data(), cnt * 4,
                                  hipMemcpyHostToDevice, c.stream));
            launch_row_scatter(me.redtmp + off, wA01, me.A01, wA01, me.d_idx,
                               cnt, wA01, c.stream);
        }
        off += i64(cnt) * wA01;
    }
    return 0;
}

// store_factors: ship this step's pivot rows' L history to row krow (C10).
// Source: hist rows fnp-cnt..fnp (post-push); destination: Fres rows
// ltik*v + order[i].
int ship_history(Ctx &c, const Step &st, StepPlan &sp) {
    if (!c.store_factors || st.k == 0) return 0;
    const int v = c.v, k = st.k, krow = st.krow;
    const int64_t Nl = c.Nl;
    const int ltik = k / c.Px;  // local row-tile of global tile k on row krow
    for (int pj = 0; pj < c.Py; ++pj) {
        const int64_t histcols =
            i64(v) * (pj < st.kcol ? k / c.Py + 1 : k / c.Py);
        if (histcols == 0) continue;
        for (int pi = 0; pi < c.Px; ++pi) {
            const int cnt = (int)sp.lrows[pi].size();
            if (!cnt) continue;
            RankState *src = get_rs(c, pi, pj, 0);
            RankState *dst = get_rs(c, krow, pj, 0);
            if (c.sim) {
                HIPCHK(hipMemcpyAsync(dst->d_idx + 2 * v, sp.order[pi].data(),
                                      cnt * 4, hipMemcpyHostToDevice,
                                      c.stream));
                launch_row_scatter(src->A10hist + i64(src->fnp - cnt) * Nl, Nl,
                                   dst->Fres + i64(ltik) * v * Nl, Nl,
                                   dst->d_idx + 2 * v, cnt, histcols,
                                   c.stream);
                continue;
            }
            RankState &me = c.rs[0];
            if (src && dst) {
                // (sliced: the second part of the A11 push still needs the
                // late list at d_idx + 2v; the order list of this one rank
                // row is already at d_idx + 3v)
                int *const d_ord = me.d_idx + (st.sliced ? 3 : 2) * v;
                if (!st.sliced)
                    HIPCHK(hipMemcpyAsync(d_ord, sp.order[pi].data(), cnt * 4,
                                          hipMemcpyHostToDevice, c.stream));
                launch_row_scatter(me.A10hist + i64(me.fnp - cnt) * Nl, Nl,
                                   me.Fres + i64(ltik) * v * Nl, Nl, d_ord,
                                   cnt, histcols, c.stream);
            } else if (src) {
                launch_copy2d(me.A10hist + i64(me.fnp - cnt) * Nl, Nl,
                              me.rowtmp, histcols, cnt, histcols, c.stream);
                NCCLCHK(ncclSend(me.rowtmp, i64(cnt) * histcols, ncclDouble,
                                 grank_of(c, krow, pj, 0), c.comm, c.stream));
            } else if (dst) {
                NCCLCHK(ncclRecv(me.rowtmp, i64(cnt) * histcols, ncclDouble,
                                 grank_of(c, pi, pj, 0), c.comm, c.stream));
                HIPCHK(hipMemcpyAsync(me.d_idx + 2 * v, sp.order[pi].data(),
                                      cnt * 4, hipMemcpyHostToDevice,
                                      c.stream));
                launch_row_scatter(me.rowtmp, histcols,
                                   me.Fres + i64(ltik) * v * Nl, Nl,
                                   me.d_idx + 2 * v, cnt, histcols, c.stream);
            }
        }
    }
    return 0;
}

// store_factors: the solved U rows (and the diagonal tile) go to Fres, on
// whichever stream the solve ran
void store_u(Ctx &c, const Step &st, RankState &r) {
    if (!c.store_factors) return;
    const int v = c.v, k = st.k;
    const int64_t Nl = c.Nl;
    double *Frow = r.Fres + i64(k / c.Px) * v * Nl;  // local row tile of k
    // U region starts at this rank's first local column tile with global
    // tile >= k; columns left of it carry stale already-factored data the
    // reference never reads (cf. oracle lu_oracle.py step-5 `gcs >= off`
    // mask)
    // (dead: the diagonal tile's columns were not solved for; A00 below)
    const int64_t ustart =
        i64(v) * (r.pj < st.kcol ? k / c.Py + 1 : k / c.Py) + st.dead;
    if (Nl - ustart > 0 && st.direct)
        launch_copy2d(r.A01Rcv + (ustart - st.loff), Nl, Frow + ustart, Nl, v,
                      Nl - ustart, c.stream);
    else if (Nl - ustart > 0)
        launch_copy2d(r.A01 + (ustart - st.loff), st.wA01, Frow + ustart, Nl,
                      v, Nl - ustart, c.stream);
    if (r.pj == st.kcol)  // diagonal tile: packed LU from A00
        launch_copy2d(r.A00, v, Frow + st.loff, Nl, v, v, c.stream);
}

// step-5 solve of columns [loff + c0, loff + c0 + w): in place in A01, or
// direct from the pivot rows in A11 (rows [fnp - v, fnp) after the push)
// into A01Rcv
int solve_left(Ctx &c, const Step &st, RankState &r, int64_t c0, int64_t w) {
    if (w <= 0) return 0;
    if (st.direct)
        return trsm_left_direct(
            c, r, st.k, r.A11 + i64(r.fnp - c.v) * c.Nl + st.loff + c0, c.Nl,
            r.A01Rcv + c0, c.Nl, w);
    return trsm_left_lower(c, r, r.A01 + c0, st.wA01, w);
}

// slice-first: what follows the slice on the solve stream (c.stream here)
int solve_rest(Ctx &c, const Step &st, const StepPlan &sp, RankState &r) {
    const int v = c.v;
    const int64_t Nl = c.Nl, s0 = st.lnext - st.loff;
    if (st.sliced) {
        // the columns the (b) pieces and later steps read
        const int64_t wrest = Nl - (st.lnext + v);
        if (wrest > 0 && push_rows(c, r, r.A11, Nl, st.lnext + v, wrest,
                                   r.fnp - v, v, sp.n_early0))
            return CONFLUX_LU_EHIP;
        if (wrest > 0 && !st.direct) {
            launch_copy2d(r.A11 + i64(r.fnp - v) * Nl + st.lnext + v, Nl,
                          r.A01pack + st.wfirst, st.wA01, v, wrest, c.stream);
            launch_row_scatter(r.A01pack + st.wfirst, st.wA01,
                               r.A01 + st.wfirst, st.wA01, r.d_idx + 3 * v, v,
                               wrest, c.stream);
        }
    }
    if (st.dead < s0 && solve_left(c, st, r, st.dead, s0 - st.dead))
        return CONFLUX_LU_EINTERNAL;
    if (solve_left(c, st, r, s0 + v, st.wA01 - s0 - v))
        return CONFLUX_LU_EINTERNAL;
    store_u(c, st, r);
    return 0;
}

// Steps 4 & 5 compute: the two panel TRSMs are independent after step 3, so
// with split_trsm the step-5 TRSM is issued here on the solve stream and runs
// concurrently with the step-4 TRSM (the spreads stay ordered on the main
// stream, C8 overlapping the step-5 solve like the reference's Iscatterv
// window, conflux_opt.hpp:1424-1615).
int start_left_solve(Ctx &c, const Step &st, const StepPlan &sp) {
    if (!st.split_trsm) return 0;
    HIPCHK(hipEventRecord(c.ev_t3, c.stream));
    HIPCHK(hipStreamWaitEvent(c.trsm_stream, c.ev_t3, 0));
    StreamGuard on_solve_stream(c, c.trsm_stream);
    for (auto &r : c.rs) {
        if (r.pi != st.krow || r.pk != 0) continue;
        if (!st.slice_first) {
            if (solve_left(c, st, r, st.dead, st.wA01 - st.dead))
                return CONFLUX_LU_EINTERNAL;
            store_u(c, st, r);
            continue;
        }
        // the slice starts at lnext - loff in A01
        if (solve_left(c, st, r, st.lnext - st.loff, c.v))
            return CONFLUX_LU_EINTERNAL;
        HIPCHK(hipEventRecord(c.ev_t5a, c.stream));
        // sliced: the rest is enqueued behind the (a) GEMM
        // (finish_left_solve).  Started here, its 32-column blocks (one per
        // CU, the whole LDS) take the CUs from under (a), which is on the
        // critical path and then runs 2.5x as long
        // (profiles/r08_gap_after.csv)
        if (!st.sliced)
            if (int rc = solve_rest(c, st, sp, r)) return rc;
    }
    if (!st.sliced) HIPCHK(hipEventRecord(c.ev_t5, c.stream));
    return 0;
}

// step 4: A10 <- A10 U^-1, slab-split, spread (C8)
int right_solve_and_spread(Ctx &c, const Step &st) {
    const int v = c.v, k = st.k;
    const int64_t Nl = c.Nl;
    for (auto &r : c.rs) {
        if (r.pj != st.kcol || r.pk != 0) continue;
        if (st.direct) {
            // source: the panel's column block of A11 below the pivot rows
            // (what the pushed A10 holds on the staged path), untouched;
            // destination: the GEMM operand itself, no slab spread
            nanscan(c, "A00", k, r.A00, i64(v) * v);
            if (r.nact > 0 &&
                trsm_right_direct(c, r, k, r.A11 + i64(r.fnp) * Nl + st.loff,
                                  Nl, r.A10Rcv, c.nlayr, r.nact))
                return CONFLUX_LU_EINTERNAL;
            if (c.store_factors)
                launch_copy2d(r.A10Rcv, c.nlayr,
                              r.A10hist + i64(r.fnp) * Nl + st.loff, Nl,
                              r.nact, v, c.stream);
            continue;
        }
        nanscan(c, "A10.pre", k, r.A10 + i64(r.fnp) * v, i64(r.nact) * v);
        nanscan(c, "A00", k, r.A00, i64(v) * v);
        if (trsm_right_upper(c, r, r.A10 + i64(r.fnp) * v, v, r.nact))
            return CONFLUX_LU_EINTERNAL;
        nanscan(c, "A10.post", k, r.A10 + i64(r.fnp) * v, i64(r.nact) * v);
        if (c.store_factors)
            launch_copy2d(r.A10 + i64(r.fnp) * v, v,
                          r.A10hist + i64(r.fnp) * Nl + st.loff, Nl, r.nact, v,
                          c.stream);
    }
    if (st.direct) return 0;
    return spread_col_slabs(c, st.kcol,
                            [](const RankState &r) { return r.fnp; });
}

// step 5: A01 <- L^-1 A01 (already issued on the solve stream when
// split_trsm; the C9 spread waits for it), spread (C9)
int left_solve_and_spread(Ctx &c, const Step &st) {
    const int64_t Nl = c.Nl, wA01 = st.wA01;
    if (!st.split_trsm) {
        for (auto &r : c.rs) {
            if (r.pi != st.krow || r.pk != 0) continue;
            if (solve_left(c, st, r, st.dead, wA01 - st.dead))
                return CONFLUX_LU_EINTERNAL;
            store_u(c, st, r);
        }
    } else if (!st.slice_first) {
        HIPCHK(hipStreamWaitEvent(c.stream, c.ev_t5, 0));
    }
    if (c.Pz != 1 || c.Px != 1)
        return spread_row_panel(
            c, st.krow, [wA01](int) { return wA01; },
            [](int) { return int64_t(0); });
    RankState &r = c.rs[0];
    if (c.sim)
        for (auto &x : c.rs)
            launch_copy2d(x.A01, wA01, x.A01Rcv, Nl, c.nlayr, wA01, c.stream);
    else if (st.slice_first) {
        // slice only; the rest is copied after ev_t5 (finish_left_solve),
        // before the (b) trailing pieces that read it
        HIPCHK(hipStreamWaitEvent(c.stream, c.ev_t5a, 0));
        const int64_t s0 = st.lnext - st.loff;
        if (!st.direct)
            launch_copy2d(r.A01 + s0, wA01, r.A01Rcv + s0, Nl, c.nlayr, c.v,
                          c.stream);
    } else if (!st.direct)
        launch_copy2d(r.A01 + st.dead, wA01, r.A01Rcv + st.dead, Nl, c.nlayr,
                      wA01 - st.dead, c.stream);
    return 0;
}

// slice-first: the rest of the A01 solve feeds the (b) pieces
int finish_left_solve(Ctx &c, const Step &st, const StepPlan &sp) {
    if (!st.slice_first) return 0;
    RankState &r = c.rs[0];
    if (st.sliced) {
        HIPCHK(hipStreamWaitEvent(c.trsm_stream, c.ev_pc, 0));
        StreamGuard on_solve_stream(c, c.trsm_stream);
        if (int rc = solve_rest(c, st, sp, r)) return rc;
        HIPCHK(hipEventRecord(c.ev_t5, c.stream));
    }
    HIPCHK(hipStreamWaitEvent(c.stream, c.ev_t5, 0));
    const int64_t s0 = st.lnext - st.loff, wA01 = st.wA01;
    if (!st.direct && s0 > st.dead)
        launch_copy2d(r.A01 + st.dead, wA01, r.A01Rcv + st.dead, c.Nl, c.nlayr,
                      s0 - st.dead, c.stream);
    if (!st.direct && wA01 - s0 - c.v > 0)
        launch_copy2d(r.A01 + s0 + c.v, wA01, r.A01Rcv + s0 + c.v, c.Nl,
                      c.nlayr, wA01 - s0 - c.v, c.stream);
    return 0;
}

// one piece of the trailing update: columns [col0, col0 + ncols) of the
// active rows, on a grid of at most `cap` workgroups (0 = uncapped)
int gemm_piece(Ctx &c, const Step &st, RankState &r, int64_t col0,
               int64_t ncols, int cap) {
    if (r.nact <= 0 || ncols <= 0) return 0;
    const double fl = 2.0 * r.nact * (double)ncols * c.nlayr;
    size_t slot;
    if (ev_begin(c, 0, fl, &slot)) return CONFLUX_LU_EHIP;
    launch_dgemm_f64(r.A10Rcv, c.nlayr, r.A01Rcv + (col0 - st.loff), c.Nl,
                     r.A11 + i64(r.fnp) * c.Nl + col0, c.Nl, r.nact, ncols,
                     c.nlayr, c.stream, cap);
    return ev_end(c, slot) ? CONFLUX_LU_EHIP : 0;
}

// The look-ahead decision of a step, made here and nowhere else (after the
// push: it reads nact).  async = step k+1's panel chain runs on the panel
// stream concurrently with the (b) pieces; gcap = the grid cap of those
// pieces (0 = uncapped).
//
// While the panel of step k+1 runs concurrently, the trailing update's grid
// is capped so whole CUs stay free for it: an uncapped GEMM flood starves
// the panel until the queue drains (measured 256 ms vs 251 ms sequential at
// N=16384 before this cap).  Panel blocks need 67 KB LDS (256x256 shape, 2
// blocks/CU); the default cap leaves 40 of 256 CUs free = up to 80
// co-resident panel blocks.
//
// INVARIANT: st.slice_first is decided before the push from the same knob
// and stays on when the residency guard below turns async off.  That is
// legal: ev_pc is recorded whenever a panel stream exists, so the sliced
// rest and the slice's waits have their events either way; the step merely
// pays the slice's 7 ms without a concurrent panel to gain from it.
struct LookAhead {
    bool async = false;
    int gcap = 0;
};
LookAhead plan_lookahead(const Ctx &c, const Step &st) {
    LookAhead la;
    if (!(st.look && !c.sim && c.panel_stream && c.knobs.lookahead)) return la;
    la.async = true;
    // Only ranks that RUN step k+1's panel factor need the cap (and the
    // residency guard): pj == ncol AND pk == 0 (the factor runs on layer 0
    // only — conflux_opt.hpp:689).  Other ranks overlap only the panel
    // chain's comm and keep the full-width GEMM (r02 fix: pk > 0 ranks on
    // 1x1xPz grids were capping for a factor they never run).
    int panel_rows = 0;
    for (const auto &r : c.rs)
        if (r.pj == st.ncol && r.pk == 0)
            panel_rows = std::max(panel_rows, r.nact);
    if (panel_rows <= 0) return la;
    la.gcap = c.knobs.gemm_cap;
    // Residency guard: the persistent capped GEMM holds its CUs for the
    // whole update, so if step k+1's panel needs more co-resident blocks
    // than the cap leaves free (tall panels at N >= 32768), the overlap
    // would serialize anyway — keep the sequential order and the full-width
    // GEMM instead.
    const int nblocks =
        (panel_rows + conflux_panel_rpb() - 1) / conflux_panel_rpb();
    const int bpc = conflux_panel_blocks_per_cu();
    const int free_cus = 256 - (la.gcap + 1) / 2;
    if ((nblocks + bpc - 1) / bpc > free_cus) la = LookAhead{};
    return la;
}

// step 6: trailing update (the flop carrier), split for the look-ahead: (a)
// the columns of step k+1's panel FIRST, (b) the rest, (c) phase01(k+1) on
// the panel stream CONCURRENTLY with (b).  Numerically identical: the column
// split does not reorder any K-sum.  On exit sp holds step k+1's plan.
int trailing_update(Ctx &c, const Step &st, StepPlan &sp) {
    const int v = c.v, k = st.k;
    const int64_t Nl = c.Nl;
    const LookAhead la = plan_lookahead(c, st);
    for (auto &r : c.rs) {
        nanscan(c, "A10Rcv", k, r.A10Rcv, i64(r.nact) * c.nlayr);
        nanscan(c, "A01Rcv", k, r.A01Rcv,
                i64(c.nlayr - 1) * Nl + (Nl - st.loff));
    }
    // (a) the columns step k+1's panel needs, first
    if (st.look)
        for (auto &r : c.rs)
            if (r.pj == st.ncol)
                if (gemm_piece(c, st, r, st.lnext, v, 0))
                    return CONFLUX_LU_EHIP;
    if (st.look)
        for (auto &r : c.rs)
            if (r.pj == st.ncol)
                nanscan(c, "A11.a-cols", k,
                        r.A11 + i64(r.fnp) * Nl + st.lnext, i64(r.nact) * Nl);
    if (st.look && !c.sim && c.panel_stream) {
        HIPCHK(hipEventRecord(c.ev_pc, c.stream));
        if (c.knobs.gap_stats) {
            g_gap.to_evpc += gap_ms(g_gap.t0, GapClock::now());
            ++g_gap.evpc_steps;
        }
    }
    if (int rc = finish_left_solve(c, st, sp)) return rc;
    // (b) the rest of the trailing update — capped while the panel runs.
    // It must be ENQUEUED before phase01: phase01 ends in a host sync (the
    // pivot D2H), so anything enqueued after it cannot overlap the panel.
    for (auto &r : c.rs) {
        if (st.look && r.pj == st.ncol) {
            // (dead: with Py = 1 this first piece is the column block of
            // the panel just factored, which no later step reads)
            if (gemm_piece(c, st, r, st.loff + st.dead,
                           st.lnext - st.loff - st.dead, la.gcap))
                return CONFLUX_LU_EHIP;
            if (gemm_piece(c, st, r, st.lnext + v, Nl - (st.lnext + v),
                           la.gcap))
                return CONFLUX_LU_EHIP;
        } else {
            if (gemm_piece(c, st, r, st.loff + st.dead, st.wA01 - st.dead,
                           la.gcap))
                return CONFLUX_LU_EHIP;
        }
    }
    // (c) lookahead: step k+1's panel chain on the panel stream, gated on
    // ev_pc (= its columns updated), running concurrently with (b) on the
    // CUs the cap left free
    if (!st.look) return 0;
    if (la.async) HIPCHK(hipStreamWaitEvent(c.panel_stream, c.ev_pc, 0));
    StreamGuard on_panel_stream(c, la.async ? c.panel_stream : c.stream);
    StepPlan nsp;
    if (int rc = phase01(c, k + 1, nsp)) return rc;
    sp = std::move(nsp);
    return 0;
}

// Steps 2..6 of superstep k; sp holds this step's pivot
// plan (from phase01) and, on exit, step k+1's.
int run_step(Ctx &c, int k, StepPlan &sp) {
    const Step st = make_step(c, k);
    if (c.knobs.gap_stats) g_gap.t0 = GapClock::now();
    if (int rc = push_pivot_rows(c, st, sp)) return rc;       // 2, C7
    if (int rc = route_pivot_rows(c, st, sp)) return rc;      // 3, C5/C6
    if (int rc = ship_history(c, st, sp)) return rc;          // C10
    if (c.knobs.gap_stats) {
        g_gap.to_trsm += gap_ms(g_gap.t0, GapClock::now());
        ++g_gap.steps;
    }
    if (int rc = start_left_solve(c, st, sp)) return rc;      // 5, split
    for (auto &r : c.rs)
        nanscan(c, "A11.postpush", k, r.A11, i64(c.Ml) * c.Nl);
    if (int rc = right_solve_and_spread(c, st)) return rc;    // 4, C8
    if (int rc = left_solve_and_spread(c, st)) return rc;     // 5, C9
    return trailing_update(c, st, sp);                        // 6, 0/1 of k+1
}

// ===========================================================================
// Cholesky (CONFCHOX path — SURVEY §8f1, reference src/conflux/cholesky/):
// the same tile-cyclic (Px,Py,Pz) machinery minus pivoting.  Per tile-column
// k (Cholesky.cpp flow: choleskyA00 :192, updateA10 :280, computeA11
// :345-351, reduce :581-620):
//   c0  depth-reduce the k-th tile column to layer 0
//   c1  potrf the diagonal tile on its owner; broadcast L_kk down the column
//   c2  L_ik = A_ik * L_kk^-T on the column ranks (strictly below diagonal)
//   c2b slab-spread the L panel over (pj, pk)            [= LU C8]
//   c3  transpose-spread: every rank receives L_jk slabs for its local
//       column tiles j (the reference's A01rcv representatives)
//   c4  A_ij -= L_ik * L_jk^T for local tiles with i >= j > k (NT GEMM)
// No pivoting -> row activation is static: rows of tiles < t owned by pi.
// ===========================================================================
inline int ntiles_lt(const Ctx &c, int pi, int t) {
    return (t <= pi) ? 0 : (t - pi + c.Px - 1) / c.Px;
}

// depth-reduce items of the k-th tile column under static row activation
// (Cholesky c0, no-pivot n0): rank row pi reduces its rows of tiles >= k
std::vector<ReduceItem> static_col_items(const Ctx &c, int k) {
    std::vector<ReduceItem> items;
    for (int pi = 0; pi < c.Px; ++pi) {
        const int v = c.v, f = v * ntiles_lt(c, pi, k);
        items.push_back({pi, k % c.Py, i64(c.Ml - f) * v,
                         [f, v](RankState &x) { return x.A10 + i64(f) * v; }});
    }
    return items;
}

int potrf_tile(Ctx &c, double *T, int64_t ld) {
    const int v = c.v, NB = conflux_panel_nb();
    size_t slot;
    if (ev_begin(c, 1, 0, &slot)) return CONFLUX_LU_EHIP;
    for (int jb = 0; jb < v; jb += NB) {
        const int nb = std::min(NB, v - jb);
        launch_potrf32(T + i64(jb) * ld + jb, ld, nb, c.stream);
        if (jb + nb < v) {
            launch_trsm_right_upper32(T + i64(jb) * ld + jb, ld,
                                      T + i64(jb + nb) * ld + jb, ld, nb,
                                      v - jb - nb, /*trans=*/1, c.stream);
            launch_dgemm_f64_nt(T + i64(jb + nb) * ld + jb, ld,
                                T + i64(jb + nb) * ld + jb, ld,
                                T + i64(jb + nb) * ld + jb + nb, ld,
                                v - jb - nb, v - jb - nb, nb, c.stream);
        }
    }
    return ev_end(c, slot);
}

int trsm_right_lowT(Ctx &c, RankState &r, double *X, int64_t ldx, int M) {
    const int v = c.v, NB = conflux_panel_nb();
    size_t slot;
    if (ev_begin(c, 2, 0, &slot)) return CONFLUX_LU_EHIP;
    if (v % 32 == 0) {  // fused single-launch MFMA solve (X * L^-T)
        if (fused_trsm_right(r, X, ldx, v, M, 1, c.stream))
            return CONFLUX_LU_EHIP;
        return ev_end(c, slot);
    }
    for (int jb = 0; jb < v; jb += NB) {
        const int nb = std::min(NB, v - jb);
        launch_trsm_right_upper32(r.A00 + i64(jb) * v + jb, v, X + jb, ldx, nb,
                                  M, /*trans=*/1, c.stream);
        if (jb + nb < v)
            launch_dgemm_f64_nt(X + jb, ldx, r.A00 + i64(jb + nb) * v + jb, v,
                                X + jb + nb, ldx, M, v - jb - nb, nb,
                                c.stream);
    }
    return ev_end(c, slot);
}

int chol_step(Ctx &c, int k) {
    const int v = c.v, Px = c.Px, Py = c.Py, Pz = c.Pz, Nt = c.Nt;
    const int64_t Nl = c.Nl;
    const int kcol = k % Py, krow = k % Px;
    const int loff = (k / Py) * v;
    auto fnp_of = [&](int pi) { return v * ntiles_lt(c, pi, k); };
    auto f2_of = [&](int pi) { return fnp_of(pi) + (pi == krow ? v : 0); };

    // ---- c0: copy the k-th tile column into A10, depth-reduce -------------
    for (auto &r : c.rs) {
        if (r.pj != kcol) continue;
        const int f = fnp_of(r.pi);
        launch_copy2d(r.A11 + i64(f) * Nl + loff, Nl, r.A10 + i64(f) * v, v,
                      c.Ml - f, v, c.stream);
    }
    if (depth_reduce(c, c.comm, static_col_items(c, k))) return CONFLUX_LU_ECOMM;

    // ---- c1: potrf diagonal tile; broadcast L_kk down the column ----------
    {
        RankState *own = get_rs(c, krow, kcol, 0);
        if (own) {
            const int fd = fnp_of(krow);
            if (potrf_tile(c, own->A10 + i64(fd) * v, v))
                return CONFLUX_LU_EINTERNAL;
            launch_copy2d(own->A10 + i64(fd) * v, v, own->A00, v, v, v,
                          c.stream);
        }
        std::vector<int> dests;  // layer 0 of process column kcol
        for (int pi = 0; pi < Px; ++pi)
            if (pi != krow) dests.push_back(grank_of(c, pi, kcol, 0));
        if (int rc = bcast_tile(c, [](RankState &x) { return x.A00; },
                                i64(v) * v, grank_of(c, krow, kcol, 0), dests))
            return rc;
    }

    // ---- c2: column TRSM (strictly below the diagonal); store L -----------
    for (auto &r : c.rs) {
        if (r.pj != kcol || r.pk != 0) continue;
        const int f2 = f2_of(r.pi);
        const int n2 = c.Ml - f2;
        if (n2 > 0 &&
            trsm_right_lowT(c, r, r.A10 + i64(f2) * v, v, n2))
            return CONFLUX_LU_EINTERNAL;
        if (c.store_factors) {
            if (n2 > 0)
                launch_copy2d(r.A10 + i64(f2) * v, v,
                              r.Fres + i64(f2) * Nl + loff, Nl, n2, v,
                              c.stream);
            if (r.pi == krow)  // diagonal tile: L_kk (upper half junk;
                               // consumers read tril only)
                launch_copy2d(r.A00, v, r.Fres + i64(fnp_of(krow)) * Nl + loff,
                              Nl, v, v, c.stream);
        }
    }

    // ---- c2b: slab-spread the L panel over (pj, pk)  [= LU C8] ------------
    if (int rc = spread_col_slabs(
            c, kcol, [&](const RankState &r) { return f2_of(r.pi); }))
        return rc;

    // ---- c3: transpose-spread L_jk slabs to the columns that need them ----
    // destination layout: A01Rcv as [local col tile][v][nlayr]
    for (int j = k + 1; j < Nt; ++j) {
        const int rpi = j % Px, dpj = j % Py;
        const int f2r = f2_of(rpi);
        const int rowoff = ntiles_lt(c, rpi, j) * v - f2r;  // rows into slab
        const int ltj = j / Py;
        RankState *root = get_rs(c, rpi, kcol, 0);
        if (c.sim) {
            for (int pi = 0; pi < Px; ++pi)
                for (int pk = 0; pk < Pz; ++pk) {
                    RankState &d = *get_rs(c, pi, dpj, pk);
                    const int n2 = c.Ml - f2r;
                    const double *srcslab = (Py == 1 && Pz == 1)
                        ? root->A10Rcv + i64(rowoff) * c.nlayr
                        : root->slabs + (i64(pk) * n2 + rowoff) * c.nlayr;
                    if (d2d(c, d.A01Rcv + i64(ltj) * v * c.nlayr, srcslab,
                            i64(v) * c.nlayr))
                        return CONFLUX_LU_EHIP;
                }
        } else {
            RankState &me = c.rs[0];
            const bool is_root = root && root->grank == me.grank;
            const bool is_dst = (me.pj == dpj);
            const int n2 = c.Ml - f2r;
            if (is_root) {
                const double *base = (Py == 1 && Pz == 1) ? me.A10Rcv : me.slabs;
                for (int pi = 0; pi < Px; ++pi)
                    for (int pk = 0; pk < Pz; ++pk) {
                        const double *srcslab = (Py == 1 && Pz == 1)
                            ? base + i64(rowoff) * c.nlayr
                            : base + (i64(pk) * n2 + rowoff) * c.nlayr;
                        if (pi == me.pi && dpj == me.pj && pk == me.pk) {
                            if (d2d(c, me.A01Rcv + i64(ltj) * v * c.nlayr,
                                    srcslab, i64(v) * c.nlayr))
                                return CONFLUX_LU_EHIP;
                        } else {
                            NCCLCHK(ncclGroupStart());
                            NCCLCHK(ncclSend(srcslab, i64(v) * c.nlayr,
                                             ncclDouble,
                                             grank_of(c, pi, dpj, pk), c.comm,
                                             c.stream));
                            NCCLCHK(ncclGroupEnd());
                        }
                    }
            } else if (is_dst) {
                NCCLCHK(ncclGroupStart());
                NCCLCHK(ncclRecv(me.A01Rcv + i64(ltj) * v * c.nlayr,
                                 i64(v) * c.nlayr, ncclDouble,
                                 grank_of(c, rpi, kcol, 0), c.comm, c.stream));
                NCCLCHK(ncclGroupEnd());
            }
        }
    }

    // ---- c4: low-rank updates of local tiles with i >= j > k --------------
    // One rectangular launch per rank with the tile-diagonal mask (v % 128
    // == 0): workgroups above the global tile diagonal exit immediately, so
    // the whole trapezoid updates at full-chip GEMM efficiency instead of
    // one narrow launch per column tile (~970 launches/factorization at
    // N=16384 averaging 22 TF; profiles/r02_kernel_stats_chol_n16384.csv).
    // A01Rcv's per-tile v x nlayr slabs are globally contiguous, so it IS
    // the (Nl x nlayr) B^T operand.  Tiles with global row tile < col tile
    // are never read anywhere (only the lower triangle is meaningful), so
    // masked-out regions are simply untouched.
    static const int rect_env = env_int("CONFLUX_CHOL_RECT", 1);
    for (auto &r : c.rs) {
        const int f2 = f2_of(r.pi);
        const int ltj0 = (r.pj <= k) ? (k - r.pj) / Py + 1 : 0;
        const int r0 = v * ntiles_lt(c, r.pi, k + 1);
        double fl = 0;  // algorithmic flops (valid tiles only)
        for (int ltj = ltj0; ltj < c.tA11y; ++ltj) {
            const int gtj = ltj * Py + r.pj;
            if (gtj >= Nt) continue;
            const int M2 = c.Ml - v * ntiles_lt(c, r.pi, gtj);
            if (M2 > 0) fl += 2.0 * M2 * (double)v * c.nlayr;
        }
        // adaptive: per-tile launches already fill the chip when a tile
        // column's grid has >= ~512 workgroups (measured: per-tile wins at
        // Ml-r0 = 32768, rect wins at <= 16384); batch with the masked
        // rectangle only when they would underfill
        const bool use_rect =
            rect_env && v % 128 == 0 && i64(c.Ml - r0) * 4 / 128 <= 512;
        if (use_rect) {
            const int M2r = c.Ml - r0;
            const int64_t N2 = Nl - i64(ltj0) * v;
            if (M2r <= 0 || N2 <= 0 || ltj0 >= c.tA11y) continue;
            size_t slot;
            if (ev_begin(c, 0, fl, &slot)) return CONFLUX_LU_EHIP;
            launch_dgemm_f64_nt_tril(
                r.A10Rcv + i64(r0 - f2) * c.nlayr, c.nlayr,
                r.A01Rcv + i64(ltj0) * v * c.nlayr, c.nlayr,
                r.A11 + i64(r0) * Nl + i64(ltj0) * v, Nl, M2r, N2, c.nlayr,
                v, r0, i64(ltj0) * v, Px, Py, r.pi, r.pj, c.stream);
            if (ev_end(c, slot)) return CONFLUX_LU_EHIP;
            continue;
        }
        for (int ltj = ltj0; ltj < c.tA11y; ++ltj) {
            const int gtj = ltj * Py + r.pj;
            if (gtj <= k || gtj >= Nt) continue;
            const int rstart = v * ntiles_lt(c, r.pi, gtj);
            const int M2 = c.Ml - rstart;
            if (M2 <= 0) continue;
            const double fl1 = 2.0 * M2 * (double)v * c.nlayr;
            size_t slot;
            if (ev_begin(c, 0, fl1, &slot)) return CONFLUX_LU_EHIP;
            launch_dgemm_f64_nt(r.A10Rcv + i64(rstart - f2) * c.nlayr, c.nlayr,
                                r.A01Rcv + i64(ltj) * v * c.nlayr, c.nlayr,
                                r.A11 + i64(rstart) * Nl + i64(ltj) * v, Nl,
                                M2, v, c.nlayr, c.stream);
            if (ev_end(c, slot)) return CONFLUX_LU_EHIP;
        }
    }
    return 0;
}

// ---------------------------------------------------------------------------
// single-rank (1x1x1, world == 1) Cholesky lookahead: while step k's
// trailing update (b) runs on the main stream, step k+1's whole serial
// chain — c0 column copy, blocked potrf, the rank-v TRSM, the slab copies —
// runs on the second stream into the OTHER receive-slab set.  Bit-identical
// to the sequential order: the (a)/(b) column split partitions the same
// per-tile updates, and the chain is gated on exactly the columns it reads.
// ---------------------------------------------------------------------------
int chol_chain_1r(Ctx &c, int k, double *rcvA, double *rcvB) {
    const int v = c.v;
    const int64_t Nl = c.Nl;
    RankState &r = c.rs[0];
    const int fnp = k * v, f2 = fnp + v;
    launch_copy2d(r.A11 + i64(fnp) * Nl + i64(k) * v, Nl,
                  r.A10 + i64(fnp) * v, v, c.Ml - fnp, v, c.stream);
    if (potrf_tile(c, r.A10 + i64(fnp) * v, v)) return CONFLUX_LU_EINTERNAL;
    launch_copy2d(r.A10 + i64(fnp) * v, v, r.A00, v, v, v, c.stream);
    const int n2 = c.Ml - f2;
    if (n2 > 0 && trsm_right_lowT(c, r, r.A10 + i64(f2) * v, v, n2))
        return CONFLUX_LU_EINTERNAL;
    if (c.store_factors) {
        if (n2 > 0)
            launch_copy2d(r.A10 + i64(f2) * v, v,
                          r.Fres + i64(f2) * Nl + i64(k) * v, Nl, n2, v,
                          c.stream);
        launch_copy2d(r.A00, v, r.Fres + i64(fnp) * Nl + i64(k) * v, Nl, v,
                      v, c.stream);
    }
    if (n2 > 0) {
        launch_copy2d(r.A10 + i64(f2) * v, v, rcvA, c.nlayr, n2, v, c.stream);
        // A01Rcv tiles k+1..Nt are rcvA shifted one tile (1x1x1: nlayr == v)
        launch_copy2d(rcvA, c.nlayr, rcvB + i64(k + 1) * v * c.nlayr,
                      c.nlayr, n2, c.nlayr, c.stream);
    }
    return 0;
}

int chol_c4_1r(Ctx &c, int k, double *rcvA, double *rcvB, bool slice_only,
               bool rest_only) {
    const int v = c.v;
    const int64_t Nl = c.Nl;
    const int Nt = c.Nt;
    RankState &r = c.rs[0];
    const int f2 = (k + 1) * v;
    if (!rest_only && k + 1 < Nt) {  // (a): tile column k+1 only
        const int M2 = c.Ml - f2;
        if (M2 > 0) {
            const double fl = 2.0 * M2 * (double)v * c.nlayr;
            size_t slot;
            if (ev_begin(c, 0, fl, &slot)) return CONFLUX_LU_EHIP;
            launch_dgemm_f64_nt(rcvA, c.nlayr,
                                rcvB + i64(k + 1) * v * c.nlayr, c.nlayr,
                                r.A11 + i64(f2) * Nl + f2, Nl, M2, v,
                                c.nlayr, c.stream);
            if (ev_end(c, slot)) return CONFLUX_LU_EHIP;
        }
    }
    if (slice_only || k + 2 >= Nt) return 0;
    // (b): tile columns k+2..Nt (adaptive rect as in chol_step)
    const int r0 = (k + 2) * v;
    const int64_t c0 = i64(k + 2) * v;
    const int M2r = c.Ml - r0;
    const int64_t N2 = Nl - c0;
    if (M2r <= 0 || N2 <= 0) return 0;
    double fl = 0;
    for (int j = k + 2; j < Nt; ++j) fl += 2.0 * (c.Ml - i64(j) * v) * v * c.nlayr;
    const bool use_rect = v % 128 == 0 && i64(M2r) * 4 / 128 <= 512;
    static const int dbg = env_int("CONFLUX_CHOL_DEBUG", 0);
    if (dbg)
        std::fprintf(stderr, "[c4_1r] k=%d M2r=%d rect=%d\n", k, M2r,
                     (int)use_rect);
    size_t slot;
    if (ev_begin(c, 0, fl, &slot)) return CONFLUX_LU_EHIP;
    if (use_rect) {
        launch_dgemm_f64_nt_tril(rcvA + i64(r0 - f2) * c.nlayr, c.nlayr,
                                 rcvB + c0 * c.nlayr, c.nlayr,
                                 r.A11 + i64(r0) * Nl + c0, Nl, M2r, N2,
                                 c.nlayr, v, r0, c0, 1, 1, 0, 0, c.stream);
    } else {
        for (int j = k + 2; j < Nt; ++j) {
            const int rs = j * v, M2 = c.Ml - rs;
            if (M2 <= 0) continue;
            launch_dgemm_f64_nt(rcvA + i64(rs - f2) * c.nlayr, c.nlayr,
                                rcvB + i64(j) * v * c.nlayr, c.nlayr,
                                r.A11 + i64(rs) * Nl + i64(j) * v, Nl, M2, v,
                                c.nlayr, c.stream);
        }
    }
    if (ev_end(c, slot)) return CONFLUX_LU_EHIP;
    return 0;
}

// every step of one Cholesky factorization (the timed body of chol_loop)
int chol_steps(Ctx &c) {
    static const int chol_look = env_int("CONFLUX_CHOL_LOOK", 1);
    if (chol_look && !c.sim && c.world == 1 && c.Px == 1 && c.Py == 1 &&
        c.Pz == 1 && c.panel_stream) {
        RankState &r = c.rs[0];
        if (!r.A10Rcv2) {
            HIPCHK(hipMalloc(&r.A10Rcv2, i64(c.Ml) * c.nlayr * 8));
            HIPCHK(hipMalloc(&r.A01Rcv2, i64(c.nlayr) * c.Nl * 8));
        }
        double *As2[2] = {r.A10Rcv, r.A10Rcv2};
        double *Bs2[2] = {r.A01Rcv, r.A01Rcv2};
        int rc = chol_chain_1r(c, 0, As2[0], Bs2[0]);
        if (rc) return rc;
        for (int k = 0; k + 1 < c.Nt; ++k) {
            const int par = k & 1;
            if ((rc = chol_c4_1r(c, k, As2[par], Bs2[par], true, false)))
                return rc;
            HIPCHK(hipEventRecord(c.ev_pc, c.stream));
            HIPCHK(hipStreamWaitEvent(c.panel_stream, c.ev_pc, 0));
            {
                StreamGuard on_panel_stream(c, c.panel_stream);
                if ((rc = chol_chain_1r(c, k + 1, As2[par ^ 1], Bs2[par ^ 1])))
                    return rc;
                HIPCHK(hipEventRecord(c.ev_t5, c.stream));
            }
            if ((rc = chol_c4_1r(c, k, As2[par], Bs2[par], false, true)))
                return rc;
            HIPCHK(hipStreamWaitEvent(c.stream, c.ev_t5, 0));
        }
    } else {
        for (int k = 0; k < c.Nt; ++k) {
            int rc = chol_step(c, k);
            if (rc) return rc;
        }
    }
    return 0;
}

int chol_loop(Ctx &c, double *elapsed_ms) {
    for (auto &r : c.rs) {
        if (c.store_factors) {
            if (ensure_factor_bufs(c, r, /*need_hist=*/false))
                return CONFLUX_LU_EHIP;
            launch_zero2d(r.Fres, c.Nl, c.Ml, c.Nl, c.stream);
        }
    }
    // perm is identity for the pivotless path (API consistency)
    c.pivotInds.resize(c.M);
    std::iota(c.pivotInds.begin(), c.pivotInds.end(), 0);
    c.evs_used = 0;
    for (auto &t : c.cats) t = TimeCat{};
    return timed_region(c, elapsed_ms, [&] { return chol_steps(c); });
}

}  // namespace

// ===========================================================================
// No-pivot LU (SURVEY §8f4 — the Python prototype's EmptyPivot strategy,
// python/conflux.py; the C++ reference implements tournament only, so this
// is parity-pinned against a numpy restatement instead): for diagonally
// dominant inputs the whole tournament/row-movement machinery drops out and
// row activation is static like Cholesky.  Per tile column k:
//   n0  depth-reduce the k-th tile column (rows of tiles >= k) to layer 0
//   n1  blocked in-place LU of the diagonal v x v tile (no pivoting);
//       broadcast the packed LU (A00) to every rank
//   n2  A10[below diag] <- A10 * U(A00)^-1 on the column ranks; C8 spread
//   n3  A01[diag-tile rows, cols > k] depth-reduced, <- L(A00)^-1 * A01 on
//       the row ranks; C9 spread
//   n4  one rectangular trailing GEMM per rank (no masking: LU updates the
//       full trailing block)
// perm stays identity, Fres mirrors the pivoted layout, so
// conflux_lu_validate works unchanged.
// ===========================================================================
namespace {

int nopiv_step(Ctx &c, int k) {
    const int v = c.v, Px = c.Px, Py = c.Py;
    const int64_t Nl = c.Nl;
    const int kcol = k % Py, krow = k % Px;
    const int64_t loff = i64(k / Py) * v;
    auto fnp_of = [&](int pi) { return v * ntiles_lt(c, pi, k); };
    auto f2_of = [&](int pi) { return fnp_of(pi) + (pi == krow ? v : 0); };
    auto ltj0_of = [&](int pj) { return (pj <= k) ? (k - pj) / Py + 1 : 0; };

    // ---- n0: copy the k-th tile column into A10, depth-reduce ------------
    for (auto &r : c.rs) {
        if (r.pj != kcol) continue;
        const int f = fnp_of(r.pi);
        launch_copy2d(r.A11 + i64(f) * Nl + loff, Nl, r.A10 + i64(f) * v, v,
                      c.Ml - f, v, c.stream);
    }
    if (depth_reduce(c, c.comm, static_col_items(c, k))) return CONFLUX_LU_ECOMM;

    // ---- n1: blocked no-pivot LU of the diagonal tile; broadcast A00 -----
    {
        RankState *own = get_rs(c, krow, kcol, 0);
        if (own) {
            double *T = own->A10 + i64(fnp_of(krow)) * v;
            size_t slot;
            if (ev_begin(c, 1, 0, &slot)) return CONFLUX_LU_EHIP;
            const int NB = conflux_panel_nb();
            for (int jb = 0; jb < v; jb += NB) {
                const int nb = std::min(NB, v - jb);
                launch_getrf32_nopiv(T + i64(jb) * v + jb, v, nb, c.stream);
                if (jb + nb < v) {
                    launch_trsm_right_upper32(T + i64(jb) * v + jb, v,
                                              T + i64(jb + nb) * v + jb, v,
                                              nb, v - jb - nb, 0, c.stream);
                    launch_trsm_left_lower_unit32(T + i64(jb) * v + jb, v,
                                                  T + i64(jb) * v + jb + nb,
                                                  v, nb, v - jb - nb,
                                                  c.stream);
                    launch_dgemm_f64(T + i64(jb + nb) * v + jb, v,
                                     T + i64(jb) * v + jb + nb, v,
                                     T + i64(jb + nb) * v + jb + nb, v,
                                     v - jb - nb, v - jb - nb, nb, c.stream);
                }
            }
            if (ev_end(c, slot)) return CONFLUX_LU_EHIP;
            launch_copy2d(T, v, own->A00, v, v, v, c.stream);
        }
        // broadcast the packed LU to every rank (both halves are consumed)
        const int root = grank_of(c, krow, kcol, 0);
        std::vector<int> dests;
        for (int g = 0; g < c.world; ++g)
            if (g != root) dests.push_back(g);
        if (int rc = bcast_tile(c, [](RankState &x) { return x.A00; },
                                i64(v) * v, root, dests))
            return rc;
    }

    // ---- n2: A10 <- A10 U^-1 below the diagonal; store L; C8 spread ------
    for (auto &r : c.rs) {
        if (r.pj != kcol || r.pk != 0) continue;
        const int f2 = f2_of(r.pi);
        const int n2 = c.Ml - f2;
        if (n2 > 0 && trsm_right_upper(c, r, r.A10 + i64(f2) * v, v, n2))
            return CONFLUX_LU_EINTERNAL;
        if (c.store_factors) {
            if (n2 > 0)
                launch_copy2d(r.A10 + i64(f2) * v, v,
                              r.Fres + i64(f2) * Nl + loff, Nl, n2, v,
                              c.stream);
            if (r.pi == krow)  // diagonal tile: packed LU
                launch_copy2d(r.A00, v, r.Fres + i64(fnp_of(krow)) * Nl + loff,
                              Nl, v, v, c.stream);
        }
    }
    if (int rc = spread_col_slabs(
            c, kcol, [&](const RankState &r) { return f2_of(r.pi); }))
        return rc;

    // ---- n3: A01 row panel (diag-tile rows, cols > k): reduce, solve,
    // store U, C9 spread ----------------------------------------------------
    for (auto &r : c.rs) {
        if (r.pi != krow) continue;
        const int64_t c0 = i64(ltj0_of(r.pj)) * v;
        const int64_t w = Nl - c0;
        if (w <= 0) continue;
        launch_copy2d(r.A11 + i64(fnp_of(krow)) * Nl + c0, Nl, r.A01, w, v, w,
                      c.stream);
    }
    {
        std::vector<ReduceItem> items;
        for (int pj = 0; pj < Py; ++pj)
            items.push_back({krow, pj, v * (Nl - i64(ltj0_of(pj)) * v),
                             [](RankState &x) { return x.A01; }});
        if (depth_reduce(c, c.comm, items)) return CONFLUX_LU_ECOMM;
    }
    for (auto &r : c.rs) {
        if (r.pi != krow || r.pk != 0) continue;
        const int64_t c0 = i64(ltj0_of(r.pj)) * v;
        const int64_t w = Nl - c0;
        if (w <= 0) continue;
        if (trsm_left_lower(c, r, r.A01, w, w)) return CONFLUX_LU_EINTERNAL;
        if (c.store_factors)
            launch_copy2d(r.A01, w, r.Fres + i64(fnp_of(krow)) * Nl + c0, Nl,
                          v, w, c.stream);
    }
    // C9: spread the solved row panel down each column (into A01Rcv at the
    // SAME local column offset, ld Nl)
    if (int rc = spread_row_panel(
            c, krow, [&](int pj) { return Nl - i64(ltj0_of(pj)) * v; },
            [&](int pj) { return i64(ltj0_of(pj)) * v; }))
        return rc;

    // ---- n4: one rectangular trailing update per rank ---------------------
    for (auto &r : c.rs) {
        const int rstart = f2_of(r.pi);
        const int64_t c0 = i64(ltj0_of(r.pj)) * v;
        const int M2 = c.Ml - rstart;
        const int64_t N2 = Nl - c0;
        if (M2 <= 0 || N2 <= 0) continue;
        const double fl = 2.0 * M2 * (double)N2 * c.nlayr;
        size_t slot;
        if (ev_begin(c, 0, fl, &slot)) return CONFLUX_LU_EHIP;
        launch_dgemm_f64(r.A10Rcv, c.nlayr, r.A01Rcv + c0, Nl,
                         r.A11 + i64(rstart) * Nl + c0, Nl, M2, N2, c.nlayr,
                         c.stream);
        if (ev_end(c, slot)) return CONFLUX_LU_EHIP;
    }
    return 0;
}

int nopiv_loop(Ctx &c, double *elapsed_ms) {
    for (auto &r : c.rs) {
        if (c.store_factors) {
            if (ensure_factor_bufs(c, r, /*need_hist=*/false))
                return CONFLUX_LU_EHIP;
            launch_zero2d(r.Fres, c.Nl, c.Ml, c.Nl, c.stream);
        }
    }
    c.pivotInds.resize(c.M);
    std::iota(c.pivotInds.begin(), c.pivotInds.end(), 0);
    c.evs_used = 0;
    for (auto &t : c.cats) t = TimeCat{};
    return timed_region(c, elapsed_ms, [&]() -> int {
        for (int k = 0; k < c.Nt; ++k) {
            int rc = nopiv_step(c, k);
            if (rc) return rc;
        }
        return 0;
    });
}

}  // namespace

// ===========================================================================
// C ABI
// ===========================================================================
struct conflux_lu_ctx : Ctx {};

extern "C" {

const char *conflux_lu_build_info(void) {
    return "conflux_lu MI355X gfx950 fp64 engine (HIP + RCCL)";
}

int conflux_lu_make_uid(char uid[CONFLUX_LU_UID_BYTES]) {
    static_assert(sizeof(ncclUniqueId) == CONFLUX_LU_UID_BYTES, "uid size");
    ncclUniqueId id;
    NCCLCHK(ncclGetUniqueId(&id));
    std::memcpy(uid, &id, sizeof id);
    return CONFLUX_LU_OK;
}

int conflux_lu_create(int N, int v, int Px, int Py, int Pz, int rank,
                      int world, const char *nccl_uid, conflux_lu_ctx **out) {
    if (N <= 0 || v <= 0 || Px <= 0 || Py <= 0 || Pz <= 0) return CONFLUX_LU_EARG;
    if (Px != Py || (Px & (Px - 1)) || v % Pz != 0) return CONFLUX_LU_EARG;
    // round N up to a multiple of v*Px exactly like the reference
    // (lu_params.hpp:67-71); conflux_lu_dims reports the padded size, and
    // the generator fills the padding like the reference's InitMatrix does
    N = v * Px * ((N + v * Px - 1) / (v * Px));
    const int P = Px * Py * Pz;
    const bool sim = (rank < 0);
    if (!sim && world != P) return CONFLUX_LU_EARG;
    if (sim && world != P) return CONFLUX_LU_EARG;

    auto *c = new conflux_lu_ctx();
    c->N = N;
    c->v = v;
    c->Px = Px;
    c->Py = Py;
    c->Pz = Pz;
    c->world = world;
    c->rank = sim ? -1 : rank;
    c->sim = sim;
    c->M = N;
    c->n = c->nf = N;
    c->Nt = N / v;
    c->Mt = N / v;
    c->tA11x = (c->Mt + Px - 1) / Px;
    c->tA11y = (c->Nt + Py - 1) / Py;
    c->Ml = c->tA11x * v;
    c->Nl = c->tA11y * v;
    c->nlayr = v / Pz;
    if (c->Ml < 2 * v) { delete c; return CONFLUX_LU_EARG; }
    if (hipStreamCreate(&c->stream) != hipSuccess) { delete c; return CONFLUX_LU_EHIP; }

    if (sim) {
        c->rs.resize(P);
        for (int pi = 0; pi < Px; ++pi)
            for (int pj = 0; pj < Py; ++pj)
                for (int pk = 0; pk < Pz; ++pk)
                    if (alloc_rank(*c, c->rs[grank_of(*c, pi, pj, pk)], pi, pj,
                                   pk)) {
                        delete c;
                        return CONFLUX_LU_EHIP;
                    }
    } else {
        c->rs.resize(1);
        const int pi = rank / (Py * Pz), pj = (rank / Pz) % Py, pk = rank % Pz;
        if (alloc_rank(*c, c->rs[0], pi, pj, pk)) { delete c; return CONFLUX_LU_EHIP; }
        // panel-stream hardware queue priority: measured a wash at
        // N=16384 (205.3 vs 204.5 ms/step) — env-gated, default off
        const int prio_on = env_int("CONFLUX_PANEL_PRIO", 0);
        int lo = 0, hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
        if ((prio_on
                 ? hipStreamCreateWithPriority(&c->panel_stream,
                                               hipStreamDefault, hi)
                 : hipStreamCreate(&c->panel_stream)) != hipSuccess ||
            hipStreamCreate(&c->trsm_stream) != hipSuccess ||
            hipEventCreate(&c->ev_pc) != hipSuccess ||
            hipEventCreate(&c->ev_t3) != hipSuccess ||
            hipEventCreate(&c->ev_t5) != hipSuccess ||
            hipEventCreate(&c->ev_t5a) != hipSuccess) {
            delete c;
            return CONFLUX_LU_EHIP;
        }
        if (world > 1) {
            if (!nccl_uid) { delete c; return CONFLUX_LU_EARG; }
            ncclUniqueId id;
            std::memcpy(&id, nccl_uid, sizeof id);
            if (ncclCommInitRank(&c->comm, world, id, rank) != ncclSuccess) {
                delete c;
                return CONFLUX_LU_ECOMM;
            }
            c->have_comm = true;
            if (ncclCommSplit(c->comm, 0, rank, &c->pcomm, nullptr) !=
                ncclSuccess) {
                delete c;
                return CONFLUX_LU_ECOMM;
            }
            c->have_pcomm = true;
        }
    }
    *out = c;
    return CONFLUX_LU_OK;
}

int conflux_lu_init_matrix(conflux_lu_ctx *c, uint64_t seed) {
    for (auto &r : c->rs)
        launch_init_matrix(r.A11, c->Ml, c->Nl, c->v, c->Px, c->Py, r.pi, r.pj,
                           r.pk != 0, seed, c->stream);
    HIPCHK(hipGetLastError());  // a rejected launch is otherwise silent
    HIPCHK(hipStreamSynchronize(c->stream));
    c->input_dirty = true;
    c->n = c->N;
    return CONFLUX_LU_OK;
}

/* SPD fill for the Cholesky path: sym(gen) + 2N on the diagonal */
int conflux_lu_init_matrix_spd(conflux_lu_ctx *c, uint64_t seed) {
    for (auto &r : c->rs)
        launch_init_matrix_spd(r.A11, c->Ml, c->Nl, c->v, c->Px, c->Py, r.pi,
                               r.pj, r.pk != 0, seed, c->N, c->stream);
    HIPCHK(hipGetLastError());  // a rejected launch is otherwise silent
    HIPCHK(hipStreamSynchronize(c->stream));
    c->input_dirty = true;
    c->n = c->N;
    return CONFLUX_LU_OK;
}

static int snapshot_or_restore(conflux_lu_ctx *c);

/* Cholesky factorization A = L L^T of the current (SPD) matrix; the
 * CONFCHOX path (reference src/conflux/cholesky/Cholesky.cpp:857
 * parallelCholesky).  Fres then holds L in the tile-cyclic layout (lower
 * triangle valid). */
int conflux_chol_factor(conflux_lu_ctx *c, double *elapsed_ms) {
    if (snapshot_or_restore(c)) return CONFLUX_LU_EHIP;
    c->factored_kind = 0;
    int rc = chol_loop(*c, elapsed_ms);
    if (rc)
        std::fprintf(stderr, "[conflux_lu] chol failed: %s\n",
                     c->err.c_str());
    else if (c->store_factors)
        c->factored_kind = 2;
    return rc;
}

int conflux_lu_set_matrix_local(conflux_lu_ctx *c, const double *local) {
    if (c->sim) return CONFLUX_LU_EARG;  // sim mode uses _set_matrix_sim
    RankState &r = c->rs[0];
    if (!local) {
        launch_zero2d(r.A11, c->Nl, c->Ml, c->Nl, c->stream);
    } else {
        HIPCHK(hipMemcpyAsync(r.A11, local, i64(c->Ml) * c->Nl * 8,
                              hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    c->input_dirty = true;
    c->n = c->N;
    return CONFLUX_LU_OK;
}

/* sim-mode extra (not in the public header; used by tests via ctypes):
 * upload one simulated rank's local buffer */
int conflux_lu_set_matrix_sim(conflux_lu_ctx *c, int grank,
                              const double *local) {
    if (!c->sim || grank < 0 || grank >= (int)c->rs.size())
        return CONFLUX_LU_EARG;
    RankState &r = c->rs[grank];
    if (!local)
        launch_zero2d(r.A11, c->Nl, c->Ml, c->Nl, c->stream);
    else
        HIPCHK(hipMemcpyAsync(r.A11, local, i64(c->Ml) * c->Nl * 8,
                              hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->input_dirty = true;
    c->n = c->N;
    return CONFLUX_LU_OK;
}

int conflux_lu_get_factors_sim(conflux_lu_ctx *c, int grank, double *F_local,
                               int *perm) {
    if (!c->sim || grank < 0 || grank >= (int)c->rs.size())
        return CONFLUX_LU_EARG;
    RankState &r = c->rs[grank];
    if (F_local) {
        if (!r.Fres) return CONFLUX_LU_EARG;
        HIPCHK(hipMemcpyAsync(F_local, r.Fres, i64(c->Ml) * c->Nl * 8,
                              hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    if (perm) std::copy(c->pivotInds.begin(), c->pivotInds.end(), perm);
    return CONFLUX_LU_OK;
}

int conflux_lu_store_factors(conflux_lu_ctx *c, int enable) {
    c->store_factors = enable != 0;
    return CONFLUX_LU_OK;
}

/* Pivoting strategy: 1 = tournament pivoting (the reference
 * algorithm, default); 0 = NO pivoting — the Python prototype's EmptyPivot
 * fast path for diagonally dominant inputs (python/conflux.py; the C++
 * reference implements tournament only).  With mode 0 the permutation is
 * identity and the tournament/row-movement machinery drops out. */
int conflux_lu_set_pivoting(conflux_lu_ctx *c, int mode) {
    if (mode != 0 && mode != 1) return CONFLUX_LU_EARG;
    c->pivoting = mode;
    return CONFLUX_LU_OK;
}

// The reference's LU_rep factors a COPY — lu_params::data survives the call
// (conflux_opt.hpp:398).  Same semantics here: the first factor() after a
// matrix upload snapshots A11; later factor() calls restore the snapshot.
// Both copies run outside the timed region.
static int snapshot_or_restore(conflux_lu_ctx *c) {
    for (auto &r : c->rs)
        if (!r.A11in)
            HIPCHK(hipMalloc(&r.A11in, i64(c->Ml) * c->Nl * 8));
    for (auto &r : c->rs) {
        if (c->input_dirty)
            HIPCHK(hipMemcpyAsync(r.A11in, r.A11, i64(c->Ml) * c->Nl * 8,
                                  hipMemcpyDeviceToDevice, c->stream));
        else
            HIPCHK(hipMemcpyAsync(r.A11, r.A11in, i64(c->Ml) * c->Nl * 8,
                                  hipMemcpyDeviceToDevice, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->input_dirty) c->nf = c->n;
    c->input_dirty = false;
    c->anorm_inf = -1;
    c->anorm_one = -1;
    c->anorm_lead[0] = c->anorm_lead[1] = -1;
    return CONFLUX_LU_OK;
}

int conflux_lu_factor(conflux_lu_ctx *c, double *elapsed_ms) {
    if (snapshot_or_restore(c)) return CONFLUX_LU_EHIP;
    c->factored_kind = 0;
    int rc = c->pivoting ? factor_loop(*c, elapsed_ms)
                         : nopiv_loop(*c, elapsed_ms);
    if (rc) {
        std::fprintf(stderr, "[conflux_lu] factor failed: %s\n",
                     c->err.c_str());
    } else if (c->store_factors) {
        c->factored_kind = 1;
    }
    return rc;
}

/* Validation: ||PA - LU||_F / ||A||_F (or ||A - L L^T||_F /
 * ||A||_F) computed ON DEVICE from the stored factors and the input
 * snapshot — the reference's CONFLUX_WITH_VALIDATION check
 * (conflux_miniapp.cpp:169-507) without ScaLAPACK.
 *
 * Stripe-streamed: global F is materialized once (N^2 doubles) and consumed
 * v rows at a time (the PA / L / residual stripes are v x N), so the
 * bench-scale single-GPU sizes (N = 65536: ~130 GB of engine state) fit
 * beside one 32 GB global buffer in 288 GB HBM.  Streaming order makes the
 * in-place triu legal: stripe i0's GEMM reads U rows k < i0+v only, and all
 * of those were already stripped of their L half.
 *
 * Distributed (world > 1): COLLECTIVE over c->comm — every rank must call.
 * pk == 0 ranks ship their A11in/Fres locals to grank 0, which assembles
 * the globals, computes, and broadcasts the residual to all ranks. */
static int validate_common(conflux_lu_ctx *c, bool chol, double *resid) {
    if (!resid) return CONFLUX_LU_EARG;
    if (!c->store_factors) return CONFLUX_LU_EARG;
    for (auto &r : c->rs)
        if ((r.pk == 0 && !r.Fres) || !r.A11in) return CONFLUX_LU_EARG;
    const int64_t N = c->N;
    const int v = c->v;
    const bool dist = !c->sim && c->world > 1;
    RankState &me = c->rs[0];

    if (dist && me.grank != 0) {
        // non-root: contribute tiles (pk == 0 layers hold the data), then
        // receive the residual broadcast
        if (me.pk == 0) {
            NCCLCHK(ncclSend(me.A11in, i64(c->Ml) * c->Nl, ncclDouble, 0,
                             c->comm, c->stream));
            NCCLCHK(ncclSend(me.Fres, i64(c->Ml) * c->Nl, ncclDouble, 0,
                             c->comm, c->stream));
        }
        double *d_r = nullptr;
        HIPCHK(hipMalloc(&d_r, 8));
        NCCLCHK(ncclBroadcast(d_r, d_r, 1, ncclDouble, 0, c->comm, c->stream));
        HIPCHK(hipMemcpyAsync(resid, d_r, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        (void)hipFree(d_r);
        return CONFLUX_LU_OK;
    }

    // root / single-process path
    double *Ag = nullptr, *Fg = nullptr, *L = nullptr, *C = nullptr,
           *d_acc = nullptr, *tmp = nullptr;
    int *d_pm = nullptr;
    // world==1 LU: A11in IS the global matrix (Px=Py=1) and is only read —
    // alias it instead of burning another N^2 (the N=65536 case needs this)
    const bool aliasA = (!chol && !c->sim && c->world == 1);
    auto cleanup = [&]() {
        if (Ag && !aliasA) (void)hipFree(Ag);
        for (double *p : {Fg, L, C, d_acc, tmp})
            if (p) (void)hipFree(p);
        if (d_pm) (void)hipFree(d_pm);
    };
#define VCHK(x)                                                               \
    if ((x) != hipSuccess) {                                                  \
        cleanup();                                                            \
        return CONFLUX_LU_EHIP;                                               \
    }
#define VNCCL(x)                                                              \
    if ((x) != ncclSuccess) {                                                 \
        cleanup();                                                            \
        return CONFLUX_LU_ECOMM;                                              \
    }
    if (aliasA)
        Ag = me.A11in;
    else
        VCHK(hipMalloc(&Ag, N * N * 8));
    VCHK(hipMalloc(&Fg, N * N * 8));
    if (!chol) {
        VCHK(hipMalloc(&L, i64(v) * N * 8));
        VCHK(hipMalloc(&d_pm, N * 4));
    }
    VCHK(hipMalloc(&C, i64(v) * N * 8));
    VCHK(hipMalloc(&d_acc, (2 + CONFLUX_FROB2_WS_DOUBLES) * 8));
    VCHK(hipMemsetAsync(d_acc, 0, 16, c->stream));

    // assemble global A (input snapshot) and F from the tile-cyclic locals
    // (owner map layout.cpp:95-123)
    const int Nt = (int)(N / v);
    auto scatter_tiles = [&](const double *localA, const double *localF,
                             int pi, int pj) {
        if (c->Px == 1 && c->Py == 1) {  // local IS global: one bulk copy
            if (localA && !aliasA)
                launch_copy2d(localA, c->Nl, Ag, N, c->Ml, c->Nl, c->stream);
            if (localF)
                launch_copy2d(localF, c->Nl, Fg, N, c->Ml, c->Nl, c->stream);
            return;
        }
        for (int ti = pi; ti < Nt; ti += c->Px)
            for (int tj = pj; tj < Nt; tj += c->Py) {
                const int64_t lo =
                    i64(ti / c->Px) * v * c->Nl + i64(tj / c->Py) * v;
                if (localA && !aliasA)
                    launch_copy2d(localA + lo, c->Nl,
                                  Ag + i64(ti) * v * N + tj * v, N, v, v,
                                  c->stream);
                if (localF)
                    launch_copy2d(localF + lo, c->Nl,
                                  Fg + i64(ti) * v * N + tj * v, N, v, v,
                                  c->stream);
            }
    };
    if (c->sim) {
        for (int pi = 0; pi < c->Px; ++pi)
            for (int pj = 0; pj < c->Py; ++pj) {
                RankState *r = get_rs(*c, pi, pj, 0);
                scatter_tiles(r->A11in, r->Fres, pi, pj);
            }
    } else if (!dist) {
        scatter_tiles(me.A11in, me.Fres, 0, 0);
    } else {
        VCHK(hipMalloc(&tmp, i64(c->Ml) * c->Nl * 8));
        for (int pi = 0; pi < c->Px; ++pi)
            for (int pj = 0; pj < c->Py; ++pj) {
                if (pi == me.pi && pj == me.pj) {
                    scatter_tiles(me.A11in, me.Fres, pi, pj);
                    continue;
                }
                const int src = grank_of(*c, pi, pj, 0);
                VNCCL(ncclRecv(tmp, i64(c->Ml) * c->Nl, ncclDouble, src,
                               c->comm, c->stream));
                scatter_tiles(tmp, nullptr, pi, pj);  // A tiles
                // (scatter_tiles writes F from its 2nd arg; split the call)
                VNCCL(ncclRecv(tmp, i64(c->Ml) * c->Nl, ncclDouble, src,
                               c->comm, c->stream));
                scatter_tiles(nullptr, tmp, pi, pj);  // F tiles
            }
    }

    if (!chol) {
        VCHK(hipMemcpyAsync(d_pm, c->pivotInds.data(), N * 4,
                            hipMemcpyHostToDevice, c->stream));
        launch_frob2(Ag, N * N, d_acc + 1, d_acc + 2, c->stream);
        for (int64_t i0 = 0; i0 < N; i0 += v) {
            const int K = (int)(i0 + v);
            // PA stripe: rows perm[i0 .. i0+v)
            launch_row_gather(Ag, N, C, N, d_pm + i0, v, N, c->stream);
            // L stripe (strict lower + unit diag), then strip those rows
            // to pure U in place — later stripes only read rows < their K
            launch_tril_unit_rows(Fg + i0 * N, N, L, N, v, i0, K, c->stream);
            launch_triu_rows(Fg + i0 * N, N, v, i0, c->stream);
            launch_dgemm_f64(L, N, Fg, N, C, N, v, N, K, c->stream);
            launch_frob2(C, i64(v) * N, d_acc, d_acc + 2, c->stream);
        }
    } else {
        // symmetrize from the lower triangle (the generator / reference
        // CholeskyIO fill lower-stored input, dsyrk 'L')
        launch_transpose_add_lower(Ag, N, c->stream);
        launch_frob2(Ag, N * N, d_acc + 1, d_acc + 2, c->stream);
        // Fg <- tril(Fg) in place (upper half of the stored L is junk);
        // the stripe GEMMs then read L directly out of Fg
        launch_tril(Fg, Fg, N, c->stream);
        for (int64_t i0 = 0; i0 < N; i0 += v) {
            const int K = (int)(i0 + v);  // L rows i0.. have cols <= i0+v-1
            launch_copy2d(Ag + i0 * N, N, C, N, v, N, c->stream);
            launch_dgemm_f64_nt(Fg + i0 * N, N, Fg, N, C, N, v, N, K,
                                c->stream);
            launch_frob2(C, i64(v) * N, d_acc, d_acc + 2, c->stream);
        }
    }
    double acc[2] = {0, 0};
    VCHK(hipMemcpyAsync(acc, d_acc, 16, hipMemcpyDeviceToHost, c->stream));
    VCHK(hipStreamSynchronize(c->stream));
    if (!(acc[1] > 0)) {
        cleanup();
        return CONFLUX_LU_EINTERNAL;
    }
    *resid = std::sqrt(acc[0] / acc[1]);
    if (dist) {
        double *d_r = nullptr;
        VCHK(hipMalloc(&d_r, 8));
        VCHK(hipMemcpyAsync(d_r, resid, 8, hipMemcpyHostToDevice, c->stream));
        const ncclResult_t e =
            ncclBroadcast(d_r, d_r, 1, ncclDouble, 0, c->comm, c->stream);
        (void)hipStreamSynchronize(c->stream);
        (void)hipFree(d_r);
        if (e != ncclSuccess) {
            cleanup();
            return CONFLUX_LU_ECOMM;
        }
    }
#undef VCHK
#undef VNCCL
    cleanup();
    return CONFLUX_LU_OK;
}

int conflux_lu_validate(conflux_lu_ctx *c, double *resid) {
    return validate_common(c, false, resid);
}

/* Cholesky counterpart: ||A - L L^T||_F / ||A||_F (the reference's
 * CholeskyValidation, Cholesky.cpp:738-772 analogue). */
int conflux_chol_validate(conflux_lu_ctx *c, double *resid) {
    return validate_common(c, true, resid);
}

/* Multi-RHS solve on the stored factors (getrs / potrs).  The reference has
 * no solve; this consumes what LU_rep leaves behind — the C result buffer
 * and perm (conflux_opt.hpp:1660-1754).
 *
 * Block right-looking, block size sb | v (solve_block), entirely on device:
 *   X <- B[perm]                              (LU; Cholesky: X <- B)
 *   forward,  k = 0 .. Nt-1:  X_k <- L_kk^-1 X_k;  X[k+1:] -= F[k+1:, k] X_k
 *   backward, k = Nt-1 .. 0:  X_k <- U_kk^-1 X_k;  X[:k]   -= F[:k, k]   X_k
 * Both updates are tall (rows x v)(v x nrhs) products — many row tiles, so
 * the chip stays busy at nrhs = 1.
 *
 * F aliasing rule: Fres is never written.  Px = Py = 1 LU reads it in place
 * (Fres IS global F, ld = Nl; no N^2 buffer, so bench-scale N still fits);
 * every other case works on one N^2 staging copy assembled with
 * validate_common's owner map.  Cholesky always stages: the stored upper
 * half of L is junk, so L is mirrored up and the backward sweep (with L^T)
 * becomes the LU code.
 *
 * Real distributed runs (world > 1 processes) are NOT YET SUPPORTED: EARG on
 * every rank before any communication (a collective solve is a follow-up). */
static bool solve_use_skinny() {  // env CONFLUX_SOLVE_SKINNY=0|1, read once
    static const int on = env_int("CONFLUX_SOLVE_SKINNY", 1);
    return on != 0;
}

// Sweep block size.  A v x v triangle is ONE block walking v/32 dependent
// panels, while the update spreads over the whole chip, so a block smaller
// than the factorization tile moves work from the serial kernel into the
// parallel one: at N=16384 v=512 a 128 block measured 21.8 / 30.1 ms
// (nrhs 1 / 128) against 34.2 / 40.1 ms with the full tile (64 and 256 are
// within 10% of 128, 32 loses at nrhs >= 128).  Default: 128 when it
// divides a larger v, else v.  env CONFLUX_SOLVE_BLOCK (read once) overrides
// when it divides v.
static int solve_block(int v) {
    static const int want = env_int("CONFLUX_SOLVE_BLOCK", 0);
    if (want > 0 && want <= v && v % want == 0) return want;
    return (v > 128 && v % 128 == 0) ? 128 : v;
}

// What every solve on one factorization shares, built once per call: global
// F (Fres in place, or one staged N^2 copy) and, for LU, perm on device.
// The refinement loop runs many permute-and-sweep rounds on one of these.
struct SolveDev {
    double *Fg = nullptr;
    int64_t ldf = 0;
    bool aliasF = false;
    int *d_pm = nullptr;  // LU only
    void release() {
        if (Fg && !aliasF) (void)hipFree(Fg);
        if (d_pm) (void)hipFree(d_pm);
        Fg = nullptr;
        d_pm = nullptr;
    }
};

// Tile-cyclic locals -> one global N x N buffer (owner map layout.cpp:95-123;
// the pk == 0 layers hold the data).  `which` picks the local buffer.
extern "C++" template <typename Pick>
static int assemble_global(conflux_lu_ctx *c, double *G, Pick which) {
    const int64_t N = c->N;
    const int v = c->v;
    const int Nt = (int)(N / v);
    RankState *r00 = c->sim ? get_rs(*c, 0, 0, 0) : &c->rs[0];
    for (int pi = 0; pi < c->Px; ++pi)
        for (int pj = 0; pj < c->Py; ++pj) {
            const RankState *r = c->sim ? get_rs(*c, pi, pj, 0) : r00;
            const double *loc = which(*r);
            if (!loc) return CONFLUX_LU_EARG;
            if (c->Px == 1 && c->Py == 1) {
                launch_copy2d(loc, c->Nl, G, N, c->Ml, c->Nl, c->stream);
                continue;
            }
            for (int ti = pi; ti < Nt; ti += c->Px)
                for (int tj = pj; tj < Nt; tj += c->Py)
                    launch_copy2d(loc + i64(ti / c->Px) * v * c->Nl +
                                      i64(tj / c->Py) * v,
                                  c->Nl, G + i64(ti) * v * N + tj * v, N, v,
                                  v, c->stream);
        }
    return CONFLUX_LU_OK;
}

// The guards every solve entry point shares (the condition estimates have
// no B: they pass their own output pointer and nrhs = 1).
static int solve_guard(conflux_lu_ctx *c, bool chol, const void *B,
                       int nrhs) {
    if (!c || !B || nrhs <= 0) return CONFLUX_LU_EARG;
    if (c->factored_kind != (chol ? 2 : 1)) return CONFLUX_LU_EARG;
    if (!c->sim && c->world > 1) return CONFLUX_LU_EARG;  // not yet supported
    RankState *r00 = c->sim ? get_rs(*c, 0, 0, 0) : &c->rs[0];
    if (!r00->Fres) return CONFLUX_LU_EARG;
    return CONFLUX_LU_OK;
}

static int solve_stage(conflux_lu_ctx *c, bool chol, SolveDev &sd) {
    const int64_t N = c->N;
    RankState *r00 = c->sim ? get_rs(*c, 0, 0, 0) : &c->rs[0];
    sd.aliasF = !chol && c->Px == 1 && c->Py == 1;
    if (sd.aliasF) {
        sd.Fg = r00->Fres;
        sd.ldf = c->Nl;
    } else {
        sd.ldf = N;
        if (hipMalloc(&sd.Fg, N * N * 8) != hipSuccess) return CONFLUX_LU_EHIP;
        if (int rc = assemble_global(
                c, sd.Fg, [](const RankState &r) { return r.Fres; }))
            return rc;
        if (chol) launch_transpose_add_lower(sd.Fg, N, c->stream);
    }
    if (!chol) {
        if (hipMalloc(&sd.d_pm, N * 4) != hipSuccess) return CONFLUX_LU_EHIP;
        if (hipMemcpyAsync(sd.d_pm, c->pivotInds.data(), N * 4,
                           hipMemcpyHostToDevice, c->stream) != hipSuccess)
            return CONFLUX_LU_EHIP;
    }
    return CONFLUX_LU_OK;
}

// Xd <- the right-hand side in the factors' row order: row r of PA is row
// perm[r] of A, so X <- B[perm] (LU); Cholesky copies (or works in place
// when Bd == Xd).  LU needs Bd != Xd.
static int solve_permute(conflux_lu_ctx *c, bool chol, const SolveDev &sd,
                         const double *Bd, double *Xd, int nrhs) {
    const int64_t N = c->N;
    if (!chol)
        launch_row_gather(Bd, nrhs, Xd, nrhs, sd.d_pm, (int)N, nrhs,
                          c->stream);
    else if (Bd != Xd &&
             hipMemcpyAsync(Xd, Bd, N * nrhs * 8, hipMemcpyDeviceToDevice,
                            c->stream) != hipSuccess)
        return CONFLUX_LU_EHIP;
    return CONFLUX_LU_OK;
}

// The two sweeps, in place on the device buffer Xd (N x nrhs, ld = nrhs).
// Both directions walk the same sb-blocks of the same F and differ in what
// they launch per block:
//   plain  forward  L_kk^-1 (unit for LU),  X[k+1:] -= F[k+1:, k] X_k
//          backward U_kk^-1,                X[:k]   -= F[:k, k]   X_k
//   trans  forward  U_kk^-T,                X[k+1:] -= F[k, k+1:]^T X_k
//          backward L_kk^-T (unit),         X[:k]   -= F[k, :k]^T   X_k
// (A^T = U^T L^T P; LU only).  The transposed update reads a ROW panel of F
// in place through k_update_skinny_t for every nrhs — there is no transposed
// GEMM to switch to, so CONFLUX_SOLVE_SKINNY does not apply to it.
static void solve_sweeps(conflux_lu_ctx *c, bool chol, const SolveDev &sd,
                         double *Xd, int nrhs, bool trans = false) {
    const int64_t N = c->N;
    const int v = c->v;
    const double *Fg = sd.Fg;
    const int64_t ldf = sd.ldf;
    const bool skinny = nrhs <= 16 && solve_use_skinny();
    const int sb = solve_block(v);  // sweep block size, divides v
    const int nb = (int)(N / sb);
    auto update = [&](const double *A, const double *Xk, double *C, int M) {
        if (M <= 0) return;
        if (trans)
            launch_update_skinny_t(A, ldf, Xk, nrhs, C, nrhs, M, nrhs, sb,
                                   c->stream);
        else if (skinny)
            launch_update_skinny(A, ldf, Xk, nrhs, C, nrhs, M, nrhs, sb,
                                 c->stream);
        else
            launch_dgemm_f64(A, ldf, Xk, nrhs, C, nrhs, M, nrhs, sb,
                             c->stream);
    };
    // diagonal block solve: plain takes the lower half first, trans the upper
    auto tri = [&](int64_t o, double *Xk, int upper_stored, int unit) {
        if (trans)
            launch_trsm_left_tri_mfma_t(Fg + o * ldf + o, ldf, Xk, nrhs, sb,
                                        nrhs, upper_stored, unit, c->stream);
        else
            launch_trsm_left_tri_mfma(Fg + o * ldf + o, ldf, Xk, nrhs, sb,
                                      nrhs, upper_stored, unit, c->stream);
    };
    for (int k = 0; k < nb; ++k) {  // forward: L (unit for LU) / U^T
        const int64_t o = i64(k) * sb;
        double *Xk = Xd + o * nrhs;
        tri(o, Xk, trans ? 1 : 0, (trans || chol) ? 0 : 1);
        update(trans ? Fg + o * ldf + o + sb : Fg + (o + sb) * ldf + o, Xk,
               Xk + i64(sb) * nrhs, (int)(N - o - sb));
    }
    for (int k = nb - 1; k >= 0; --k) {  // backward: U (or L^T, mirrored up)
        const int64_t o = i64(k) * sb;   //           / L^T (unit)
        double *Xk = Xd + o * nrhs;
        tri(o, Xk, trans ? 0 : 1, trans ? 1 : 0);
        update(trans ? Fg + o * ldf : Fg + o, Xk, Xd, (int)o);
    }
}

// trans (LU only): A^T X = B.  The sweeps run on B as uploaded and the
// permutation comes last, as a scatter: P x = z, X[perm[r]] = Z[r].
//
// Two kinds of B share everything between staging and the sweeps.  Host
// (ldb == 0): N_padded x nrhs, ld = nrhs, uploaded whole and downloaded whole.
// Device (ldb >= nrhs): the caller's nf x nrhs window, ld = ldb, staged into
// the same contiguous N x nrhs buffer with rows nf..N zero and cropped on the
// way back; only the window's nf x nrhs doubles are written.
static int solve_common(conflux_lu_ctx *c, bool chol, double *B, int nrhs,
                        double *elapsed_ms, bool trans = false,
                        int64_t ldb = 0) {
    if (int rc = solve_guard(c, chol, B, nrhs)) return rc;
    const int64_t N = c->N;
    const bool dev = ldb > 0;

    SolveDev sd;
    double *Xd = nullptr, *Bd = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    auto cleanup = [&]() {
        sd.release();
        for (double *p : {Xd, Bd})
            if (p) (void)hipFree(p);
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    };
#define SCHK(x)                                                               \
    if ((x) != hipSuccess) {                                                  \
        cleanup();                                                            \
        return CONFLUX_LU_EHIP;                                               \
    }
    if (int rc = solve_stage(c, chol, sd)) {
        cleanup();
        return rc;
    }
    SCHK(hipMalloc(&Xd, N * nrhs * 8));
    if (dev) {
        launch_rhs_stage_in(B, ldb, c->nf, (chol || trans) ? nullptr : sd.d_pm,
                            Xd, N, nrhs, c->stream);
    } else if (chol || trans) {
        SCHK(hipMemcpyAsync(Xd, B, N * nrhs * 8, hipMemcpyHostToDevice,
                            c->stream));
        if (trans) SCHK(hipMalloc(&Bd, N * nrhs * 8));
    } else {
        SCHK(hipMalloc(&Bd, N * nrhs * 8));
        SCHK(hipMemcpyAsync(Bd, B, N * nrhs * 8, hipMemcpyHostToDevice,
                            c->stream));
    }
    if (!dev && !trans &&
        solve_permute(c, chol, sd, chol ? Xd : Bd, Xd, nrhs)) {
        cleanup();
        return CONFLUX_LU_EHIP;
    }
    SCHK(hipEventCreate(&e0));
    SCHK(hipEventCreate(&e1));
    SCHK(hipEventRecord(e0, c->stream));
    solve_sweeps(c, chol, sd, Xd, nrhs, trans);
    SCHK(hipEventRecord(e1, c->stream));
    if (dev) {
        launch_rhs_stage_out(Xd, nrhs, c->nf, trans ? sd.d_pm : nullptr, B,
                             ldb, c->stream);
    } else {
        if (trans)
            launch_row_scatter(Xd, nrhs, Bd, nrhs, sd.d_pm, (int)N, nrhs,
                               c->stream);
        SCHK(hipMemcpyAsync(B, trans ? Bd : Xd, N * nrhs * 8,
                            hipMemcpyDeviceToHost, c->stream));
    }
    SCHK(hipStreamSynchronize(c->stream));
    SCHK(hipGetLastError());
    if (elapsed_ms) {
        float ms = 0;
        SCHK(hipEventElapsedTime(&ms, e0, e1));
        *elapsed_ms = ms;
    }
#undef SCHK
    cleanup();
    return CONFLUX_LU_OK;
}

int conflux_lu_solve(conflux_lu_ctx *c, double *B, int nrhs,
                     double *elapsed_ms) {
    return solve_common(c, false, B, nrhs, elapsed_ms);
}

int conflux_chol_solve(conflux_lu_ctx *c, double *B, int nrhs,
                       double *elapsed_ms) {
    return solve_common(c, true, B, nrhs, elapsed_ms);
}

/* A^T X = B on the stored LU factors (getrs with trans = 'T').  EARG after a
 * Cholesky run through the shared guard: there A = A^T and
 * conflux_chol_solve is the answer. */
int conflux_lu_solve_trans(conflux_lu_ctx *c, double *B, int nrhs,
                           double *elapsed_ms) {
    return solve_common(c, false, B, nrhs, elapsed_ms, true);
}

/* The device-resident dense interface: the caller's n x n device matrix is
 * embedded as blockdiag(A, I) in the padded order N.  All-zero candidate rows
 * lose every tournament playoff and the leaf's zero-pivot rule never scales
 * by them, so the padding stays an inert identity block: perm[n:] is the
 * identity, F[n:, n:] == I, both off-diagonal blocks are zero, and the
 * leading n rows of every solve answer the caller's own system.  Single
 * process only (the one-rank engine and the simulation grids). */
static bool dense_single_process(conflux_lu_ctx *c) {
    return c && (c->sim || c->world == 1);
}

int conflux_lu_set_matrix_device(conflux_lu_ctx *c, const double *dA,
                                 int64_t lda, int n, int order) {
    if (!dense_single_process(c) || !dA || n < 1 || n > c->N || lda < n ||
        (order != 0 && order != 1))
        return CONFLUX_LU_EARG;
    for (auto &r : c->rs) {
        if (r.pk != 0)
            launch_zero2d(r.A11, c->Nl, c->Ml, c->Nl, c->stream);
        else
            launch_dense_import(dA, lda, n, order, r.A11, c->Ml, c->Nl, c->v,
                                c->Px, c->Py, r.pi, r.pj, c->stream);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    c->input_dirty = true;
    c->n = n;
    return CONFLUX_LU_OK;
}

int conflux_lu_logical_order(conflux_lu_ctx *c, int *n) {
    if (!c || !n) return CONFLUX_LU_EARG;
    *n = c->n;
    return CONFLUX_LU_OK;
}

int conflux_lu_get_factors_device(conflux_lu_ctx *c, double *dF, int64_t ldf,
                                  int *dperm) {
    if (!dense_single_process(c) || c->factored_kind == 0 ||
        (dF && ldf < c->nf))
        return CONFLUX_LU_EARG;
    const int n = c->nf;
    if (dF) {
        for (auto &r : c->rs) {
            if (r.pk != 0) continue;
            if (!r.Fres) return CONFLUX_LU_EARG;
            launch_dense_export(r.Fres, c->Ml, c->Nl, c->v, c->Px, c->Py, r.pi,
                                r.pj, dF, ldf, n, c->stream);
        }
        HIPCHK(hipGetLastError());
    }
    if (dperm) {
        if ((int)c->pivotInds.size() < n) return CONFLUX_LU_EARG;
        HIPCHK(hipMemcpyAsync(dperm, c->pivotInds.data(), size_t(n) * 4,
                              hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    return CONFLUX_LU_OK;
}

int conflux_lu_solve_device(conflux_lu_ctx *c, double *dB, int64_t ldb,
                            int nrhs, int trans, double *elapsed_ms) {
    if ((trans != 0 && trans != 1) || nrhs <= 0 || ldb < nrhs)
        return CONFLUX_LU_EARG;
    return solve_common(c, false, dB, nrhs, elapsed_ms, trans == 1, ldb);
}

int conflux_chol_solve_device(conflux_lu_ctx *c, double *dB, int64_t ldb,
                              int nrhs, double *elapsed_ms) {
    if (nrhs <= 0 || ldb < nrhs) return CONFLUX_LU_EARG;
    return solve_common(c, true, dB, nrhs, elapsed_ms, false, ldb);
}

// {sum log|d_i|, negatives, flags} over the leading nf diagonal entries of
// the stored factors: every (p, p, 0) rank contributes the diagonal tiles it
// holds to one nf-vector, one block reduces it in a fixed order.
static int logdet_common(conflux_lu_ctx *c, bool chol, double out3[3]) {
    if (int rc = solve_guard(c, chol, out3, 1)) return rc;
    const int n = c->nf;
    double *d_diag = nullptr, *d_out = nullptr;
    auto cleanup = [&]() {
        if (d_diag) (void)hipFree(d_diag);
        if (d_out) (void)hipFree(d_out);
    };
#define SCHK(x)                                                               \
    if ((x) != hipSuccess) {                                                  \
        cleanup();                                                            \
        return CONFLUX_LU_EHIP;                                               \
    }
    SCHK(hipMalloc(&d_diag, size_t(n) * 8));
    SCHK(hipMalloc(&d_out, 3 * 8));
    for (int p = 0; p < c->Px; ++p) {
        RankState *r = c->sim ? get_rs(*c, p, p, 0) : &c->rs[0];
        if (!r || !r->Fres) {
            cleanup();
            return CONFLUX_LU_EARG;
        }
        launch_diag_gather(r->Fres, c->Ml, c->Nl, c->v, c->Px, p, n, d_diag,
                           c->stream);
    }
    launch_logdet_reduce(d_diag, n, d_out, c->stream);
    SCHK(hipGetLastError());
    SCHK(hipMemcpyAsync(out3, d_out, 3 * 8, hipMemcpyDeviceToHost, c->stream));
    SCHK(hipStreamSynchronize(c->stream));
#undef SCHK
    cleanup();
    return CONFLUX_LU_OK;
}

int conflux_lu_slogdet(conflux_lu_ctx *c, double *sign, double *logabsdet) {
    if (!sign || !logabsdet) return CONFLUX_LU_EARG;
    double o[3];
    if (int rc = logdet_common(c, false, o)) return rc;
    const int flags = (int)o[2];
    if (flags & 2) {  // a NaN or an infinity on the diagonal
        *sign = *logabsdet = std::nan("");
        return CONFLUX_LU_OK;
    }
    if (flags & 1) {  // a zero pivot: the matrix is singular
        *sign = 0.0;
        *logabsdet = -INFINITY;
        return CONFLUX_LU_OK;
    }
    // det(P): parity of the permutation from its cycle lengths
    const std::vector<int> &pm = c->pivotInds;
    std::vector<char> seen(pm.size(), 0);
    int odd = (int)o[1] & 1;
    for (size_t i = 0; i < pm.size(); ++i) {
        if (seen[i]) continue;
        size_t len = 0;
        for (size_t j = i; !seen[j]; j = (size_t)pm[j]) {
            seen[j] = 1;
            ++len;
        }
        odd ^= (int)((len - 1) & 1);
    }
    *sign = odd ? -1.0 : 1.0;
    *logabsdet = o[0];
    return CONFLUX_LU_OK;
}

int conflux_chol_logdet(conflux_lu_ctx *c, double *logdet) {
    if (!logdet) return CONFLUX_LU_EARG;
    double o[3];
    if (int rc = logdet_common(c, true, o)) return rc;
    const int flags = (int)o[2];
    *logdet = (flags & 2) ? std::nan("") : (flags & 1) ? -INFINITY : 2.0 * o[0];
    return CONFLUX_LU_OK;
}

/* test hook (not in the public header): one rank's slice of the input
 * snapshot the last factorization kept (Ml x Nl, host).  grank is ignored by
 * the one-rank engine. */
int conflux_lu_debug_get_input(conflux_lu_ctx *c, int grank, double *local) {
    if (!dense_single_process(c) || !local) return CONFLUX_LU_EARG;
    if (!c->sim) grank = 0;
    if (grank < 0 || grank >= (int)c->rs.size() || !c->rs[grank].A11in)
        return CONFLUX_LU_EARG;
    HIPCHK(hipMemcpyAsync(local, c->rs[grank].A11in, i64(c->Ml) * c->Nl * 8,
                          hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return CONFLUX_LU_OK;
}

/* Reciprocal condition number 1 / (||A|| ||A^-1||) of the matrix last
 * factored (gecon / pocon): ||A|| from the input snapshot, ||A^-1||
 * estimated by norm1est.hpp from single-RHS solves with A and A^T on the
 * stored factors.  The solves run on device; the estimator's O(N) steps run
 * on the host between them in a fixed order (one N-double upload and
 * download per solve), so two calls agree bitwise.  F and perm are staged
 * once per call.  ||A||1 (k_col_abs_sums) and ||A||inf (k_row_abs_sums) are
 * computed on first use and cached until the next factorization; the
 * snapshot is read in place on a Px = Py = 1 grid, else assembled into one
 * N^2 staging copy that is freed before the solves start.
 * inf-norm: ||A^-1||inf = ||A^-T||1, so the two callbacks swap roles.
 * Cholesky: A = A^T, both callbacks are conflux_chol_solve's sweeps. */
static int rcond_common(conflux_lu_ctx *c, bool chol, int norm, double *rcond,
                        double *anorm_out, int *nsolves, double *elapsed_ms) {
    if (int rc = solve_guard(c, chol, rcond, 1)) return rc;
    if (norm != 0 && norm != 1) return CONFLUX_LU_EARG;
    const int64_t N = c->N;
    // logical order: with n < N the figure describes the caller's n x n
    // matrix, not blockdiag(A, I) — ||A|| over the leading block only (a
    // padding column sums to 1 and could win), the estimator at dimension n
    // with callbacks that zero-extend the vector going in and crop the one
    // coming out (the padding block of the inverse is the identity and does
    // not couple to the leading one).  n == N is the path as it always was.
    const int64_t n = c->nf;
    RankState *r00 = c->sim ? get_rs(*c, 0, 0, 0) : &c->rs[0];
    if (!r00->A11in) return CONFLUX_LU_EARG;
    const bool aliasA = c->Px == 1 && c->Py == 1;

    SolveDev sd;
    double *Ag = nullptr, *Xd = nullptr, *Bd = nullptr, *d_sums = nullptr,
           *d_sc = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    auto cleanup = [&]() {
        sd.release();
        if (Ag && !aliasA) (void)hipFree(Ag);
        for (double *p : {Xd, Bd, d_sums, d_sc})
            if (p) (void)hipFree(p);
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    };
#define SCHK(x)                                                               \
    if ((x) != hipSuccess) {                                                  \
        cleanup();                                                            \
        return CONFLUX_LU_EHIP;                                               \
    }
    double &cached = n < N ? c->anorm_lead[norm]
                           : (norm == 0 ? c->anorm_one : c->anorm_inf);
    if (cached < 0) {  // once per factorization and norm
        int64_t lda = N;
        if (aliasA) {
            Ag = r00->A11in;
            lda = c->Nl;
        } else {
            SCHK(hipMalloc(&Ag, N * N * 8));
            if (int rc = assemble_global(
                    c, Ag, [](const RankState &r) { return r.A11in; })) {
                cleanup();
                return rc;
            }
        }
        SCHK(hipMalloc(&d_sums, (size_t)N * 8));
        SCHK(hipMalloc(&d_sc, 8));
        if (norm == 0)
            launch_col_abs_sums(Ag, lda, (int)n, (int)n, d_sums, c->stream);
        else
            launch_row_abs_sums(Ag, lda, (int)n, (int)n, d_sums, c->stream);
        launch_colmax_abs(d_sums, n, 1, d_sc, c->stream);
        double nrm = 0;
        SCHK(hipMemcpyAsync(&nrm, d_sc, 8, hipMemcpyDeviceToHost, c->stream));
        SCHK(hipStreamSynchronize(c->stream));
        cached = nrm;
        if (!aliasA) {
            (void)hipFree(Ag);
            Ag = nullptr;
        }
    }
    const double anorm = cached;

    if (int rc = solve_stage(c, chol, sd)) {
        cleanup();
        return rc;
    }
    SCHK(hipMalloc(&Xd, (size_t)N * 8));
    if (!chol) SCHK(hipMalloc(&Bd, (size_t)N * 8));
    hipError_t herr = hipSuccess;  // the callbacks cannot return: first error
    auto up = [&](double *dst, const double *x) {
        if (herr == hipSuccess && n < N)
            herr = hipMemsetAsync(dst + n, 0, (size_t)(N - n) * 8, c->stream);
        if (herr == hipSuccess)
            herr = hipMemcpyAsync(dst, x, (size_t)n * 8,
                                  hipMemcpyHostToDevice, c->stream);
    };
    auto down = [&](double *x, const double *src) {
        if (herr == hipSuccess)
            herr = hipMemcpyAsync(x, src, (size_t)n * 8,
                                  hipMemcpyDeviceToHost, c->stream);
        if (herr == hipSuccess) herr = hipStreamSynchronize(c->stream);
    };
    auto apply = [&](double *x) {  // x <- A^-1 x
        up(chol ? Xd : Bd, x);
        if (herr == hipSuccess && solve_permute(c, chol, sd, chol ? Xd : Bd,
                                                Xd, 1))
            herr = hipErrorUnknown;
        if (herr == hipSuccess) solve_sweeps(c, chol, sd, Xd, 1);
        down(x, Xd);
    };
    auto apply_t = [&](double *x) {  // x <- A^-T x
        if (chol) return apply(x);
        up(Xd, x);
        if (herr == hipSuccess) {
            solve_sweeps(c, false, sd, Xd, 1, true);
            launch_row_scatter(Xd, 1, Bd, 1, sd.d_pm, (int)N, 1, c->stream);
        }
        down(x, Bd);
    };
    SCHK(hipEventCreate(&e0));
    SCHK(hipEventCreate(&e1));
    SCHK(hipEventRecord(e0, c->stream));
    const norm1est::Result est =
        norm == 0 ? norm1est::estimate((int)n, apply, apply_t)
                  : norm1est::estimate((int)n, apply_t, apply);
    SCHK(herr);
    SCHK(hipEventRecord(e1, c->stream));
    SCHK(hipStreamSynchronize(c->stream));
    SCHK(hipGetLastError());
    *rcond = norm1est::rcond_from(anorm, est.est);
    if (anorm_out) *anorm_out = anorm;
    if (nsolves) *nsolves = est.nsolves;
    if (elapsed_ms) {
        float ms = 0;
        SCHK(hipEventElapsedTime(&ms, e0, e1));
        *elapsed_ms = ms;
    }
#undef SCHK
    cleanup();
    return CONFLUX_LU_OK;
}

int conflux_lu_rcond(conflux_lu_ctx *c, int norm, double *rcond,
                     double *anorm, int *nsolves, double *elapsed_ms) {
    return rcond_common(c, false, norm, rcond, anorm, nsolves, elapsed_ms);
}

int conflux_chol_rcond(conflux_lu_ctx *c, double *rcond, double *anorm,
                       int *nsolves, double *elapsed_ms) {
    return rcond_common(c, true, 0, rcond, anorm, nsolves, elapsed_ms);
}

/* Solve with extra-precise iterative refinement (the xGERFSX idea: the
 * residual is accumulated in doubled precision and rounded once, so the
 * correction solve sees the true residual even where B - A X cancels to
 * nothing in working precision).  The reference has no counterpart.
 *
 *   X = solve(B);  it = 0
 *   loop:
 *     R = B - A X                      k_residual_dd on the stored input
 *     berr_j = max|R_j| / (||A||inf max|X_j| + max|B_j|)
 *     stop if it == max_iter or no column is active
 *     D = solve(R)
 *     per active column, d_j = max|D_j|:
 *       it > 0 and d_j > d_prev_j / 2  -> stagnated: freeze, D_j NOT applied
 *       else X_j += D_j, ferr_j = d_j / max|X_j|, and freeze as converged
 *            when d_j <= 2^-53 max|X_j|
 *     it += 1
 * A column whose residual is exactly zero is frozen on the spot: there is
 * nothing left to correct.  The decisions are taken on the host from the
 * per-column maxima — nrhs doubles per download, two downloads and one
 * nrhs-int mask upload per pass; X, R and D never leave the device.
 *
 * A is the input snapshot A11in, which the factorization never touches:
 * read in place on a Px = Py = 1 grid (no N^2 buffer), else assembled into
 * one N^2 staging copy with the owner map of the F staging.  ||A||inf is
 * computed on first use and cached until the next factorization.  F and
 * perm are staged once per call; every pass reuses them.
 *
 * Determinism: the residual kernels combine their partial accumulators in an
 * order fixed by lane, wave and chunk indices, the maxima are exact, so two
 * calls agree bitwise.
 *
 * trans (LU only): the same loop on A^T X = B.  solve() is the transposed
 * solve — sweeps in place, then the scatter X[perm[r]] = Z[r] — the residual
 * B - A^T X comes from launch_residual_dd_t on the same snapshot, read in
 * place (its workspace is row-chunks x N x column-group, not N^2), and berr
 * takes ||A^T||inf = ||A||1, the norm the condition estimate caches.
 *
 * Two kinds of B, as in solve_common.  Host (ldb == 0): N_padded x nrhs, and
 * everything describes the padded matrix, as it always did.  Device
 * (ldb >= nrhs): the caller's nf x nrhs window; it is kept, zero-extended to
 * N rows, for the residual (X overwrites the window), and everything
 * describes the caller's nf x nf matrix: the norm is the leading block's,
 * the residual runs over the leading nf rows and columns, and the padding
 * rows of X, R and D stay exactly zero (R's are zeroed once and never
 * written, the sweeps map zero rows to zero rows), so they cannot win a
 * column maximum.  With nf == N the two describe the same thing, launch for
 * launch. */
static int solve_refined_common(conflux_lu_ctx *c, bool chol, double *B,
                                int nrhs, int max_iter, double *berr,
                                double *ferr, int *iters, double *elapsed_ms,
                                bool trans = false, int64_t ldb = 0) {
    if (int rc = solve_guard(c, chol, B, nrhs)) return rc;
    if (max_iter < 0) return CONFLUX_LU_EARG;
    const int64_t N = c->N;
    const bool dev = ldb > 0;
    const int64_t m = dev ? c->nf : N;  // the order everything describes
    RankState *r00 = c->sim ? get_rs(*c, 0, 0, 0) : &c->rs[0];
    if (!r00->A11in) return CONFLUX_LU_EARG;
    const bool aliasA = c->Px == 1 && c->Py == 1;

    SolveDev sd;
    double *Ag = nullptr, *Bd = nullptr, *Xd = nullptr, *Rd = nullptr,
           *Dd = nullptr, *d_sc = nullptr, *d_rows = nullptr, *d_ws = nullptr;
    int *d_mask = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    auto cleanup = [&]() {
        sd.release();
        if (Ag && !aliasA) (void)hipFree(Ag);
        if (Dd && Dd != Rd) (void)hipFree(Dd);
        for (double *p : {Bd, Xd, Rd, d_sc, d_rows, d_ws})
            if (p) (void)hipFree(p);
        if (d_mask) (void)hipFree(d_mask);
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    };
#define SCHK(x)                                                               \
    if ((x) != hipSuccess) {                                                  \
        cleanup();                                                            \
        return CONFLUX_LU_EHIP;                                               \
    }
    if (int rc = solve_stage(c, chol, sd)) {
        cleanup();
        return rc;
    }
    int64_t lda = N;
    if (aliasA) {
        Ag = r00->A11in;
        lda = c->Nl;
    } else {
        SCHK(hipMalloc(&Ag, N * N * 8));
        if (int rc = assemble_global(
                c, Ag, [](const RankState &r) { return r.A11in; })) {
            cleanup();
            return rc;
        }
    }
    const size_t xb = (size_t)N * nrhs * 8;
    SCHK(hipMalloc(&Bd, xb));
    SCHK(hipMalloc(&Xd, xb));
    SCHK(hipMalloc(&Rd, xb));
    if (chol)
        Dd = Rd;  // the Cholesky sweeps run in place on the residual
    else
        SCHK(hipMalloc(&Dd, xb));
    SCHK(hipMalloc(&d_sc, (size_t)nrhs * 8));
    SCHK(hipMalloc(&d_mask, (size_t)nrhs * 4));
    if (trans)
        SCHK(hipMalloc(&d_ws, residual_dd_t_ws_bytes((int)m, (int)m, nrhs)));
    if (dev)
        launch_rhs_stage_in(B, ldb, (int)m, nullptr, Bd, N, nrhs, c->stream);
    else
        SCHK(hipMemcpyAsync(Bd, B, xb, hipMemcpyHostToDevice, c->stream));
    if (m < N) SCHK(hipMemsetAsync(Rd, 0, xb, c->stream));

    std::vector<double> xmax(nrhs), bmax(nrhs), rmax(nrhs), dmax(nrhs),
        dprev(nrhs, 0.0), be(nrhs, 0.0), fe(nrhs, 0.0);
    std::vector<int> active(nrhs, 1), mask(nrhs, 0);
    // per-column max|.| of a device N x nrhs array -> host (synchronises)
    auto colmax = [&](const double *V, std::vector<double> &out) {
        launch_colmax_abs(V, N, nrhs, d_sc, c->stream);
        hipError_t e = hipMemcpyAsync(out.data(), d_sc, (size_t)nrhs * 8,
                                      hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        return e;
    };
    // ||A||inf, or ||A^T||inf = ||A||1, of the order-m matrix: the slots the
    // condition estimate fills, once per factorization
    double &cached = m < N ? c->anorm_lead[trans ? 0 : 1]
                           : (trans ? c->anorm_one : c->anorm_inf);
    if (cached < 0) {
        SCHK(hipMalloc(&d_rows, (size_t)N * 8));
        if (trans)
            launch_col_abs_sums(Ag, lda, (int)m, (int)m, d_rows, c->stream);
        else
            launch_row_abs_sums(Ag, lda, (int)m, (int)m, d_rows, c->stream);
        launch_colmax_abs(d_rows, m, 1, d_sc, c->stream);
        double nrm = 0;
        SCHK(hipMemcpyAsync(&nrm, d_sc, 8, hipMemcpyDeviceToHost, c->stream));
        SCHK(hipStreamSynchronize(c->stream));
        cached = nrm;
    }
    const double anorm = cached;
    SCHK(colmax(Bd, bmax));

    // dst <- solve(src), dst != src unless Cholesky.  trans sweeps in place
    // on src (clobbered) and scatters into dst.
    auto solve_into = [&](double *src, double *dst) {
        if (trans) {
            solve_sweeps(c, false, sd, src, nrhs, true);
            launch_row_scatter(src, nrhs, dst, nrhs, sd.d_pm, (int)N, nrhs,
                               c->stream);
            return 0;
        }
        if (solve_permute(c, chol, sd, src, dst, nrhs)) return 1;
        solve_sweeps(c, chol, sd, dst, nrhs);
        return 0;
    };
    SCHK(hipEventCreate(&e0));
    SCHK(hipEventCreate(&e1));
    SCHK(hipEventRecord(e0, c->stream));
    // trans: B goes through Rd, which the first residual overwrites anyway
    if (trans)
        SCHK(hipMemcpyAsync(Rd, Bd, xb, hipMemcpyDeviceToDevice, c->stream));
    if (solve_into(trans ? Rd : Bd, Xd)) {
        cleanup();
        return CONFLUX_LU_EHIP;
    }
    SCHK(colmax(Xd, xmax));

    const double u = 0x1p-53;
    int it = 0, applied_passes = 0;
    for (;;) {
        if (trans)
            (void)launch_residual_dd_t(Ag, lda, Xd, Bd, Rd, (int)m, (int)m,
                                       nrhs, c->stream, d_ws);
        else
            launch_residual_dd(Ag, lda, Xd, Bd, Rd, (int)m, (int)m, nrhs,
                               c->stream);
        SCHK(colmax(Rd, rmax));
        int nactive = 0;
        for (int j = 0; j < nrhs; ++j) {
            const double den = anorm * xmax[j] + bmax[j];
            be[j] = den == 0 ? 0.0 : rmax[j] / den;
            if (rmax[j] == 0) active[j] = 0;  // exact: nothing to correct
            nactive += active[j];
        }
        if (it == max_iter || nactive == 0) break;
        if (solve_into(Rd, Dd)) {
            cleanup();
            return CONFLUX_LU_EHIP;
        }
        SCHK(colmax(Dd, dmax));
        int napplied = 0;
        for (int j = 0; j < nrhs; ++j) {
            mask[j] = 0;
            if (!active[j]) continue;
            // !(d <= d_prev / 2) also catches a NaN correction
            if (it > 0 && !(dmax[j] <= 0.5 * dprev[j])) {
                active[j] = 0;  // stagnated: this correction is not applied
                continue;
            }
            mask[j] = 1;
            dprev[j] = dmax[j];
            ++napplied;
        }
        ++it;
        if (!napplied) break;  // X unchanged: berr above still describes it
        SCHK(hipMemcpyAsync(d_mask, mask.data(), (size_t)nrhs * 4,
                            hipMemcpyHostToDevice, c->stream));
        launch_axpy_masked(Xd, Dd, d_mask, N, nrhs, c->stream);
        SCHK(colmax(Xd, xmax));
        for (int j = 0; j < nrhs; ++j) {
            if (!mask[j]) continue;
            fe[j] = xmax[j] == 0 ? 0.0 : dmax[j] / xmax[j];
            if (dmax[j] <= u * xmax[j]) active[j] = 0;  // converged
        }
        ++applied_passes;
    }
    SCHK(hipEventRecord(e1, c->stream));
    if (dev)
        launch_rhs_stage_out(Xd, nrhs, (int)m, nullptr, B, ldb, c->stream);
    else
        SCHK(hipMemcpyAsync(B, Xd, xb, hipMemcpyDeviceToHost, c->stream));
    SCHK(hipStreamSynchronize(c->stream));
    SCHK(hipGetLastError());
    if (berr) std::copy(be.begin(), be.end(), berr);
    if (ferr) std::copy(fe.begin(), fe.end(), ferr);
    if (iters) *iters = applied_passes;
    if (elapsed_ms) {
        float ms = 0;
        SCHK(hipEventElapsedTime(&ms, e0, e1));
        *elapsed_ms = ms;
    }
#undef SCHK
    cleanup();
    return CONFLUX_LU_OK;
}

int conflux_lu_solve_refined(conflux_lu_ctx *c, double *B, int nrhs,
                             int max_iter, double *berr, double *ferr,
                             int *iters, double *elapsed_ms) {
    return solve_refined_common(c, false, B, nrhs, max_iter, berr, ferr,
                                iters, elapsed_ms);
}

int conflux_chol_solve_refined(conflux_lu_ctx *c, double *B, int nrhs,
                               int max_iter, double *berr, double *ferr,
                               int *iters, double *elapsed_ms) {
    return solve_refined_common(c, true, B, nrhs, max_iter, berr, ferr, iters,
                                elapsed_ms);
}

int conflux_lu_solve_refined_trans(conflux_lu_ctx *c, double *B, int nrhs,
                                   int max_iter, double *berr, double *ferr,
                                   int *iters, double *elapsed_ms) {
    return solve_refined_common(c, false, B, nrhs, max_iter, berr, ferr,
                                iters, elapsed_ms, true);
}

int conflux_lu_solve_refined_device(conflux_lu_ctx *c, double *dB, int64_t ldb,
                                    int nrhs, int trans, int max_iter,
                                    double *berr, double *ferr, int *iters,
                                    double *elapsed_ms) {
    if ((trans != 0 && trans != 1) || nrhs <= 0 || ldb < nrhs)
        return CONFLUX_LU_EARG;
    return solve_refined_common(c, false, dB, nrhs, max_iter, berr, ferr,
                                iters, elapsed_ms, trans == 1, ldb);
}

int conflux_chol_solve_refined_device(conflux_lu_ctx *c, double *dB,
                                      int64_t ldb, int nrhs, int max_iter,
                                      double *berr, double *ferr, int *iters,
                                      double *elapsed_ms) {
    if (nrhs <= 0 || ldb < nrhs) return CONFLUX_LU_EARG;
    return solve_refined_common(c, true, dB, nrhs, max_iter, berr, ferr,
                                iters, elapsed_ms, false, ldb);
}

int conflux_lu_get_factors(conflux_lu_ctx *c, double *F_local, int *perm) {
    if (c->sim) return conflux_lu_get_factors_sim(c, 0, F_local, perm);
    RankState &r = c->rs[0];
    if (F_local) {
        if (!r.Fres) return CONFLUX_LU_EARG;
        HIPCHK(hipMemcpyAsync(F_local, r.Fres, i64(c->Ml) * c->Nl * 8,
                              hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    if (perm) std::copy(c->pivotInds.begin(), c->pivotInds.end(), perm);
    return CONFLUX_LU_OK;
}

int conflux_lu_dims(conflux_lu_ctx *c, int *Ml, int *Nl, int *Nt, int *nlayr,
                    int *M_padded, int *N_padded) {
    if (Ml) *Ml = c->Ml;
    if (Nl) *Nl = c->Nl;
    if (Nt) *Nt = c->Nt;
    if (nlayr) *nlayr = c->nlayr;
    if (M_padded) *M_padded = c->M;
    if (N_padded) *N_padded = c->N;
    return CONFLUX_LU_OK;
}

int conflux_lu_kernel_stats(conflux_lu_ctx *c, int kernel, double *seconds,
                            long *launches, double *flops) {
    if (kernel < 0 || kernel > 3) return CONFLUX_LU_EARG;
    if (seconds) *seconds = c->cats[kernel].seconds;
    if (launches) *launches = c->cats[kernel].launches;
    if (flops) *flops = c->cats[kernel].flops;
    return CONFLUX_LU_OK;
}

// ---- kernel-level debug entry points (host buffers in/out; used by the
// numerics unit tests to pin each kernel against a numpy reference) --------
int conflux_lu_debug_dgemm(int M, int64_t N, int K, const double *A,
                           const double *B, double *C) {
    hipStream_t s;
    HIPCHK(hipStreamCreate(&s));
    double *dA, *dB, *dC;
    HIPCHK(hipMalloc(&dA, i64(M) * K * 8));
    HIPCHK(hipMalloc(&dB, i64(K) * N * 8));
    HIPCHK(hipMalloc(&dC, i64(M) * N * 8));
    HIPCHK(hipMemcpy(dA, A, i64(M) * K * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dB, B, i64(K) * N * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dC, C, i64(M) * N * 8, hipMemcpyHostToDevice));
    launch_dgemm_f64(dA, K, dB, N, dC, N, M, N, K, s);
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipMemcpy(C, dC, i64(M) * N * 8, hipMemcpyDeviceToHost));
    (void)hipFree(dA); (void)hipFree(dB); (void)hipFree(dC);
    (void)hipStreamDestroy(s);
    return CONFLUX_LU_OK;
}

// ---- kernel pins: one launcher per entry, on host buffers that are uploaded
// and downloaded WHOLE (padding rows and columns included), so a test sees
// every byte a kernel could have touched.  Each returns CONFLUX_LU_EARG before
// any launch for a size, leading dimension or mask argument outside the
// launcher's domain.
}  // extern "C"
namespace {
struct PinBuf {  // device image of one whole host buffer
    double *d = nullptr;
    int64_t n = 0;
    ~PinBuf() {
        if (d) (void)hipFree(d);
    }
    int up(const double *h, int64_t nelem) {
        n = nelem;
        HIPCHK(hipMalloc(&d, n * 8));
        HIPCHK(hipMemcpy(d, h, n * 8, hipMemcpyHostToDevice));
        return 0;
    }
    int down(double *h) const {
        HIPCHK(hipMemcpy(h, d, n * 8, hipMemcpyDeviceToHost));
        return 0;
    }
};
struct PinStream {
    hipStream_t s{};
    bool live = false;
    ~PinStream() {
        if (live) (void)hipStreamDestroy(s);
    }
    int make() {
        HIPCHK(hipStreamCreate(&s));
        live = true;
        return 0;
    }
};
const int64_t PIN_MAX_ELEMS = int64_t(1) << 28;  // 2 GiB per buffer
bool pin_dims_ok(int64_t rows, int64_t ld, int64_t width) {
    return rows > 0 && width > 0 && ld >= width && ld <= PIN_MAX_ELEMS &&
           rows <= PIN_MAX_ELEMS / ld;
}
}  // namespace
extern "C" {

// launch_dgemm_f64 on the top-left M x N of a c_rows x ldc host C (A: M x
// lda, B: K x ldb) with `variant` selected for this one call and `maxwg` as
// the launcher takes it.
int conflux_lu_debug_dgemm_ex(int variant, int maxwg, int M, int64_t N, int K,
                              int64_t lda, int64_t ldb, int64_t ldc,
                              int64_t c_rows, const double *A, const double *B,
                              double *C) {
    if (variant < 0 || variant > 3 || maxwg < 0 || !A || !B || !C ||
        c_rows < M || !pin_dims_ok(M, lda, K) || !pin_dims_ok(K, ldb, N) ||
        !pin_dims_ok(c_rows, ldc, N))
        return CONFLUX_LU_EARG;
    PinStream st;
    PinBuf dA, dB, dC;
    if (st.make() || dA.up(A, M * lda) || dB.up(B, K * ldb) ||
        dC.up(C, c_rows * ldc))
        return CONFLUX_LU_EHIP;
    const int prev = conflux_gemm_set_variant(variant);
    launch_dgemm_f64(dA.d, lda, dB.d, ldb, dC.d, ldc, M, N, K, st.s, maxwg);
    conflux_gemm_set_variant(prev);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st.s));
    return dC.down(C);
}

// strip width of the GEMM tile order (0/1 = flat) and the non-temporal C
// epilogue of the GemmW8 edition, for this process; each returns the previous value
int conflux_lu_debug_set_gemm_strip(int w) {
    return conflux_gemm_set_strip_w(w);
}
int conflux_lu_debug_set_gemm_ntc(int on) { return conflux_gemm_set_ntc(on); }

// C (top-left M x N of c_rows x ldc) -= A (M x lda) B^T (B: N x ldb).  v == 0:
// launch_dgemm_f64_nt; otherwise launch_dgemm_f64_nt_tril with that mask.
// A == B (one host pointer, as in potrf_tile) is uploaded once and passed
// twice; it then needs lda == ldb.
int conflux_lu_debug_dgemm_nt(int M, int64_t N, int K, int64_t lda,
                              int64_t ldb, int64_t ldc, int64_t c_rows,
                              const double *A, const double *B, double *C,
                              int v, int r0off, int64_t c0off, int Px, int Py,
                              int pi, int pj) {
    if (!A || !B || !C || c_rows < M || !pin_dims_ok(M, lda, K) ||
        !pin_dims_ok(N, ldb, K) || !pin_dims_ok(c_rows, ldc, N) ||
        (A == B && lda != ldb) || v < 0)
        return CONFLUX_LU_EARG;
    if (v > 0 &&
        (v % 128 != 0 || M % v != 0 || N % v != 0 || r0off < 0 || c0off < 0 ||
         r0off % v != 0 || c0off % v != 0 || r0off > (1 << 28) ||
         c0off > (1 << 28) || Px < 1 || Py < 1 || Px > 4096 || Py > 4096 ||
         pi < 0 || pi >= Px || pj < 0 || pj >= Py))
        return CONFLUX_LU_EARG;
    const bool alias = A == B;
    PinStream st;
    PinBuf dA, dB, dC;
    if (st.make() || dC.up(C, c_rows * ldc)) return CONFLUX_LU_EHIP;
    if (alias) {
        if (dA.up(A, std::max<int64_t>(M, N) * lda)) return CONFLUX_LU_EHIP;
    } else if (dA.up(A, M * lda) || dB.up(B, N * ldb)) {
        return CONFLUX_LU_EHIP;
    }
    const double *pB = alias ? dA.d : dB.d;
    if (v == 0)
        launch_dgemm_f64_nt(dA.d, lda, pB, ldb, dC.d, ldc, M, N, K, st.s);
    else
        launch_dgemm_f64_nt_tril(dA.d, lda, pB, ldb, dC.d, ldc, M, N, K, v,
                                 r0off, c0off, Px, Py, pi, pj, st.s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st.s));
    return dC.down(C);
}

// launch_potrf32 / launch_getrf32_nopiv on the top-left nb x nb of a rows x
// lda host A
static int debug_factor32(bool chol, int nb, int64_t lda, int64_t rows,
                          double *A) {
    if (!A || nb < 1 || nb > 32 || rows < nb || !pin_dims_ok(rows, lda, nb))
        return CONFLUX_LU_EARG;
    PinStream st;
    PinBuf dA;
    if (st.make() || dA.up(A, rows * lda)) return CONFLUX_LU_EHIP;
    if (chol)
        launch_potrf32(dA.d, lda, nb, st.s);
    else
        launch_getrf32_nopiv(dA.d, lda, nb, st.s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st.s));
    return dA.down(A);
}
int conflux_lu_debug_potrf32(int nb, int64_t lda, int64_t rows, double *A) {
    return debug_factor32(true, nb, lda, rows, A);
}
int conflux_lu_debug_getrf32_nopiv(int nb, int64_t lda, int64_t rows,
                                   double *A) {
    return debug_factor32(false, nb, lda, rows, A);
}

// launch_trsm_right_upper32: X (M x ldx, first nb columns) <- X U^-1 (trans =
// 0, U upper) or X L^-T (trans = 1, L lower), U / L the top-left nb x nb of an
// nb x ldu host array
int conflux_lu_debug_trsm32(int trans, int nb, int64_t M, int64_t ldu,
                            int64_t ldx, const double *U, double *X) {
    if (!U || !X || (trans != 0 && trans != 1) || nb < 1 || nb > 32 ||
        !pin_dims_ok(nb, ldu, nb) || !pin_dims_ok(M, ldx, nb))
        return CONFLUX_LU_EARG;
    PinStream st;
    PinBuf dU, dX;
    if (st.make() || dU.up(U, nb * ldu) || dX.up(X, M * ldx))
        return CONFLUX_LU_EHIP;
    launch_trsm_right_upper32(dU.d, ldu, dX.d, ldx, nb, M, trans, st.s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st.s));
    return dX.down(X);
}

// the engine's blocked potrf_tile (potrf32 / trsm32 / NT GEMM chain) on the
// top-left v x v of a rows x ld host T
int conflux_lu_debug_potrf_tile(int v, int64_t ld, int64_t rows, double *T) {
    if (!T || v < 1 || v > 4096 || rows < v || !pin_dims_ok(rows, ld, v))
        return CONFLUX_LU_EARG;
    Ctx c;
    c.v = v;
    PinStream st;
    PinBuf dT;
    if (st.make() || dT.up(T, rows * ld)) return CONFLUX_LU_EHIP;
    c.stream = st.s;
    int rc = potrf_tile(c, dT.d, ld);
    if (!rc && hipGetLastError() != hipSuccess) rc = CONFLUX_LU_EHIP;
    if (hipStreamSynchronize(st.s) != hipSuccess) rc = CONFLUX_LU_EHIP;
    for (auto &e : c.evs) {
        (void)hipEventDestroy(e.a);
        (void)hipEventDestroy(e.b);
    }
    return rc ? rc : dT.down(T);
}

// Fres[grow][gcol] += delta on the pk == 0 rank that owns the element (rows in
// pivoted order, columns global; validate_common's owner map).  Simulation
// grids and the one-rank real mode; EARG without stored factors or when
// world > 1.
int conflux_lu_debug_poke_factor(conflux_lu_ctx *c, int64_t grow, int64_t gcol,
                                 double delta) {
    if (!c || !c->store_factors || c->factored_kind == 0 ||
        (!c->sim && c->world > 1) || grow < 0 || gcol < 0 || grow >= c->M ||
        gcol >= c->N)
        return CONFLUX_LU_EARG;
    const int v = c->v;
    const int ti = (int)(grow / v), tj = (int)(gcol / v);
    RankState *r = c->sim ? get_rs(*c, ti % c->Px, tj % c->Py, 0) : &c->rs[0];
    const int64_t lrow = i64(ti / c->Px) * v + grow % v;
    const int64_t lcol = i64(tj / c->Py) * v + gcol % v;
    if (!r || !r->Fres || lrow >= c->Ml || lcol >= c->Nl ||
        (!c->sim && (c->Px != 1 || c->Py != 1)))
        return CONFLUX_LU_EARG;
    double *p = r->Fres + lrow * c->Nl + lcol;
    double x = 0;
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(&x, p, 8, hipMemcpyDeviceToHost));
    x += delta;
    HIPCHK(hipMemcpy(p, &x, 8, hipMemcpyHostToDevice));
    return CONFLUX_LU_OK;
}

int conflux_lu_debug_dgemm_bench(int M, int64_t N, int K, int iters,
                                 double *tflops) {
    hipStream_t s;
    HIPCHK(hipStreamCreate(&s));
    double *dA, *dB, *dC;
    HIPCHK(hipMalloc(&dA, i64(M) * K * 8));
    HIPCHK(hipMalloc(&dB, i64(K) * N * 8));
    HIPCHK(hipMalloc(&dC, i64(M) * N * 8));
    launch_init_matrix(dA, M, K, K, 1, 1, 0, 0, 0, 7, s);
    launch_init_matrix(dB, K, (int)N, (int)N, 1, 1, 0, 0, 0, 8, s);
    launch_init_matrix(dC, M, (int)N, (int)N, 1, 1, 0, 0, 0, 9, s);
    launch_dgemm_f64(dA, K, dB, N, dC, N, M, N, K, s);  // warmup
    hipEvent_t a, b;
    HIPCHK(hipEventCreate(&a));
    HIPCHK(hipEventCreate(&b));
    HIPCHK(hipEventRecord(a, s));
    for (int i = 0; i < iters; ++i)
        launch_dgemm_f64(dA, K, dB, N, dC, N, M, N, K, s);
    HIPCHK(hipEventRecord(b, s));
    HIPCHK(hipEventSynchronize(b));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, a, b));
    *tflops = 2.0 * M * (double)N * K * iters / (ms * 1e-3) / 1e12;
    (void)hipFree(dA); (void)hipFree(dB); (void)hipFree(dC);
    (void)hipEventDestroy(a); (void)hipEventDestroy(b);
    (void)hipStreamDestroy(s);
    return CONFLUX_LU_OK;
}

int conflux_lu_debug_dgemm_nt_bench(int M, int64_t N, int K, int iters,
                                    double *tflops) {
    hipStream_t s;
    HIPCHK(hipStreamCreate(&s));
    double *dA, *dB, *dC;
    HIPCHK(hipMalloc(&dA, i64(M) * K * 8));
    HIPCHK(hipMalloc(&dB, N * K * 8));
    HIPCHK(hipMalloc(&dC, i64(M) * N * 8));
    launch_init_matrix(dA, M, K, K, 1, 1, 0, 0, 0, 7, s);
    launch_init_matrix(dB, (int)N, K, K, 1, 1, 0, 0, 0, 8, s);
    launch_init_matrix(dC, M, (int)N, (int)N, 1, 1, 0, 0, 0, 9, s);
    launch_dgemm_f64_nt(dA, K, dB, K, dC, N, M, N, K, s);  // warmup
    hipEvent_t a, b;
    HIPCHK(hipEventCreate(&a));
    HIPCHK(hipEventCreate(&b));
    HIPCHK(hipEventRecord(a, s));
    for (int i = 0; i < iters; ++i)
        launch_dgemm_f64_nt(dA, K, dB, K, dC, N, M, N, K, s);
    HIPCHK(hipEventRecord(b, s));
    HIPCHK(hipEventSynchronize(b));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, a, b));
    *tflops = 2.0 * M * (double)N * K * iters / (ms * 1e-3) / 1e12;
    (void)hipFree(dA); (void)hipFree(dB); (void)hipFree(dC);
    (void)hipEventDestroy(a); (void)hipEventDestroy(b);
    (void)hipStreamDestroy(s);
    return CONFLUX_LU_OK;
}

/* achieved-GB/s probe for the row-shuffle kernels (report
 * the HBM-bound kernels separately): gathers `rows` pivot rows of `cols`
 * doubles out of an Ml x cols matrix through k_row_gather, `iters` times.
 * Reported bytes = read + write of the moved rows. */
int conflux_lu_debug_rowmove_bench(int Ml, int64_t cols, int rows, int iters,
                                   double *gbps) {
    hipStream_t s;
    HIPCHK(hipStreamCreate(&s));
    double *src, *dst;
    int *idx;
    HIPCHK(hipMalloc(&src, i64(Ml) * cols * 8));
    HIPCHK(hipMalloc(&dst, i64(rows) * cols * 8));
    HIPCHK(hipMalloc(&idx, rows * 4));
    launch_init_matrix(src, Ml, (int)cols, (int)cols, 1, 1, 0, 0, 0, 11, s);
    std::vector<int> h(rows);
    for (int i = 0; i < rows; ++i)
        h[i] = (int)((i64(i) * 2654435761u) % Ml);  // scattered rows
    HIPCHK(hipMemcpy(idx, h.data(), rows * 4, hipMemcpyHostToDevice));
    launch_row_gather(src, cols, dst, cols, idx, rows, cols, s);  // warmup
    hipEvent_t a, b;
    HIPCHK(hipEventCreate(&a));
    HIPCHK(hipEventCreate(&b));
    HIPCHK(hipEventRecord(a, s));
    for (int i = 0; i < iters; ++i)
        launch_row_gather(src, cols, dst, cols, idx, rows, cols, s);
    HIPCHK(hipEventRecord(b, s));
    HIPCHK(hipEventSynchronize(b));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, a, b));
    *gbps = 2.0 * rows * (double)cols * 8 * iters / (ms * 1e-3) / 1e9;
    (void)hipFree(src); (void)hipFree(dst); (void)hipFree(idx);
    (void)hipEventDestroy(a); (void)hipEventDestroy(b);
    (void)hipStreamDestroy(s);
    return CONFLUX_LU_OK;
}

// select the panel's inter-leaf glue for this process (1 = fused, 0 = the
// four-launch chain); returns the previous mode
int conflux_lu_debug_set_panel_glue(int mode) {
    const int prev = panel_glue_mode();
    g_panel_glue = mode != 0;
    return prev;
}

// select the leaf kernel of full 32-column leaves for this process (1 = the
// register-resident k_panel_factor_reg, 0 = k_panel_factor); returns the
// previous mode
int conflux_lu_debug_set_panel_reg(int mode) {
    return conflux_panel_set_reg_mode(mode);
}

// select the register leaf's hand-off form (1 = drain-free granule payload,
// 0 = sc1 payload, drain, key); returns the previous mode
int conflux_lu_debug_set_panel_publish(int mode) {
    return conflux_panel_set_publish_mode(mode);
}

// switch the instrumented leaf kernels on or off (CONFLUX_PANEL_PHASE_STATS);
// returns the previous mode
int conflux_lu_debug_set_panel_phase_stats(int mode) {
    return conflux_panel_set_phase_stats_mode(mode);
}

// the phase totals gathered since the last call: out9[0..3] cycles of wave 0
// summed over all blocks (poll wait, load, update, publish), out9[4..7] block
// 0's, out9[8] the columns covered; resets them
int conflux_lu_debug_panel_phase_stats(unsigned long long *out9) {
    if (!out9) return CONFLUX_LU_EARG;
    for (int i = 0; i < 8; ++i) {
        out9[i] = g_panel_phase_acc[i];
        g_panel_phase_acc[i] = 0;
    }
    out9[8] = g_panel_phase_cols;
    g_panel_phase_cols = 0;
    return CONFLUX_LU_OK;
}

int conflux_lu_debug_getrf(int n, int v, double *panel, int *ipiv_out) {
    Ctx c;
    c.v = v;
    HIPCHK(hipStreamCreate(&c.stream));
    RankState r;
    HIPCHK(hipMalloc(&r.panel, i64(std::max(n, 2 * v)) * v * 8));
    HIPCHK(hipMalloc(&r.d_ipiv, (v + 8) * 4));
    HIPCHK(hipMalloc(&r.d_swap, 128 * 4));
    HIPCHK(hipMalloc(&r.rowtmp, i64(64) * v * 8));
    HIPCHK(hipMalloc(&r.sync, conflux_panel_sync_bytes()));
    HIPCHK(hipMemset(r.sync, 0, conflux_panel_sync_bytes()));
    HIPCHK(hipMemcpy(r.panel, panel, i64(n) * v * 8, hipMemcpyHostToDevice));
    std::vector<int> ipiv;
    int rc = factor_panel(c, r, n, ipiv);
    if (!rc) {
        HIPCHK(hipMemcpy(panel, r.panel, i64(n) * v * 8,
                         hipMemcpyDeviceToHost));
        std::copy(ipiv.begin(), ipiv.end(), ipiv_out);
    }
    (void)hipFree(r.panel); (void)hipFree(r.d_ipiv);
    (void)hipFree(r.d_swap); (void)hipFree(r.rowtmp);
    (void)hipFree(r.sync);
    for (auto &e : c.evs) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    (void)hipStreamDestroy(c.stream);
    return rc;
}

int conflux_lu_debug_trsm(int side_right, int M_or_v, int64_t N_or_M,
                          int v, const double *T, double *X) {
    // side_right: X (N_or_M x v) <- X * U^-1 ; else X (v x N_or_M) <- L^-1 X
    Ctx c;
    c.v = v;
    HIPCHK(hipStreamCreate(&c.stream));
    RankState r;
    HIPCHK(hipMalloc(&r.A00, i64(v) * v * 8));
    HIPCHK(hipMemcpy(r.A00, T, i64(v) * v * 8, hipMemcpyHostToDevice));
    double *dX;
    const int64_t xsz = side_right ? N_or_M * v : i64(v) * N_or_M;
    HIPCHK(hipMalloc(&dX, xsz * 8));
    HIPCHK(hipMemcpy(dX, X, xsz * 8, hipMemcpyHostToDevice));
    int rc = side_right ? trsm_right_upper(c, r, dX, v, (int)N_or_M)
                        : trsm_left_lower(c, r, dX, N_or_M, N_or_M);
    HIPCHK(hipStreamSynchronize(c.stream));
    if (!rc) HIPCHK(hipMemcpy(X, dX, xsz * 8, hipMemcpyDeviceToHost));
    (void)hipFree(r.A00); (void)hipFree(dX);
    if (r.triws) (void)hipFree(r.triws);
    for (auto &e : c.evs) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    (void)hipStreamDestroy(c.stream);
    (void)M_or_v;
    return rc;
}

// select the fused panel solves for this process (1 = stripe-resident, 0 =
// panel-streaming); returns the previous mode
int conflux_lu_debug_set_trsm_stripe(int mode) {
    const int prev = trsm_stripe_mode();
    g_trsm_stripe = mode != 0;
    return prev;
}

// columns (left solve) / rows (right solve) one block of the stripe-resident
// solves owns
int conflux_lu_debug_trsm_stripe_width() { return conflux_trsm_stripe_width(); }

// conflux_lu_debug_trsm on a window of a wider host array X with leading
// dimension ldx: side_right -> X[0:n, off:off+v] <- that * U^-1 (trans=0, T
// upper) or * L^-T (trans=1, T lower; the Cholesky solve); else
// X[0:v, off:off+n] <- L^-1 * that (T unit lower).  Nothing outside the
// window is written.
int conflux_lu_debug_trsm_ld(int side_right, int trans, int v, int64_t n,
                             int64_t ldx, int64_t off, const double *T,
                             double *X) {
    if (v <= 0 || n <= 0 || off < 0 || !T || !X ||
        ldx < off + (side_right ? i64(v) : n) || n > INT32_MAX)
        return CONFLUX_LU_EARG;
    Ctx c;
    c.v = v;
    HIPCHK(hipStreamCreate(&c.stream));
    RankState r;
    HIPCHK(hipMalloc(&r.A00, i64(v) * v * 8));
    HIPCHK(hipMemcpy(r.A00, T, i64(v) * v * 8, hipMemcpyHostToDevice));
    double *dX;
    const int64_t xsz = (side_right ? n : i64(v)) * ldx;
    HIPCHK(hipMalloc(&dX, xsz * 8));
    HIPCHK(hipMemcpy(dX, X, xsz * 8, hipMemcpyHostToDevice));
    int rc = !side_right ? trsm_left_lower(c, r, dX + off, ldx, n)
             : trans     ? trsm_right_lowT(c, r, dX + off, ldx, (int)n)
                         : trsm_right_upper(c, r, dX + off, ldx, (int)n);
    HIPCHK(hipStreamSynchronize(c.stream));
    if (!rc) HIPCHK(hipMemcpy(X, dX, xsz * 8, hipMemcpyDeviceToHost));
    (void)hipFree(r.A00); (void)hipFree(dX);
    if (r.triws) (void)hipFree(r.triws);
    for (auto &e : c.evs) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    (void)hipStreamDestroy(c.stream);
    return rc;
}

// select the one-rank direct step for this process (bit mask, see
// one_rank_direct_mode; 0 = the staged path); returns the previous mode.
// Read at the start of each factorization.
int conflux_lu_debug_set_one_rank_direct(int mode) {
    const int prev = one_rank_direct_mode();
    g_one_rank_direct = mode & ORD_ALL;
    return prev;
}

// The stripe solves out of place, as the one-rank direct step uses them: the
// window of Xs (host, leading dimension lds) at column soff is solved into
// the window of Xd (host, ldd) at column doff; side_right -> windows are n x
// v and the result is Xs_win * U^-1 (T upper), else v x n and L^-1 * Xs_win
// (T unit lower).  Xd == NULL solves in place in Xs (ldd, doff ignored).
// Both arrays are written back whole, so a caller sees that nothing outside
// the destination window changed and that Xs was only read.
int conflux_lu_debug_trsm_oop(int side_right, int v, int64_t n, int64_t lds,
                              int64_t soff, int64_t ldd, int64_t doff,
                              const double *T, double *Xs, double *Xd) {
    const int64_t w = side_right ? i64(v) : n;
    if (v <= 0 || n <= 0 || !T || !Xs || soff < 0 || lds < soff + w ||
        (Xd && (doff < 0 || ldd < doff + w)) || n > INT32_MAX ||
        !conflux_trsm_stripe_fits(v))
        return CONFLUX_LU_EARG;
    const int64_t rows = side_right ? n : i64(v);
    double *dT = nullptr, *dS = nullptr, *dD = nullptr, *ws = nullptr;
    auto cleanup = [&]() {
        for (double *p : {dT, dS, dD, ws})
            if (p) (void)hipFree(p);
    };
    hipError_t e = hipMalloc(&dT, i64(v) * v * 8);
    if (e == hipSuccess) e = hipMalloc(&dS, rows * lds * 8);
    if (e == hipSuccess && Xd) e = hipMalloc(&dD, rows * ldd * 8);
    if (e == hipSuccess)
        e = hipMalloc(&ws, conflux_trsm_stripe_ws_doubles(v) * 8);
    if (e == hipSuccess)
        e = hipMemcpy(dT, T, i64(v) * v * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = hipMemcpy(dS, Xs, rows * lds * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess && Xd)
        e = hipMemcpy(dD, Xd, rows * ldd * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        double *dst = Xd ? dD + doff : dS + soff;
        const int64_t ld2 = Xd ? ldd : lds;
        launch_trsm_pack_tri(dT, v, v, side_right ? 0 : 1, 0, ws, nullptr);
        if (side_right)
            launch_trsm_right_stripe_packed(ws, dS + soff, lds, dst, ld2, v, n,
                                            nullptr);
        else
            launch_trsm_left_stripe_packed(ws, dS + soff, lds, dst, ld2, v, n,
                                           nullptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess)
        e = hipMemcpy(Xs, dS, rows * lds * 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess && Xd)
        e = hipMemcpy(Xd, dD, rows * ldd * 8, hipMemcpyDeviceToHost);
    cleanup();
    HIPCHK(e);
    return CONFLUX_LU_OK;
}

// X (v x N) <- T^-1 X with T (v x ldt host, only its triangle read)
int conflux_lu_debug_trsm_left(int upper, int unit, int v, int64_t N,
                               int64_t ldt, const double *T, double *X) {
    if (v <= 0 || N <= 0 || ldt < v || !T || !X) return CONFLUX_LU_EARG;
    double *dT = nullptr, *dX = nullptr;
    auto cleanup = [&]() {
        for (double *p : {dT, dX})
            if (p) (void)hipFree(p);
    };
    hipError_t e = hipMalloc(&dT, i64(v) * ldt * 8);
    if (e == hipSuccess) e = hipMalloc(&dX, i64(v) * N * 8);
    if (e == hipSuccess)
        e = hipMemcpy(dT, T, i64(v) * ldt * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = hipMemcpy(dX, X, i64(v) * N * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        launch_trsm_left_tri_mfma(dT, ldt, dX, N, v, N, upper, unit, nullptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess)
        e = hipMemcpy(X, dX, i64(v) * N * 8, hipMemcpyDeviceToHost);
    cleanup();
    HIPCHK(e);
    return CONFLUX_LU_OK;
}

// C (M x nrhs) -= A (M x lda host, K columns used) * B (K x nrhs)
int conflux_lu_debug_update_skinny(int M, int nrhs, int K, int64_t lda,
                                   const double *A, const double *B,
                                   double *C) {
    if (M <= 0 || nrhs <= 0 || nrhs > 16 || K <= 0 || lda < K || !A || !B ||
        !C)
        return CONFLUX_LU_EARG;
    double *dA = nullptr, *dB = nullptr, *dC = nullptr;
    auto cleanup = [&]() {
        for (double *p : {dA, dB, dC})
            if (p) (void)hipFree(p);
    };
    hipError_t e = hipMalloc(&dA, i64(M) * lda * 8);
    if (e == hipSuccess) e = hipMalloc(&dB, i64(K) * nrhs * 8);
    if (e == hipSuccess) e = hipMalloc(&dC, i64(M) * nrhs * 8);
    if (e == hipSuccess)
        e = hipMemcpy(dA, A, i64(M) * lda * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = hipMemcpy(dB, B, i64(K) * nrhs * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = hipMemcpy(dC, C, i64(M) * nrhs * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        launch_update_skinny(dA, lda, dB, nrhs, dC, nrhs, M, nrhs, K, nullptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess)
        e = hipMemcpy(C, dC, i64(M) * nrhs * 8, hipMemcpyDeviceToHost);
    cleanup();
    HIPCHK(e);
    return CONFLUX_LU_OK;
}

// X (v x N) <- T^-T X with T (v x ldt host, only its stored triangle read)
int conflux_lu_debug_trsm_left_trans(int upper_stored, int unit, int v,
                                     int64_t N, int64_t ldt, const double *T,
                                     double *X) {
    if (v <= 0 || N <= 0 || ldt < v || !T || !X) return CONFLUX_LU_EARG;
    double *dT = nullptr, *dX = nullptr;
    auto cleanup = [&]() {
        for (double *p : {dT, dX})
            if (p) (void)hipFree(p);
    };
    hipError_t e = hipMalloc(&dT, i64(v) * ldt * 8);
    if (e == hipSuccess) e = hipMalloc(&dX, i64(v) * N * 8);
    if (e == hipSuccess)
        e = hipMemcpy(dT, T, i64(v) * ldt * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = hipMemcpy(dX, X, i64(v) * N * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        launch_trsm_left_tri_mfma_t(dT, ldt, dX, N, v, N, upper_stored, unit,
                                    nullptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess)
        e = hipMemcpy(X, dX, i64(v) * N * 8, hipMemcpyDeviceToHost);
    cleanup();
    HIPCHK(e);
    return CONFLUX_LU_OK;
}

// C (M x nrhs) -= A^T B, A (K x lda host, M columns used), B (K x nrhs)
int conflux_lu_debug_update_skinny_t(int M, int nrhs, int K, int64_t lda,
                                     const double *A, const double *B,
                                     double *C) {
    if (M <= 0 || nrhs <= 0 || nrhs > 16 || K <= 0 || lda < M || !A || !B ||
        !C)
        return CONFLUX_LU_EARG;
    double *dA = nullptr, *dB = nullptr, *dC = nullptr;
    auto cleanup = [&]() {
        for (double *p : {dA, dB, dC})
            if (p) (void)hipFree(p);
    };
    hipError_t e = hipMalloc(&dA, i64(K) * lda * 8);
    if (e == hipSuccess) e = hipMalloc(&dB, i64(K) * nrhs * 8);
    if (e == hipSuccess) e = hipMalloc(&dC, i64(M) * nrhs * 8);
    if (e == hipSuccess)
        e = hipMemcpy(dA, A, i64(K) * lda * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = hipMemcpy(dB, B, i64(K) * nrhs * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = hipMemcpy(dC, C, i64(M) * nrhs * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        launch_update_skinny_t(dA, lda, dB, nrhs, dC, nrhs, M, nrhs, K,
                               nullptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess)
        e = hipMemcpy(C, dC, i64(M) * nrhs * 8, hipMemcpyDeviceToHost);
    cleanup();
    HIPCHK(e);
    return CONFLUX_LU_OK;
}

// R (M x nrhs) = B - A (M x lda host, K columns used) * X (K x nrhs) with
// the doubled-precision accumulator
int conflux_lu_debug_residual_dd(int M, int K, int nrhs, int64_t lda,
                                 const double *A, const double *X,
                                 const double *B, double *R) {
    if (M <= 0 || nrhs <= 0 || K <= 0 || lda < K || !A || !X || !B || !R)
        return CONFLUX_LU_EARG;
    double *dA = nullptr, *dX = nullptr, *dB = nullptr, *dR = nullptr;
    auto cleanup = [&]() {
        for (double *p : {dA, dX, dB, dR})
            if (p) (void)hipFree(p);
    };
    hipError_t e = hipMalloc(&dA, i64(M) * lda * 8);
    if (e == hipSuccess) e = hipMalloc(&dX, i64(K) * nrhs * 8);
    if (e == hipSuccess) e = hipMalloc(&dB, i64(M) * nrhs * 8);
    if (e == hipSuccess) e = hipMalloc(&dR, i64(M) * nrhs * 8);
    if (e == hipSuccess)
        e = hipMemcpy(dA, A, i64(M) * lda * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = hipMemcpy(dX, X, i64(K) * nrhs * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = hipMemcpy(dB, B, i64(M) * nrhs * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        launch_residual_dd(dA, lda, dX, dB, dR, M, K, nrhs, nullptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess)
        e = hipMemcpy(R, dR, i64(M) * nrhs * 8, hipMemcpyDeviceToHost);
    cleanup();
    HIPCHK(e);
    return CONFLUX_LU_OK;
}

int conflux_lu_debug_residual_group_width() {
    return conflux_residual_group_width();
}

// R (K x nrhs) = B - A^T X, A (M x lda host, K columns used), X (M x nrhs),
// with the doubled-precision accumulator; A is uploaded as it lies and read
// in place
int conflux_lu_debug_residual_dd_t(int M, int K, int nrhs, int64_t lda,
                                   const double *A, const double *X,
                                   const double *B, double *R) {
    if (M <= 0 || nrhs <= 0 || K <= 0 || lda < K || !A || !X || !B || !R)
        return CONFLUX_LU_EARG;
    double *dA = nullptr, *dX = nullptr, *dB = nullptr, *dR = nullptr;
    auto cleanup = [&]() {
        for (double *p : {dA, dX, dB, dR})
            if (p) (void)hipFree(p);
    };
    hipError_t e = hipMalloc(&dA, i64(M) * lda * 8);
    if (e == hipSuccess) e = hipMalloc(&dX, i64(M) * nrhs * 8);
    if (e == hipSuccess) e = hipMalloc(&dB, i64(K) * nrhs * 8);
    if (e == hipSuccess) e = hipMalloc(&dR, i64(K) * nrhs * 8);
    if (e == hipSuccess)
        e = hipMemcpy(dA, A, i64(M) * lda * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = hipMemcpy(dX, X, i64(M) * nrhs * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = hipMemcpy(dB, B, i64(K) * nrhs * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        if (launch_residual_dd_t(dA, lda, dX, dB, dR, M, K, nrhs, nullptr))
            e = hipErrorOutOfMemory;
        else
            e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess)
        e = hipMemcpy(R, dR, i64(K) * nrhs * 8, hipMemcpyDeviceToHost);
    cleanup();
    HIPCHK(e);
    return CONFLUX_LU_OK;
}

int conflux_lu_debug_residual_t_chunk() { return conflux_residual_t_chunk(); }

/* Device-only timing of the residual (tools/solve_bench.py --refine):
 * ms_resid = mean ms of one R = B - A X over an M x K matrix and nrhs
 * columns (ceil(nrhs / group width) passes over A); ms_copy = mean ms of a
 * device-to-device copy of the same M*K*8 bytes, the bandwidth yardstick
 * of the same run. */
int conflux_lu_debug_residual_dd_bench(int M, int K, int nrhs, int iters,
                                       double *ms_resid, double *ms_copy) {
    if (M <= 0 || K <= 0 || nrhs <= 0 || iters <= 0 || !ms_resid || !ms_copy)
        return CONFLUX_LU_EARG;
    hipStream_t s;
    HIPCHK(hipStreamCreate(&s));
    double *dA, *dA2, *dX, *dB, *dR;
    HIPCHK(hipMalloc(&dA, i64(M) * K * 8));
    HIPCHK(hipMalloc(&dA2, i64(M) * K * 8));
    HIPCHK(hipMalloc(&dX, i64(K) * nrhs * 8));
    HIPCHK(hipMalloc(&dB, i64(M) * nrhs * 8));
    HIPCHK(hipMalloc(&dR, i64(M) * nrhs * 8));
    launch_init_matrix(dA, M, K, K, 1, 1, 0, 0, 0, 7, s);
    launch_init_matrix(dX, K, nrhs, nrhs, 1, 1, 0, 0, 0, 8, s);
    launch_init_matrix(dB, M, nrhs, nrhs, 1, 1, 0, 0, 0, 9, s);
    hipEvent_t a, b;
    HIPCHK(hipEventCreate(&a));
    HIPCHK(hipEventCreate(&b));
    float ms = 0;
    launch_residual_dd(dA, K, dX, dB, dR, M, K, nrhs, s);  // warmup
    HIPCHK(hipEventRecord(a, s));
    for (int i = 0; i < iters; ++i)
        launch_residual_dd(dA, K, dX, dB, dR, M, K, nrhs, s);
    HIPCHK(hipEventRecord(b, s));
    HIPCHK(hipEventSynchronize(b));
    HIPCHK(hipEventElapsedTime(&ms, a, b));
    *ms_resid = ms / iters;
    HIPCHK(hipMemcpyAsync(dA2, dA, i64(M) * K * 8, hipMemcpyDeviceToDevice,
                          s));  // warmup
    HIPCHK(hipEventRecord(a, s));
    for (int i = 0; i < iters; ++i)
        HIPCHK(hipMemcpyAsync(dA2, dA, i64(M) * K * 8,
                              hipMemcpyDeviceToDevice, s));
    HIPCHK(hipEventRecord(b, s));
    HIPCHK(hipEventSynchronize(b));
    HIPCHK(hipEventElapsedTime(&ms, a, b));
    *ms_copy = ms / iters;
    HIPCHK(hipGetLastError());
    (void)hipFree(dA); (void)hipFree(dA2); (void)hipFree(dX);
    (void)hipFree(dB); (void)hipFree(dR);
    (void)hipEventDestroy(a); (void)hipEventDestroy(b);
    (void)hipStreamDestroy(s);
    return CONFLUX_LU_OK;
}

/* The same for the transposed residual (tools/solve_bench.py --refine
 * --trans): ms_resid_t = mean ms of one R = B - A^T X over the M x K matrix
 * (workspace allocated once, outside the timed window), ms_resid = one plain
 * R = B - A X over the same matrix, ms_copy = the device copy of its bytes —
 * all three in one run, on one buffer. */
int conflux_lu_debug_residual_dd_t_bench(int M, int K, int nrhs, int iters,
                                         double *ms_resid_t, double *ms_resid,
                                         double *ms_copy) {
    if (M <= 0 || K <= 0 || nrhs <= 0 || iters <= 0 || !ms_resid_t ||
        !ms_resid || !ms_copy)
        return CONFLUX_LU_EARG;
    hipStream_t s;
    HIPCHK(hipStreamCreate(&s));
    const int L = std::max(M, K);
    double *dA, *dA2, *dX, *dB, *dR, *dW;
    HIPCHK(hipMalloc(&dA, i64(M) * K * 8));
    HIPCHK(hipMalloc(&dA2, i64(M) * K * 8));
    HIPCHK(hipMalloc(&dX, i64(L) * nrhs * 8));
    HIPCHK(hipMalloc(&dB, i64(L) * nrhs * 8));
    HIPCHK(hipMalloc(&dR, i64(L) * nrhs * 8));
    HIPCHK(hipMalloc(&dW, residual_dd_t_ws_bytes(M, K, nrhs)));
    launch_init_matrix(dA, M, K, K, 1, 1, 0, 0, 0, 7, s);
    launch_init_matrix(dX, L, nrhs, nrhs, 1, 1, 0, 0, 0, 8, s);
    launch_init_matrix(dB, L, nrhs, nrhs, 1, 1, 0, 0, 0, 9, s);
    hipEvent_t a, b;
    HIPCHK(hipEventCreate(&a));
    HIPCHK(hipEventCreate(&b));
    auto timed = [&](auto &&run, double *out) -> int {
        float ms = 0;
        run();  // warmup
        HIPCHK(hipEventRecord(a, s));
        for (int i = 0; i < iters; ++i) run();
        HIPCHK(hipEventRecord(b, s));
        HIPCHK(hipEventSynchronize(b));
        HIPCHK(hipEventElapsedTime(&ms, a, b));
        *out = ms / iters;
        return CONFLUX_LU_OK;
    };
    int rc = timed(
        [&] {
            (void)launch_residual_dd_t(dA, K, dX, dB, dR, M, K, nrhs, s, dW);
        },
        ms_resid_t);
    if (!rc)
        rc = timed(
            [&] { launch_residual_dd(dA, K, dX, dB, dR, M, K, nrhs, s); },
            ms_resid);
    if (!rc)
        rc = timed(
            [&] {
                (void)hipMemcpyAsync(dA2, dA, i64(M) * K * 8,
                                     hipMemcpyDeviceToDevice, s);
            },
            ms_copy);
    const hipError_t e = hipGetLastError();
    for (double *p : {dA, dA2, dX, dB, dR, dW}) (void)hipFree(p);
    (void)hipEventDestroy(a); (void)hipEventDestroy(b);
    (void)hipStreamDestroy(s);
    if (rc) return rc;
    HIPCHK(e);
    return CONFLUX_LU_OK;
}

int conflux_lu_destroy(conflux_lu_ctx *c) {
    for (auto &r : c->rs) free_rank(r);
    for (auto &e : c->evs) {
        (void)hipEventDestroy(e.a);
        (void)hipEventDestroy(e.b);
    }
    if (c->have_pcomm) (void)ncclCommDestroy(c->pcomm);
    if (c->have_comm) (void)ncclCommDestroy(c->comm);
    if (c->panel_stream) (void)hipStreamDestroy(c->panel_stream);
    if (c->trsm_stream) (void)hipStreamDestroy(c->trsm_stream);
    if (c->ev_pc) (void)hipEventDestroy(c->ev_pc);
    if (c->ev_t3) (void)hipEventDestroy(c->ev_t3);
    if (c->ev_t5) (void)hipEventDestroy(c->ev_t5);
    if (c->ev_t5a) (void)hipEventDestroy(c->ev_t5a);
    (void)hipStreamDestroy(c->stream);
    delete c;
    return CONFLUX_LU_OK;
}

}  // extern "C"
