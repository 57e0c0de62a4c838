"""High-precision references, derived error bounds and fp64 emulations for the
kernel-level pins (test_hp_ref.py on the CPU; test_gemm_modes_gpu.py and
test_chol_kernels_gpu.py on the GPU).  Not a conftest: import it.

Reference
---------
The same operation in numpy.longdouble.  On x86 that is the 80-bit format
(64-bit significand, eps 1.08e-19 = 2^-11 u), so the reference's own rounding
is at most K * 2^-11 u relative to |A||B|: three orders below one fp64
rounding, and inside the slack of every bound below.

Bounds (u = 2^-53, all ELEMENTWISE, none fitted to any output)
--------------------------------------------------------------
GEMM  got = C - A B  (or C - A B^T), K terms.
    The kernels form acc = sum_k a_k b_k from a zero accumulator and subtract
    it from C once.  For ANY summation order, with or without FMA,
    |acc - sum| <= gamma_K |a|.|b|, gamma_K = K u / (1 - K u)  (Higham, ASNA
    2nd ed., eq. 3.5).  The subtraction adds one rounding of (C - acc):
    |got - ref| <= gamma_K |A||B| + u (|C| + (1 + gamma_K) |A||B|)
                <= (K + 2) u (|A||B| + |C|)          for K^2 u << 1.
potrf32  (lower Cholesky of an nb x nb block).
    Higham Thm 10.3: |A - L L^T| <= gamma_{n+1} |L||L^T|.  The kernel scales a
    column by fl(1 / l_cc) instead of dividing: one more rounding per element,
    gamma_{n+2}; (nb + 3) u covers gamma's second-order term.  Only the lower
    triangle is compared (the kernel neither reads nor writes the upper one).
getrf32_nopiv  (LU without pivoting, unit lower L).
    Higham Thm 9.3: |A - L U| <= gamma_n |L||U|; the reciprocal adds one:
    (nb + 2) u.
trsm32  (X_out T = X_in by substitution, T = U or L^T, true division).
    Higham Thm 8.5 row by row: |X_out T - X_in| <= gamma_n |X_out||T|;
    (nb + 2) u leaves the same second-order slack.
potrf_tile at width v  (potrf32 / trsm32 / NT-GEMM chain).
    A blocked Cholesky computes every l_ij from a_ij minus v-or-fewer products
    and one division or reciprocal multiply, in another order; Thm 10.3's proof
    holds for any order, so the potrf32 constant carries over: (v + 3) u.

Emulations
----------
emu_* repeat each kernel's operation order in plain fp64 numpy (no FMA; the
GPU contracts a*b+c into FMA, which only removes roundings, and the bounds
hold either way).  test_hp_ref.py shows that they sit inside the bounds and
that one planted defect of each kind lands far outside.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
TILE = 128                      # GEMM workgroup tile (GEMM_BM = GEMM_BN)
CANARY = np.uint64(0x7FF8DEADBEEFCAFE)   # a quiet NaN with a payload


# ---- canaries -------------------------------------------------------------
def canvas(rows, cols):
    a = np.empty((rows, cols), dtype=np.float64)
    a.view(np.uint64)[...] = CANARY
    return a


def framed(win, rows, ld):
    """win in the top-left corner of a rows x ld canvas of canaries."""
    c = canvas(rows, ld)
    c[:win.shape[0], :win.shape[1]] = win
    return c


def frame_intact(buf, m, n):
    """Every element outside buf[:m, :n] still holds the canary bits."""
    u = buf.view(np.uint64)
    return bool((u[:m, n:] == CANARY).all() and (u[m:, :] == CANARY).all())


def bits_equal(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(
        (a.view(np.uint64) == b.view(np.uint64)).all())


# ---- ratio of an error to its bound -----------------------------------------
def worst_ratio(err, bound):
    """max err / bound; inf where the bound is 0 and the error is not, or
    where anything is not finite."""
    err = np.asarray(err, dtype=LD)
    bound = np.asarray(bound, dtype=LD)
    if err.size == 0:
        return 0.0
    if not (np.isfinite(err).all() and np.isfinite(bound).all()):
        return float("inf")
    pos = bound > 0
    r = np.where(pos, err / np.where(pos, bound, 1), np.where(err > 0, np.inf, 0))
    return float(r.max())


# ---- references and bounds ----------------------------------------------------
def gemm_ref(A, B, C, nt=False):
    """(ref, bound) of C - A B (nt: C - A B^T) in longdouble."""
    A, B, C = (np.asarray(x, dtype=LD) for x in (A, B, C))
    Bk = B.T if nt else B
    K = A.shape[1]
    ref = C - A @ Bk
    bound = (K + 2) * LD(U) * (np.abs(A) @ np.abs(Bk) + np.abs(C))
    return ref, bound


def gemm_ratio(got, A, B, C, nt=False):
    ref, bound = gemm_ref(A, B, C, nt)
    return worst_ratio(np.abs(np.asarray(got, dtype=LD) - ref), bound)


def gemm_exact(A, B, C, nt=False):
    """fp64 image of the longdouble reference (exact for integer inputs)."""
    return gemm_ref(A, B, C, nt)[0].astype(np.float64)


def potrf_ratio(A, F, width=None):
    """A: input block; F: the kernel's output (L in its lower triangle)."""
    n = A.shape[0]
    width = n if width is None else width
    L = np.tril(np.asarray(F, dtype=LD))
    if not (np.isfinite(L).all() and (np.diag(L) > 0).all()):
        return float("inf")
    low = np.tril(np.ones((n, n), dtype=bool))
    err = np.abs(np.asarray(A, dtype=LD) - L @ L.T)
    bound = (width + 3) * LD(U) * (np.abs(L) @ np.abs(L).T)
    return worst_ratio(err[low], bound[low])


def getrf_ratio(A, F):
    n = A.shape[0]
    F = np.asarray(F, dtype=LD)
    L = np.tril(F, -1) + np.eye(n, dtype=LD)
    Uf = np.triu(F)
    err = np.abs(np.asarray(A, dtype=LD) - L @ Uf)
    return worst_ratio(err, (n + 2) * LD(U) * (np.abs(L) @ np.abs(Uf)))


def trsm_ratio(Xin, Xout, T, trans):
    """T: the nb x nb array handed to the kernel (U upper, or L lower with
    trans); only the triangle the operation is defined on is used."""
    T = np.asarray(T, dtype=LD)
    Tm = np.tril(T).T if trans else np.triu(T)
    nb = T.shape[0]
    Xo = np.asarray(Xout, dtype=LD)
    err = np.abs(Xo @ Tm - np.asarray(Xin, dtype=LD))
    return worst_ratio(err, (nb + 2) * LD(U) * (np.abs(Xo) @ np.abs(Tm)))


def tri_mask(M, N, v, r0off, c0off, Px, Py, pi, pj):
    """The TriMask rule per 128 x 128 block: block (bi, bj) is updated iff
    ((r0off + row) // v) * Px + pi >= ((c0off + col) // v) * Py + pj."""
    rows = np.arange(0, M, TILE)
    cols = np.arange(0, N, TILE)
    gti = ((r0off + rows) // v) * Px + pi
    gtj = ((c0off + cols) // v) * Py + pj
    return gti[:, None] >= gtj[None, :]


def blocks_to_elements(upd, M, N):
    return np.kron(upd, np.ones((TILE, TILE), dtype=bool))[:M, :N]


def masked_nt_check(got, A, B, C, upd):
    """(worst ratio over the updated blocks, untouched blocks bitwise equal
    to C)."""
    M, N = C.shape
    e = blocks_to_elements(upd, M, N)
    ref, bound = gemm_ref(A, B, C, nt=True)
    err = np.abs(np.asarray(got, dtype=LD) - ref)
    same = np.asarray(got).view(np.uint64) == np.asarray(C).view(np.uint64)
    return worst_ratio(err[e], bound[e]), bool(same[~e].all())


# ---- inputs ---------------------------------------------------------------------
def ints(rng, shape, lo=-8, hi=8):
    return rng.integers(lo, hi + 1, size=shape).astype(np.float64)


def spd(rng, n):
    G = rng.standard_normal((n, n))
    return G @ G.T + n * np.eye(n)


def diag_dominant(rng, n):
    A = rng.standard_normal((n, n))
    A[np.arange(n), np.arange(n)] = np.abs(A).sum(axis=1) + 1.0
    return A


def exact_lower(rng, n, unit=False):
    """Lower triangle of small integers; diagonal 1 (unit) or a positive
    power of two, so sqrt, reciprocal and division are all exact."""
    L = np.tril(ints(rng, (n, n), -3, 3), -1)
    d = np.ones(n) if unit else 2.0 ** rng.integers(0, 3, size=n)
    return L + np.diag(d)


def exact_upper(rng, n):
    return exact_lower(rng, n).T.copy()


# ---- fp64 emulations in the kernels' operation order ----------------------------
def emu_gemm(A, B, C, nt=False, drop=None, swap=None):
    """Accumulator from zero, k ascending, one subtraction from C.
    drop = (i, j, k): that one product is left out.
    swap = (n, k) (nt only): B[n, k] is read from B[k, n]."""
    Bk = (B.T if nt else B).copy()           # K x N
    if swap is not None:
        n, k = swap
        Bk[k, n] = B[k, n]
    acc = np.zeros(C.shape)
    for k in range(A.shape[1]):
        t = np.outer(A[:, k], Bk[k])
        if drop is not None and drop[2] == k:
            t[drop[0], drop[1]] = 0.0
        acc += t
    return C - acc


def emu_masked_nt(A, B, C, upd):
    out = C.copy()
    e = blocks_to_elements(upd, *C.shape)
    out[e] = emu_gemm(A, B, C, nt=True)[e]
    return out


def emu_potrf32(A):
    S = A.copy()
    n = S.shape[0]
    for c in range(n):
        S[c, c] = np.sqrt(S[c, c])
        inv = 1.0 / S[c, c]
        S[c + 1:, c] *= inv
        upd = np.outer(S[c + 1:, c], S[c + 1:, c])
        low = np.tril(np.ones((n - c - 1, n - c - 1), dtype=bool))
        S[c + 1:, c + 1:][low] -= upd[low]
    return S


def emu_getrf32_nopiv(A):
    S = A.copy()
    n = S.shape[0]
    for c in range(n):
        piv = S[c, c]
        if piv != 0.0:                       # no scaling on a zero pivot
            S[c + 1:, c] *= 1.0 / piv
        S[c + 1:, c + 1:] -= np.outer(S[c + 1:, c], S[c, c + 1:])
    return S


def emu_trsm32(T, X, trans, skip_rows=()):
    """X <- X U^-1 (or X L^-T), one row at a time, true division.
    skip_rows: rows left as they came in."""
    sU = T.T if trans else T
    out = X.copy()
    nb = T.shape[0]
    for c in range(nb):
        acc = out[:, c].copy()
        for i in range(c):
            acc -= out[:, i] * sU[i, c]
        out[:, c] = acc / sU[c, c]
    for r in skip_rows:
        out[r] = X[r]
    return out


def emu_potrf_tile(T, NB=32):
    S = T.copy()
    v = S.shape[0]
    for jb in range(0, v, NB):
        nb = min(NB, v - jb)
        e = jb + nb
        S[jb:e, jb:e] = emu_potrf32(S[jb:e, jb:e])
        if e < v:
            S[e:, jb:e] = emu_trsm32(S[jb:e, jb:e], S[e:, jb:e], 1)
            S[e:, e:] = emu_gemm(S[e:, jb:e], S[e:, jb:e], S[e:, e:], nt=True)
    return S
