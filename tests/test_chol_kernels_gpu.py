"""The Cholesky / no-pivot kernel family, one launcher at a time, against the
longdouble references and derived elementwise bounds of tests/_hp_ref.py:
k_dgemm_mfma<GemmW8NT> with and without the TriMask, k_potrf32,
k_getrf32_nopiv, k_trsm_right_upper32 and the blocked potrf_tile chain.
Operands sit in canvases of NaN canaries, and every kernel also runs a case
built from exactly representable factors whose result must match bit for
bit."""
import ctypes

import numpy as np
import pytest

import _hp_ref as hp

pytestmark = pytest.mark.gpu


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def lib():
    import conflux_amd
    return conflux_amd.lib()


def _show(kernel, what, r):
    print(f"RATIO {kernel} {what} {r:.3f}")
    return r


# ---- NT GEMM ------------------------------------------------------------------
def run_nt(lib, A, B, C, pad, mask=(0, 0, 0, 1, 1, 0, 0), alias=False):
    M, K = A.shape
    N = B.shape[0]
    lda, ldb, ldc, crows = (K + 3, K + 5, N + 7, M + 2) if pad else (K, K, N, M)
    if alias:
        ldb = lda
    fA = hp.framed(A, max(M, N) if alias else M, lda)
    fB = fA if alias else hp.framed(B, N, ldb)
    fC = hp.framed(C, crows, ldc)
    rc = lib.conflux_lu_debug_dgemm_nt(M, N, K, lda, ldb, ldc, crows, _ptr(fA),
                                       _ptr(fB), _ptr(fC), *mask)
    assert rc == 0
    assert hp.frame_intact(fC, M, N), "wrote outside the M x N window of C"
    return fC[:M, :N].copy()


@pytest.mark.parametrize("pad", [0, 1])
@pytest.mark.parametrize("M,N,K", [(1, 1, 1), (129, 257, 17), (300, 130, 8)])
def test_gemm_nt(lib, M, N, K, pad):
    rng = np.random.default_rng([M, N, K])
    A, B, C = (rng.standard_normal(s) for s in ((M, K), (N, K), (M, N)))
    got = run_nt(lib, A, B, C, pad)
    assert _show("gemm_nt", f"{M}x{N}x{K}",
                 hp.gemm_ratio(got, A, B, C, nt=True)) <= 1.0
    A, B, C = (hp.ints(rng, s) for s in ((M, K), (N, K), (M, N)))
    assert hp.bits_equal(run_nt(lib, A, B, C, pad),
                         hp.gemm_exact(A, B, C, nt=True))


@pytest.mark.parametrize("pad", [0, 1])
def test_gemm_nt_aliased(lib, pad):
    """A and B one buffer, as in potrf_tile: C -= A A^T."""
    rng = np.random.default_rng(64)
    A, C = rng.standard_normal((64, 32)), rng.standard_normal((64, 64))
    got = run_nt(lib, A, A, C, pad, alias=True)
    assert _show("gemm_nt", "64x64x32 aliased",
                 hp.gemm_ratio(got, A, A, C, nt=True)) <= 1.0
    A, C = hp.ints(rng, (64, 32)), hp.ints(rng, (64, 64))
    assert hp.bits_equal(run_nt(lib, A, A, C, pad, alias=True),
                         hp.gemm_exact(A, A, C, nt=True))


GRIDS = [(1, 1, 0, 0), (2, 2, 0, 1), (2, 2, 1, 0), (2, 2, 1, 1), (4, 4, 3, 0)]
MASKS = [(128, 384, 512, 64, r0, c0, g) for r0 in (0, 128) for c0 in (0, 256)
         for g in GRIDS] + [(256, 512, 512, 128, 0, 0, (2, 2, 1, 0))]
# the one set of the list that the rule puts wholly above the tile diagonal
# (global tile rows 0, 2, 4 against tile columns 5, 7, 9, 11): the launch may
# write nothing at all
ALL_MASKED = (128, 384, 512, 64, 0, 256, (2, 2, 0, 1))

_MASK_INPUTS = {}


def mask_inputs(M, N, K, exact):
    key = (M, N, K, exact)
    if key not in _MASK_INPUTS:
        rng = np.random.default_rng([M, N, K, int(exact)])
        shapes = ((M, K), (N, K), (M, N))
        ABC = tuple(hp.ints(rng, s) if exact else rng.standard_normal(s)
                    for s in shapes)
        ref, bound = hp.gemm_ref(*ABC, nt=True)
        for x in ABC + (ref, bound):
            x.setflags(write=False)
        _MASK_INPUTS[key] = ABC + (ref, bound)
    return _MASK_INPUTS[key]


@pytest.mark.parametrize("v,M,N,K,r0off,c0off,grid", MASKS)
def test_gemm_nt_masked(lib, v, M, N, K, r0off, c0off, grid):
    """The TriMask rule restated in numpy decides, 128 x 128 block by block,
    what is updated (held to the GEMM bound) and what must keep its bits."""
    upd = hp.tri_mask(M, N, v, r0off, c0off, *grid)
    assert not upd.all()
    assert upd.any() != ((v, M, N, K, r0off, c0off, grid) == ALL_MASKED)
    e = hp.blocks_to_elements(upd, M, N)
    mask = (v, r0off, c0off) + grid
    A, B, C, ref, bound = mask_inputs(M, N, K, False)
    got = run_nt(lib, A, B, C, 1, mask)
    assert hp.bits_equal(got[~e], C[~e]), "a masked block was written"
    err = np.abs(got.astype(hp.LD) - ref)
    assert _show("gemm_nt_tril", f"v={v} {r0off},{c0off} {grid}",
                 hp.worst_ratio(err[e], bound[e])) <= 1.0
    A, B, C, ref, _ = mask_inputs(M, N, K, True)
    want = np.where(e, ref.astype(np.float64), C)
    assert hp.bits_equal(run_nt(lib, A, B, C, 0, mask), want)


@pytest.mark.parametrize("bad", [
    dict(v=64), dict(v=-128), dict(M=320), dict(N=192), dict(r0off=64),
    dict(c0off=-128), dict(pi=2), dict(pj=-1), dict(Px=0), dict(lda=63),
    dict(ldb=63), dict(ldc=511), dict(c_rows=383), dict(K=0),
])
def test_gemm_nt_bad_arguments_are_refused(lib, bad):
    a = dict(M=384, N=512, K=64, lda=64, ldb=64, ldc=512, c_rows=384, v=128,
             r0off=0, c0off=0, Px=2, Py=2, pi=1, pj=0)
    a.update(bad)
    A, B, C = hp.canvas(384, 64), hp.canvas(512, 64), hp.canvas(384, 512)
    rc = lib.conflux_lu_debug_dgemm_nt(
        a["M"], a["N"], a["K"], a["lda"], a["ldb"], a["ldc"], a["c_rows"],
        _ptr(A), _ptr(B), _ptr(C), a["v"], a["r0off"], a["c0off"], a["Px"],
        a["Py"], a["pi"], a["pj"])
    assert rc == -1
    assert hp.frame_intact(C, 0, 0)


# ---- 32-wide micro-factors ------------------------------------------------------
def run_factor32(fn, A, lda):
    nb = A.shape[0]
    f = hp.framed(A, nb + 2, lda)
    assert fn(nb, lda, nb + 2, _ptr(f)) == 0
    assert hp.frame_intact(f, nb, nb), "wrote outside the nb x nb block"
    return f[:nb, :nb].copy()


@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("nb", [1, 7, 16, 31, 32])
def test_potrf32(lib, nb, pad):
    rng = np.random.default_rng([1, nb])
    A = hp.spd(rng, nb)
    F = run_factor32(lib.conflux_lu_debug_potrf32, A, nb + pad)
    assert hp.bits_equal(np.triu(F, 1), np.triu(A, 1)), \
        "the strict upper triangle changed"
    assert _show("potrf32", f"nb={nb}", hp.potrf_ratio(A, F)) <= 1.0
    L0 = hp.exact_lower(rng, nb)
    F = run_factor32(lib.conflux_lu_debug_potrf32, L0 @ L0.T, nb + pad)
    assert hp.bits_equal(np.tril(F), L0)


@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("nb", [1, 7, 16, 31, 32])
def test_getrf32_nopiv(lib, nb, pad):
    rng = np.random.default_rng([2, nb])
    A = hp.diag_dominant(rng, nb)
    F = run_factor32(lib.conflux_lu_debug_getrf32_nopiv, A, nb + pad)
    assert _show("getrf32_nopiv", f"nb={nb}", hp.getrf_ratio(A, F)) <= 1.0
    L0, U0 = hp.exact_lower(rng, nb, unit=True), hp.exact_upper(rng, nb)
    F = run_factor32(lib.conflux_lu_debug_getrf32_nopiv, L0 @ U0, nb + pad)
    assert hp.bits_equal(F, np.tril(L0, -1) + U0)


@pytest.mark.parametrize("nb", [7, 32])
def test_getrf32_nopiv_zero_pivot(lib, nb):
    """A first column that is exactly zero: no scaling on the zero pivot, the
    factorization goes on.  The rest of the input is a product of exactly
    representable factors, so the emulation's bits are the only right answer
    whether or not the compiler fuses the multiply-adds; a random input with
    the same zero column must stay finite and inside the bound."""
    rng = np.random.default_rng([3, nb])
    L0 = hp.exact_lower(rng, nb - 1, unit=True)
    U0 = hp.exact_upper(rng, nb - 1)
    A = np.zeros((nb, nb))
    A[0, 1:] = hp.ints(rng, nb - 1)
    A[1:, 1:] = L0 @ U0
    F = run_factor32(lib.conflux_lu_debug_getrf32_nopiv, A, nb + 5)
    assert np.isfinite(F).all()
    assert hp.bits_equal(F, hp.emu_getrf32_nopiv(A))
    A = hp.diag_dominant(rng, nb)
    A[:, 0] = 0.0
    F = run_factor32(lib.conflux_lu_debug_getrf32_nopiv, A, nb)
    assert np.isfinite(F).all() and hp.bits_equal(F[:, 0], A[:, 0])
    assert _show("getrf32_nopiv", f"nb={nb} zero pivot",
                 hp.getrf_ratio(A, F)) <= 1.0


@pytest.mark.parametrize("bad", [dict(nb=0), dict(nb=33), dict(lda=15),
                                 dict(rows=15)])
@pytest.mark.parametrize("name", ["conflux_lu_debug_potrf32",
                                  "conflux_lu_debug_getrf32_nopiv"])
def test_factor32_bad_arguments_are_refused(lib, name, bad):
    a = dict(nb=16, lda=16, rows=16)
    a.update(bad)
    A = hp.canvas(40, 40)
    assert getattr(lib, name)(a["nb"], a["lda"], a["rows"], _ptr(A)) == -1
    assert hp.frame_intact(A, 0, 0)


# ---- 32-wide right solve -----------------------------------------------------------
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("M", [1, 255, 256, 257, 700])
@pytest.mark.parametrize("nb", [1, 7, 32])
@pytest.mark.parametrize("trans", [0, 1])
def test_trsm32(lib, trans, nb, M, pad):
    rng = np.random.default_rng([4, trans, nb, M])
    ldu, ldx = nb + pad, nb + pad

    def solve(T, X):
        fT, fX = hp.framed(T, nb, ldu), hp.framed(X, M + 1, ldx)
        assert lib.conflux_lu_debug_trsm32(trans, nb, M, ldu, ldx, _ptr(fT),
                                           _ptr(fX)) == 0
        assert hp.frame_intact(fX, M, nb), "wrote outside the M x nb window"
        return fX[:M, :nb].copy()

    # both triangles full and different: the kernel must use only its own
    T = rng.standard_normal((nb, nb)) + nb * np.eye(nb)
    X = rng.standard_normal((M, nb))
    assert _show("trsm32", f"trans={trans} nb={nb} M={M}",
                 hp.trsm_ratio(X, solve(T, X), T, trans)) <= 1.0
    T0 = hp.exact_lower(rng, nb) if trans else hp.exact_upper(rng, nb)
    X0 = hp.ints(rng, (M, nb))
    assert hp.bits_equal(solve(T0, X0 @ (T0.T if trans else T0)), X0)


@pytest.mark.parametrize("bad", [dict(trans=2), dict(nb=0), dict(nb=33),
                                 dict(M=0), dict(ldu=15), dict(ldx=15)])
def test_trsm32_bad_arguments_are_refused(lib, bad):
    a = dict(trans=0, nb=16, M=64, ldu=16, ldx=16)
    a.update(bad)
    T, X = hp.canvas(40, 40), hp.canvas(64, 40)
    assert lib.conflux_lu_debug_trsm32(a["trans"], a["nb"], a["M"], a["ldu"],
                                       a["ldx"], _ptr(T), _ptr(X)) == -1
    assert hp.frame_intact(X, 0, 0)


# ---- blocked tile factorization --------------------------------------------------
@pytest.mark.parametrize("pad", [0, 4])
@pytest.mark.parametrize("v", [8, 32, 48, 96, 128])
def test_potrf_tile(lib, v, pad):
    """v = 48 is the 32 + 16 chain (a ragged last block) that no grid of the
    whole-factorization tests reaches."""
    rng = np.random.default_rng([5, v])

    def factor(A):
        f = hp.framed(A, v + 2, v + pad)
        assert lib.conflux_lu_debug_potrf_tile(v, v + pad, v + 2, _ptr(f)) == 0
        assert hp.frame_intact(f, v, v), "wrote outside the v x v window"
        return f[:v, :v].copy()

    A = hp.spd(rng, v)
    assert _show("potrf_tile", f"v={v}",
                 hp.potrf_ratio(A, factor(A), width=v)) <= 1.0
    L0 = hp.exact_lower(rng, v)
    assert hp.bits_equal(np.tril(factor(L0 @ L0.T)), L0)


@pytest.mark.parametrize("bad", [dict(v=0), dict(ld=31), dict(rows=31)])
def test_potrf_tile_bad_arguments_are_refused(lib, bad):
    a = dict(v=32, ld=32, rows=32)
    a.update(bad)
    T = hp.canvas(40, 40)
    assert lib.conflux_lu_debug_potrf_tile(a["v"], a["ld"], a["rows"],
                                           _ptr(T)) == -1
    assert hp.frame_intact(T, 0, 0)
