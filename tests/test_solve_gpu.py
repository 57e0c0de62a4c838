"""GPU tests of the multi-RHS solve (conflux_lu_solve / conflux_chol_solve):
the two new kernels against scipy/numpy, then the end-to-end solves against
numpy.linalg.solve by normwise backward error.

All tests run on ONE MI355X; multi-rank grids use the engine's
single-process simulation mode (rank=-1).
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import gen_matrix  # noqa: E402

EARG = -1


@pytest.fixture(scope="module")
def eng():
    import conflux_amd
    return conflux_amd


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


# ---------------- kernel: general left triangular solve ---------------------

TRSM_V = [8, 32, 48, 64, 96, 512]   # ragged single block, exactly one block,
                                    # ragged tail, one update, both LDS
                                    # buffers, the bench tile
TRSM_N = [1, 127, 129, 700]


@pytest.mark.parametrize("v", TRSM_V)
@pytest.mark.parametrize("unit", [0, 1])
@pytest.mark.parametrize("upper", [0, 1])
def test_trsm_left_tri(eng, upper, unit, v):
    """k_trsm_left_tri_mfma vs scipy.linalg.solve_triangular, max abs error
    < 1e-12 (the bar of test_trsm_left_lower_unit).  The half of T the solve
    must not read — and the ldt padding columns — hold NaN.

    The unit cases use the SAME triangle with its diagonal scaled out of
    each row (strict triangle of (tri(R) + 5I) / diag, plus I), so both
    kinds pose equally conditioned systems and an absolute bar means the
    same thing for both.  An unscaled strict U[0,1) triangle plus I is
    exponentially ill-conditioned in v: at v = 512 its solutions reach 6e11
    and scipy and a 32-blocked numpy substitution differ by 1e-3 on the
    host, so no absolute fp64 bar holds there for any algorithm; with the
    scaled triangle the same two host algorithms agree to 1.2e-14."""
    import scipy.linalg as la
    rng = np.random.default_rng(100 * v + 2 * upper + unit)
    R = rng.random((v, v))
    tri = np.triu if upper else np.tril
    T = tri(R) + 5.0 * np.eye(v)
    if unit:
        T = T / np.diag(T)[:, None]
        assert (np.diag(T) == 1.0).all()
    keep = tri(np.ones((v, v), dtype=bool))
    worst = 0.0
    for N in TRSM_N:
        X = rng.standard_normal((v, N))
        ref = la.solve_triangular(T, X, lower=not upper,
                                  unit_diagonal=bool(unit))
        for ldt in (v, v + 24):
            Td = np.full((v, ldt), np.nan)
            Td[:, :v] = np.where(keep, T, np.nan)
            if unit:  # in F the unit triangle's diagonal holds U
                np.fill_diagonal(Td, np.nan)
            X1 = X.copy()
            rc = eng.lib().conflux_lu_debug_trsm_left(
                upper, unit, v, N, ldt, _p(Td), _p(X1))
            assert rc == 0
            assert np.isfinite(X1).all(), \
                f"NaN leaked from the unused half: N={N} ldt={ldt}"
            err = np.abs(X1 - ref).max()
            print(f"trsm upper={upper} unit={unit} v={v} N={N} ldt={ldt}: "
                  f"err={err:.3g} max|X|={np.abs(ref).max():.3g}")
            worst = max(worst, err)
    assert worst < 1e-12, f"upper={upper} unit={unit} v={v}: err={worst}"


# ---------------- kernel: skinny update -------------------------------------

@pytest.mark.parametrize("K", [8, 32, 48, 512])
@pytest.mark.parametrize("nrhs", [1, 3, 16])
def test_update_skinny(eng, nrhs, K):
    """k_update_skinny vs numpy C - A@B, relative max error < 1e-13 (the bar
    of test_dgemm_numerics).  lda > K pads A's rows with NaN: the kernel must
    not read past column K."""
    rng = np.random.default_rng(1000 * K + nrhs)
    for M in (1, 15, 17, 300):
        A = rng.standard_normal((M, K))
        B = rng.standard_normal((K, nrhs))
        C = rng.standard_normal((M, nrhs))
        ref = C - A @ B
        for lda in (K, K + 40):
            Ad = np.full((M, lda), np.nan)
            Ad[:, :K] = A
            C1 = C.copy()
            rc = eng.lib().conflux_lu_debug_update_skinny(
                M, nrhs, K, lda, _p(Ad), _p(B), _p(C1))
            assert rc == 0
            err = np.abs(C1 - ref).max() / (np.abs(ref).max() + 1)
            assert err < 1e-13, \
                f"skinny M={M} nrhs={nrhs} K={K} lda={lda}: err={err}"


@pytest.mark.parametrize("nrhs", [3, 16])
def test_update_skinny_transpose_detecting(eng, nrhs):
    # asymmetric A and B catch a row/col swap in the MFMA C layout or a
    # k-permutation that A and B disagree on
    M, K = 64, 80
    A = np.arange(M * K, dtype=np.float64).reshape(M, K) / 100
    B = (np.arange(K * nrhs, dtype=np.float64).reshape(K, nrhs) ** 1.5) / 1000
    C1 = np.zeros((M, nrhs))
    assert eng.lib().conflux_lu_debug_update_skinny(
        M, nrhs, K, K, _p(A), _p(B), _p(C1)) == 0
    assert np.allclose(C1, -A @ B, atol=1e-10)


def test_update_skinny_rejects_wide(eng):
    a = np.zeros((16, 16))
    b = np.zeros((16, 17))
    c = np.zeros((16, 17))
    assert eng.lib().conflux_lu_debug_update_skinny(
        16, 17, 16, 16, _p(a), _p(b), _p(c)) == EARG


# ---------------- end-to-end ------------------------------------------------

def _eta(A, X, B):
    """Normwise backward error ||B - A X||_F / (||A||_F ||X||_F + ||B||_F);
    independent of cond(A)."""
    return np.linalg.norm(B - A @ X) / (
        np.linalg.norm(A) * np.linalg.norm(X) + np.linalg.norm(B))


def _check_eta(A, X, B, tag):
    eta = _eta(A, X, B)
    eta_np = _eta(A, np.linalg.solve(A, B), B)
    print(f"{tag}: eta={eta:.3g} eta_numpy={eta_np:.3g} "
          f"ratio={eta / eta_np:.2f}")
    assert eta <= 10 * eta_np, f"{tag}: eta={eta} vs numpy {eta_np}"


def _spd(N):
    G = gen_matrix(N)
    return 0.5 * (G + G.T) + 2.0 * N * np.eye(N)


NRHS = [1, 3, 17, 130]   # skinny VALU-sized, skinny, just past the skinny
                         # kernel's 16, more than one 128-column TRSM block

LU_GRIDS = [
    (64, 8, 1, 1, 1),
    (128, 16, 1, 1, 2),
    (256, 32, 2, 2, 1),
    (512, 64, 1, 1, 1),
    (512, 32, 8, 8, 1),
    (1024, 128, 1, 1, 1),
]


@pytest.mark.parametrize("N,v,Px,Py,Pz", LU_GRIDS)
def test_lu_solve(eng, N, v, Px, Py, Pz):
    A = gen_matrix(N)
    rng = np.random.default_rng(N + v)
    with eng.Engine(N, v, Px, Py, Pz, rank=-1) as e:
        e.store_factors(True)
        e.set_matrix_global(A)
        e.factor()
        for nrhs in NRHS:
            B = rng.standard_normal((N, nrhs))
            X = e.solve(B)
            assert X.shape == B.shape
            _check_eta(A, X, B, f"lu {N},{v},{Px}x{Py}x{Pz} nrhs={nrhs}")


def test_solve_tile_larger_than_sweep_block(eng):
    """v = 256 > 128: the sweeps run on 128-row blocks inside each
    factorization tile (every grid above has v <= 128 and sweeps whole
    tiles)."""
    N, v = 1024, 256
    rng = np.random.default_rng(9)
    A = gen_matrix(N)
    with eng.Engine(N, v, 1, 1, 1, rank=-1) as e:
        e.store_factors(True)
        e.set_matrix_global(A)
        e.factor()
        for nrhs in (1, 17, 130):
            B = rng.standard_normal((N, nrhs))
            _check_eta(A, e.solve(B), B, f"lu 1024,256 nrhs={nrhs}")
    S = _spd(N)
    with eng.Engine(N, v, 2, 2, 1, rank=-1) as e:
        e.store_factors(True)
        e.set_matrix_global(S)
        e.factor_cholesky()
        B = rng.standard_normal((N, 17))
        _check_eta(S, e.solve_cholesky(B), B, "chol 1024,256,2x2x1 nrhs=17")


def test_lu_solve_real_single_rank(eng):
    """rank=0, world=1 (not the simulation): Fres is read in place."""
    N, v = 512, 64
    A = gen_matrix(N)
    rng = np.random.default_rng(5)
    with eng.Engine(N, v, 1, 1, 1, rank=0, world=1) as e:
        e.store_factors(True)
        e.set_matrix_local(A)
        e.factor()
        F0 = e.get_F_local().copy()
        for nrhs in NRHS:
            B = rng.standard_normal((N, nrhs))
            _check_eta(A, e.solve(B), B, f"lu real 512,64 nrhs={nrhs}")
        assert np.array_equal(F0, e.get_F_local()), "solve wrote into Fres"


def test_lu_solve_conventions(eng):
    """1-D round trip, argument untouched, factors not mutated."""
    N, v = 256, 32
    A = gen_matrix(N)
    rng = np.random.default_rng(6)
    with eng.Engine(N, v, 2, 2, 1, rank=-1) as e:
        e.store_factors(True)
        e.set_matrix_global(A)
        e.factor()
        F0 = e.get_F_global().copy()
        b = rng.standard_normal(N)
        b0 = b.copy()
        x = e.solve(b)
        assert x.shape == (N,) and x is not b
        assert np.array_equal(b, b0), "caller's B was modified"
        _check_eta(A, x, b, "lu 1-D")
        x2d = e.solve(b.reshape(N, 1))
        assert x2d.shape == (N, 1)
        assert np.array_equal(x2d[:, 0], x)
        B = rng.standard_normal((N, 17))
        B0 = B.copy()
        X1 = e.solve(B)
        X2, ms = e.solve(B, return_ms=True)
        assert np.array_equal(B, B0)
        assert np.array_equal(X1, X2), "second solve differs: factors mutated"
        assert ms > 0
        assert np.array_equal(F0, e.get_F_global()), "solve wrote into Fres"


def test_lu_solve_padded(eng):
    """N = 1000 rounds up to 1024: B carries Npad rows and A is extended
    with the same nonsingular random fill."""
    with eng.Engine(1000, 128, 1, 1, 1, rank=-1) as e:
        assert e.Npad == 1024
        A = gen_matrix(e.Npad)
        B = np.random.default_rng(7).standard_normal((e.Npad, 3))
        e.store_factors(True)
        e.set_matrix_global(A)
        e.factor()
        _check_eta(A, e.solve(B), B, "lu padded 1000->1024")
        with pytest.raises(ValueError):
            e.solve(B[:1000])


def test_lu_solve_nopivot(eng):
    N, v = 256, 64
    A = gen_matrix(N)
    S = 0.5 * (A + A.T) + 2.0 * N * np.eye(N)  # == init_matrix_spd fill
    rng = np.random.default_rng(8)
    with eng.Engine(N, v, 2, 2, 1, rank=-1) as e:
        e.store_factors(True)
        e.set_pivoting(0)
        e.set_matrix_global(S)
        e.factor()
        for nrhs in (1, 17):
            B = rng.standard_normal((N, nrhs))
            _check_eta(S, e.solve(B), B, f"lu nopiv nrhs={nrhs}")


@pytest.mark.parametrize("N,v,Px,Py,Pz", [(256, 64, 1, 1, 1),
                                          (512, 64, 2, 2, 1),
                                          (128, 16, 1, 1, 2)])
def test_chol_solve(eng, N, v, Px, Py, Pz):
    A = _spd(N)
    rng = np.random.default_rng(N + v + 1)
    with eng.Engine(N, v, Px, Py, Pz, rank=-1) as e:
        e.store_factors(True)
        e.set_matrix_global(A)
        e.factor_cholesky()
        F0 = e.get_F_global().copy()
        for nrhs in (1, 17):
            B = rng.standard_normal((N, nrhs))
            X = e.solve_cholesky(B)
            _check_eta(A, X, B, f"chol {N},{v},{Px}x{Py}x{Pz} nrhs={nrhs}")
        assert np.array_equal(F0, e.get_F_global()), "solve wrote into Fres"


# ---------------- guards ----------------------------------------------------

def test_solve_guards(eng):
    lib = eng.lib()
    N, v = 64, 8
    B = np.ones((N, 2))
    ms = ctypes.c_double()
    with eng.Engine(N, v, 1, 1, 1, rank=-1) as e:
        e.set_matrix_global(gen_matrix(N))
        # before any factorization
        assert lib.conflux_lu_solve(e._h, _p(B), 2, ctypes.byref(ms)) == EARG
        assert lib.conflux_chol_solve(e._h, _p(B), 2, None) == EARG
        # last factorization ran with store_factors off
        e.store_factors(False)
        e.factor()
        assert lib.conflux_lu_solve(e._h, _p(B), 2, None) == EARG
        e.store_factors(True)
        e.factor()
        assert lib.conflux_lu_solve(e._h, _p(B), 0, None) == EARG
        assert lib.conflux_lu_solve(e._h, _p(B), -1, None) == EARG
        assert lib.conflux_lu_solve(e._h, None, 2, None) == EARG
        # kind mismatch
        assert lib.conflux_chol_solve(e._h, _p(B), 2, None) == EARG
        with pytest.raises(eng.ConfluxLuError):
            e.solve_cholesky(B)
        # the guards left the engine usable; elapsed_ms may be NULL
        assert np.array_equal(B, np.ones((N, 2)))
        assert lib.conflux_lu_solve(e._h, _p(B.copy()), 2, None) == 0
        # a store_factors-off run invalidates the earlier factors
        e.store_factors(False)
        e.factor()
        assert lib.conflux_lu_solve(e._h, _p(B), 2, None) == EARG
    with eng.Engine(N, v, 1, 1, 1, rank=-1) as e:
        e.store_factors(True)
        e.set_matrix_global(_spd(N))
        e.factor_cholesky()
        assert lib.conflux_lu_solve(e._h, _p(B), 2, None) == EARG
        assert lib.conflux_chol_solve(e._h, None, 2, None) == EARG
        assert lib.conflux_chol_solve(e._h, _p(B), 0, None) == EARG
        assert lib.conflux_chol_solve(e._h, _p(B.copy()), 2, None) == 0
