"""GPU tests of the refined solves (conflux_lu_solve_refined /
conflux_chol_solve_refined): the doubled-precision residual kernel against the
exactly rounded residual, then the refinement loop end to end — exact recovery
on ill-conditioned integer systems, the no-pivot fast path rescued, the
reported error figures, contracts and guards.

All tests run on ONE MI355X; multi-rank grids use the engine's
single-process simulation mode (rank=-1).
"""
import ctypes
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import gen_matrix  # noqa: E402

EARG = -1
U = 2.0 ** -53
GRIDS = [(1, 1, 1), (2, 2, 1)]


@pytest.fixture(scope="module")
def eng():
    import conflux_amd
    return conflux_amd


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


# ---------------- kernel: doubled-precision residual ------------------------

def _two_prod(a, x):
    """Dekker/Veltkamp: p + e == a * x exactly (no FMA needed)."""
    p = a * x
    c = 134217729.0  # 2^27 + 1
    t = c * a
    ah = t - (t - a)
    al = a - ah
    t = c * x
    xh = t - (t - x)
    xl = x - xh
    e = ((ah * xh - p) + ah * xl + al * xh) + al * xl
    return p, e


def _exact_residual(A, X, B):
    """fl(B - A X): every product split into p + e exactly, then one
    correctly rounded sum (math.fsum) per entry."""
    M, n = A.shape[0], X.shape[1]
    R = np.empty((M, n))
    for j in range(n):
        p, e = _two_prod(A, X[:, j][None, :])
        T = np.concatenate([B[:, j:j + 1], -p, -e], axis=1)
        for i in range(M):
            R[i, j] = math.fsum(T[i])
    return R


def _residual_bar(A, X, B, Rex):
    K = A.shape[1]
    return 2 * U * np.abs(Rex) + \
        2 * (K + 2) ** 2 * U * U * (np.abs(A) @ np.abs(X) + np.abs(B))


def _gpu_residual(eng, A, X, B, lda):
    M, K = A.shape
    nrhs = X.shape[1]
    Ad = np.full((M, lda), np.nan)  # padding columns must never be read
    Ad[:, :K] = A
    R = np.full((M, nrhs), np.nan)
    rc = eng.lib().conflux_lu_debug_residual_dd(
        M, K, nrhs, lda, _p(Ad), _p(np.ascontiguousarray(X)),
        _p(np.ascontiguousarray(B)), _p(R))
    assert rc == 0
    return R


def _group_width(eng):
    return eng.lib().conflux_lu_debug_residual_group_width()


RES_M = [1, 15, 17, 300]
RES_K = [1, 63, 64, 65, 1000]
RES_NRHS = ["1", "3", "G", "G+1", "17"]  # G = the kernel's column group


@pytest.mark.parametrize("nrhs_tag", RES_NRHS)
@pytest.mark.parametrize("K", RES_K)
def test_residual_dd_exact(eng, K, nrhs_tag):
    """k_residual_dd vs the exactly rounded residual, elementwise
        |R - R_exact| <= 2u|R_exact| + 2(K+2)^2 u^2 (|A||X| + |B|).
    B = fl(A X), so the true residual is pure rounding error and a
    working-precision B - A@X has no correct digit: at K = 1000 numpy's own
    misses the bar on more than half the entries (asserted).  One reference
    at M = 300 serves every M (rows are independent)."""
    G = _group_width(eng)
    assert G >= 1
    nrhs = {"G": G, "G+1": G + 1}.get(nrhs_tag) or int(nrhs_tag)
    rng = np.random.default_rng(1000 * K + nrhs)
    A = rng.standard_normal((max(RES_M), K))
    X = rng.standard_normal((K, nrhs))
    B = A @ X
    Rex = _exact_residual(A, X, B)
    bar = _residual_bar(A, X, B, Rex)
    if K == 1000:
        miss = np.abs((B - A @ X) - Rex) > bar
        print(f"numpy residual misses the bar on {miss.mean():.0%}")
        assert miss.mean() > 0.5
    for M in RES_M:
        for lda in (K, K + 3):
            R = _gpu_residual(eng, A[:M], X, B[:M], lda)
            assert np.isfinite(R).all(), \
                f"NaN leaked from the padding: M={M} K={K} lda={lda}"
            excess = (np.abs(R - Rex[:M]) / bar[:M]).max()
            print(f"resid M={M} K={K} nrhs={nrhs} lda={lda}: "
                  f"max err/bar={excess:.3g}")
            assert (np.abs(R - Rex[:M]) <= bar[:M]).all(), \
                f"M={M} K={K} nrhs={nrhs} lda={lda}: err/bar={excess}"


@pytest.mark.parametrize("nrhs", [3, 17])
def test_residual_dd_transpose_detecting(eng, nrhs):
    # asymmetric A, X and B catch a row/col swap, a k-permutation that A and
    # X disagree on, or columns landing in the wrong group
    M, K = 70, 200
    A = np.arange(M * K, dtype=np.float64).reshape(M, K) / 100
    X = (np.arange(K * nrhs, dtype=np.float64).reshape(K, nrhs) ** 1.5) / 1000
    B = np.sqrt(np.arange(M * nrhs, dtype=np.float64).reshape(M, nrhs))
    Rex = _exact_residual(A, X, B)
    R = _gpu_residual(eng, A, X, B, K)
    assert (np.abs(R - Rex) <= _residual_bar(A, X, B, Rex)).all()


def test_residual_dd_guards(eng):
    lib = eng.lib()
    a = np.zeros((4, 4))
    x = np.zeros((4, 2))
    b = np.zeros((4, 2))
    r = np.zeros((4, 2))
    ok = (4, 4, 2, 4, _p(a), _p(x), _p(b), _p(r))
    assert lib.conflux_lu_debug_residual_dd(*ok) == 0
    for i, bad in ((0, 0), (1, 0), (2, 0), (3, 3), (4, None), (5, None),
                   (6, None), (7, None)):
        args = list(ok)
        args[i] = bad
        assert lib.conflux_lu_debug_residual_dd(*args) == EARG, i


# ---------------- exact recovery on ill-conditioned integer systems ---------

def _int_system(N, dens, seed, nrhs):
    """A = P L U with small integer factors: exactly representable, cond
    ~1e7, integer solution."""
    rng = np.random.default_rng(seed)
    L = np.tril(rng.integers(-1, 2, (N, N)) * (rng.random((N, N)) < dens),
                -1) + np.eye(N, dtype=np.int64)
    Uf = np.triu(rng.integers(-1, 2, (N, N)) * (rng.random((N, N)) < dens),
                 1) + np.diag(rng.choice([-1, 1], N))
    A = (L.astype(np.int64) @ Uf.astype(np.int64))[rng.permutation(N)]
    Xt = np.random.default_rng(50 + seed).integers(-1000, 1001, (N, nrhs))
    B = A @ Xt
    assert np.abs(A).max() < 2 ** 30 and np.abs(B).max() < 2 ** 53
    return A.astype(np.float64), Xt.astype(np.float64), B.astype(np.float64)


@pytest.mark.parametrize("Px,Py,Pz", GRIDS)
@pytest.mark.parametrize("N,dens", [(128, 0.15), (256, 0.08)])
def test_refine_recovers_integer_solution_exactly(eng, N, dens, Px, Py, Pz):
    """cond(A) ~ 1e7: the plain solve loses 6-7 digits (asserted: the case is
    hard); refinement with the exact residual returns X == Xt bit for bit."""
    with eng.Engine(N, 32, Px, Py, Pz, rank=-1) as e:
        e.store_factors(True)
        A = _int_system(N, dens, 0, 1)[0]
        e.set_matrix_global(A)
        e.factor()
        for nrhs in (1, 3):
            A, Xt, B = _int_system(N, dens, 0, nrhs)
            X0 = e.solve_refined(B, max_iter=0)
            f0 = np.abs(X0 - Xt).max() / np.abs(Xt).max()
            X, info = e.solve_refined(B, max_iter=10, return_info=True)
            print(f"int N={N} {Px}x{Py}x{Pz} nrhs={nrhs}: plain ferr={f0:.3g} "
                  f"refined maxdiff={np.abs(X - Xt).max():.3g} {info}")
            assert f0 >= 1e-12
            assert np.array_equal(X, Xt)
            assert (info["berr"] == 0.0).all()
            assert info["iters"] <= 4


# ---------------- the no-pivot path is rescued ------------------------------

def _berr_host(A, X, B):
    """The engine's berr formula with an np.longdouble residual."""
    Al, Xl, Bl = (np.asarray(t, dtype=np.longdouble) for t in (A, X, B))
    R = np.abs(Bl - Al @ Xl).max(axis=0)
    den = np.abs(Al).sum(axis=1).max() * np.abs(Xl).max(axis=0) + \
        np.abs(Bl).max(axis=0)
    return np.asarray(R / den, dtype=np.float64)


@pytest.mark.parametrize("Px,Py,Pz", GRIDS)
def test_refine_rescues_nopivot(eng, Px, Py, Pz):
    """Gaussian random A, no pivoting: element growth 1e3-1e4 puts the plain
    solve's backward error at 1e-13..1e-12; refinement brings it below
    numpy.linalg.solve's (partial pivoting).  The reported berr agrees with
    the host's longdouble evaluation of the same formula."""
    N = 256
    A = np.random.default_rng(0).standard_normal((N, N))
    with eng.Engine(N, 32, Px, Py, Pz, rank=-1) as e:
        e.store_factors(True)
        e.set_pivoting(0)
        e.set_matrix_global(A)
        e.factor()
        for nrhs in (1, 17):
            B = np.random.default_rng(nrhs).standard_normal((N, nrhs))
            X0, i0 = e.solve_refined(B, max_iter=0, return_info=True)
            X1, i1 = e.solve_refined(B, max_iter=10, return_info=True)
            b0, b1 = i0["berr"], i1["berr"]
            bnp = _berr_host(A, np.linalg.solve(A, B), B)
            print(f"nopiv {Px}x{Py}x{Pz} nrhs={nrhs}: b0={b0.min():.3g}.."
                  f"{b0.max():.3g} b1={b1.min():.3g}..{b1.max():.3g} "
                  f"numpy={bnp.min():.3g}..{bnp.max():.3g} "
                  f"iters={i1['iters']} ferr={i1['ferr'].max():.3g}")
            assert (b1 <= bnp).all()
            assert (b0 >= 100 * b1).all()
            # reported numbers are true
            for X, b in ((X0, b0), (X1, b1)):
                bh = _berr_host(A, X, B)
                print(f"   engine berr vs host: max |diff|="
                      f"{np.abs(b - bh).max():.3g}")
                assert (np.abs(b - bh) <= 1e-3 * b + (N + 2) * 2.0 ** -64).all()


# ---------------- contracts -------------------------------------------------

def test_refine_contracts(eng):
    N, v = 256, 32
    A = gen_matrix(N)
    rng = np.random.default_rng(6)
    with eng.Engine(N, v, 2, 2, 1, rank=-1) as e:
        e.store_factors(True)
        e.set_matrix_global(A)
        e.factor()
        F0 = e.get_F_global().copy()
        B = rng.standard_normal((N, 17))
        B0 = B.copy()
        # max_iter = 0 is the plain solve, bit for bit
        assert np.array_equal(e.solve_refined(B, max_iter=0), e.solve(B))
        # deterministic
        X1, i1 = e.solve_refined(B, return_info=True)
        X2, i2 = e.solve_refined(B, return_info=True)
        assert np.array_equal(X1, X2)
        assert np.array_equal(i1["berr"], i2["berr"])
        assert np.array_equal(i1["ferr"], i2["ferr"])
        assert i1["iters"] == i2["iters"] and i1["ms"] > 0
        assert np.array_equal(B, B0), "caller's B was modified"
        assert X1.shape == B.shape and X1 is not B
        # well-conditioned pivoted system: done in at most 2 passes, and at
        # least as good as numpy
        bnp = _berr_host(A, np.linalg.solve(A, B), B)
        print(f"contracts: iters={i1['iters']} berr={i1['berr'].max():.3g} "
              f"numpy={bnp.min():.3g}")
        assert i1["iters"] <= 2
        assert (i1["berr"] <= bnp).all()
        assert i1["ferr"].shape == (17,) and (i1["ferr"] >= 0).all()
        # 1-D round trip
        b = rng.standard_normal(N)
        b0 = b.copy()
        x = e.solve_refined(b)
        assert x.shape == (N,) and x is not b and np.array_equal(b, b0)
        x2d, info = e.solve_refined(b.reshape(N, 1), return_info=True)
        assert x2d.shape == (N, 1) and np.array_equal(x2d[:, 0], x)
        assert info["berr"].shape == (1,)
        with pytest.raises(ValueError):
            e.solve_refined(B[:100])
        with pytest.raises(ValueError):
            e.solve_refined(np.zeros((N, 2, 2)))
        assert np.array_equal(F0, e.get_F_global()), "refinement wrote Fres"


def test_refine_real_single_rank(eng):
    """rank=0, world=1 (not the simulation): A11in and Fres read in place."""
    N, v = 512, 64
    A = gen_matrix(N)
    B = np.random.default_rng(5).standard_normal((N, 5))
    with eng.Engine(N, v, 1, 1, 1, rank=0, world=1) as e:
        e.store_factors(True)
        e.set_matrix_local(A)
        e.factor()
        F0 = e.get_F_local().copy()
        X, info = e.solve_refined(B, return_info=True)
        assert (info["berr"] <= _berr_host(A, np.linalg.solve(A, B), B)).all()
        assert np.array_equal(F0, e.get_F_local())


def test_refine_padded(eng):
    """N = 1000 rounds up to 1024, as in test_lu_solve_padded."""
    with eng.Engine(1000, 128, 1, 1, 1, rank=-1) as e:
        assert e.Npad == 1024
        A = gen_matrix(e.Npad)
        B = np.random.default_rng(7).standard_normal((e.Npad, 3))
        e.store_factors(True)
        e.set_matrix_global(A)
        e.factor()
        X, info = e.solve_refined(B, return_info=True)
        assert (info["berr"] <= _berr_host(A, np.linalg.solve(A, B), B)).all()
        assert (np.abs(info["berr"] - _berr_host(A, X, B)) <=
                1e-3 * info["berr"] + (e.Npad + 2) * 2.0 ** -64).all()
        with pytest.raises(ValueError):
            e.solve_refined(B[:1000])


# ---------------- Cholesky --------------------------------------------------

def _spd(N):
    G = gen_matrix(N)
    return 0.5 * (G + G.T) + 2.0 * N * np.eye(N)


@pytest.mark.parametrize("N,v,Px,Py,Pz", [(256, 64, 1, 1, 1),
                                          (512, 64, 2, 2, 1)])
def test_chol_refine(eng, N, v, Px, Py, Pz):
    A = _spd(N)
    rng = np.random.default_rng(N + v + 1)
    with eng.Engine(N, v, Px, Py, Pz, rank=-1) as e:
        e.store_factors(True)
        e.set_matrix_global(A)
        e.factor_cholesky()
        F0 = e.get_F_global().copy()
        for nrhs in (1, 17):
            B = rng.standard_normal((N, nrhs))
            assert np.array_equal(e.solve_cholesky_refined(B, max_iter=0),
                                  e.solve_cholesky(B))
            X, info = e.solve_cholesky_refined(B, return_info=True)
            bnp = _berr_host(A, np.linalg.solve(A, B), B)
            print(f"chol {N},{v},{Px}x{Py}x{Pz} nrhs={nrhs}: "
                  f"berr={info['berr'].max():.3g} numpy={bnp.min():.3g} "
                  f"iters={info['iters']}")
            assert (info["berr"] <= bnp).all()
        assert np.array_equal(F0, e.get_F_global()), "refinement wrote Fres"


# ---------------- guards ----------------------------------------------------

def test_refine_guards(eng):
    lib = eng.lib()
    N, v = 64, 8
    B = np.ones((N, 2))
    ms = ctypes.c_double()
    it = ctypes.c_int()
    be = np.zeros(2)
    lu, ch = lib.conflux_lu_solve_refined, lib.conflux_chol_solve_refined
    with eng.Engine(N, v, 1, 1, 1, rank=-1) as e:
        e.set_matrix_global(gen_matrix(N))
        # before any factorization
        assert lu(e._h, _p(B), 2, 3, _p(be), None, ctypes.byref(it),
                  ctypes.byref(ms)) == EARG
        assert ch(e._h, _p(B), 2, 3, None, None, None, None) == EARG
        # last factorization ran with store_factors off
        e.store_factors(False)
        e.factor()
        assert lu(e._h, _p(B), 2, 3, None, None, None, None) == EARG
        e.store_factors(True)
        e.factor()
        assert lu(e._h, _p(B), 0, 3, None, None, None, None) == EARG
        assert lu(e._h, _p(B), -1, 3, None, None, None, None) == EARG
        assert lu(e._h, None, 2, 3, None, None, None, None) == EARG
        assert lu(e._h, _p(B), 2, -1, None, None, None, None) == EARG
        # kind mismatch
        assert ch(e._h, _p(B), 2, 3, None, None, None, None) == EARG
        with pytest.raises(eng.ConfluxLuError):
            e.solve_cholesky_refined(B)
        with pytest.raises(eng.ConfluxLuError):
            e.solve_refined(B, max_iter=-1)
        # the guards left B alone and the engine usable; every out pointer
        # may be NULL
        assert np.array_equal(B, np.ones((N, 2)))
        assert lu(e._h, _p(B.copy()), 2, 3, None, None, None, None) == 0
        assert lu(e._h, _p(B.copy()), 2, 0, _p(be), None, ctypes.byref(it),
                  None) == 0
        assert it.value == 0 and np.isfinite(be).all() and (be >= 0).all()
        # a store_factors-off run invalidates the earlier factors
        e.store_factors(False)
        e.factor()
        assert lu(e._h, _p(B), 2, 3, None, None, None, None) == EARG
    with eng.Engine(N, v, 1, 1, 1, rank=-1) as e:
        e.store_factors(True)
        e.set_matrix_global(_spd(N))
        e.factor_cholesky()
        assert lu(e._h, _p(B), 2, 3, None, None, None, None) == EARG
        assert ch(e._h, None, 2, 3, None, None, None, None) == EARG
        assert ch(e._h, _p(B), 0, 3, None, None, None, None) == EARG
        assert ch(e._h, _p(B), 2, -1, None, None, None, None) == EARG
        assert ch(e._h, _p(B.copy()), 2, 3, None, None, None, None) == 0
