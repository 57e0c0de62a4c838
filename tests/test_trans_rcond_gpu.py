"""GPU tests of the transposed LU solve (conflux_lu_solve_trans) and the
condition estimates (conflux_lu_rcond / conflux_chol_rcond): the two new
device paths against scipy/numpy, the end-to-end A^T X = B solves against
numpy.linalg.solve by normwise backward error, rcond against the exact
||A|| ||A^-1|| from numpy.linalg.inv.

All tests run on ONE MI355X; multi-rank grids use the engine's
single-process simulation mode (rank=-1).  The world = 2 guard runs two
real ranks through the shimccl mock transport (tests/shimccl.cpp).
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import gen_matrix  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SHIM = os.path.join(HERE, "shimccl.so")
EARG = -1


@pytest.fixture(scope="module")
def eng():
    import conflux_amd
    return conflux_amd


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


# ---------------- kernel: transposed triangular solve -----------------------

TRSM_V = [8, 32, 48, 64, 96]   # ragged single block, exactly one block,
                               # ragged tail, one update, both LDS buffers
TRSM_N = [1, 127, 129]


@pytest.mark.parametrize("v", TRSM_V)
@pytest.mark.parametrize("unit", [0, 1])
@pytest.mark.parametrize("upper", [0, 1])
def test_trsm_left_tri_trans(eng, upper, unit, v):
    """k_trsm_left_tri_mfma<.., TRANS> vs scipy.linalg.solve_triangular with
    trans='T', max abs error < 1e-12: the construction and the bar of
    test_trsm_left_tri (the scaled triangle, so unit and non-unit pose
    equally conditioned systems).  The half of T the solve must not read,
    the diagonal when unit, and the ldt padding columns hold NaN."""
    import scipy.linalg as la
    rng = np.random.default_rng(100 * v + 2 * upper + unit + 50000)
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
        ref = la.solve_triangular(T, X, lower=not upper, trans="T",
                                  unit_diagonal=bool(unit))
        for ldt in (v, v + 24):
            Td = np.full((v, ldt), np.nan)
            Td[:, :v] = np.where(keep, T, np.nan)
            if unit:  # in F the unit triangle's diagonal holds U
                np.fill_diagonal(Td, np.nan)
            X1 = X.copy()
            rc = eng.lib().conflux_lu_debug_trsm_left_trans(
                upper, unit, v, N, ldt, _p(Td), _p(X1))
            assert rc == 0
            assert np.isfinite(X1).all(), \
                f"NaN leaked from the unused half: N={N} ldt={ldt}"
            err = np.abs(X1 - ref).max()
            print(f"trsm^T upper={upper} unit={unit} v={v} N={N} ldt={ldt}: "
                  f"err={err:.3g} max|X|={np.abs(ref).max():.3g}")
            worst = max(worst, err)
    assert worst < 1e-12, f"upper={upper} unit={unit} v={v}: err={worst}"


# ---------------- kernel: transposed skinny update --------------------------

@pytest.mark.parametrize("K", [8, 32, 48, 128])
@pytest.mark.parametrize("nrhs", [1, 3, 16])
def test_update_skinny_t(eng, nrhs, K):
    """k_update_skinny_t vs numpy C - A.T @ B, relative max error < 1e-13
    (the bar of test_update_skinny).  A is stored K x M; lda > M pads its
    rows with NaN: the kernel must not read past column M."""
    rng = np.random.default_rng(1000 * K + nrhs + 7)
    for M in (1, 15, 17, 300):
        A = rng.standard_normal((K, M))
        B = rng.standard_normal((K, nrhs))
        C = rng.standard_normal((M, nrhs))
        ref = C - A.T @ B
        for lda in (M, M + 40):
            Ad = np.full((K, lda), np.nan)
            Ad[:, :M] = A
            C1 = C.copy()
            rc = eng.lib().conflux_lu_debug_update_skinny_t(
                M, nrhs, K, lda, _p(Ad), _p(B), _p(C1))
            assert rc == 0
            err = np.abs(C1 - ref).max() / (np.abs(ref).max() + 1)
            assert err < 1e-13, \
                f"skinny_t M={M} nrhs={nrhs} K={K} lda={lda}: err={err}"


@pytest.mark.parametrize("nrhs", [3, 16])
def test_update_skinny_t_transpose_detecting(eng, nrhs):
    # asymmetric A and B catch a missing transpose, a row/col swap in the
    # MFMA C layout or a k-permutation that A and B disagree on
    M, K = 64, 80
    A = np.arange(K * M, dtype=np.float64).reshape(K, M) / 100
    B = (np.arange(K * nrhs, dtype=np.float64).reshape(K, nrhs) ** 1.5) / 1000
    C1 = np.zeros((M, nrhs))
    assert eng.lib().conflux_lu_debug_update_skinny_t(
        M, nrhs, K, M, _p(A), _p(B), _p(C1)) == 0
    assert np.allclose(C1, -A.T @ B, atol=1e-10)


def test_update_skinny_t_rejects_wide(eng):
    a = np.zeros((16, 16))
    b = np.zeros((16, 17))
    c = np.zeros((16, 17))
    assert eng.lib().conflux_lu_debug_update_skinny_t(
        16, 17, 16, 16, _p(a), _p(b), _p(c)) == EARG


# ---------------- end-to-end: A^T X = B --------------------------------------

def _eta(A, X, B):
    """Normwise backward error ||B - A X||_F / (||A||_F ||X||_F + ||B||_F);
    independent of cond(A)."""
    return np.linalg.norm(B - A @ X) / (
        np.linalg.norm(A) * np.linalg.norm(X) + np.linalg.norm(B))


def _check_eta_t(A, X, B, tag, symmetric=False):
    """X must solve A^T X = B as well as numpy does (10x its backward
    error) — and, on a non-symmetric A, must NOT solve A X = B."""
    eta = _eta(A.T, X, B)
    eta_np = _eta(A.T, np.linalg.solve(A.T, B), B)
    print(f"{tag}: eta={eta:.3g} eta_numpy={eta_np:.3g} "
          f"ratio={eta / eta_np:.2f}")
    assert eta <= 10 * eta_np, f"{tag}: eta={eta} vs numpy {eta_np}"
    if not symmetric:
        wrong = _eta(A, X, B)
        assert wrong > 1e-3, f"{tag}: solved the untransposed system ({wrong})"


def _spd(N):
    G = gen_matrix(N)
    return 0.5 * (G + G.T) + 2.0 * N * np.eye(N)


def _prescribed(rng, n, lo):
    """Singular values logspace(0, lo) between random orthogonal factors."""
    Q1, _ = np.linalg.qr(rng.standard_normal((n, n)))
    Q2, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return (Q1 * np.logspace(0, lo, n)) @ Q2.T


NRHS = [1, 3, 17, 40]   # single, skinny, just past one 16-column group,
                        # three groups with a ragged last one

LU_GRIDS = [
    (64, 8, 1, 1, 1),
    (128, 16, 1, 1, 2),
    (256, 32, 2, 2, 1),
    (512, 256, 1, 1, 1),   # sweep blocks of 128 inside a 256 tile
]


@pytest.mark.parametrize("N,v,Px,Py,Pz", LU_GRIDS)
def test_lu_solve_transposed(eng, N, v, Px, Py, Pz):
    A = gen_matrix(N)
    rng = np.random.default_rng(N + v + 3)
    with eng.Engine(N, v, Px, Py, Pz, rank=-1) as e:
        e.store_factors(True)
        e.set_matrix_global(A)
        e.factor()
        for nrhs in NRHS:
            B = rng.standard_normal((N, nrhs))
            X = e.solve_transposed(B)
            assert X.shape == B.shape
            _check_eta_t(A, X, B,
                         f"lu^T {N},{v},{Px}x{Py}x{Pz} nrhs={nrhs}")


def test_lu_solve_transposed_real_single_rank(eng):
    """rank=0, world=1 (not the simulation): Fres is read in place."""
    N, v = 256, 32
    A = gen_matrix(N)
    rng = np.random.default_rng(15)
    with eng.Engine(N, v, 1, 1, 1, rank=0, world=1) as e:
        e.store_factors(True)
        e.set_matrix_local(A)
        e.factor()
        F0 = e.get_F_local().copy()
        for nrhs in NRHS:
            B = rng.standard_normal((N, nrhs))
            _check_eta_t(A, e.solve_transposed(B), B,
                         f"lu^T real 256,32 nrhs={nrhs}")
        assert np.array_equal(F0, e.get_F_local()), "solve wrote into Fres"


def test_lu_solve_transposed_padded(eng):
    """N = 250 rounds up to 256: B carries Npad rows and A is extended with
    the same nonsingular random fill."""
    with eng.Engine(250, 32, 1, 1, 1, rank=-1) as e:
        assert e.Npad == 256
        A = gen_matrix(e.Npad)
        rng = np.random.default_rng(17)
        e.store_factors(True)
        e.set_matrix_global(A)
        e.factor()
        for nrhs in NRHS:
            B = rng.standard_normal((e.Npad, nrhs))
            _check_eta_t(A, e.solve_transposed(B), B,
                         f"lu^T padded 250->256 nrhs={nrhs}")
        with pytest.raises(ValueError):
            e.solve_transposed(np.ones((250, 3)))


def test_lu_solve_transposed_nopivot(eng):
    N, v = 256, 64
    S = _spd(N)  # == init_matrix_spd fill; symmetric
    rng = np.random.default_rng(18)
    with eng.Engine(N, v, 2, 2, 1, rank=-1) as e:
        e.store_factors(True)
        e.set_pivoting(0)
        e.set_matrix_global(S)
        e.factor()
        for nrhs in NRHS:
            B = rng.standard_normal((N, nrhs))
            _check_eta_t(S, e.solve_transposed(B), B,
                         f"lu^T nopiv nrhs={nrhs}", symmetric=True)


def test_lu_solve_transposed_conventions(eng):
    """1-D round trip, argument untouched, two calls bitwise equal, factors
    not mutated, the plain solve undisturbed."""
    N, v = 256, 32
    A = gen_matrix(N)
    rng = np.random.default_rng(16)
    with eng.Engine(N, v, 2, 2, 1, rank=-1) as e:
        e.store_factors(True)
        e.set_matrix_global(A)
        e.factor()
        F0 = e.get_F_global().copy()
        B = rng.standard_normal((N, 17))
        B0 = B.copy()
        Xplain0 = e.solve(B)
        b = rng.standard_normal(N)
        b0 = b.copy()
        x = e.solve_transposed(b)
        assert x.shape == (N,) and x is not b
        assert np.array_equal(b, b0), "caller's B was modified"
        _check_eta_t(A, x, b, "lu^T 1-D")
        x2d = e.solve_transposed(b.reshape(N, 1))
        assert x2d.shape == (N, 1)
        assert np.array_equal(x2d[:, 0], x)
        X1 = e.solve_transposed(B)
        X2, ms = e.solve_transposed(B, return_ms=True)
        assert np.array_equal(B, B0)
        assert np.array_equal(X1, X2), "second transposed solve differs"
        assert ms > 0
        assert np.array_equal(F0, e.get_F_global()), "solve wrote into Fres"
        assert np.array_equal(Xplain0, e.solve(B)), \
            "plain solve changed after a transposed one"


# ---------------- rcond -------------------------------------------------------

def _check_rcond(A, which, rc, info, tag):
    p = 1 if which == "1" else np.inf
    anorm = np.linalg.norm(A, p)
    true = 1.0 / (anorm * np.linalg.norm(np.linalg.inv(A), p))
    ratio = rc / true
    print(f"{tag} norm={which}: rcond={rc:.6g} true={true:.6g} "
          f"ratio={ratio:.6f} nsolves={info['nsolves']} ms={info['ms']:.3g}")
    assert 1 - 1e-3 <= ratio <= 3, (tag, which, ratio)
    assert abs(info["anorm"] - anorm) <= 1e-13 * anorm, (tag, which)
    assert 1 <= info["nsolves"] <= 12
    assert info["ms"] > 0


def _cond1e6():
    return _prescribed(np.random.default_rng(7256), 256, -6)


@pytest.mark.parametrize("name,Px", [("gen", 1), ("gen", 2), ("cond1e6", 1)])
def test_lu_rcond(eng, name, Px):
    N, v = 256, 32
    A = gen_matrix(N) if name == "gen" else _cond1e6()
    with eng.Engine(N, v, Px, Px, 1, rank=-1) as e:
        e.store_factors(True)
        e.set_matrix_global(A)
        e.factor()
        F0 = e.get_F_global().copy()
        x0 = e.solve(np.ones(N))
        for which in ("1", "I"):
            rc, info = e.rcond(which, return_info=True)
            _check_rcond(A, which, rc, info, f"rcond {name} {Px}x{Px}x1")
            rc2, info2 = e.rcond(which, return_info=True)  # cached ||A||
            assert rc2 == rc and info2["anorm"] == info["anorm"] and \
                info2["nsolves"] == info["nsolves"], "two calls differ"
            assert e.rcond(which) == rc
        assert np.array_equal(F0, e.get_F_global()), "rcond wrote into Fres"
        assert np.array_equal(x0, e.solve(np.ones(N)))
        # the optional outputs may be NULL
        r = ctypes.c_double()
        assert eng.lib().conflux_lu_rcond(e._h, 0, ctypes.byref(r), None,
                                          None, None) == 0
        assert r.value == e.rcond("1")


def test_rcond_cholesky_and_nopivot(eng):
    """pocon on the SPD matrix, and gecon after the no-pivot LU of the same
    matrix: the same bar."""
    N, v = 256, 32
    S = _spd(N)
    with eng.Engine(N, v, 2, 2, 1, rank=-1) as e:
        e.store_factors(True)
        e.set_matrix_global(S)
        e.factor_cholesky()
        F0 = e.get_F_global().copy()
        rc, info = e.rcond_cholesky(return_info=True)
        _check_rcond(S, "1", rc, info, "rcond chol")
        rc2, info2 = e.rcond_cholesky(return_info=True)
        assert rc2 == rc and info2["nsolves"] == info["nsolves"]
        assert np.array_equal(F0, e.get_F_global())
    with eng.Engine(N, v, 1, 1, 1, rank=-1) as e:
        e.store_factors(True)
        e.set_pivoting(0)
        e.set_matrix_global(S)
        e.factor()
        for which in ("1", "I"):
            rc, info = e.rcond(which, return_info=True)
            _check_rcond(S, which, rc, info, "rcond nopiv")


# ---------------- guards ------------------------------------------------------

def test_trans_rcond_guards(eng):
    lib = eng.lib()
    N, v = 64, 8
    B = np.ones((N, 2))
    r = ctypes.c_double()

    def all_three(h):
        return (lib.conflux_lu_solve_trans(h, _p(B), 2, None),
                lib.conflux_lu_rcond(h, 0, ctypes.byref(r), None, None, None),
                lib.conflux_chol_rcond(h, ctypes.byref(r), None, None, None))

    with eng.Engine(N, v, 1, 1, 1, rank=-1) as e:
        e.set_matrix_global(gen_matrix(N))
        # before any factorization
        assert all_three(e._h) == (EARG, EARG, EARG)
        # last factorization ran with store_factors off
        e.store_factors(False)
        e.factor()
        assert all_three(e._h) == (EARG, EARG, EARG)
        e.store_factors(True)
        e.factor()
        # after an LU run: rcond_cholesky refuses, bad arguments refuse
        assert lib.conflux_chol_rcond(e._h, ctypes.byref(r), None, None,
                                      None) == EARG
        with pytest.raises(eng.ConfluxLuError):
            e.rcond_cholesky()
        assert lib.conflux_lu_solve_trans(e._h, _p(B), 0, None) == EARG
        assert lib.conflux_lu_solve_trans(e._h, None, 2, None) == EARG
        assert lib.conflux_lu_rcond(e._h, 0, None, None, None, None) == EARG
        assert lib.conflux_lu_rcond(e._h, 2, ctypes.byref(r), None, None,
                                    None) == EARG
        with pytest.raises(ValueError):
            e.rcond(norm="F")
        # the guards left the engine usable
        assert np.array_equal(B, np.ones((N, 2)))
        assert lib.conflux_lu_solve_trans(e._h, _p(B.copy()), 2, None) == 0
        assert e.rcond("I") > 0
    with eng.Engine(N, v, 1, 1, 1, rank=-1) as e:
        e.store_factors(True)
        e.set_matrix_global(_spd(N))
        e.factor_cholesky()
        # after a Cholesky run: the LU entry points refuse
        assert lib.conflux_lu_solve_trans(e._h, _p(B), 2, None) == EARG
        assert lib.conflux_lu_rcond(e._h, 0, ctypes.byref(r), None, None,
                                    None) == EARG
        with pytest.raises(eng.ConfluxLuError):
            e.solve_transposed(B)
        with pytest.raises(eng.ConfluxLuError):
            e.rcond()
        assert e.rcond_cholesky() > 0


def test_trans_rcond_refuse_world_2(tmp_path):
    """Two real ranks (1x1x2 grid, shimccl transport): after a factorization
    all three entry points return EARG on every rank, before any
    communication, and leave B alone."""
    assert os.path.exists(SHIM), "shimccl.so not built (make -C tests)"
    env = dict(os.environ)
    pre = env.get("LD_PRELOAD")
    env["LD_PRELOAD"] = SHIM + (":" + pre if pre else "")
    env["SHIMCCL_DIR"] = str(tmp_path / "box")
    env.pop("HIP_VISIBLE_DEVICES", None)  # both ranks share device 0
    outs = [str(tmp_path / f"rank{r}.txt") for r in range(2)]
    procs = [subprocess.Popen(
        [sys.executable, os.path.join(HERE, "trans_rcond_dist_worker.py"),
         str(r), outs[r]], env=env, stdout=subprocess.PIPE,
        stderr=subprocess.STDOUT, text=True) for r in range(2)]
    logs = []
    try:
        for p in procs:
            o, _ = p.communicate(timeout=120)
            logs.append(o)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, (p, log) in enumerate(zip(procs, logs)):
        assert p.returncode == 0, f"rank {r} failed:\n{log}"
    for r in range(2):
        got = open(outs[r]).read().split()
        assert got == [str(EARG)] * 4 + ["1"], f"rank {r}: {got}"
